#!/usr/bin/env python3
"""The optimiser step after the all-gather of sparse payloads (SketchGradient blobs), three ways, same
blobs, same GPU (tools/bench_optim_fixed.py is the same comparison for fixed-point payloads).

Shapes: 8 payloads at dim 2^28 with 10 % nnz (the C3 shape) and one small shape (dim 2^22); Adam and
SGD; fp32 and fp64 state.  Per shape, ms per step of
  (a) decode_sum+torch  skml_sparse_decode_sum_f64, then the update written in torch ops on the sum;
  (b) decode_sum+step   skml_sparse_decode_sum_f64, then skml_opt_step_f32/_f64 on the double sum;
  (c) fused             skml_sparse_decode_sum_step_f32/_f64.
Each timing is a loop of --steps calls between two HIP events on the codec stream, after a warm-up
of sustained load past the clock ramp, in alternating rounds (a, b, c, a, b, c, ...); the spread of
a leg's own rounds is the margin a difference has to clear.  The fused leg's keys-only check kernel
is reported on its own (check_ms: the context's events around that launch, SKML_K_SPARSE_CHECK, in a
pass of its own after the rounds).  Beside each leg: the bytes the algorithm has to move after the
restore, which all three share -- restored keys (4 B) and bins (1 B), the state read and written, for
(a) and (b) the double sum written and read back, for (c) the keys once more.
Every shape runs in a child process under its own timeout; the parent never touches the GPU and
stops at the first step that fails.  Recorded, not gated.

usage: python tools/bench_optim_sparse.py [--log2dims 28,22] [--density 0.1] [--steps 3] [--rounds 6]
                                          [--out profiles/optim_sparse_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 8
LEGS = ("decode_sum+torch", "decode_sum+step", "fused")


def _timed(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def algorithmic_bytes(dim, nnz, adam, wide, fused):
    state = (3 if adam else 1) * 2 * (8 if wide else 4) * dim
    return 5 * nnz + state + (4 * nnz if fused else 2 * 8 * dim)


def step(log2dim, density, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    from sketchml_amd.distributed import blob_stride
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    dim = 1 << log2dim
    pls = []
    for r in range(P):
        g = torch.Generator(device=dev).manual_seed(2 + r)
        keys = torch.nonzero(torch.rand(dim, device=dev, generator=g) < density).flatten().to(torch.int32)
        vals = torch.randn(keys.numel(), device=dev, generator=g, dtype=torch.float64) * 1e-3
        pls.append(sk.encode_sparse(keys, vals, 256, 8, 2, 0.3, r, r + 100))
        del keys, vals
    nnz = sum(p.nnz() for p in pls)
    stride = blob_stride([p.export_bytes() for p in pls])
    allb = torch.zeros(stride * P, dtype=torch.uint8, device=dev)
    for i, p in enumerate(pls):
        p.export(allb[i * stride:(i + 1) * stride])
    del pls
    torch.cuda.synchronize()
    summed = torch.empty(dim, dtype=torch.float64, device=dev)
    scale = 1.0 / P

    def ok(st):
        if st:
            raise RuntimeError(_lib.last_error())

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    results = []
    for wide in (False, True):
        dt = torch.float64 if wide else torch.float32
        for adam in (True, False):
            p = _lib.OptParams()
            lib.skml_opt_params_default(C.byref(p))
            p.kind, p.lr = (_lib.SKML_OPT_ADAM if adam else _lib.SKML_OPT_SGD), 1e-3
            w = torch.randn(dim, dtype=dt, device=dev)
            m = torch.zeros(dim, dtype=dt, device=dev) if adam else None
            v = torch.zeros(dim, dtype=dt, device=dev) if adam else None
            c_m, c_d = math.sqrt(1 - p.beta2_t), 1 - p.beta1_t
            fused_fn = lib.skml_sparse_decode_sum_step_f64 if wide else lib.skml_sparse_decode_sum_step_f32
            step_fn = lib.skml_opt_step_f64 if wide else lib.skml_opt_step_f32

            def decode_sum():
                ok(lib.skml_sparse_decode_sum_f64(ctx, ptr(allb), P, stride, dim, scale, ptr(summed)))

            def torch_update():
                decode_sum()
                g = summed if wide else summed.float()
                if adam:
                    m.mul_(p.beta1).add_(g, alpha=1 - p.beta1)
                    v.mul_(p.beta2).addcmul_(g, g, value=1 - p.beta2)
                    w.addcdiv_(m, v.sqrt().add_(p.eps).mul_(c_d), value=-p.lr * c_m)
                else:
                    w.add_(g, alpha=-p.lr)

            def array_step():
                decode_sum()
                ok(step_fn(ctx, ptr(summed), 1, dim, 1.0, C.byref(p), ptr(w), ptr(m), ptr(v)))

            def fused():
                ok(fused_fn(ctx, ptr(allb), P, stride, dim, scale, C.byref(p), ptr(w), ptr(m), ptr(v)))

            variants = dict(zip(LEGS, (torch_update, array_step, fused)))
            spent = 0.0
            while spent < 300.0:  # sustained load past the clock ramp
                for fn in variants.values():
                    spent += _timed(torch, fn, 2) * 2
            ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    ms[k].append(round(_timed(torch, fn, steps), 4))
            lib.skml_ctx_reset_stats(ctx)
            lib.skml_ctx_set_timing(ctx, 1 << _lib.SKML_K_SPARSE_CHECK)
            for _ in range(steps):
                fused()
            lib.skml_ctx_set_timing(ctx, 0)
            n_chk, chk_ms = C.c_int64(), C.c_double()
            ok(lib.skml_ctx_kernel_stats(ctx, _lib.SKML_K_SPARSE_CHECK, C.byref(n_chk), C.byref(chk_ms)))
            best = {k: min(x) for k, x in ms.items()}
            by = {k: algorithmic_bytes(dim, nnz, adam, wide, k == "fused") for k in variants}
            results.append({
                "P": P, "dim": dim, "nnz_total": nnz, "kind": "adam" if adam else "sgd", "state": "fp64" if wide else "fp32",
                "steps": steps, "rounds": rounds, "ms_per_step": ms, "best_ms": best,
                "spread": {k: round((max(x) - min(x)) / min(x), 4) for k, x in ms.items()},
                "check_ms": round(chk_ms.value / max(n_chk.value, 1), 4),
                "algorithmic_bytes": by,
                "GBps": {k: round(by[k] / (best[k] * 1e-3) / 1e9, 1) for k in variants},
                "fused_over_torch": round(best["fused"] / best["decode_sum+torch"], 3),
                "fused_over_step": round(best["fused"] / best["decode_sum+step"], 3),
                "fused_over_step_by_bytes": round(by["fused"] / by["decode_sum+step"], 3)})
            del w, m, v
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2dims", default="28,22")
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 3 or a.rounds < 6:
        ap.error("at least 3 steps per window and 6 alternating rounds")
    if a.child:
        print("RESULT " + json.dumps(step(a.child, a.density, a.steps, a.rounds)))
        return 0
    out = {"tool": "tools/bench_optim_sparse.py",
           "data": f"{P} sparse payloads, keys uniform at density {a.density}, values N(0,1) * 1e-3 fp64, 256 bins, 8 groups",
           "results": []}
    for s in a.log2dims.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", s,
               "--density", str(a.density), "--steps", str(a.steps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"step log2dim={s} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        out["results"].extend(json.loads(lines[-1][7:]))
        for res in out["results"][-4:]:
            print(f"2^{s} {res['kind']} {res['state']}: {res['best_ms']} check {res['check_ms']} spread {res['spread']}",
                  file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
