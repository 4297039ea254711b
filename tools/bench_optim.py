#!/usr/bin/env python3
"""The optimiser step after the all-gather, three ways, same payloads, same GPU.

Shapes: C4's consumer (8 payloads x 2^26 values, 256 bins = 8-bit codes) and C5's (8 x 2^27, 4 bins =
2-bit codes); Adam and SGD; fp32 and fp64 state.  Per shape, ms per step of
  (a) decode_sum+torch  skml_dense_decode_sum_f32, then the update written in torch ops on the fp32
                        sum (what a user of the library had before the optimiser entries);
  (b) decode_sum+step   skml_dense_decode_sum_f32, then skml_opt_step_f32/_f64 on the fp32 sum;
  (c) fused             skml_dense_decode_sum_step_f32/_f64.
Each timing is a loop of --steps calls between two HIP events on the codec stream, after a warm-up,
in alternating rounds; the spread of a variant's own rounds is the margin a difference has to clear.
Beside each: the bytes the one-pass algorithm has to move (codes + state read and written, and for
(a) and (b) the fp32 sum written and read back) and that over the time as a fraction of 8 TB/s.  The
torch form moves more than its algorithmic bytes; the figure says so by being small.
Every shape runs in a child process under its own timeout; the parent never touches the GPU and
stops at the first step that fails.  Recorded, not gated.

usage: python tools/bench_optim.py [--configs c4,c5] [--steps 5] [--rounds 3] [--out profiles/optim_bench.json]
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

CONFIGS = {"c4": (8, 2**26, 256), "c5": (8, 2**27, 4), "tiny": (8, 2**16 + 5, 256)}
PEAK = 8e12


def _timed(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def algorithmic_bytes(P, n, bits, adam, wide, fused):
    state = (3 if adam else 1) * 2 * (8 if wide else 4) * n
    return P * n * bits // 8 + state + (0 if fused else 2 * 4 * n)


def step(name, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    P, n, bins = CONFIGS[name]
    bits = 8 if bins == 256 else 2
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    nb = lib.skml_dense_payload_bytes(n, bins)
    stride = (nb + 255) // 256 * 256
    allp = sk.alloc_aligned(stride * P, dev)
    for r in range(P):
        g = torch.Generator(device=dev).manual_seed(2 + r)
        q = sk.UniformQuantizer(bins)
        q.quantize(torch.randn(n, device=dev, generator=g) * 1e-3)
        allp[r * stride:r * stride + q.payload.numel()].copy_(q.payload)
        del q
    torch.cuda.synchronize()
    summed = torch.empty(n, dtype=torch.float32, device=dev)
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
            w = torch.randn(n, dtype=dt, device=dev)
            m = torch.zeros(n, dtype=dt, device=dev) if adam else None
            v = torch.zeros(n, dtype=dt, device=dev) if adam else None
            c_m, c_d = math.sqrt(1 - p.beta2_t), 1 - p.beta1_t
            fused_fn = lib.skml_dense_decode_sum_step_f64 if wide else lib.skml_dense_decode_sum_step_f32
            step_fn = lib.skml_opt_step_f64 if wide else lib.skml_opt_step_f32

            def decode_sum():
                ok(lib.skml_dense_decode_sum_f32(ctx, ptr(allp), P, stride, ptr(summed), n, scale))

            def torch_update():
                decode_sum()
                g = summed if not wide else summed.double()
                if adam:
                    m.mul_(p.beta1).add_(g, alpha=1 - p.beta1)
                    v.mul_(p.beta2).addcmul_(g, g, value=1 - p.beta2)
                    w.addcdiv_(m, v.sqrt().add_(p.eps).mul_(c_d), value=-p.lr * c_m)
                else:
                    w.add_(g, alpha=-p.lr)

            def array_step():
                decode_sum()
                ok(step_fn(ctx, ptr(summed), 0, n, 1.0, C.byref(p), ptr(w), ptr(m), ptr(v)))

            def fused():
                ok(fused_fn(ctx, ptr(allp), P, stride, n, scale, C.byref(p), ptr(w), ptr(m), ptr(v)))

            variants = {"decode_sum+torch": torch_update, "decode_sum+step": array_step, "fused": fused}
            spent = 0.0
            while spent < 300.0:  # sustained load past the clock ramp
                for fn in variants.values():
                    spent += _timed(torch, fn, 2) * 2
            ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    ms[k].append(round(_timed(torch, fn, steps), 4))
            best = {k: min(x) for k, x in ms.items()}
            by = {k: algorithmic_bytes(P, n, bits, adam, wide, k == "fused") for k in variants}
            results.append({
                "config": name, "P": P, "n": n, "bins": bins, "code_bits": bits, "kind": "adam" if adam else "sgd",
                "state": "fp64" if wide else "fp32", "steps": steps, "rounds": rounds, "ms_per_step": ms, "best_ms": best,
                "spread": {k: round((max(x) - min(x)) / min(x), 4) for k, x in ms.items()},
                "algorithmic_bytes": by,
                "fraction_of_8TBps": {k: round(by[k] / (best[k] * 1e-3) / PEAK, 4) for k in variants},
                "fused_over_torch": round(best["fused"] / best["decode_sum+torch"], 3),
                "fused_over_step": round(best["fused"] / best["decode_sum+step"], 3),
                "fused_over_step_by_bytes": round(by["fused"] / by["decode_sum+step"], 3)})
            del w, m, v
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 3 or a.rounds < 3:
        ap.error("at least 3 steps per window and 3 alternating rounds")
    if a.child:
        print("RESULT " + json.dumps(step(a.child, a.steps, a.rounds)))
        return 0
    out = {"tool": "tools/bench_optim.py", "data": "uniform-quantizer payloads of N(0,1) * 1e-3 fp32, torch generator",
           "results": []}
    for s in a.configs.split(","):
        if s not in CONFIGS:
            ap.error(f"unknown config {s}")
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", s,
               "--steps", str(a.steps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"step {s} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        out["results"].extend(json.loads(lines[-1][7:]))
        for res in out["results"][-4:]:
            print(f"{s} {res['kind']} {res['state']}: {res['best_ms']}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
