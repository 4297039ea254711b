#!/usr/bin/env python3
"""The optimiser step after the all-gather of FixedPointGradient payloads, three ways, same payloads,
same GPU (tools/bench_optim.py is the same comparison for dense payloads).

Shapes: 8 payloads x 2^26 codes at 8 and at 4 bits; Adam and SGD; fp32 and fp64 state.  Per shape,
ms per step of
  (a) decode_sum+torch  skml_fixed_decode_sum_f32, then the update written in torch ops on the fp32 sum;
  (b) decode_sum+step   skml_fixed_decode_sum_f32, then skml_opt_step_f32/_f64 on the fp32 sum;
  (c) fused             skml_fixed_decode_sum_step_f32/_f64 (the only one whose gradient is the double).
Each timing is a loop of --steps calls between two HIP events on the codec stream, after a warm-up
of sustained load past the clock ramp, in alternating rounds (a, b, c, a, b, c, ...); the spread of
a leg's own rounds is the margin a difference has to clear.  Beside each leg: the bytes the
algorithm has to move (codes, state read and written, and for (a) and (b) the fp32 sum written and
read back) and that over the best time in GB/s.  The torch leg moves more than its algorithmic
bytes; its figure says so by being small.
Every width runs in a child process under its own timeout; the parent never touches the GPU and
stops at the first step that fails.  Recorded, not gated.

usage: python tools/bench_optim_fixed.py [--bits 8,4] [--log2n 26] [--steps 5] [--rounds 6]
                                         [--out profiles/optim_fixed_bench.json]
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


def algorithmic_bytes(n, bits, adam, wide, fused):
    state = (3 if adam else 1) * 2 * (8 if wide else 4) * n
    return P * n * bits // 8 + state + (0 if fused else 2 * 4 * n)


def step(bits, n, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    nb = sk.fixed_point.payload_bytes(n, bits)
    stride = nb
    allp = sk.alloc_aligned(stride * P, dev)
    for r in range(P):
        g = torch.Generator(device=dev).manual_seed(2 + r)
        sk.fixed_point.encode(torch.randn(n, device=dev, generator=g) * 1e-3, bits, 5 + r, out=allp[r * stride:(r + 1) * stride])
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
            fused_fn = lib.skml_fixed_decode_sum_step_f64 if wide else lib.skml_fixed_decode_sum_step_f32
            step_fn = lib.skml_opt_step_f64 if wide else lib.skml_opt_step_f32

            def decode_sum():
                ok(lib.skml_fixed_decode_sum_f32(ctx, ptr(allp), P, stride, ptr(summed), n, scale))

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

            variants = dict(zip(LEGS, (torch_update, array_step, fused)))
            spent = 0.0
            while spent < 300.0:  # sustained load past the clock ramp
                for fn in variants.values():
                    spent += _timed(torch, fn, 2) * 2
            ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    ms[k].append(round(_timed(torch, fn, steps), 4))
            best = {k: min(x) for k, x in ms.items()}
            by = {k: algorithmic_bytes(n, bits, adam, wide, k == "fused") for k in variants}
            results.append({
                "P": P, "n": n, "num_bits": bits, "kind": "adam" if adam else "sgd", "state": "fp64" if wide else "fp32",
                "steps": steps, "rounds": rounds, "ms_per_step": ms, "best_ms": best,
                "spread": {k: round((max(x) - min(x)) / min(x), 4) for k, x in ms.items()},
                "algorithmic_bytes": by,
                "GBps": {k: round(by[k] / (best[k] * 1e-3) / 1e9, 1) for k in variants},
                "fused_over_torch": round(best["fused"] / best["decode_sum+torch"], 3),
                "fused_over_step": round(best["fused"] / best["decode_sum+step"], 3),
                "fused_over_step_by_bytes": round(by["fused"] / by["decode_sum+step"], 3)})
            del w, m, v
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="8,4")
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 3 or a.rounds < 6:
        ap.error("at least 3 steps per window and 6 alternating rounds")
    n = 1 << a.log2n
    if a.child:
        print("RESULT " + json.dumps(step(a.child, n, a.steps, a.rounds)))
        return 0
    out = {"tool": "tools/bench_optim_fixed.py",
           "data": "fixed-point payloads (seeds 5 + p) of N(0,1) * 1e-3 fp32, torch generator", "results": []}
    for s in a.bits.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", s,
               "--log2n", str(a.log2n), "--steps", str(a.steps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"step bits={s} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        out["results"].extend(json.loads(lines[-1][7:]))
        for res in out["results"][-4:]:
            print(f"{s} bits {res['kind']} {res['state']}: {res['best_ms']} spread {res['spread']}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
