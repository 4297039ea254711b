#!/usr/bin/env python3
"""The mini-batch gradient over dense instances stored as float32, bfloat16 or float16
(skml_glm_gradient_dense_lowp_*) beside the float64 route (skml_glm_gradient_dense_*), at the two shapes of
tools/bench_glm_dense.py.  The values are drawn once and rounded to float16 (so that all four routes hold
the same values exactly); every narrow route has to give the bits of the float64 route, which is asserted
here at the timed sizes.

The four routes alternate over --rounds in one process; a timed window is at least --steps calls and
--window-ms long, between two host clock reads around device synchronisations, after a warm-up.  A route's
spread is (max - min) / min of its rounds.  Per-kernel times come from skml_ctx_kernel_stats (the context's
own events around its launches) in a pass of their own; the share of the HBM roofline is the bytes of x the
kernel has to read in that route's storage type (batch * dim * sizeof) over its time and the peak.

usage: python tools/bench_glm_dense_lowp.py [--steps 10] [--rounds 5] [--window-ms 300] [--out profiles/glm_dense_lowp_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s, MI355X
SHAPES = {"many_rows": (1 << 17, 512), "few_rows": (2048, 1 << 15)}
LEGS = (("dot_and_loss_sum", "SKML_K_GLM_PREDICT"), ("column_sum", "SKML_K_GLM_PLUS_BY"))
HBM_BOUND = {"many_rows": "dot_and_loss_sum", "few_rows": "column_sum"}  # the leg with enough chains to fill the chip


def timed(torch, fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0, help="a timed window lasts at least this long: more calls for a fast route")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_dense_lowp_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_glm_dense_lowp: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib, dev = _lib.lib, torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    props = torch.cuda.get_device_properties(0)
    loss = sk.L2LogLoss(0.0)
    types = {"float64": None, "float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
    out = {"tool": "tools/bench_glm_dense_lowp.py",
           "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                   "compute_units": props.multi_processor_count, "simds": props.multi_processor_count * 4},
           "hbm_peak_bytes_per_s": HBM_PEAK, "steps": a.steps, "rounds": a.rounds, "min_window_ms": a.window_ms,
           "weight": "float64", "loss": "L2LogLoss(0)", "yardstick": "the float64 route of the same run",
           "kernel_constants": {"float64": {k: _lib.glm_dense_constant(k) for k in _lib.GLM_DENSE_CONSTANTS},
                                **{n: {k: _lib.glm_dense_lowp_constant(_lib.X_KINDS[t], k) for k in _lib.GLM_DENSE_CONSTANTS}
                                   for n, t in types.items() if t is not None}},
           "kernel_times_from": "skml_ctx_kernel_stats (the context's own events around its launches)", "shapes": {}}
    for name in a.shapes.split(","):
        rows, dim = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        x16 = torch.randn(rows, dim, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16).to(torch.float16)
        assert bool(torch.isfinite(x16).all()) and torch.equal(x16.to(torch.bfloat16).to(torch.float16), x16)  # exact in all four types
        label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
        w = torch.randn(dim, dtype=torch.float64, device=dev, generator=g) * 1e-2
        routes = {n: sk.DenseDataSet.fromArray(x16.to(t if t is not None else torch.float64), label, dim, device=dev, xDtype=t)
                  for n, t in types.items()}
        del x16
        last = {}

        def run(k):
            last[k] = optim.batch_gradient(w, routes[k], 0, rows, loss, want_pre=True)

        steps = {}
        for k in routes:
            timed(torch, lambda: run(k), 2)
            steps[k] = max(a.steps, int(a.window_ms / timed(torch, lambda: run(k), 2)) + 1)
        same = {k: all(torch.equal(last[k][f].view(torch.int64), last["float64"][f].view(torch.int64)) for f in ("pre", "coef", "loss", "grad"))
                and last[k]["nnz"] == last["float64"]["nnz"] and last[k]["objLoss"] == last["float64"]["objLoss"] for k in routes}
        assert all(same.values()), f"{name}: a narrow route's bits differ from the float64 route's: {same}"
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k in routes:
                ms[k].append(round(timed(torch, lambda: run(k), steps[k]), 4))
        best = {k: min(v) for k, v in ms.items()}
        spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()}
        kern = {k: {leg: [] for leg, _ in LEGS} for k in routes}
        for _ in range(a.rounds):  # per-kernel times: the routes alternate here too
            for k in routes:
                lib.skml_ctx_set_timing(ctx, -1)
                lib.skml_ctx_reset_stats(ctx)
                for _ in range(a.steps):
                    run(k)
                torch.cuda.synchronize()
                for leg, kid in LEGS:
                    cnt, tot = C.c_int64(), C.c_double()
                    lib.skml_ctx_kernel_stats(ctx, getattr(_lib, kid), C.byref(cnt), C.byref(tot))
                    kern[k][leg].append(round(tot.value / a.steps, 4))
                lib.skml_ctx_set_timing(ctx, 0)
        res = {}
        for k, ds in routes.items():
            nbytes = rows * ds.pitch * ds.x.element_size()
            res[k] = {"bytes_of_x": nbytes, "calls_per_window": steps[k], "call_ms": ms[k], "call_best_ms": best[k], "call_spread": spread[k],
                      "call_ratio_float64_over_this": round(best["float64"] / best[k], 3)}
            for leg, _ in LEGS:
                v, ref = kern[k][leg], kern["float64"][leg]
                sp, sp_ref = (max(v) - min(v)) / min(v), (max(ref) - min(ref)) / min(ref)
                ratio = min(ref) / min(v)
                res[k][leg] = {"ms": v, "best_ms": min(v), "spread": round(sp, 4), "share_of_hbm_roofline": round(nbytes / (min(v) * 1e-3) / HBM_PEAK, 4),
                               "ratio_float64_over_this": round(ratio, 3), "faster_than_float64_by_more_than_both_spreads": bool(ratio - 1.0 > sp + sp_ref),
                               "slower_than_float64_beyond_the_spread": bool(1.0 / ratio - 1.0 > sp + sp_ref)}
        out["shapes"][name] = {"rows": rows, "dim": dim, "batch": rows, "hbm_bound_leg": HBM_BOUND[name], "same_bits_as_float64": same,
                               "waves": {"row_dot": (rows + 63) // 64, "column_sum": {k: -(-dim // (64 * (out["kernel_constants"][k]["V"]))) for k in routes}},
                               "routes": res}
        del routes, last
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
