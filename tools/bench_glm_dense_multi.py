#!/usr/bin/env python3
"""The dense mini-batch gradient of K models per pass (skml_glm_gradient_dense_*multi_*, optim.batch_gradient_multi)
beside the route it replaces, K calls of batch_gradient(order="blocked"), at the two shapes of
tools/bench_glm_dense_blocked.py, the four storages of x and K = 1, 4, 16; fp64 weights, L2LogLoss.  The values are
drawn once and rounded to float16, so that all storages hold the same values exactly.

The routes (storage x K x {blocked_x_K, multi}) alternate over --rounds in one process after a warm-up of every route;
a timed window is at least --steps calls and --window-ms long, between two host clock reads around device
synchronisations.  A route's spread is (max - min) / min of its rounds.  Per-kernel times come from
skml_ctx_kernel_stats in a pass of their own.  A leg's algorithmic bytes are the bytes of x it has to read (K times
for the blocked route) plus the partial sums, written and read once; its share of the HBM roofline is those bytes over
the leg's time and the peak, its FLOP/s are 2 * K * batch * dim over the leg's time.  "faster" is claimed only where
the difference exceeds both spreads.

usage: python tools/bench_glm_dense_multi.py [--steps 10] [--rounds 5] [--window-ms 300] [--out profiles/glm_dense_multi_bench.json]
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
PLAN = ("rows_per_tile", "tiles_per_wave", "waves_per_tile", "columns_per_lane_step", "columns_per_strip", "RB", "NB", "partial_bytes")
MODELS = (1, 4, 16)


def timed(torch, fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def spread(v):
    return (max(v) - min(v)) / min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0, help="a timed window lasts at least this long: more calls for a fast route")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_dense_multi_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_glm_dense_multi: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib, dev = _lib.lib, torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    props = torch.cuda.get_device_properties(0)
    loss = sk.L2LogLoss(0.0)
    types = {"float64": None, "float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
    out = {"tool": "tools/bench_glm_dense_multi.py",
           "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                   "compute_units": props.multi_processor_count, "simds": props.multi_processor_count * 4},
           "hbm_peak_bytes_per_s": HBM_PEAK, "steps": a.steps, "rounds": a.rounds, "min_window_ms": a.window_ms,
           "weight": "float64", "loss": "L2LogLoss(0)", "yardstick": "K calls of batch_gradient(order='blocked') in the same run",
           "kernel_times_from": "skml_ctx_kernel_stats (the context's own events around its launches)", "shapes": {}}
    for name in a.shapes.split(","):
        rows, dim = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        x16 = torch.randn(rows, dim, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16).to(torch.float16)
        label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
        ws = torch.randn(max(MODELS), dim, dtype=torch.float64, device=dev, generator=g) * 1e-2
        labels = torch.where(torch.rand(max(MODELS), rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
        data = {n: sk.DenseDataSet.fromArray(x16.to(t if t is not None else torch.float64), label, dim, device=dev, xDtype=t)
                for n, t in types.items()}
        del x16
        routes = [(n, k, r) for n in types for k in MODELS for r in ("blocked_x_K", "multi")]

        def run(key):
            n, k, route = key
            if route == "multi":
                optim.batch_gradient_multi(ws[:k], data[n], 0, rows, loss, labels=labels[:k])
            else:  # the labels are the data set's here: the blocked entries read one label vector, the times do not depend on it
                for m in range(k):
                    optim.batch_gradient(ws[m], data[n], 0, rows, loss, order="blocked")

        steps = {}
        for key in routes:  # the warm-up of every route, and the calls its window needs
            timed(torch, lambda: run(key), 2)
            steps[key] = max(a.steps, int(a.window_ms / timed(torch, lambda: run(key), 2)) + 1)
        ms = {key: [] for key in routes}
        for _ in range(a.rounds):
            for key in routes:
                ms[key].append(round(timed(torch, lambda: run(key), steps[key]), 4))
        kern = {key: {leg: [] for leg, _ in LEGS} for key in routes}
        for _ in range(a.rounds):  # per-kernel times: the routes alternate here too
            for key in routes:
                lib.skml_ctx_set_timing(ctx, -1)
                lib.skml_ctx_reset_stats(ctx)
                for _ in range(a.steps):
                    run(key)
                torch.cuda.synchronize()
                for leg, kid in LEGS:
                    cnt, tot = C.c_int64(), C.c_double()
                    lib.skml_ctx_kernel_stats(ctx, getattr(_lib, kid), C.byref(cnt), C.byref(tot))
                    kern[key][leg].append(round(tot.value / a.steps, 4))
                lib.skml_ctx_set_timing(ctx, 0)
        res = {}
        for n, ds in data.items():
            xb = ds.x.element_size()
            xbytes = rows * ds.pitch * xb
            res[n] = {"bytes_of_x": xbytes}
            for k in MODELS:
                plans = {"multi": dict(zip(PLAN, _lib.glm_dense_multi_plan(xb, k, rows, dim))),
                         "blocked_x_K": {"partial_bytes": _lib.glm_dense_blocked_plan(xb, rows, dim)[5]}}
                entry = {}
                for route in ("blocked_x_K", "multi"):
                    key, ref = (n, k, route), (n, k, "blocked_x_K")
                    passes = k if route == "blocked_x_K" else 1
                    r = {"plan": plans[route], "calls_per_window": steps[key], "call_ms": ms[key], "call_best_ms": min(ms[key]),
                         "call_spread": round(spread(ms[key]), 4), "call_ratio_blocked_over_this": round(min(ms[ref]) / min(ms[key]), 3),
                         "call_faster_than_blocked_by_more_than_both_spreads": bool(min(ms[ref]) / min(ms[key]) - 1.0 > spread(ms[key]) + spread(ms[ref])),
                         "call_slower_than_blocked_beyond_both_spreads": bool(min(ms[key]) / min(ms[ref]) - 1.0 > spread(ms[key]) + spread(ms[ref]))}
                    for leg, _ in LEGS:
                        v, rv = kern[key][leg], kern[ref][leg]
                        nbytes = passes * (xbytes + (2 * plans[route]["partial_bytes"] if leg == "column_sum" else 0))
                        r[leg] = {"ms": v, "best_ms": min(v), "spread": round(spread(v), 4), "algorithmic_bytes": nbytes,
                                  "share_of_hbm_roofline": round(nbytes / (min(v) * 1e-3) / HBM_PEAK, 4),
                                  "fp64_flop_per_s": round(2.0 * k * rows * dim / (min(v) * 1e-3), 0),
                                  "ratio_blocked_over_this": round(min(rv) / min(v), 3),
                                  "faster_than_blocked_by_more_than_both_spreads": bool(min(rv) / min(v) - 1.0 > spread(v) + spread(rv))}
                    entry[route] = r
                res[n]["K=%d" % k] = entry
        out["shapes"][name] = {"rows": rows, "dim": dim, "batch": rows, "storages": res}
        del data
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
