#!/usr/bin/env python3
"""The dense mini-batch gradient in the blocked summation order (skml_glm_gradient_dense_*blocked_*) beside the
sequential entries, at the two shapes of tools/bench_glm_dense.py and the four storages of x.  The values are
drawn once and rounded to float16, so that all storages hold the same values exactly.

The eight routes (storage x order) alternate over --rounds in one process after a warm-up of every route; a
timed window is at least --steps calls and --window-ms long, between two host clock reads around device
synchronisations.  A route's spread is (max - min) / min of its rounds.  Per-kernel times come from
skml_ctx_kernel_stats in a pass of their own.  A leg's share of the HBM roofline is that route's own bytes of x
(the blocked column sum's: plus its partial sums, written and read once) over the leg's time and the peak.  The
yardstick is the sequential route of the same storage in the same run.  Recorded too: the plan of every blocked
route, and the largest |blocked - sequential| as a share of gamma_n * sum |terms| (the bound each order keeps
against the exact sum, n = dim for pre and batch for grad; grad's terms with the sequential route's coef).

usage: python tools/bench_glm_dense_blocked.py [--steps 10] [--rounds 5] [--window-ms 300] [--out profiles/glm_dense_blocked_bench.json]
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
PLAN = ("lanes_per_row", "waves_per_row", "rows_in_flight_per_wave", "RB", "NB", "partial_bytes")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_dense_blocked_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_glm_dense_blocked: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib, dev = _lib.lib, torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    props = torch.cuda.get_device_properties(0)
    loss = sk.L2LogLoss(0.0)
    types = {"float64": None, "float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
    out = {"tool": "tools/bench_glm_dense_blocked.py",
           "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                   "compute_units": props.multi_processor_count, "simds": props.multi_processor_count * 4},
           "hbm_peak_bytes_per_s": HBM_PEAK, "steps": a.steps, "rounds": a.rounds, "min_window_ms": a.window_ms,
           "weight": "float64", "loss": "L2LogLoss(0)", "yardstick": "the sequential route of the same storage in the same run",
           "kernel_times_from": "skml_ctx_kernel_stats (the context's own events around its launches)", "shapes": {}}
    for name in a.shapes.split(","):
        rows, dim = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        x16 = torch.randn(rows, dim, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16).to(torch.float16)
        label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
        w = torch.randn(dim, dtype=torch.float64, device=dev, generator=g) * 1e-2
        data = {n: sk.DenseDataSet.fromArray(x16.to(t if t is not None else torch.float64), label, dim, device=dev, xDtype=t)
                for n, t in types.items()}
        ax = x16.double().abs()
        del x16
        routes = [(n, o) for n in types for o in optim.ORDERS]
        last = {}

        def run(k):
            last[k] = optim.batch_gradient(w, data[k[0]], 0, rows, loss, want_pre=True, order=k[1])

        steps = {}
        for k in routes:  # the warm-up of every route, and the calls its window needs
            timed(torch, lambda: run(k), 2)
            steps[k] = max(a.steps, int(a.window_ms / timed(torch, lambda: run(k), 2)) + 1)
        u, off = 2.0 ** -53, {}
        for n in types:
            b, s = last[(n, "blocked")], last[(n, "sequential")]
            gd, gb = dim * u / (1 - dim * u), rows * u / (1 - rows * u)
            off[n] = {"pre": float(((b["pre"] - s["pre"]).abs() / (gd * (ax @ w.abs()))).max()),
                      "grad": float(((b["grad"] - s["grad"]).abs() / (gb * (ax.T @ s["coef"].abs()))).max())}
        del ax
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k in routes:
                ms[k].append(round(timed(torch, lambda: run(k), steps[k]), 4))
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
        for n, ds in data.items():
            xbytes = rows * ds.pitch * ds.x.element_size()
            plan = dict(zip(PLAN, _lib.glm_dense_blocked_plan(ds.x.element_size(), rows, dim)))
            res[n] = {"bytes_of_x": xbytes, "plan": plan, "blocked_minus_sequential_over_the_bound": off[n]}
            for o in optim.ORDERS:
                k, ref = (n, o), (n, "sequential")
                r = {"calls_per_window": steps[k], "call_ms": ms[k], "call_best_ms": min(ms[k]),
                     "call_spread": round((max(ms[k]) - min(ms[k])) / min(ms[k]), 4), "call_ratio_sequential_over_this": round(min(ms[ref]) / min(ms[k]), 3)}
                for leg, _ in LEGS:
                    v, rv = kern[k][leg], kern[ref][leg]
                    sp, sp_ref, ratio = (max(v) - min(v)) / min(v), (max(rv) - min(rv)) / min(rv), min(rv) / min(v)
                    nbytes = xbytes + (2 * plan["partial_bytes"] if o == "blocked" and leg == "column_sum" else 0)
                    r[leg] = {"ms": v, "best_ms": min(v), "spread": round(sp, 4), "bytes": nbytes,
                              "share_of_hbm_roofline": round(nbytes / (min(v) * 1e-3) / HBM_PEAK, 4), "ratio_sequential_over_this": round(ratio, 3),
                              "faster_than_sequential_by_more_than_both_spreads": bool(ratio - 1.0 > sp + sp_ref),
                              "slower_than_sequential_beyond_the_spread": bool(1.0 / ratio - 1.0 > sp + sp_ref)}
                res[n][o] = r
        out["shapes"][name] = {"rows": rows, "dim": dim, "batch": rows, "storages": res}
        del data, last
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
