#!/usr/bin/env python3
"""The mini-batch gradient over dense instances (skml_glm_gradient_dense_*) beside the route it replaces:
the same rows as a DataSet.fromCSR that stores every column (skml_glm_gradient_*).  Both give the same
bits (checked here at the timed sizes), so only the time differs.

Two shapes (seeded, generated on the device), the batch being the whole set, weights float64, L2LogLoss:
  many_rows   rows >= 64 x the chip's SIMD count, a moderate dim: every SIMD can hold a wave of the row dot,
              but the column sum has only dim / 64 waves
  few_rows    few rows, a large dim: the row dot has only rows / 64 waves
The contract (one chain of rounded adds per row and per column) leaves no other parallelism; the
JSON states both limits with the numbers.

Each timed window is a loop of at least --steps calls, and as many as fill --window-ms, between two host
clock reads around device synchronisations, after a warm-up; the two routes alternate over --rounds in
one process, and each route's own spread (max - min) / min is the margin a difference has to clear.
Per-kernel times come from skml_ctx_kernel_stats (the context's own events around its launches, not a
profiler) in a pass of their own; the share of the HBM roofline is the bytes the kernel has to read
by the algorithm (batch * dim * 8 dense, * 12 with the int32 index of the CSR) over its time and the
peak.  Nothing is gated: the tool writes down what it measured and on which box.

usage: python tools/bench_glm_dense.py [--steps 10] [--rounds 5] [--window-ms 300] [--out profiles/glm_dense_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_dense_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_glm_dense: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib, dev = _lib.lib, torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    props = torch.cuda.get_device_properties(0)
    simds = props.multi_processor_count * 4
    loss = sk.L2LogLoss(0.0)
    out = {"tool": "tools/bench_glm_dense.py", "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip,
                                                        "torch": torch.__version__, "compute_units": props.multi_processor_count, "simds": simds},
           "hbm_peak_bytes_per_s": HBM_PEAK, "steps": a.steps, "rounds": a.rounds, "weight": "float64", "loss": "L2LogLoss(0)",
           "kernel_constants": {k: _lib.glm_dense_constant(k) for k in _lib.GLM_DENSE_CONSTANTS},
           "min_window_ms": a.window_ms, "kernel_times_from": "skml_ctx_kernel_stats (the context's own events around its launches)",
           "shapes": {}}
    for name in a.shapes.split(","):
        rows, dim = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(rows, dim, dtype=torch.float64, device=dev, generator=g)
        label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
        w = torch.randn(dim, dtype=torch.float64, device=dev, generator=g) * 1e-2
        dense = sk.DenseDataSet.fromArray(x, label, dim, device=dev)
        col = torch.arange(dim, dtype=torch.int32, device=dev).repeat(rows)
        csr = sk.DataSet.fromCSR(torch.arange(rows + 1, dtype=torch.int64, device=dev) * dim, col, x.view(-1), label, dim, device=dev)
        csr.glm_data()
        del col
        routes = {"dense": dense, "full_csr": csr}
        last = {}

        def run(k):
            last[k] = optim.batch_gradient(w, routes[k], 0, rows, loss, want_pre=True)

        steps = {}
        for k in routes:
            timed(torch, lambda: run(k), 2)
            steps[k] = max(a.steps, int(a.window_ms / timed(torch, lambda: run(k), 2)) + 1)
        same = all(torch.equal(last["dense"][f].view(torch.int64), last["full_csr"][f].view(torch.int64)) for f in ("pre", "coef", "loss", "grad"))
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k in routes:
                ms[k].append(round(timed(torch, lambda: run(k), steps[k]), 4))
        kern = {}
        for k, per_elem in (("dense", 8), ("full_csr", 12)):
            lib.skml_ctx_set_timing(ctx, -1)
            lib.skml_ctx_reset_stats(ctx)
            for _ in range(a.steps):
                run(k)
            torch.cuda.synchronize()
            kern[k] = {}
            for kname, kid in (("predict_and_loss_sum", _lib.SKML_K_GLM_PREDICT), ("plus_by", _lib.SKML_K_GLM_PLUS_BY)):
                cnt, tot = C.c_int64(), C.c_double()
                lib.skml_ctx_kernel_stats(ctx, kid, C.byref(cnt), C.byref(tot))
                per_call, nbytes = tot.value / a.steps, rows * dim * per_elem
                kern[k][kname] = {"ms_per_call": round(per_call, 4), "algorithmic_bytes": nbytes,
                                  "share_of_hbm_roofline": round(nbytes / (per_call * 1e-3) / HBM_PEAK, 4) if per_call else None}
            lib.skml_ctx_set_timing(ctx, 0)
        best = {k: min(v) for k, v in ms.items()}
        spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()}
        ratio = best["full_csr"] / best["dense"]
        out["shapes"][name] = {
            "rows": rows, "dim": dim, "batch": rows, "bytes_held": {"dense": rows * dim * 8, "full_csr": rows * dim * 24},
            "parallelism": {"row_dot_waves": (rows + 63) // 64, "column_sum_waves": (dim + 63) // 64, "column_sum_lanes": dim,
                            "simds": simds,
                            "note": "a wave of the row dot owns 64 rows, a lane of the column sum one column; with fewer waves "
                                    "than SIMDs the rest of the chip idles, and the bytes in flight are waves x 8 KiB (row dot) "
                                    "or waves x 16 KiB (column sum)"},
            "same_bits": bool(same), "calls_per_window": steps, "ms_per_call": ms, "best_ms": best, "spread": spread,
            "ratio_full_csr_over_dense": round(ratio, 3),
            "dense_faster_by_more_than_the_spread": bool(ratio - 1.0 > max(spread.values())),
            "kernels": kern}
        del dense, csr, routes, last, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0 if all(s["same_bits"] for s in out["shapes"].values()) else 2


if __name__ == "__main__":
    sys.exit(main())
