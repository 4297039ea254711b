#!/usr/bin/env python3
"""The sparse mini-batch gradient's column sum in the segmented order beside the sequential one
(optim.batch_gradient(order=...)), on tools/bench_glm.py's data set and on the same one without its bias feature.

Data (seeded, generated on the device): 2^20 instances over 2^26 features, 64 entries per instance: feature 0 and
one feature from each of 63 equal strata of the others ("bias"), or one from each of 64 strata ("no_bias");
values N(0,1), labels +-1, weights N(0,1) * 1e-2, L2LogLoss, the window of batchSpRatio 0.1 from row 0.

The two legs alternate in one process over --rounds; a round is --steps calls between two host clock reads, each
after a device synchronisation (every call synchronises by itself), after a warm-up.  A leg's best round and its
own spread (max - min over min) are reported; a difference counts when it exceeds both legs' spreads.  The
per-kernel times come from skml_ctx_kernel_stats (SKML_K_GLM_PLUS_BY: k_glm_plus_by, or the tile pass, the wide
pass and the slice reduction together) in a pass of their own per leg, with the bytes the column sum has to move
by the algorithm: 16 * dim (col_ptr in, g out) + 20 * window entries (row, value, coefficient).  --other-lib times
the sequential leg once more in a child process that loads another build of the library (tools/build_other_lib.py),
to show that the existing entry is untouched.  Nothing is gated: the tool writes down what it measured.

usage: python tools/bench_glm_segmented.py [--steps 10] [--rounds 3] [--other-lib PATH] [--out profiles/glm_segmented_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from bench_glm import RATIO, ROW_LEN, stats, timed  # noqa: E402

HBM_TBPS = 8.0  # MI355X: the roofline the shares are quoted against


def make_data(torch, sk, rows, dim, dev, bias):
    g = torch.Generator(device=dev).manual_seed(1)
    free = ROW_LEN - 1 if bias else ROW_LEN
    stratum = (dim - 1) // free
    col = torch.empty((rows, ROW_LEN), dtype=torch.int64, device=dev)
    col[:, 0] = 0
    col[:, ROW_LEN - free:] = 1 + torch.arange(free, device=dev) * stratum + torch.randint(0, stratum, (rows, free), device=dev, generator=g)
    val = torch.randn(rows * ROW_LEN, dtype=torch.float64, device=dev, generator=g)
    label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
    ds = sk.DataSet.fromCSR(torch.arange(rows + 1, dtype=torch.int64, device=dev) * ROW_LEN, col.view(-1), val, label, dim, device=dev)
    ds.glm_data()  # validates and builds the column order
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=20)
    ap.add_argument("--dim-log2", type=int, default=26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--sequential-only", action="store_true", help="the child's mode: the bias shape's sequential leg alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_segmented_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_glm_segmented: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib, dev, ctx = _lib.lib, torch.device("cuda", 0), sk.get_context(0).handle
    rows, dim = 1 << a.rows_log2, 1 << a.dim_log2
    batch, loss = int(rows * RATIO), sk.L2LogLoss(0.0)
    w = torch.randn(dim, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 1e-2
    orders = ("sequential",) if a.sequential_only else ("sequential", "segmented")
    shapes = {}
    for name, bias in (("bias", True),) if a.sequential_only else (("bias", True), ("no_bias", False)):
        ds = make_data(torch, sk, rows, dim, dev, bias)
        last = {}
        legs = {o: (lambda o=o: last.__setitem__(o, optim.batch_gradient(w, ds, 0, batch, loss, order=o))) for o in orders}
        for fn in legs.values():
            timed(torch, fn, 3)
        ms = {o: [] for o in orders}
        for _ in range(a.rounds):
            for o, fn in legs.items():
                ms[o].append(round(timed(torch, fn, a.steps), 4))
        nbytes, kern = 16 * dim + 20 * batch * ROW_LEN, {}
        for o, fn in legs.items():  # the column sum alone, a pass of its own per leg
            lib.skml_ctx_set_timing(ctx, -1)
            lib.skml_ctx_reset_stats(ctx)
            timed(torch, fn, a.steps)
            cnt, tot = stats(lib, ctx, _lib.SKML_K_GLM_PLUS_BY)
            lib.skml_ctx_set_timing(ctx, 0)
            per = tot / a.steps
            kern[o] = {"column_sum_ms_per_call": round(per, 4), "algorithmic_bytes_per_call": nbytes,
                       "algorithmic_tbps": round(nbytes / (per * 1e-3) / 1e12, 4), "share_of_hbm_roofline": round(nbytes / (per * 1e-3) / 1e12 / HBM_TBPS, 4)}
        best = {o: min(v) for o, v in ms.items()}
        spread = {o: round((max(v) - min(v)) / min(v), 4) for o, v in ms.items()}
        shapes[name] = {"ms_per_call": ms, "best_ms": best, "spread": spread, "column_sum": kern, "window_entries": batch * ROW_LEN}
        if not a.sequential_only:
            g0, g1 = last["sequential"], last["segmented"]
            ratio = kern["sequential"]["column_sum_ms_per_call"] / kern["segmented"]["column_sum_ms_per_call"]
            shapes[name].update({"column_sum_ratio_sequential_over_segmented": round(ratio, 3),
                                 "whole_call_ratio_sequential_over_segmented": round(best["sequential"] / best["segmented"], 3),
                                 "faster_by_more_than_both_spreads": bool(best["segmented"] * (1 + max(spread.values())) < best["sequential"]),
                                 "nnz": [g0["nnz"], g1["nnz"]], "objLoss_equal": g0["objLoss"] == g1["objLoss"],
                                 "largest_abs_difference_of_grad": float((g0["grad"] - g1["grad"]).abs().max())})
        del ds, last, legs
    out = {"tool": "tools/bench_glm_segmented.py", "lib": _lib.LIB_PATH if a.sequential_only else "this tree's",
           "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
           "data": {"rows": rows, "dim": dim, "entries_per_row": ROW_LEN, "batch": batch, "weight": "float64", "loss": "L2LogLoss"},
           "constants": {k: _lib.glm_segmented_constant(k) for k in _lib.GLM_SEGMENTED_CONSTANTS},
           "steps": a.steps, "rounds": a.rounds, "hbm_roofline_tbps": HBM_TBPS, "shapes": shapes}
    if a.other_lib and not a.sequential_only:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--sequential-only", "--rows-log2", str(a.rows_log2), "--dim-log2",
                                str(a.dim_log2), "--steps", str(a.steps), "--rounds", str(a.rounds)], env=dict(os.environ, SKML_LIB=os.path.abspath(a.other_lib)),
                               capture_output=True, text=True, check=True)
        other = json.loads(child.stdout.strip().splitlines()[-1])["shapes"]["bias"]
        mine = shapes["bias"]
        out["existing_entry_against_other_lib"] = {
            "entry": "skml_glm_gradient_f64", "other_lib": a.other_lib, "this_best_ms": mine["best_ms"]["sequential"],
            "other_best_ms": other["best_ms"]["sequential"], "this_spread": mine["spread"]["sequential"], "other_spread": other["spread"]["sequential"],
            "within_own_spread": bool(abs(mine["best_ms"]["sequential"] - other["best_ms"]["sequential"]) <=
                                      max(mine["spread"]["sequential"], other["spread"]["sequential"]) * mine["best_ms"]["sequential"])}
    if not a.sequential_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
