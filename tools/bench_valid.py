#!/usr/bin/env python3
"""The validation pass on the device (validation.calLossAucPrecision) on tools/bench_glm.py's synthetic
data set with 2^18 rows, per kernel and beside two other routes to the same numbers:

- the route the pass replaces: pre from optim.batch_gradient(..., want_pre=True) over every row, copied
  to the host and finished in numpy (the losses, the counts, the sequential sum, a stable sort, the
  rank sum);
- a torch-ops route from the device's pre: torch.sort and cumsum.

The per-kernel times come from skml_ctx_kernel_stats in passes of their own (the per-launch events
slow the loop), with the bytes each kernel has to move by the algorithm, computed from the shapes.
The ordered sum is a chain of n dependent additions run by one wave: its time is also given in
nanoseconds per element.  Each timed window is a loop of --steps calls between host clock reads after
device synchronisations, after a warm-up; the variants alternate over --rounds and each variant's own
spread is the margin a difference has to clear.  Nothing is gated: the tool writes down what it
measured and on which box.

usage: python tools/bench_valid.py [--rows-log2 18] [--dim-log2 26] [--steps 10] [--rounds 3] [--out profiles/valid_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_glm import ROW_LEN, make_data, stats, timed  # noqa: E402


def host_finish(np, pre, label):
    """What a user without the pass does with pre on the host: L2LogLoss, the counts, the sums."""
    z = pre * label
    with np.errstate(all="ignore"):
        loss = np.where(z > 18, np.exp(-z), np.where(z < -18, -z, np.log1p(np.exp(-z))))
    pos = pre > 0
    counts = (int((pos & (z > 0)).sum()), int((~pos & (z > 0)).sum()), int((pos & (z < 0)).sum()), int((~pos & (z < 0)).sum()))
    total = float(np.cumsum(loss)[-1])  # cumsum adds in index order
    order = np.argsort(pre, kind="stable")
    hit = label[order] == 1.0
    return total, counts, int(np.nonzero(hit)[0].sum()), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=18)
    ap.add_argument("--dim-log2", type=int, default=26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valid_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_valid: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib, optim
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    rows, dim = 1 << a.rows_log2, 1 << a.dim_log2
    ds, build_ms = make_data(torch, sk, rows, dim, dev)
    nnz = rows * ROW_LEN
    w = torch.randn(dim, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 1e-2
    loss = sk.L2LogLoss(1e-4)
    last = {}

    def device_loss_precision():
        last["lp"] = sk.calLossPrecision(w, ds, loss)

    def device_loss_precision_tree():
        last["tree"] = sk.calLossPrecision(w, ds, loss, order="tree")

    def device_loss_auc_precision():
        last["auc"] = sk.calLossAucPrecision(w, ds, loss)

    def host_route():
        pre = optim.batch_gradient(w, ds, 0, rows, loss, want_pre=True)["pre"].cpu().numpy()
        last["host"] = host_finish(np, pre, ds.label.cpu().numpy())

    def torch_route():
        r = last["lp"]
        total = torch.cumsum(r.loss, 0)[-1]
        idx = torch.sort(r.pre, stable=True).indices
        hit = ds.label[idx] == 1.0
        sigma = torch.cumsum(torch.where(hit, torch.arange(rows, device=dev), 0), 0)[-1]
        last["torch"] = (float(total), int(sigma), int(hit.sum()))

    variants = {"device_calLossPrecision": device_loss_precision, "device_calLossPrecision_tree": device_loss_precision_tree,
                "device_calLossAucPrecision": device_loss_auc_precision, "batch_gradient_pre_to_host_numpy": host_route,
                "torch_sort_cumsum_after_device_pre": torch_route}
    for fn in variants.values():
        timed(torch, fn, 2)
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(round(timed(torch, fn, a.steps), 4))

    # the routes agree: the integers exactly, the sums to the last bits (numpy's and torch's libm and order)
    r = last["auc"]
    agree = {"counts_equal_host": tuple(r[1:5]) == last["host"][1], "sigma_equal_host": r.sigma == last["host"][2],
             "M_equal_host": r.M == last["host"][3], "sigma_equal_torch": r.sigma == last["torch"][1],
             "loss_rel_diff_host": abs(r[0] - last["host"][0]) / abs(r[0]),
             "loss_rel_diff_tree": abs(r[0] - last["tree"][0]) / abs(r[0])}

    def kernel_pass(fn):
        lib.skml_ctx_set_timing(ctx, -1)
        lib.skml_ctx_reset_stats(ctx)
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        got = {kid: stats(lib, ctx, kid) for kid in (_lib.SKML_K_GLM_VALID, _lib.SKML_K_SEQ_SUM, _lib.SKML_K_VALID_SORT,
                                                     _lib.SKML_K_VALID_RANK)}
        lib.skml_ctx_set_timing(ctx, 0)
        return got

    def entry(cnt, tot, nbytes):
        per = tot / a.steps
        return {"launches_per_call": cnt / a.steps, "ms_per_call": round(per, 4), "algorithmic_bytes_per_call": nbytes,
                "algorithmic_tbps": round(nbytes / (per * 1e-3) / 1e12, 4) if per else None}

    seq, tree = kernel_pass(device_loss_auc_precision), kernel_pass(device_loss_precision_tree)
    kern = {"k_glm_valid": entry(*seq[_lib.SKML_K_GLM_VALID], nnz * (4 + 8 + 8) + rows * (16 + 8 + 8 + 8)),
            "ordered_sum_k_glm_seq_sum": entry(*seq[_lib.SKML_K_SEQ_SUM], rows * 8),
            "tree_sum_k_glm_loss_sum": entry(*tree[_lib.SKML_K_SEQ_SUM], rows * 8),
            "sort_keys_and_8_passes": entry(*seq[_lib.SKML_K_VALID_SORT], rows * (8 + 12) + 8 * rows * (8 + 12 + 12)),
            "rank_sum_k_valid_rank_sum": entry(*seq[_lib.SKML_K_VALID_RANK], rows * (4 + 8))}
    kern["ordered_sum_k_glm_seq_sum"]["ns_per_element"] = round(kern["ordered_sum_k_glm_seq_sum"]["ms_per_call"] * 1e6 / rows, 3)
    kern["sort_keys_and_8_passes"]["ms_per_pass"] = round(kern["sort_keys_and_8_passes"]["ms_per_call"] / 8, 4)
    kern["sort_keys_and_8_passes"]["note"] = "a pass is the tile histogram, the scan of the counts and the scatter; ms_per_pass counts the keys launch in"
    kernel_ms = sum(k["ms_per_call"] for n_, k in kern.items() if n_ != "tree_sum_k_glm_loss_sum")

    best = {k: min(v) for k, v in ms.items()}
    out = {"tool": "tools/bench_valid.py", "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
           "data": {"rows": rows, "dim": dim, "entries_per_row": ROW_LEN, "nnz": nnz, "weight": "float64", "loss": "L2LogLoss(1e-4)",
                    "column_order_build_ms": round(build_ms, 1)},
           "result": {"validLoss": r[0], "truePos": r[1], "trueNeg": r[2], "falsePos": r[3], "falseNeg": r[4], "validNum": r[5],
                      "M": r.M, "N": r.N, "sigma": r.sigma, "auc": r.auc},
           "agreement": agree, "steps": a.steps, "rounds": a.rounds, "ms_per_call": ms, "best_ms": best,
           "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()},
           "kernels": kern, "kernel_ms_of_calLossAucPrecision": round(kernel_ms, 4),
           "ordered_sum_share_of_kernel_ms": round(kern["ordered_sum_k_glm_seq_sum"]["ms_per_call"] / kernel_ms, 4),
           "ratio_host_route_over_device_auc": round(best["batch_gradient_pre_to_host_numpy"] / best["device_calLossAucPrecision"], 3),
           "note": "device_* are whole Python calls: two output tensors, the kernels, one synchronisation.  The host route computes "
                   "the gradient it does not need (batch_gradient is the only entry that returned pre before this pass existed).  "
                   "The torch route starts from the device's pre and loss and is not bit-pinned."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    assert np.isfinite(r[0]) and all(v for k, v in agree.items() if k.endswith(("host", "torch")) and isinstance(v, bool))
    return 0


if __name__ == "__main__":
    sys.exit(main())
