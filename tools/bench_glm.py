#!/usr/bin/env python3
"""The mini-batch gradient on the device (optim.GradientDescent.miniBatchGradientDescent) on a synthetic
sparse data set, beside the route it replaces: the same gradient as a host array, uploaded, then
SketchGradient.

Data (seeded, generated on the device): 2^20 instances over 2^26 features, 64 entries per instance: the
bias feature 0 and one feature from each of 63 equal strata of the others, so the columns of a row
ascend; values N(0,1), labels +-1, weights N(0,1) * 1e-2.  batchSpRatio 0.1, L2LogLoss(1e-4).

Each timed window is a loop of --steps calls between a host clock read after a device
synchronisation and another after the loop's last synchronisation (every call synchronises by
itself), after a warm-up; the variants alternate over --rounds and each variant's own spread is the
margin a difference has to clear.  The per-kernel times come from skml_ctx_kernel_stats in a pass
of their own, with the bytes each kernel has to move by the algorithm (computed from the shapes
and the windows' entry counts; the binary searches' reads are not counted).  Nothing is gated: the
tool writes down what it measured and on which box.

usage: python tools/bench_glm.py [--rows-log2 20] [--dim-log2 26] [--steps 10] [--rounds 3] [--out profiles/glm_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_LEN = 64
RATIO = 0.1


def make_data(torch, sk, rows, dim, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    stratum = (dim - 1) // (ROW_LEN - 1)
    col = torch.empty((rows, ROW_LEN), dtype=torch.int64, device=dev)
    col[:, 0] = 0
    col[:, 1:] = 1 + torch.arange(ROW_LEN - 1, device=dev) * stratum + torch.randint(
        0, stratum, (rows, ROW_LEN - 1), device=dev, generator=g)
    val = torch.randn(rows * ROW_LEN, dtype=torch.float64, device=dev, generator=g)
    label = torch.where(torch.rand(rows, device=dev, generator=g) < 0.5, 1.0, -1.0).double()
    row_ptr = torch.arange(rows + 1, dtype=torch.int64, device=dev) * ROW_LEN
    ds = sk.DataSet.fromCSR(row_ptr, col.view(-1), val, label, dim, device=dev)
    t0 = time.perf_counter()
    ds.glm_data()  # validates and builds the column order
    torch.cuda.synchronize()
    return ds, (time.perf_counter() - t0) * 1e3


def timed(torch, fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def stats(lib, ctx, kid):
    cnt, ms = C.c_int64(), C.c_double()
    lib.skml_ctx_kernel_stats(ctx, kid, C.byref(cnt), C.byref(ms))
    return cnt.value, ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=20)
    ap.add_argument("--dim-log2", type=int, default=26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_glm: no GPU; a time is never taken on the CPU", file=sys.stderr)
        return 1
    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    rows, dim = 1 << a.rows_log2, 1 << a.dim_log2
    ds, build_ms = make_data(torch, sk, rows, dim, dev)
    w = torch.randn(dim, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 1e-2
    loss = sk.L2LogLoss(1e-4)
    opt = sk.GradientDescent(dim, 0.1, 0.0, RATIO)
    batch = int(rows * RATIO)
    last = {}

    def device_gradient():
        last["grad"], _, last["obj"], last["reg"] = opt.miniBatchGradientDescent(w, ds, loss)

    def device_route():
        device_gradient()
        last["sketch"] = sk.SketchGradient(last["grad"])

    # the route this replaces: the gradient is born on the host (toAuto's form, as the reference holds
    # it), goes up through pageable memory, and is compressed there
    device_gradient()
    grad = last["grad"]
    sparse = grad.kind() == sk.Kind.SparseDouble
    host_vals = grad.values.cpu().numpy()
    host_keys = grad.indices.cpu().numpy() if sparse else None

    def host_route():
        vals = torch.from_numpy(host_vals).to(dev)
        if sparse:
            g = sk.SparseDoubleGradient(dim, torch.from_numpy(host_keys).to(dev), vals)
        else:
            g = sk.DenseDoubleGradient(dim, vals)
        last["host_sketch"] = sk.SketchGradient(g)

    def upload_only():
        last["up"] = torch.from_numpy(host_vals).to(dev)
        if sparse:
            last["upk"] = torch.from_numpy(host_keys).to(dev)

    variants = {"device_gradient": device_gradient, "device_gradient_then_sketch": device_route,
                "host_array_upload_then_sketch": host_route, "host_array_upload_only": upload_only}
    for fn in variants.values():
        timed(torch, fn, 3)
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(round(timed(torch, fn, a.steps), 4))

    # per-kernel times and their algorithmic bytes, a pass of their own
    lib.skml_ctx_set_timing(ctx, -1)
    lib.skml_ctx_reset_stats(ctx)
    entries = 0
    form_nnz = 0
    for _ in range(a.steps):
        r0 = 0 if ds.readIndex >= rows else ds.readIndex
        device_gradient()
        end = r0 + batch
        entries += int(ds.row_ptr[min(end, rows)] - ds.row_ptr[r0]) + (int(ds.row_ptr[end - rows]) if end > rows else 0)
        form_nnz += last["grad"].values.numel()
    torch.cuda.synchronize()
    kern = {}
    per = {"predict_and_loss_sum": (_lib.SKML_K_GLM_PREDICT,
                                    entries * (4 + 8 + 8) + a.steps * batch * (16 + 8 + 16 + 8)),
           "plus_by": (_lib.SKML_K_GLM_PLUS_BY, a.steps * dim * (8 + 8) + entries * (4 + 8 + 8)),
           "finish": (_lib.SKML_K_GLM_FINISH, form_nnz * (8 + 8 + ((4 + 8) if sparse else 8))),
           "compaction_skml_sparse_compact_f64": (6, a.steps * dim * 8 + form_nnz * 12 if sparse else 0)}
    for name, (kid, nbytes) in per.items():
        cnt, tot = stats(lib, ctx, kid)
        if cnt:
            kern[name] = {"launches_per_call": cnt / a.steps, "ms_per_call": round(tot / a.steps, 4),
                          "algorithmic_bytes_per_call": nbytes // a.steps,
                          "algorithmic_tbps": round(nbytes / a.steps / (tot / a.steps * 1e-3) / 1e12, 4) if tot else None}
    lib.skml_ctx_set_timing(ctx, 0)

    best = {k: min(v) for k, v in ms.items()}
    out = {"tool": "tools/bench_glm.py", "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
           "data": {"rows": rows, "dim": dim, "entries_per_row": ROW_LEN, "nnz": rows * ROW_LEN, "bias_column": 0,
                    "batchSpRatio": RATIO, "batch": batch, "weight": "float64", "loss": "L2LogLoss(1e-4)",
                    "column_order_build_ms": round(build_ms, 1)},
           "gradient": {"form": "sparse" if sparse else "dense", "nnz": int(grad.values.numel()),
                        "window_entries_per_call": entries // a.steps, "objLoss": last["obj"], "regLoss": last["reg"]},
           "steps": a.steps, "rounds": a.rounds, "ms_per_call": ms, "best_ms": best,
           "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()},
           "kernels": kern,
           "host_bytes_uploaded": int(host_vals.nbytes + (host_keys.nbytes if sparse else 0)),
           "ratio_host_route_over_device_route": round(best["host_array_upload_then_sketch"] / best["device_gradient_then_sketch"], 3),
           "note": "device_gradient is the whole miniBatchGradientDescent call: its kernels, toAuto's compaction, two host "
                   "synchronisations and regLoss.  The host route does not include computing the gradient on the host at all: "
                   "it starts from the finished host array."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    assert np.isfinite(last["obj"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
