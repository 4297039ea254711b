#!/usr/bin/env python3
"""The ZipML codec (skml_zip_encode_f32) beside the sketch's dense encode, same gradient, same GPU.

For each size (fp32, N(0,1) * 1e-3, 256 bins): ms per encode of skml_zip_encode_f32 and of
skml_dense_encode_f32, each a loop of --steps calls between two HIP events on the codec stream over
two rotating inputs, after a warm-up, in alternating rounds (the spread of a variant's own rounds is
the margin a difference has to clear).  The stages of the Zip encode come from skml_ctx_kernel_stats
in a pass of their own: sort = the debug hook without the prefix sums, scan = the whole hook minus
that, rounds = the encode's SKML_K_SUMMARY minus the whole hook (the split search with its host
round trips, and the header), quantize = SKML_K_QUANTIZE.  Also the round count, the scratch the call
allocates, and the decode's relative L2 error for Zip, Sketch and Uniform on the same values.
Every size runs in a child process under its own timeout; the parent never touches the GPU and
stops at the first step that fails.  Recorded, not gated.

usage: python tools/bench_zip.py [--sizes 1048576,16777216,67108864,268435456] [--steps 5] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_SUMMARY, K_QUANTIZE = 2, 3
BINS = 256


def _timed(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _stats(lib, ctx, kid):
    cnt, ms = C.c_int64(), C.c_double()
    lib.skml_ctx_kernel_stats(ctx, kid, C.byref(cnt), C.byref(ms))
    return ms.value


def step(n, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    xs = []
    for r in range(2):
        g = torch.Generator(device=dev).manual_seed(2 + r)
        xs.append(torch.randn(n, device=dev, generator=g) * 1e-3)
    nb = lib.skml_dense_payload_bytes(n, BINS)
    zpl, dpl = sk.alloc_aligned(nb, dev), sk.alloc_aligned(nb, dev)
    p = _lib.Params()
    lib.skml_params_default(C.byref(p))
    p.bin_num, p.seed = BINS, 2

    def ok(st):
        if st:
            raise RuntimeError(_lib.last_error())

    def zip_encode(i):
        ok(lib.skml_zip_encode_f32(ctx, C.c_void_p(xs[i & 1].data_ptr()), n, BINS, C.c_void_p(zpl.data_ptr()), nb))

    def dense_encode(i):
        ok(lib.skml_dense_encode_f32(ctx, C.c_void_p(xs[i & 1].data_ptr()), n, C.byref(p), C.c_void_p(dpl.data_ptr()), nb))

    variants = {"zip_encode": zip_encode, "dense_encode": dense_encode}
    spent = 0.0
    while spent < 300.0:  # sustained load past the clock ramp
        for fn in variants.values():
            spent += _timed(torch, fn, 2) * 2
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(round(_timed(torch, fn, steps), 4))

    # the stages, a pass of their own
    srt, r, t = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))

    def timed_stats(fn, kid):
        lib.skml_ctx_set_timing(ctx, -1)
        lib.skml_ctx_reset_stats(ctx)
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        out = [_stats(lib, ctx, k) / steps for k in kid]
        lib.skml_ctx_set_timing(ctx, 0)
        return out

    def hook(full):
        rp, tp = (C.c_void_p(r.data_ptr()), C.c_void_p(t.data_ptr())) if full else (None, None)
        return lambda i: ok(lib.skml_debug_zip_prefix_f32(ctx, C.c_void_p(xs[i & 1].data_ptr()), n, C.c_void_p(srt.data_ptr()), rp, tp))

    sort_ms, = timed_stats(hook(False), [K_SUMMARY])
    prefix_ms, = timed_stats(hook(True), [K_SUMMARY])
    summary_ms, quant_ms = timed_stats(zip_encode, [K_SUMMARY, K_QUANTIZE])
    del srt, r, t
    n_rounds = lib.skml_debug_zip_rounds(ctx)

    # decode error of the three quantizers on xs[0]
    x = xs[0]
    norm = float(torch.linalg.vector_norm(x.double()))
    err = {}
    for name, q in (("zip", sk.ZipMLQuantizer(BINS)), ("sketch", sk.QuantileQuantizer(BINS, seed=2)), ("uniform", sk.UniformQuantizer(BINS))):
        q.quantize(x)
        d = q.decode()
        err[name] = float(torch.linalg.vector_norm((d - x).double())) / norm
        del d, q
    hdr = _lib.DenseHeader()
    lib.skml_dense_info(ctx, C.c_void_p(zpl.data_ptr()), C.byref(hdr), None, 0)
    best = {k: min(v) for k, v in ms.items()}
    ws = lib.skml_zip_workspace_bytes(n, 0)
    return {"n": n, "bins": BINS, "zip_bin_num": hdr.bin_num, "steps": steps, "rounds": rounds, "ms_per_call": ms,
            "best_ms": best, "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()},
            "ratio_zip_over_dense": round(best["zip_encode"] / best["dense_encode"], 2),
            "zip_stage_ms": {"sort": round(sort_ms, 4), "scan": round(prefix_ms - sort_ms, 4),
                             "rounds": round(summary_ms - prefix_ms, 4), "quantize": round(quant_ms, 4)},
            "zip_halving_rounds": n_rounds, "zip_workspace_bytes": ws, "zip_workspace_bytes_per_value": round(ws / n, 2),
            "decode_rel_l2_error": {k: float(f"{v:.6g}") for k, v in err.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,16777216,67108864,268435456")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 3 or a.rounds < 3:
        ap.error("at least 3 steps per window and 3 alternating rounds")
    if a.child:
        print("RESULT " + json.dumps(step(int(a.child), a.steps, a.rounds)))
        return 0
    out = {"tool": "tools/bench_zip.py", "data": "N(0,1) * 1e-3 fp32, torch generator", "results": []}
    for s in a.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(int(s)),
               "--steps", str(a.steps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"step {s} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        out["results"].append(json.loads(lines[-1][7:]))
        print(f"step {s}: {out['results'][-1]['best_ms']} {out['results'][-1]['zip_stage_ms']}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
