#!/usr/bin/env python3
"""The FixedPointGradient codec against the sketch's dense codec, same gradient, same GPU.

For each size (fp32, N(0,1) * 1e-3) and each width b: skml_fixed_encode_f32 / _decode_f32 /
_decode_sum_f32 (8 payloads) beside skml_dense_encode_f32 / _decode_f32 / _decode_sum_f32 at the
paired bin count (b = 8 with 256 requested bins: the same bytes per element as k_quantize /
k_decode; b = 4 with 4 bins), all six in one process.  Each timed window is a loop of --steps calls
between two HIP events on the codec stream, over two rotating buffers, after a warm-up of sustained
load past the clock ramp; the variants are timed in alternating rounds (--rounds, at least 3) and
the spread of each variant's own rounds is reported as the margin a difference has to clear.  The
per-kernel times (the norm's two launches under SKML_K_SUMMARY, the quantize + pack pass under
SKML_K_QUANTIZE, the decodes) come from skml_ctx_kernel_stats in a pass of their own: the per-launch
events slow the loop.  Every (size, width) runs in a child process under its own timeout; the parent
never touches the GPU and stops at the first step that fails.  Recorded, not gated.

usage: python tools/bench_fixed_point.py [--sizes 67108864,268435456] [--bits 8,4] [--steps 20] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_LEAF, K_MERGE, K_SUMMARY, K_QUANTIZE, K_DECODE, K_DECODE_SUM = 0, 1, 2, 3, 4, 5
PAIRED_BINS = {8: 256, 4: 4}
P = 8


def _timed(torch, fn, steps):
    """ms per call of fn(i), i = 0..steps-1, between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _warm(torch, fns, ms=300.0):
    """Every variant, until `ms` of sustained load has passed (the engine clock has settled)."""
    spent = 0.0
    while spent < ms:
        for fn in fns:
            spent += _timed(torch, fn, 4) * 4


def _stats(lib, ctx, kid):
    cnt, ms = C.c_int64(), C.c_double()
    lib.skml_ctx_kernel_stats(ctx, kid, C.byref(cnt), C.byref(ms))
    return cnt.value, 1000.0 * ms.value


def _spread(v):
    return round((max(v) - min(v)) / min(v), 4)


def step(n, bits, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    bins = PAIRED_BINS.get(bits, 1 << min(bits, 16))
    xs = []
    for r in range(2):  # two rotating buffers
        g = torch.Generator(device=dev).manual_seed(2 + r)
        xs.append(torch.randn(n, device=dev, generator=g) * 1e-3)
    fnb, dnb = lib.skml_fixed_payload_bytes(n, bits), lib.skml_dense_payload_bytes(n, bins)
    fstride, dstride = fnb, (dnb + 255) // 256 * 256
    fall, dall = sk.alloc_aligned(fstride * P, dev), sk.alloc_aligned(dstride * P, dev)
    p = _lib.Params()
    lib.skml_params_default(C.byref(p))
    p.bin_num = bins

    def ok(st):
        if st:
            raise RuntimeError(_lib.last_error())

    for r in range(P):  # the gathered payloads of the decode-sums: P distinct gradients
        g = torch.Generator(device=dev).manual_seed(40 + r)
        x = torch.randn(n, device=dev, generator=g) * 1e-3
        p.seed = 4 + r
        ok(lib.skml_fixed_encode_f32(ctx, C.c_void_p(x.data_ptr()), n, bits, 4 + r, C.c_void_p(fall.data_ptr() + r * fstride), fstride))
        ok(lib.skml_dense_encode_f32(ctx, C.c_void_p(x.data_ptr()), n, C.byref(p), C.c_void_p(dall.data_ptr() + r * dstride), dstride))
        torch.cuda.synchronize()
        del x
    fpl, dpl = sk.alloc_aligned(fnb, dev), sk.alloc_aligned(dnb, dev)
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    p.seed = 2

    def fx_encode(i):
        ok(lib.skml_fixed_encode_f32(ctx, C.c_void_p(xs[i & 1].data_ptr()), n, bits, 2, C.c_void_p(fpl.data_ptr()), fnb))

    def dn_encode(i):
        ok(lib.skml_dense_encode_f32(ctx, C.c_void_p(xs[i & 1].data_ptr()), n, C.byref(p), C.c_void_p(dpl.data_ptr()), dnb))

    def fx_decode(i):
        ok(lib.skml_fixed_decode_f32(ctx, C.c_void_p(fall.data_ptr() + (i % P) * fstride), C.c_void_p(outs[i & 1].data_ptr()), n))

    def dn_decode(i):
        ok(lib.skml_dense_decode_f32(ctx, C.c_void_p(dall.data_ptr() + (i % P) * dstride), C.c_void_p(outs[i & 1].data_ptr()), n))

    def fx_sum(i):
        ok(lib.skml_fixed_decode_sum_f32(ctx, C.c_void_p(fall.data_ptr()), P, fstride, C.c_void_p(outs[i & 1].data_ptr()), n, 1.0 / P))

    def dn_sum(i):
        ok(lib.skml_dense_decode_sum_f32(ctx, C.c_void_p(dall.data_ptr()), P, dstride, C.c_void_p(outs[i & 1].data_ptr()), n, 1.0 / P))

    variants = {"fixed_encode": fx_encode, "dense_encode": dn_encode, "fixed_decode": fx_decode, "dense_decode": dn_decode,
                "fixed_decode_sum": fx_sum, "dense_decode_sum": dn_sum}
    _warm(torch, list(variants.values()))
    ms = {k: [] for k in variants}
    for _ in range(rounds):  # alternating
        for k, fn in variants.items():
            ms[k].append(round(_timed(torch, fn, steps), 4))
    # per-kernel times, a pass of their own
    kern = {}
    for k, fn in variants.items():
        lib.skml_ctx_set_timing(ctx, -1)
        lib.skml_ctx_reset_stats(ctx)
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        kern[k] = {}
        for name, kid in (("leaf", K_LEAF), ("merge", K_MERGE), ("summary_or_norm", K_SUMMARY), ("quantize", K_QUANTIZE),
                          ("decode", K_DECODE), ("decode_sum", K_DECODE_SUM)):
            cnt, us = _stats(lib, ctx, kid)
            if cnt:
                kern[k][name + "_us_per_call"] = round(us / steps, 2)
        lib.skml_ctx_set_timing(ctx, 0)
    hdr = _lib.DenseHeader()
    lib.skml_dense_info(ctx, C.c_void_p(dpl.data_ptr()), C.byref(hdr), None, 0)
    best = {k: min(v) for k, v in ms.items()}
    fq, dq = kern["fixed_encode"]["quantize_us_per_call"], kern["dense_encode"]["quantize_us_per_call"]
    res = {"n": n, "num_bits": bits, "dense_bins": bins, "dense_bin_num": hdr.bin_num, "dense_code_bits": hdr.code_bits,
           "P": P, "steps": steps, "rounds": rounds, "ms_per_call": ms, "best_ms": best,
           "spread": {k: _spread(v) for k, v in ms.items()}, "kernels": kern,
           "ratio_fixed_over_dense": {"encode": round(best["fixed_encode"] / best["dense_encode"], 4),
                                      "decode": round(best["fixed_decode"] / best["dense_decode"], 4),
                                      "decode_sum": round(best["fixed_decode_sum"] / best["dense_decode_sum"], 4),
                                      "quantize_pass": round(fq / dq, 4)},
           "fixed_quantize_tbps": round(n * (4.0 + bits / 8.0) / (fq * 1e-6) / 1e12, 3),
           "dense_quantize_tbps": round(n * (4.0 + hdr.code_bits / 8.0) / (dq * 1e-6) / 1e12, 3),
           "fixed_norm_tbps": round(n * 4.0 / (kern["fixed_encode"]["summary_or_norm_us_per_call"] * 1e-6) / 1e12, 3),
           "fixed_decode_tbps": round(n * (4.0 + bits / 8.0) / (best["fixed_decode"] * 1e-3) / 1e12, 3),
           "fixed_decode_sum_tbps": round(n * (4.0 + P * bits / 8.0) / (best["fixed_decode_sum"] * 1e-3) / 1e12, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="67108864,268435456")
    ap.add_argument("--bits", default="8,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20 or a.rounds < 3:
        ap.error("at least 20 steps per window and 3 alternating rounds")
    if a.child:
        n, bits = a.child.split(":")
        print("RESULT " + json.dumps(step(int(n), int(bits), a.steps, a.rounds)))
        return 0
    out = {"tool": "tools/bench_fixed_point.py", "data": "N(0,1) * 1e-3 fp32, torch generator", "results": []}
    for s in a.sizes.split(","):
        for b in a.bits.split(","):
            job = f"{int(s)}:{int(b)}"
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", job,
                   "--steps", str(a.steps), "--rounds", str(a.rounds)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                print(f"step {job} failed with status {r.returncode}; stopping", file=sys.stderr)
                return r.returncode or 1
            out["results"].append(json.loads(lines[-1][7:]))
            print(f"step {job}: {out['results'][-1]['best_ms']}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
