#!/usr/bin/env python3
"""bf16 gradients through the dense codec against the fp32 upcast they replace, on one MI355X.

Three things, on N(0,1) data rounded to bf16, 256 bins:
  (a) what the library did before the 16-bit entries: x.float() then skml_dense_encode_f32, timed
      as cast + encode together and as the encode alone (on a buffer cast beforehand);
  (b) skml_dense_encode_bf16 on the bf16 buffer itself;
  (c) skml_dense_decode_sum_f32 against skml_dense_decode_sum_bf16 for 8 payloads of 2^26 codes.
Each timed window is a loop of --steps calls between two HIP events on the codec stream, over two
rotating input buckets, after a warm-up of sustained load past the clock ramp.  The variants are
timed in alternating rounds (--rounds, at least 3 each) in one process; the spread of (a)'s own
rounds is reported as the margin a difference has to clear.  The per-kernel leaf / merge / quantize
times come from skml_ctx_kernel_stats in a pass of their own (the per-launch events slow the loop).
Every GPU step (one size, or the decode-sum) runs in a child process under its own timeout; the
parent never touches the GPU and stops at the first step that fails.

usage: python tools/bench_lowp.py [--sizes 67108864,268435456] [--steps 20] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_LEAF, K_MERGE, K_QUANTIZE, K_DECODE_SUM = 0, 1, 3, 5
BINS = 256


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
    return 1000.0 * ms.value / max(cnt.value, 1)


def _spread(v):
    return round((max(v) - min(v)) / min(v), 4)


def step_encode(n, steps, rounds):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    xb, xf = [], []
    for r in range(2):  # two rotating buckets
        g = torch.Generator(device=dev).manual_seed(2 + r)
        x = torch.randn(n, device=dev, generator=g)
        xb.append(x.to(torch.bfloat16))
        xf.append(xb[r].float())
        del x
    nb = lib.skml_dense_payload_bytes(n, BINS)
    pl = sk.alloc_aligned(nb, dev)
    p = _lib.Params()
    lib.skml_params_default(C.byref(p))
    p.bin_num, p.seed = BINS, 2

    def enc(name, x):
        if getattr(lib, name)(ctx, C.c_void_p(x.data_ptr()), n, C.byref(p), C.c_void_p(pl.data_ptr()), nb):
            raise RuntimeError(_lib.last_error())

    def cast_f32(i):
        enc("skml_dense_encode_f32", xb[i & 1].float())  # the 4 n-byte temporary lives for this call

    def f32(i):
        enc("skml_dense_encode_f32", xf[i & 1])

    def bf16(i):
        enc("skml_dense_encode_bf16", xb[i & 1])

    variants = {"cast_plus_encode_f32": cast_f32, "encode_f32_alone": f32, "encode_bf16": bf16}
    # the two encodes of one bucket give the same payload (checked on the bytes that carry data)
    hdr = _lib.DenseHeader()
    f32(0)
    lib.skml_dense_info(ctx, C.c_void_p(pl.data_ptr()), C.byref(hdr), None, 0)
    live = slice(hdr.codes_offset, hdr.codes_offset + n * hdr.code_bits // 8)
    ref_codes, ref_head = pl[live].clone(), pl[:64 + 8 * (hdr.bin_num - 1)].clone()
    bf16(0)
    torch.cuda.synchronize()
    same = bool(torch.equal(pl[live], ref_codes) and torch.equal(pl[:64 + 8 * (hdr.bin_num - 1)], ref_head))
    del ref_codes
    _warm(torch, list(variants.values()))
    ms = {k: [] for k in variants}
    for _ in range(rounds):  # alternating
        for k, fn in variants.items():
            ms[k].append(round(_timed(torch, fn, steps), 4))
    # per-kernel times, a pass of their own
    kern = {}
    for k, fn in (("f32", f32), ("bf16", bf16)):
        lib.skml_ctx_set_timing(ctx, (1 << K_LEAF) | (1 << K_MERGE) | (1 << K_QUANTIZE))
        lib.skml_ctx_reset_stats(ctx)
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        kern[k] = {"leaf_us": round(_stats(lib, ctx, K_LEAF), 2), "merge_us_per_launch": round(_stats(lib, ctx, K_MERGE), 2),
                   "quantize_us": round(_stats(lib, ctx, K_QUANTIZE), 2)}
        lib.skml_ctx_set_timing(ctx, 0)
    code_b = hdr.code_bits / 8.0
    for k, in_b in (("f32", 4.0), ("bf16", 2.0)):
        kern[k]["quantize_bytes_per_elem"] = in_b + code_b
        kern[k]["quantize_tbps"] = round(n * (in_b + code_b) / (kern[k]["quantize_us"] * 1e-6) / 1e12, 3)
    best = {k: min(v) for k, v in ms.items()}
    return {"n": n, "bins": BINS, "bin_num": hdr.bin_num, "steps": steps, "rounds": rounds, "ms_per_step": ms,
            "best_ms": best, "spread_encode_f32_alone": _spread(ms["encode_f32_alone"]),
            "spread_cast_plus_encode_f32": _spread(ms["cast_plus_encode_f32"]),
            "bf16_over_f32_alone": round(best["encode_bf16"] / best["encode_f32_alone"], 4),
            "bf16_over_cast_plus_f32": round(best["encode_bf16"] / best["cast_plus_encode_f32"], 4),
            "payload_identical": same, "kernels": kern}


def step_decode_sum(n, steps, rounds, P=8):
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    ctx = sk.get_context(0).handle
    nb = lib.skml_dense_payload_bytes(n, BINS)
    stride = (nb + 255) // 256 * 256
    allp = sk.alloc_aligned(stride * P, dev)
    p = _lib.Params()
    lib.skml_params_default(C.byref(p))
    p.bin_num = BINS
    for r in range(P):
        g = torch.Generator(device=dev).manual_seed(4 + r)
        x = torch.randn(n, device=dev, generator=g).to(torch.bfloat16)
        p.seed = 4 + r
        if lib.skml_dense_encode_bf16(ctx, C.c_void_p(x.data_ptr()), n, C.byref(p),
                                      C.c_void_p(allp.data_ptr() + r * stride), stride):
            raise RuntimeError(_lib.last_error())
        torch.cuda.synchronize()
        del x
    outs = {"f32": [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)],
            "bf16": [torch.empty(n, dtype=torch.bfloat16, device=dev) for _ in range(2)]}

    def run(kind):
        fn = getattr(lib, "skml_dense_decode_sum_" + kind)

        def call(i):
            if fn(ctx, C.c_void_p(allp.data_ptr()), P, stride, C.c_void_p(outs[kind][i & 1].data_ptr()), n, 1.0 / P):
                raise RuntimeError(_lib.last_error())
        return call

    variants = {"decode_sum_f32": run("f32"), "decode_sum_bf16": run("bf16")}
    _warm(torch, list(variants.values()))
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(round(_timed(torch, fn, steps), 4))
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["f32"][0].to(torch.bfloat16), outs["bf16"][0]))
    hdr = _lib.DenseHeader()
    lib.skml_dense_info(ctx, C.c_void_p(allp.data_ptr()), C.byref(hdr), None, 0)
    best = {k: min(v) for k, v in ms.items()}
    res = {"n": n, "P": P, "bins": BINS, "code_bits": hdr.code_bits, "steps": steps, "rounds": rounds,
           "ms_per_call": ms, "best_ms": best, "spread_decode_sum_f32": _spread(ms["decode_sum_f32"]),
           "bf16_over_f32": round(best["decode_sum_bf16"] / best["decode_sum_f32"], 4),
           "bf16_equals_rounded_f32": same}
    for k, out_b in (("decode_sum_f32", 4.0), ("decode_sum_bf16", 2.0)):
        alg = P * n * hdr.code_bits / 8.0 + out_b * n
        res[k + "_tbps"] = round(alg / (best[k] * 1e-3) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="67108864,268435456")
    ap.add_argument("--sum-n", type=int, default=2**26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20 or a.rounds < 3:
        ap.error("at least 20 steps per window and 3 alternating rounds")
    if a.child:
        kind, n = a.child.split(":")
        res = step_encode(int(n), a.steps, a.rounds) if kind == "encode" else step_decode_sum(int(n), a.steps, a.rounds)
        print("RESULT " + json.dumps(res))
        return 0
    jobs = [f"encode:{int(s)}" for s in a.sizes.split(",") if s] + [f"decode_sum:{a.sum_n}"]
    out = {"tool": "tools/bench_lowp.py", "data": "N(0,1) rounded to bf16, torch generator", "encode": [], "decode_sum": None}
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", job,
               "--steps", str(a.steps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"step {job} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        res = json.loads(lines[-1][7:])
        if job.startswith("encode"):
            out["encode"].append(res)
        else:
            out["decode_sum"] = res
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
