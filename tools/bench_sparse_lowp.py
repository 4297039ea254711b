#!/usr/bin/env python3
"""bf16 / fp16 at the two ends of the sparse path against the routes they replace, on one MI355X,
at C3's shape: dim 2^28, 10 % non-zeros, 8 distinct payloads for the sum.

  (a) x16.float() + skml_sparse_encode_f32 (what sparse.encode_dense_as_sparse did with a 16-bit
      tensor) against skml_sparse_encode_bf16 / _f16 on the 16-bit buffer itself; the fp32 encode
      alone (on a buffer cast beforehand) is timed beside them;
  (b) skml_sparse_decode_sum_f64 + .to(float32) / .to(bfloat16) against skml_sparse_decode_sum_f32 /
      _bf16 / _f16;
  (c) skml_sparse_encode_f32 and skml_sparse_decode_sum_f64 of this tree against another build of
      the library (--other-lib, e.g. the parent commit's, loaded through SKML_LIB), in child
      processes that alternate between the two libraries.  The other build must export every
      name of sketchml_amd/_lib.py's table: tools/build_other_lib.py builds a revision's library
      with stubs for the entries it lacks (python tools/build_other_lib.py HEAD~1 gpu_jobs/parent_lib).
Each timed window is a loop of --steps calls between two device events on the codec stream; every
entry ends in a synchronise of its own.  The legs of (a) and of (b) alternate in rounds in one
process after a warm-up; the spread of each leg over its rounds is reported, and a difference has to
clear it.  Every GPU step runs in a child process under its own timeout; the parent process never
touches the GPU and stops at the first step that fails.  Kernel times (k_compact*, the sum-tile
kernels) come from a profiler run of their own: --profile-step encode|sum runs one short loop and
nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_lowp.py --profile-step ...`.

usage: python tools/bench_sparse_lowp.py [--dim 268435456] [--steps 10] [--rounds 3] [--other-lib PATH] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS, GROUPS, ROWS, RATIO, P = 256, 8, 2, 0.3, 8
DENSITY = 0.1


def _timed(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _warm(torch, fns, ms=300.0):
    spent = 0.0
    while spent < ms:
        for fn in fns:
            spent += _timed(torch, fn, 2) * 2


def _spread(v):
    return round((max(v) - min(v)) / min(v), 4)


def _rounds(torch, variants, steps, rounds):
    _warm(torch, list(variants.values()))
    ms = {k: [] for k in variants}
    for _ in range(rounds):  # alternating
        for k, fn in variants.items():
            ms[k].append(round(_timed(torch, fn, steps), 4))
    return ms


def _summary(ms):
    return {"ms_per_call": ms, "best_ms": {k: min(v) for k, v in ms.items()}, "spread": {k: _spread(v) for k, v in ms.items()}}


def _dense(torch, dim, seed):
    """A C3-shaped gradient as bench.py builds one: N(0, 1), 10 % kept."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(dim, device="cuda", generator=g)
    x[torch.rand(dim, device="cuda", generator=g) >= DENSITY] = 0.0
    return x


def _setup():
    import torch

    import sketchml_amd as sk
    from sketchml_amd import _lib
    from sketchml_amd.sparse import _params
    return torch, sk, _lib, _lib.lib, sk.get_context(0).handle, _params(BINS, GROUPS, ROWS, RATIO, 3, 3)


def _encoder(_lib, lib, ctx, p, dim):
    def enc(name, x):
        h = C.c_void_p()
        if getattr(lib, name)(ctx, C.c_void_p(x.data_ptr()), dim, C.byref(p), C.byref(h)):
            raise RuntimeError(_lib.last_error())
        return h
    return enc


def step_encode(dim, steps, rounds, only_f32=False, profile=False):
    torch, sk, _lib, lib, ctx, p = _setup()
    enc = _encoder(_lib, lib, ctx, p, dim)
    xf = _dense(torch, dim, 3)
    xb, xh = xf.to(torch.bfloat16), xf.to(torch.float16)
    xfb = xb.float()  # the fp32 encode's input: the widened bf16 buffer
    del xf

    def run(name, src, cast=False):
        def call(i):
            lib.skml_sparse_free(enc(name, src.float() if cast else src))
        return call

    variants = {"encode_f32_alone": run("skml_sparse_encode_f32", xfb)}
    if not only_f32:
        variants.update({"cast_bf16_plus_encode_f32": run("skml_sparse_encode_f32", xb, True),
                         "encode_bf16": run("skml_sparse_encode_bf16", xb),
                         "cast_f16_plus_encode_f32": run("skml_sparse_encode_f32", xh, True),
                         "encode_f16": run("skml_sparse_encode_f16", xh)})
    if profile:
        for fn in variants.values():
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        return {"profiled": list(variants)}
    res = {"dim": dim, "density": DENSITY, "steps": steps, "rounds": rounds}
    if not only_f32:  # the 16-bit encode gives the fp32 encode's payload
        from sketchml_amd.sparse import SparsePayload
        blobs = []
        for name, src in (("skml_sparse_encode_f32", xfb), ("skml_sparse_encode_bf16", xb)):
            pl = SparsePayload(enc(name, src), 0, ROWS)
            blobs.append(pl.export(sk.alloc_aligned(pl.export_bytes(), "cuda").zero_()))
            res["nnz"] = pl.nnz()
            del pl
        res["payload_identical"] = bool(torch.equal(blobs[0], blobs[1]))
        del blobs
        nnz = res["nnz"]
        # algorithmic bytes of the compaction: the dense read, keys and values written
        res["compaction_bytes"] = {"f32": 4 * dim + 8 * nnz, "cast_plus_f32": 2 * dim + 4 * dim + 4 * dim + 8 * nnz,
                                   "bf16": 2 * dim + 8 * nnz}
    res.update(_summary(_rounds(torch, variants, steps, rounds)))
    return res


def step_sum(dim, steps, rounds, only_f64=False, profile=False):
    torch, sk, _lib, lib, ctx, p = _setup()
    enc = _encoder(_lib, lib, ctx, p, dim)
    from sketchml_amd.distributed import blob_stride
    from sketchml_amd.sparse import SparsePayload
    blobs = []
    for r in range(P):
        x = _dense(torch, dim, 3 + r)
        p.seed = p.hash_seed = 3 + r
        pl = SparsePayload(enc("skml_sparse_encode_f32", x), 0, ROWS)
        blobs.append(pl.export(sk.alloc_aligned(pl.export_bytes(), "cuda")))
        del x, pl
    stride = blob_stride([b.numel() for b in blobs])
    allb = sk.alloc_aligned(stride * P, "cuda").zero_()
    for r, b in enumerate(blobs):
        allb[r * stride:r * stride + b.numel()].copy_(b)
    del blobs
    dts = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    kinds = ["f64"] if only_f64 else list(dts)
    outs = {k: torch.empty(dim, dtype=dts[k], device="cuda") for k in kinds}

    def run(kind, cast=None):
        fn = getattr(lib, "skml_sparse_decode_sum_" + kind)

        def call(i):
            if fn(ctx, C.c_void_p(allb.data_ptr()), P, stride, dim, 1.0 / P, C.c_void_p(outs[kind].data_ptr())):
                raise RuntimeError(_lib.last_error())
            if cast is not None:
                outs[kind].to(cast)
                torch.cuda.current_stream().synchronize()
        return call

    variants = {"sum_f64_alone": run("f64")}
    if not only_f64:
        variants.update({"sum_f64_plus_to_f32": run("f64", torch.float32), "sum_f32": run("f32"),
                         "sum_f64_plus_to_bf16": run("f64", torch.bfloat16), "sum_bf16": run("bf16"), "sum_f16": run("f16")})
    if profile:
        for fn in variants.values():
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        return {"profiled": list(variants)}
    res = {"dim": dim, "P": P, "steps": steps, "rounds": rounds}
    if not only_f64:
        run("f64")(0), run("f32")(0), run("bf16")(0), run("f16")(0)
        torch.cuda.synchronize()
        f = outs["f64"].to(torch.float32)
        res["equals_cast_of_f64"] = {"f32": bool(torch.equal(f.view(torch.int32), outs["f32"].view(torch.int32))),
                                     "bf16": bool(torch.equal(f.to(torch.bfloat16).view(torch.int16), outs["bf16"].view(torch.int16))),
                                     "f16": bool(torch.equal(f.to(torch.float16).view(torch.int16), outs["f16"].view(torch.int16)))}
        del f
        # algorithmic bytes of the sum's store (and of the cast that follows the f64 sum)
        res["store_bytes"] = {"f64": 8 * dim, "f64_plus_to_f32": 8 * dim + 8 * dim + 4 * dim, "f32": 4 * dim,
                              "f64_plus_to_bf16": 8 * dim + 8 * dim + 2 * dim, "bf16": 2 * dim, "f16": 2 * dim}
    res.update(_summary(_rounds(torch, variants, steps, rounds)))
    return res


def _child(job, a, lib=None, timeout=None):
    env = dict(os.environ)
    if lib:
        env["SKML_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(timeout or a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", job,
           "--dim", str(a.dim), "--steps", str(a.steps), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print(f"step {job} failed with status {r.returncode}; stopping", file=sys.stderr)
        sys.exit(r.returncode or 1)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2**28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other-lib", default=None, help="leg (c): another build of libskml.so (the parent commit's)")
    ap.add_argument("--lib-rounds", type=int, default=2, help="leg (c): child processes per library, alternating")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-step", default=None, choices=["encode", "sum"])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_step:
        (step_encode if a.profile_step == "encode" else step_sum)(a.dim, 3, 1, profile=True)
        return 0
    if a.child:
        fn = {"encode": step_encode, "sum": step_sum, "encode_f32": lambda *x: step_encode(*x, only_f32=True),
              "sum_f64": lambda *x: step_sum(*x, only_f64=True)}[a.child]
        print("RESULT " + json.dumps(fn(a.dim, a.steps, a.rounds)))
        return 0
    if a.rounds < 3:
        ap.error("at least 3 alternating rounds")
    out = {"tool": "tools/bench_sparse_lowp.py", "data": "N(0,1), 10 % kept, torch generator seeds 3..10",
           "a_encode": _child("encode", a), "b_sum": _child("sum", a)}
    if a.other_lib:
        legs = {"this_tree": {"encode_f32": [], "sum_f64": []}, "other_lib": {"encode_f32": [], "sum_f64": []}}
        for _ in range(a.lib_rounds):  # alternating processes
            for who, lib in (("this_tree", None), ("other_lib", a.other_lib)):
                legs[who]["encode_f32"] += _child("encode_f32", a, lib)["ms_per_call"]["encode_f32_alone"]
                legs[who]["sum_f64"] += _child("sum_f64", a, lib)["ms_per_call"]["sum_f64_alone"]
        out["c_against_other_lib"] = {
            who: {k: {"ms_per_call": v, "best_ms": min(v), "spread": _spread(v)} for k, v in d.items()}
            for who, d in legs.items()}
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
