"""Null-stream lint of the HIP host code (sketchml_amd/csrc/*.{cpp,hip,hpp,h}).

Every entry's device work must run on the context's stream (DESIGN.md "Stream-ordering contract").
A call that lands on the null stream is not ordered with a non-blocking stream, so it can run
before or after the kernels that depend on it: the batched encode's side lane once counted on a
workspace that a null-stream hipMemset had not zeroed yet.  This scan, over the sources with
comments and string literals stripped, fails on

- a synchronous call that lands on the null stream (hipMemset, hipMemcpy, ... hipDeviceSynchronize);
- an ...Async call, hipLaunchKernelGGL, hipEventRecord or hipStreamWaitEvent whose stream argument
  is the literal 0 / nullptr / NULL / hipStreamDefault, or is left to its default (which is 0).

The allow-list is keyed by file and by the stripped text of the call, never by line number; an
entry that matches nothing fails the test.  tests/test_gpu_stream_order.py is the run-time side.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sketchml_amd", "csrc")

SYNC_NULL = ("hipMemset", "hipMemsetD8", "hipMemsetD16", "hipMemsetD32", "hipMemcpy", "hipMemcpy2D",
             "hipMemcpyToSymbol", "hipMemcpyFromSymbol", "hipMemcpyDtoD", "hipMemcpyHtoD", "hipMemcpyDtoH",
             "hipDeviceSynchronize")
# position of the stream argument; for the ...Async calls also the full argument count, because
# their stream parameter defaults to 0 when it is left out
STREAM_ARG = {"hipLaunchKernelGGL": 4, "hipEventRecord": 1, "hipStreamWaitEvent": 0}
ASYNC_ARITY = {"hipMemcpyAsync": 5, "hipMemsetAsync": 4, "hipMemsetD8Async": 4, "hipMemsetD16Async": 4,
               "hipMemsetD32Async": 4, "hipMemcpy2DAsync": 8, "hipMemcpyDtoDAsync": 4, "hipMemcpyHtoDAsync": 4,
               "hipMemcpyDtoHAsync": 4, "hipMemcpyToSymbolAsync": 6, "hipMemcpyFromSymbolAsync": 6,
               "hipMallocAsync": 3, "hipFreeAsync": 2, "hipMemPrefetchAsync": 4}
NULL_STREAMS = {"0", "nullptr", "NULL", "hipStreamDefault", "(hipStream_t)0", "hipStream_t(0)", "(hipStream_t)nullptr",
                "hipStream_t{}", "hipStream_t{0}"}

# (file, stripped call text) -> one-line reason
# (skml_ctx_create's jump-table upload was the one product-path entry; it now runs on the context's
# stream, because behind a busy null stream it stalled context creation: test_gpu_stream_order.py)
ALLOW = {
    ("skml_sketch.hip", "hipMemcpyFromSymbol(out,HIP_SYMBOL(skml::g_leafprof),sizeof(unsigned long long)*(size_t)cap)"):
        "skml_debug_leafprof (SKML_PROF_LEAF builds only): host read-back of profiling counters, no product path",
    ("skml_sketch.hip", "hipMemcpyFromSymbol(out,HIP_SYMBOL(skml::g_prof),sizeof(unsigned long long)*(size_t)(cap<32?cap:32))"):
        "skml_debug_prof: host read-back of profiling counters after the caller synchronised, no product path",
}

_CALL = re.compile(r"\b(hip\w+)\s*\(")
_OPEN, _CLOSE = "([{", ")]}"


def strip_source(src: str) -> str:
    """The source without comments; string and character literals emptied.  Line breaks stay."""
    out, i, n = [], 0, len(src)
    while i < n:
        ch = src[i]
        two = src[i:i + 2]
        if two == "//":
            while i < n and src[i] != "\n":
                i += 1
        elif two == "/*":
            j = src.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("\n" * src.count("\n", i, j) or " ")
            i = j
        elif ch == '"' or (ch == "'" and not (i and src[i - 1].isalnum())):  # 1'000 is a digit separator
            j = i + 1
            while j < n and src[j] != ch:
                j += 2 if src[j] == "\\" else 1
            out.append(ch + ch)
            i = j + 1
        else:
            out.append(ch)
            i += 1
    return "".join(out)


def squeeze(text: str) -> str:
    """Whitespace-independent form of a piece of code: no space next to punctuation, one elsewhere."""
    return re.sub(r"\s*([^\w\s])\s*", r"\1", re.sub(r"\s+", " ", text)).strip()


def calls(stripped: str):
    """(name, [arguments], call text) of every hip* call; arguments split at commas of bracket depth 0,
    across line breaks."""
    for m in _CALL.finditer(stripped):
        depth, start, args, i = 1, m.end(), [], m.end()
        while i < len(stripped) and depth:
            c = stripped[i]
            if c in _OPEN:
                depth += 1
            elif c in _CLOSE:
                depth -= 1
            elif c == "," and depth == 1:
                args.append(stripped[start:i])
                start = i + 1
            i += 1
        if depth:
            continue  # unbalanced: not a call this scan can read
        last = stripped[start:i - 1]
        if args or last.strip():
            args.append(last)
        yield m.group(1), [squeeze(a) for a in args], squeeze(stripped[m.start():i])


def violations(src: str):
    """[(stripped call text, what is wrong)] of one source text."""
    bad = []
    for name, args, text in calls(strip_source(src)):
        if name in SYNC_NULL:
            bad.append((text, f"{name} is synchronous on the null stream"))
            continue
        if name in STREAM_ARG:
            pos = STREAM_ARG[name]
        elif name.endswith("Async"):
            pos = ASYNC_ARITY.get(name, len(args)) - 1
        else:
            continue
        if pos >= len(args):
            bad.append((text, f"{name} leaves its stream argument to the default, the null stream"))
        elif args[pos] in NULL_STREAMS:
            bad.append((text, f"{name} on the literal null stream {args[pos]}"))
    return bad


def _sources():
    files = sorted(f for ext in ("cpp", "hip", "hpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 8, f"the HIP sources are not where the lint looks: {CSRC}"
    return files


def test_no_null_stream_work_in_the_hip_sources():
    found, used = [], set()
    for path in _sources():
        with open(path, encoding="utf-8") as f:
            src = f.read()
        for text, why in violations(src):
            key = (os.path.basename(path), text)
            if key in ALLOW:
                used.add(key)
            else:
                found.append(f"{key[0]}: {why}: {text}")
    assert not found, "work on the null stream (use the context's stream):\n  " + "\n  ".join(found)
    stale = sorted(set(ALLOW) - used)
    assert not stale, f"allow-list entries that match no call any more: {stale}"


def test_the_scan_reads_launches_and_waits():
    """The scan is only worth its verdict if it sees the calls: every translation unit's launches."""
    seen = {}
    for path in _sources():
        with open(path, encoding="utf-8") as f:
            for name, args, _ in calls(strip_source(f.read())):
                seen[name] = seen.get(name, 0) + 1
                if name == "hipLaunchKernelGGL":
                    assert len(args) >= 5, f"{os.path.basename(path)}: a launch with {len(args)} arguments"
    assert seen.get("hipLaunchKernelGGL", 0) >= 100
    assert seen.get("hipMemsetAsync", 0) >= 5 and seen.get("hipMemcpyAsync", 0) >= 20
    assert seen.get("hipStreamWaitEvent", 0) >= 5 and seen.get("hipEventRecord", 0) >= 5


def test_the_lint_checks_itself():
    null_memset = """
        int ensure(ctx_t* ctx) {
            HIP_TRY(hipMemset(ctx->ws, 0, 256));  // hipMemsetAsync(ctx->ws, 0, 256, ctx->stream) was meant
            return 0;
        }"""
    got = violations(null_memset)
    assert [t for t, _ in got] == ["hipMemset(ctx->ws,0,256)"] and "synchronous" in got[0][1]

    null_async = "void f(void* p, size_t n) {\n    (void)hipMemsetAsync(p, 0,\n        n, 0);\n}"
    got = violations(null_async)
    assert [t for t, _ in got] == ["hipMemsetAsync(p,0,n,0)"] and "literal null stream" in got[0][1]

    clean = """
        /* hipMemset(p, 0, n) would be wrong here */
        const char* hint = "never hipMemcpy(dst, src, n, kind) \\" hipDeviceSynchronize()";
        HIP_TRY(hipMemsetAsync(ctx->ws, 0, 256, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dst, src, f(a, b), hipMemcpyDeviceToHost, c->stream));
        hipLaunchKernelGGL((k_sum<8, O>), dim3(grid), dim3(256), 0, st, pl, P,
                           stride, out, n, 0);
        HIP_TRY(hipEventRecord(ev, c->stream));
        HIP_TRY(hipStreamWaitEvent(side, ev, 0));
        HIP_TRY(hipStreamSynchronize(c->stream));"""
    assert violations(clean) == []

    # the other shapes of the same mistake
    assert len(violations("hipLaunchKernelGGL(k, dim3(g), dim3(256), 0, 0, a, b);")) == 1
    assert len(violations("hipLaunchKernelGGL((k<1, 2>), dim3(g),\n dim3(256), lds,\n nullptr, a);")) == 1
    assert len(violations("hipEventRecord(ev);")) == 1
    assert len(violations("hipEventRecord(ev, NULL);")) == 1
    assert len(violations("hipStreamWaitEvent(hipStreamDefault, ev, 0);")) == 1
    assert len(violations("hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice);")) == 1
    assert len(violations("hipMemcpy2DAsync(h, w, p, s, w, P, hipMemcpyDeviceToHost, (hipStream_t)0);")) == 1
    assert len(violations("hipDeviceSynchronize();")) == 1
    assert violations("hipMemcpy2DAsync(h, w, p, s, w, P, hipMemcpyDeviceToHost, c->stream);") == []
