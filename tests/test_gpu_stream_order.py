"""Stream ordering of every device entry, made deterministic with a delay (DESIGN.md "Stream-ordering
contract").

The parity files run on torch's legacy default stream, where a producer ahead of a call and a consumer
behind it are ordered with the library implicitly.  Here the context sits on a non-blocking
torch.cuda.Stream, as under a DDP comm hook, and a calibrated torch.cuda._sleep holds one stream
busy while the call is made, so a mis-ordered operation gives a wrong answer against the oracle on
every run:

A (slow producer, immediate consumer), all on a fresh stream S: the inputs hold stale but valid data
  (another dataset of the same shape; for sparse keys another ascending key set of the same length),
  the outputs a stale valid result (the same call made on the stale data).  Queued on S: the sleep,
  the copies of the fresh data into the inputs and of the stale result back over the outputs, the
  library call, clones of the outputs.  Internal work not ordered after S runs during the sleep: it
  reads the stale input, and what it writes is overwritten by the stale result.  Work not joined
  back into S is missed by the clones.  The clones are compared with the oracle's result for the
  fresh data, field by field as the parity files do.
B (busy null stream, fresh context, recycled memory): 256 MiB of 0xFF released to HIP, the sleep on
  the legacy default stream, then on S a new Context (every workspace, scratch slot, side context,
  event and pinned buffer a first use) and the call.  Anything the library sends to the null stream
  lands after the kernels that depend on it.

A test never passes because the delay was too short: the delayed stream is asserted busy before
each call, and after it for entries that do not synchronise the host; a failure of those assertions
says "calibration failure".  The oracle is the only reference; all device work goes through
libskml.so.  tests/test_stream_lint.py is the static side of the same contract.
"""
import ctypes as C
import functools
import time
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

# The delay: 20 x the longest host-side duration of one library call of this file on an idle stream,
# and not less than 20 ms.  Measured on an MI355X over four runs of this file: the longest call is
# skml_dense_encode_batch_f32 on a fresh context (it creates the side context and its high-priority
# stream), 6.4 to 10.4 ms; next skml_dense_encode_f32 3.3 ms, skml_sparse_encode_kv_f32 2.5 ms, the
# host entries 1.5 ms, everything else under 1 ms.  20 x 10.4 ms = 208 ms.  The module fixture prints
# the figures of each run (pytest -s).
LONGEST_CALL_MS = 10.4
DELAY_MS = 210.0
assert DELAY_MS >= max(20.0, 20 * LONGEST_CALL_MS)
CALIB = "calibration failure (the delay is too short for this machine; not an ordering result)"

N_BASE = 16384 + 20 * 256 + 100   # one full leaf tile, one partial tile, a tail
N_PAR = 4 * 16384 + 300
N_BUCKET = 3 * 16384 + 300
N_SUM = 40005
N_REF = 7000
BINS = 256
MAGIC = 0x444D4B53
DIM = 200003
GROUPS, ROWS, RATIO = 8, 2, 0.3


def _L():
    from sketchml_amd import _lib
    return _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _params(bins=BINS, seed=0, dedup=1):
    L = _L()
    p = L.Params()
    L.lib.skml_params_default(C.byref(p))
    p.bin_num, p.seed, p.dedup = bins, seed, dedup
    return p


def _sparse_params(seed, hash_seed, bins=BINS):
    from sketchml_amd.sparse import _params as sp
    return sp(bins, GROUPS, ROWS, RATIO, seed, hash_seed)


def _payload_buf(n, bins=BINS):
    from sketchml_amd.context import alloc_aligned
    nb = _L().lib.skml_dense_payload_bytes(n, bins)
    return alloc_aligned(nb, "cuda").zero_(), nb


# --------------------------------------------------------------------------------------------
# the delay and the two patterns
# --------------------------------------------------------------------------------------------
class _Delay:
    """torch.cuda._sleep scaled to DELAY_MS (one _sleep timed with two events), the record of the
    library calls' host-side durations on an idle stream, and the call wrapper that keeps it."""

    def __init__(self):
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        probe = 4000000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        self.cycles_per_ms = probe / a.elapsed_time(b)
        self.cycles = int(DELAY_MS * self.cycles_per_ms)
        a.record()
        torch.cuda._sleep(self.cycles)
        b.record()
        b.synchronize()
        self.delay_ms = a.elapsed_time(b)
        assert self.delay_ms >= 0.8 * DELAY_MS, f"{CALIB}: a sleep scaled to {DELAY_MS} ms took {self.delay_ms:.2f} ms"
        self.idle = False
        self.calls = []  # (entry, ms): host-side duration of a call made on an idle stream
        self.token = torch.zeros(64, device="cuda")
        self.shared_queue = 0  # pool streams found to run behind the null stream (independent_stream)
        self.held = []  # pattern-B calls of host-synchronising entries that returned with the null stream drained

    def sleep(self):
        torch.cuda._sleep(self.cycles)  # on torch's current stream

    def independent_stream(self):
        """A pool stream on which a new context does not wait for the legacy null stream.  Observed on
        the MI355X (not derived from the library's code): on about one torch pool stream in four, the
        creation of a context -- its first copy and stream synchronisation -- returns only when the
        null stream has drained, although a kernel of that stream runs beside the null stream's.
        The supposed cause is that a process has fewer hardware queues (GPU_MAX_HW_QUEUES) than
        streams, so some non-blocking streams share the null stream's queue and their markers wait
        for what is queued ahead of them there; this was not measured directly.  On such a stream
        pattern B could show nothing, so it departs from "a fresh torch.cuda.Stream()": each candidate
        is tried with a short sleep on the null stream and a throw-away context, and one that held
        its creator up for half of that sleep is passed over.  A product context bound to such a
        stream still stalls behind the null stream; no change of the library avoids that."""
        from sketchml_amd.context import Context
        d = torch.cuda.default_stream()
        probe_ms = 4.0
        for _ in range(64):
            S = torch.cuda.Stream()
            torch.cuda.synchronize()
            torch.cuda._sleep(int(probe_ms * self.cycles_per_ms))
            t0 = time.perf_counter()
            with torch.cuda.stream(S):
                ctx = Context(0)
            held = (time.perf_counter() - t0) * 1e3
            independent = held < probe_ms / 2 and not d.query()
            d.synchronize()
            del ctx
            if independent:
                return S
            self.shared_queue += 1
        raise AssertionError(f"{CALIB}: every pool stream runs behind the null stream")

    def c(self, name, *args):
        """One library call; the status must be SKML_OK."""
        L = _L()
        fn = getattr(L.lib, name)
        t0 = time.perf_counter()
        st = fn(*args)
        ms = (time.perf_counter() - t0) * 1e3
        if self.idle:
            self.calls.append((name, ms))
        assert st == 0, f"{name}: status {st}: {L.last_error()}"


@pytest.fixture(scope="module")
def sl(gpu):
    d = _Delay()
    yield d
    if d.calls:
        name, ms = max(d.calls, key=lambda t: t[1])
        print(f"\nstream-order calibration: {len(d.calls)} idle-stream calls, the longest {ms:.3f} ms ({name}); "
              f"delay {DELAY_MS} ms (measured {d.delay_ms:.2f} ms, {d.cycles_per_ms:.0f} cycles/ms) = "
              f"{DELAY_MS / ms:.1f} x the longest call; {d.shared_queue} candidate streams shared the null stream's queue")
        worst = {}
        for n_, m_ in d.calls:
            worst[n_] = max(worst.get(n_, 0.0), m_)
        for n_, m_ in sorted(worst.items(), key=lambda t: -t[1])[:14]:
            print(f"    {n_}: {m_:.3f} ms")
        print(f"    pattern-B calls held until the null stream drained: {d.held}")
        if ms > DELAY_MS / 20:
            warnings.warn(f"the longest idle-stream call, {name} {ms:.2f} ms, is more than DELAY_MS / 20: re-measure LONGEST_CALL_MS")
        # the busy assertions guard each case; this keeps the constant from going stale unnoticed
        assert ms <= DELAY_MS / 10, f"{CALIB}: {name} took {ms:.2f} ms on an idle stream, the delay is under 10 x that"


@pytest.fixture(autouse=True)
def _drain(gpu):
    """Nothing sleeps into the next test, whatever a comparison raised."""
    yield
    torch.cuda.synchronize()


def _busy(stream, when):
    assert not stream.query(), f"{CALIB}: the delayed stream had drained {when}"


def run_a(sl, inputs, call, outputs, scribble=(), host_sync=False, completes=False, ctx=None, warm=True):
    """Pattern A.  inputs: [(device tensor holding stale data, device-resident fresh data)]; call(h)
    makes the library call(s) with context handle h; outputs(): the tensors to clone afterwards;
    scribble: output tensors that exist before the call (their stale result is copied back over them
    behind the sleep).  host_sync: the entry synchronises the host, so the stream need not be busy
    when it returns; completes: it must have drained the stream (the sparse entries).  The warm-up
    is the same call on the stale data: it leaves the stale valid result in the outputs and sizes
    the context's buffers, so the delayed call frees nothing (hipFree waits for the device)."""
    from sketchml_amd.context import get_context
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        h = (ctx or get_context()).handle
        if warm:
            sl.idle = True
            try:
                call(h)
            finally:
                sl.idle = False
            S.synchronize()
        stale = [t.clone() for t in scribble]
        S.synchronize()
        sl.sleep()
        for t, f in inputs:
            t.copy_(f, non_blocking=True)
        for t, s in zip(scribble, stale):
            t.copy_(s, non_blocking=True)
        _busy(S, "before the library call")
        call(h)
        if completes:
            assert S.query(), "a sparse entry returned with device work still queued on its stream (BlockPool invariant)"
        elif not host_sync:
            _busy(S, "when the library call returned")
        got = [o.clone() for o in outputs()]
    S.synchronize()
    return got


def run_b(sl, call, outputs=lambda: [], host_sync=False):
    """Pattern B.  Returns (clones, the fresh context): the caller compares, the default stream is
    synchronised only afterwards (by _drain).  host_sync: the entry synchronises the host, and the
    HIP runtime may then hold it until the null stream drains (a copy into or out of pageable host
    memory whose pages it has not registered yet waits for the null stream), so the null stream
    need not be busy any more when it returns."""
    from sketchml_amd.context import Context
    torch.cuda.synchronize()
    junk = torch.full((256 << 20,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    del junk
    torch.cuda.empty_cache()
    d = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == d
    S = sl.independent_stream()
    t0 = time.perf_counter()
    sl.sleep()
    with torch.cuda.stream(S):
        ctx = Context(0)
        assert (time.perf_counter() - t0) * 1e3 < DELAY_MS / 2, f"{CALIB}: creating the context took half of the delay"
        _busy(d, "before the library call")
        sl.idle, mark = True, len(sl.calls)
        try:
            call(ctx.handle)
        finally:
            sl.idle = False
        if d.query():
            # held until the null stream drained (allowed for a host-synchronising entry only): what it
            # queued after that point was not raced against the null stream.  Kept on record per test.
            names = sorted({n_ for n_, _ in sl.calls[mark:]})
            sl.held.append(names)
            warnings.warn(f"pattern B: {names} returned only when the null stream had drained", stacklevel=2)
            del sl.calls[mark:]  # no idle-stream duration
        if not host_sync:
            _busy(d, "when the library call returned")
        got = [o.clone() for o in outputs()]
    S.synchronize()
    return got, ctx


def run(sl, pattern, inputs, call, outputs, **kw):
    """Pattern A (kw: run_a's), or pattern B with the inputs already holding the fresh data.  Returns
    (clones, the fresh context of pattern B or None)."""
    if pattern == "A":
        return run_a(sl, inputs, call, outputs, **kw), None
    for t, f in inputs:
        t.copy_(f)
    return run_b(sl, call, outputs, host_sync=kw.get("host_sync", False) or kw.get("completes", False))


# --------------------------------------------------------------------------------------------
# data and oracle results: computed once, shared, never modified
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense(kind, n, which, tag=0):
    """Dataset `which` (0 fresh, 1 stale) as (the device dtype's host tensor, the values as doubles).
    The stale set is another distribution, so its header, splits and bins all differ."""
    rng = np.random.default_rng(7919 * which + 31 * tag + n)
    x = rng.standard_normal(n) if which == 0 else 3.0 * rng.standard_normal(n) + 1.0
    if kind == "f64":
        return torch.from_numpy(x), x
    t = torch.from_numpy(x.astype(np.float32))
    if kind in ("bf16", "f16"):
        t = t.to(torch.bfloat16 if kind == "bf16" else torch.float16)
    return t, t.float().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _oq(kind, n, mode, seed, tag=0):
    xd = _dense(kind, n, 0, tag)[1]
    if mode == "quantile":
        return O.quantize(xd, BINS, seed)
    if mode == "uniform":
        return O.uniform_quantize(xd, BINS)
    return O.parallel_quantize(xd, BINS, threads=int(mode[1:]), seed=seed)  # "T4": parallelQuantize, 4 slices


def _pair(kind, n, tag=0):
    """(input tensor on the device holding the stale set, the fresh set on the device)."""
    return _dense(kind, n, 1, tag)[0].cuda(), _dense(kind, n, 0, tag)[0].cuda()


@functools.lru_cache(maxsize=None)
def _sparse_case(wide, seed, dim=DIM, density=0.2):
    """(fresh keys, fresh values, stale keys, stale values, oracle of the fresh pair)."""
    rng = np.random.default_rng(seed)
    fk = np.nonzero(rng.random(dim) < density)[0].astype(np.int32)
    fv = rng.standard_normal(len(fk))
    sk = np.sort(rng.choice(dim, len(fk), replace=False)).astype(np.int32)
    sv = 3.0 * rng.standard_normal(len(fk)) + 1.0
    if not wide:
        fv, sv = fv.astype(np.float32), sv.astype(np.float32)
    osp = O.sparse_compress(fk, fv.astype(np.float64), BINS, GROUPS, ROWS, RATIO, seed, seed + 1)
    return fk, fv, sk, sv, osp


@functools.lru_cache(maxsize=None)
def _dense_gradient(which, dim=3 * 65536 + 77, density=0.1):
    rng = np.random.default_rng(50 + which)
    x = np.where(rng.random(dim) < density, rng.standard_normal(dim) * (1 + 2 * which), 0.0).astype(np.float32)
    x[rng.random(dim) < 0.001] = np.float32(1e-8)  # not > 1e-8 in double: dropped
    return x


@functools.lru_cache(maxsize=None)
def _dense_gradient_oracle():
    keys, vals = O.to_sparse(_dense_gradient(0).astype(np.float64))
    return keys, vals, O.sparse_compress(keys, vals, BINS, GROUPS, ROWS, RATIO, 4, 9)


@functools.lru_cache(maxsize=None)
def _delta_keys(which):
    rng = np.random.default_rng(5 + which)  # the "mixed" gaps of tests/test_gpu_sparse.py
    gaps = np.where(rng.random(70000) < 0.9, rng.integers(1, 8, 70000), rng.integers(1, 1 << 16, 70000))
    return np.cumsum(gaps).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _delta_oracle():
    return O.delta_encode(_delta_keys(0))


# --------------------------------------------------------------------------------------------
# comparisons (as the parity files make them), on clones
# --------------------------------------------------------------------------------------------
def _unpack_codes(codes, bits, count):
    """Bins from a payload's packed codes (code_bits per element, LSB-first; include/skml.h)."""
    if bits == 8:
        return codes[:count].astype(np.int32)
    if bits == 16:
        return codes[: 2 * count].view(np.uint16).astype(np.int32)
    per = 8 // bits
    shifts = (np.arange(per, dtype=np.uint8) * bits)[None, :]
    out = (codes[: (count + per - 1) // per, None] >> shifts) & np.uint8((1 << bits) - 1)
    return out.reshape(-1)[:count].astype(np.int32)


def _parse(pl):
    """(header, splits, bins) of a dense payload's bytes, on the host."""
    b = pl.cpu().numpy()
    h = _L().DenseHeader.from_buffer_copy(b[:64].tobytes())
    assert h.magic == MAGIC, f"the payload has no finished header (magic {h.magic:#x}): unfinished or skipped summary"
    assert h.status == 0, f"payload status {h.status}"
    sp = np.frombuffer(b[64: 64 + 8 * (h.bin_num - 1)].tobytes(), dtype=np.float64)
    codes = b[h.codes_offset: h.codes_offset + (h.n * h.code_bits + 7) // 8]
    return h, sp, _unpack_codes(codes, h.code_bits, h.n)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_payload(pl, n, oq, bins=None):
    h, sp, got = _parse(pl)
    assert (h.n, h.bin_num, h.zero_idx) == (n, oq.bin_num, oq.zero_idx)
    assert np.array_equal(_bits64([h.min, h.max]), _bits64([oq.min, oq.max]))
    assert sp.shape == oq.splits.shape and np.array_equal(_bits64(sp), _bits64(oq.splits))
    assert np.array_equal(got, oq.bins if bins is None else bins)


def _tbits(t):
    """Bit patterns of a tensor's elements."""
    t = t.cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def _decoded(oq_values, bins, dtype):
    """values[bins] as the decode of that dtype gives it: the doubles, their fp32 rounding, or that
    rounded to the 16-bit type by torch on the CPU (nearest even)."""
    v = oq_values[bins]
    if dtype == torch.float64:
        return torch.from_numpy(v)
    return torch.from_numpy(v.astype(np.float32)).to(dtype)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    g, w = _tbits(got), _tbits(want)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{bad.size} of {g.size} values differ from the oracle, first at {int(bad[0])}"


def _sparse_payload(handle, ctx=None):
    """A SparsePayload over a raw handle whose calls go through `ctx` (default: the shared context)."""
    from sketchml_amd.sparse import SparsePayload
    pl = SparsePayload(handle, 0, ROWS)
    if ctx is not None:
        pl._ctx = lambda: ctx
    return pl


def _check_sparse_payload(pl, osp):
    """Quantizer header and splits, then every group's table, interval choice, bit lengths and
    flag / delta words (tests/test_gpu_sparse.py::_check_sparse)."""
    hdr, splits = pl.quant_header()
    assert hdr.bin_num == osp.q.bin_num and hdr.zero_idx == osp.q.zero_idx
    assert hdr.min == osp.q.min and hdr.max == osp.q.max
    assert np.array_equal(_bits64(splits), _bits64(osp.q.splits))
    for g in range(GROUPS):
        gg = pl.group(g)
        assert gg["size"] == osp.group_size[g], g
        if osp.tables[g] is None:
            assert gg["size"] == 0
            continue
        assert gg["col_num"] == osp.col_num[g]
        assert gg["hash_ids"] == list(osp.hash_ids[g])
        assert np.array_equal(gg["table"], osp.tables[g]), g
        d = osp.deltas[g]
        assert gg["num_intervals"] == d["num_intervals"] and gg["flag_kind"] == d["flag_kind"]
        assert gg["n_flag_bits"] == d["n_flag_bits"] and gg["n_delta_bits"] == d["n_delta_bits"]
        assert np.array_equal(gg["flag_words"], d["flag_words"]), g
        assert np.array_equal(gg["delta_words"], d["delta_words"]), g


def _check_restored(rk, rv, osp, n):
    ok, ob = osp.restore()
    assert len(ok) == n and np.array_equal(rk.cpu().numpy()[:n], ok)
    if rv.dtype == torch.int32:
        assert np.array_equal(rv.cpu().numpy()[:n], ob)
    else:
        _same(rv[:n], _decoded(osp.q.values(), ob, rv.dtype))


# --------------------------------------------------------------------------------------------
# dense encodes
# --------------------------------------------------------------------------------------------
ENCODES = {"f32": ("skml_dense_encode_f32", "f32", "quantile"), "f64": ("skml_dense_encode_f64", "f64", "quantile"),
           "bf16": ("skml_dense_encode_bf16", "bf16", "quantile"), "f16": ("skml_dense_encode_f16", "f16", "quantile"),
           "uniform_f32": ("skml_dense_encode_uniform_f32", "f32", "uniform"),
           "uniform_f64": ("skml_dense_encode_uniform_f64", "f64", "uniform")}


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("entry", list(ENCODES))
def test_dense_encode(gpu, sl, entry, pattern):
    fn, kind, mode = ENCODES[entry]
    n = N_BASE
    x, fresh = _pair(kind, n)
    pl, nb = _payload_buf(n)
    p = _params(BINS, 7)
    (got,), _ = run(sl, pattern, [(x, fresh)], lambda h: sl.c(fn, h, _ptr(x), n, C.byref(p), _ptr(pl), nb),
                    lambda: [pl], scribble=[pl])
    _check_payload(got, n, _oq(kind, n, mode, 7))


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_dense_encode_parallel(gpu, sl, pattern):
    """parallelQuantize with 4 slice sketches merged in slice order (no Maths.unique)."""
    n = N_PAR
    x, fresh = _pair("f32", n)
    pl, nb = _payload_buf(n)
    p = _params(BINS, 11, dedup=0)
    kw = dict(scribble=[pl])
    (got,), _ = run(sl, pattern, [(x, fresh)],
                    lambda h: sl.c("skml_dense_encode_parallel_f32", h, _ptr(x), n, 4, C.byref(p), _ptr(pl), nb),
                    lambda: [pl], **kw)
    _check_payload(got, n, _oq("f32", n, "T4", 11))


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_dense_encode_sharded_pair(gpu, sl, pattern):
    """sketch_shard -> quantize_sharded for two shards on one GPU, the four calls back to back: both
    shards' bins against parallelQuantize with T = 2 over the whole gradient."""
    from sketchml_amd import distributed as D
    L = _L()
    n = N_PAR
    sizes = D.parallel_slices(n, 2)
    offs = [0, sizes[0], n]
    stale, fresh = _dense("f32", n, 1)[0], _dense("f32", n, 0)[0]
    xs = [stale[offs[r]:offs[r + 1]].cuda() for r in range(2)]       # one tensor per shard, as on two ranks
    fr = [fresh[offs[r]:offs[r + 1]].cuda() for r in range(2)]
    rb = D.record_bytes(False)
    assert rb % 16 == 0
    recs = torch.zeros(2 * rb, dtype=torch.uint8, device="cuda")
    bufs = [_payload_buf(sizes[r]) for r in range(2)]
    p = _params(BINS, 9, dedup=0)
    sz = (C.c_int64 * 2)(*sizes)

    def call(h):
        for r in range(2):
            sl.c("skml_dense_sketch_shard_f32", h, _ptr(xs[r]), sizes[r], sz, 2, r, 9, C.c_void_p(recs.data_ptr() + r * rb))
        for r in range(2):
            sl.c("skml_dense_encode_sharded_f32", h, _ptr(xs[r]), sizes[r], sz, 2, r, _ptr(recs), C.byref(p),
                 _ptr(bufs[r][0]), bufs[r][1])

    outs = [recs, bufs[0][0], bufs[1][0]]
    kw = dict(scribble=outs)
    got, _ = run(sl, pattern, list(zip(xs, fr)), call, lambda: outs, **kw)
    oq = _oq("f32", n, "T2", 9)
    assert L.lib.skml_sketch_record_bytes(0) == rb
    for r in range(2):
        _check_payload(got[1 + r], sizes[r], oq, bins=oq.bins[offs[r]:offs[r + 1]])


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("shape", ["four_buckets", "tiny_first_bucket"])
def test_dense_encode_batch(gpu, sl, shape, pattern):
    """The batched encode's two lanes.  four_buckets: both lanes take two buckets.  tiny_first_bucket:
    bucket 0 has no leaf (n < 256), so the event that starts lane 1 is recorded by hand.  Pattern B
    is the deterministic form of the round-6 race (a fresh side workspace's arrival counter zeroed
    on the null stream): see test_gpu_configs.py::test_batch_encode_fresh_side_lane_on_recycled_memory."""
    ns = [N_BUCKET] * 4 if shape == "four_buckets" else [100, N_BUCKET, N_BUCKET]
    P = len(ns)
    pairs = [_pair("f32", ns[i], tag=i + 1) for i in range(P)]  # stale data in every bucket
    bufs = [_payload_buf(ns[i]) for i in range(P)]
    p = _params(BINS, 6)
    ptrs = (C.c_void_p * P)(*[x.data_ptr() for x, _ in pairs])
    pptr = (C.c_void_p * P)(*[b.data_ptr() for b, _ in bufs])
    nn = (C.c_int64 * P)(*ns)
    caps = (C.c_size_t * P)(*[nb for _, nb in bufs])
    outs = [b for b, _ in bufs]
    kw = dict(scribble=outs)
    got, _ = run(sl, pattern, pairs, lambda h: sl.c("skml_dense_encode_batch_f32", h, P, ptrs, nn, C.byref(p), pptr, caps),
                 lambda: outs, **kw)
    for i in range(P):
        _check_payload(got[i], ns[i], _oq("f32", ns[i], "quantile", 6, tag=i + 1))


def test_dense_encode_with_splits(gpu, sl):
    """Pattern A; the entry synchronises the host (its staged splits are reused by later calls)."""
    n = N_BASE
    x, fresh = _pair("f32", n)
    oq = _oq("f32", n, "quantile", 7)
    sp = np.ascontiguousarray(oq.splits)
    pl, nb = _payload_buf(n, len(sp) + 1)
    L = _L()
    got = run_a(sl, [(x, fresh)],
                lambda h: sl.c("skml_dense_encode_with_splits_f32", h, _ptr(x), n, sp.ctypes.data_as(L.dblp), len(sp),
                               oq.min, oq.max, _ptr(pl), nb), lambda: [pl], scribble=[pl], host_sync=True)
    _check_payload(got[0], n, oq)


# --------------------------------------------------------------------------------------------
# dense decodes
# --------------------------------------------------------------------------------------------
DECODES = {"f32": ("skml_dense_decode_f32", torch.float32), "f64": ("skml_dense_decode_f64", torch.float64),
           "bf16": ("skml_dense_decode_bf16", torch.bfloat16), "f16": ("skml_dense_decode_f16", torch.float16),
           "bins": ("skml_dense_bins_i32", torch.int32)}


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("entry", list(DECODES))
def test_dense_decode(gpu, sl, entry, pattern):
    """A: the payload comes from an encode queued on S behind the sleep, the decode follows with no
    synchronisation.  B: a finished payload, decoded through a fresh context."""
    fn, dtype = DECODES[entry]
    n = N_BASE
    x, fresh = _pair("f32", n)
    pl, nb = _payload_buf(n)
    out = torch.zeros(n, dtype=dtype, device="cuda")
    p = _params(BINS, 7)

    def encode(h):
        sl.c("skml_dense_encode_f32", h, _ptr(x), n, C.byref(p), _ptr(pl), nb)

    def decode(h):
        sl.c(fn, h, _ptr(pl), _ptr(out), n)

    if pattern == "A":
        (got,) = run_a(sl, [(x, fresh)], lambda h: (encode(h), decode(h)), lambda: [out], scribble=[pl, out])
    else:
        from sketchml_amd.context import get_context
        x.copy_(fresh)
        encode(get_context().handle)
        (got,), _ = run_b(sl, decode, lambda: [out])
    oq = _oq("f32", n, "quantile", 7)
    if entry == "bins":
        assert np.array_equal(got.cpu().numpy(), oq.bins)
    else:
        _same(got, _decoded(oq.values(), oq.bins, dtype))


def test_dense_times_by_then_decode(gpu, sl):
    """Pattern A: encode, timesBy (the payload edited in place on the stream), decode, back to back."""
    n = N_BASE
    x, fresh = _pair("f32", n)
    pl, nb = _payload_buf(n)
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    p = _params(BINS, 7)

    def call(h):
        sl.c("skml_dense_encode_f32", h, _ptr(x), n, C.byref(p), _ptr(pl), nb)
        sl.c("skml_dense_times_by", h, _ptr(pl), 0.25)
        sl.c("skml_dense_decode_f32", h, _ptr(pl), _ptr(out), n)

    got_pl, got = run_a(sl, [(x, fresh)], call, lambda: [pl, out], scribble=[pl, out])
    oq = _oq("f32", n, "quantile", 7)
    hdr = O.QuantHeader.from_buffer_copy(bytes(oq.hdr))  # the cached oracle result stays as it is
    O.lib().orc_times_by(C.byref(hdr), 0.25)
    scaled = O.OracleQuant(hdr, oq.bins)
    _check_payload(got_pl, n, scaled)
    _same(got, _decoded(scaled.values(), oq.bins, torch.float32))


@functools.lru_cache(maxsize=None)
def _sum_case(which):
    """P = 3 gathered payloads of N_SUM values of dataset `which` on the device (encoded once on the
    shared context), and for the fresh set the oracle's decodes summed in double in payload order."""
    from sketchml_amd.context import alloc_aligned, get_context
    L = _L()
    P, n = 3, N_SUM
    nb = L.lib.skml_dense_payload_bytes(n, BINS)
    stride = (nb + 255) // 256 * 256
    allp = alloc_aligned(stride * P, "cuda").zero_()
    acc = np.zeros(n, dtype=np.float64)
    for r in range(P):
        x = _dense("f32", n, which, tag=r + 1)[0].cuda()
        p = _params(BINS, r)
        assert L.lib.skml_dense_encode_f32(get_context().handle, _ptr(x), n, C.byref(p),
                                           C.c_void_p(allp.data_ptr() + r * stride), stride) == 0, L.last_error()
        torch.cuda.synchronize()
        if which == 0:
            oq = _oq("f32", n, "quantile", r, tag=r + 1)
            acc += oq.values()[oq.bins]
    return allp, stride, (acc * (1.0 / P)).astype(np.float32)


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("form", [0, 1], ids=["own_form", "per_payload_form"])
@pytest.mark.parametrize("entry", ["f32", "bf16"])
def test_dense_decode_sum(gpu, sl, entry, form, pattern):
    """A: the gathered buffer is filled by copies on S behind the sleep (as an all-gather leaves it).
    The entry reads the headers back first, so it synchronises the host."""
    L = _L()
    P, n = 3, N_SUM
    fresh, stride, want32 = _sum_case(0)
    dtype = torch.float32 if entry == "f32" else torch.bfloat16
    fn = "skml_dense_decode_sum_f32" if entry == "f32" else "skml_dense_decode_sum_bf16"
    allp = _sum_case(1)[0].clone()
    out = torch.zeros(n, dtype=dtype, device="cuda")
    with L.forced_forms(decode_sum=form):
        def call(h):
            sl.c(fn, h, _ptr(allp), P, stride, _ptr(out), n, 1.0 / P)

        if pattern == "A":
            (got,) = run_a(sl, [(allp, fresh)], call, lambda: [out], scribble=[out], host_sync=True)
        else:  # the header read-back goes through pinned staging: the entry must not wait for the null stream
            allp.copy_(fresh)
            (got,), _ = run_b(sl, call, lambda: [out])
    _same(got, torch.from_numpy(want32).to(dtype))


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_dense_write_read_object(gpu, sl, pattern):
    """Quantizer.writeObject / readObject: the field stream equals the oracle's byte for byte, and
    the payload read back from it carries the oracle's header, splits and bins.  A: the round trip
    follows an encode queued behind the sleep.  Both entries synchronise the host."""
    L = _L()
    n = N_REF
    x, fresh = _pair("f32", n)
    pl, nb = _payload_buf(n)
    back, _ = _payload_buf(n)
    p = _params(BINS, 3)
    oq = _oq("f32", n, "quantile", 3)
    want = oq.write_ref()
    buf = np.zeros(len(want) + 4096, dtype=np.uint8)  # the stale stream may be longer (more bins kept)
    wrote = C.c_size_t()

    def encode(h):
        sl.c("skml_dense_encode_f32", h, _ptr(x), n, C.byref(p), _ptr(pl), nb)

    def round_trip(h):
        sl.c("skml_dense_serialize_ref", h, _ptr(pl), buf.ctypes.data_as(L.u8p), buf.nbytes, C.byref(wrote))
        sl.c("skml_dense_deserialize_ref", h, buf.ctypes.data_as(L.u8p), wrote.value, _ptr(back), nb)

    if pattern == "A":
        (got,) = run_a(sl, [(x, fresh)], lambda h: (encode(h), round_trip(h)), lambda: [back], scribble=[pl, back],
                       host_sync=True)
    else:
        from sketchml_amd.context import get_context
        x.copy_(fresh)
        encode(get_context().handle)
        (got,), _ = run_b(sl, round_trip, lambda: [back], host_sync=True)
    assert buf[: wrote.value].tobytes() == want
    _check_payload(got, n, oq)


def test_dense_host_entries_on_a_fresh_context(gpu, sl):
    """Pattern B only (the host entries synchronise): a float[] in, payload bytes out, and back."""
    L = _L()
    n = N_REF
    xh = _dense("f32", n, 0)[0].numpy()
    oq = _oq("f32", n, "quantile", 3)
    p = _params(BINS, 3)
    cap = L.lib.skml_dense_payload_bytes(n, BINS)
    pl = np.zeros(cap, dtype=np.uint8)
    wrote = C.c_size_t()
    _, ctx = run_b(sl, lambda h: sl.c("skml_dense_encode_host_f32", h, xh.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                      pl.ctypes.data_as(C.c_void_p), cap, C.byref(wrote)), host_sync=True)
    _check_payload(torch.from_numpy(pl[: wrote.value]), n, oq)
    torch.cuda.synchronize()
    dec = np.zeros(n, dtype=np.float32)
    _, ctx2 = run_b(sl, lambda h: sl.c("skml_dense_decode_host_f32", h, pl.ctypes.data_as(C.c_void_p), wrote.value,
                                       dec.ctypes.data_as(C.c_void_p), n), host_sync=True)
    _same(torch.from_numpy(dec), _decoded(oq.values(), oq.bins, torch.float32))


# --------------------------------------------------------------------------------------------
# sparse entries
# --------------------------------------------------------------------------------------------
def _sp_encode(sl, h, k, v, p, ctx=None):
    out = C.c_void_p()
    fn = "skml_sparse_encode_kv_f64" if v.dtype == torch.float64 else "skml_sparse_encode_kv_f32"
    sl.c(fn, h, _ptr(k), _ptr(v), k.numel(), C.byref(p), C.byref(out))
    return _sparse_payload(out, ctx)


def _sp_restore(sl, h, pl, rk, rv):
    fn = {torch.float32: "skml_sparse_decode_f32", torch.float64: "skml_sparse_decode_f64",
          torch.int32: "skml_sparse_restore_bins"}[rv.dtype]
    sl.c(fn, h, pl.handle, _ptr(rk), _ptr(rv))


def _sp_free(pl):
    _L().lib.skml_sparse_free(pl.handle)
    pl.handle = None


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("wide", [False, True], ids=["fp32_values", "fp64_values"])
def test_sparse_encode_restore(gpu, sl, wide, pattern):
    """encode_sparse, then restore and restore_bins, each call under the pattern on its own: the
    group tables and key streams, then the restored keys, values and bins, against O.sparse_compress."""
    seed = 21 + int(wide)
    fk, fv, sk, sv, osp = _sparse_case(wide, seed)
    n = len(fk)
    k, v = torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda()
    fkd, fvd = torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda()
    p = _sparse_params(seed, seed + 1)
    box = {}

    def encode(h, ctx=None):
        if box.get("pl") is not None:
            _sp_free(box["pl"])  # the warm-up's payload: its block goes back to the pool
        box["pl"] = _sp_encode(sl, h, k, v, p, ctx)

    vdt = torch.float64 if wide else torch.float32
    rk, rv = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=vdt, device="cuda")
    bk, bb = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    if pattern == "A":
        run_a(sl, [(k, fkd), (v, fvd)], encode, lambda: [], completes=True)
        pl = box["pl"]
        _check_sparse_payload(pl, osp)
        # restore: the stale result behind the sleep is the restore of a payload of the stale pair
        from sketchml_amd.context import get_context
        stale_pl = _sp_encode(sl, get_context().handle, torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda(), p)
        for outs in ((rk, rv), (bk, bb)):
            _sp_restore(sl, get_context().handle, stale_pl, *outs)
            torch.cuda.synchronize()
            got = run_a(sl, [], lambda h: _sp_restore(sl, h, pl, *outs), lambda: list(outs), scribble=list(outs),
                        completes=True, warm=False)
            _check_restored(got[0], got[1], osp, n)
    else:
        k.copy_(fkd)
        v.copy_(fvd)
        _, ctx = run_b(sl, encode, host_sync=True)
        pl = box["pl"]
        pl._ctx = lambda: ctx
        _check_sparse_payload(pl, osp)
        for outs in ((rk, rv), (bk, bb)):
            torch.cuda.synchronize()
            got, ctx_r = run_b(sl, lambda h: _sp_restore(sl, h, pl, *outs), lambda: list(outs), host_sync=True)
            _check_restored(got[0], got[1], osp, n)


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_to_sparse(gpu, sl, pattern):
    """DenseDoubleGradient.toSparse (|x| > 1e-8 compared in double): keys and values exact."""
    fresh_h, stale_h = _dense_gradient(0), _dense_gradient(1)
    dim = len(fresh_h)
    x, fresh = torch.from_numpy(stale_h).cuda(), torch.from_numpy(fresh_h).cuda()
    keys = torch.zeros(dim, dtype=torch.int32, device="cuda")
    vals = torch.zeros(dim, dtype=torch.float32, device="cuda")
    nnz = C.c_int64()
    kw = dict(scribble=[keys, vals], completes=True)
    (gk, gv), _ = run(sl, pattern, [(x, fresh)],
                      lambda h: sl.c("skml_sparse_compact_f32", h, _ptr(x), dim, _ptr(keys), _ptr(vals), C.byref(nnz)),
                      lambda: [keys, vals], **kw)
    want = np.nonzero(np.abs(fresh_h.astype(np.float64)) > 1e-8)[0]
    assert nnz.value == len(want)
    assert np.array_equal(gk.cpu().numpy()[: len(want)], want)
    assert np.array_equal(gv.cpu().numpy()[: len(want)].view(np.uint32), fresh_h[want].view(np.uint32))


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_encode_dense_as_sparse(gpu, sl, pattern):
    """SketchGradient.fromSparse after toSparse in one entry: the compaction's count comes back
    through the context's host word, the encode follows on the same stream."""
    fresh_h, stale_h = _dense_gradient(0), _dense_gradient(1)
    dim = len(fresh_h)
    x, fresh = torch.from_numpy(stale_h).cuda(), torch.from_numpy(fresh_h).cuda()
    keys, vals, osp = _dense_gradient_oracle()
    p = _sparse_params(4, 9)
    box = {}

    def call(h):
        if box.get("pl") is not None:
            _sp_free(box["pl"])
        out = C.c_void_p()
        sl.c("skml_sparse_encode_f32", h, _ptr(x), dim, C.byref(p), C.byref(out))
        box["pl"] = _sparse_payload(out)

    kw = dict(completes=True)
    _, ctx = run(sl, pattern, [(x, fresh)], call, lambda: [], **kw)
    pl = box["pl"]
    if ctx is not None:
        pl._ctx = lambda: ctx
    assert pl.nnz() == len(keys)
    _check_sparse_payload(pl, osp)
    rk, rv = pl.restore()
    torch.cuda.synchronize()
    _check_restored(rk, rv, osp, len(keys))


def _parse_sparse_stream(b):
    """Reader of skml_sparse_serialize's field stream (GroupedMinMaxSketch.writeObject order)."""
    import struct
    off = 0

    def take(fmt):
        nonlocal off
        v = struct.unpack_from(fmt, b, off)[0]
        off += struct.calcsize(fmt)
        return v

    head = dict(G=take(">i"), rows=take(">i"), ratio=take(">d"), B=take(">i"), zero=take(">i"))
    sketches, encoders = [], []
    for _ in range(head["G"]):
        if not take(">B"):
            sketches.append(None)
            continue
        sk = dict(rows=take(">i"), cols=take(">i"), zero=take(">i"))
        sk["hashes"] = [(take(">i"), take(">i"), take(">i")) for _ in range(sk["rows"])]
        sk["items"] = [(take(">i"), take(">i"), take(">i")) for _ in range(take(">i"))]
        sk["longs"] = np.array([take(">Q") for _ in range(take(">i"))], dtype=np.uint64)
        sk["size"] = take(">i")
        sketches.append(sk)
    for _ in range(head["G"]):
        if not take(">B"):
            encoders.append(None)
            continue
        e = dict(size=take(">i"), m=take(">i"), kind=bool(take(">B")))
        e["flags"] = np.array([take(">Q") for _ in range(take(">i"))], dtype=np.uint64)
        e["deltas"] = np.array([take(">Q") for _ in range(take(">i"))], dtype=np.uint64)
        encoders.append(e)
    assert off == len(b)
    return head, sketches, encoders


def _check_sparse_stream(data, osp):
    """tests/test_gpu_sparse.py::test_sparse_serialize_matches_oracle on one stream."""
    head, sketches, encoders = _parse_sparse_stream(data)
    assert (head["G"], head["rows"], head["ratio"], head["B"], head["zero"]) == \
        (GROUPS, ROWS, RATIO, osp.q.bin_num, osp.q.zero_idx)
    for g in range(GROUPS):
        if osp.tables[g] is None:
            assert sketches[g] is None and encoders[g] is None
            continue
        s = sketches[g]
        assert (s["rows"], s["cols"], s["zero"], s["size"]) == (ROWS, osp.col_num[g], osp.q.zero_idx, ROWS * osp.col_num[g])
        want = O.huffman_encode(osp.tables[g])
        assert s["items"] == [tuple(int(v) for v in it) for it in want["items"]]
        assert np.array_equal(s["longs"], want["words"])
        d, e = osp.deltas[g], encoders[g]
        assert (e["size"], e["m"], e["kind"]) == (d["size"], d["num_intervals"], d["flag_kind"])
        assert np.array_equal(e["flags"], d["flag_words"]) and np.array_equal(e["deltas"], d["delta_words"])


def test_sparse_export_import_restore_and_serialize(gpu, sl):
    """Pattern A on the payload of test_sparse_encode_restore: export into a buffer that holds another
    payload's blob (copied back over it behind the sleep), import of that blob and restore of the
    import with no synchronisation of the test's own; then the writeObject stream."""
    from sketchml_amd.context import get_context
    from sketchml_amd.sparse import SparsePayload
    fk, fv, sk, sv, osp = _sparse_case(False, 21)
    n = len(fk)
    p = _sparse_params(21, 22)
    h0 = get_context().handle
    pl = _sp_encode(sl, h0, torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda(), p)
    stale_pl = _sp_encode(sl, h0, torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda(), p)
    cap = (max(pl.export_bytes(), stale_pl.export_bytes()) + 255) // 256 * 256
    from sketchml_amd.context import alloc_aligned
    blob = alloc_aligned(cap, "cuda").zero_()
    stale_pl.export(blob)
    rk = torch.zeros(n, dtype=torch.int32, device="cuda")
    rv = torch.zeros(n, dtype=torch.float64, device="cuda")
    _sp_restore(sl, h0, stale_pl, rk, rv)
    torch.cuda.synchronize()
    box = {}

    def call(h):
        sl.c("skml_sparse_export", h, pl.handle, _ptr(blob), cap)
        out = C.c_void_p()
        sl.c("skml_sparse_import", h, _ptr(blob), pl.export_bytes(), C.byref(out))
        box["back"] = SparsePayload(out, 0, ROWS)
        _sp_restore(sl, h, box["back"], rk, rv)

    gk, gv = run_a(sl, [], call, lambda: [rk, rv], scribble=[blob, rk, rv], completes=True, warm=False)
    _check_restored(gk, gv, osp, n)
    _check_sparse_payload(box["back"], osp)
    data = {}

    def serialize(h):
        L = _L()
        need = C.c_size_t()
        sl.c("skml_sparse_serialize", h, pl.handle, None, 0, C.byref(need))
        buf = np.zeros(max(need.value, 1), dtype=np.uint8)
        sl.c("skml_sparse_serialize", h, pl.handle, buf.ctypes.data_as(L.u8p), need.value, C.byref(need))
        data["stream"] = buf[: need.value].tobytes()

    run_a(sl, [], serialize, lambda: [], completes=True, warm=False)
    _check_sparse_stream(data["stream"], osp)
    assert box["back"].serialize() == data["stream"]  # the import writes the same stream


@functools.lru_cache(maxsize=None)
def _sparse_sum_oracle():
    osps = [_sparse_case(False, 31 + r)[4] for r in range(3)]
    want, forms = O.gradient_sum(((k, osp.q.values()[b]) for osp in osps for k, b in [osp.restore()]), DIM, 1.0 / 3)
    return want, forms


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_sparse_decode_sum(gpu, sl, pattern):
    """Gradient.sum of P = 3 distinct payloads (the restores run on two lanes): the float64 sum of the
    oracle's restores in payload order, x 1/3.  A: the blobs are exported on S behind the sleep into
    slots that hold three other payloads' blobs; B: finished blobs, a fresh context."""
    from sketchml_amd.context import alloc_aligned, get_context
    P = 3
    h0 = get_context().handle
    pls, stales = [], []
    for r in range(P):
        fk, fv, sk, sv, _ = _sparse_case(False, 31 + r)
        p = _sparse_params(31 + r, 32 + r)
        pls.append(_sp_encode(sl, h0, torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda(), p))
        stales.append(_sp_encode(sl, h0, torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda(), p))
    stride = (max(q.export_bytes() for q in pls + stales) + 255) // 256 * 256
    allb = alloc_aligned(stride * P, "cuda").zero_()
    out = torch.zeros(DIM, dtype=torch.float64, device="cuda")
    for r, q in enumerate(stales if pattern == "A" else pls):
        q.export(allb[r * stride:(r + 1) * stride])
    torch.cuda.synchronize()

    def decode_sum(h):
        sl.c("skml_sparse_decode_sum_f64", h, _ptr(allb), P, stride, DIM, 1.0 / P, _ptr(out))

    if pattern == "A":
        decode_sum(h0)  # the stale sum, copied back over `out` behind the sleep
        torch.cuda.synchronize()

        def call(h):
            for r, q in enumerate(pls):
                sl.c("skml_sparse_export", h, q.handle, C.c_void_p(allb.data_ptr() + r * stride), stride)
            decode_sum(h)

        (got,) = run_a(sl, [], call, lambda: [out], scribble=[allb, out], completes=True, warm=False)
    else:
        (got,), _ = run_b(sl, decode_sum, lambda: [out], host_sync=True)
    want, forms = _sparse_sum_oracle()
    assert set(forms) == {"sparse"}
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))


def _trim(words, bits):
    """BitSet.toLongArray of a device word stream: up to the last non-zero word."""
    w = words.cpu().numpy().view(np.uint64)[: (bits + 63) // 64]
    nz = np.nonzero(w)[0]
    return w[: nz[-1] + 1] if len(nz) else w[:0]


def test_delta_adaptive_encode_decode(gpu, sl):
    """Pattern A for the standalone DeltaAdaptiveEncoder: 70,000 keys with mixed gaps."""
    keys_h, stale_h = _delta_keys(0), _delta_keys(1)
    n = len(keys_h)
    k, fresh = torch.from_numpy(stale_h).cuda(), torch.from_numpy(keys_h).cuda()
    cap = n + 2
    fw = torch.zeros(cap, dtype=torch.int64, device="cuda")
    dw = torch.zeros(cap, dtype=torch.int64, device="cuda")
    m, kind, nf, nd = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    gf, gd = run_a(sl, [(k, fresh)],
                   lambda h: sl.c("skml_delta_encode", h, _ptr(k), n, C.byref(m), C.byref(kind), C.byref(nf), C.byref(nd),
                                  _ptr(fw), _ptr(dw), cap), lambda: [fw, dw], scribble=[fw, dw], completes=True)
    want = _delta_oracle()
    assert (m.value, bool(kind.value), nf.value, nd.value) == (want["num_intervals"], want["flag_kind"],
                                                              want["n_flag_bits"], want["n_delta_bits"])
    flags, deltas = _trim(gf, nf.value), _trim(gd, nd.value)
    assert np.array_equal(flags, want["flag_words"]) and np.array_equal(deltas, want["delta_words"])
    # decode: the streams are copied into place behind the sleep, over the stale key set's streams
    from sketchml_amd.context import get_context
    sfw, sdw = torch.zeros_like(fw), torch.zeros_like(dw)
    sm, skind, snf, snd = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    stale_k = torch.from_numpy(stale_h).cuda()
    sl.c("skml_delta_encode", get_context().handle, _ptr(stale_k), n, C.byref(sm), C.byref(skind), C.byref(snf),
         C.byref(snd), _ptr(sfw), _ptr(sdw), cap)
    torch.cuda.synchronize()
    out = stale_k.clone()
    fw.copy_(sfw)
    dw.copy_(sdw)
    (got,) = run_a(sl, [(fw, gf), (dw, gd)],
                   lambda h: sl.c("skml_delta_decode", h, n, m.value, kind.value, _ptr(fw), len(flags), _ptr(dw),
                                  len(deltas), _ptr(out)), lambda: [out], scribble=[out], completes=True, warm=False)
    assert np.array_equal(got.cpu().numpy(), keys_h)
    assert np.array_equal(want["decoded"], keys_h)


# --------------------------------------------------------------------------------------------
# whole sequences
# --------------------------------------------------------------------------------------------
def _batch_args(pairs, bufs, ns):
    P = len(ns)
    return (P, (C.c_void_p * P)(*[x.data_ptr() for x, _ in pairs]), (C.c_int64 * P)(*ns),
            (C.c_void_p * P)(*[b.data_ptr() for b, _ in bufs]), (C.c_size_t * P)(*[nb for _, nb in bufs]))


def test_back_to_back_reuse_of_one_context(gpu, sl):
    """Pattern A on a new context, in two delayed phases.  Phase 1: two encodes of different sizes
    with no synchronisation between them, the second larger, so ensure_ws frees and regrows the
    workspace while the first is still queued.  That hipFree waits for the device: the second encode
    returns with the stream drained, so nothing after it in phase 1 could be mis-ordered.  Phase 2
    therefore re-arms the delay: the sleep, the fresh buckets and keys copied in, the stale batch
    results copied back over the payloads, then a batched encode and a sparse encode, which share the
    (new) side context through different event pairs, the stream asserted busy before each of them.
    Every result against its own oracle result."""
    from sketchml_amd.context import Context, get_context
    n1, n2 = N_BASE, 2**20 + 777
    x1, f1 = _pair("f32", n1)
    x2, f2 = _pair("f32", n2)
    (pl1, nb1), (pl2, nb2) = _payload_buf(n1), _payload_buf(n2)
    ns = [N_BUCKET] * 4
    pairs = [_pair("f32", N_BUCKET, tag=i + 1) for i in range(4)]
    bufs = [_payload_buf(N_BUCKET) for _ in range(4)]
    P, ptrs, nn, pptr, caps = _batch_args(pairs, bufs, ns)
    fk, fv, sk, sv, osp = _sparse_case(False, 21)
    k, v = torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda()
    fkd, fvd = torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda()
    p1, p2, p6, sp = _params(BINS, 7), _params(BINS, 5), _params(BINS, 6), _sparse_params(21, 22)
    # the stale valid batch result, made by the shared context: the new one stays unused until phase 1
    sl.c("skml_dense_encode_batch_f32", get_context().handle, P, ptrs, nn, C.byref(p6), pptr, caps)
    torch.cuda.synchronize()
    stale = [b.clone() for b, _ in bufs]
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        ctx = Context(0)
        h = ctx.handle
        sl.sleep()
        for t, f in [(x1, f1), (x2, f2)]:
            t.copy_(f, non_blocking=True)
        _busy(S, "before the first encode")
        sl.c("skml_dense_encode_f32", h, _ptr(x1), n1, C.byref(p1), _ptr(pl1), nb1)
        _busy(S, "when the first encode returned")
        sl.c("skml_dense_encode_f32", h, _ptr(x2), n2, C.byref(p2), _ptr(pl2), nb2)  # regrows: waits the sleep out
        got = [pl1.clone(), pl2.clone()]
        sl.sleep()
        for t, f in [(k, fkd), (v, fvd)] + pairs:
            t.copy_(f, non_blocking=True)
        for (b, _), st in zip(bufs, stale):
            b.copy_(st, non_blocking=True)
        _busy(S, "before the batched encode")
        sl.c("skml_dense_encode_batch_f32", h, P, ptrs, nn, C.byref(p6), pptr, caps)
        _busy(S, "when the batched encode returned")
        spl = _sp_encode(sl, h, k, v, sp, ctx)
        assert S.query(), "the sparse encode returned with device work still queued"
        got += [b.clone() for b, _ in bufs]
    S.synchronize()
    _check_payload(got[0], n1, _oq("f32", n1, "quantile", 7))
    _check_payload(got[1], n2, _oq("f32", n2, "quantile", 5))
    for i in range(4):
        _check_payload(got[2 + i], N_BUCKET, _oq("f32", N_BUCKET, "quantile", 6, tag=i + 1))
    _check_sparse_payload(spl, osp)


def test_stream_switch_with_lanes_pending(gpu, sl):
    """Pattern A: a batched encode on S1; with no synchronisation, a sparse encode of the same context
    on S2 (skml_ctx_set_stream's event, while lane 1 holds queued buckets and the context's rank
    table and workspace are still to be read by them), S1 asserted busy right before it; back on S1,
    a decode of a lane-1 payload.  The sparse encode completes before it returns, so that decode
    runs on drained streams and cannot be delayed: it checks the switch back and the payload only."""
    from sketchml_amd.context import Context
    ns = [N_BUCKET] * 4
    pairs = [_pair("f32", N_BUCKET, tag=i + 1) for i in range(4)]
    bufs = [_payload_buf(N_BUCKET) for _ in range(4)]
    P, ptrs, nn, pptr, caps = _batch_args(pairs, bufs, ns)
    fk, fv, sk, sv, osp = _sparse_case(False, 21)
    k, v = torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda()
    fkd, fvd = torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda()
    p6, sp = _params(BINS, 6), _sparse_params(21, 22)
    out = torch.zeros(N_BUCKET, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(S1):
        ctx = Context(0)
        # warm-up on the stale data: the side context and every buffer exist, nothing is freed later
        sl.c("skml_dense_encode_batch_f32", ctx.handle, P, ptrs, nn, C.byref(p6), pptr, caps)
        _sp_free(_sp_encode(sl, ctx.handle, k, v, sp, ctx))
        sl.c("skml_dense_decode_f32", ctx.handle, _ptr(bufs[1][0]), _ptr(out), N_BUCKET)
        S1.synchronize()
        sl.sleep()
        for t, f in pairs:
            t.copy_(f, non_blocking=True)
        _busy(S1, "before the library call")
        sl.c("skml_dense_encode_batch_f32", ctx.handle, P, ptrs, nn, C.byref(p6), pptr, caps)
        _busy(S1, "when the batched encode returned")
    with torch.cuda.stream(S2):
        k.copy_(fkd, non_blocking=True)
        v.copy_(fvd, non_blocking=True)
        _busy(S1, "before the stream switch")
        h2 = ctx.handle  # moves the context to S2: skml_ctx_set_stream
        _busy(S1, "before the sparse encode on the second stream")
        spl = _sp_encode(sl, h2, k, v, sp, ctx)
        assert S1.query() and S2.query(), "the sparse encode returned before the first stream's work was done"
    with torch.cuda.stream(S1):
        sl.c("skml_dense_decode_f32", ctx.handle, _ptr(bufs[1][0]), _ptr(out), N_BUCKET)
        got = [b.clone() for b, _ in bufs] + [out.clone()]
    S1.synchronize()
    S2.synchronize()
    oqs = [_oq("f32", N_BUCKET, "quantile", 6, tag=i + 1) for i in range(4)]
    for i in range(4):
        _check_payload(got[i], N_BUCKET, oqs[i])
    _same(got[4], _decoded(oqs[1].values(), oqs[1].bins, torch.float32))
    _check_sparse_payload(spl, osp)


# The sparse entries held to "completes its device work before it returns", the invariant the
# device-wide pool of payload blocks rests on (a freed payload's block has no pending user).
SPARSE_ENTRIES_THAT_COMPLETE = (
    "skml_sparse_encode_kv_f32", "skml_sparse_encode_kv_f64", "skml_sparse_encode_f32", "skml_sparse_encode_f64",
    "skml_sparse_compact_f32", "skml_sparse_compact_f64", "skml_sparse_decode_f32", "skml_sparse_decode_f64",
    "skml_sparse_restore_bins", "skml_sparse_group_info", "skml_sparse_serialize", "skml_sparse_deserialize",
    "skml_sparse_export", "skml_sparse_import", "skml_sparse_decode_sum_f64", "skml_delta_encode", "skml_delta_decode")


def test_sparse_entries_complete_before_returning(gpu, sl):
    """Each entry of SPARSE_ENTRIES_THAT_COMPLETE, called on S behind the sleep, must have waited the
    sleep out and finished its own work when it returns: S.query() is true."""
    from sketchml_amd.context import alloc_aligned, get_context
    L = _L()
    fk, fv, _, _, _ = _sparse_case(False, 21)
    fk64, fv64, _, _, _ = _sparse_case(True, 22)
    n = len(fk)
    k, v = torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda()
    k64, v64 = torch.from_numpy(fk64).cuda(), torch.from_numpy(fv64).cuda()
    dense = torch.from_numpy(_dense_gradient(0)).cuda()
    dense64 = dense.double()
    dim = dense.numel()
    p = _sparse_params(21, 22)
    pl = _sp_encode(sl, get_context().handle, k, v, p)
    cap = (pl.export_bytes() + 255) // 256 * 256
    blob = alloc_aligned(cap, "cuda").zero_()
    pl.export(blob)
    stream_bytes = np.frombuffer(pl.serialize(), dtype=np.uint8).copy()
    qv = np.ascontiguousarray(pl.values())
    ik = torch.zeros(max(dim, n), dtype=torch.int32, device="cuda")
    f32 = torch.zeros(max(dim, n), dtype=torch.float32, device="cuda")
    f64 = torch.zeros(max(dim, n, DIM), dtype=torch.float64, device="cuda")
    i32 = torch.zeros(n, dtype=torch.int32, device="cuda")
    dk = torch.from_numpy(_delta_keys(0)).cuda()
    nd_ = dk.numel()
    fw, dw = torch.zeros(nd_ + 2, dtype=torch.int64, device="cuda"), torch.zeros(nd_ + 2, dtype=torch.int64, device="cuda")
    m, kind, nf, nd, cnt = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    info, need = L.SparseGroup(), C.c_size_t()
    table = np.zeros(ROWS * n + 16, dtype=np.int32)
    wire = np.zeros(len(stream_bytes) + 16, dtype=np.uint8)
    made = []

    def new_payload(name, *args):
        def f(h):
            out = C.c_void_p()
            sl.c(name, h, *args, C.byref(out))
            made.append(_sparse_payload(out))
        return f

    last_group = max(g for g in range(GROUPS) if pl.group(g)["size"] > 0)
    entries = {
        "skml_sparse_encode_kv_f32": new_payload("skml_sparse_encode_kv_f32", _ptr(k), _ptr(v), n, C.byref(p)),
        "skml_sparse_encode_kv_f64": new_payload("skml_sparse_encode_kv_f64", _ptr(k64), _ptr(v64), len(fk64), C.byref(p)),
        "skml_sparse_encode_f32": new_payload("skml_sparse_encode_f32", _ptr(dense), dim, C.byref(p)),
        "skml_sparse_encode_f64": new_payload("skml_sparse_encode_f64", _ptr(dense64), dim, C.byref(p)),
        "skml_sparse_compact_f32": lambda h: sl.c("skml_sparse_compact_f32", h, _ptr(dense), dim, _ptr(ik), _ptr(f32),
                                                  C.byref(cnt)),
        "skml_sparse_compact_f64": lambda h: sl.c("skml_sparse_compact_f64", h, _ptr(dense64), dim, _ptr(ik), _ptr(f64),
                                                  C.byref(cnt)),
        "skml_sparse_decode_f32": lambda h: sl.c("skml_sparse_decode_f32", h, pl.handle, _ptr(ik), _ptr(f32)),
        "skml_sparse_decode_f64": lambda h: sl.c("skml_sparse_decode_f64", h, pl.handle, _ptr(ik), _ptr(f64)),
        "skml_sparse_restore_bins": lambda h: sl.c("skml_sparse_restore_bins", h, pl.handle, _ptr(ik), _ptr(i32)),
        "skml_sparse_group_info": lambda h: sl.c("skml_sparse_group_info", h, pl.handle, last_group, C.byref(info),
                                                 table.ctypes.data_as(L.i32p), None, None),
        "skml_sparse_serialize": lambda h: sl.c("skml_sparse_serialize", h, pl.handle, wire.ctypes.data_as(L.u8p),
                                                wire.nbytes, C.byref(need)),
        "skml_sparse_deserialize": new_payload("skml_sparse_deserialize", stream_bytes.ctypes.data_as(L.u8p),
                                               len(stream_bytes), qv.ctypes.data_as(L.dblp), len(qv)),
        "skml_sparse_export": lambda h: sl.c("skml_sparse_export", h, pl.handle, _ptr(blob), cap),
        "skml_sparse_import": new_payload("skml_sparse_import", _ptr(blob), pl.export_bytes()),
        "skml_sparse_decode_sum_f64": lambda h: sl.c("skml_sparse_decode_sum_f64", h, _ptr(blob), 1, cap, DIM, 1.0, _ptr(f64)),
        "skml_delta_encode": lambda h: sl.c("skml_delta_encode", h, _ptr(dk), nd_, C.byref(m), C.byref(kind), C.byref(nf),
                                            C.byref(nd), _ptr(fw), _ptr(dw), nd_ + 2),
        "skml_delta_decode": lambda h: sl.c("skml_delta_decode", h, nd_, m.value, kind.value, _ptr(fw),
                                            (nf.value + 63) // 64, _ptr(dw), (nd.value + 63) // 64, _ptr(ik)),
    }
    assert set(entries) == set(SPARSE_ENTRIES_THAT_COMPLETE)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    pending = []
    with torch.cuda.stream(S):
        h = get_context().handle
        for name in SPARSE_ENTRIES_THAT_COMPLETE:
            sl.sleep()
            _busy(S, f"before {name}")
            entries[name](h)
            if not S.query():
                pending.append(name)
    S.synchronize()
    assert not pending, f"returned with device work still queued on the context's stream: {pending}"


def test_payload_block_recycling_across_contexts(gpu, sl):
    """The scenario the invariant exists for: payload 1 encoded and restored on S1, dropped, and at
    once another payload of the same size (so it takes the pooled block) encoded by a second
    context on S2.  The clone of the first restore and the second payload against the oracle."""
    from sketchml_amd.context import Context, get_context
    fk, fv, sk, sv, osp1 = _sparse_case(False, 21)
    n = len(fk)
    # payload 2: the stale pair's keys with other values -- the same nnz, so the same block size
    rng = np.random.default_rng(99)
    k2h, v2h = sk, rng.standard_normal(n).astype(np.float32)
    osp2 = O.sparse_compress(k2h, v2h.astype(np.float64), BINS, GROUPS, ROWS, RATIO, 23, 24)
    k1, v1 = torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda()
    fkd, fvd = torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda()
    k2, v2 = torch.from_numpy(k2h).cuda(), torch.from_numpy(v2h).cuda()
    rk = torch.zeros(n, dtype=torch.int32, device="cuda")
    rv = torch.zeros(n, dtype=torch.float32, device="cuda")
    p1, p2 = _sparse_params(21, 22), _sparse_params(23, 24)
    torch.cuda.synchronize()
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(S2):
        ctx2 = Context(0)
    with torch.cuda.stream(S1):
        h1 = get_context().handle
        sl.sleep()
        k1.copy_(fkd, non_blocking=True)
        v1.copy_(fvd, non_blocking=True)
        _busy(S1, "before the library call")
        pl1 = _sp_encode(sl, h1, k1, v1, p1)
        assert S1.query(), "the sparse encode returned with device work still queued"
        _sp_restore(sl, h1, pl1, rk, rv)
        assert S1.query(), "the sparse restore returned with device work still queued"
        got = [rk.clone(), rv.clone()]
        _sp_free(pl1)
    with torch.cuda.stream(S2):
        pl2 = _sp_encode(sl, ctx2.handle, k2, v2, p2, ctx2)
    S1.synchronize()
    S2.synchronize()
    _check_restored(got[0], got[1], osp1, n)
    _check_sparse_payload(pl2, osp2)
    r2k, r2v = pl2.restore()
    torch.cuda.synchronize()
    _check_restored(r2k, r2v, osp2, n)
