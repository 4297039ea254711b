"""Stream ordering of the sparse codec's bf16 / fp16 entries, in pattern A of
tests/test_gpu_stream_order.py (whose delay, fixtures, data and run_a this file uses, as
tests/test_gpu_fixed_optim_stream.py does): the context sits on a non-blocking stream, a calibrated
sleep is queued ahead of the copies that bring the fresh input in, and clones of the outputs are
queued behind the call.  A call that is not ordered after the stream reads the stale input; the
sparse entries' contract is that they have drained the stream when they return (S.query()).
test_decode_sum_in_two_batches runs a Gradient.sum of more than one scratch batch in that pattern
and in pattern B (run_b: a fresh context beside a busy null stream)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_stream_order import (DIM, _check_restored, _check_sparse_payload, _dense_gradient,  # noqa: F401
                                   _drain, _ptr, _sp_encode, _sp_free, _sparse_case, _sparse_params, _sparse_payload,
                                   _sparse_sum_oracle, run_a, run_b, sl)
from oracle import oracle as O
from test_gpu_stream_order import BINS, GROUPS, RATIO, ROWS

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _gradient16(kind, which):
    """_dense_gradient rounded to the 16-bit type by torch on the CPU, and its numpy compaction."""
    t = torch.from_numpy(_dense_gradient(which)).to(DTYPES[kind])
    w = t.float().numpy()
    keys = np.nonzero(np.abs(w.astype(np.float64)) > 1e-8)[0].astype(np.int32)
    return t, keys, w[keys]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_compact_16_bit(gpu, sl, kind):
    fresh, keys_w, vals_w = _gradient16(kind, 0)
    stale, _, _ = _gradient16(kind, 1)
    dim = fresh.numel()
    x, fresh_d = stale.cuda(), fresh.cuda()
    keys = torch.zeros(dim, dtype=torch.int32, device="cuda")
    vals = torch.zeros(dim, dtype=torch.float32, device="cuda")
    nnz = C.c_int64()
    gk, gv = run_a(sl, [(x, fresh_d)],
                   lambda h: sl.c("skml_sparse_compact_" + kind, h, _ptr(x), dim, _ptr(keys), _ptr(vals), C.byref(nnz)),
                   lambda: [keys, vals], scribble=[keys, vals], completes=True)
    assert nnz.value == len(keys_w)
    assert np.array_equal(gk.cpu().numpy()[: len(keys_w)], keys_w)
    assert np.array_equal(gv.cpu().numpy()[: len(keys_w)].view(np.uint32), vals_w.view(np.uint32))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_encode_16_bit(gpu, sl, kind):
    fresh, keys_w, vals_w = _gradient16(kind, 0)
    stale, _, _ = _gradient16(kind, 1)
    dim = fresh.numel()
    x, fresh_d = stale.cuda(), fresh.cuda()
    osp = O.sparse_compress(keys_w, vals_w.astype(np.float64), BINS, GROUPS, ROWS, RATIO, 4, 9)
    p = _sparse_params(4, 9)
    box = {}

    def call(h):
        if box.get("pl") is not None:
            _sp_free(box["pl"])
        out = C.c_void_p()
        sl.c("skml_sparse_encode_" + kind, h, _ptr(x), dim, C.byref(p), C.byref(out))
        box["pl"] = _sparse_payload(out)

    run_a(sl, [(x, fresh_d)], call, lambda: [], completes=True)
    pl = box["pl"]
    assert pl.nnz() == len(keys_w)
    _check_sparse_payload(pl, osp)
    rk, rv = pl.restore()
    torch.cuda.synchronize()
    _check_restored(rk, rv, osp, len(keys_w))


@pytest.mark.parametrize("out_kind", ["f32", "bf16", "f16"])
def test_decode_sum_narrow(gpu, sl, out_kind):
    """tests/test_gpu_stream_order.py::test_sparse_decode_sum, pattern A, on the three narrow entries:
    the blobs are exported on S behind the sleep into slots that hold three other payloads' blobs."""
    from sketchml_amd.context import alloc_aligned, get_context
    P = 3
    dt = {"f32": torch.float32, **DTYPES}[out_kind]
    h0 = get_context().handle
    pls, stales = [], []
    for r in range(P):
        fk, fv, sk, sv, _ = _sparse_case(False, 31 + r)
        p = _sparse_params(31 + r, 32 + r)
        pls.append(_sp_encode(sl, h0, torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda(), p))
        stales.append(_sp_encode(sl, h0, torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda(), p))
    stride = (max(q.export_bytes() for q in pls + stales) + 255) // 256 * 256
    allb = alloc_aligned(stride * P, "cuda").zero_()
    out = torch.zeros(DIM, dtype=dt, device="cuda")
    for r, q in enumerate(stales):
        q.export(allb[r * stride:(r + 1) * stride])
    torch.cuda.synchronize()

    def decode_sum(h):
        sl.c("skml_sparse_decode_sum_" + out_kind, h, _ptr(allb), P, stride, DIM, 1.0 / P, _ptr(out))

    decode_sum(h0)  # the stale sum, copied back over `out` behind the sleep
    torch.cuda.synchronize()

    def call(h):
        for r, q in enumerate(pls):
            sl.c("skml_sparse_export", h, q.handle, C.c_void_p(allb.data_ptr() + r * stride), stride)
        decode_sum(h)

    (got,) = run_a(sl, [], call, lambda: [out], scribble=[allb, out], completes=True, warm=False)
    want, _ = _sparse_sum_oracle()
    f = torch.from_numpy(want.astype(np.float32))
    if out_kind == "f32":
        assert np.array_equal(got.cpu().numpy().view(np.uint32), f.numpy().view(np.uint32))
    else:
        assert torch.equal(got.cpu().view(torch.int16), f.to(dt).view(torch.int16))


_SUM4 = []


def _sum_of_four():
    """oracle.gradient_sum x 1/4 of the four fresh payloads of test_decode_sum_in_two_batches; once."""
    if not _SUM4:
        osps = [_sparse_case(False, 31 + r)[4] for r in range(4)]
        _SUM4.append(O.gradient_sum(((k, osp.q.values()[b]) for osp in osps for k, b in [osp.restore()]), DIM, 0.25))
    return _SUM4[0]


@pytest.mark.parametrize("pattern", ["A", "B"])
@pytest.mark.parametrize("out_kind", ["f64", "bf16"])
def test_decode_sum_in_two_batches(gpu, sl, out_kind, pattern):
    """Gradient.sum of four payloads in two scratch batches of two (skml_debug_sparse_sum_budget; the
    budget is derived from the payloads' needs as in tests/test_gpu_sparse_sum_batches.py), in both
    patterns of tests/test_gpu_stream_order.py::test_sparse_decode_sum: A on a busy non-blocking
    stream (the blobs exported behind the sleep over four other payloads' blobs), B on a fresh context
    beside a busy null stream.  Each batch forks its second restore to the side lane and joins it
    before the tiles, synchronises the stream before the next batch reuses the scratch, and the second
    batch continues the sum from `out` (f64) or from the accumulator (bf16).  The call must have
    made two batches and two launches."""
    from sketchml_amd import _lib
    from sketchml_amd.context import alloc_aligned, get_context
    from test_gpu_sparse_sum_batches import _budget_for, _need
    P = 4
    dt = {"f64": torch.float64, **DTYPES}[out_kind]
    h0 = get_context().handle
    pls, stales, needs = [], [], []
    for r in range(P):
        fk, fv, sk, sv, osp = _sparse_case(False, 31 + r)
        p = _sparse_params(31 + r, 32 + r)
        pls.append(_sp_encode(sl, h0, torch.from_numpy(fk).cuda(), torch.from_numpy(fv).cuda(), p))
        stales.append(_sp_encode(sl, h0, torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda(), p))
        assert len(sk) == len(fk) and osp.group_num == GROUPS  # the stale set has the fresh set's need
        needs.append(_need(len(fk), len(osp.q.values()), GROUPS, DIM))
    budget = _budget_for(needs, [2, 4])
    stride = (max(q.export_bytes() for q in pls + stales) + 255) // 256 * 256
    allb = alloc_aligned(stride * P, "cuda").zero_()
    out = torch.zeros(DIM, dtype=dt, device="cuda")
    for r, q in enumerate(stales if pattern == "A" else pls):
        q.export(allb[r * stride:(r + 1) * stride])
    torch.cuda.synchronize()

    def decode_sum(h):
        sl.c("skml_sparse_decode_sum_" + out_kind, h, _ptr(allb), P, stride, DIM, 1.0 / P, _ptr(out))
        assert _lib.sum_path() == (2, 2)

    with _lib.sum_budget(budget):
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
    assert _lib.lib.skml_debug_sparse_sum_budget(0) == 0
    want, forms = _sum_of_four()
    assert set(forms) == {"sparse"}
    if out_kind == "f64":
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    else:
        f = torch.from_numpy(want.astype(np.float32))
        assert torch.equal(got.cpu().view(torch.int16), f.to(dt).view(torch.int16))
