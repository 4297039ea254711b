"""One context's grow-only buffers regrown in a stated order across the codecs.

The other files run nearly everything on the shared per-device context, whose buffers grow whenever
pytest's order makes them grow.  Here a fresh context goes through a fixed sequence in which the
record scratch changes from the fp32 to the fp64 layout, the dense workspace regrows twice (its
arrival counter must come back zeroed on the context's stream), the ZipML workspace and the stage
buffer grow, and the first call is repeated at the end, when every buffer is larger than it needs.
No host synchronisation besides what the entries themselves perform; every result is compared with
its reference after the sequence.

Sizes: 50,000 = 3 leaf tiles of 16,384 values and a ragged tail; 2^20 + 77 has bit 12 of the chunk
count set (an upper merge pass, which on the fp64 path uses the dense workspace's arrival counter);
2^20 + 777 and 2^22 + 5 each need a larger dense workspace than everything before them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import fixed_point_ref as R
from tests import zipml_ref as Z
from tests.test_gpu_fixed_point import _parse as _parse_fixed
from tests.test_gpu_stream_order import (BINS, _bits64, _check_payload, _dense, _L, _oq, _params, _parse, _payload_buf,
                                         _ptr)
from tests.test_gpu_zipml import _hook

pytestmark = pytest.mark.gpu

N_SMALL, N_MID, N_WS, N_BIG = 50000, 2**20 + 77, 2**20 + 777, 2**22 + 5
FIXED_BITS, FIXED_SEED, ZIP_BINS = 8, 3, 16


@functools.lru_cache(maxsize=None)
def _small(n):
    """N(0, 1) * 1e-3 in fp32 (the FixedPoint and ZipML files' inputs); read-only, shared."""
    v = (np.random.default_rng(4242 + n).standard_normal(n) * 1e-3).astype(np.float32)
    v.setflags(write=False)
    return v


def _check_fixed(pl, v):
    """As tests/test_gpu_fixed_point.py: the norm within its bound, the words with the header's norm."""
    n = len(v)
    h, words = _parse_fixed(pl, n, FIXED_BITS)
    assert h.status == 0 and h.seed == FIXED_SEED
    want_norm = math.sqrt(math.fsum((v.astype(np.float64) ** 2).tolist()))
    assert abs(h.norm - want_norm) <= 2.0 ** -40 * want_norm
    want = R.pack_words(R.encode_codes(v.astype(np.float64), FIXED_BITS, FIXED_SEED, norm=h.norm), FIXED_BITS)
    bad = np.nonzero(words != want)[0]
    assert bad.size == 0, f"{bad.size} of {len(words)} words differ, first at {int(bad[0])}"


def _check_zip(pl, v, prefix):
    """As tests/test_gpu_zipml.py: the restatement run on the device's own sorted copy and prefix sums."""
    z = Z.quantize(v, ZIP_BINS, *prefix)
    assert z.status == Z.OK
    h, sp, got = _parse(pl)
    assert (h.n, h.bin_num, h.req_bins, h.zero_idx) == (len(v), z.bin_num, ZIP_BINS, z.zero_idx)
    assert np.array_equal(_bits64([h.min, h.max]), _bits64([z.min, z.max]))
    assert np.array_equal(_bits64(sp), _bits64(z.splits))
    assert np.array_equal(got, z.bins(v))


def test_buffers_regrow_in_order_on_one_context(gpu):
    from sketchml_amd.context import Context, alloc_aligned
    L = _L()
    lib = L.lib
    steps = []  # (entry, arguments after the context, check of its payload)

    def dense(entry, kind, n, mode, seed, *extra):
        x = _dense(kind, n, 0)[0].cuda()
        pl, nb = _payload_buf(n)
        p = _params(BINS, seed, dedup=0 if mode.startswith("T") else 1)
        steps.append((entry, (_ptr(x), n, *extra, C.byref(p), _ptr(pl), nb), (x, p),
                      lambda: _check_payload(pl, n, _oq(kind, n, mode, seed))))

    def fixed(n):
        v = _small(n)
        x = torch.from_numpy(np.array(v)).cuda()
        nb = lib.skml_fixed_payload_bytes(n, FIXED_BITS)
        pl = alloc_aligned(nb, "cuda").zero_()
        steps.append(("skml_fixed_encode_f32", (_ptr(x), n, FIXED_BITS, FIXED_SEED, _ptr(pl), nb), (x,),
                      lambda: _check_fixed(pl, v)))

    def zipml(n):
        v = _small(n)
        prefix = _hook(np.array(v))  # on the shared context: the tree is fixed, so the sums are the encode's own
        x = torch.from_numpy(np.array(v)).cuda()
        pl, nb = _payload_buf(n, ZIP_BINS)
        steps.append(("skml_zip_encode_f32", (_ptr(x), n, ZIP_BINS, _ptr(pl), nb), (x,),
                      lambda: _check_zip(pl, v, prefix)))

    dense("skml_dense_encode_parallel_f32", "f32", N_SMALL, "T3", 11, 3)   # 1
    dense("skml_dense_encode_parallel_f64", "f64", N_MID, "T5", 12, 5)     # 2: record scratch fp32 -> fp64 layout
    dense("skml_dense_encode_f32", "f32", N_WS, "quantile", 5)             # 3: the dense workspace regrows
    for n in (N_SMALL, N_MID):                                             # 4
        dense("skml_dense_encode_uniform_f64", "f64", n, "uniform", 0)
        fixed(n)
        zipml(n)
    dense("skml_dense_encode_f32", "f32", N_BIG, "quantile", 6)            # 5: second regrow, and the rank table's
    dense("skml_dense_encode_parallel_f32", "f32", N_SMALL, "T3", 11, 3)   # 6: step 1 in buffers larger than it needs
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        ctx = Context(0)
        for entry, args, _keep, _check in steps:
            st = getattr(lib, entry)(ctx.handle, *args)
            assert st == 0, f"{entry}: status {st}: {L.last_error()}"
    S.synchronize()
    for entry, _args, _keep, check in steps:
        check()
