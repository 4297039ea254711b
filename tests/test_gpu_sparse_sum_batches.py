"""Gradient.sum of sparse payloads over more than one scratch batch (skml_sparse_decode_sum_*,
sketchml_amd/csrc/skml_sparse_blob.cpp decode_sum_any).

The sum restores its payloads in batches whose keys, bins and run bounds fit a scratch budget of
3 GiB; the first batch starts the sum at +0.0, every later one continues it (from_out), and only the
last launch scales it and, for a float / bf16 / fp16 result, writes `out`: until then the sum lives in
a `dim`-double accumulator.  At the library's budget a second batch needs over 3 GB of restored
keys, so these tests lower the budget through the test hook skml_debug_sparse_sum_budget
(_lib.sum_budget) and every one of them asserts, through skml_debug_sparse_sum_path
(_lib.sum_path), how many batches and tile launches the call really made: a case that ran as one
batch fails.

A payload's need, as decode_sum_any's need_of computes it (stated in _need below): its keys rounded
up to 4 words x 4 B, its bins (1 B each for at most 256 quantValues, else 2 B) rounded up to 16 B,
G x (tiles of 512 keys + 1) x 4 B of run bounds, and 1,024 B.  Budgets are derived from it (never
written as byte counts) with the planner's rule restated in _plan: batches in payload order, a batch
closes before the first payload that would take it above the budget, and never before it holds one.

Every comparison is bit for bit against oracle.gradient_sum (oracle_sum): the double sum itself for
the f64 entry, and for the narrow entries the double sum x scale cast to float32 by numpy and from
there to the 16-bit type by torch on the CPU (_cast of tests/test_gpu_sparse_lowp.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_sparse_exchange import _dup_payload, _gather_local, _payload, oracle_sum
from test_gpu_sparse_lowp import OUT_DTYPES, SHAPES, _cast, _pattern

pytestmark = pytest.mark.gpu

OUTS = ["f64", "f32", "bf16", "f16"]
NARROW = ["f32", "bf16", "f16"]
DTYPES = {"f64": torch.float64, **OUT_DTYPES}
WAVE_TILES = {"agg_tiles": 1}   # SKML_FORM_AGG_TILES = 1: the 4,096-key form for payloads the LDS form would take
LDS_PER_LAUNCH = 8              # kAggVPayloads: the LDS sum-tile form takes 8 payloads a launch


def _L():
    from sketchml_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------
# the host's arithmetic, restated
# --------------------------------------------------------------------------------------------
def _need(nnz, nq, groups, dim):
    """need_of (decode_sum_any): the scratch bytes of one payload in a batch."""
    keys = (nnz + 3) // 4 * 4 * 4
    bins = (nnz * (1 if nq <= 256 else 2) + 15) // 16 * 16
    return keys + bins + groups * ((dim + 511) // 512 + 1) * 4 + 1024


def _plan(needs, budget):
    """plan_sum_batches: the batches' end indices."""
    ends, count, total = [], 0, 0
    for p, n in enumerate(needs):
        if count and total + n > budget:
            ends.append(p)
            count = total = 0
        count += 1
        total += n
    return ends + [len(needs)]


def _budget_for(needs, ends):
    """A budget under which `needs` fall into the batches ending at `ends`: the largest sum of
    consecutive needs that does (the plan only changes at such sums), so that where it can, a batch
    closes because the next payload does not fit and not because its own payload is above the budget."""
    sums = sorted({sum(needs[i:j]) for i in range(len(needs)) for j in range(i + 1, len(needs) + 1)}, reverse=True)
    for b in sums:
        if _plan(needs, b) == list(ends):
            return b
    raise AssertionError(f"no budget cuts needs {needs} at {ends}")


class Case:
    """Payloads gathered once, their needs and the oracle's sums (scale 1 and 1/P); left unchanged."""

    def __init__(self, pairs, dim):
        self.pls, self.osps = zip(*pairs)
        self.dim, self.P = dim, len(pairs)
        self.allb, self.stride = _gather_local(self.pls)
        self.needs = [_need(pl.nnz(), len(osp.q.values()), osp.group_num, dim) for pl, osp in pairs]
        self._wants = {}

    def want(self, scale):
        if scale not in self._wants:
            self._wants[scale], self.forms = oracle_sum(self.osps, self.dim, scale)
        return self._wants[scale]

    def scales(self):
        return (1.0, 1.0 / self.P)

    def budget(self, ends):
        return _budget_for(self.needs, ends)


_CASES = {}


def _case(name, build):
    if name not in _CASES:
        _CASES[name] = build()
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()


@pytest.fixture(autouse=True)
def _budget_is_back(gpu):
    """No test leaves a budget (or a form) behind for the next one."""
    yield
    assert _L().lib.skml_debug_sparse_sum_budget(0) == 0


def _equal(got, want64, out):
    if out == "f64":
        return got.dtype == torch.float64 and np.array_equal(got.cpu().numpy().view(np.uint64), want64.view(np.uint64))
    return got.dtype == OUT_DTYPES[out] and np.array_equal(_pattern(got), _cast(want64, out))


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _sum(gpu, case, out, scale, budget, path, forms={}, dst=None):
    """One decode_sum under `budget` (0: the library's) and `forms`; the call must have taken
    path = (batches, launches)."""
    L = _L()
    with L.sum_budget(budget), L.forced_forms(**forms):
        got = gpu.decode_sum(case.allb, case.P, case.stride, case.dim, scale, out=dst, dtype=DTYPES[out])
        assert L.sum_path() == path, (L.sum_path(), path, budget)
    assert got.numel() == case.dim
    return got


def _check(gpu, case, budget, path, forms={}, outs=OUTS):
    for out in outs:
        for scale in case.scales():
            got = _sum(gpu, case, out, scale, budget, path, forms)
            assert _equal(got, case.want(scale), out), (out, scale, budget, path)


def _launches(sizes, lds):
    """Tile launches of batches of `sizes` payloads: 8 payloads a launch in the LDS form, the whole
    batch in one launch of the 4,096-key form."""
    return sum(-(-n // LDS_PER_LAUNCH) if lds else 1 for n in sizes)


# --------------------------------------------------------------------------------------------
# 1. the 4,096-key form, one payload per batch
# --------------------------------------------------------------------------------------------
DIM_W = 3 * 4096 + 17   # three whole 4,096-key tiles and a ragged one: x < nk decides what the continuation reads


def _wave_case(gpu, groups):
    return _case(("wave", groups), lambda: Case([_payload(gpu, DIM_W, 0.4, 400 + p, groups=groups) for p in range(3)],
                                                DIM_W))


@pytest.mark.parametrize("groups", [12, 8])
def test_wave_tiles_one_payload_per_batch(gpu, groups):
    """Three payloads, three batches, three launches of k_agg_tiles_w (f64) or two of it into the
    accumulator and one of k_agg_tiles_w_o (narrow): payloads of 12 groups take the form by
    themselves, payloads of 8 groups under SKML_FORM_AGG_TILES = 1."""
    case = _wave_case(gpu, groups)
    assert (case.dim + 4095) // 4096 == 4 and case.dim % 4096 == 17
    budget = case.budget([1, 2, 3])
    assert budget < min(a + b for a, b in zip(case.needs, case.needs[1:]))  # below any two payloads' need
    _check(gpu, case, budget, (3, 3), forms={} if groups == 12 else WAVE_TILES)
    _check(gpu, case, 0, (1, 1), forms={} if groups == 12 else WAVE_TILES, outs=["f64", "bf16"])


# --------------------------------------------------------------------------------------------
# 2. the persistent walk with a continuation
# --------------------------------------------------------------------------------------------
DIM_BIG = 2**23 + 5


@pytest.mark.parametrize("form", ["lds", "wave"])
def test_persistent_walk_continues_tile_after_tile(gpu, form):
    """Both tile kernels are persistent: a workgroup walks tiles t, t + grid, ... and defers the
    store of tile t - 1 until tile t's element loads are in flight, so in a continuing launch the
    store of one tile and the read of the next tile's partial sum interleave (for the f64 entry in
    the same array, out).  That only happens when a workgroup takes several tiles.

    dim = 2^23 + 5.  4,096-key form: 2,049 tiles; k_agg_tiles_w holds about 56 KB of LDS a workgroup
    (the sum tile 32 KB, the quantValues 16 KB, presence bits 4 KB, run tables), so at most 2
    workgroups of the CU's 160 KB are resident, 512 on 256 CUs: workgroup 0 walks 5 tiles, every
    workgroup at least 4.  LDS sum-tile form: 16,385 tiles of 512 keys, 8 a workgroup round (one per
    wave); k_agg_rmw holds 32 KB of sum tiles and 16 KB of quantValues besides its piece tables,
    again at most 2 workgroups a CU: 512 x 8 = 4,096 tiles a round, 5 rounds.  The grid is min(tiles
    or tile groups, what hipOccupancy reports resident); a larger residency than the LDS bound
    allows cannot be reported, and even 4 a CU would leave 2 tiles a workgroup, so the dim holds
    without reading the occupancy back.  Three payloads of ~42,000 keys, two batches (2 + 1)."""
    case = _case("big", lambda: Case([_payload(gpu, DIM_BIG, 0.005, 500 + p) for p in range(3)], DIM_BIG))
    assert (case.dim + 4095) // 4096 == 2049 and (case.dim + 511) // 512 == 16385
    assert 2049 > 2 * 2 * 256 and 16385 > 2 * 8 * 2 * 256   # several tiles a workgroup at 2 (even twice 2) a CU
    budget = case.budget([2, 3])
    _check(gpu, case, budget, (2, 2), forms=WAVE_TILES if form == "wave" else {})


# --------------------------------------------------------------------------------------------
# 3. rounded once, in the 4,096-key form
# --------------------------------------------------------------------------------------------
def _narrowed(x64, out):
    """x64 rounded to the narrow type and widened again."""
    f = x64.astype(np.float32)
    return f.astype(np.float64) if out == "f32" else torch.from_numpy(f).to(OUT_DTYPES[out]).double().numpy()


@pytest.mark.parametrize("out", NARROW)
def test_wave_tiles_continued_sum_is_rounded_once(gpu, out):
    """The counterpart of test_gpu_sparse_lowp.py::test_a_continued_sum_is_rounded_once for the
    4,096-key form, where only a second batch continues a sum: with one payload per batch, a partial
    sum that passed through the narrow type after the first batch, or after the second, gives
    another result than the cast of the whole double sum on this data (shown on the oracle's
    numbers), so the device's result, which must be that cast, cannot have been rounded in between."""
    case = _wave_case(gpu, 12)
    want = case.want(1.0)
    for cut in (1, 2):
        partial, _ = oracle_sum(case.osps[:cut], case.dim)
        partial = _narrowed(partial, out)
        for osp in case.osps[cut:]:
            k, b = osp.restore()
            partial[k] += osp.q.values()[b]
        assert not np.array_equal(_cast(partial, out), _cast(want, out)), (out, cut)
    got = _sum(gpu, case, out, 1.0, case.budget([1, 2, 3]), (3, 3))
    assert _equal(got, want, out)
    got64 = _sum(gpu, case, "f64", 1.0, case.budget([1, 2, 3]), (3, 3))
    assert _equal(got64, want, "f64")   # the f64 entry's result is the sum this is the cast of


# --------------------------------------------------------------------------------------------
# 4. the tile form changes between batches
# --------------------------------------------------------------------------------------------
def _switch_case(gpu, dim, why, order):
    def build():
        lds = [_payload(gpu, dim, 0.3, 600 + p) for p in range(2)]                       # 8 groups, 256 bins
        # 512 requested bins give more than 256 quantValues only from ~384 keys on, which at dim 513 is
        # more than dim * 2 / 3: there the 512-bin payload reaches plusBy in dense form
        density = 0.8 if (dim, why) == (513, "bins") else 0.6
        other = _payload(gpu, dim, density, 610, **({"groups": 12} if why == "groups" else {"bins": 512}))
        return Case(lds + [other] if order == "lds_first" else [other] + lds, dim)
    return _case(("switch", dim, why, order), build)


@pytest.mark.parametrize("order", ["lds_first", "lds_last"])
@pytest.mark.parametrize("why", ["groups", "bins"])
@pytest.mark.parametrize("dim", [513, 200003])
def test_tile_form_changes_between_batches(gpu, dim, why, order):
    """A batch of two payloads the LDS sum-tile form takes (512-key tiles) and a batch holding a
    payload it cannot take (12 groups, or 512 bins and so 2-byte bins), which runs the 4,096-key
    form, in either order: the tile size, the tile count and the run bounds' layout change between
    the batches, the sum continues through out / the accumulator."""
    case = _switch_case(gpu, dim, why, order)
    i = 2 if order == "lds_first" else 0
    assert case.osps[i].group_num == (12 if why == "groups" else 8)
    assert (len(case.osps[i].q.values()) > 256) == (why == "bins")
    assert all(len(o.q.values()) <= 256 and o.group_num == 8 for j, o in enumerate(case.osps) if j != i)
    case.want(1.0)
    assert [f == "dense" for f in case.forms] == [j == i and (dim, why) == (513, "bins") for j in range(3)]
    ends = [2, 3] if order == "lds_first" else [1, 3]
    _check(gpu, case, case.budget(ends), (2, 2))
    _check(gpu, case, 0, (1, 1), outs=["f64", "f16"])   # one batch: the 4,096-key form for all three


# --------------------------------------------------------------------------------------------
# 5. more than 8 payloads and more than one batch in the LDS form
# --------------------------------------------------------------------------------------------
def test_lds_form_many_payloads_in_batches(gpu):
    """19 payloads at dim 200003: 4 batches of 5, 5, 5, 4 (a launch each) and 2 batches of 10 and 9
    (two launches each, 8 + 2 and 8 + 1), against the oracle and against the one batch of three
    launches the library's own budget gives."""
    dim = 200003
    case = _case("nineteen", lambda: Case([_payload(gpu, dim, 0.05, 700 + p) for p in range(19)], dim))
    assert all(o.group_num == 8 and len(o.q.values()) <= 256 for o in case.osps)
    for out in OUTS:
        for scale in case.scales():
            want = case.want(scale)
            base = _sum(gpu, case, out, scale, 0, (1, _launches([19], True)))
            assert _launches([19], True) == 3 and _equal(base, want, out)
            for ends, sizes in (([5, 10, 15, 19], [5, 5, 5, 4]), ([10, 19], [10, 9])):
                path = (len(ends), _launches(sizes, True))
                assert path in ((4, 4), (2, 4))
                got = _sum(gpu, case, out, scale, case.budget(ends), path)
                assert _equal(got, want, out), (out, scale, ends)
                assert torch.equal(_bits(got), _bits(base)), (out, scale, ends)


# --------------------------------------------------------------------------------------------
# 6. narrow output, more than 8 payloads inside one 4,096-key launch
# --------------------------------------------------------------------------------------------
def test_nine_twelve_group_payloads_in_one_launch(gpu):
    """Nine payloads of 12 groups at the library's budget: one batch, one launch, in which the kernel
    itself takes the payloads 8 at a time (its !one_batch path: payload table, quantValues and run
    bounds reloaded per tile), for every output type."""
    dim = 200003
    case = _case("nine12", lambda: Case([_payload(gpu, dim, 0.1, 800 + p, groups=12) for p in range(9)], dim))
    _check(gpu, case, 0, (1, 1))
    _check(gpu, case, case.budget([5, 9]), (2, 2))


# --------------------------------------------------------------------------------------------
# 7. dense-form payloads by position
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "wave"])
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_dense_form_payloads_by_batch(gpu, rot, form):
    """The dense, sparse, dense trio of test_gpu_sparse_lowp.py (tiny values that only the sparse
    form adds; the dense form's + 0.0 turns -0.0 sums into +0.0), one payload per batch, rotated so
    that a dense form comes first, in the middle and last."""
    dim = 30011
    trio = _case("dense_trio", lambda: SHAPES["dense_forms"](gpu))
    case = _case(("dense", rot), lambda: Case(trio[rot:] + trio[:rot], dim))
    base = ["dense", "sparse", "dense"]
    case.want(1.0)
    assert case.forms == base[rot:] + base[:rot]
    _check(gpu, case, case.budget([1, 2, 3]), (3, 3), forms=WAVE_TILES if form == "wave" else {})


# --------------------------------------------------------------------------------------------
# 8. errors across batches
# --------------------------------------------------------------------------------------------
def _raw_sum(gpu, allb, P, stride, dim, out, scale=1.0):
    """The C entry itself: (status, skml_last_error, the result)."""
    L = _L()
    dst = torch.zeros(dim, dtype=DTYPES[out], device="cuda")
    fn = getattr(L.lib, "skml_sparse_decode_sum_" + out)
    st = fn(gpu.get_context().handle, C.c_void_p(allb.data_ptr()), P, stride, dim, scale, C.c_void_p(dst.data_ptr()))
    return st, L.last_error(), dst


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("shape", ["lds", "twelve_groups"])
def test_refusals_across_batches(gpu, shape, out):
    """A payload with a key repeated across its groups in the first and in the last of three
    batches: err is zeroed once and read once at the end, so both give SKML_E_ARG with the
    single-batch message.  A payload that restores no keys is refused before any batch.  After each
    refusal a multi-batch sum and a sum at the library's budget on the same context are exact: no
    error word, accumulator or budget outlives the refused call."""
    L = _L()
    dim = 100003
    groups = 12 if shape == "twelve_groups" else 4

    def build():
        good = [_payload(gpu, dim, 0.2, 71 + p, groups=groups) for p in range(2)]
        dup = _dup_payload(gpu, dim, 72, groups=groups)
        k, _ = dup[1].restore()
        assert len(np.unique(k)) < len(k)
        with pytest.raises(O.GradientSumError, match="strictly increasing"):
            oracle_sum([good[0][1], dup[1]], dim)
        empty = gpu.encode_sparse(torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float64).cuda())
        return Case(good, dim), dup, empty

    good, dup, empty = _case(("refusals", shape), build)
    assert all(o.group_num == groups for o in good.osps + (dup[1],))
    dup_need = _need(dup[0].nnz(), len(dup[1].q.values()), dup[1].group_num, dim)

    def still_exact():
        _check(gpu, good, good.budget([1, 2]), (2, 2), outs=[out])
        _check(gpu, good, 0, (1, 1), outs=[out])

    # the single-batch refusal, for its message
    allb, stride = _gather_local([good.pls[0], dup[0]])
    st1, msg1, _ = _raw_sum(gpu, allb, 2, stride, dim, out)
    assert st1 == L.SKML_E_ARG and "strictly increasing" in msg1 and L.sum_path() == (1, 1)
    for pos in (0, 2):
        pls = list(good.pls)
        pls.insert(pos, dup[0])
        needs = list(good.needs)
        needs.insert(pos, dup_need)
        allb, stride = _gather_local(pls)
        with L.sum_budget(_budget_for(needs, [1, 2, 3])):
            st, msg, _ = _raw_sum(gpu, allb, 3, stride, dim, out)
            assert L.sum_path() == (3, 3)       # every batch ran: the error is read once, at the end
        assert (st, msg) == (L.SKML_E_ARG, msg1), (pos, st, msg)
        still_exact()
    for pos in (0, 2):
        pls = list(good.pls)
        pls.insert(pos, empty)
        allb, stride = _gather_local(pls)
        with L.sum_budget(min(good.needs)):
            st, msg, _ = _raw_sum(gpu, allb, 3, stride, dim, out)
            assert L.sum_path() == (0, 0)       # refused before the first batch
        assert st == L.SKML_E_ARG and f"payload {pos} restores no keys: head of empty list" in msg, (pos, st, msg)
        still_exact()


# --------------------------------------------------------------------------------------------
# 9. a budget below any single payload
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "wave"])
def test_a_budget_of_one_byte_gives_one_payload_per_batch(gpu, form):
    """Every payload is above a budget of 1 byte; a batch still takes one, so the call makes P
    batches, returns no error and sums exactly."""
    dim = 40009
    case = _case("five", lambda: Case([_payload(gpu, dim, 0.2, 900 + p) for p in range(5)], dim))
    assert min(case.needs) > 1 and _plan(case.needs, 1) == [1, 2, 3, 4, 5]
    _check(gpu, case, 1, (5, 5), forms=WAVE_TILES if form == "wave" else {})


# --------------------------------------------------------------------------------------------
# 10. the scratch grows between batches
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", OUTS)
def test_scratch_grows_between_batches(gpu, out):
    """On a context that has summed nothing yet, batch after batch needs more key, bin and bounds
    scratch than the one before (ascending nnz, one payload per batch), so each batch's request
    grows the buffers the batch before used; then the descending order on the same context, whose
    first batch already finds them large enough."""
    from sketchml_amd.context import Context
    L = _L()
    dim = 200003
    up = _case("ascending", lambda: Case([_payload(gpu, dim, d, 1000 + p) for p, d in enumerate((0.02, 0.15, 0.6))], dim))
    down = _case("descending", lambda: Case(list(zip(up.pls[::-1], up.osps[::-1])), dim))
    assert up.needs[0] < up.needs[1] < up.needs[2] and down.needs == up.needs[::-1]
    ctx = Context(torch.cuda.current_device())
    fn = getattr(L.lib, "skml_sparse_decode_sum_" + out)
    for case in (up, down):
        for scale in case.scales():
            dst = torch.zeros(dim, dtype=DTYPES[out], device="cuda")
            with L.sum_budget(case.budget([1, 2, 3])):
                st = fn(ctx.handle, C.c_void_p(case.allb.data_ptr()), case.P, case.stride, dim, scale,
                        C.c_void_p(dst.data_ptr()))
                assert st == 0, L.last_error()
                assert L.sum_path() == (3, 3)
            assert _equal(dst, case.want(scale), out), (out, scale, case is up)


# --------------------------------------------------------------------------------------------
# 11. an unaligned narrow out with a continuation
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", NARROW)
def test_unaligned_narrow_out_with_a_continuation(gpu, out):
    """`out` one element past a 16-byte boundary, dim 4097 (a whole 4,096-key tile, which cannot
    take its 16-byte stores here, and a tile of one key), two batches: the first batch writes the
    accumulator only, the elements before and after out[0, dim) stay as they were."""
    dim = 4097
    case = _case("unaligned", lambda: Case([_payload(gpu, dim, 0.6, 300 + dim + p) for p in range(2)], dim))
    dt = OUT_DTYPES[out]
    per = 16 // torch.empty(0, dtype=dt).element_size()
    for scale in case.scales():
        buf = torch.full((dim + 2 * per,), 7.0, dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        dst = buf[1:1 + dim]
        got = _sum(gpu, case, out, scale, case.budget([1, 2]), (2, 2), forms=WAVE_TILES, dst=dst)
        assert got.data_ptr() == dst.data_ptr()
        assert _equal(got, case.want(scale), out), (out, scale)
        rest = torch.cat([buf[:1], buf[1 + dim:]]).float()
        assert rest.numel() == 2 * per and bool((rest == 7.0).all())   # nothing written outside out[0, dim)
