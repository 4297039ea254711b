"""The optimiser update on the device against tests/optim_ref.py, bit for bit.

The reference is fed with the oracle's decoded doubles (oracle.uniform_quantize: values()[bins]; the
uniform quantizer keeps exactly the requested bin count at every n, so the code width of a case is
the one its name says), summed and scaled in float64 in payload order.  The library's own decode is
never the reference.  Every comparison is on the bit patterns of w, m and v.
"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import optim_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DT = {"f32": (np.float32, torch.float32, np.uint32), "f64": (np.float64, torch.float64, np.uint64)}
N_EDGES = [1, 7, 8, 9, 2047, 2048, 2049, 65539, 2**20 + 1]
N_TWO_TRIPS = 2**23 + 2048 + 5  # 4,096 workgroups x 256 lanes x 8 elements, and a step more


def _L():
    from sketchml_amd import _lib
    return _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _same(got, want, what):
    ut = np.uint32 if want.dtype == np.float32 else np.uint64
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(got.view(ut) != want.view(ut))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def _params(kind, select=R.ALL, second_epoch=True):
    """The library's parameters and the reference's, with beta_t one epoch on so that no constant
    equals its default."""
    L = _L()
    p = L.OptParams()
    L.lib.skml_opt_params_default(C.byref(p))
    p.kind, p.select, p.lr = kind, select, 0.05
    rp = R.Params(kind, 0.05)
    if second_epoch:
        p.beta1_t, p.beta2_t = 0.9 * 0.9, 0.999 * 0.999
        rp.beta1_t, rp.beta2_t = 0.9 * 0.9, 0.999 * 0.999
    return p, rp


@functools.lru_cache(maxsize=None)
def _state(n, dt, seed=5):
    """A recognisable non-zero state (never modified): w ~ N(0,1), m ~ 0.1 N(0,1), v ~ 0.01 N(0,1)^2."""
    rng = np.random.default_rng(seed + n)
    t = DT[dt][0]
    return (rng.standard_normal(n).astype(t), (0.1 * rng.standard_normal(n)).astype(t),
            (0.01 * rng.standard_normal(n) ** 2).astype(t))


@functools.lru_cache(maxsize=None)
def _gathered(n, bins, P, mul=1.0, seed0=0):
    """P payloads (bins: one count, or one per payload) laid out `stride` apart, and the oracle's
    decoded doubles.  Computed once per shape, shared, never modified."""
    import sketchml_amd as sk
    L = _L()
    blist = [bins] * P if isinstance(bins, int) else list(bins)
    assert len(blist) == P
    stride = max((L.lib.skml_dense_payload_bytes(n, b) + 255) // 256 * 256 for b in blist)
    allp = sk.alloc_aligned(stride * P, "cuda").zero_()
    decoded = []
    for r, b in enumerate(blist):
        x = (np.random.default_rng(1000 * seed0 + 97 * r + n).standard_normal(n) * mul).astype(np.float32)
        oq = O.uniform_quantize(x.astype(np.float64), b)
        q = sk.UniformQuantizer(b)
        q.quantize(torch.from_numpy(x).cuda())
        assert q.getBinNum() == oq.bin_num == b
        assert np.array_equal(q.getBins().cpu().numpy(), oq.bins)
        allp[r * stride:r * stride + q.payload.numel()].copy_(q.payload)
        decoded.append(oq.values()[oq.bins])
    torch.cuda.synchronize()
    return allp, stride, tuple(decoded)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_cases():
    """The shared cases live as long as the module that uses them: their host arrays (a few hundred
    MB with the 2^23 case) and device tensors are not kept for the rest of the session."""
    yield
    _gathered.cache_clear()
    _state.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _dev(state, adam):
    w, m, v = (torch.from_numpy(a.copy()).cuda() for a in state)
    return (w, m, v) if adam else (w, None, None)


def _host(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _fused(gpu, allp, stride, P, n, scale, p, dt, dev, form=0):
    L = _L()
    fn = L.lib.skml_dense_decode_sum_step_f64 if dt == "f64" else L.lib.skml_dense_decode_sum_step_f32
    with L.forced_forms(decode_sum=form):
        st = fn(gpu.get_context().handle, _ptr(allp), P, stride, n, scale, C.byref(p), *(_ptr(t) for t in dev))
    assert st == 0, L.last_error()


def _check_fused(gpu, n, bins, P, kind, dt, scale, select=R.ALL, steps=1, forms=(0,), mul=1.0, pool=None):
    allp, stride, decoded = _gathered(n, bins, pool or P, mul)
    g = R.gradient(decoded[:P], scale)
    p, rp = _params(kind, select)
    adam = kind == R.ADAM
    want = _state(n, dt)
    mask = R.selection(g, select)
    results = []
    for form in forms:
        dev = _dev(_state(n, dt), adam)
        for _ in range(steps):
            _fused(gpu, allp, stride, P, n, scale, p, dt, dev, form)
        results.append(_host(dev))
    for _ in range(steps):
        want = R.step(rp, g, want[0], want[1] if adam else None, want[2] if adam else None, mask)
    for got in results:
        for name, a, b in zip("wmv", got, want):
            if b is not None:
                _same(a, b, f"{name} (n={n} bins={bins} P={P} kind={kind} {dt} scale={scale} select={select})")
    return g, mask, results


# ---- fused, occupancy form ---------------------------------------------------------------------
@pytest.mark.parametrize("n", N_EDGES)
def test_fused_n_edges(gpu, n):
    """The edges of a lane's 8 elements, of a workgroup step (256 x 8) and of several workgroups; two
    consecutive steps, so the second reads back what the first stored."""
    for dt in DT:
        _check_fused(gpu, n, 256, 2, R.ADAM, dt, 0.5, steps=2)
        _check_fused(gpu, n, 256, 2, R.SGD, dt, 1.0)


@pytest.mark.parametrize("bins", [4, 16, 256])
@pytest.mark.parametrize("P", [1, 2, 8])
def test_fused_widths_and_payload_counts(gpu, bins, P):
    n = 65539
    for dt in DT:
        for kind in (R.ADAM, R.SGD):
            for scale in (1.0, 1.0 / P):
                _check_fused(gpu, n, bins, P, kind, dt, scale, pool=8)


def test_fused_16_bit_codes(gpu):
    for dt in DT:
        for kind in (R.ADAM, R.SGD):
            _check_fused(gpu, 40005, 1024, 2, kind, dt, 0.5)


def test_fused_second_trip_of_the_prefetch_loop(gpu):
    """The grid is capped at 4,096 workgroups: past 2^23 elements a lane takes a second step."""
    _check_fused(gpu, N_TWO_TRIPS, 256, 2, R.ADAM, "f32", 0.5)


# ---- generic form ------------------------------------------------------------------------------
def test_generic_nine_payloads(gpu):
    for dt in DT:
        for kind in (R.ADAM, R.SGD):
            _check_fused(gpu, 65539, 256, 9, kind, dt, 1.0 / 9)


def test_generic_mixed_code_widths(gpu):
    for dt in DT:
        _check_fused(gpu, 40005, (4, 256), 2, R.ADAM, dt, 0.5)


def test_generic_tables_beyond_the_lds_bound(gpu):
    """8 tables of 1,024 doubles do not fit beside the occupancy form's static LDS."""
    _check_fused(gpu, 40005, 1024, 8, R.ADAM, "f64", 0.125)


@pytest.mark.parametrize("n", [9, 2049, 65539])
def test_generic_form_forced_gives_the_same_bytes(gpu, n):
    for dt in DT:
        for bins in (4, 256):
            _, _, (occ, gen) = _check_fused(gpu, n, bins, 2, R.ADAM, dt, 0.5, steps=2, forms=(0, 1))
            for a, b in zip(occ, gen):
                assert a.tobytes() == b.tobytes()


# ---- selection ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("kind", [R.ADAM, R.SGD])
def test_live_leaves_the_rest_bit_for_bit(gpu, kind, dt):
    n = 65539
    g, mask, ((w, m, v),) = _check_fused(gpu, n, 256, 2, kind, dt, 0.5, select=R.LIVE, mul=2e-8)
    share = mask.mean()
    assert 0.10 < share < 0.90, share
    w0, m0, v0 = _state(n, dt)
    _same(w[~mask], w0[~mask], "untouched w")
    if kind == R.ADAM:
        _same(m[~mask], m0[~mask], "untouched m")
        _same(v[~mask], v0[~mask], "untouched v")
    assert not np.array_equal(w[mask], w0[mask])


def test_auto_takes_both_sides(gpu):
    n = 65539
    sides = []
    for mul in (2e-8, 4e-8):
        for dt in DT:
            g, mask, _ = _check_fused(gpu, n, 256, 1, R.ADAM, dt, 1.0, select=R.AUTO, mul=mul)
        nnz = int(R.live(g).sum())
        assert 0 < nnz < n
        sides.append(R.auto_dense(nnz, n))
        assert mask.all() == sides[-1]
    assert sides == [False, True]


# ---- array form --------------------------------------------------------------------------------
def _opt_step(gpu, g_dev, n, scale, p, dt, dev):
    L = _L()
    fn = L.lib.skml_opt_step_f64 if dt == "f64" else L.lib.skml_opt_step_f32
    st = fn(gpu.get_context().handle, _ptr(g_dev), int(g_dev.dtype == torch.float64), n, scale, C.byref(p),
            *(_ptr(t) for t in dev))
    assert st == 0, L.last_error()


@pytest.mark.parametrize("n", N_EDGES)
def test_array_form(gpu, n):
    rng = np.random.default_rng(n)
    for gdt in DT:
        x = rng.standard_normal(n).astype(DT[gdt][0])
        x[rng.random(n) < 0.3] *= 1e-9
        g = x.astype(np.float64) * np.float64(0.25)
        gd = torch.from_numpy(x).cuda()
        for dt in DT:
            for kind, select in ((R.ADAM, R.ALL), (R.SGD, R.LIVE), (R.ADAM, R.AUTO)):
                p, rp = _params(kind, select)
                adam = kind == R.ADAM
                dev = _dev(_state(n, dt), adam)
                _opt_step(gpu, gd, n, 0.25, p, dt, dev)
                w0, m0, v0 = _state(n, dt)
                want = R.step(rp, g, w0, m0 if adam else None, v0 if adam else None, R.selection(g, select))
                for name, a, b in zip("wmv", _host(dev), want):
                    if b is not None:
                        _same(a, b, f"{name} (n={n} g={gdt} state={dt} kind={kind} select={select})")


def test_sparse_decode_sum_composed_with_the_array_form(gpu):
    dim, P = 50000, 2
    pls, restored = [], []
    for r in range(P):
        rng = np.random.default_rng(40 + r)
        keys = np.nonzero(rng.random(dim) < 0.2)[0].astype(np.int32)
        vals = rng.standard_normal(len(keys))
        pls.append(gpu.encode_sparse(torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda(), 256, 8, 2, 0.3, r, r + 100))
        osp = O.sparse_compress(keys, vals, 256, 8, 2, 0.3, r, r + 100)
        ok, ob = osp.restore()
        restored.append((ok, osp.q.values()[ob]))
    from sketchml_amd.distributed import blob_stride
    stride = blob_stride([p.export_bytes() for p in pls])
    allb = torch.zeros(stride * P, dtype=torch.uint8, device="cuda")
    for i, pl in enumerate(pls):
        pl.export(allb[i * stride:(i + 1) * stride])
    summed = gpu.decode_sum(allb, P, stride, dim, 1.0 / P)
    g, _ = O.gradient_sum(restored, dim, 1.0 / P)
    p, rp = _params(R.ADAM, R.LIVE)
    dev = _dev(_state(dim, "f64"), True)
    _opt_step(gpu, summed, dim, 1.0, p, "f64", dev)
    want = R.step(rp, g, *_state(dim, "f64"), R.selection(g, R.LIVE))
    for name, a, b in zip("wmv", _host(dev), want):
        _same(a, b, name)


# ---- key / value form --------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, 20000])
def test_kv_form(gpu, nnz):
    L = _L()
    dim = 50003
    rng = np.random.default_rng(nnz)
    inner = np.sort(rng.choice(np.arange(1, dim - 1), max(nnz - 2, 0), replace=False))
    keys = np.concatenate([[0], inner, [dim - 1]]).astype(np.int32) if nnz > 1 else np.array([dim - 1], dtype=np.int32)
    assert len(keys) == nnz and np.all(np.diff(keys) > 0)  # the first and the last element among them
    for vdt in DT:
        vals = rng.standard_normal(nnz).astype(DT[vdt][0])
        vals[rng.random(nnz) < 0.3] *= 1e-9
        kd, vd = torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda()
        for dt in DT:
            for kind, select in ((R.ADAM, R.ALL), (R.SGD, R.ALL), (R.ADAM, R.LIVE)):
                p, rp = _params(kind, select)
                adam = kind == R.ADAM
                dev = _dev(_state(dim, dt), adam)
                fn = L.lib.skml_opt_step_kv_f64 if dt == "f64" else L.lib.skml_opt_step_kv_f32
                st = fn(gpu.get_context().handle, _ptr(kd), _ptr(vd), int(vdt == "f64"), nnz, dim, 0.5, C.byref(p),
                        *(_ptr(t) for t in dev))
                assert st == 0, L.last_error()
                gv = vals.astype(np.float64) * np.float64(0.5)
                w0, m0, v0 = _state(dim, dt)
                want = R.step_kv(rp, keys, gv, w0, m0 if adam else None, v0 if adam else None,
                                 None if select == R.ALL else R.live(gv))
                for name, a, b in zip("wmv", _host(dev), want):
                    if b is not None:
                        _same(a, b, f"{name} (nnz={nnz} vals={vdt} state={dt} kind={kind} select={select})")


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals(gpu):
    L = _L()
    n = 2049
    allp, stride, _ = _gathered(n, 256, 2)
    h = gpu.get_context().handle
    p, _ = _params(R.ADAM)
    sgd, _ = _params(R.SGD)
    w, m, v = _dev(_state(n, "f32"), True)
    before = _host((w, m, v))
    f32 = L.lib.skml_dense_decode_sum_step_f32

    def args(pl=allp, n_=n, par=p, w_=None, m_=None, v_=None, P=2):
        return (h, _ptr(pl), P, stride, n_, 0.5, C.byref(par), w_ if w_ is not None else _ptr(w),
                m_ if m_ is not None else _ptr(m), v_ if v_ is not None else _ptr(v))

    # a payload whose header carries the NaN status
    x = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    x[77] = np.nan
    q = gpu.QuantileQuantizer(256, seed=3, deferred=True)
    q.quantize(torch.from_numpy(x).cuda())
    nanp = allp.clone()
    nanp[stride:stride + q.payload.numel()].copy_(q.payload)
    assert f32(*args(pl=nanp)) == L.SKML_E_NAN
    assert f32(*args(n_=n - 1)) == L.SKML_E_ARG                      # the payloads hold n values
    assert f32(*args(m_=_ptr(w))) == L.SKML_E_ARG and "overlap" in L.last_error()
    half = C.c_void_p(w.data_ptr() + 4 * (n // 2 // 4 * 4))
    assert f32(*args(m_=half)) == L.SKML_E_ARG and "overlap" in L.last_error()
    assert f32(*args(par=sgd)) == L.SKML_E_ARG and "SGD" in L.last_error()  # m non-NULL with SGD
    assert f32(*args(w_=C.c_void_p(w.data_ptr() + 4))) == L.SKML_E_ARG and "aligned" in L.last_error()
    assert f32(*args(P=17)) == L.SKML_E_ARG
    bad, _ = _params(R.ADAM)
    bad.lr = float("inf")
    assert f32(*args(par=bad)) == L.SKML_E_ARG and "finite" in L.last_error()
    bad, _ = _params(R.ADAM)
    bad.beta2 = float("nan")
    assert f32(*args(par=bad)) == L.SKML_E_ARG
    # the array and key / value entries share the checks
    g = torch.zeros(n, device="cuda")
    assert L.lib.skml_opt_step_f32(h, _ptr(g), 0, n, 1.0, C.byref(p), _ptr(w), _ptr(w), _ptr(v)) == L.SKML_E_ARG
    assert L.lib.skml_opt_step_f32(h, _ptr(w), 0, n, 1.0, C.byref(p), _ptr(w), _ptr(m), _ptr(v)) == L.SKML_E_ARG
    k = torch.zeros(4, dtype=torch.int32, device="cuda")
    auto, _ = _params(R.ADAM, R.AUTO)
    assert L.lib.skml_opt_step_kv_f32(h, _ptr(k), _ptr(g), 0, 4, n, 1.0, C.byref(auto), _ptr(w), _ptr(m), _ptr(v)) == L.SKML_E_ARG
    assert L.lib.skml_opt_step_kv_f32(h, _ptr(k), _ptr(g), 0, 4, n, 1.0, C.byref(sgd), _ptr(w), _ptr(m), None) == L.SKML_E_ARG
    torch.cuda.synchronize()
    for a, b in zip(_host((w, m, v)), before):  # a refused call changes nothing
        assert a.tobytes() == b.tobytes()


# ---- Python mirror -----------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["dense", "sparse"])
def test_adam_update_over_an_epoch_boundary(gpu, source):
    """Adam.update on a SketchGradient for three batches, two per epoch: the third advances beta_t.
    From sparse, toAuto hands update a SparseDoubleGradient (the key / value form)."""
    from sketchml_amd import optim
    dim = 30011
    opt, ref = optim.Adam(dim, 0.05, 0.1, 0.5), R.Adam(dim, 0.05, 0.1, 0.5)
    w0 = _state(dim, "f64")[0]
    w = torch.from_numpy(w0.copy()).cuda()
    want = (w0, np.zeros(dim), np.zeros(dim))
    for b in range(3):
        rng = np.random.default_rng(70 + b)
        if source == "dense":
            x = rng.standard_normal(dim)
            sg = gpu.SketchGradient(gpu.DenseDoubleGradient(dim, torch.from_numpy(x).cuda()), 256, seed=b)
            oq = O.quantize(x, 256, b)
            g = oq.values()[oq.bins]
            mask = R.selection(g, R.AUTO)
            assert mask.all()  # toAuto of a dense N(0,1) gradient stays dense: update(DenseDoubleGradient)
        else:
            keys = np.nonzero(rng.random(dim) < 0.2)[0].astype(np.int32)
            vals = rng.standard_normal(len(keys))
            sp = gpu.SparseDoubleGradient(dim, torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda())
            sg = gpu.SketchGradient(sp, 256, 8, 2, 0.3, seed=b, hashSeed=b + 9)
            osp = O.sparse_compress(keys, vals, 256, 8, 2, 0.3, b, b + 9)
            ok, ob = osp.restore()
            g = np.zeros(dim)
            g[ok] = osp.q.values()[ob]
            mask = np.zeros(dim, dtype=bool)
            mask[ok] = True  # update(SparseDoubleGradient) touches every restored key
            assert not R.auto_dense(int(R.live(g).sum()), dim)
        opt.update(sg, w)
        ref.begin_update()
        want = R.step(ref.params(), g, *want, mask)
        opt.nextBatch()
        ref.next_batch()
        _same(w.cpu().numpy(), want[0], f"w after batch {b} ({source})")
    assert (opt.epoch, opt.batch) == (1, 1) and opt.beta1_t == 0.9 * 0.9 and opt.beta2_t == 0.999 * 0.999
    _same(opt.m.cpu().numpy(), want[1], "m")
    _same(opt.v.cpu().numpy(), want[2], "v")


def test_decode_sum_update_is_the_fused_consumer(gpu):
    from sketchml_amd import distributed as D
    from sketchml_amd import optim
    n, P = 65539, 8
    allp, stride, decoded = _gathered(n, 256, P)
    g = R.gradient(decoded, 1.0 / P)
    for dt in DT:
        for cls, rcls in ((optim.Adam, R.Adam), (optim.GradientDescent, R.GradientDescent)):
            opt, ref = cls(n, 0.05, 0.1, 1.0), rcls(n, 0.05, 0.1, 1.0)
            w0 = _state(n, dt)[0]
            w = torch.from_numpy(w0.copy()).cuda()
            want = (w0, np.zeros(n, dtype=w0.dtype), np.zeros(n, dtype=w0.dtype))
            for _ in range(2):  # one batch per epoch: the second update runs in epoch 1
                D.decode_sum_update(gpu.get_context().handle, allp, P, stride, n, 1.0 / P, opt, w)
                ref.begin_update()
                adam = ref.kind == R.ADAM
                nw, nm, nv = R.step(ref.params(), g, want[0], want[1] if adam else None, want[2] if adam else None)
                want = (nw, nm if adam else want[1], nv if adam else want[2])
                opt.nextBatch()
                ref.next_batch()
            _same(w.cpu().numpy(), want[0], f"w ({dt}, {cls.__name__})")
            if adam:
                _same(opt.m.cpu().numpy(), want[1], "m")
                _same(opt.v.cpu().numpy(), want[2], "v")
