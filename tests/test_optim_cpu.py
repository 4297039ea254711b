"""The optimiser update as far as a machine without a GPU can check it: the numpy reference
(tests/optim_ref.py) against examples worked by hand, the beta_t schedule, toAuto's rule, and the C
ABI's new entries (bound, and refusing a NULL context before they touch a device)."""
import ctypes as C
import math

import numpy as np
import pytest

import optim_ref as R

ENTRIES = ("skml_dense_decode_sum_step_f32", "skml_dense_decode_sum_step_f64", "skml_opt_step_f32", "skml_opt_step_f64",
           "skml_opt_step_kv_f32", "skml_opt_step_kv_f64")


def _hand_adam(g, lr):
    """One Adam step from m = v = 0 with the default betas, in plain Python floats, in the order of
    Adam.scala:54-57."""
    m_t = 0.9 * 0.0 + (1 - 0.9) * g
    v_t = 0.999 * 0.0 + (1 - 0.999) * g * g
    ng = (math.sqrt(1 - 0.999) * m_t) / ((1 - 0.9) * (math.sqrt(v_t) + 1e-8))
    return ng * lr, m_t, v_t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_adam_step_by_hand(dtype):
    g = np.array([3.0, -4.0, 0.0, 1e-9])
    w0 = np.array([1.0, 2.0, 3.0, 4.0], dtype=dtype)
    z = np.zeros(4, dtype=dtype)
    p = R.Params(R.ADAM, lr=0.1)
    w, m, v = R.step(p, g, w0, z, z, R.selection(g, R.ALL))
    # from zero state the step is sign(g) * lr * sqrt(1 - beta2_t) / (1 - beta1_t) * (1 - beta1) / sqrt(1 - beta2)
    # up to eps, i.e. about lr * 1.0 for the default betas: 3 and -4 move by -0.1 and +0.1
    assert abs(float(w[0]) - 0.9) < 1e-6 and abs(float(w[1]) - 2.1) < 1e-6
    assert abs(float(m[0]) - 0.3) < 1e-7 and abs(float(m[1]) + 0.4) < 1e-7
    assert abs(float(v[0]) - 0.009) < 1e-9 and abs(float(v[1]) - 0.016) < 1e-9
    # g = 0: m_t = v_t = 0 and the step is 0 / (0.1 * 1e-8) = 0
    assert w[2] == dtype(3.0) and m[2] == 0 and v[2] == 0
    # g = 1e-9 is below eps: sqrt(v_t) = 3.2e-11, so the step is 0.1 * 0.0316e-10 / (0.1 * 1.003e-8) = 3.15e-4
    assert abs(float(w0[3]) - float(w[3]) - 3.152e-4) < (1e-6 if dtype == np.float32 else 1e-7)
    for i in range(4):  # and exactly the scalar arithmetic, rounded once at the store
        d, m_t, v_t = _hand_adam(float(g[i]), 0.1)
        assert w[i] == dtype(float(w0[i]) - d) and m[i] == dtype(m_t) and v[i] == dtype(v_t)

    # LIVE: |g| <= 1e-8 is left alone, bit for bit
    w0 = np.array([1.0, 2.0, 3.0, 4.0], dtype=dtype)
    m0 = np.array([0.5, 0.5, 0.5, 0.5], dtype=dtype)
    v0 = np.array([0.25, 0.25, 0.25, 0.25], dtype=dtype)
    mask = R.selection(g, R.LIVE)
    assert mask.tolist() == [True, True, False, False]
    wl, ml, vl = R.step(p, g, w0, m0, v0, mask)
    assert wl[2] == 3 and wl[3] == 4 and (ml[2:] == 0.5).all() and (vl[2:] == 0.25).all()
    wa, ma, va = R.step(p, g, w0, m0, v0, R.selection(g, R.ALL))
    assert (wl[:2] == wa[:2]).all() and (ml[:2] == ma[:2]).all() and (vl[:2] == va[:2]).all()
    # ALL with g = 0 and a non-zero state: m and v decay and w still moves
    assert ma[2] == dtype(0.9 * 0.5) and va[2] == dtype(0.999 * 0.25) and wa[2] < 3


def test_sgd_step_by_hand():
    g = np.array([3.0, -4.0, 0.0, 1e-9])
    w0 = np.array([1.0, 2.0, 3.0, 4.0])
    w, m, v = R.step(R.Params(R.SGD, lr=0.5), g, w0)
    assert m is None and v is None
    assert w.tolist() == [1.0 - 1.5, 2.0 + 2.0, 3.0, 4.0 - 1e-9 * 0.5]
    w32, _, _ = R.step(R.Params(R.SGD, lr=0.5), g, w0.astype(np.float32))
    assert w32.dtype == np.float32 and w32[3] == np.float32(4.0 - 5e-10)
    wk, _, _ = R.step_kv(R.Params(R.SGD, lr=0.5), [1, 3], [-4.0, 1e-9], w0)
    assert wk.tolist() == [1.0, 4.0, 3.0, 4.0 - 5e-10]


def test_beta_t_advances_at_the_first_batch_of_a_later_epoch():
    o = R.Adam(10, 0.1, 0.5, 0.5)  # two batches per epoch
    assert o.batchNum == 2.0
    seen = []
    for _ in range(5):
        o.begin_update()
        seen.append((o.epoch, o.batch, o.beta1_t, o.beta2_t))
        o.next_batch()
    assert [s[:2] for s in seen] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    assert seen[0][2:] == (0.9, 0.999) and seen[1][2:] == (0.9, 0.999)
    assert seen[2][2:] == (0.9 * 0.9, 0.999 * 0.999) == seen[3][2:]
    assert seen[4][2:] == (0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999)
    assert o.params().lr == 0.1  # Adam passes lr_0 itself
    s = R.GradientDescent(10, 0.1, 0.5, 0.5)
    s.epoch = 2
    assert s.params().lr == 0.1 / math.sqrt(1.0 + 0.5 * 2)


def test_python_optimisers_keep_the_same_schedule():
    """sketchml_amd.optim's host side against the restatement (no device work)."""
    from sketchml_amd import optim
    for cls, ref in ((optim.Adam, R.Adam), (optim.GradientDescent, R.GradientDescent)):
        a, b = cls(10, 0.1, 0.5, 0.3), ref(10, 0.1, 0.5, 0.3)
        assert a.batchNum == b.batchNum == 4.0
        for _ in range(9):
            a._begin_update()
            b.begin_update()
            pa, pb = a.params(), b.params()
            assert (a.epoch, a.batch) == (b.epoch, b.batch)
            assert (pa.kind, pa.lr) == (pb.kind, pb.lr)
            if ref is R.Adam:
                assert (pa.beta1, pa.beta2, pa.beta1_t, pa.beta2_t, pa.eps) == (pb.beta1, pb.beta2, pb.beta1_t, pb.beta2_t, pb.eps)
            a.nextBatch()
            b.next_batch()


def test_auto_on_both_sides_of_two_thirds():
    from sketchml_amd.gradient import auto_dense
    g = np.zeros(9)
    g[:6] = 1.0
    assert R.selection(g, R.AUTO).tolist() == [True] * 6 + [False] * 3  # 6 > 6 is false: LIVE
    g[6] = -1.0
    assert R.selection(g, R.AUTO).all()                                  # 7 > 6: ALL
    for nnz, dim in ((6, 9), (7, 9), (0, 1), (1, 1), (666, 1000), (667, 1000), (0, 1_200_000_000), (5, 1_073_741_824),
                     (715_827_882, 1_073_741_823), (715_827_883, 1_073_741_823)):
        assert R.auto_dense(nnz, dim) == auto_dense(nnz, dim)
    # dim * 2 overflows a Java int from 2^30 on: the limit is negative and every count is "dense"
    assert R.auto_dense(0, 1_200_000_000) and R.auto_dense(0, 1 << 30)
    assert not R.auto_dense(715_827_882, (1 << 30) - 1) and R.auto_dense(715_827_883, (1 << 30) - 1)
    assert R.selection(np.zeros(4), R.AUTO, dim=1_200_000_000).all()


def test_optimiser_entries_are_exported():
    from sketchml_amd import _lib
    for name in ENTRIES + ("skml_opt_params_default",):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib, name)
    for a, b in zip(ENTRIES[0::2], ENTRIES[1::2]):
        assert _lib._SIGS[a] == _lib._SIGS[b]
    p = _lib.OptParams()
    _lib.lib.skml_opt_params_default(C.byref(p))
    assert (p.kind, p.select) == (_lib.SKML_OPT_ADAM, _lib.SKML_OPT_ALL)
    assert (p.lr, p.beta1, p.beta2, p.beta1_t, p.beta2_t, p.eps) == (0.0, 0.9, 0.999, 0.9, 0.999, 1e-8)
    assert C.sizeof(_lib.OptParams) == 56


def test_optimiser_entries_refuse_a_null_context():
    from sketchml_amd import _lib
    L = _lib.lib
    p = _lib.OptParams()
    L.skml_opt_params_default(C.byref(p))
    buf = C.c_void_p(4096)  # never dereferenced: the context is checked first
    for name in ENTRIES[:2]:
        assert getattr(L, name)(None, buf, 1, 4096, 16, 1.0, C.byref(p), buf, buf, buf) == _lib.SKML_E_ARG
        assert "ctx" in _lib.last_error()
    for name in ENTRIES[2:4]:
        assert getattr(L, name)(None, buf, 0, 16, 1.0, C.byref(p), buf, buf, buf) == _lib.SKML_E_ARG
        assert "ctx" in _lib.last_error()
    for name in ENTRIES[4:]:
        assert getattr(L, name)(None, buf, buf, 0, 4, 16, 1.0, C.byref(p), buf, buf, buf) == _lib.SKML_E_ARG
        assert "ctx" in _lib.last_error()
