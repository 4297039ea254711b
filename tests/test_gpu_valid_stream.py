"""Stream ordering of the validation entries, in pattern A of tests/test_gpu_stream_order.py (whose
delay, fixtures and run_a this file uses, as tests/test_gpu_glm_stream.py does): the context sits on
a non-blocking stream, a calibrated sleep is queued ahead of the copies that bring the fresh weight,
labels or scores in, and clones of the outputs are queued behind the call.  Work that is not ordered
after the stream reads the stale inputs; work that is not joined into the stream is missed by the
clones.  The entries synchronise the host for their scalars, so those are the fresh data's too.  The
reference is tests/glm_ref.py and tests/valid_ref.py on the fresh data (the square loss, whose every
bit is pinned)."""
import ctypes as C

import numpy as np
import pytest
import torch

import glm_fixtures as FX
import glm_ref as R
import valid_ref as V
from test_gpu_glm import _same
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu


def test_validate_with_the_auc(gpu, sl):
    from sketchml_amd import _lib
    from sketchml_amd.data import DataSet
    data, dim = FX.lengths_data("mid")
    rows_n = len(data[3])
    ds = DataSet.fromCSR(*data, dim, device="cuda")
    d = ds.glm_data()
    w_fresh, w_stale = FX.weights(dim), FX.weights(dim, seed=77)
    y_fresh = data[3]
    y_stale = np.where(np.arange(rows_n) % 3 == 0, 1.0, -3.0)
    w, label = torch.from_numpy(w_stale.copy()).cuda(), ds.label
    label.copy_(torch.from_numpy(y_stale))
    pre, loss = (torch.zeros(rows_n, dtype=torch.float64, device="cuda") for _ in range(2))
    res = _lib.ValidResult()

    def call(h):
        sl.c("skml_glm_validate_f64", h, C.byref(d), R.L2_SQUARE, _ptr(w), _lib.SKML_VALID_AUC, _ptr(pre), _ptr(loss), C.byref(res))

    got = run_a(sl, [(w, torch.from_numpy(w_fresh).cuda()), (label, torch.from_numpy(y_fresh).cuda())], call,
                lambda: [pre, loss], scribble=[pre, loss], host_sync=True)
    r_pre, _, r_loss = R.predict(data, w_fresh, list(range(rows_n)), R.L2_SQUARE)
    _same(got[0].cpu().numpy(), r_pre, "pre")
    _same(got[1].cpu().numpy(), r_loss, "loss")
    want = V.cal_loss_precision(r_pre, r_loss, y_fresh)
    assert (res.loss, res.true_pos, res.true_neg, res.false_pos, res.false_neg, res.num) == want
    assert (res.rank_sum, res.pos, res.neg) == V.rank_sum(y_fresh[V.stable_order(r_pre)])
    # the stale data would have given another answer
    s_pre, _, s_loss = R.predict(data, w_stale, list(range(rows_n)), R.L2_SQUARE)
    assert V.cal_loss_precision(s_pre, s_loss, y_stale)[:5] != want[:5]
    assert V.rank_sum(y_stale[V.stable_order(s_pre)]) != V.rank_sum(y_fresh[V.stable_order(r_pre)])


def test_rank_sum_and_ordered_sum(gpu, sl):
    n = 24581
    rng = np.random.default_rng(12)
    s_fresh, s_stale = rng.permutation(n) * 1e-6 - 0.01, rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n).astype(np.float64))
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    s, yd = torch.from_numpy(s_stale.copy()).cuda(), torch.from_numpy(y).cuda()
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    pos, neg, nan, sig, total = C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64(), C.c_double()

    def call(h):
        sl.c("skml_auc_rank_sum", h, _ptr(s), _ptr(yd), n, _ptr(order), C.byref(pos), C.byref(neg), C.byref(sig), C.byref(nan))

    got = run_a(sl, [(s, torch.from_numpy(s_fresh).cuda())], call, lambda: [order], scribble=[order], host_sync=True)
    stable = V.stable_order(s_fresh)
    assert np.array_equal(got[0].cpu().numpy(), stable.astype(np.int32))
    assert (sig.value, pos.value, neg.value, nan.value) == V.rank_sum(y[stable]) + (0,)
    assert V.rank_sum(y[V.stable_order(s_stale)])[0] != sig.value

    x_fresh = s_stale[::-1].copy()  # the same values in another order: another sum
    x = torch.from_numpy(s_stale.copy()).cuda()

    def call_sum(h):
        sl.c("skml_glm_seq_sum", h, _ptr(x), n, C.byref(total))

    run_a(sl, [(x, torch.from_numpy(x_fresh).cuda())], call_sum, lambda: [], host_sync=True)
    assert R.bits([total.value])[0] == R.bits([V.sum_forward(x_fresh)])[0]
    assert R.bits([V.sum_forward(s_stale)])[0] != R.bits([total.value])[0]
