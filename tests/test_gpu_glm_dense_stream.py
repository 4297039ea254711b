"""Stream ordering of the dense gradient and validation entries, in pattern A of
tests/test_gpu_stream_order.py as tests/test_gpu_glm_stream.py applies it to their sparse twins: stale
weight and labels, the fresh ones copied in behind a sleep on the context's non-blocking stream, clones
of the outputs queued behind the call.  The reference is tests/glm_ref.py on the fresh data."""
import ctypes as C

import pytest
import torch

import glm_ref as R
from test_gpu_glm_dense import _case, _same
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", ["gradient", "validate"])
def test_dense_entries(gpu, sl, entry):
    from sketchml_amd import _lib as L
    from sketchml_amd.data import DenseDataSet
    rows, dim = 200, 37
    x, y_fresh, w_fresh, csr = _case(rows, dim, True)
    ds = DenseDataSet.fromArray(x, -3.0 * y_fresh, dim, device="cuda")  # the stale labels
    d = ds.glm_data()
    w = torch.from_numpy(_case(70, dim)[2].copy()).cuda()               # the stale weight
    r0, batch = (150, 130) if entry == "gradient" else (0, rows)
    pre, coef, loss = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(3))
    grad = torch.zeros(dim, dtype=torch.float64, device="cuda")
    nnz, obj, res = C.c_int64(), C.c_double(), L.ValidResult()
    outs = [pre, coef, loss, grad] if entry == "gradient" else [pre, loss]

    def call(h):
        if entry == "gradient":
            sl.c("skml_glm_gradient_dense_f64", h, C.byref(d), r0, batch, R.L2_SQUARE, _ptr(w), _ptr(pre), _ptr(coef), _ptr(loss),
                 _ptr(grad), C.byref(nnz), C.byref(obj))
        else:
            sl.c("skml_glm_validate_dense_f64", h, C.byref(d), R.L2_SQUARE, _ptr(w), L.SKML_VALID_AUC, _ptr(pre), _ptr(loss), C.byref(res))

    got = run_a(sl, [(w, torch.from_numpy(w_fresh).cuda()), (ds.label, torch.from_numpy(y_fresh).cuda())], call, lambda: outs,
                scribble=outs, host_sync=True)
    win, _ = R.window_rows(rows, r0, batch)
    r_pre, r_coef, r_loss = R.predict(csr, w_fresh, win, R.L2_SQUARE)
    want = (r_pre, r_coef, r_loss, R.plus_by(csr, dim, win, r_coef)) if entry == "gradient" else (r_pre, r_loss)
    for a, b in zip(got, want):
        _same(a, b, entry)
    assert nnz.value == R.count_nnz(want[-1]) if entry == "gradient" else (
        res.loss == float(R.sum_forward(list(r_loss))) and res.pos == int((y_fresh == 1.0).sum()) and res.num == rows)
