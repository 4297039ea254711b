"""Host-side checks of the mini-batch gradient (no GPU): the restatement tests/glm_ref.py and the host
scalars of sketchml_amd/loss.py on hand-worked cases of every loss branch, the looping window, toAuto's
threshold, the sparse form of L2, the parsers, the ABI surface, the sensitivity of the shared
fixture to the order of its additions, and the header's window split and column walk as a
stand-alone program (tests/glm_check.cpp) under the address and undefined-behaviour sanitizers."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import glm_fixtures as FX
import glm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _losses():
    from sketchml_amd import loss as L
    return {R.L1_LOG: L.L1LogLoss, R.L2_HINGE: L.L2HingeLoss, R.L2_LOG: L.L2LogLoss, R.L2_SQUARE: L.L2SquareLoss}


def _up(x):
    return float(np.nextafter(x, np.inf))


def _down(x):
    return float(np.nextafter(x, -np.inf))


@pytest.mark.parametrize("kind", [R.L1_LOG, R.L2_LOG])
def test_log_loss_branches_at_18(kind):
    """z > 18 -> exp(-z), y * exp(-z); z < -18 -> -z, y; else log(1 + exp(-z)), y / (1 + exp(z)): z = +-18
    exactly is the middle branch, one ulp outside is not."""
    host = _losses()[kind](0.0)
    e18 = math.exp(-18.0)
    for y in (1.0, -1.0):
        for z, want_loss, want_grad in [
            (18.0, math.log(1.0 + e18), y / (1.0 + math.exp(18.0))),
            (_up(18.0), math.exp(-_up(18.0)), y * math.exp(-_up(18.0))),
            (_down(18.0), math.log(1.0 + math.exp(-_down(18.0))), y / (1.0 + math.exp(_down(18.0)))),
            (-18.0, math.log(1.0 + math.exp(18.0)), y / (1.0 + math.exp(-18.0))),
            (_down(-18.0), -_down(-18.0), y),
            (_up(-18.0), math.log(1.0 + math.exp(-_up(-18.0))), y / (1.0 + math.exp(_up(-18.0)))),
        ]:
            pre = z * y  # y = +-1: pre * y == z exactly
            assert pre * y == z
            assert host.loss(pre, y) == want_loss and host.grad(pre, y) == want_grad, (z, y)
            # numpy's exp and log are not Python's: the restatement takes the same branch, within 2 ulp
            assert math.isclose(float(R.loss_of(kind, pre, y)), want_loss, rel_tol=2 ** -51)
            assert math.isclose(float(R.grad_of(kind, pre, y)), want_grad, rel_tol=2 ** -51)
    # the branch, not only the value: just past 18 the loss is exp(-z) itself, not log1p of it
    assert float(R.loss_of(kind, _up(18.0), 1.0)) == float(np.exp(-np.float64(_up(18.0))))
    assert float(R.loss_of(kind, _down(-18.0), 1.0)) == -_down(-18.0)
    assert float(R.grad_of(kind, -_down(-18.0), -1.0)) == -1.0  # pre * y < -18: the gradient is y


def test_hinge_at_one_and_square():
    hinge = _losses()[R.L2_HINGE](0.0)
    for y in (1.0, -1.0):
        pre = 1.0 * y
        # loss tests `< 1.0`, the gradient `<= 1.0`: at pre * y == 1.0 the loss is 0.0 and the gradient y
        assert hinge.loss(pre, y) == 0.0 and hinge.grad(pre, y) == y
        assert float(R.loss_of(R.L2_HINGE, pre, y)) == 0.0 and float(R.grad_of(R.L2_HINGE, pre, y)) == y
        assert hinge.loss(_down(1.0) * y, y) == 1.0 - _down(1.0) and hinge.grad(_down(1.0) * y, y) == y
        assert hinge.loss(_up(1.0) * y, y) == 0.0 and hinge.grad(_up(1.0) * y, y) == 0.0
        assert float(R.grad_of(R.L2_HINGE, _up(1.0) * y, y)) == 0.0
    sq = _losses()[R.L2_SQUARE](0.0)
    assert sq.loss(3.0, 1.0) == 2.0 and sq.grad(3.0, 1.0) == -2.0
    assert float(R.loss_of(R.L2_SQUARE, 3.0, 1.0)) == 2.0 and float(R.grad_of(R.L2_SQUARE, 3.0, 1.0)) == -2.0
    # 0.5 * (pre - y) * (pre - y) associates to the left
    a, b = 1e-200, 0.0
    assert sq.loss(a, b) == (0.5 * a) * a == float(R.loss_of(R.L2_SQUARE, a, b))


def test_regulariser_flags_and_getreg():
    import torch
    L = _losses()
    w = torch.tensor([3.0, -4.0, 0.0], dtype=torch.float64)
    l1, l2, off = L[R.L1_LOG](0.5), L[R.L2_HINGE](0.5), L[R.L2_LOG](1e-9)
    assert l1.isL1Reg and not l1.isL2Reg and l1.getRegParam == 0.5 and l1.getReg(w) == 3.5
    assert l2.isL2Reg and not l2.isL1Reg and l2.getReg(w) == 2.5
    assert not off.isL2Reg and off.getReg(w) == 0.0  # lambda > 1e-8 turns it on
    assert (l1.reg_kind(), l2.reg_kind(), off.reg_kind()) == (R.REG_L1, R.REG_L2, R.REG_NONE)
    assert l2.predict(w, ([0, 1], [2.0, 0.5])) == 4.0


def test_window_order_and_read_index():
    from sketchml_amd.data import DataSet
    from sketchml_amd.exceptions import SketchMLException
    rows = [(1.0, [0], [1.0]), (-1.0, [], []), (1.0, [1, 2], [2.0, 3.0]), (1.0, [2], [4.0]), (-1.0, [0, 2], [5.0, 6.0])]
    ds = DataSet.fromRows(rows, 3, device="cpu")
    assert ds.size == 5
    ri = 0
    for batch in (2, 3, 4, 5, 1, 4):  # no wrap, ends at size (readIndex == size), wraps, a full turn, ...
        want, ri_after = R.window_rows(5, ri, batch)
        before = ds.readIndex
        r0 = ds.take(batch)
        assert r0 == (0 if before >= 5 else before) == want[0]
        assert DataSet.window_rows(5, r0, batch) == want and ds.readIndex == ri_after
        ri = ri_after
    assert R.window_rows(5, 2, 3) == ([2, 3, 4], 5)  # readIndex == size is left standing ...
    assert R.window_rows(5, 5, 2) == ([0, 1], 2)     # ... and reset by the next read
    ds.readIndex = 5
    assert ds.take(2) == 0 and ds.readIndex == 2
    ds.readIndex = 4
    assert ds.loopingRead() == (-1.0, [0, 2], [5.0, 6.0]) and ds.readIndex == 5
    assert ds.loopingRead() == (1.0, [0], [1.0]) and ds.readIndex == 1
    with pytest.raises(SketchMLException):
        ds.take(6)
    with pytest.raises(SketchMLException):
        ds.add(rows[0])  # the column order exists
    # the (column, row) order of the same entries
    assert ds.col_ptr.tolist() == [0, 2, 3, 6] and ds.csc_row.tolist() == [0, 4, 2, 2, 3, 4]
    assert ds.csc_val.tolist() == [1.0, 5.0, 2.0, 3.0, 4.0, 6.0]


def test_dataset_refuses_bad_rows():
    from sketchml_amd.data import DataSet
    from sketchml_amd.exceptions import SketchMLException
    for bad in ([(1.0, [2, 1], [1.0, 1.0])], [(1.0, [1, 1], [1.0, 1.0])], [(1.0, [3], [1.0])], [(1.0, [-1], [1.0])]):
        with pytest.raises(SketchMLException):
            DataSet.fromRows(bad, 3, device="cpu")._build()
    # a row may end on a column above the next row's first one
    DataSet.fromRows([(1.0, [2], [1.0]), (1.0, [0], [1.0])], 3, device="cpu")._build()
    csr = DataSet.fromCSR(np.array([0, 1, 3]), np.array([2, 0, 1]), np.array([1.0, 2.0, 3.0]), np.array([1.0, -1.0]), 3,
                          device="cpu")
    csr._build()
    assert csr.size == 2 and csr.csc_row.tolist() == [1, 1, 0]


def test_to_auto_threshold():
    """dense iff nnz > dim * 2 / 3 in Java int arithmetic: dim = 30 -> 20 stays sparse, 21 is dense."""
    g = np.zeros(30)
    g[:20] = 1.0
    g[25] = 1e-8  # |g| > 1e-8 is strict
    assert R.count_nnz(g) == 20 and R.to_auto(g)[0] == "sparse"
    g[20] = -2e-8
    form, keys, vals = R.to_auto(g)
    assert R.count_nnz(g) == 21 and form == "dense" and keys is None and len(vals) == 30
    from sketchml_amd.gradient import auto_dense
    for nnz, dim in [(20, 30), (21, 30), (0, 1), (1, 1), (3, 5), (4, 5), (1, 1073741824)]:
        assert auto_dense(nnz, dim) == R.auto_dense(nnz, dim)
    assert R.auto_dense(1, 1073741824)  # dim * 2 wraps to a negative int


def test_l2_on_the_sparse_form_leaves_dropped_keys_alone():
    g = np.array([4.0, 5e-9, 0.0, -8.0])
    w = np.array([1.0, 1.0, 1.0, 1.0])
    form, keys, vals = R.to_auto(g)
    assert form == "sparse" and keys.tolist() == [0, 3]
    out = R.finish(keys, vals, 0.5, R.REG_L2, 0.25, w)
    assert out.tolist() == [2.25, -3.75]  # keys 1 and 2 get no w * lambda: they are not in the gradient
    dense = R.finish(None, g, 0.5, R.REG_L2, 0.25, w)
    assert dense.tolist() == [2.25, 2.5e-9 + 0.25, 0.25, -3.75]


def test_l1_as_written():
    theta = 0.5
    v = np.array([-0.0, 0.0, 0.5, _up(0.5), -0.5, _down(-0.5), 0.25, -0.25, np.nan])
    out = R.finish(None, v, 1.0, R.REG_L1, theta, None)
    assert R.bits(out[:1])[0] == 0  # Math.max(-0.0 - 0, 0) is +0.0
    assert np.array_equal(R.bits(out[1:]), R.bits(v[1:]))  # the identity everywhere else


def test_parsers():
    from sketchml_amd import data as D
    from sketchml_amd.exceptions import SketchMLException
    assert D.parseLibSVM(" 1 3:0.5 10:-2e-3 \n", 20) == (1.0, [3, 10], [0.5, -0.002])
    assert D.parseLibSVM("0 1:1", 20) == (-1.0, [1], [1.0])            # negY: anything but 1 is -1
    assert D.parseLibSVM("0.5 1:1", 20, negY=False) == (0.5, [1], [1.0])
    assert D.parseLibSVM("1.000000001 4:2", 20)[0] == 1.000000001      # |y - 1| <= 1e-8 keeps y
    assert D.parseLibSVM("-1", 20) == (-1.0, [], [])
    assert D.parseDummy("1, 3, 7,9", 20) == (1.0, [3, 7, 9], [1.0, 1.0, 1.0])
    assert D.parseDummy("2,5", 20) == (-1.0, [5], [1.0])
    with pytest.raises(SketchMLException, match="not built here"):
        D.parseCSV("1,0.5,0.25", 2)
    ds = D.DataSet.fromRows([D.parseLibSVM("1 0:2 2:3", 3), D.parseDummy("0,1", 3)], 3, device="cpu")
    assert ds.loopingRead() == (1.0, [0, 2], [2.0, 3.0]) and ds.loopingRead() == (-1.0, [1], [1.0])


def test_abi_surface():
    import sketchml_amd as sk
    from sketchml_amd import _lib
    names = ("skml_glm_gradient_f64", "skml_glm_gradient_f32", "skml_glm_finish_dense_f64", "skml_glm_finish_kv_f64")
    for n in names:
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n)
    assert _lib._SIGS[names[0]] == _lib._SIGS[names[1]]
    assert (_lib.SKML_LOSS_L1_LOG, _lib.SKML_LOSS_L2_HINGE, _lib.SKML_LOSS_L2_LOG, _lib.SKML_LOSS_L2_SQUARE) == (
        R.L1_LOG, R.L2_HINGE, R.L2_LOG, R.L2_SQUARE)
    assert (_lib.SKML_REG_NONE, _lib.SKML_REG_L1, _lib.SKML_REG_L2) == (R.REG_NONE, R.REG_L1, R.REG_L2)
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for name, value in (("LOSS_L1_LOG", 0), ("LOSS_L2_HINGE", 1), ("LOSS_L2_LOG", 2), ("LOSS_L2_SQUARE", 3),
                        ("REG_NONE", 0), ("REG_L1", 1), ("REG_L2", 2), ("K_GLM_PREDICT", 7), ("K_GLM_PLUS_BY", 8),
                        ("K_GLM_FINISH", 9)):
        assert f"#define SKML_{name} {value}" in text and getattr(_lib, f"SKML_{name}") == value
    import ctypes as C
    assert C.sizeof(_lib.GlmData) == 80
    for n in ("DataSet", "parseLibSVM", "parseDummy", "parseCSV", "L1LogLoss", "L2HingeLoss", "L2LogLoss", "L2SquareLoss",
              "GradientDescent", "Adam"):
        assert n in sk.__all__ and hasattr(sk, n)
    assert hasattr(sk.GradientDescent, "miniBatchGradientDescent") and hasattr(sk.Adam, "miniBatchGradientDescent")


def test_mini_batch_refuses_an_empty_or_oversized_batch():
    """batchSize == 0 divides by zero in the reference and batchSpRatio > 1 reads an instance twice: both
    are refused before anything is read (no GPU is needed to get there)."""
    import torch

    import sketchml_amd as sk
    ds = sk.DataSet.fromRows([(1.0, [0], [1.0])] * 3, 2, device="cpu")
    for ratio in (0.1, 1.5):
        opt = sk.GradientDescent(2, 0.1, 0.0, ratio)
        with pytest.raises(sk.SketchMLException, match="batchSpRatio"):
            opt.miniBatchGradientDescent(torch.zeros(2, dtype=torch.float64), ds, sk.L2LogLoss(0.0))
        assert ds.readIndex == 0 and opt.batch == 0


def test_fixture_sums_depend_on_the_order():
    """For at least half of the fixture's columns with 64 or more window entries, the terms summed in
    reverse give other bits than plusBy's order, and so do the terms summed pairwise: a kernel that
    adds in another order cannot pass the GPU comparison."""
    data, dim = FX.bias_data()
    rows, _ = R.window_rows(700, 500, 600)
    w = FX.weights(dim)
    _, coef, _ = R.predict(data, w, rows, R.L2_LOG)
    terms = {k: ts for k, ts in R.column_terms(data, rows, coef).items() if len(ts) >= 64}
    assert len(terms) >= 30 and len(terms[0]) == 600
    fwd = {k: R.sum_forward(ts) for k, ts in terms.items()}
    rev = sum(1 for k, ts in terms.items() if R.bits([R.sum_reverse(ts)])[0] != R.bits([fwd[k]])[0])
    pair = sum(1 for k, ts in terms.items() if R.bits([R.sum_pairwise(ts)])[0] != R.bits([fwd[k]])[0])
    print(f"{len(terms)} columns with >= 64 entries: reversed differs in {rev}, pairwise in {pair}")
    assert 2 * rev >= len(terms) and 2 * pair >= len(terms)
    # the fixtures reach every branch of the log losses and both sides of the hinge
    pre, _, _ = R.predict(data, w, rows, R.L2_LOG)
    z = pre * data[3][rows]
    assert (z > 18).any() and (z < -18).any() and ((z >= -18) & (z <= 18)).sum() >= 20
    assert (z < 1).any() and (z > 1).any()


def test_window_split_and_column_walk_on_the_host_under_sanitizers():
    """tests/glm_check.cpp: skml_glm.hpp's window split, binary searches and ordered column walk
    against a scatter in CSR order over 1,350 windows (random, wrapped, full, one row), built with
    -fsanitize=address,undefined and run as a program of its own."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok 1350 windows", out.stdout + out.stderr
