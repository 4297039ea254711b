"""Host-side checks of the validation pass (no GPU): the restatement tests/valid_ref.py on hand-worked
cases, the conditions that tests/test_gpu_valid.py rests on asserted on the fixtures of
tests/glm_fixtures.py with w = FX.weights(dim) in float64, the host scalars of
sketchml_amd/validation.py and sketchml_amd/model.py, the ABI surface, and skml_valid.hpp's index
arithmetic as a stand-alone program (tests/valid_check.cpp) under the address and
undefined-behaviour sanitizers."""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import glm_fixtures as FX
import glm_ref as R
import valid_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXTURES = ("bias", "tiny", "short", "mid", "long")


def raw(name):
    return {"bias": FX.bias_data, "tiny": FX.tiny_data}[name]() if name in ("bias", "tiny") else FX.lengths_data(name)


@functools.lru_cache(maxsize=None)
def predicted(name, kind):
    """(pre, loss) of every row of a fixture at FX.weights(dim), float64."""
    data, dim = raw(name)
    pre, _, loss = R.predict(data, FX.weights(dim), list(range(len(data[3]))), kind)
    return pre, loss


# ---- the restatement ----
def test_classification_edges():
    assert [V.classify(p, y) for p, y in [(2.0, 1.0), (-2.0, -1.0), (2.0, -1.0), (-2.0, 1.0)]] == [1, 2, 3, 4]
    assert 1e-200 * 1e-200 == 0.0 and V.classify(1e-200, 1e-200) == 0  # the product underflows
    assert V.classify(3.0, 0.0) == 0 and V.classify(0.0, 1.0) == 0 and V.classify(-0.0, -1.0) == 0
    assert V.classify(math.nan, 1.0) == 0 and V.classify(1.0, math.nan) == 0 and V.classify(math.inf, 0.0) == 0
    assert V.classify(0.5, 0.25) == 1 and V.classify(-0.5, 0.25) == 4  # any real label, not only +-1
    t = V.cal_loss_precision([2.0, -2.0, 2.0, -2.0, 0.0, math.nan], [0.5, 0.25, 0.125, 1.0, 2.0, 0.0], [1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    assert t == (3.875, 1, 1, 1, 1, 6)
    assert V.ratios(t) == (2.0 / 6, 0.5, 0.5)


def test_ratios_follow_javas_division():
    p, tr, fr = V.ratios((0.0, 0, 3, 2, 0, 5))  # truePos + falseNeg == 0
    assert p == 0.6 and math.isnan(tr) and fr == 0.6
    p, tr, fr = V.ratios((0.0, 0, 0, 0, 0, 4))
    assert p == 0.0 and math.isnan(tr) and math.isnan(fr)
    assert V.java_div(1.0, 0) == math.inf and V.java_div(-1.0, 0) == -math.inf and math.isnan(V.java_div(0.0, 0))
    from sketchml_amd import validation as S
    for a, b in [(1.0, 0), (-1.0, 0), (0.0, 0), (3.0, 4), (math.nan, 0), (math.inf, 2), (1.0, -0.0)]:
        x, y = S.java_div(a, b), V.java_div(a, b)
        assert (math.isnan(x) and math.isnan(y)) or x == y, (a, b)
    r = S.ValidationResult(1.5, 0, 3, 2, 0, 5)
    assert r == (1.5, 0, 3, 2, 0, 5) and isinstance(r, tuple) and len(r) == 6
    assert r.precision == 0.6 and math.isnan(r.trueRecall) and r.falseRecall == 0.6
    assert r.auc is None and r.M is None and r.N is None and r.sigma is None
    assert (r.validLoss, r.truePos, r.trueNeg, r.falsePos, r.falseNeg, r.validNum) == tuple(r)


def test_auc_formula():
    # labels in sorted order: - + - + +  ->  positions 1, 3, 4: sigma = 8, M = 3, N = 2
    assert V.rank_sum([-1.0, 1.0, -1.0, 1.0, 1.0]) == (8, 3, 2)
    assert V.auc(8, 3, 2) == (8.0 - 6.0) / 3 / 2  # (M + 1) * M / 2 = 6 in Long
    assert V.auc(1, 2, 3) == (1.0 - 3.0) / 2 / 3
    assert V.rank_sum([0.0, 1.0, 2.0, 1.0]) == (4, 2, 2)  # 0 / 1 labels: only == 1.0 is positive
    assert math.isnan(V.auc(0, 0, 5))                      # no positive: 0.0 / 0
    assert V.auc(10, 5, 0) == -math.inf and V.auc(20, 5, 0) == math.inf and math.isnan(V.auc(15, 5, 0))
    from sketchml_amd import validation as S
    for s, m, n in [(8, 3, 2), (0, 0, 5), (10, 5, 0), (20, 5, 0), (15, 5, 0), (119295561, 9747, 14834)]:
        a, b = S.auc_of(s, m, n), V.auc(s, m, n)
        assert (math.isnan(a) and math.isnan(b)) or a == b


def test_key_order_and_tie_rule():
    x = np.array([0.0, -0.0, 1.0, -math.inf, 5e-324, -5e-324, math.inf, 0.0, -0.0, 1.0])
    o = V.stable_order(x)
    assert o.tolist() == [3, 5, 1, 8, 0, 7, 4, 2, 9, 6]  # -0.0 before +0.0, equal keys in instance order
    k = V.key64(x)
    assert np.all(np.diff(k[o].astype(object)) >= 0)


def test_quicksort_restatement_on_separated_scores():
    """With every gap above 1e-11 the comparator is a total order and the reference's sort is the sort."""
    rng = np.random.default_rng(17)
    for n in (0, 1, 2, 6, 7, 8, 40, 50, 51, 300, 2000):
        s = rng.permutation(n) * 1e-3 - 0.4
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        qs, ql = V.quick_sort(s, y)
        o = np.argsort(s, kind="stable")
        assert qs == s[o].tolist() and ql == y[o].tolist(), n
    # the comparator is not transitive: a ~ b and b ~ c although a < c
    a, b, c = 0.0, 0.7e-11, 1.4e-11
    assert V._cmp(a, b) == 0 and V._cmp(b, c) == 0 and V._cmp(a, c) == -1


# ---- the conditions the GPU tests rest on ----
@pytest.mark.parametrize("name,sigma,M", [("bias", 122283, 346), ("tiny", 635, 23)])
def test_fixtures_without_near_ties_sort_as_the_reference(name, sigma, M):
    pre, _ = predicted(name, R.L2_HINGE)
    y = raw(name)[0][3]
    assert V.min_gap(pre) > 2e-11
    stable = V.rank_sum(y[V.stable_order(pre)])
    quick = V.rank_sum(V.quick_sort(pre, y)[1])
    assert stable == quick == (sigma, M, len(y) - M)


def test_short_fixture_has_ties_and_the_two_orders_differ():
    pre, _ = predicted("short", R.L2_HINGE)
    y = raw("short")[0][3]
    assert int((pre == 0.0).sum()) == 156
    assert int((np.diff(np.sort(pre)) <= 2e-11).sum()) == 179
    qs, ql = V.quick_sort(pre, y)
    stable, quick = V.rank_sum(y[V.stable_order(pre)]), V.rank_sum(ql)
    assert (stable[0], quick[0]) == (131985, 131883) and stable[1:] == quick[1:]
    assert any(qs[i] > qs[i + 1] for i in range(len(qs) - 1))  # the reference's output does not even ascend


def test_large_synthetic_case():
    """permutation(n) * 1e-6 - 0.01 at n = 24,581, default_rng(3) drawing the permutation, then the labels."""
    rng = np.random.default_rng(3)
    n = 24581
    s = rng.permutation(n) * 1e-6 - 0.01
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    assert V.min_gap(s) > 2e-11
    assert V.rank_sum(y[V.stable_order(s)])[0] == V.rank_sum(V.quick_sort(s, y)[1])[0] == 119295561


# the (fixture, loss) pairs whose forward sum differs from the 1,024-thread tree of k_glm_loss_sum
ORDER_PAIRS = [(n, k) for n in ("short", "mid", "long") for k in (R.L2_LOG, R.L2_HINGE, R.L2_SQUARE)] + [
    ("bias", R.L2_SQUARE), ("bias", R.L2_LOG), ("tiny", R.L2_SQUARE)]
SAME_PAIRS = [("bias", R.L2_HINGE), ("tiny", R.L2_HINGE), ("tiny", R.L2_LOG)]


def test_loss_sums_depend_on_the_order():
    for name, kind in ORDER_PAIRS:
        _, loss = predicted(name, kind)
        assert R.bits([V.sum_forward(loss)])[0] != R.bits([V.sum_tree(loss)])[0], (name, kind)
    for name, kind in SAME_PAIRS:  # and where they do not, the order test learns nothing: it leaves these out
        _, loss = predicted(name, kind)
        assert R.bits([V.sum_forward(loss)])[0] == R.bits([V.sum_tree(loss)])[0], (name, kind)
    x = np.arange(1.0, 3000.0)
    assert V.sum_tree(x) == V.sum_forward(x) == 2999 * 3000 / 2  # exact sums agree in any order


# ---- the Python surface ----
def test_abi_surface():
    import ctypes as C

    import sketchml_amd as sk
    from sketchml_amd import _lib
    names = ("skml_glm_validate_f64", "skml_glm_validate_f32", "skml_auc_rank_sum", "skml_glm_seq_sum")
    for n in names:
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n)
    assert _lib._SIGS[names[0]] == _lib._SIGS[names[1]]
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for name, value in (("VALID_AUC", 1), ("VALID_TREE_SUM", 2), ("K_GLM_VALID", 10), ("K_SEQ_SUM", 11), ("K_VALID_SORT", 12),
                        ("K_VALID_RANK", 13)):
        assert f"#define SKML_{name} {value}" in text and getattr(_lib, f"SKML_{name}") == value
    assert C.sizeof(_lib.ValidResult) == 80
    for n in ("calLossPrecision", "calLossAucPrecision", "ValidationResult", "MLConf", "GeneralizedLinearModel", "LRModel",
              "SVMModel", "LinearRegModel", "validation", "model"):
        assert n in sk.__all__ and hasattr(sk, n)
    import inspect
    assert inspect.signature(sk.GradientDescent.miniBatchGradientDescent).parameters["sequentialLoss"].default is False
    assert inspect.signature(sk.calLossPrecision).parameters["order"].default == "sequential"


def test_mlconf_and_the_one_worker_limit():
    import sketchml_amd as sk
    c = sk.MLConf("LogisticRegression", "in", "libsvm", 1, 10)
    assert (c.validRatio, c.epochNum, c.batchSpRatio, c.learnRate, c.learnDecay, c.l1Reg, c.l2Reg) == (0.25, 100, 0.1, 0.1, 0.9, 0.1, 0.1)
    assert (c.compressor, c.quantBinNum, c.sketchGroupNum, c.sketchRowNum, c.sketchColRatio, c.fixedPointBitNum) == (
        "Sketch", 256, 8, 2, 0.3, 8)
    for kw, msg in ((dict(algo="KMeans"), "Unsupported algorithm"), (dict(format="parquet"), "Unrecognizable file format"),
                    (dict(compressor="sketch"), "Unrecognizable gradient compressor")):
        args = dict(algo="LogisticRegression", input="in", format="libsvm", workerNum=1, featureNum=10)
        args.update(kw)
        with pytest.raises(sk.SketchMLException, match=msg):
            sk.MLConf(**args)
    ds = sk.DataSet.fromRows([(1.0, [0], [1.0])] * 3, 10, device="cpu")
    with pytest.raises(sk.SketchMLException, match="not built here"):
        sk.SVMModel(sk.MLConf("SupportVectorMachine", "in", "libsvm", 2, 10), ds, ds)
    assert [m.name for m in (sk.LRModel, sk.SVMModel, sk.LinearRegModel)] == ["LogisticRegression", "SupportVectorMachine",
                                                                             "LinearRegression"]


def test_a_host_weight_is_refused_before_the_device():
    import torch

    import sketchml_amd as sk
    ds = sk.DataSet.fromRows([(1.0, [0], [1.0])] * 3, 2, device="cpu")
    with pytest.raises(sk.SketchMLException):
        sk.calLossPrecision(torch.zeros(2, dtype=torch.float64), ds, sk.L2LogLoss(0.0))  # a host weight


def test_index_arithmetic_on_the_host_under_sanitizers():
    """tests/valid_check.cpp: skml_valid.hpp's classification, the ordered sum's chunk walk and the
    scatter's offsets, built with -fsanitize=address,undefined and run as a program of its own."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "valid_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "valid_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok 20 classes 17 sums 36 sorts", out.stdout + out.stderr
