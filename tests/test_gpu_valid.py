"""The validation pass on the device (skml_glm_validate_*, skml_auc_rank_sum, skml_glm_seq_sum,
validation.calLossPrecision / calLossAucPrecision, miniBatchGradientDescent(sequentialLoss=True) and the
training loop of sketchml_amd/model.py) against tests/glm_ref.py, tests/optim_ref.py and
tests/valid_ref.py, bit for bit wherever Java pins the bits:

- pre for every loss, loss_i for the hinge and the square loss, the four counts, M, N and sigma;
- loss_i of the log losses to |loss - ref| <= 2^-50 (1 + |ref|), the bound of tests/test_gpu_glm.py:
  Math.exp / Math.log, numpy's and the device's are each within 1 ulp;
- validLoss against the forward sum of the device's own loss_i for every loss, which pins the order
  whatever the libm; with SKML_VALID_TREE_SUM against the tree restatement;
- the sorted permutation against the stable order of the keys, and against the restated quicksort
  of the reference where no two scores are within 2e-11 (tests/test_valid_cpu.py asserts on which
  fixtures that holds, and that the two loss sums differ where this file says they do)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import glm_fixtures as FX
import glm_ref as R
import optim_ref as O
import valid_ref as V
from test_valid_cpu import FIXTURES, ORDER_PAIRS, raw

pytestmark = pytest.mark.gpu

AUC, TREE = 1, 2
KINDS = [R.L1_LOG, R.L2_HINGE, R.L2_LOG, R.L2_SQUARE]


def _L():
    from sketchml_amd import _lib
    return _lib


def _h():
    from sketchml_amd.context import get_context
    return get_context().handle


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    bad = np.nonzero(R.bits(got) != R.bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, the first at {bad[0]}: {got[bad[0]]!r} against {want[bad[0]]!r}"


def _loss(kind, lam=0.0):
    from sketchml_amd import loss as Lo
    return {R.L1_LOG: Lo.L1LogLoss, R.L2_HINGE: Lo.L2HingeLoss, R.L2_LOG: Lo.L2LogLoss, R.L2_SQUARE: Lo.L2SquareLoss}[kind](lam)


@functools.lru_cache(maxsize=None)
def _dataset(name):
    from sketchml_amd.data import DataSet
    data, dim = raw(name)
    return DataSet.fromCSR(*data, dim, device="cuda")


@functools.lru_cache(maxsize=None)
def _weights(name, dt):
    return FX.weights(raw(name)[1]).astype(np.float32 if dt == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def _predicted(name, dt, kind):
    data = raw(name)[0]
    pre, _, loss = R.predict(data, _weights(name, dt), list(range(len(data[3]))), kind)
    return pre, loss


def _validate(ds, kind, w, flags, keep=True):
    L = _L()
    n = ds.size
    pre = torch.full((n,), -7.0, dtype=torch.float64, device="cuda") if keep else None
    loss = torch.full((n,), -7.0, dtype=torch.float64, device="cuda") if keep else None
    res = L.ValidResult()
    d = ds.glm_data()
    fn = L.lib.skml_glm_validate_f64 if w.dtype == torch.float64 else L.lib.skml_glm_validate_f32
    st = fn(_h(), C.byref(d), kind, _ptr(w), flags, _ptr(pre), _ptr(loss), C.byref(res))
    assert st == 0, L.last_error()
    return res, pre, loss


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_validate_on_the_fixtures(gpu, name, kind, dt):
    ds, y = _dataset(name), raw(name)[0][3]
    w = torch.from_numpy(_weights(name, dt)).cuda()
    r_pre, r_loss = _predicted(name, dt, kind)
    res, pre, loss = _validate(ds, kind, w, AUC)
    d_pre, d_loss = pre.cpu().numpy(), loss.cpu().numpy()
    _same(d_pre, r_pre, "pre")
    if kind in (R.L2_HINGE, R.L2_SQUARE):
        _same(d_loss, r_loss, "loss")
    else:
        el = np.abs(d_loss - r_loss) / (1.0 + np.abs(r_loss))
        print(f"log loss against numpy: off by {el.max() * 2.0 ** 52:.3f} x 2^-52 (1 + |ref|)")
        assert np.all(np.abs(d_loss - r_loss) <= 2.0 ** -50 * (1.0 + np.abs(r_loss))), "loss of a log loss"
    want = V.cal_loss_precision(r_pre, d_loss, y)
    assert (res.true_pos, res.true_neg, res.false_pos, res.false_neg, res.num) == want[1:]
    assert res.true_pos + res.true_neg + res.false_pos + res.false_neg <= res.num and res.nan_scores == 0
    _same([res.loss], [want[0]], "validLoss against the forward sum of the device's losses")
    # the AUC stage: the stable order of the keys; the reference's own sort where it is defined
    sigma, M, N = V.rank_sum(y[V.stable_order(r_pre)])
    assert (res.rank_sum, res.pos, res.neg) == (sigma, M, N)
    if V.min_gap(r_pre) > 2e-11:
        assert V.rank_sum(V.quick_sort(r_pre, y)[1]) == (sigma, M, N)
    # the fixed tree instead, the stand-in buffers, and no AUC
    tree, _, _ = _validate(ds, kind, w, TREE, keep=False)
    _same([tree.loss], [V.sum_tree(d_loss)], "validLoss with SKML_VALID_TREE_SUM")
    assert (tree.true_pos, tree.true_neg, tree.false_pos, tree.false_neg, tree.num) == want[1:]
    assert (tree.pos, tree.neg, tree.rank_sum) == (0, 0, 0)
    bare, _, _ = _validate(ds, kind, w, AUC, keep=False)
    assert (bare.rank_sum, bare.pos, bare.neg) == (sigma, M, N)
    _same([bare.loss], [want[0]], "validLoss with the context's buffers")
    if dt == "f64" and kind in (R.L2_HINGE, R.L2_SQUARE) and (name, kind) in ORDER_PAIRS:
        assert R.bits([res.loss])[0] != R.bits([tree.loss])[0]  # the two orders are told apart on this pair


def _edge_set(labels, with_nan):
    """Rows over four features with w = [1e-200, 2, -3, NaN]: pre = 1e-200, 2, 0 (empty), 2, -3, 2, -3 and,
    with_nan, NaN."""
    from sketchml_amd.data import DataSet
    rows = [[0], [1], [], [1], [2], [1], [2]] + ([[3]] if with_nan else [])
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    return DataSet.fromCSR(row_ptr, col, np.ones(len(col)), np.asarray(labels[:len(rows)], dtype=np.float64), 4, device="cuda")


def test_classification_edges(gpu):
    import sketchml_amd as sk
    w = torch.tensor([1e-200, 2.0, -3.0, math.nan], dtype=torch.float64, device="cuda")
    pre = [1e-200, 2.0, 0.0, 2.0, -3.0, 2.0, -3.0, math.nan]
    # an underflowing product, a zero label, an empty row, a negative product with pre > 0, falseNeg, truePos, trueNeg
    labels = [1e-200, 0.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0]
    r = sk.calLossAucPrecision(w, _edge_set(labels, False), sk.L2HingeLoss(0.0))
    _same(r.pre.cpu().numpy(), pre[:7], "pre")
    assert r[1:] == (1, 1, 1, 1, 7) and r.nanScores == 0
    hinge = [float(R.loss_of(R.L2_HINGE, p, y)) for p, y in zip(pre[:7], labels)]
    _same(r.loss.cpu().numpy(), hinge, "loss")
    _same([r[0]], [V.sum_forward(hinge)], "validLoss")
    order = V.stable_order(np.array(pre[:7]))
    assert (r.sigma, r.M, r.N) == V.rank_sum(np.array(labels[:7])[order]) and r.M == 3  # 1e-200 and 0.0 are not 1.0
    assert r.auc == V.auc(r.sigma, r.M, r.N) and (r.precision, r.trueRecall, r.falseRecall) == (2.0 / 7, 0.5, 0.5)
    # a NaN weight: no counter moves for its row, the flag is up, the AUC is NaN
    r = sk.calLossAucPrecision(w, _edge_set(labels, True), sk.L2HingeLoss(0.0))
    assert r[1:] == (1, 1, 1, 1, 8) and r.nanScores == 1 and math.isnan(r.auc) and math.isnan(float(r.pre[7]))
    r = sk.calLossPrecision(w, _edge_set(labels, True), sk.L2HingeLoss(0.0))
    assert r[1:] == (1, 1, 1, 1, 8) and r.nanScores == 1 and r.auc is None and r.sigma is None
    # labels of 0 / 1 form: only == 1.0 counts as positive; a zero label moves no counter
    labels01 = [0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0]
    r = sk.calLossAucPrecision(w, _edge_set(labels01, False), sk.L2SquareLoss(0.0))
    assert r[1:] == (2, 0, 0, 1, 7) and (r.M, r.N) == (4, 3)
    assert r.sigma == V.rank_sum(np.array(labels01)[order])[0]
    assert r == V.cal_loss_precision(pre[:7], r.loss.cpu().numpy(), labels01)


SEQ_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 70001)


@functools.lru_cache(maxsize=None)
def _seq_values():
    rng = np.random.default_rng(4)
    return {n: rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n).astype(np.float64)) for n in SEQ_SIZES}


@pytest.mark.parametrize("n", SEQ_SIZES)
def test_ordered_sum(gpu, n):
    from sketchml_amd.validation import seq_sum
    x = _seq_values()[n]
    fwd = V.sum_forward(x)
    if n >= 63:
        assert R.bits([fwd])[0] != R.bits([V.sum_forward(x[::-1])])[0]  # another order gives other bits
    _same([seq_sum(torch.from_numpy(x).cuda())], [fwd], f"the ordered sum of {n}")


AUC_SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 24581)


@functools.lru_cache(maxsize=None)
def _distinct(n):
    """permutation(n) * 1e-6 - 0.01 and labels 40 % positive, default_rng(3) drawing in that order."""
    rng = np.random.default_rng(3)
    s = rng.permutation(n) * 1e-6 - 0.01
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    stable = V.stable_order(s)
    return s, y, stable, V.rank_sum(y[stable]), V.rank_sum(V.quick_sort(s, y)[1])


def _auc(s, y, want_order=True):
    from sketchml_amd.validation import auc_rank_sum
    return auc_rank_sum(torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda(), want_order)


@pytest.mark.parametrize("n", AUC_SIZES)
def test_rank_sum_of_distinct_scores(gpu, n):
    s, y, stable, want, quick = _distinct(n)
    assert want == quick
    if n == 24581:
        assert want[0] == 119295561
    got = _auc(s, y)
    assert np.array_equal(got["order"].cpu().numpy(), stable.astype(np.int32))
    assert (got["sigma"], got["M"], got["N"], got["nanScores"]) == want + (0,)
    a, b = got["auc"], V.auc(*want)
    assert (math.isnan(a) and math.isnan(b)) or a == b
    assert _auc(s, y, want_order=False)["sigma"] == want[0]


@pytest.mark.parametrize("n", AUC_SIZES)
def test_rank_sum_under_the_tie_rule(gpu, n):
    """+-0.0, +-infinity, denormals and long runs of one value, one run of more than 1,024 slots (a
    scatter step) wherever n has room for it: the order is the keys', equal keys in instance order."""
    rng = np.random.default_rng(1000 + n)
    pool = np.array([0.0, -0.0, math.inf, -math.inf, 5e-324, -5e-324, 1e-310, -1e-310, 0.25, 0.25, -1.5, 3.0])
    s = pool[rng.integers(0, len(pool), n)]
    if n >= 1025:
        run = min(n, 1500)
        at = (n - run) // 2
        s[at:at + run] = 0.25
        assert run > 1024
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    stable = V.stable_order(s)
    got = _auc(s, y)
    assert np.array_equal(got["order"].cpu().numpy(), stable.astype(np.int32))
    assert (got["sigma"], got["M"], got["N"], got["nanScores"]) == V.rank_sum(y[stable]) + (0,)


def test_auc_with_one_class_and_with_a_nan(gpu):
    s = _distinct(1025)[0]
    got = _auc(s, np.ones(1025))
    assert (got["M"], got["N"], got["sigma"]) == (1025, 0, 1025 * 1024 // 2) and got["auc"] == V.auc(got["sigma"], 1025, 0) == -math.inf
    got = _auc(s, -np.ones(1025))
    assert (got["M"], got["N"], got["sigma"]) == (0, 1025, 0) and math.isnan(got["auc"]) and math.isnan(V.auc(0, 0, 1025))
    got = _auc(s[:7], np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0])[np.argsort(np.argsort(s[:7]))])  # the negative sorts last
    assert got["auc"] == V.auc(got["sigma"], 6, 1) and got["sigma"] == 15
    t = s.copy()
    t[[3, 700]] = math.nan
    got = _auc(t, np.ones(1025))
    assert got["nanScores"] == 2 and math.isnan(got["auc"])


def test_python_entries(gpu):
    import sketchml_amd as sk
    name = "bias"
    ds, y = _dataset(name), raw(name)[0][3]
    w = torch.from_numpy(_weights(name, "f64")).cuda()
    r_pre, r_loss = _predicted(name, "f64", R.L2_SQUARE)
    want = V.cal_loss_precision(r_pre, r_loss, y)
    r = sk.calLossPrecision(w, ds, sk.L2SquareLoss(0.0))
    assert isinstance(r, tuple) and r == want and r.auc is None and r.M is None
    assert (r.precision, r.trueRecall, r.falseRecall) == V.ratios(want)
    _same(r.pre.cpu().numpy(), r_pre, "pre")
    _same(r.loss.cpu().numpy(), r_loss, "loss")
    a = sk.calLossAucPrecision(w, ds, sk.L2SquareLoss(0.0))
    assert a == want and (a.sigma, a.M, a.N) == (122283, 346, 354) and a.auc == V.auc(122283, 346, 354)
    t = sk.calLossPrecision(w, ds, sk.L2SquareLoss(0.0), order="tree")
    assert t[1:] == want[1:] and t[0] == float(V.sum_tree(r_loss)) and t[0] != r[0]
    with pytest.raises(sk.SketchMLException):
        sk.calLossPrecision(w, ds, sk.L2SquareLoss(0.0), order="pairwise")
    # no positive label: truePos + falseNeg == 0, trueRecall is 0.0 / 0
    data, dim = raw("tiny")
    neg = sk.DataSet.fromCSR(data[0], data[1], data[2], -np.ones(len(data[3])), dim, device="cuda")
    r = sk.calLossAucPrecision(torch.from_numpy(FX.weights(dim)).cuda(), neg, sk.L2HingeLoss(0.0))
    assert r.truePos + r.falseNeg == 0 and math.isnan(r.trueRecall) and r.trueNeg + r.falsePos == 50
    assert r.falseRecall == r.trueNeg / 50 and r.precision == r.trueNeg / 50 and math.isnan(r.auc) and r.M == 0


@pytest.mark.parametrize("kind", [R.L2_LOG, R.L2_SQUARE])
def test_sequential_obj_loss(gpu, kind):
    import sketchml_amd as sk
    from sketchml_amd import optim
    from sketchml_amd.data import DataSet
    data, dim = FX.bias_data()
    w = torch.from_numpy(FX.weights(dim)).cuda()
    loss = _loss(kind)
    out = {}
    for seq in (False, True):
        ds = DataSet.fromCSR(*data, dim, device="cuda")
        opt = sk.GradientDescent(dim, 0.1, 0.5, 0.6)
        _, batch, obj, _ = opt.miniBatchGradientDescent(w, ds, loss, sequentialLoss=seq) if seq else opt.miniBatchGradientDescent(w, ds, loss)
        out[seq] = (obj, opt.lastLoss.cpu().numpy())
        assert batch == 420
    today = optim.batch_gradient(w, _dataset("bias"), 0, 420, loss)["objLoss"]
    assert R.bits([out[False][0]])[0] == R.bits([today])[0]  # the default keeps today's value
    _same(out[True][1], out[False][1], "lastLoss")
    _same([out[True][0]], [V.sum_forward(out[True][1])], "objLoss with sequentialLoss")
    if kind == R.L2_SQUARE:  # every bit of the square loss is pinned: the two sums differ on this batch
        assert R.bits([out[True][0]])[0] != R.bits([out[False][0]])[0]


def _restated_training(train, valid, dim, kind, conf):
    """GeneralizedLinearModel.scala:80-177 for one worker and compressor "None", from the restatements."""
    size, vsize = len(train[3]), len(valid[3])
    batch_size = int(size * conf.batchSpRatio)
    batch_num = int(math.ceil(1.0 / conf.batchSpRatio))
    opt = O.Adam(dim, conf.learnRate, conf.learnDecay, conf.batchSpRatio)
    w, m, v = np.zeros(dim), np.zeros(dim), np.zeros(dim)
    read = 0
    train_losses, valid_losses, last = [float(conf.epochNum)], [float(conf.epochNum)], None
    for _ in range(conf.epochNum):
        total = 0.0
        for _ in range(batch_num):
            rows, read = R.window_rows(size, read, batch_size)
            _, coef, loss = R.predict(train, w, rows, kind)
            form, keys, vals = R.to_auto(R.plus_by(train, dim, rows, coef))
            fin = R.finish(keys, vals, 1.0 / batch_size, R.REG_NONE, 0.0, w)
            opt.next_batch()
            total += float(V.sum_forward(loss)) / batch_size + 0.0 / conf.workerNum
            dense = np.zeros(dim)  # Gradient.sum: a zero DenseDoubleGradient plusBy the worker's gradient
            if form == "dense":
                dense = dense + fin
            else:
                dense[keys] = dense[keys] + fin
            form, keys, vals = R.to_auto(dense)
            vals = vals * np.float64(1.0 / conf.workerNum)
            opt.begin_update()
            if form == "dense":
                w, m, v = O.step(opt.params(), vals, w, m, v)
            else:
                w, m, v = O.step_kv(opt.params(), keys, vals, w, m, v)
        train_losses.append(total / batch_num)
        pre, _, loss = R.predict(valid, w, list(range(vsize)), kind)
        last = V.cal_loss_precision(pre, loss, valid[3])
        valid_losses.append(last[0] / vsize)
    return w, m, v, train_losses, valid_losses, last


def _split_tiny():
    data, dim = FX.tiny_data()
    row_ptr, col, val, label = data
    cut = int(row_ptr[40])
    train = (row_ptr[:41].copy(), col[:cut].copy(), val[:cut].copy(), label[:40].copy())
    valid = (row_ptr[40:] - cut, col[cut:].copy(), val[cut:].copy(), label[40:].copy())
    return train, valid, dim


@pytest.mark.parametrize("model,kind", [("SVMModel", R.L2_HINGE), ("LinearRegModel", R.L2_SQUARE)])
def test_training_loop_against_the_restatement(gpu, model, kind):
    import sketchml_amd as sk
    train, valid, dim = _split_tiny()
    conf = sk.MLConf(getattr(sk, model).name, "", "libsvm", 1, dim, epochNum=2, batchSpRatio=0.25, learnRate=0.1, l2Reg=0.0,
                     compressor="None")
    mdl = getattr(sk, model)(conf, sk.DataSet.fromCSR(*train, dim, device="cuda"), sk.DataSet.fromCSR(*valid, dim, device="cuda"))
    tl, vl, last = mdl.train()
    w, m, v, r_tl, r_vl, r_last = _restated_training(train, valid, dim, kind, conf)
    _same(mdl.weights.cpu().numpy(), w, "weights")
    _same(mdl.optimizer.m.cpu().numpy(), m, "m")
    _same(mdl.optimizer.v.cpu().numpy(), v, "v")
    _same(tl, r_tl, "trainLosses")
    _same(vl, r_vl, "validLosses")
    assert last == r_last and len(tl) == 3 and np.count_nonzero(w) > 0
    assert (mdl.optimizer.epoch, mdl.optimizer.batch, mdl.trainData.readIndex) == (2, 0, 40)


def test_training_loop_with_the_sketch_compressor(gpu):
    import sketchml_amd as sk
    train, valid, dim = _split_tiny()
    conf = sk.MLConf("LogisticRegression", "", "libsvm", 1, dim, epochNum=2, batchSpRatio=0.25, l2Reg=0.0, compressor="Sketch")
    mdl = sk.LRModel(conf, sk.DataSet.fromCSR(*train, dim, device="cuda"), sk.DataSet.fromCSR(*valid, dim, device="cuda"))
    tl, vl, last = mdl.train()
    assert len(tl) == len(vl) == 3 and all(math.isfinite(x) for x in tl + vl)
    assert last.validNum == 10 and 0 < last.truePos + last.trueNeg + last.falsePos + last.falseNeg <= 10
    assert vl[-1] == last[0] / 10 and bool(torch.isfinite(mdl.weights).all()) and bool((mdl.weights != 0).any())


def test_bad_arguments_leave_the_outputs_untouched(gpu):
    L, h = _L(), _h()
    ds = _dataset("bias")
    w = torch.from_numpy(_weights("bias", "f64")).cuda()
    mark = 123.456
    pre = torch.full((700,), mark, dtype=torch.float64, device="cuda")
    loss = torch.full((700,), mark, dtype=torch.float64, device="cuda")
    res = L.ValidResult()
    res.loss, res.num = -7.0, -7

    def call(data=None, kind=R.L2_LOG, wp=None, flags=AUC, p=None, l=None, fn="skml_glm_validate_f64", ctx=h, out=res):
        d = data if data is not None else ds.glm_data()
        return getattr(L.lib, fn)(ctx, C.byref(d), kind, wp if wp is not None else _ptr(w), flags, p if p is not None else _ptr(pre),
                                  l if l is not None else _ptr(loss), C.byref(out) if out is not None else None)

    def edited(**kw):
        d = ds.glm_data()
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731
    cases = {
        "ctx NULL": dict(ctx=None),
        "out NULL": dict(out=None),
        "row_ptr NULL": dict(data=edited(row_ptr=None)),
        "label NULL": dict(data=edited(label=None)),
        "val NULL": dict(data=edited(val=None)),
        "w NULL": dict(wp=C.c_void_p(0)),
        "val misaligned": dict(data=edited(val=ds.val.data_ptr() + 4)),
        "w misaligned": dict(wp=off4(w)),
        "pre misaligned": dict(p=off4(pre)),
        "loss misaligned": dict(l=off4(loss)),
        "dim beyond a Java int": dict(data=edited(dim=1 << 31)),
        "rows beyond a Java int": dict(data=edited(rows=1 << 31)),
        "rows 0": dict(data=edited(rows=0)),
        "dim 0": dict(data=edited(dim=0)),
        "nnz < 0": dict(data=edited(nnz=-1)),
        "unknown loss": dict(kind=4),
        "negative loss": dict(kind=-1),
        "unknown flag": dict(flags=4),
        "negative flags": dict(flags=-1),
        "pre is w": dict(p=_ptr(w)),
        "loss inside val": dict(l=_ptr(ds.val)),
        "loss is label": dict(l=_ptr(ds.label)),
        "pre is loss": dict(p=_ptr(loss)),
        "f32 entry, pre is w": dict(fn="skml_glm_validate_f32", p=_ptr(w)),
    }
    before = {k: getattr(ds, k).clone() for k in ("val", "label")}
    w_before = w.clone()
    for what, kw in cases.items():
        assert call(**kw) == L.SKML_E_ARG, f"{what}: {L.last_error()}"
        assert L.last_error(), what
    torch.cuda.synchronize()
    assert bool((pre == mark).all()) and bool((loss == mark).all()) and (res.loss, res.num) == (-7.0, -7)
    assert torch.equal(w, w_before) and all(torch.equal(getattr(ds, k), t) for k, t in before.items())
    # the column order is not read: NULLs there are accepted, and the same arguments made right
    assert call(data=edited(col_ptr=None, csc_row=None, csc_val=None)) == 0 and res.num == 700 and res.pos == 346
    # the AUC stage and the ordered sum alone
    s = torch.full((64,), 0.5, dtype=torch.float64, device="cuda")
    y = torch.ones(64, dtype=torch.float64, device="cuda")
    order = torch.full((64,), -5, dtype=torch.int32, device="cuda")
    pos, neg, nan, sig, total = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_uint64(7), C.c_double(-7.0)
    rs = L.lib.skml_auc_rank_sum
    refs = (C.byref(pos), C.byref(neg), C.byref(sig), C.byref(nan))
    assert rs(None, _ptr(s), _ptr(y), 64, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, None, _ptr(y), 64, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, _ptr(s), None, 64, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, _ptr(s), _ptr(y), 0, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, _ptr(s), _ptr(y), 1 << 31, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, off4(s), _ptr(y), 32, _ptr(order), *refs) == L.SKML_E_ARG
    assert rs(h, _ptr(s), _ptr(y), 64, C.c_void_p(order.data_ptr() + 2), *refs) == L.SKML_E_ARG
    assert rs(h, _ptr(s), _ptr(y), 64, _ptr(s), *refs) == L.SKML_E_ARG  # the permutation over the scores
    assert rs(h, _ptr(s), _ptr(y), 64, _ptr(order), None, C.byref(neg), C.byref(sig), C.byref(nan)) == L.SKML_E_ARG
    ss = L.lib.skml_glm_seq_sum
    assert ss(None, _ptr(s), 64, C.byref(total)) == L.SKML_E_ARG and ss(h, None, 64, C.byref(total)) == L.SKML_E_ARG
    assert ss(h, _ptr(s), 0, C.byref(total)) == L.SKML_E_ARG and ss(h, off4(s), 32, C.byref(total)) == L.SKML_E_ARG
    assert ss(h, _ptr(s), 64, None) == L.SKML_E_ARG
    torch.cuda.synchronize()
    assert bool((order == -5).all()) and bool((s == 0.5).all()) and (pos.value, neg.value, nan.value, sig.value, total.value) == (-7, -7, -7, 7, -7.0)
    assert rs(h, _ptr(s), _ptr(y), 64, _ptr(order), *refs) == 0
    assert (pos.value, neg.value, nan.value, sig.value) == (64, 0, 0, 63 * 64 // 2) and order.cpu().tolist() == list(range(64))
    assert ss(h, _ptr(s), 64, C.byref(total)) == 0 and total.value == 32.0
