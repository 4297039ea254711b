"""The mini-batch gradient of the reference restated in numpy float64 scalars, never fused, with
Python loops in the reference's order (ml/objective/GradientDescent.scala:23-87, Loss.scala:56-137,
ml/util/Maths.scala:57-69, ml/data/DataSet.scala:15-21, DenseDoubleGradient.scala:51-95): the dot, the
four losses, plusBy over the looping window, toAuto, timesBy and the two regularisers.

A data set here is (row_ptr, col, val, label) as numpy arrays.  Loss kinds and regulariser kinds are
the SKML_LOSS_* / SKML_REG_* ids of include/skml.h.
"""
import math

import numpy as np

F = np.float64
L1_LOG, L2_HINGE, L2_LOG, L2_SQUARE = 0, 1, 2, 3
REG_NONE, REG_L1, REG_L2 = 0, 1, 2
EPS = 1e-8


def window_rows(size, read_index, batch):
    """DataSet.loopingRead, batch times: ([rows], the readIndex afterwards)."""
    rows = []
    for _ in range(batch):
        if read_index >= size:
            read_index = 0
        rows.append(read_index)
        read_index += 1
    return rows, read_index


def dot(w, idx, val):
    """Maths.dot(DenseVector, SparseVector): a fp32 weight widens exactly."""
    acc = F(0.0)
    for i, v in zip(idx, val):
        acc = acc + F(w[i]) * F(v)
    return acc


def loss_of(kind, pre, y):
    pre, y = F(pre), F(y)
    with np.errstate(all="ignore"):
        if kind in (L1_LOG, L2_LOG):
            z = pre * y
            if z > 18:
                return np.exp(-z)
            if z < -18:
                return -z
            return np.log(F(1.0) + np.exp(-z))
        if kind == L2_HINGE:
            z = pre * y
            return F(1.0) - z if z < 1.0 else F(0.0)
        return F(0.5) * (pre - y) * (pre - y)


def grad_of(kind, pre, y):
    pre, y = F(pre), F(y)
    with np.errstate(all="ignore"):
        if kind in (L1_LOG, L2_LOG):
            z = pre * y
            if z > 18:
                return y * np.exp(-z)
            if z < -18:
                return y
            return y / (F(1.0) + np.exp(z))
        if kind == L2_HINGE:
            return y if pre * y <= 1.0 else F(0.0)
        return y - pre


def predict(data, w, rows, kind):
    """(pre, coef, loss) of the batch's instances: coef = -1.0 * loss.grad."""
    row_ptr, col, val, label = data
    pre, coef, loss = np.empty(len(rows)), np.empty(len(rows)), np.empty(len(rows))
    for j, r in enumerate(rows):
        s, e = int(row_ptr[r]), int(row_ptr[r + 1])
        pre[j] = dot(w, col[s:e], val[s:e])
        coef[j] = F(-1.0) * grad_of(kind, pre[j], label[r])
        loss[j] = loss_of(kind, pre[j], label[r])
    return pre, coef, loss


def column_terms(data, rows, coef):
    """{feature: [val * coef_j in batch order]}: what plusBy adds to each element, one after the other."""
    row_ptr, col, val, _ = data
    terms = {}
    for j, r in enumerate(rows):
        for i in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            terms.setdefault(int(col[i]), []).append(F(val[i]) * F(coef[j]))
    return terms


def sum_forward(ts):
    acc = F(0.0)
    for t in ts:
        acc = acc + t
    return acc


def sum_reverse(ts):
    return sum_forward(ts[::-1])


def sum_pairwise(ts):
    ts = list(ts)
    while len(ts) > 1:
        ts = [ts[i] + ts[i + 1] if i + 1 < len(ts) else ts[i] for i in range(0, len(ts), 2)]
    return ts[0] if ts else F(0.0)


def plus_by(data, dim, rows, coef):
    """denseGrad after the loop: dim values from +0.0."""
    g = np.zeros(dim)
    for k, ts in column_terms(data, rows, coef).items():
        g[k] = sum_forward(ts)
    return g


def _jint(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def count_nnz(g):
    return sum(1 for v in g if abs(v) > EPS)


def auto_dense(nnz, dim):
    return nnz > int(_jint(dim * 2) / 3)


def to_auto(g):
    """("dense", None, values) or ("sparse", keys, values) of the unscaled g."""
    nnz = count_nnz(g)
    if auto_dense(nnz, len(g)):
        return "dense", None, np.array(g, dtype=np.float64)
    keys = np.array([i for i, v in enumerate(g) if abs(v) > EPS], dtype=np.int32)
    return "sparse", keys, np.array([g[i] for i in keys], dtype=np.float64)


def java_max(a, b):
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0:
        return b
    return a if a >= b else b


def java_min(a, b):
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0:
        return b
    return a if a <= b else b


def finish(keys, values, times, reg, lam, w):
    """timesBy(times), then l1Reg(grad, 0, lam) or l2Reg(grad, w, lam) on the values; keys None: dense."""
    out = np.empty(len(values))
    times, lam, alpha = F(times), F(lam), F(0.0)
    for i, v in enumerate(values):
        v = F(v) * times
        if reg == REG_L1:
            if v >= 0 and v <= lam:
                v = F(java_max(v - alpha, F(0.0)))
            elif v < 0 and v >= -lam:
                v = F(java_min(v - alpha, F(0.0)))
        elif reg == REG_L2:
            k = i if keys is None else int(keys[i])
            v = v + F(w[k]) * lam
        out[i] = v
    return out


def reg_loss(reg, lam, w):
    """(terms, the exactly summed norm taken through sqrt and the product) of loss.getReg(w)."""
    w = np.asarray(w, dtype=np.float64)
    if reg == REG_L1:
        terms = np.abs(w)
        return terms, math.fsum(terms) * lam
    if reg == REG_L2:
        terms = w * w
        return terms, math.sqrt(math.fsum(terms)) * lam
    return np.zeros(0), 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
