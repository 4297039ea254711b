"""The validation pass of the reference restated in numpy float64 scalars and pure Python, in the
reference's order (ml/util/ValidationUtil.scala:12-93, sketch/util/Sort.java:168-259,341-360):

- the classification of one instance and the six-tuple of calLossPrecision, fed per-instance
  predictions and losses (tests/glm_ref.py makes those);
- the derived ratios and the AUC formula in Java's double division;
- the device's order of the scores: the IEEE total-order key, equal keys in instance order;
- Sort.quickSort(double[], double[], from, to) with its 1e-11 comparator, med3 and selection sort,
  written from the algorithm;
- sigma, M and N from a sorted pair of arrays;
- the 1,024-thread tree of k_glm_loss_sum, for the order test.
"""
import math

import numpy as np

F = np.float64


def classify(pre, label):
    """0 none, 1 truePos, 2 trueNeg, 3 falsePos, 4 falseNeg (ValidationUtil.scala:23-29)."""
    pre, label = F(pre), F(label)
    with np.errstate(all="ignore"):
        z = pre * label
    if z > 0:
        return 1 if pre > 0 else 2
    if z < 0:
        return 3 if pre > 0 else 4
    return 0


def sum_forward(xs):
    acc = F(0.0)
    with np.errstate(all="ignore"):
        for x in xs:
            acc = acc + F(x)
    return acc


def sum_tree(xs, threads=1024):
    """k_glm_loss_sum: thread t adds x[t], x[t + threads], ... from +0.0, then a binary tree."""
    xs = np.asarray(xs, dtype=np.float64)
    part = np.zeros(threads)
    with np.errstate(all="ignore"):
        for t in range(min(threads, len(xs))):
            part[t] = sum_forward(xs[t::threads])
        st = threads // 2
        while st > 0:
            part[:st] = part[:st] + part[st:2 * st]
            st //= 2
    return F(part[0])


def cal_loss_precision(pre, loss, label):
    """(validLoss, truePos, trueNeg, falsePos, falseNeg, validNum) from the per-instance values."""
    counts = [0, 0, 0, 0, 0]
    for p, y in zip(pre, label):
        counts[classify(p, y)] += 1
    return (float(sum_forward(loss)), counts[1], counts[2], counts[3], counts[4], len(pre))


def java_div(a, b):
    with np.errstate(all="ignore"):
        return float(F(a) / F(b))


def ratios(t):
    """(precision, trueRecall, falseRecall) of a six-tuple (ValidationUtil.scala:33-35)."""
    _, tp, tn, fp, fn, num = t
    return java_div(1.0 * (tp + tn), num), java_div(1.0 * tp, tp + fn), java_div(1.0 * tn, tn + fp)


def key64(x):
    """Arrays.sort(double[])'s total order as uint64: -0.0 before +0.0, infinities ordinary."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def stable_order(scores):
    """The device's permutation: ascending by key, equal keys in instance order."""
    return np.argsort(key64(scores), kind="stable")


# ---- Sort.quickSort(double[] x, double[] y, int from, int to) ----
def _cmp(v, v1):
    if abs(v - v1) < 10e-12:
        return 0
    return 1 if v - v1 > 10e-12 else -1


def _swap(a, i, j):
    a[i], a[j] = a[j], a[i]


def _vec_swap(a, i, j, n):
    for _ in range(n):
        _swap(a, i, j)
        i += 1
        j += 1


def _med3(x, a, b, c):
    ab, ac, bc = _cmp(x[a], x[b]), _cmp(x[a], x[c]), _cmp(x[b], x[c])
    if ab < 0:
        return b if bc < 0 else (c if ac < 0 else a)
    return b if bc > 0 else (c if ac > 0 else a)


def _selection_sort(x, y, lo, hi):
    for i in range(lo, hi - 1):
        m = i
        for u in range(i + 1, hi):
            if _cmp(x[u], x[m]) < 0:
                m = u
        if m != i:
            _swap(x, i, m)
            _swap(y, i, m)


def _quick_sort(x, y, lo, hi):
    n = hi - lo
    if n < 7:
        _selection_sort(x, y, lo, hi)
        return
    m = lo + n // 2
    if n > 7:
        v, a = lo, hi - 1
        if n > 50:
            b = n // 8
            v = _med3(x, lo, lo + b, lo + 2 * b)
            m = _med3(x, m - b, m, m + b)
            a = _med3(x, a - 2 * b, a - b, a)
        m = _med3(x, v, m, a)
    seed = x[m]
    a = b = lo
    c = d = hi - 1
    while True:
        while b <= c:
            s = _cmp(x[b], seed)
            if s > 0:
                break
            if s == 0:
                _swap(x, a, b)
                _swap(y, a, b)
                a += 1
            b += 1
        while c >= b:
            s = _cmp(x[c], seed)
            if s < 0:
                break
            if s == 0:
                _swap(x, c, d)
                _swap(y, c, d)
                d -= 1
            c -= 1
        if b > c:
            break
        _swap(x, b, c)
        _swap(y, b, c)
        b += 1
        c -= 1
    s = min(a - lo, b - a)
    _vec_swap(x, lo, b - s, s)
    _vec_swap(y, lo, b - s, s)
    s = min(d - c, hi - d - 1)
    _vec_swap(x, b, hi - s, s)
    _vec_swap(y, b, hi - s, s)
    s = b - a
    if s > 1:
        _quick_sort(x, y, lo, lo + s)
    s = d - c
    if s > 1:
        _quick_sort(x, y, hi - s, hi)


def quick_sort(scores, labels):
    """The reference's sort of a copy of (scores, labels): two lists, scores "ascending" under the
    1e-11 comparator.  Scores must be finite (the comparator is all the reference has)."""
    import sys
    x, y = [float(v) for v in scores], [float(v) for v in labels]
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 20000))
    try:
        _quick_sort(x, y, 0, len(x))
    finally:
        sys.setrecursionlimit(old)
    return x, y


def rank_sum(sorted_labels):
    """(sigma, M, N) of ValidationUtil.scala:69-83 over the labels in sorted order; sigma is the exact
    integer (the reference's double sum is exact while n (n - 1) / 2 < 2^53)."""
    M = sum(1 for v in sorted_labels if v == 1.0)
    sigma = sum(i for i, v in enumerate(sorted_labels) if v == 1.0)
    return sigma, M, len(sorted_labels) - M


def auc(sigma, M, N):
    """(sigma - (M + 1) * M / 2) / M / N: the product and its halving in Long, the rest in double."""
    return java_div(java_div(float(sigma) - float((M + 1) * M // 2), float(M)), float(N))


def min_gap(scores):
    """The smallest gap between two neighbours of the sorted scores (0.0 when a score repeats)."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return float(np.min(np.diff(s))) if len(s) > 1 else math.inf
