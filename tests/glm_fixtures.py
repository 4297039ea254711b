"""The data sets the mini-batch gradient tests share (tests/test_glm_cpu.py, tests/test_gpu_glm.py):
built once, never modified.  Values and weights are normal draws times 2^e with e uniform in
[-20, 20] (values) or [-24, -4] (weights): sums of such terms depend on the order of their
additions, which tests/test_glm_cpu.py verifies for this very data, so a kernel that adds in
another order cannot pass the comparison with tests/glm_ref.py.
"""
import functools

import numpy as np

SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 200)


def _values(rng, n):
    return rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n).astype(np.float64))


def weights(dim, dtype=np.float64, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(dim) * np.exp2(rng.integers(-24, -3, dim).astype(np.float64))).astype(dtype)


def _csr(rows_cols, rng, dim, labels=None):
    row_ptr = np.zeros(len(rows_cols) + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum([len(c) for c in rows_cols])
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c in rows_cols] + [np.zeros(0, np.int32)])
    val = _values(rng, len(col))
    if labels is None:
        labels = np.where(rng.random(len(rows_cols)) < 0.5, 1.0, -1.0)
    assert all(np.all(np.diff(c) > 0) for c in rows_cols if len(c) > 1) and (len(col) == 0 or col.max() < dim)
    return row_ptr, col, val, np.asarray(labels, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def lengths_data(filler):
    """Rows of 0, 1, 63, 64, 65 and 200 entries (three of each, spread out) among filler rows whose
    mean length puts the data set's mean in one class of lanes per row: filler "short" (mean <= 4,
    one lane per row), "mid" (<= 32, 8 lanes), "long" (64 lanes).  Columns 0 and dim - 1 are used;
    most of the 5,000 columns are empty.  Returns (data, dim)."""
    rows, lo, hi = {"short": (700, 0, 5), "mid": (300, 8, 25), "long": (200, 60, 81)}[filler]
    dim = 5000
    rng = np.random.default_rng({"short": 11, "mid": 12, "long": 13}[filler])
    lens = rng.integers(lo, hi, rows)
    for t, at in enumerate(np.linspace(1, rows - 2, 3 * len(SPECIAL_LENGTHS)).astype(int)):
        lens[at] = SPECIAL_LENGTHS[t % len(SPECIAL_LENGTHS)]
    rows_cols = []
    for r, n in enumerate(lens):
        pool = 400 if r % 2 else dim  # half the rows share 400 columns, so columns collect several rows
        c = np.sort(rng.choice(pool, int(n), replace=False))
        if n >= 2 and r % 3 == 0:
            c[0], c[-1] = 0, dim - 1
        rows_cols.append(c)
    data = _csr(rows_cols, rng, dim)
    mean = len(data[1]) // rows
    assert {"short": mean <= 4, "mid": 4 < mean <= 32, "long": mean > 32}[filler], mean
    return data, dim


@functools.lru_cache(maxsize=None)
def bias_data():
    """700 rows over 3,000 columns: column 0 (the bias) in every row, 40 hot columns each in about
    half of the rows, column dim - 1 in every seventh row, a few of the others; most columns are
    empty.  A column's window length is the batch for the bias and about half of it for a hot column.
    Labels are +-1 with a few real ones (the square loss takes any).  Returns (data, dim)."""
    rows, dim = 700, 3000
    rng = np.random.default_rng(21)
    hot = 1 + 7 * np.arange(40)
    rows_cols = []
    for r in range(rows):
        c = {0} | {int(h) for h in hot[rng.random(40) < 0.5]} | {int(x) for x in rng.integers(300, dim - 1, 2)}
        if r % 7 == 0:
            c.add(dim - 1)
        rows_cols.append(np.array(sorted(c)))
    labels = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    labels[::50] = rng.standard_normal(len(labels[::50]))
    return _csr(rows_cols, rng, dim, labels), dim


@functools.lru_cache(maxsize=None)
def tiny_data():
    """50 rows over 30 columns, every column hit by every window of 20 rows or more: toAuto's dense side."""
    rows, dim = 50, 30
    rng = np.random.default_rng(31)
    rows_cols = [np.sort(rng.choice(dim, 12, replace=False)) for _ in range(rows)]
    return _csr(rows_cols, rng, dim), dim
