"""The optimiser update restated in numpy, the reference of tests/test_optim_cpu.py and
tests/test_gpu_optim.py.  Every operation is a float64 numpy ufunc (IEEE, correctly rounded, never
fused), in the reference's order:

- ml/objective/GradientDescent.scala:104-109 (dense) and :111-117 (sparse): w(i) -= g(i) * lr, with
  lr = lr_0 / Math.sqrt(1.0 + decay * epoch) (:91);
- ml/objective/Adam.scala:50-61 (dense) and :63-77 (sparse):
      m_t = beta1 * m(i) + (1 - beta1) * g(i)
      v_t = beta2 * v(i) + (1 - beta2) * g(i) * g(i)
      newGrad = (Math.sqrt(1 - beta2_t) * m_t) / ((1 - beta1_t) * (Math.sqrt(v_t) + Maths.EPS))
      w(i) -= newGrad * lr ; m(i) = m_t ; v(i) = v_t
  with beta1_t *= beta1, beta2_t *= beta2 when epoch > 0 && batch == 0 (:29-32) and lr = lr_0 (:39-45);
- ml/gradient/DenseDoubleGradient.scala:64-95: toSparse keeps Math.abs(x) > Maths.EPS, toAuto is
  dense iff nnz > dim * 2 / 3 in Java int arithmetic;
- ml/gradient/Gradient.scala:44-49: Gradient.sum adds the gradients in order, from zeros, in double.

State of dtype float32 is widened (exact), the arithmetic above runs in float64 on the unrounded
m_t and v_t, and each of w, m, v is rounded to float32 once, where it is stored.  Elements outside
the selection are not touched.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-8  # ml/util/Maths.scala:8
SGD, ADAM = 0, 1
ALL, LIVE, AUTO = 0, 1, 2


def _jint(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def auto_dense(nnz: int, dim: int) -> bool:
    """DenseDoubleGradient.scala:92-95: nnz > dim * 2 / 3, the product wrapping like a Java int and the
    division truncating toward zero."""
    return nnz > int(_jint(dim * 2) / 3)


def gradient(decoded, scale: float) -> np.ndarray:
    """scale * (((0 + d_0) + d_1) + ...), all in float64."""
    acc = np.zeros(len(decoded[0]), dtype=np.float64)
    for d in decoded:
        acc = acc + np.asarray(d, dtype=np.float64)
    return acc * np.float64(scale)


def live(g: np.ndarray) -> np.ndarray:
    return np.abs(g) > EPS


def selection(g: np.ndarray, select: int, dim: int | None = None) -> np.ndarray:
    """The elements an update touches."""
    if select == ALL:
        return np.ones(len(g), dtype=bool)
    lv = live(g)
    if select == AUTO and auto_dense(int(lv.sum()), len(g) if dim is None else dim):
        return np.ones(len(g), dtype=bool)
    return lv


class Params:
    def __init__(self, kind=ADAM, lr=0.0, beta1=0.9, beta2=0.999, beta1_t=0.9, beta2_t=0.999, eps=EPS):
        self.kind, self.lr = kind, float(lr)
        self.beta1, self.beta2, self.beta1_t, self.beta2_t, self.eps = beta1, beta2, beta1_t, beta2_t, eps


def step(p: Params, g, w, m=None, v=None, mask=None):
    """One update of the selected elements; returns new (w, m, v) arrays of the state's dtype."""
    g = np.asarray(g, dtype=np.float64)
    mask = np.ones(len(g), dtype=bool) if mask is None else mask
    wd = w.astype(np.float64)
    lr = np.float64(p.lr)
    if p.kind == SGD:
        w_t = wd - g * lr
        out = w.copy()
        out[mask] = w_t.astype(w.dtype)[mask]
        return out, None, None
    b1, b2 = np.float64(p.beta1), np.float64(p.beta2)
    m_t = b1 * m.astype(np.float64) + (1 - b1) * g
    v_t = b2 * v.astype(np.float64) + (1 - b2) * g * g
    with np.errstate(invalid="ignore", divide="ignore"):
        ng = (np.float64(math.sqrt(1 - p.beta2_t)) * m_t) / ((1 - np.float64(p.beta1_t)) * (np.sqrt(v_t) + np.float64(p.eps)))
    w_t = wd - ng * lr
    ow, om, ov = w.copy(), m.copy(), v.copy()
    ow[mask] = w_t.astype(w.dtype)[mask]
    om[mask] = m_t.astype(m.dtype)[mask]
    ov[mask] = v_t.astype(v.dtype)[mask]
    return ow, om, ov


def step_kv(p: Params, keys, vals, w, m=None, v=None, mask=None):
    """The sparse overloads: the same update at w(k(i)) for every i (every selected i)."""
    keys = np.asarray(keys, dtype=np.int64)
    g = np.zeros(len(w), dtype=np.float64)
    g[keys] = np.asarray(vals, dtype=np.float64)
    touched = np.zeros(len(w), dtype=bool)
    touched[keys if mask is None else keys[mask]] = True
    return step(p, g, w, m, v, touched)


class GradientDescent:
    """The host side of GradientDescent.scala:16-21,48-49,91."""

    kind = SGD

    def __init__(self, dim, lr_0, decay, batchSpRatio):
        self.dim, self.lr_0, self.decay = dim, lr_0, decay
        self.epoch, self.batch = 0, 0
        self.batchNum = float(int(math.ceil(1.0 / batchSpRatio)))

    def next_batch(self):
        self.batch += 1
        if self.batch == self.batchNum:
            self.epoch += 1
            self.batch = 0

    def begin_update(self):
        pass

    def params(self) -> Params:
        return Params(SGD, self.lr_0 / math.sqrt(1.0 + self.decay * self.epoch))


class Adam(GradientDescent):
    """Adam.scala:16-35."""

    kind = ADAM

    def __init__(self, dim, lr_0, decay, batchSpRatio):
        super().__init__(dim, lr_0, decay, batchSpRatio)
        self.beta1, self.beta2, self.beta1_t, self.beta2_t = 0.9, 0.999, 0.9, 0.999

    def begin_update(self):
        if self.epoch > 0 and self.batch == 0:
            self.beta1_t *= self.beta1
            self.beta2_t *= self.beta2

    def params(self) -> Params:
        return Params(ADAM, self.lr_0, self.beta1, self.beta2, self.beta1_t, self.beta2_t)
