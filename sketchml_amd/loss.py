"""The loss classes of ml/objective/Loss.scala:6-137: L1LogLoss, L2HingeLoss, L2LogLoss, L2SquareLoss.

loss / grad / predict are host scalars in the reference's operation order, for mirroring and for
tests; the per-instance work of a mini-batch runs in libskml's k_glm_predict (skml_glm.hip), which
takes the class's `kind`.  getReg is a float64 reduction over the device weight.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .gradient import EPS


def _exp(x: float) -> float:
    """Math.exp: +Infinity on overflow, where Python raises."""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _values(v) -> list:
    return v.detach().cpu().double().tolist() if isinstance(v, torch.Tensor) else [float(t) for t in v]


class Loss:
    """trait Loss (Loss.scala:6-20)."""

    kind = -1

    def __init__(self, lam: float):
        self.lam = float(lam)

    def loss(self, pre: float, y: float) -> float:
        raise NotImplementedError

    def grad(self, pre: float, y: float) -> float:
        raise NotImplementedError

    def predict(self, w, x) -> float:
        """Maths.dot(w, x) (ml/util/Maths.scala:57-69) for x = (indices, values): from 0.0, w[ind] * val
        added in stored order."""
        indices, values = x
        wv = w.detach().cpu().double() if isinstance(w, torch.Tensor) else w
        dot = 0.0
        for ind, val in zip(_values(indices), _values(values)):
            dot += float(wv[int(ind)]) * val
        return dot

    @property
    def isL1Reg(self) -> bool:
        return False

    @property
    def isL2Reg(self) -> bool:
        return False

    @property
    def getRegParam(self) -> float:
        return self.lam

    def getReg(self, w) -> float:
        return 0.0

    def reg_kind(self) -> int:
        """The SKML_REG_* id of the regulariser that is on."""
        return _lib.SKML_REG_L1 if self.isL1Reg else (_lib.SKML_REG_L2 if self.isL2Reg else _lib.SKML_REG_NONE)


class L1Loss(Loss):
    """abstract class L1Loss (Loss.scala:22-37)."""

    @property
    def isL1Reg(self) -> bool:
        return self.lam > EPS

    def getReg(self, w) -> float:
        if not self.isL1Reg:
            return 0.0
        return float(torch.as_tensor(w).double().abs().sum().item()) * self.lam  # Vectors.norm(w, 1) * lambda


class L2Loss(Loss):
    """abstract class L2Loss (Loss.scala:39-54)."""

    @property
    def isL2Reg(self) -> bool:
        return self.lam > EPS

    def getReg(self, w) -> float:
        if not self.isL2Reg:
            return 0.0
        wd = torch.as_tensor(w).double()
        return math.sqrt(float((wd * wd).sum().item())) * self.lam  # Vectors.norm(w, 2) * lambda


def _log_loss(pre: float, y: float) -> float:
    z = pre * y
    if z > 18:
        return _exp(-z)
    if z < -18:
        return -z
    return math.log(1.0 + _exp(-z))


def _log_grad(pre: float, y: float) -> float:
    z = pre * y
    if z > 18:
        return y * _exp(-z)
    if z < -18:
        return y
    return y / (1.0 + _exp(z))


class L1LogLoss(L1Loss):
    """Loss.scala:56-80."""

    kind = _lib.SKML_LOSS_L1_LOG

    def loss(self, pre: float, y: float) -> float:
        return _log_loss(pre, y)

    def grad(self, pre: float, y: float) -> float:
        return _log_grad(pre, y)


class L2HingeLoss(L2Loss):
    """Loss.scala:82-101: the loss tests `< 1.0`, the gradient `<= 1.0`."""

    kind = _lib.SKML_LOSS_L2_HINGE

    def loss(self, pre: float, y: float) -> float:
        z = pre * y
        return 1.0 - z if z < 1.0 else 0.0

    def grad(self, pre: float, y: float) -> float:
        return y if pre * y <= 1.0 else 0.0


class L2LogLoss(L2Loss):
    """Loss.scala:103-127."""

    kind = _lib.SKML_LOSS_L2_LOG

    def loss(self, pre: float, y: float) -> float:
        return _log_loss(pre, y)

    def grad(self, pre: float, y: float) -> float:
        return _log_grad(pre, y)


class L2SquareLoss(L2Loss):
    """Loss.scala:129-137."""

    kind = _lib.SKML_LOSS_L2_SQUARE

    def loss(self, pre: float, y: float) -> float:
        return 0.5 * (pre - y) * (pre - y)

    def grad(self, pre: float, y: float) -> float:
        return y - pre
