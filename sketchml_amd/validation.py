"""The validation pass on the device: ValidationUtil.calLossPrecision and calLossAucPrecision
(ml/util/ValidationUtil.scala:12-93) over skml_glm_validate_* of include/skml.h.

The predictions, the per-instance losses, the four confusion counts, the loss sum in instance order
and, for the AUC, the sort of the scores and the rank sum run in libskml's kernels; this module keeps
what the reference keeps in scalars: the derived ratios and the AUC formula, in Java's double
division (0.0 / 0 is NaN, x / 0 is +-Infinity; nothing raises).

The order of the AUC's sort is the device's own where the reference's is not defined: scores by their
IEEE total-order key (-0.0 before +0.0), equal scores in instance order; a NaN score makes auc NaN
(include/skml.h).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .context import get_context
from .exceptions import SketchMLException, check


def java_div(a: float, b: float) -> float:
    """a / b as Java divides doubles: NaN for 0.0 / 0 and NaN operands, +-Infinity for x / 0."""
    a, b = float(a), float(b)
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    try:
        return a / b
    except OverflowError:
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def auc_of(sigma: int, M: int, N: int) -> float:
    """(sigma - (M + 1) * M / 2) / M / N as ValidationUtil.scala:84 writes it: the product and its
    halving in Long, converted once, the rest in double."""
    return java_div(java_div(float(sigma) - float((M + 1) * M // 2), float(M)), float(N))


class ValidationResult(tuple):
    """(validLoss, truePos, trueNeg, falsePos, falseNeg, validNum), the reference's tuple, with the
    values the reference logs as attributes: precision, trueRecall, falseRecall; auc, M, N, sigma
    (None without the AUC); pre and loss, the per-instance device tensors; nanScores."""

    def __new__(cls, validLoss, truePos, trueNeg, falsePos, falseNeg, validNum, **extra):
        self = super().__new__(cls, (float(validLoss), int(truePos), int(trueNeg), int(falsePos), int(falseNeg), int(validNum)))
        self.auc = self.M = self.N = self.sigma = None
        self.pre = self.loss = None
        self.nanScores = 0
        for k, v in extra.items():
            setattr(self, k, v)
        return self

    validLoss = property(lambda self: self[0])
    truePos = property(lambda self: self[1])
    trueNeg = property(lambda self: self[2])
    falsePos = property(lambda self: self[3])
    falseNeg = property(lambda self: self[4])
    validNum = property(lambda self: self[5])

    @property
    def precision(self) -> float:
        return java_div(1.0 * (self[1] + self[2]), self[5])

    @property
    def trueRecall(self) -> float:
        return java_div(1.0 * self[1], self[1] + self[4])

    @property
    def falseRecall(self) -> float:
        return java_div(1.0 * self[2], self[2] + self[3])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _flags(order: str, auc: bool) -> int:
    if order not in ("sequential", "tree"):
        raise SketchMLException(f"order={order!r}: 'sequential' (the reference's sum) or 'tree' (the fixed-shape device sum)")
    return (_lib.SKML_VALID_AUC if auc else 0) | (_lib.SKML_VALID_TREE_SUM if order == "tree" else 0)


def _validate(weights: torch.Tensor, validData, loss, order: str, auc: bool) -> ValidationResult:
    if not (isinstance(weights, torch.Tensor) and weights.is_cuda and weights.is_contiguous()
            and weights.dtype in (torch.float32, torch.float64)):
        raise SketchMLException("the weight must be a contiguous float32 or float64 device tensor")
    flags = _flags(order, auc)
    dev = weights.device
    if validData.device != dev:
        raise SketchMLException(f"the data set lives on {validData.device}, the weight on {dev}")
    if weights.numel() != validData.dim:
        raise SketchMLException(f"the weight holds {weights.numel()} values, the data set has {validData.dim} features")
    data = validData.glm_data()
    pre = torch.empty(validData.rows, dtype=torch.float64, device=dev)
    per = torch.empty(validData.rows, dtype=torch.float64, device=dev)
    res = _lib.ValidResult()
    fn = _lib.lib.skml_glm_validate_f64 if weights.dtype == torch.float64 else _lib.lib.skml_glm_validate_f32
    check(fn(get_context(dev).handle, C.byref(data), int(loss.kind), _ptr(weights), flags, _ptr(pre), _ptr(per), C.byref(res)),
          "glm_validate")
    extra = {"pre": pre, "loss": per, "nanScores": int(res.nan_scores)}
    if auc:
        M, N, sigma = int(res.pos), int(res.neg), int(res.rank_sum)
        extra.update(M=M, N=N, sigma=sigma, auc=math.nan if res.nan_scores else auc_of(sigma, M, N))
    return ValidationResult(res.loss, res.true_pos, res.true_neg, res.false_pos, res.false_neg, res.num, **extra)


def calLossPrecision(weights: torch.Tensor, validData, loss, order: str = "sequential") -> ValidationResult:
    """ValidationUtil.calLossPrecision (ValidationUtil.scala:12-41): the sum of the losses over
    validData in instance order, the confusion counts and validNum.  order="tree" takes the sum from
    the fixed-shape device reduction instead: faster on a large set, not the reference's bits."""
    return _validate(weights, validData, loss, order, False)


def calLossAucPrecision(weights: torch.Tensor, validData, loss, order: str = "sequential") -> ValidationResult:
    """ValidationUtil.calLossAucPrecision (ValidationUtil.scala:43-93): the same tuple; the AUC the
    reference logs is in .auc, with .M, .N and .sigma behind it."""
    return _validate(weights, validData, loss, order, True)


def seq_sum(x: torch.Tensor) -> float:
    """skml_glm_seq_sum: ((0.0 + x[0]) + x[1]) + ... over a float64 device tensor."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.dtype == torch.float64 and x.numel() >= 1):
        raise SketchMLException("seq_sum takes a contiguous float64 device tensor of at least one value")
    out = C.c_double()
    check(_lib.lib.skml_glm_seq_sum(get_context(x.device).handle, _ptr(x), x.numel(), C.byref(out)), "glm_seq_sum")
    return float(out.value)


def auc_rank_sum(scores: torch.Tensor, labels: torch.Tensor, want_order: bool = False):
    """skml_auc_rank_sum: the AUC stage alone over float64 device tensors.  Returns a dict: M, N, sigma,
    nanScores, auc, and order (the sorted permutation as an int32 device tensor) when asked for."""
    for t in (scores, labels):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64):
            raise SketchMLException("scores and labels must be contiguous float64 device tensors")
    n = scores.numel()
    if n < 1 or labels.numel() != n or labels.device != scores.device:
        raise SketchMLException(f"{n} scores and {labels.numel()} labels")
    order = torch.empty(n, dtype=torch.int32, device=scores.device) if want_order else None
    pos, neg, nan, sigma = C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64()
    check(_lib.lib.skml_auc_rank_sum(get_context(scores.device).handle, _ptr(scores), _ptr(labels), n, _ptr(order), C.byref(pos),
                                     C.byref(neg), C.byref(sigma), C.byref(nan)), "auc_rank_sum")
    M, N, s = int(pos.value), int(neg.value), int(sigma.value)
    return {"M": M, "N": N, "sigma": s, "nanScores": int(nan.value), "order": order,
            "auc": math.nan if nan.value else auc_of(s, M, N)}
