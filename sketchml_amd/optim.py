"""The optimiser update on the device: the reference's GradientDescent and Adam
(ml/objective/GradientDescent.scala:16-21,89-117, ml/objective/Adam.scala:16-77) over the
skml_opt_step_* / skml_dense_decode_sum_step_* / skml_fixed_decode_sum_step_* entries of include/skml.h.

The weight is a device tensor (float64 as the reference's DenseVector, or float32); Adam's m and
v are tensors of the weight's dtype that the optimiser owns.  All arithmetic runs in double in the
reference's operation order inside libskml's kernels; this module keeps what the reference keeps
on the host: the epoch / batch counters, the learning-rate decay, the beta_t products and the
dispatch on the gradient's kind.

miniBatchGradientDescent (GradientDescent.scala:23-87) is here too, over skml_glm_gradient_* and
skml_glm_finish_*: the predictions, losses and plusBy of a batch of a data.DataSet, toAuto, timesBy
and the regularisers run on the device; objLoss and regLoss, which the reference only logs, are
the two scalars that come back.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .context import LOWP_DTYPES, as_device_f32, as_device_values, get_context
from .exceptions import SketchMLException, check
from .gradient import EPS, DenseDoubleGradient, Kind, SparseDoubleGradient, auto_dense
from .sparse import to_sparse

ALL, LIVE, AUTO = _lib.SKML_OPT_ALL, _lib.SKML_OPT_LIVE, _lib.SKML_OPT_AUTO


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _gradient_values(values) -> torch.Tensor:
    x = as_device_values(values)
    return as_device_f32(x) if x.dtype in LOWP_DTYPES else x


def batch_gradient(weight: torch.Tensor, dataSet, row0: int, batch: int, loss, want_pre: bool = False):
    """skml_glm_gradient_*: the loop of miniBatchGradientDescent over the rows (row0 + j) mod size,
    j < batch, of a data.DataSet.  Returns a dict of float64 device tensors and two host scalars:
    grad (dim values, unscaled), coef (-1.0 * loss.grad per instance), loss (per instance), pre (when
    asked for), nnz (toAuto's count of |grad| > 1e-8) and objLoss."""
    dev = weight.device
    if dataSet.device != dev:
        raise SketchMLException(f"the data set lives on {dataSet.device}, the weight on {dev}")
    data = dataSet.glm_data()
    out = {"grad": torch.empty(dataSet.dim, dtype=torch.float64, device=dev),
           "coef": torch.empty(batch, dtype=torch.float64, device=dev),
           "loss": torch.empty(batch, dtype=torch.float64, device=dev),
           "pre": torch.empty(batch, dtype=torch.float64, device=dev) if want_pre else None}
    nnz, obj = C.c_int64(), C.c_double()
    fn = _lib.lib.skml_glm_gradient_f64 if weight.dtype == torch.float64 else _lib.lib.skml_glm_gradient_f32
    check(fn(get_context(dev).handle, C.byref(data), int(row0), int(batch), int(loss.kind), _ptr(weight), _ptr(out["pre"]),
             _ptr(out["coef"]), _ptr(out["loss"]), _ptr(out["grad"]), C.byref(nnz), C.byref(obj)), "glm_gradient")
    out["nnz"], out["objLoss"] = int(nnz.value), float(obj.value)
    return out


def finish_gradient(grad, times: float, loss, weight: torch.Tensor) -> None:
    """skml_glm_finish_*: grad.timesBy(times), then l1Reg / l2Reg when the loss has one on, in place on
    a DenseDoubleGradient or a SparseDoubleGradient of float64 values."""
    h = get_context(weight.device).handle
    reg, lam, w32 = loss.reg_kind(), float(loss.getRegParam), int(weight.dtype == torch.float32)
    if grad.kind() == Kind.DenseDouble:
        check(_lib.lib.skml_glm_finish_dense_f64(h, _ptr(grad.values), grad.dim, float(times), reg, lam, _ptr(weight), w32),
              "glm_finish_dense")
    elif grad.kind() == Kind.SparseDouble:
        check(_lib.lib.skml_glm_finish_kv_f64(h, _ptr(grad.indices), _ptr(grad.values), grad.indices.numel(), grad.dim,
                                              float(times), reg, lam, _ptr(weight), w32), "glm_finish_kv")
    else:
        raise SketchMLException(f"Cannot regularize {grad.kind().value} kind of gradients")


class GradientDescent:
    """ml/objective/GradientDescent.scala: w -= g * lr with lr = lr_0 / sqrt(1 + decay * epoch)."""

    kind = _lib.SKML_OPT_SGD

    def __init__(self, dim: int, lr_0: float, decay: float, batchSpRatio: float):
        self.dim, self.lr_0, self.decay, self.batchSpRatio = int(dim), float(lr_0), float(decay), float(batchSpRatio)
        self.epoch = 0
        self.batch = 0
        self.batchNum = float(int(math.ceil(1.0 / batchSpRatio)))  # GradientDescent.scala:21

    def miniBatchGradientDescent(self, weight: torch.Tensor, dataSet, loss, sequentialLoss: bool = False):
        """GradientDescent.scala:23-51: (grad, batchSize, objLoss, regLoss) of the next
        (size * batchSpRatio).toInt instances of dataSet.loopingRead.  grad is toAuto's choice, a
        DenseDoubleGradient or a SparseDoubleGradient of float64 device tensors, scaled by
        1.0 / batchSize and regularised.  objLoss is a fixed-shape device sum of the per-instance
        losses, which stay in self.lastLoss; with sequentialLoss it is their sum in batch order
        (skml_glm_seq_sum), the reference's `objLoss += ...` bit for bit given the losses."""
        batchSize = int(dataSet.size * self.batchSpRatio)
        if batchSize == 0 or self.batchSpRatio > 1:
            raise SketchMLException(f"batchSpRatio={self.batchSpRatio} over {dataSet.size} instances gives a batch of "
                                    f"{batchSize}: the reference divides by zero, or reads an instance twice")
        self._check_weight(weight)
        if dataSet.dim != self.dim:
            raise SketchMLException(f"the data set has {dataSet.dim} features, the optimiser {self.dim}")
        out = batch_gradient(weight, dataSet, dataSet.take(batchSize), batchSize, loss)
        self.lastLoss = out["loss"]
        if auto_dense(out["nnz"], self.dim):
            grad = DenseDoubleGradient(self.dim, out["grad"])
        else:
            keys, vals = to_sparse(out["grad"])  # toSparse of the unscaled values
            grad = SparseDoubleGradient(self.dim, keys, vals)
        finish_gradient(grad, 1.0 / batchSize, loss, weight)
        regLoss = float(loss.getReg(weight))
        objLoss = out["objLoss"]
        if sequentialLoss:
            from .validation import seq_sum
            objLoss = seq_sum(out["loss"])
        self.nextBatch()
        return grad, batchSize, objLoss, regLoss

    def nextBatch(self) -> None:
        """The counters' step at the end of miniBatchGradientDescent (GradientDescent.scala:48-49)."""
        self.batch += 1
        if self.batch == self.batchNum:
            self.epoch += 1
            self.batch = 0

    def learningRate(self) -> float:
        return self.lr_0 / math.sqrt(1.0 + self.decay * self.epoch)  # GradientDescent.scala:91

    def _begin_update(self) -> None:
        pass

    def params(self, select: int = ALL) -> _lib.OptParams:
        p = _lib.OptParams()
        _lib.lib.skml_opt_params_default(C.byref(p))
        p.kind, p.select, p.lr = self.kind, int(select), self.learningRate()
        return p

    def _state(self, weight: torch.Tensor):
        return None, None

    def _check_weight(self, weight: torch.Tensor) -> None:
        if not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.is_contiguous()
                and weight.dtype in (torch.float32, torch.float64)):
            raise SketchMLException("the weight must be a contiguous float32 or float64 device tensor")
        if weight.numel() != self.dim:
            raise SketchMLException(f"the weight holds {weight.numel()} values, the optimiser {self.dim}")

    def update(self, grad, weight: torch.Tensor) -> None:
        """update(grad, weight) (GradientDescent.scala:89-102, Adam.scala:27-48): a
        DenseDoubleGradient updates every element, a SparseDoubleGradient its keys, and a
        SketchGradient / FixedPointGradient / ZipGradient goes through toAuto first."""
        self._check_weight(weight)
        self._begin_update()
        self._update0(grad, weight)

    def _update0(self, grad, weight: torch.Tensor) -> None:
        kind = grad.kind()
        if kind == Kind.DenseDouble:
            self.step_array(grad.values, weight, 1.0, ALL)
        elif kind == Kind.SparseDouble:
            self.step_kv(grad.indices, grad.values, weight)
        elif kind in (Kind.Sketch, Kind.FixedPoint, Kind.Zip):
            self._update0(grad.toAuto(), weight)
        else:
            raise SketchMLException(f"ClassNotFoundException: {kind}")

    # ---- the device forms; none of them advances beta_t ----
    def step_array(self, values, weight: torch.Tensor, scale: float = 1.0, select: int = ALL) -> None:
        """skml_opt_step_*: g = scale * values (float32 or float64, in double)."""
        self._check_weight(weight)
        g = _gradient_values(values)
        if g.numel() != self.dim:
            raise SketchMLException(f"the gradient holds {g.numel()} values, the optimiser {self.dim}")
        m, v = self._state(weight)
        p = self.params(select)
        fn = _lib.lib.skml_opt_step_f64 if weight.dtype == torch.float64 else _lib.lib.skml_opt_step_f32
        check(fn(get_context(weight.device).handle, _ptr(g), int(g.dtype == torch.float64), self.dim, float(scale),
                 C.byref(p), _ptr(weight), _ptr(m), _ptr(v)), "opt_step")

    def step_kv(self, indices: torch.Tensor, values, weight: torch.Tensor, scale: float = 1.0, select: int = ALL) -> None:
        """skml_opt_step_kv_*: strictly increasing int32 keys and their values."""
        self._check_weight(weight)
        vals = _gradient_values(values)
        keys = indices.to(device=weight.device, dtype=torch.int32).contiguous()
        if keys.numel() != vals.numel():
            raise SketchMLException(
                f"Lengths of key array and value array do not match: {keys.numel()}, {vals.numel()}")
        m, v = self._state(weight)
        p = self.params(select)
        fn = _lib.lib.skml_opt_step_kv_f64 if weight.dtype == torch.float64 else _lib.lib.skml_opt_step_kv_f32
        check(fn(get_context(weight.device).handle, _ptr(keys), _ptr(vals), int(vals.dtype == torch.float64),
                 keys.numel(), self.dim, float(scale), C.byref(p), _ptr(weight), _ptr(m), _ptr(v)), "opt_step_kv")

    def step_payloads(self, ctx_handle, payloads: torch.Tensor, nranks: int, stride: int, scale: float,
                      weight: torch.Tensor, select: int = ALL) -> None:
        """skml_dense_decode_sum_step_*: Gradient.sum of the gathered dense payloads, timesBy(scale)
        and the update in one pass; the sum is never rounded to float."""
        self._check_weight(weight)
        m, v = self._state(weight)
        p = self.params(select)
        fn = (_lib.lib.skml_dense_decode_sum_step_f64 if weight.dtype == torch.float64
              else _lib.lib.skml_dense_decode_sum_step_f32)
        check(fn(ctx_handle, _ptr(payloads), int(nranks), int(stride), self.dim, float(scale), C.byref(p),
                 _ptr(weight), _ptr(m), _ptr(v)), "decode_sum_step")

    def step_fixed_payloads(self, ctx_handle, payloads: torch.Tensor, nranks: int, stride: int, scale: float,
                            weight: torch.Tensor, select: int = ALL) -> None:
        """skml_fixed_decode_sum_step_*: the same for gathered FixedPointGradient payloads of one numBits."""
        self._check_weight(weight)
        m, v = self._state(weight)
        p = self.params(select)
        fn = (_lib.lib.skml_fixed_decode_sum_step_f64 if weight.dtype == torch.float64
              else _lib.lib.skml_fixed_decode_sum_step_f32)
        check(fn(ctx_handle, _ptr(payloads), int(nranks), int(stride), self.dim, float(scale), C.byref(p),
                 _ptr(weight), _ptr(m), _ptr(v)), "fixed_decode_sum_step")


class Adam(GradientDescent):
    """ml/objective/Adam.scala:16-77.  The learning rate is lr_0 itself (Adam.scala:39-45 pass lr_0);
    beta1_t / beta2_t advance at the first update of every epoch after the first (Adam.scala:29-32)."""

    kind = _lib.SKML_OPT_ADAM

    def __init__(self, dim: int, lr_0: float, decay: float, batchSpRatio: float):
        super().__init__(dim, lr_0, decay, batchSpRatio)
        self.beta1, self.beta2 = 0.9, 0.999
        self.beta1_t, self.beta2_t = 0.9, 0.999
        self.eps = EPS
        self.m: torch.Tensor | None = None
        self.v: torch.Tensor | None = None

    def learningRate(self) -> float:
        return self.lr_0

    def _begin_update(self) -> None:
        if self.epoch > 0 and self.batch == 0:
            self.beta1_t *= self.beta1
            self.beta2_t *= self.beta2

    def params(self, select: int = ALL) -> _lib.OptParams:
        p = super().params(select)
        p.beta1, p.beta2, p.beta1_t, p.beta2_t, p.eps = self.beta1, self.beta2, self.beta1_t, self.beta2_t, self.eps
        return p

    def _state(self, weight: torch.Tensor):
        if self.m is None:
            self.m = torch.zeros(self.dim, dtype=weight.dtype, device=weight.device)
            self.v = torch.zeros(self.dim, dtype=weight.dtype, device=weight.device)
        elif self.m.dtype != weight.dtype or self.m.device != weight.device:
            raise SketchMLException("the weight changed dtype or device: m and v are of the first weight's")
        return self.m, self.v
