"""The `ml` module's gradient containers around the codec:
DenseDoubleGradient / SparseDoubleGradient (ml/gradient/DenseDoubleGradient.scala,
SparseDoubleGradient.scala) and SketchGradient (ml/gradient/SketchGradient.scala:8-80), the
caller that compresses a worker's gradient.

Values live on the GPU (float32 or float64 tensors).  The compaction (toSparse), quantisation,
MinMax sketch and key codec run in libskml's kernels; this module is the glue the reference
keeps in Scala: which codec to use, bucketValues and its timesBy, the nnz rule of toAuto.
"""
from __future__ import annotations

from enum import Enum

import numpy as np
import torch

from . import fixed_point
from .exceptions import SketchMLException
from .quantization import QuantileQuantizer, ZipMLQuantizer
from .sparse import encode_sparse, to_sparse

EPS = 1e-8  # ml/util/Maths.scala:8


class Kind(Enum):
    DenseDouble = "DenseDouble"
    SparseDouble = "SparseDouble"
    Sketch = "Sketch"
    FixedPoint = "FixedPoint"
    Zip = "Zip"


def _jint(x: int) -> int:
    """Java int wrap-around."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def auto_dense(nnz: int, dim: int) -> bool:
    """toAuto's rule: dense iff nnz > dim * 2 / 3 in Java int arithmetic (the product wraps for
    dim > 1,073,741,823; DenseDoubleGradient.scala:92-95)."""
    lim = _jint(dim * 2)
    lim = int(lim / 3)  # Java division truncates toward zero
    return nnz > lim


class DenseDoubleGradient:
    """ml/gradient/DenseDoubleGradient.scala."""

    def __init__(self, dim: int, values: torch.Tensor):
        self.dim = int(dim)
        self.values = values

    def _sparse(self):
        # |v| > EPS compaction on the device (k_compact; fp64 values are tested in double and kept
        # as doubles, so fromSparse bins the reference's own double values)
        return to_sparse(self.values)

    def countNNZ(self) -> int:
        return int(self._sparse()[0].numel())

    def timesBy(self, x: float) -> None:
        self.values.mul_(x)

    def toDense(self) -> "DenseDoubleGradient":
        return self

    def toSparse(self) -> "SparseDoubleGradient":
        keys, vals = self._sparse()
        return SparseDoubleGradient(self.dim, keys, vals)

    def toAuto(self):
        keys, vals = self._sparse()
        return self if auto_dense(int(keys.numel()), self.dim) else SparseDoubleGradient(self.dim, keys, vals)

    def kind(self) -> Kind:
        return Kind.DenseDouble


class SparseDoubleGradient:
    """ml/gradient/SparseDoubleGradient.scala: strictly increasing int keys and their values."""

    def __init__(self, dim: int, indices: torch.Tensor, values: torch.Tensor):
        if indices.numel() != values.numel():
            raise SketchMLException(
                f"Lengths of key array and value array do not match: {indices.numel()}, {values.numel()}")
        self.dim = int(dim)
        self.indices = indices
        self.values = values

    def _live(self) -> torch.Tensor:
        return self.values.abs() > EPS

    def countNNZ(self) -> int:
        return int(self._live().sum().item())

    def timesBy(self, x: float) -> None:
        self.values.mul_(x)

    def toDense(self) -> DenseDoubleGradient:
        dense = torch.zeros(self.dim, dtype=self.values.dtype, device=self.values.device)
        live = self._live()
        dense[self.indices[live].long()] = self.values[live]
        return DenseDoubleGradient(self.dim, dense)

    def toSparse(self) -> "SparseDoubleGradient":
        return self

    def toAuto(self):
        return self.toDense() if auto_dense(self.countNNZ(), self.dim) else self

    def kind(self) -> Kind:
        return Kind.SparseDouble


class SketchGradient:
    """ml/gradient/SketchGradient.scala:8-80.

    fromDense: QuantileQuantizer.quantize over all values, bins kept (as the device payload);
    fromSparse: quantize the values, then GroupedMinMaxSketch over (indices, bins).
    bucketValues is the host double array Quantizer.getValues() returns, scaled in place by
    timesBy exactly as the Scala loop does, so toDense / toSparse return the same doubles.
    """

    def __init__(self, grad=None, binNum: int = 256, groupNum: int = 8, rowNum: int = 2, colRatio: float = 0.3,
                 dim: int | None = None, seed: int = 0, hashSeed: int = 0):
        self.binNum, self.groupNum, self.rowNum, self.colRatio = int(binNum), int(groupNum), int(rowNum), colRatio
        self.seed, self.hashSeed = seed, hashSeed
        self.dim = int(dim if dim is not None else (grad.dim if grad is not None else 0))
        self.nnz = 0
        self.bucketValues: np.ndarray | None = None
        self.quantizer: QuantileQuantizer | None = None  # dense: the bins live in its payload
        self.sketch = None                                # sparse: the GroupedMinMaxSketch payload
        if grad is not None:
            if grad.kind() == Kind.DenseDouble:
                self.fromDense(grad)
            elif grad.kind() == Kind.SparseDouble:
                self.fromSparse(grad)
            else:
                raise SketchMLException(f"Cannot create {Kind.Sketch.value} from {grad.kind().value}")

    def fromDense(self, dense: DenseDoubleGradient) -> None:
        q = QuantileQuantizer(self.binNum, self.seed)
        q.quantize(dense.values)
        self.bucketValues = q.getValues()
        self.quantizer, self.sketch = q, None
        self.nnz = self.dim

    def fromSparse(self, sparse: SparseDoubleGradient) -> None:
        self.sketch = encode_sparse(sparse.indices, sparse.values, self.binNum, self.groupNum, self.rowNum,
                                    self.colRatio, self.seed, self.hashSeed)
        self.bucketValues = self.sketch.values()
        self.quantizer = None
        self.nnz = int(sparse.indices.numel())

    def timesBy(self, x: float) -> None:
        self.bucketValues = self.bucketValues * x  # element-wise double products, as the Scala loop

    def countNNZ(self) -> int:
        return self.nnz

    def _values_of(self, bins: torch.Tensor) -> torch.Tensor:
        lut = torch.from_numpy(np.ascontiguousarray(self.bucketValues)).to(bins.device)
        return lut[bins.long()]

    def toDense(self) -> DenseDoubleGradient:
        if self.quantizer is None:
            raise SketchMLException("toDense of a sparse SketchGradient: bins is null")
        return DenseDoubleGradient(self.dim, self._values_of(self.quantizer.getBins()))

    def toSparse(self) -> SparseDoubleGradient:
        if self.sketch is None:
            raise SketchMLException("toSparse of a dense SketchGradient: sketch is null")
        keys, bins = self.sketch.restore_bins()
        return SparseDoubleGradient(self.dim, keys, self._values_of(bins))

    def toAuto(self):
        return (self.toDense() if self.quantizer is not None else self.toSparse()).toAuto()

    def kind(self) -> Kind:
        return Kind.Sketch


class FixedPointGradient:
    """ml/gradient/FixedPointGradient.scala:13-80, the QSGD-style baseline of Gradient.compress:
    norm-scaled sign + (numBits - 1)-bit magnitudes with a coin flip added to every code, packed
    into a BitSet word stream.  The payload (header with the norm, then the words) lives on the
    device; `seed` names the coin flips (the i-th nextBoolean() of java.util.Random(seed)), which
    the reference draws from an unseeded global Bernoulli.

    fromSparse keeps the indices tensor as it is and encodes the values, as the reference does.
    """

    def __init__(self, grad=None, numBits: int = 8, seed: int = 0, dim: int | None = None):
        if numBits >= 30 or numBits < 2:  # require(numBits < 30, ...); one bit divides by max = 0
            raise SketchMLException(f"Bit num out of range: {numBits}")
        self.numBits, self.seed = int(numBits), int(seed)
        self.dim = int(dim if dim is not None else (grad.dim if grad is not None else 0))
        self.size = 0
        self.indices: torch.Tensor | None = None
        self.payload: torch.Tensor | None = None
        if grad is not None:
            if grad.kind() == Kind.DenseDouble:
                self.fromDense(grad)
            elif grad.kind() == Kind.SparseDouble:
                self.fromSparse(grad)
            else:
                raise SketchMLException(f"Cannot create {Kind.FixedPoint.value} from {grad.kind().value}")

    def _from_array(self, values: torch.Tensor) -> None:
        self.size = int(values.numel())
        self.payload = fixed_point.encode(values, self.numBits, self.seed)

    def fromDense(self, dense: DenseDoubleGradient) -> None:
        self.indices = None
        self._from_array(dense.values)

    def fromSparse(self, sparse: SparseDoubleGradient) -> None:
        self.indices = sparse.indices
        self._from_array(sparse.values)

    @property
    def norm(self) -> float:
        return float(fixed_point.info(self.payload).norm)

    def timesBy(self, x: float) -> None:
        fixed_point.times_by(self.payload, x)

    def countNNZ(self) -> int:
        return self.size

    def _to_array(self) -> torch.Tensor:
        return fixed_point.decode(self.payload, self.size, torch.float64)

    def toDense(self) -> DenseDoubleGradient:
        return DenseDoubleGradient(self.dim, self._to_array())

    def toSparse(self) -> SparseDoubleGradient:
        if self.indices is None:
            raise SketchMLException("toSparse of a dense FixedPointGradient: indices is null")
        return SparseDoubleGradient(self.dim, self.indices, self._to_array())

    def toAuto(self):
        return (self.toDense() if self.indices is None else self.toSparse()).toAuto()

    def kind(self) -> Kind:
        return Kind.FixedPoint


class ZipGradient:
    """ml/gradient/ZipGradient.scala:11-58: the ZipMLQuantizer over all values of a dense gradient or
    over the values of a sparse one, whose indices it keeps as they are.  toDense / toSparse return
    getValues()[bin] in double."""

    def __init__(self, grad=None, binNum: int = 256, dim: int | None = None):
        self.binNum = int(binNum)
        self.dim = int(dim if dim is not None else (grad.dim if grad is not None else 0))
        self.size = 0
        self.indices: torch.Tensor | None = None
        self.quantizer: ZipMLQuantizer | None = None
        if grad is not None:
            if grad.kind() == Kind.DenseDouble:
                self.fromDense(grad)
            elif grad.kind() == Kind.SparseDouble:
                self.fromSparse(grad)
            else:
                raise SketchMLException(f"Cannot create {Kind.Zip.value} from {grad.kind().value}")

    def _from_array(self, values: torch.Tensor) -> None:
        self.size = int(values.numel())
        self.quantizer = ZipMLQuantizer(self.binNum)
        self.quantizer.quantize(values)

    def fromDense(self, dense: DenseDoubleGradient) -> None:
        self._from_array(dense.values)

    def fromSparse(self, sparse: SparseDoubleGradient) -> None:
        self.indices = sparse.indices
        self._from_array(sparse.values)

    def timesBy(self, x: float) -> None:
        self.quantizer.timesBy(x)

    def countNNZ(self) -> int:
        return self.size

    def _values(self) -> torch.Tensor:
        bins = self.quantizer.getBins()
        lut = torch.from_numpy(np.ascontiguousarray(self.quantizer.getValues())).to(bins.device)
        return lut[bins.long()]

    def toDense(self) -> DenseDoubleGradient:
        return DenseDoubleGradient(self.dim, self._values())

    def toSparse(self) -> SparseDoubleGradient:
        if self.indices is None:
            raise SketchMLException("toSparse of a dense ZipGradient: indices is null")
        return SparseDoubleGradient(self.dim, self.indices, self._values())

    def toAuto(self):
        return (self.toDense() if self.indices is None else self.toSparse()).toAuto()

    def kind(self) -> Kind:
        return Kind.Zip


def compress(grad, compressor: str = "Sketch", **conf):
    """Gradient.compress's switch (ml/gradient/Gradient.scala:18-36) over MLConf's compressor names
    ("Sketch", "FixedPoint", "None"; case and underscores are ignored, so "fixed_point" works).
    conf: quantBinNum, sketchGroupNum, sketchRowNum, sketchColRatio, fixedPointBitNum (MLConf's
    names and defaults), and seed / hashSeed for the streams this library makes explicit."""
    name = str(compressor).replace("_", "").lower()
    if name == "sketch":
        return SketchGradient(grad, conf.get("quantBinNum", 256), conf.get("sketchGroupNum", 8),
                              conf.get("sketchRowNum", 2), conf.get("sketchColRatio", 0.3),
                              seed=conf.get("seed", 0), hashSeed=conf.get("hashSeed", 0))
    if name == "fixedpoint":
        return FixedPointGradient(grad, conf.get("fixedPointBitNum", 8), seed=conf.get("seed", 0))
    if name == "none":
        return grad
    if name in ("zip", "float"):
        raise SketchMLException(f"Compressor not built here: {compressor} (the Zip codec itself is built: construct "
                                f"ZipGradient(grad, quantBinNum), only this switch is left; the Float codec is a cast; "
                                f"DESIGN.md section 9)")
    raise SketchMLException(f"Unrecognizable compressor: {compressor}")
