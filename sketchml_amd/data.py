"""The training data of the `ml` module: DataSet (ml/data/DataSet.scala:5-25) and the line parsers
(ml/data/Parser.scala:23-76).

A DataSet is the CSR of its sparse instances (row_ptr, col, val, label) plus the same entries in
(column, row) order (col_ptr, csc_row, csc_val), which the mini-batch gradient's column kernel walks
(skml_glm_data, include/skml.h).  A batch of DataSet.loopingRead is a window of consecutive rows, so
the column order is built once, at first use, with a stable sort; nothing is sorted per batch.

A DenseDataSet holds dense instances (format csv) as one row-major array (skml_glm_dense_data), of
float64 values or, with xDtype, of float32, bfloat16 or float16 values (skml_glm_dense_lowp_data).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .exceptions import SketchMLException
from .gradient import EPS

JAVA_INT_MAX = 2147483647


def _label(text: str, negY: bool) -> float:
    y = float(text)
    if negY and abs(y - 1) > EPS:  # Parser.scala:29-30
        y = -1.0
    return y


def parseLibSVM(line: str, maxDim: int, negY: bool = True):
    """Parser.parseLibSVM (Parser.scala:23-43): "y i:v i:v ..." -> (label, indices, values)."""
    splits = line.strip().split(" ")
    y = _label(splits[0], negY)
    indices, values = [], []
    for item in splits[1:]:
        kv = item.strip().split(":")
        indices.append(int(kv[0]))
        values.append(float(kv[1]))
    return y, indices, values


def parseDummy(line: str, maxDim: int, negY: bool = True):
    """Parser.parseDummy (Parser.scala:61-76): "y,i,i,..." -> (label, indices, ones)."""
    splits = line.strip().split(",")
    y = _label(splits[0], negY)
    indices = [int(t.strip()) for t in splits[1:]]
    return y, indices, [1.0] * len(indices)


def parseCSV(line: str, maxDim: int, negY: bool = True):
    """Parser.parseCSV (Parser.scala:45-59) makes dense rows, which the sparse DataSet does not hold:
    parseDense is the same parser for a DenseDataSet."""
    raise SketchMLException("parseCSV: a sparse instance from a csv line is not built here; parseDense gives the dense "
                            "instance (label, values) for a DenseDataSet")


def parseDense(line: str, maxDim: int, negY: bool = True):
    """Parser.parseCSV (Parser.scala:45-59): "y,v,v,..." -> (label, values), a dense instance for a
    DenseDataSet.  maxDim is not read, as in the reference; the data set checks the length."""
    splits = line.strip().split(",")
    return _label(splits[0], negY), [float(t.strip()) for t in splits[1:]]


def _device(device):
    dev = torch.device(device) if device is not None else torch.device(
        "cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def one_vs_rest_labels(y, classes, device=None) -> torch.Tensor:
    """The K x rows matrix of +-1.0 labels of K one-vs-rest models from a vector of class ids: row m is +1.0 where
    y == classes[m] and -1.0 elsewhere (float64, contiguous, on the device), the `labels` of
    optim.batch_gradient_multi.  classes: the K class ids, in the order of the models."""
    y = torch.as_tensor(y).reshape(-1).to(_device(device))
    ids = torch.as_tensor(classes).reshape(-1).to(device=y.device, dtype=y.dtype)
    if ids.numel() < 1 or y.numel() < 1:
        raise SketchMLException("one_vs_rest_labels needs at least one class and one instance")
    return torch.where(y[None, :] == ids[:, None], 1.0, -1.0).to(torch.float64).contiguous()


class DataSet:
    """ml/data/DataSet.scala over device tensors.

    DataSet(dim) then add((label, indices, values)) row by row, or DataSet.fromCSR(...) /
    DataSet.fromRows(...).  The first use (size stays open until then) checks every row (columns
    strictly ascending inside [0, dim), as Spark's SparseVector requires), moves the CSR to `device`
    and builds the column order there.  readIndex is loopingRead's cursor.
    """

    dense = False
    entry = ""  # the entries of include/skml.h that serve it: skml_glm_<gradient | validate>_ + entry + f64 / f32

    def __init__(self, dim: int, device=None):
        self.dim = int(dim)
        if not 1 <= self.dim <= JAVA_INT_MAX:
            raise SketchMLException(f"dim={dim} outside [1, 2^31 - 1]")
        self.device = _device(device)
        self.readIndex = 0
        self._labels: list = []
        self._indices: list = []
        self._values: list = []
        self._csr = None  # (row_ptr, col, val, label) as given to fromCSR
        self._built = False

    # ---- construction ----
    @classmethod
    def fromRows(cls, rows, dim: int, device=None) -> "DataSet":
        ds = cls(dim, device)
        for ins in rows:
            ds.add(ins)
        return ds

    @classmethod
    def fromCSR(cls, row_ptr, col, val, label, dim: int, device=None) -> "DataSet":
        ds = cls(dim, device)
        ds._csr = (torch.as_tensor(row_ptr), torch.as_tensor(col), torch.as_tensor(val), torch.as_tensor(label))
        return ds

    def add(self, ins) -> None:
        """data += ins, for ins = (label, indices, values); only before the first use."""
        if self._built or self._csr is not None:
            raise SketchMLException("DataSet.add after the first use: the column order is built once")
        y, indices, values = ins
        if len(indices) != len(values):
            raise SketchMLException(f"Lengths of key array and value array do not match: {len(indices)}, {len(values)}")
        self._labels.append(float(y))
        self._indices.append([int(i) for i in indices])
        self._values.append([float(v) for v in values])

    def __iadd__(self, ins) -> "DataSet":  # DataSet.+=
        self.add(ins)
        return self

    @property
    def size(self) -> int:
        if self._csr is not None:
            return int(self._csr[0].numel()) - 1
        return len(self._labels)

    # ---- loopingRead ----
    def take(self, batch: int) -> int:
        """The first row of the next `batch` loopingRead calls (1 <= batch <= size), which it makes:
        readIndex is reset when it has reached size (DataSet.scala:16-17), then advanced."""
        size = self.size
        if not 1 <= batch <= size:
            raise SketchMLException(f"a batch of {batch} instances from a data set of {size}")
        r0 = 0 if self.readIndex >= size else self.readIndex
        end = r0 + batch
        self.readIndex = end if end <= size else end - size
        return r0

    def loopingRead(self):
        """(label, indices, values) of the next instance, as host lists."""
        r = self.take(1)
        self._build()
        s, e = int(self.row_ptr[r]), int(self.row_ptr[r + 1])
        return float(self.label[r]), self.col[s:e].tolist(), self.val[s:e].tolist()

    @staticmethod
    def window_rows(size: int, r0: int, batch: int) -> list:
        """The rows of a batch in batch order: [r0, size) first, then [0, r0 + batch - size)."""
        return [(r0 + j) % size for j in range(batch)]

    # ---- the device form ----
    def _build(self) -> None:
        if self._built:
            return
        if self._csr is not None:
            row_ptr, col, val, label = self._csr
        else:
            lens = torch.tensor([len(r) for r in self._indices], dtype=torch.int64)
            row_ptr = torch.zeros(len(self._indices) + 1, dtype=torch.int64)
            row_ptr[1:] = torch.cumsum(lens, 0)
            col = torch.tensor([i for r in self._indices for i in r], dtype=torch.int64)
            val = torch.tensor([v for r in self._values for v in r], dtype=torch.float64)
            label = torch.tensor(self._labels, dtype=torch.float64)
        dev = self.device
        row_ptr = row_ptr.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        col64 = col.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        val = val.to(device=dev, dtype=torch.float64).contiguous().view(-1)
        label = label.to(device=dev, dtype=torch.float64).contiguous().view(-1)
        rows, nnz = int(row_ptr.numel()) - 1, int(col64.numel())
        if rows < 1 or rows > JAVA_INT_MAX:
            raise SketchMLException(f"{rows} instances: outside [1, 2^31 - 1]")
        if label.numel() != rows or val.numel() != nnz:
            raise SketchMLException("the CSR arrays do not fit each other")
        lens = row_ptr[1:] - row_ptr[:-1]
        if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != nnz or bool((lens < 0).any()):
            raise SketchMLException("row_ptr must ascend from 0 to nnz")
        row_of = torch.repeat_interleave(torch.arange(rows, device=dev, dtype=torch.int64), lens)
        if nnz:
            if int(col64.min()) < 0 or int(col64.max()) >= self.dim:
                raise SketchMLException(f"a feature index outside [0, {self.dim})")
            same_row = row_of[1:] == row_of[:-1]
            if bool((same_row & (col64[1:] <= col64[:-1])).any()):
                raise SketchMLException("the feature indices of an instance must ascend strictly")
        # (column, row) order: a stable sort by column keeps the rows of a column ascending
        order = torch.sort(col64, stable=True).indices
        counts = torch.bincount(col64, minlength=self.dim)
        col_ptr = torch.zeros(self.dim + 1, dtype=torch.int64, device=dev)
        col_ptr[1:] = torch.cumsum(counts, 0)
        self.row_ptr, self.col, self.val, self.label = row_ptr, col64.to(torch.int32), val, label
        self.col_ptr = col_ptr
        self.csc_row = row_of[order].to(torch.int32)
        self.csc_val = val[order].contiguous()
        self.rows, self.nnz = rows, nnz
        self._csr = (row_ptr, self.col, val, label)
        self._labels = self._indices = self._values = None
        self._built = True

    def glm_data(self) -> _lib.GlmData:
        """The skml_glm_data of this data set; the tensors stay owned by it."""
        self._build()
        d = _lib.GlmData()
        d.rows, d.dim, d.nnz = self.rows, self.dim, self.nnz
        for name in ("row_ptr", "col", "val", "label", "col_ptr", "csc_row", "csc_val"):
            setattr(d, name, C.c_void_p(getattr(self, name).data_ptr()).value)
        return d


class DenseDataSet:
    """A DataSet of dense instances (Parser.parseCSV -> Vectors.dense): rows * dim float64 values,
    row-major, on the device (skml_glm_dense_data, include/skml.h).  Every element takes part in the
    dot and in plusBy, stored zeros included, so the bits are those of a DataSet that stores every
    column; it holds 8 bytes per element instead of 24 and needs no column order.

    DenseDataSet(dim) then add((label, values)) row by row, or fromRows / fromArray.  A row whose
    length is not dim is refused, where the reference's `require` or an array bound would throw.

    xDtype = torch.float32, torch.bfloat16 or torch.float16 stores x in that type instead (a csv value
    parsed to float32 gains nothing from 8 bytes): `x` is then a rows x pitch tensor of that type, the
    rows padded to a multiple of 16 bytes (`pitch` elements, `x_kind` the SKML_X_* id), built with one
    copy at first use.  A device tensor already of that type whose rows are 16-byte aligned (rows x
    dim with dim a multiple of 16 bytes, or a [:, :dim] view of a wider such tensor) is taken as it
    is; a wider input is rounded once, to nearest even, by torch's conversion.  The gradient and the
    validation pass then give the bits of a float64 DenseDataSet over the widened values
    (skml_glm_*_dense_lowp_*), and read a half, a quarter of the bytes.
    """

    dense = True

    def __init__(self, dim: int, device=None, xDtype=None):
        self.dim = int(dim)
        if not 1 <= self.dim <= JAVA_INT_MAX:
            raise SketchMLException(f"dim={dim} outside [1, 2^31 - 1]")
        if xDtype is not None and xDtype not in _lib.X_KINDS:
            raise SketchMLException(f"xDtype={xDtype}: torch.float32, torch.bfloat16, torch.float16, or None for float64")
        self.xDtype = xDtype
        self.x_kind = _lib.X_KINDS.get(xDtype)  # None: float64
        per16 = 16 // torch.empty(0, dtype=xDtype).element_size() if xDtype is not None else 1
        self.pitch = -(-self.dim // per16) * per16
        # the entries of include/skml.h that serve it: skml_glm_*_dense_f64 / _f32, or _dense_lowp_
        self.entry = "dense_" if xDtype is None else "dense_lowp_"
        self.device = _device(device)
        self.readIndex = 0
        self._labels: list = []
        self._values: list = []
        self._arrays = None  # (x, label) as given to fromArray
        self._built = False

    @classmethod
    def fromRows(cls, rows, dim: int, device=None, xDtype=None) -> "DenseDataSet":
        ds = cls(dim, device, xDtype)
        for ins in rows:
            ds.add(ins)
        return ds

    @classmethod
    def fromArray(cls, x, label, dim: int, device=None, xDtype=None) -> "DenseDataSet":
        """x: rows * dim values (rows x dim, or flat and row-major); label: rows values."""
        ds = cls(dim, device, xDtype)
        ds._arrays = (torch.as_tensor(x), torch.as_tensor(label))
        return ds

    def add(self, ins) -> None:
        """data += ins, for ins = (label, values); only before the first use."""
        if self._built or self._arrays is not None:
            raise SketchMLException("DenseDataSet.add after the first use or on arrays: the rows are fixed")
        y, values = ins
        if len(values) != self.dim:
            raise SketchMLException(f"a dense instance of {len(values)} values in a data set of {self.dim} features")
        self._labels.append(float(y))
        self._values.append([float(v) for v in values])

    def __iadd__(self, ins) -> "DenseDataSet":
        self.add(ins)
        return self

    @property
    def size(self) -> int:
        if self._arrays is not None:
            return int(self._arrays[1].numel())
        return len(self._labels)

    take = DataSet.take
    window_rows = staticmethod(DataSet.window_rows)

    def loopingRead(self):
        """(label, values) of the next instance, as a host float and list (a narrow x widened exactly)."""
        r = self.take(1)
        self._build()
        if self.xDtype is not None:
            return float(self.label[r]), self.x[r, :self.dim].double().tolist()
        return float(self.label[r]), self.x[r * self.dim:(r + 1) * self.dim].tolist()

    def _narrow(self, x: torch.Tensor, rows: int) -> torch.Tensor:
        """x as rows x pitch values of xDtype on the device, every row on a 16-byte boundary."""
        x = x.to(device=self.device).reshape(rows, self.dim)
        size = x.element_size()
        if (x.dtype == self.xDtype and x.stride(1) == 1 and x.stride(0) >= self.dim and (x.stride(0) * size) % 16 == 0
                and x.data_ptr() % 16 == 0
                and (x.storage_offset() + rows * x.stride(0)) * size <= x.untyped_storage().nbytes()):  # the last row's pad exists
            self.pitch = x.stride(0)
            return x  # as it is: a view of rows x pitch values
        full = torch.zeros(rows, self.pitch, dtype=self.xDtype, device=self.device)
        full[:, :self.dim] = x  # the one rounding of a wider input
        return full

    def _build(self) -> None:
        if self._built:
            return
        if self._arrays is not None:
            x, label = self._arrays
        else:
            x = torch.tensor(self._values, dtype=torch.float64)
            label = torch.tensor(self._labels, dtype=torch.float64)
        label = label.to(device=self.device, dtype=torch.float64).contiguous().view(-1)
        rows = int(label.numel())
        if rows < 1 or rows > JAVA_INT_MAX:
            raise SketchMLException(f"{rows} instances: outside [1, 2^31 - 1]")
        if x.numel() != rows * self.dim:
            raise SketchMLException(f"{x.numel()} values for {rows} instances of {self.dim} features")
        if self.xDtype is not None:
            x = self._narrow(x, rows)
        else:
            x = x.to(device=self.device, dtype=torch.float64).contiguous().view(-1)
        self.x, self.label, self.rows = x, label, rows
        self._arrays = (x, label)
        self._labels = self._values = None
        self._built = True

    def glm_data(self):
        """The skml_glm_dense_data of this data set, or its skml_glm_dense_lowp_data with an xDtype; the
        tensors stay owned by it."""
        self._build()
        if self.xDtype is not None:
            d = _lib.GlmDenseLowpData()
            d.pitch, d.x_kind = self.pitch, self.x_kind
        else:
            d = _lib.GlmDenseData()
        d.rows, d.dim = self.rows, self.dim
        d.x, d.label = C.c_void_p(self.x.data_ptr()).value, C.c_void_p(self.label.data_ptr()).value
        return d
