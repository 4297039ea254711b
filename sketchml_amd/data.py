"""The training data of the `ml` module: DataSet (ml/data/DataSet.scala:5-25) and the line parsers
(ml/data/Parser.scala:23-76).

A DataSet is the CSR of its sparse instances (row_ptr, col, val, label) plus the same entries in
(column, row) order (col_ptr, csc_row, csc_val), which the mini-batch gradient's column kernel walks
(skml_glm_data, include/skml.h).  A batch of DataSet.loopingRead is a window of consecutive rows, so
the column order is built once, at first use, with a stable sort; nothing is sorted per batch.
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
    """Parser.parseCSV (Parser.scala:45-59) makes dense rows, which the device data set does not hold."""
    raise SketchMLException("parseCSV: dense instances are not built here (DESIGN.md section 9); use parseLibSVM or parseDummy")


class DataSet:
    """ml/data/DataSet.scala over device tensors.

    DataSet(dim) then add((label, indices, values)) row by row, or DataSet.fromCSR(...) /
    DataSet.fromRows(...).  The first use (size stays open until then) checks every row (columns
    strictly ascending inside [0, dim), as Spark's SparseVector requires), moves the CSR to `device`
    and builds the column order there.  readIndex is loopingRead's cursor.
    """

    def __init__(self, dim: int, device=None):
        self.dim = int(dim)
        if not 1 <= self.dim <= JAVA_INT_MAX:
            raise SketchMLException(f"dim={dim} outside [1, 2^31 - 1]")
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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
