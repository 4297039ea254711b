"""sketchml_amd -- MI355X-native SketchML gradient codec.

The hot path (k=128 quantile sketch, bucket quantisation, packed codes, sparse key/value
codec) runs in hand-written gfx950 HIP kernels in lib/libskml.so behind the C ABI of
include/skml.h; this package mirrors the reference's Java surface over that ABI.
"""
from . import _lib, data, fixed_point, loss, model, optim, validation
from .compressor import DenseVectorCompressor
from .constants import Constants, Parallel
from .data import DataSet, parseCSV, parseDummy, parseLibSVM
from .context import Context, alloc_aligned, get_context
from .exceptions import QuantileSketchException, SketchMLException
from .loss import L1LogLoss, L2HingeLoss, L2LogLoss, L2SquareLoss, Loss
from .model import GeneralizedLinearModel, LinearRegModel, LRModel, MLConf, SVMModel
from .optim import Adam, GradientDescent
from .validation import ValidationResult, calLossAucPrecision, calLossPrecision
from .distributed import decode_sum_fixed_point, decode_sum_update, decode_sum_update_fixed_point
from .gradient import DenseDoubleGradient, FixedPointGradient, Kind, SketchGradient, SparseDoubleGradient, ZipGradient, compress
from .quantization import QuantileQuantizer, QuantizationType, Quantizer, UniformQuantizer, ZipMLQuantizer
from .sparse import (DeltaAdaptiveEncoder, GroupedMinMaxSketch, SparsePayload, SparseVectorCompressor, decode_sum,
                     encode_dense_as_sparse, encode_sparse, to_sparse)

__all__ = ["optim", "data", "loss", "model", "validation", "calLossPrecision", "calLossAucPrecision", "ValidationResult", "MLConf",
           "GeneralizedLinearModel", "LRModel", "SVMModel", "LinearRegModel", "DataSet", "parseLibSVM", "parseDummy", "parseCSV", "Loss", "L1LogLoss", "L2HingeLoss",
           "L2LogLoss", "L2SquareLoss", "GradientDescent", "Adam", "decode_sum_update", "decode_sum_update_fixed_point", "ZipGradient", "ZipMLQuantizer", "FixedPointGradient", "compress", "decode_sum_fixed_point", "fixed_point", "Constants", "Parallel", "DenseDoubleGradient", "Kind", "SketchGradient", "SparseDoubleGradient", "Context", "DeltaAdaptiveEncoder", "DenseVectorCompressor", "GroupedMinMaxSketch", "SparsePayload",
           "SparseVectorCompressor", "decode_sum", "encode_dense_as_sparse", "encode_sparse", "to_sparse", "QuantileQuantizer", "QuantizationType", "Quantizer", "UniformQuantizer",
           "QuantileSketchException", "SketchMLException", "get_context", "alloc_aligned"]

LIB_PATH = _lib.LIB_PATH
