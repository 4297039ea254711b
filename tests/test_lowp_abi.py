"""The bf16 / fp16 entries of the dense codec, as far as a machine without a GPU can check them:
the six names are bound, each refuses a NULL context with SKML_E_ARG before it touches a device,
and (where a device is present) as_device_values leaves a 16-bit gradient in its dtype."""
import ctypes as C

import numpy as np
import pytest
import torch

ENCODES = ("skml_dense_encode_bf16", "skml_dense_encode_f16")
DECODES = ("skml_dense_decode_bf16", "skml_dense_decode_f16")
DECODE_SUMS = ("skml_dense_decode_sum_bf16", "skml_dense_decode_sum_f16")


def test_lowp_entries_are_exported():
    from sketchml_amd import _lib
    for name in ENCODES + DECODES + DECODE_SUMS:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib, name)
    # one entry per type, with the fp32 entry's signature
    for names, f32 in ((ENCODES, "skml_dense_encode_f32"), (DECODES, "skml_dense_decode_f32"),
                       (DECODE_SUMS, "skml_dense_decode_sum_f32")):
        for name in names:
            assert _lib._SIGS[name] == _lib._SIGS[f32]


def test_lowp_entries_refuse_a_null_context():
    from sketchml_amd import _lib
    L = _lib.lib
    p = _lib.Params()
    L.skml_params_default(C.byref(p))
    buf = C.c_void_p(4096)  # never dereferenced: the context is checked first
    for name in ENCODES:
        assert getattr(L, name)(None, buf, 16, C.byref(p), buf, 1 << 20) == _lib.SKML_E_ARG
        assert "ctx" in _lib.last_error()
    for name in DECODES:
        assert getattr(L, name)(None, buf, buf, 16) == _lib.SKML_E_ARG
    for name in DECODE_SUMS:
        assert getattr(L, name)(None, buf, 1, 4096, buf, 16, 1.0) == _lib.SKML_E_ARG


@pytest.mark.skipif(not torch.cuda.is_available(), reason="as_device_values places its result on a device")
def test_as_device_values_keeps_16_bit_dtypes():
    from sketchml_amd.context import as_device_values
    for dt in (torch.bfloat16, torch.float16):
        t = as_device_values(torch.arange(40, dtype=torch.float32).to(dt))
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0
    t = as_device_values(np.arange(40, dtype=np.float16))
    assert t.dtype == torch.float16 and t.is_cuda
    assert as_device_values(np.arange(40, dtype=np.float32)).dtype == torch.float32
    assert as_device_values(torch.arange(40, dtype=torch.float64)).dtype == torch.float64
    assert as_device_values(torch.arange(40, dtype=torch.int32)).dtype == torch.float32
