"""FixedPointGradient's codec on the device (ml/gradient/FixedPointGradient.scala:39-75): thin
wrappers over the skml_fixed_* entries of include/skml.h.

A payload is caller-owned device memory: a 64-byte header padded to 256 bytes (norm, numBits, n,
seed, status), then the java.util.BitSet word stream of the codes.  It is relocatable, so the
all-gather moves it as it is and distributed.decode_sum_fixed_point sums the gathered payloads.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .context import LOWP_DTYPES, alloc_aligned, as_device_f32, as_device_values, get_context
from .exceptions import SketchMLException, check


def payload_bytes(n: int, numBits: int) -> int:
    nb = int(_lib.lib.skml_fixed_payload_bytes(int(n), int(numBits)))
    if nb == 0:
        if numBits >= 30 or numBits < 2:
            raise SketchMLException(f"Bit num out of range: {numBits}")  # FixedPointGradient.scala:16
        raise SketchMLException(f"n={n} outside [1, 2^31 - 1]")
    return nb


def encode(values, numBits: int, seed: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """fromArray (FixedPointGradient.scala:39-53) of a device gradient (fp32, or fp64 as the
    reference's double[]; 16-bit tensors are widened to fp32 first, which is exact).  sigma_i is the
    i-th nextBoolean() of java.util.Random(seed).  Returns the payload (uint8, 256-byte aligned);
    `out` reuses a buffer of at least payload_bytes(n, numBits).  Asynchronous: info() reports a
    refused input (NaN, infinity, a norm that is not finite or underflowed to 0)."""
    x = as_device_values(values)
    if x.dtype in LOWP_DTYPES:
        x = as_device_f32(x)
    n = x.numel()
    nb = payload_bytes(n, numBits)
    if out is None:
        out = alloc_aligned(nb, x.device)
    elif out.data_ptr() % 256 or out.numel() * out.element_size() < nb:
        raise SketchMLException(f"payload buffer must be 256-byte aligned and hold {nb} bytes")
    ctx = get_context(x.device)
    fn = _lib.lib.skml_fixed_encode_f64 if x.dtype == torch.float64 else _lib.lib.skml_fixed_encode_f32
    check(fn(ctx.handle, C.c_void_p(x.data_ptr()), n, int(numBits), int(seed), C.c_void_p(out.data_ptr()),
             out.numel() * out.element_size()), "fixed_encode")
    return out


def decode(payload: torch.Tensor, n: int, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """toArray (FixedPointGradient.scala:63-75): the doubles themselves, or their (float)."""
    if dtype not in (torch.float32, torch.float64):
        raise SketchMLException(f"fixed-point decode: unsupported output dtype {dtype}")
    out = torch.empty(int(n), dtype=dtype, device=payload.device)
    ctx = get_context(payload.device)
    fn = _lib.lib.skml_fixed_decode_f64 if dtype == torch.float64 else _lib.lib.skml_fixed_decode_f32
    check(fn(ctx.handle, C.c_void_p(payload.data_ptr()), C.c_void_p(out.data_ptr()), int(n)), "fixed_decode")
    return out


def codes(payload: torch.Tensor, n: int) -> torch.Tensor:
    """BinaryUtils.getBits of every field, as int32."""
    out = torch.empty(int(n), dtype=torch.int32, device=payload.device)
    ctx = get_context(payload.device)
    check(_lib.lib.skml_fixed_codes_i32(ctx.handle, C.c_void_p(payload.data_ptr()), C.c_void_p(out.data_ptr()),
                                        int(n)), "fixed_codes")
    return out


def info(payload: torch.Tensor, strict: bool = True) -> _lib.FixedHeader:
    """Synchronise and read the header.  A refused input raises SketchMLException unless strict is
    False (the header's status then says SKML_E_NAN)."""
    hdr = _lib.FixedHeader()
    ctx = get_context(payload.device)
    st = _lib.lib.skml_fixed_info(ctx.handle, C.c_void_p(payload.data_ptr()), C.byref(hdr))
    if st == _lib.SKML_E_NAN:
        if strict:
            raise SketchMLException("fixed_info: " + _lib.last_error())
        return hdr
    check(st, "fixed_info")
    return hdr


def times_by(payload: torch.Tensor, x: float) -> None:
    """timesBy (FixedPointGradient.scala:55): norm *= x."""
    ctx = get_context(payload.device)
    check(_lib.lib.skml_fixed_times_by(ctx.handle, C.c_void_p(payload.data_ptr()), float(x)), "fixed_times_by")
