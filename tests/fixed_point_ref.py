"""numpy restatement of FixedPointGradient's codec (test infrastructure only).

The rules are the reference's (ml/gradient/FixedPointGradient.scala:39-75,
sketch/binary/BinaryUtils.java:6-29), with the library's one addition: the coin flips sigma_i,
which the reference draws from an unseeded global Bernoulli(0.5) (FixedPointGradient.scala:10,47),
are the i-th nextBoolean() of java.util.Random(seed), i from 0 (oracle/np_oracle.py::lcg_bit).
All arithmetic is IEEE double in the reference's order: numpy's element-wise divide, multiply and
floor are correctly rounded single operations, as the JVM's are.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle.np_oracle import MASK48, MULT, JRandom, lcg_bit  # noqa: F401  (JRandom, lcg_bit: re-exported)


@functools.lru_cache(maxsize=8)
def sigma_stream(seed: int, n: int) -> np.ndarray:
    """sigma_0 .. sigma_{n-1}: bit 47 of java.util.Random(seed)'s state after i + 1 steps
    (Random.next(1), as nextBoolean reads it).  Built by doubling: the states of steps
    [m + 1, 2m] are A^m s + C_m of the states of steps [1, m] (uint64 products wrap mod 2^64, a
    multiple of 2^48).  Read-only; shared between tests."""
    s = np.empty(max(n, 1), dtype=np.uint64)
    s[0] = ((((seed ^ MULT) & MASK48) * MULT) + 0xB) & MASK48
    a, c, m = MULT, 0xB, 1
    while m < n:
        k = min(m, n - m)
        s[m:m + k] = (np.uint64(a) * s[:k] + np.uint64(c)) & np.uint64(MASK48)
        c = (a * c + c) & MASK48
        a = (a * a) & MASK48
        m *= 2
    out = ((s[:n] >> np.uint64(47)) & np.uint64(1)).astype(np.int64)
    out.setflags(write=False)
    return out


def norm_sequential(values) -> float:
    """norm = 0; values.foreach(v => norm += v * v); Math.sqrt(norm) (FixedPointGradient.scala:41-43)."""
    acc = 0.0
    for v in np.asarray(values, dtype=np.float64).tolist():
        acc += v * v
    return math.sqrt(acc)


def encode_codes(values, num_bits: int, seed: int, norm: float | None = None) -> np.ndarray:
    """x_i = Math.floor(Math.abs(v_i) / norm * max).toInt + sigma_i; x_i |= sign when v_i < 0
    (FixedPointGradient.scala:44-51).  Scala's Double.toInt turns NaN (0 / 0 when norm is 0) into 0.
    `norm`: the norm to divide by (the device's, when its codes are checked); default the
    reference's sequential sum."""
    v = np.asarray(values, dtype=np.float64)
    if norm is None:
        norm = norm_sequential(v)
    maxv = (1 << (num_bits - 1)) - 1
    sign = 1 << (num_bits - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.floor(np.abs(v) / np.float64(norm) * np.float64(maxv))
    x = np.where(np.isnan(q), 0.0, q).astype(np.int64) + sigma_stream(int(seed), len(v))
    x = np.where(v < 0, x | sign, x)  # a plain <: -0.0 gets no sign
    return x.astype(np.int64)


def pack_words(codes, num_bits: int) -> np.ndarray:
    """BinaryUtils.setBits (BinaryUtils.java:6-14) of code i at offset i * numBits, most significant
    bit first, into a java.util.BitSet; the result is BitSet.toLongArray padded with zero words to
    ceil(n * numBits / 64): stream bit k is bit k & 63 of word k >> 6.  Offsets are 64-bit here."""
    codes = np.asarray(codes, dtype=np.int64)
    n = len(codes)
    nwords = (n * num_bits + 63) // 64
    full = np.zeros(nwords * 64, dtype=np.uint8)
    field = full[: n * num_bits].reshape(n, num_bits)
    for j in range(num_bits):  # stream bit j of a field is bit numBits - 1 - j of the code
        field[:, j] = (codes >> (num_bits - 1 - j)) & 1
    return np.packbits(full.reshape(nwords, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def unpack_codes(words, n: int, num_bits: int) -> np.ndarray:
    """BinaryUtils.getBits (BinaryUtils.java:20-29) of every field."""
    w = np.ascontiguousarray(words, dtype="<u8")
    bits = np.unpackbits(w.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    field = bits[: n * num_bits].reshape(n, num_bits)
    res = np.zeros(n, dtype=np.int64)
    for j in range(num_bits):  # res <<= 1; res |= bit
        res = (res << 1) | field[:, j]
    return res


def decode_values(codes, num_bits: int, norm: float) -> np.ndarray:
    """v = (x & mask).toDouble / max * norm; v = -v when x & sign (FixedPointGradient.scala:69-71)."""
    x = np.asarray(codes, dtype=np.int64)
    maxv = (1 << (num_bits - 1)) - 1
    sign = 1 << (num_bits - 1)
    v = (x & maxv).astype(np.float64) / np.float64(maxv) * np.float64(norm)
    return np.where((x & sign) != 0, -v, v)


def decode_sum(values_per_payload, scale: float) -> np.ndarray:
    """(float)(scale * sum_p v_p) with the sum in double from +0.0 in payload order
    (Gradient.sum adds into a zeroed DenseDoubleGradient, ml/gradient/Gradient.scala:44-49)."""
    acc = np.zeros(len(values_per_payload[0]), dtype=np.float64)
    for v in values_per_payload:
        acc = acc + v
    return (acc * np.float64(scale)).astype(np.float32)
