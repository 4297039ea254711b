"""FixedPointGradient without a GPU: the numpy restatement against the issue's worked examples, the
word layout for every width, the Python surface and the C ABI's argument checks (which run before
any device work)."""
import ctypes as C

import numpy as np
import pytest

from oracle.np_oracle import JRandom, lcg_bit
from tests import fixed_point_ref as R


def test_sigma_stream_is_java_random_next_boolean():
    for seed in (0, 5, -3, 123456789):
        rng = JRandom(seed)
        want = [int(rng.next_boolean()) for _ in range(300)]
        assert R.sigma_stream(seed, 300).tolist() == want
    s = R.sigma_stream(7, 70001)
    for i in (0, 1, 63, 64, 4095, 4096, 65535, 70000):
        assert s[i] == lcg_bit(7, i)


def test_worked_example_six_values():
    v = np.array([3.0, -4.0, 0.0, 12.0, -0.0, -13.0])
    assert R.sigma_stream(0, 6).tolist() == [1, 1, 0, 1, 1, 0]
    assert R.norm_sequential(v) == np.sqrt(338.0)
    codes = R.encode_codes(v, 4, 0)
    assert codes.tolist() == [2, 10, 0, 5, 1, 12]
    words = R.pack_words(codes, 4)
    assert words.tolist() == [0x38A054]
    assert R.unpack_codes(words, 6, 4).tolist() == [2, 10, 0, 5, 1, 12]
    dec = R.decode_values(codes, 4, np.sqrt(338.0))
    n = np.sqrt(338.0)
    assert dec.tolist() == [2.0 / 7.0 * n, -(2.0 / 7.0 * n), 0.0, 5.0 / 7.0 * n, 1.0 / 7.0 * n, -(4.0 / 7.0 * n)]


def test_worked_example_single_value_decodes_to_minus_zero():
    assert lcg_bit(0, 0) == 1
    codes = R.encode_codes(np.array([5.0]), 4, 0)
    assert codes.tolist() == [8]  # max + 1 = sign
    assert R.pack_words(codes, 4).tolist() == [0x1]
    dec = R.decode_values(codes, 4, 5.0)
    assert dec[0] == 0.0 and np.signbit(dec[0])


def test_all_zero_input_codes_are_the_coin_flips():
    codes = R.encode_codes(np.zeros(100), 8, 3)  # norm 0: the quotient is NaN, .toInt gives 0
    assert codes.tolist() == R.sigma_stream(3, 100).tolist()
    dec = R.decode_values(codes, 8, 0.0)
    assert not dec.any() and not np.signbit(dec).any()


@pytest.mark.parametrize("bits", range(2, 30))
def test_words_unpack_to_codes(bits):
    n = 129
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 1 << bits, n)
    codes[0], codes[-1] = (1 << bits) - 1, 1 << (bits - 1)
    words = R.pack_words(codes, bits)
    assert len(words) == (n * bits + 63) // 64
    assert np.array_equal(R.unpack_codes(words, n, bits), codes)
    # the tail bits past n * bits are zero, and every field is most significant bit first
    tail = n * bits - 64 * (len(words) - 1)
    assert tail == 64 or int(words[-1]) >> tail == 0
    assert int(words[0]) & ((1 << bits) - 1) == (1 << bits) - 1
    k = (n - 1) * bits
    assert (int(words[k >> 6]) >> (k & 63)) & 1 == 1  # the last code's top bit is its first stream bit


def test_python_surface():
    import sketchml_amd as sk
    assert sk.Kind.FixedPoint.value == "FixedPoint"
    assert sk.FixedPointGradient().kind() == sk.Kind.FixedPoint
    for name in ("encode", "decode", "codes", "info", "times_by"):
        assert callable(getattr(sk.fixed_point, name))
    assert callable(sk.decode_sum_fixed_point) and callable(sk.compress)
    for name in ("zip", "Zip", "float"):
        with pytest.raises(sk.SketchMLException, match="not built"):
            sk.compress(None, name)
    with pytest.raises(sk.SketchMLException, match="Unrecognizable compressor"):
        sk.compress(None, "lz4")
    marker = object()
    assert sk.compress(marker, "none") is marker and sk.compress(marker, "None") is marker
    for bits in (1, 30):
        with pytest.raises(sk.SketchMLException, match="Bit num out of range"):
            sk.FixedPointGradient(None, bits)

    class _Other:
        dim = 4

        def kind(self):
            return sk.Kind.Sketch

    with pytest.raises(sk.SketchMLException, match="Cannot create FixedPoint from Sketch"):
        sk.FixedPointGradient(_Other(), 8)


def test_payload_bytes():
    from sketchml_amd import _lib
    f = _lib.lib.skml_fixed_payload_bytes
    assert f(1, 2) == 256 + 256            # one word, padded to 256 bytes
    assert f(6, 4) == 512
    assert f(4096, 8) == 256 + 4096        # 512 words
    assert f(4097, 3) == 256 + 1792        # ceil(12291 / 64) = 193 words = 1,544 bytes -> 1,792
    assert f(129, 29) == 256 + 512         # 59 words
    assert f((1 << 28), 8) == 256 + (1 << 28)
    assert f((1 << 31) - 1, 29) == 256 + ((((1 << 31) - 1) * 29 + 63) // 64 * 8 + 255) // 256 * 256
    for n, b in ((0, 8), (-1, 8), (1 << 31, 8), (10, 1), (10, 30), (10, 0)):
        assert f(n, b) == 0
    assert C.sizeof(_lib.FixedHeader) == 64 and _lib.FixedHeader.norm.offset == 24
    assert _lib.FixedHeader.words_offset.offset == 32 and _lib.FixedHeader.seed.offset == 40


def test_encode_refuses_bad_arguments_before_any_device_work():
    from sketchml_amd import _lib
    assert {"skml_fixed_encode_f32", "skml_fixed_encode_f64", "skml_fixed_decode_f32", "skml_fixed_decode_f64",
            "skml_fixed_decode_sum_f32", "skml_fixed_codes_i32", "skml_fixed_times_by", "skml_fixed_info",
            "skml_fixed_payload_bytes"} <= set(_lib._SIGS)
    for fn in (_lib.lib.skml_fixed_encode_f32, _lib.lib.skml_fixed_encode_f64):
        for n, bits, what in ((10, 1, "Bit num out of range: 1"), (10, 30, "Bit num out of range: 30"), (0, 8, "n=0")):
            assert fn(None, None, n, bits, 0, None, 0) == _lib.SKML_E_ARG
            assert what in _lib.last_error()
