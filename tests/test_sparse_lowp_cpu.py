"""The bf16 / fp16 entries of the sparse codec, as far as a machine without a GPU can check them:
the seven names are bound with their fp32 / fp64 twins' signatures, each refuses a NULL context with
SKML_E_ARG before it touches a device, and the HIP-free header the compaction kernels take their
16-bit keep tests from agrees with the fp32 test of the widened value for every pattern
(tests/sparse_lowp_check.cpp under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMPACTS = ("skml_sparse_compact_bf16", "skml_sparse_compact_f16")
ENCODES = ("skml_sparse_encode_bf16", "skml_sparse_encode_f16")
DECODE_SUMS = ("skml_sparse_decode_sum_f32", "skml_sparse_decode_sum_bf16", "skml_sparse_decode_sum_f16")


def test_sparse_lowp_entries_are_exported():
    from sketchml_amd import _lib
    for name in COMPACTS + ENCODES + DECODE_SUMS:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib, name)
    for names, twin in ((COMPACTS, "skml_sparse_compact_f32"), (ENCODES, "skml_sparse_encode_f32"),
                        (DECODE_SUMS, "skml_sparse_decode_sum_f64")):
        for name in names:
            assert _lib._SIGS[name] == _lib._SIGS[twin]


def test_sparse_lowp_entries_refuse_a_null_context():
    from sketchml_amd import _lib
    L = _lib.lib
    p = _lib.Params()
    L.skml_params_default(C.byref(p))
    buf = C.c_void_p(4096)  # never dereferenced: the context is checked first
    nnz = C.c_int64(-7)
    for name in COMPACTS:
        assert getattr(L, name)(None, buf, 16, buf, buf, C.byref(nnz)) == _lib.SKML_E_ARG
        assert nnz.value == -7
    out = C.c_void_p()
    for name in ENCODES:
        assert getattr(L, name)(None, buf, 16, C.byref(p), C.byref(out)) == _lib.SKML_E_ARG
        assert not out.value
    for name in DECODE_SUMS:
        assert getattr(L, name)(None, buf, 1, 4096, 16, 1.0, buf) == _lib.SKML_E_ARG


def test_lowp_keep_tests_and_widenings_on_the_host_under_sanitizers():
    """tests/sparse_lowp_check.cpp: skml_lowp.hpp's keep_bf16_bits / keep_f16_bits against
    keep_f32_bits of the widened value and against |x| > 1e-8 in double (NaN out, +-inf in), and
    widen_bf16_bits / widen_f16_bits against the value the pattern's fields spell out, for all
    65,536 patterns of both types; built with -fsanitize=address,undefined and run as a program of
    its own."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sparse_lowp_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "sparse_lowp_check.cpp")],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok 131072 patterns", out.stdout + out.stderr
