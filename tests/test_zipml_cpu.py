"""ZipMLQuantizer without a GPU: known answers of the numpy restatement (tests/zipml_ref.py), the
Python surface, the numpy model of the device's prefix-sum tree (tests/zip_scan_model.py) against exact
sums, and the round arithmetic the kernels share (sketchml_amd/csrc/skml_zip.hpp) driven
by a host loop against a sequential implementation, under the address and undefined-behaviour
sanitizers, as a stand-alone program (tests/zip_check.cpp)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import zip_scan_model as M
from tests import zipml_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ten_values_by_hand():
    """sorted = the triangular numbers 0..45 (gaps 1..9), B = 4.  Round 1 (splitNum 10, thrNum 2):
    the pairs' errors are gap^2 / 2 = 0.5, 4.5, 12.5, 24.5, 40.5, the 2nd largest of them and five
    zeros is 24.5, pairs 3 and 4 stay split: splitIndex = 0 2 4 6 7 8 9.  Round 2 (splitNum 7, odd,
    thrNum 1): ranges [0,3], [4,6], [7,8] have errors 21, 60.67, 32; only the middle one stays
    split: 0 4 6 7, and the singleton 9 is dropped.  binNum 4, splits = sorted[4], [6], [7]."""
    x = np.array([15.0, 0.0, 45.0, 3.0, 28.0, 1.0, 36.0, 6.0, 21.0, 10.0])
    z = Z.quantize(x, 4)
    assert z.status == Z.OK and z.rounds == 2 and z.bin_num == 4
    assert z.split_index.tolist() == [0, 4, 6, 7]
    assert z.splits.tolist() == [10.0, 21.0, 28.0]
    assert (z.min, z.max, z.zero_idx) == (0.0, 45.0, 0)
    assert z.values().tolist() == [5.0, 15.5, 24.5, 36.5]
    assert z.bins(x).tolist() == [1, 0, 3, 0, 3, 0, 3, 0, 2, 1]
    # round 1 alone
    s = Z.java_sort(x)
    r, t = Z.prefix_sums(s)
    assert Z.round_errors(np.arange(10), 10, 10, r, t).tolist() == [0.5, 4.5, 12.5, 24.5, 40.5]
    assert Z.select_kth_largest(np.array([0.5, 4.5, 12.5, 24.5, 40.5, 0, 0, 0, 0, 0]), 2) == 24.5


def test_java_sort_orders_signed_zeros():
    x = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 5e-324, -5e-324])
    s = Z.java_sort(x)
    assert s.view(np.uint64).tolist() == np.array([-1.0, -5e-324, -0.0, -0.0, 0.0, 0.0, 5e-324, 1.0]).view(np.uint64).tolist()


def test_n_not_above_bins_runs_no_round():
    x = np.array([3.0, -1.0, 2.0, -0.5, 7.0])
    for bins in (5, 8, 256):
        z = Z.quantize(x, bins)
        assert z.status == Z.OK and z.rounds == 0 and z.bin_num == 5
        assert z.splits.tolist() == [-0.5, 2.0, 3.0, 7.0] and (z.min, z.max) == (-1.0, 7.0) and z.zero_idx == 1


@pytest.mark.parametrize("bins", [4, 16, 256])
@pytest.mark.parametrize("n", [257, 258, 300, 1000, 4097, 65539])
def test_terminates_on_gaussian(n, bins):
    x = (np.random.default_rng(n).standard_normal(n) * 1e-3).astype(np.float32)
    z = Z.quantize(x, bins)
    assert z.status == Z.OK and z.bin_num in (bins, bins - 1)
    assert 1 <= z.rounds <= 20 or n <= bins
    assert len(z.splits) == z.bin_num - 1 and np.all(np.diff(z.splits) >= 0)
    assert z.min == float(x.min()) and z.max == float(x.max())


def test_no_progress_and_thr_zero():
    z = Z.quantize(np.full(300, 0.25), 256)
    assert z.status == Z.NO_PROGRESS and z.stuck_at == 300 and z.rounds == 0
    z = Z.quantize(Z.mostly_zeros(), 256)  # ten rounds go well, then the zeros' ties keep every split
    assert z.status == Z.NO_PROGRESS and z.stuck_at == 260 and z.rounds == 10
    x = np.random.default_rng(1).standard_normal(1000)
    for bins in (2, 3):
        assert Z.quantize(x, bins).status == Z.THR_ZERO


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scan_input(name, n):
    """The inputs of tests/test_gpu_zipml.py's _gauss, and the two with long runs of equal values."""
    if name == "mostly_zeros":
        return Z.mostly_zeros(n, 1)
    x = np.random.default_rng(1000 + n).standard_normal(n) * 1e-3
    if name == "bf16":
        return Z.bf16_rounded(x.astype(np.float32))
    return x.astype(np.float32) if name == "f32" else x


@pytest.mark.parametrize("name,n", [(k, n) for n in (257, 2049, 4097, 65539) for k in ("f32", "f64")]
                         + [("mostly_zeros", 65539), ("bf16", 65539)])
def test_scan_tree_model_gives_the_correctly_rounded_sums(name, n):
    """The tree of k_zip_scan_dd in numpy (hi + lo pairs, exact squares) against the exact sums in
    Python integers rounded once: equal at every index, r and t, which is what the GPU tests ask of
    the kernel on these inputs.  The same tree in plain double is not (nor is np.cumsum), so that
    test tells a tree that lost its low parts from one that kept them."""
    s = Z.java_sort(_scan_input(name, n).astype(np.float64))
    r, t = M.scan(s)
    er, et = M.exact_prefix_sums(s)
    assert np.array_equal(_bits(r), _bits(er)) and np.array_equal(_bits(t), _bits(et))
    pr, pt = M.scan(s, M.zdd_add_plain)
    cr, ct = Z.prefix_sums(s)
    if name in ("f32", "bf16"):  # 24-bit values: small sums of them are exact in any order, the squares' are not
        assert not np.array_equal(_bits(pt), _bits(et)) and not np.array_equal(_bits(ct), _bits(et))
    else:
        assert not np.array_equal(_bits(pr), _bits(er)) and not np.array_equal(_bits(pt), _bits(et))
        assert not np.array_equal(_bits(cr), _bits(er)) and not np.array_equal(_bits(ct), _bits(et))
    if name == "mostly_zeros":
        run = np.nonzero(s == 0)[0]
        assert len(run) == 58968 and run[-1] - run[0] + 1 == len(run)
        assert len(np.unique(_bits(r[run]))) == 1 and len(np.unique(_bits(t[run]))) == 1


def test_scan_tree_model_pieces():
    """Exact squares (p + e = v * v in integers), exact sums by hand, and the model on integers, where
    every order gives np.cumsum."""
    v = np.random.default_rng(7).standard_normal(1000) * 1e-3
    p, e = M.two_square(v)
    vi = M.as_ints(v, -140)
    assert np.array_equal(M.as_ints(p, -280) + M.as_ints(e, -280), vi * vi) and np.array_equal(p, v * v)
    r, t = M.exact_prefix_sums(np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]))
    assert r.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51]  # ties to even: 1 + 1/2 ulp down, 1 + 3/2 ulp up
    assert t.tolist() == [1.0, 1.0, 1.0, 1.0]
    x = np.sort(np.random.default_rng(3).permutation(np.arange(-(1 << 17), 1 << 17))[:5000].astype(np.float64))
    r, t = M.scan(x)
    assert np.array_equal(_bits(r), _bits(np.cumsum(x))) and np.array_equal(_bits(t), _bits(np.cumsum(x * x)))


def test_python_surface():
    import sketchml_amd as sk
    from sketchml_amd import _lib
    assert sk.Kind.Zip.value == "Zip" and sk.ZipGradient().kind() == sk.Kind.Zip
    q = sk.ZipMLQuantizer(16)
    assert isinstance(q, sk.Quantizer) and q.binNum == 16 and sk.ZipMLQuantizer().binNum == 256
    with pytest.raises(NotImplementedError):
        q.quantizationType()
    for name in ("skml_zip_workspace_bytes", "skml_zip_encode_f32", "skml_zip_encode_f64", "skml_debug_zip_prefix_f32",
                 "skml_debug_zip_prefix_f64", "skml_debug_zip_rounds", "skml_zip_release_workspace"):
        assert name in _lib._SIGS
    # argument checks that need no device
    assert _lib.lib.skml_zip_workspace_bytes(1, 0) == 0 and _lib.lib.skml_zip_workspace_bytes(1 << 31, 0) == 0
    for n in (2, 1 << 20, 1 << 28):
        assert 36 * n <= _lib.lib.skml_zip_workspace_bytes(n, 0) <= 37 * n + (1 << 20)
        assert 44 * n <= _lib.lib.skml_zip_workspace_bytes(n, 1) <= 45 * n + (1 << 20)
    for bins in (2, 3, 65537):
        assert _lib.lib.skml_zip_encode_f32(None, None, 100, bins, None, 0) == _lib.SKML_E_ARG
    assert _lib.lib.skml_zip_encode_f32(None, None, 1, 256, None, 0) == _lib.SKML_E_ARG
    with pytest.raises(sk.SketchMLException, match="ZipGradient"):
        sk.compress(None, "zip")


def test_round_arithmetic_on_the_host_under_sanitizers():
    """tests/zip_check.cpp: the shared helpers (keys, pair ranges and errors, the select's digit walk,
    the compaction offsets) in a host loop shaped like the kernels' against a plain sequential
    ZipMLQuantizer, on LCG inputs at n = 257, 258, 300, 1000, 4097, 65539 and B = 4, 16, 256, built
    with -fsanitize=address,undefined and run as a program of its own."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "zip_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "zip_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok 18 searches, 2 refusals", out.stdout + out.stderr
