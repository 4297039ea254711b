"""The K-model dense gradient without a GPU: the ABI surface, the plan's invariants and partial-sum cap over a sweep,
the Python entries' refusals, and skml_glm_dense_multi.hpp's walks as a stand-alone program
(tests/glm_dense_multi_check.cpp) under the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface_and_python_refusals():
    import torch
    from sketchml_amd import _lib, optim
    from sketchml_amd.data import DataSet, DenseDataSet, one_vs_rest_labels
    from sketchml_amd.exceptions import SketchMLException
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for n in ["skml_glm_gradient_dense_%smulti_%s" % (lp, t) for lp in ("", "lowp_") for t in ("f64", "f32")]:
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n) and f"int {n}(" in text
        blocked = _lib._SIGS[n.replace("multi_", "blocked_")][1]  # the blocked entry's arguments, with models and labels_dev
        assert _lib._SIGS[n][1] == blocked[:5] + [_lib._SIGS[n][1][5], blocked[5], blocked[5]] + blocked[6:]
    assert "skml_debug_glm_dense_multi_plan" in _lib.EXPORTED and "int skml_debug_glm_dense_multi_plan(" in text
    w = torch.zeros(2, 3, dtype=torch.float64)
    for ds, weights in ((DataSet(3, device="cpu"), w), (DenseDataSet(3, device="cpu"), w[0]), (DenseDataSet(3, device="cpu"), w[:, :2])):
        with pytest.raises(SketchMLException):
            optim.batch_gradient_multi(weights, ds, 0, 1, None)
    assert one_vs_rest_labels([2, 0, 2], [0, 2], "cpu").tolist() == [[-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]]


@pytest.mark.parametrize("xb", [8, 4, 2])
def test_plan_invariants_and_the_partial_sum_cap(xb):
    from sketchml_amd import _lib
    e = 16 // xb
    for models in (1, 2, 15, 16):
        for batch in (1, 2, 255, 256, 257, 1024, 1025, 2048, 65535, 65536, 131072, 2 ** 31 - 1):
            for dim in (1, 4 * e - 1, 4 * e + 1, 16 * (8 // xb) * 2 + 1, 512, 32768, 2 ** 31 - 1):
                tile, r, s, lane_cols, strip, rb, nb, ws = _lib.glm_dense_multi_plan(xb, models, batch, dim)
                tiles = -(-batch // 16)
                assert (tile, lane_cols, strip) == (16, e, 32 * (8 // xb)) and r == (4 if tiles >= 4096 else 1)
                assert s in (1, 2, 4, 8) and (s == 1 or (r == 1 and tiles * s <= 1024 and -(-dim // (4 * e)) >= 2 * s))
                assert rb * nb >= batch > (nb - 1) * rb and rb % 32 == 0 and rb >= 256 and ws == (nb * models * dim * 8 if nb > 1 else 0)
                assert ws * 8 <= batch * dim * xb  # the cap: the partial sums are at most 1 / 8 of the window's bytes of x
    for bad in ((3, 1, 1, 1), (8, 0, 1, 1), (8, 17, 1, 1), (8, 1, 0, 1), (8, 1, 1, 0), (4, 1, 2 ** 31, 1), (2, 1, 1, 2 ** 31)):
        assert _lib.glm_dense_multi_plan(*bad) is None
    assert _lib.lib.skml_debug_glm_dense_multi_plan(8, 1, 1, 1, None) == -1


def test_walks_on_the_host_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_dense_multi_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_dense_multi_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
