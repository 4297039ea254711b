"""The blocked dense gradient without a GPU: the ABI surface, the plan's invariants over a sweep, the `order`
argument's refusals, and skml_glm_dense_blocked.hpp's walks as a stand-alone program
(tests/glm_dense_blocked_check.cpp) under the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface_and_order_argument():
    import torch
    from sketchml_amd import _lib, optim
    from sketchml_amd.data import DataSet, DenseDataSet
    from sketchml_amd.exceptions import SketchMLException
    from sketchml_amd.model import GeneralizedLinearModel, MLConf
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for n in ["skml_glm_gradient_dense_%sblocked_%s" % (lp, t) for lp in ("", "lowp_") for t in ("f64", "f32")]:
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n) and f"int {n}(" in text
        assert _lib._SIGS[n] == _lib._SIGS[n.replace("blocked_", "")]  # the sequential twin's signature
    assert "skml_debug_glm_dense_blocked_plan" in _lib.EXPORTED and "int skml_debug_glm_dense_blocked_plan(" in text
    w = torch.zeros(3, dtype=torch.float64)
    for ds, order in ((DataSet(3, device="cpu"), "blocked"), (DenseDataSet(3, device="cpu"), "tree"), (DataSet(3, device="cpu"), "")):
        with pytest.raises(SketchMLException):
            optim.batch_gradient(w, ds, 0, 1, None, order=order)
        with pytest.raises(SketchMLException):  # refused where it is written, not at the first batch
            GeneralizedLinearModel(MLConf("LinearRegression", "", "csv", 1, 3), ds, ds, gradientOrder=order)
    assert GeneralizedLinearModel(MLConf("LinearRegression", "", "csv", 1, 3), ds, ds).gradientOrder == "sequential"


@pytest.mark.parametrize("xb", [8, 4, 2])
def test_plan_invariants(xb):
    from sketchml_amd import _lib
    for batch in (1, 2, 255, 256, 257, 512, 513, 2048, 131072, 2 ** 31 - 1):
        for dim in (1, 16 // xb * 8, 16 // xb * 8 + 1, 16 // xb * 64, 16 // xb * 64 + 1, 512, 32768, 2 ** 31 - 1):
            lanes, split, inflight, rb, nb, ws = _lib.glm_dense_blocked_plan(xb, batch, dim)
            groups = -(-dim * xb // 16)
            assert lanes in (8, 16, 32, 64) and (lanes >= groups or lanes == 64) and (lanes == 8 or lanes // 2 < groups)
            assert split in (1, 2, 4, 8) and (split == 1 or groups > 64) and inflight == (1 if groups > 64 else 256 // lanes)
            assert rb * nb >= batch > (nb - 1) * rb and rb >= 256 and ws == (nb * dim * 8 if nb > 1 else 0)
            assert ws * 32 <= batch * dim * xb  # the cap: the partial sums are at most 1 / 32 of the window's bytes of x
    for bad in ((3, 1, 1), (8, 0, 1), (8, 1, 0), (4, 2 ** 31, 1), (2, 1, 2 ** 31)):
        assert _lib.glm_dense_blocked_plan(*bad) is None
    assert _lib.lib.skml_debug_glm_dense_blocked_plan(8, 1, 1, None) == -1


def test_walks_on_the_host_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_dense_blocked_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_dense_blocked_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
