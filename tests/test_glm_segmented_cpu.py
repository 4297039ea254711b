"""The segmented sparse gradient without a GPU: the ABI surface, the `order` argument, and skml_glm_segmented.hpp's
walks as a stand-alone program (tests/glm_segmented_check.cpp) under the address and undefined-behaviour sanitizers."""
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
    for n in ("skml_glm_gradient_segmented_f64", "skml_glm_gradient_segmented_f32"):
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n) and f"int {n}(" in text
        assert _lib._SIGS[n] == _lib._SIGS[n.replace("segmented_", "")]  # the sequential twin's signature
    m_seq, split_at, piece, tile = (_lib.glm_segmented_constant(k) for k in ("M_SEQ", "SPLIT_AT", "SLICE", "TILE"))
    assert 1 <= m_seq < piece < split_at and piece % 64 == 0 and tile % 64 == 0 and _lib.lib.skml_debug_glm_segmented_constant(4) == -1
    sparse, dense, conf = DataSet(3, device="cpu"), DenseDataSet(3, device="cpu"), MLConf("LinearRegression", "", "csv", 1, 3)
    assert optim._order_infix(sparse, "segmented") == "segmented_" and "segmented" in optim.ORDERS
    assert GeneralizedLinearModel(conf, sparse, sparse, gradientOrder="segmented").gradientOrder == "segmented"
    with pytest.raises(SketchMLException, match="blocked"):
        optim.batch_gradient(torch.zeros(3, dtype=torch.float64), dense, 0, 1, None, order="segmented")
    with pytest.raises(SketchMLException, match="blocked"):  # refused where it is written, not at the first batch
        GeneralizedLinearModel(conf, dense, dense, gradientOrder="segmented")


def test_walks_on_the_host_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_segmented_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_segmented_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
