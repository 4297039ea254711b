"""Dense instances stored as fp32, bf16 or fp16, without a GPU: DenseDataSet's xDtype (storage type, pitch and
pad, window, loopingRead, refusals, the default path unchanged), the ABI surface, and skml_glm_dense_lowp.hpp's
slab and column arithmetic as a stand-alone program (tests/glm_dense_lowp_check.cpp) under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import glm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(torch.float32, 0, 4), (torch.bfloat16, 1, 8), (torch.float16, 2, 8)]  # type, SKML_X_*, elements per 16 bytes


@pytest.mark.parametrize("dt,kind,per16", KINDS)
def test_dense_dataset_with_x_dtype(dt, kind, per16):
    from sketchml_amd import _lib
    from sketchml_amd.data import DenseDataSet
    from sketchml_amd.exceptions import SketchMLException
    x = np.arange(55.0).reshape(5, 11) / 3.0 - 4.0  # thirds: every type rounds them, once
    y = [1.0, -1.0, 1.0, 1.0, -1.0]
    ds, ri = DenseDataSet.fromArray(x, y, 11, device="cpu", xDtype=dt), 0
    d, want = ds.glm_data(), torch.from_numpy(x).to(dt)
    assert isinstance(d, _lib.GlmDenseLowpData) and (d.rows, d.dim, d.pitch, d.x_kind) == (5, 11, -(-11 // per16) * per16, kind)
    assert (ds.x_kind, ds.pitch, ds.entry, ds.dense) == (kind, d.pitch, "dense_lowp_", True)
    assert ds.x.dtype == dt and ds.x.shape == (5, d.pitch) and d.x == ds.x.data_ptr() and d.x % 16 == 0 and ds.label.dtype == torch.float64
    assert torch.equal(ds.x[:, :11], want) and not ds.x[:, 11:].any()
    for batch in (2, 3, 4, 5, 1, 4):  # the window is the float64 data set's
        rows, ri = R.window_rows(5, ri, batch)
        assert DenseDataSet.window_rows(5, ds.take(batch), batch) == rows and ds.readIndex == ri
    ds.readIndex = 4
    assert ds.loopingRead() == (-1.0, want[4].double().tolist()) and ds.loopingRead() == (1.0, want[0].double().tolist())
    rows = DenseDataSet.fromRows([(y[r], list(x[r])) for r in range(5)], 11, device="cpu", xDtype=dt)
    assert rows.glm_data().pitch == d.pitch and torch.equal(rows.x, ds.x)
    # taken as it is: a tensor of the type whose rows are 16-byte aligned, contiguous or a view of padded rows
    whole = torch.from_numpy(np.arange(48.0).reshape(3, 16)).to(dt)
    as_is = DenseDataSet.fromArray(whole, y[:3], 16, device="cpu", xDtype=dt)
    padded = torch.full((3, 2 * per16), float("nan"), dtype=dt)
    padded[:, :per16 + 1] = 2.5
    view = DenseDataSet.fromArray(padded[:, :per16 + 1], y[:3], per16 + 1, device="cpu", xDtype=dt)
    assert as_is.glm_data().x == whole.data_ptr() and as_is.pitch == 16
    assert view.glm_data().x == padded.data_ptr() and view.pitch == 2 * per16 and view.loopingRead() == (1.0, [2.5] * (per16 + 1))
    for bad in (lambda: DenseDataSet(3, device="cpu", xDtype=torch.float64), lambda: DenseDataSet(3, device="cpu", xDtype=torch.int32),
                lambda: DenseDataSet.fromArray(np.zeros(7), np.zeros(2), 3, device="cpu", xDtype=dt).glm_data(),
                lambda: DenseDataSet(3, device="cpu", xDtype=dt).add((1.0, [1.0, 2.0])), lambda: ds.add((1.0, [0.0] * 11))):
        with pytest.raises(SketchMLException):
            bad()


def test_the_default_path_is_unchanged():
    from sketchml_amd import _lib
    from sketchml_amd.data import DataSet, DenseDataSet
    ds = DenseDataSet.fromArray(np.arange(6, dtype=np.float32).reshape(2, 3), [1.0, -1.0], 3, device="cpu")
    d = ds.glm_data()
    assert isinstance(d, _lib.GlmDenseData) and ds.x.dtype == torch.float64 and ds.x.shape == (6,) and d.x == ds.x.data_ptr()
    assert (ds.x_kind, ds.pitch, ds.entry, DataSet.entry) == (None, 3, "dense_", "") and ds.loopingRead() == (1.0, [0.0, 1.0, 2.0])


def test_abi_surface():
    from sketchml_amd import _lib
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for n in ["skml_glm_%s_dense_lowp_%s" % (e, t) for e in ("gradient", "validate") for t in ("f64", "f32")]:
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n) and f"int {n}(" in text
        assert _lib._SIGS[n][1][2:] == _lib._SIGS[n.replace("_lowp", "")][1][2:]  # the dense twin's arguments behind the struct
    assert C.sizeof(_lib.GlmDenseData) == 32 and C.sizeof(_lib.GlmDenseLowpData) == 48 and "} skml_glm_dense_lowp_data;" in text
    assert _lib.GlmDenseLowpData.x.offset == 24 and _lib.GlmDenseLowpData.x_kind.offset == 40
    assert all(f"#define SKML_X_{n} {i}\n" in text for n, i in (("F32", 0), ("BF16", 1), ("F16", 2)))
    for _, kind, per16 in KINDS:
        k = {n: _lib.glm_dense_lowp_constant(kind, n) for n in _lib.GLM_DENSE_CONSTANTS}
        assert (k["C"], k["V"]) == (8 * per16, per16 // 4) and k["STRIDE"] >= 64 and min(k.values()) >= 1
        assert _lib.lib.skml_debug_glm_dense_lowp_constant(kind, 6) == -1
    assert _lib.lib.skml_debug_glm_dense_lowp_constant(3, 0) == -1 and _lib.lib.skml_debug_glm_dense_lowp_constant(-1, 0) == -1


def test_slab_and_column_arithmetic_on_the_host_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_dense_lowp_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_dense_lowp_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
