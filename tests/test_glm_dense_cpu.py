"""Dense instances without a GPU: parseDense on the lines tests/test_glm_cpu.py gives the other parsers,
DenseDataSet's window and refusals, the ABI surface, and skml_glm_dense.hpp's tile arithmetic as a
stand-alone program (tests/glm_dense_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import glm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("line,negY,want", [
    (" 1,0.5, -2e-3 \n", True, (1.0, [0.5, -0.002])),
    ("0,1", True, (-1.0, [1.0])),                       # negY: anything but 1 is -1
    ("0.5,1,2", False, (0.5, [1.0, 2.0])),
    ("1.000000001,4", True, (1.000000001, [4.0])),      # |y - 1| <= 1e-8 keeps y
    ("-1", True, (-1.0, [])),
    ("2,-0.0,inf", True, (-1.0, [-0.0, float("inf")])),
])
def test_parse_dense(line, negY, want):
    from sketchml_amd import data as D
    y, v = D.parseDense(line, 20, negY)
    assert (y, v) == want and [np.signbit(t) for t in v] == [np.signbit(t) for t in want[1]]


def test_dense_dataset_window_and_refusals():
    from sketchml_amd.data import DenseDataSet, parseDense
    from sketchml_amd.exceptions import SketchMLException
    rows = [(1.0, [1.0, 0.0, 2.0]), (-1.0, [0.0, 0.0, 0.0]), (1.0, [3.0, 4.0, 5.0]), (1.0, [-0.0, 6.0, 7.0]), (-1.0, [8.0, 9.0, 1.5])]
    ds, ri = DenseDataSet.fromRows(rows, 3, device="cpu"), 0
    assert ds.size == 5 and ds.dense
    for batch in (2, 3, 4, 5, 1, 4):  # no wrap, ends at size, wraps, a full turn, ...
        want, ri = R.window_rows(5, ri, batch)
        assert DenseDataSet.window_rows(5, ds.take(batch), batch) == want and ds.readIndex == ri
    d, ds.readIndex = ds.glm_data(), 4
    assert ds.loopingRead() == rows[4] and ds.loopingRead() == rows[0] and ds.readIndex == 1
    assert (d.rows, d.dim) == (5, 3) and d.x == ds.x.data_ptr() and ds.x.tolist() == [v for _, r in rows for v in r]
    for bad in (lambda: ds.take(6), lambda: ds.add(rows[0]),                       # the rows are fixed after the first use
                lambda: DenseDataSet(3, device="cpu").add((1.0, [1.0, 2.0])),        # a short row
                lambda: DenseDataSet(3, device="cpu").add((1.0, [1.0] * 4)),         # a long row
                lambda: DenseDataSet(0, device="cpu"),
                lambda: DenseDataSet.fromArray(np.zeros(7), np.zeros(2), 3, device="cpu").glm_data(),
                lambda: DenseDataSet(3, device="cpu").glm_data()):                   # no instance
        with pytest.raises(SketchMLException):
            bad()
    assert DenseDataSet.fromArray(np.arange(6.0).reshape(2, 3), [1.0, -1.0], 3, device="cpu").loopingRead() == (1.0, [0.0, 1.0, 2.0])
    assert DenseDataSet.fromRows([parseDense("1,2,3", 2)], 2, device="cpu").loopingRead() == (1.0, [2.0, 3.0])


def test_abi_surface():
    import sketchml_amd as sk
    from sketchml_amd import _lib
    names = ["skml_glm_%s_dense_%s" % (e, t) for e in ("gradient", "validate") for t in ("f64", "f32")]
    with open(os.path.join(ROOT, "include", "skml.h")) as f:
        text = f.read()
    for n in names:  # exported, declared, and the arguments of the sparse twin behind the data struct
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n) and f"int {n}(" in text
        assert _lib._SIGS[n][1][2:] == _lib._SIGS[n.replace("_dense", "")][1][2:]
    assert C.sizeof(_lib.GlmDenseData) == 32 and C.sizeof(_lib.GlmData) == 80 and "} skml_glm_dense_data;" in text
    assert all(n in sk.__all__ and hasattr(sk, n) for n in ("DenseDataSet", "parseDense"))
    k = {n: _lib.glm_dense_constant(n) for n in _lib.GLM_DENSE_CONSTANTS}
    assert all(f"#define SKML_GLM_DENSE_{n} {i} " in text for n, i in _lib.GLM_DENSE_CONSTANTS.items())
    assert _lib.lib.skml_debug_glm_dense_constant(6) == -1 and min(k.values()) >= 1 and k["STRIDE"] >= 64


def test_tile_arithmetic_on_the_host_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "glm_dense_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "glm_dense_check.cpp")], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
