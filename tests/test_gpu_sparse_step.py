"""The optimiser step fused into the sparse Gradient.sum (skml_sparse_decode_sum_step_f32 / _f64),
bit for bit against the oracle's double sum (oracle_sum, CPU) fed into tests/optim_ref.py's step:
never the library's own two-call route.  The cases are those of tests/test_gpu_sparse_sum_batches.py
(whose payload builders, budgets and path assertions this file uses) with w, m, v in place of
`out`; the state is the recognisable non-zero one of tests/test_gpu_optim.py.  A refused call must
leave every state bit as it was: the entry checks the payloads before the one launch that updates."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_optim as T
from test_gpu_optim import _release_shared_cases  # noqa: F401  (this module fills T._state's cache)
from test_gpu_sparse_lowp import SHAPES
from test_gpu_sparse_sum_batches import (DIM_BIG, DIM_W, WAVE_TILES, Case, _budget_for, _dup_payload, _gather_local,
                                         _need, _payload)

pytestmark = pytest.mark.gpu

_CASES = {}
BUILD = {
    "d513": lambda gpu: Case([_payload(gpu, 513, 0.5, 40 + p) for p in range(3)], 513),  # a whole 512-key tile + 1 key
    "d513_sparse": lambda gpu: Case([_payload(gpu, 513, 0.3, 600 + p) for p in range(2)], 513),
    "w8": lambda gpu: Case([_payload(gpu, DIM_W, 0.4, 400 + p, groups=8) for p in range(3)], DIM_W),
    "w12": lambda gpu: Case([_payload(gpu, DIM_W, 0.4, 400 + p, groups=12) for p in range(3)], DIM_W),
    "nine4": lambda gpu: Case([_payload(gpu, 100003, 0.1, 800 + p, groups=4) for p in range(9)], 100003),
    "big": lambda gpu: Case([_payload(gpu, DIM_BIG, 0.005, 500 + p) for p in range(3)], DIM_BIG),
    "dense": lambda gpu: Case(SHAPES["dense_forms"](gpu), 30011),
    "good4": lambda gpu: Case([_payload(gpu, 100003, 0.2, 71 + p, groups=4) for p in range(2)], 100003),
}


def _case(gpu, name):
    if name not in _CASES:
        _CASES[name] = BUILD[name](gpu)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()


def _grid(f):
    for name, vals in (("mean", [False, True]), ("select", [R.ALL, R.LIVE]), ("dt", ["f32", "f64"]), ("kind", [R.SGD, R.ADAM])):
        f = pytest.mark.parametrize(name, vals)(f)
    return f


def _call(gpu, allb, P, stride, dim, scale, p, dt, dev):
    fn = getattr(T._L().lib, "skml_sparse_decode_sum_step_" + dt)
    return fn(gpu.get_context().handle, T._ptr(allb), P, stride, dim, scale, C.byref(p), *(T._ptr(t) for t in dev))


def _check(gpu, case, kind, dt, select, mean, budget=0, path=None, forms={}):
    """One fused step from T._state against optim_ref.step on the oracle's sum; returns the mask."""
    L = T._L()
    scale = 1.0 / case.P if mean else 1.0
    g = case.want(scale)
    p, rp = T._params(kind, select)
    adam = kind == R.ADAM
    state = T._state(case.dim, dt)
    dev = T._dev(state, adam)
    with L.sum_budget(budget), L.forced_forms(**forms):
        st = _call(gpu, case.allb, case.P, case.stride, case.dim, scale, p, dt, dev)
        assert st == 0, L.last_error()
        assert path is None or L.sum_path() == path, (L.sum_path(), path)
    mask = R.selection(g, select)
    want = R.step(rp, g, state[0], state[1] if adam else None, state[2] if adam else None, mask)
    for name, a, b in zip("wmv", T._host(dev), want):
        if b is not None:
            T._same(a, b, f"{name} (dim={case.dim} kind={kind} {dt} select={select} scale={scale} {forms} {path})")
    return mask


# 1. both tile forms, whole and ragged tiles; 2. the final launch continues from the accumulator
@_grid
@pytest.mark.parametrize("name,forms,ends,path", [
    ("d513", {}, None, (1, 1)), ("w8", {}, None, (1, 1)), ("w8", WAVE_TILES, None, (1, 1)), ("w12", {}, None, (1, 1)),
    ("w12", {}, [1, 2, 3], (3, 3)), ("w8", {}, [1, 2, 3], (3, 3)), ("nine4", {}, None, (1, 2))])
def test_forms_tiles_and_continuation(gpu, name, forms, ends, path, kind, dt, select, mean):
    case = _case(gpu, name)
    _check(gpu, case, kind, dt, select, mean, case.budget(ends) if ends else 0, path, forms)


# 3. several tiles per wave: the deferred update of tile t - 1 interleaves with tile t's loads
@pytest.mark.parametrize("forms", [{}, WAVE_TILES])
def test_persistent_walk(gpu, forms):
    case = _case(gpu, "big")
    _check(gpu, case, R.ADAM, "f32", R.ALL, True, case.budget([2, 3]), (2, 2), forms)


# 4. a dense-form payload among sparse ones: its -0.0 -> +0.0 and |v| > 1e-8 rules reach the update
@pytest.mark.parametrize("forms", [{}, WAVE_TILES])
@pytest.mark.parametrize("select", [R.ALL, R.LIVE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_dense_form_payload(gpu, dt, select, forms):
    case = _case(gpu, "dense")
    case.want(1.0)
    assert case.forms == ["dense", "sparse", "dense"]
    mask = _check(gpu, case, R.ADAM, dt, select, False, forms=forms)
    assert select == R.ALL or 0 < mask.sum() < case.dim


# 5. AUTO: the count launch picks ALL for the dense sum and LIVE for the sparse one
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name,dense", [("d513", True), ("d513_sparse", False)])
def test_auto(gpu, name, dense, dt):
    case = _case(gpu, name)
    nnz = int(R.live(case.want(1.0)).sum())
    assert 0 < nnz < case.dim and R.auto_dense(nnz, case.dim) == dense, nnz
    assert _check(gpu, case, R.ADAM, dt, R.AUTO, False).all() == dense


# 6. atomic refusal
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("batches", [1, 3])
@pytest.mark.parametrize("bad,pos", [("dup", 0), ("dup", 2), ("empty", 1)])
def test_a_refused_call_changes_no_state_bit(gpu, bad, pos, batches, dt):
    L = T._L()
    good = _case(gpu, "good4")
    dim = good.dim
    if ("bad", bad) not in _CASES:
        _CASES["bad", bad] = _dup_payload(gpu, dim, 72, groups=4)[0] if bad == "dup" else gpu.encode_sparse(
            torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float64).cuda())
    pl = _CASES["bad", bad]
    pls, needs = list(good.pls), list(good.needs)
    pls.insert(pos, pl)
    needs.insert(pos, _need(pl.nnz(), 256, 4, dim))
    allb, stride = _gather_local(pls)
    p, _ = T._params(R.ADAM)
    dev = T._dev(T._state(dim, dt), True)
    before = [t.clone() for t in dev]
    out = torch.zeros(dim, dtype=torch.float64, device="cuda")
    with L.sum_budget(_budget_for(needs, [1, 2, 3]) if batches == 3 else 0):
        st0 = L.lib.skml_sparse_decode_sum_f64(gpu.get_context().handle, T._ptr(allb), 3, stride, dim, 0.5, T._ptr(out))
        msg0 = L.last_error()
        st = _call(gpu, allb, 3, stride, dim, 0.5, p, dt, dev)
        assert (st, L.last_error()) == (st0, msg0) and st == L.SKML_E_ARG
        assert ("strictly increasing" if bad == "dup" else "restores no keys") in msg0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(dev, before))
    _check(gpu, good, R.ADAM, dt, R.ALL, True)   # the next good call on the context is exact


# 7. argument refusals
@pytest.mark.parametrize("what,word", [("misaligned_w", "aligned"), ("m_for_sgd", "SGD"), ("w_in_blobs", "overlap"),
                                       ("inf_lr", "finite"), ("P0", "P >= 1")])
def test_argument_refusals(gpu, what, word):
    L = T._L()
    case = _case(gpu, "w8")
    p, _ = T._params(R.SGD if what == "m_for_sgd" else R.ADAM)
    if what == "inf_lr":
        p.lr = float("inf")
    w, m, v = T._dev(T._state(case.dim, "f32"), True)
    before = [t.clone() for t in (w, m, v)]
    blobs = case.allb.clone()
    wp = {"misaligned_w": C.c_void_p(w.data_ptr() + 4), "w_in_blobs": C.c_void_p(blobs.data_ptr() + 512)}.get(what, T._ptr(w))
    st = L.lib.skml_sparse_decode_sum_step_f32(gpu.get_context().handle, T._ptr(blobs), 0 if what == "P0" else case.P,
                                               case.stride, case.dim, 1.0, C.byref(p), wp, T._ptr(m), T._ptr(v))
    assert st == L.SKML_E_ARG and word in L.last_error(), L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(blobs, case.allb) and all(torch.equal(a, b) for a, b in zip((w, m, v), before))


# the Python surface: distributed.decode_sum_update_sparse on case 1's shapes
@pytest.mark.parametrize("name", ["d513", "w12"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_decode_sum_update_sparse(gpu, name, dt):
    from sketchml_amd import distributed as D
    from sketchml_amd import optim
    case = _case(gpu, name)
    opt, ref = optim.Adam(case.dim, 0.05, 0.1, 0.5), R.Adam(case.dim, 0.05, 0.1, 0.5)
    w0 = T._state(case.dim, dt)[0]
    w = torch.from_numpy(w0.copy()).cuda()
    D.decode_sum_update_sparse(gpu.get_context().handle, case.allb, case.P, case.stride, case.dim, 1.0 / case.P, opt, w)
    ref.begin_update()
    want = R.step(ref.params(), case.want(1.0 / case.P), w0, np.zeros_like(w0), np.zeros_like(w0))
    for name_, a, b in zip("wmv", (w, opt.m, opt.v), want):
        T._same(a.cpu().numpy(), b, name_)
