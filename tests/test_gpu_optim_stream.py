"""Stream ordering of the optimiser entries, one case per entry, in pattern A of
tests/test_gpu_stream_order.py (whose delay, fixtures and run_a this file uses): the context sits on
a non-blocking stream, a calibrated sleep is queued ahead of the copies that bring the fresh
gradient and state in, and clones of w, m, v are queued behind the call.  Work that is not ordered
after the stream updates the stale state from the stale gradient and is overwritten by the fresh
state; work that is not joined into the stream is missed by the clones.  The reference is
tests/optim_ref.py on the fresh data."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_optim as T
from test_gpu_optim import _release_shared_cases  # noqa: F401  (this module fills the same caches)
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu

N = 40005


def _stale_and_fresh(dt, adam):
    """[(device tensor holding the stale state, the fresh state on the device)] and the fresh host arrays."""
    fresh = T._state(N, dt)
    stale = T._state(N, dt, seed=11)
    k = 3 if adam else 1
    return [(torch.from_numpy(s.copy()).cuda(), torch.from_numpy(f.copy()).cuda()) for s, f in zip(stale[:k], fresh[:k])], fresh


def _compare(got, want, adam):
    for name, a, b in zip("wmv", got, want[:3 if adam else 1]):
        T._same(a.cpu().numpy(), b, name)


@pytest.mark.parametrize("dt,kind", [("f32", R.ADAM), ("f64", R.SGD)])
def test_fused_step(gpu, sl, dt, kind):
    L = T._L()
    adam = kind == R.ADAM
    fresh_p, stride, decoded = T._gathered(N, 256, 2)
    stale_p, _, _ = T._gathered(N, 256, 2, 3.0, 1)
    buf = stale_p.clone()
    state, fresh = _stale_and_fresh(dt, adam)
    p, rp = T._params(kind, R.LIVE)
    ts = [t for t, _ in state] + [None] * (3 - len(state))
    fn = "skml_dense_decode_sum_step_f64" if dt == "f64" else "skml_dense_decode_sum_step_f32"

    def call(h):
        sl.c(fn, h, _ptr(buf), 2, stride, N, 0.5, C.byref(p), *(T._ptr(t) for t in ts))

    got = run_a(sl, [(buf, fresh_p)] + state, call, lambda: ts[:len(state)], host_sync=True)  # the header read-back
    g = R.gradient(decoded, 0.5)
    want = R.step(rp, g, fresh[0], fresh[1] if adam else None, fresh[2] if adam else None, R.selection(g, R.LIVE))
    _compare(got, want, adam)


@pytest.mark.parametrize("dt,kind", [("f32", R.ADAM), ("f64", R.SGD)])
def test_array_step(gpu, sl, dt, kind):
    adam = kind == R.ADAM
    rng = np.random.default_rng(3)
    xf, xs = rng.standard_normal(N), 3.0 * rng.standard_normal(N) + 1.0
    gd, gf = torch.from_numpy(xs).cuda(), torch.from_numpy(xf).cuda()
    state, fresh = _stale_and_fresh(dt, adam)
    p, rp = T._params(kind, R.ALL)
    ts = [t for t, _ in state] + [None] * (3 - len(state))
    fn = "skml_opt_step_f64" if dt == "f64" else "skml_opt_step_f32"

    def call(h):
        sl.c(fn, h, _ptr(gd), 1, N, 0.5, C.byref(p), *(T._ptr(t) for t in ts))

    got = run_a(sl, [(gd, gf)] + state, call, lambda: ts[:len(state)])
    want = R.step(rp, xf * np.float64(0.5), fresh[0], fresh[1] if adam else None, fresh[2] if adam else None)
    _compare(got, want, adam)


@pytest.mark.parametrize("dt,kind", [("f32", R.SGD), ("f64", R.ADAM)])
def test_kv_step(gpu, sl, dt, kind):
    adam = kind == R.ADAM
    rng = np.random.default_rng(4)
    nnz = 9000
    fk = np.sort(rng.choice(N, nnz, replace=False)).astype(np.int32)
    sk = np.sort(rng.choice(N, nnz, replace=False)).astype(np.int32)
    fv, sv = rng.standard_normal(nnz), 3.0 * rng.standard_normal(nnz) + 1.0
    kd, vd = torch.from_numpy(sk).cuda(), torch.from_numpy(sv).cuda()
    state, fresh = _stale_and_fresh(dt, adam)
    p, rp = T._params(kind, R.ALL)
    ts = [t for t, _ in state] + [None] * (3 - len(state))
    fn = "skml_opt_step_kv_f64" if dt == "f64" else "skml_opt_step_kv_f32"

    def call(h):
        sl.c(fn, h, _ptr(kd), _ptr(vd), 1, nnz, N, 1.0, C.byref(p), *(T._ptr(t) for t in ts))

    got = run_a(sl, [(kd, torch.from_numpy(fk).cuda()), (vd, torch.from_numpy(fv).cuda())] + state, call,
                lambda: ts[:len(state)])
    want = R.step_kv(rp, fk, fv, fresh[0], fresh[1] if adam else None, fresh[2] if adam else None)
    _compare(got, want, adam)
