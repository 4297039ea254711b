"""Stream ordering of the fused fixed-point optimiser step, in pattern A of
tests/test_gpu_stream_order.py (whose delay, fixtures and run_a this file uses, as
tests/test_gpu_optim_stream.py does): the context sits on a non-blocking stream, a calibrated sleep is
queued ahead of the copies that bring the fresh payloads and state in, and clones of w, m, v are
queued behind the call.  Work that is not ordered after the stream updates the stale state from the
stale payloads and is overwritten by the fresh state; work that is not joined into the stream is
missed by the clones.  The reference runs on the fresh data."""
import ctypes as C

import pytest
import torch

import optim_ref as R
import test_gpu_fixed_optim as FX
import test_gpu_optim as T
from test_gpu_fixed_optim import _release_fixed_cases  # noqa: F401  (this module fills the same caches)
from test_gpu_optim import _release_shared_cases  # noqa: F401
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu

N, BITS, P = 40005, 8, 2


@pytest.mark.parametrize("dt,kind,select", [("f32", R.ADAM, R.LIVE), ("f64", R.SGD, R.ALL)])
def test_fused_fixed_step(gpu, sl, dt, kind, select):
    adam = kind == R.ADAM
    fresh_p, stride, decoded = FX._gathered(N, BITS, P)
    stale_p, _, _ = FX._gathered(N, BITS, P, 1, 3.0)
    buf = stale_p.clone()
    fresh = T._state(N, dt)
    stale = T._state(N, dt, seed=11)
    k = 3 if adam else 1
    state = [(torch.from_numpy(s.copy()).cuda(), torch.from_numpy(f.copy()).cuda()) for s, f in zip(stale[:k], fresh[:k])]
    p, rp = T._params(kind, select)
    ts = [t for t, _ in state] + [None] * (3 - k)
    fn = "skml_fixed_decode_sum_step_f64" if dt == "f64" else "skml_fixed_decode_sum_step_f32"

    def call(h):
        sl.c(fn, h, _ptr(buf), P, stride, N, 0.5, C.byref(p), *(T._ptr(t) for t in ts))

    got = run_a(sl, [(buf, fresh_p)] + state, call, lambda: ts[:k], host_sync=True)  # the header read-back
    g = R.gradient(decoded, 0.5)
    want = R.step(rp, g, fresh[0], fresh[1] if adam else None, fresh[2] if adam else None, R.selection(g, select))
    for name, a, b in zip("wmv", got, want[:k]):
        T._same(a.cpu().numpy(), b, name)
