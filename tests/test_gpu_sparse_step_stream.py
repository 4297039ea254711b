"""Stream ordering of skml_sparse_decode_sum_step_*, in pattern A of tests/test_gpu_stream_order.py as
tests/test_gpu_optim_stream.py applies it: stale blobs and stale state are overwritten by the fresh
ones behind a queued delay, and the result must be the reference's on the fresh data.  The restore,
the side lane, the check, the err read-back and the fused launch all have to follow the context's
stream for that."""
import ctypes as C

import pytest
import torch

import optim_ref as R
import test_gpu_optim as T
from test_gpu_optim import _release_shared_cases  # noqa: F401  (this module fills the same caches)
from test_gpu_optim_stream import _compare, _stale_and_fresh
from test_gpu_optim_stream import N
from test_gpu_sparse_exchange import _gather_local, _payload, oracle_sum
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt,kind", [("f32", R.ADAM), ("f64", R.SGD)])
def test_fused_sparse_step(gpu, sl, dt, kind):
    adam = kind == R.ADAM
    pairs = [_payload(gpu, N, 0.2, 30 + p) for p in range(4)]  # two fresh payloads, two stale ones
    allb, stride = _gather_local([pl for pl, _ in pairs])
    fresh_b, buf = allb[:2 * stride].clone(), allb[2 * stride:].clone()
    state, fresh = _stale_and_fresh(dt, adam)
    p, rp = T._params(kind, R.LIVE)
    ts = [t for t, _ in state] + [None] * (3 - len(state))

    def call(h):
        sl.c("skml_sparse_decode_sum_step_" + dt, h, _ptr(buf), 2, stride, N, 0.5, C.byref(p), *(T._ptr(t) for t in ts))

    got = run_a(sl, [(buf, fresh_b)] + state, call, lambda: ts[:len(state)], host_sync=True)  # the err read-back
    g, _ = oracle_sum([osp for _, osp in pairs[:2]], N, 0.5)
    want = R.step(rp, g, fresh[0], fresh[1] if adam else None, fresh[2] if adam else None, R.selection(g, R.LIVE))
    _compare(got, want, adam)
