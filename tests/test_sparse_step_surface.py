"""distributed.decode_sum_update_sparse refuses a dim that is not the optimiser's before it touches a
device (the GPU cases are in tests/test_gpu_sparse_step.py)."""
import pytest


def test_decode_sum_update_sparse_refuses_another_dim():
    import sketchml_amd as sk
    from sketchml_amd import distributed as D
    from sketchml_amd import optim
    opt = optim.Adam(1000, 0.05, 0.1, 0.5)
    with pytest.raises(sk.SketchMLException, match="dim=1001"):
        D.decode_sum_update_sparse(None, None, 2, 256, 1001, 0.5, opt, None)
    assert (opt.beta1_t, opt.beta2_t, opt.m) == (0.9, 0.999, None)   # refused before _begin_update
