"""The fused fixed-point optimiser step as far as a machine without a GPU can check it: the C ABI's
two entries are exported and bound, refuse a NULL context before they touch a device, and the Python
optimisers carry the method that calls them."""
import ctypes as C

ENTRIES = ("skml_fixed_decode_sum_step_f32", "skml_fixed_decode_sum_step_f64")


def test_entries_are_exported_and_bound():
    from sketchml_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib, name)
    assert _lib._SIGS[ENTRIES[0]] == _lib._SIGS[ENTRIES[1]] == _lib._SIGS["skml_dense_decode_sum_step_f32"]


def test_entries_refuse_a_null_context():
    from sketchml_amd import _lib
    p = _lib.OptParams()
    _lib.lib.skml_opt_params_default(C.byref(p))
    buf = C.c_void_p(4096)  # never dereferenced: the context is checked first
    for name in ENTRIES:
        assert getattr(_lib.lib, name)(None, buf, 1, 4096, 16, 1.0, C.byref(p), buf, buf, buf) == _lib.SKML_E_ARG
        assert "ctx" in _lib.last_error()


def test_python_surface():
    import sketchml_amd as sk
    from sketchml_amd import distributed, optim
    assert callable(optim.GradientDescent.step_fixed_payloads)
    assert optim.Adam.step_fixed_payloads is optim.GradientDescent.step_fixed_payloads  # inherited
    assert sk.decode_sum_update_fixed_point is distributed.decode_sum_update_fixed_point
