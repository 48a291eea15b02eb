"""The device-resident data calls (tomo_set_*_device / tomo_get_*_device) are declared, exported and bound, their constants agree
between the header and Python, and the public classes carry the tensor options with defaults that keep today's return types."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

DEVICE_CALLS = ("tomo_set_volume_device", "tomo_get_volume_device", "tomo_set_sinogram_device", "tomo_get_sinogram_device")


def _header():
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_constant(name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, _header())
    assert m, f"{name} is not defined in include/tomo_hip.h"
    return int(m.group(1))


def test_device_calls_are_declared_exported_and_bound():
    from tomo_tv_amd import _lib
    src = _header()
    L = _lib.load()
    _p, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {"tomo_set_volume_device": [_p, _i, _p, _i, _i64, _p], "tomo_get_volume_device": [_p, _i, _p, _i, _i64, _p],
            "tomo_set_sinogram_device": [_p, _i, _p, _i, _i, _i64, _p], "tomo_get_sinogram_device": [_p, _i, _p, _i, _i, _i64, _p]}
    for name in DEVICE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/tomo_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libtomo_hip.so"
        assert _lib.SIGNATURES[name] == want[name]
        assert getattr(L, name).argtypes == want[name] and getattr(L, name).restype is _i


def test_dtype_and_layout_constants_equal_the_headers():
    from tomo_tv_amd import _lib
    assert _lib.F32 == _header_constant("TOMO_F32") and _lib.F64 == _header_constant("TOMO_F64")
    assert _lib.F32 != _lib.F64
    assert _lib.SINO_PACKED == _header_constant("TOMO_SINO_PACKED") and _lib.SINO_PUBLIC == _header_constant("TOMO_SINO_PUBLIC")
    assert _lib.SINO_PACKED != _lib.SINO_PUBLIC


def test_device_calls_refuse_a_null_engine_without_a_gpu():
    from tomo_tv_amd import _lib
    L = _lib.load()
    assert L.tomo_set_volume_device(None, 0, None, _lib.F32, 0, None) != 0 and L.tomo_last_error()
    assert L.tomo_get_volume_device(None, 0, None, _lib.F32, 0, None) != 0
    assert L.tomo_set_sinogram_device(None, 0, None, _lib.F32, _lib.SINO_PACKED, 0, None) != 0
    assert L.tomo_get_sinogram_device(None, 0, None, _lib.F32, _lib.SINO_PUBLIC, 0, None) != 0


def test_tomogpu_tensor_options_keep_todays_return_types_by_default():
    from tomo_tv_amd.reconstructor import TomoGPU
    for f in (TomoGPU.get_recon, TomoGPU.get_projections):
        p = inspect.signature(f).parameters
        assert p["as_tensor"].default is False, f.__name__
        assert p["dtype"].default is None, f.__name__
    assert "torch" in (TomoGPU.__init__.__doc__ or "")


def test_engines_carry_the_tensor_calls():
    from tomo_tv_amd import engine
    for cls in (engine._SlabBackend, engine._GroupBackend, engine.tomoengine, engine.multigpuengine, engine.ctvlib):
        for name in ("set_tilt_series_tensor", "set_volume_tensor", "get_volume_tensor", "get_projections_tensor"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    p = inspect.signature(engine.tomoengine.get_volume_tensor).parameters
    assert p["dtype"].default is None and p["out"].default is None


def test_a_host_tensor_is_refused_in_python_before_any_c_call():
    """The refusal is Python's own: it needs neither a device nor an engine."""
    import pytest
    import torch
    from tomo_tv_amd import engine
    with pytest.raises(ValueError, match="CPU"):
        engine._on_device(torch.zeros(2, 3), 0)
    with pytest.raises(TypeError):
        engine._on_device([[0.0]], 0)


def test_numpy_input_keeps_the_host_path():
    """``TomoGPU`` tells device tensors from host arrays without touching a device: numpy arrays and CPU tensors stay host data."""
    import numpy as np
    import torch
    from tomo_tv_amd.reconstructor import _device_tensor
    assert _device_tensor(np.zeros((2, 3, 4), np.float32)) is None
    assert _device_tensor(torch.zeros(2, 3, 4)) is None
