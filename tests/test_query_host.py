"""Mixture queries, the parts that need no GPU: the Python surface (Device.query_*), the ctypes signatures
against libvr_hip.so, argument checks that must fail before the library is called, and the C++ mirror
(include/vr/query.h) in the driver build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, scene_path


def test_device_has_the_three_query_methods():
    import vr_amd as vr
    for name in ("query_transmittance", "query_sigma", "query_events"):
        assert callable(getattr(vr.Device, name))


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name in ("vr_query_transmittance", "vr_query_transmittance_device", "vr_query_sigma", "vr_query_sigma_device",
                 "vr_query_events_count_device", "vr_query_events_fill_device", "vr_query_events",
                 "vr_query_pack_rays_device"):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1]
    assert ctypes.sizeof(L.vr_ray) == 32 and L.vr_ray.tmax.offset == 12 and L.vr_ray.direction.offset == 16


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    tr = np.zeros(1, np.float32)
    assert L.lib().vr_query_transmittance(None, None, 1, L.fptr(tr), None) == 1  # VR_ERR_INVALID
    assert b"NULL ctx" in L.lib().vr_last_error()
    total = ctypes.c_uint64(5)
    assert L.lib().vr_query_events(None, None, 0, None, None, None, 0, ctypes.byref(total)) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


GOOD = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("origins,directions,tmax", [
    (np.zeros((4, 2), np.float32), GOOD, np.inf),           # wrong trailing shape
    (np.zeros(12, np.float32), GOOD, np.inf),               # flat
    (GOOD, np.zeros((5, 3), np.float32), np.inf),           # counts differ
    (GOOD.astype(np.float64), GOOD, np.inf),                # dtype
    (GOOD, GOOD.astype(np.int32), np.inf),
    (GOOD.tolist(), GOOD, np.inf),                          # not an array
    (GOOD, GOOD, np.zeros(3, np.float32)),                  # tmax does not broadcast
    (GOOD, GOOD, np.zeros(4, np.float64)),                  # tmax dtype
    (GOOD, GOOD, "far"),
])
def test_ray_argument_errors(origins, directions, tmax):
    dev = _no_device()
    with pytest.raises(ValueError):
        dev.query_transmittance(None, origins, directions, tmax=tmax)
    if not isinstance(tmax, (np.ndarray, str)):
        with pytest.raises(ValueError):
            dev.query_events(None, origins, directions)


@pytest.mark.parametrize("points", [np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float64), np.zeros(3, np.float32),
                                    [[0.0, 0.0, 0.0]]])
def test_point_argument_errors(points):
    with pytest.raises(ValueError):
        _no_device().query_sigma(None, points)


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().query_transmittance(None, torch.zeros(4, 3), GOOD)
    with pytest.raises(ValueError):
        _no_device().query_transmittance(None, torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64))


def test_cpp_header_compiles_in_the_driver_build(tmp_path):
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        assert '#include "vr/query.h"' in f.read()
    # the query mode's file errors surface as the driver's runtime_error, before any device is needed
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path("1_gaussian.txt"), "--query",
                        str(tmp_path / "missing.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "missing.bin" in r.stderr
