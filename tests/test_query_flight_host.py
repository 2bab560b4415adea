"""The free-flight query, the parts that need no GPU: the Python surface (Device.query_free_flight), the ctypes
signatures against libvr_hip.so, argument checks that must fail before the library is called, and the C++ mirror
(include/vr/query.h, MixtureQuery::query_free_flight) in the driver build."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT


def test_device_has_the_method_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.query_free_flight)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "tau", "unit", "return_albedo", "return_active"]
    assert [sig.parameters[k].default for k in ("unit", "return_albedo", "return_active")] == [False, False, False]


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_free_flight", 7), ("vr_query_free_flight_device", 8)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs


def test_abi_version_is_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        assert "#define VR_ABI_VERSION 11\n" in f.read()


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    t = np.zeros(1, np.float32)
    tau = np.ones(1, np.float32)
    assert L.lib().vr_query_free_flight(None, None, L.fptr(tau), 1, L.fptr(t), None, None) == 1  # VR_ERR_INVALID
    assert b"NULL ctx" in L.lib().vr_last_error()
    assert L.lib().vr_query_free_flight(None, None, None, 0, None, None, None) == 1
    assert L.lib().vr_query_free_flight_device(None, None, None, 1, None, None, None, None) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


GOOD = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("origins,directions,tau", [
    (np.zeros((4, 2), np.float32), GOOD, 1.0),              # wrong trailing shape
    (np.zeros(12, np.float32), GOOD, 1.0),                  # flat
    (GOOD, np.zeros((5, 3), np.float32), 1.0),              # counts differ
    (GOOD.astype(np.float64), GOOD, 1.0),                   # dtype
    (GOOD, GOOD.astype(np.int32), 1.0),
    (GOOD.tolist(), GOOD, 1.0),                             # not an array
    (GOOD, GOOD, np.zeros(3, np.float32)),                  # tau does not broadcast
    (GOOD, GOOD, np.zeros(4, np.float64)),                  # tau dtype
    (GOOD, GOOD, np.zeros((4, 1), np.float32)),             # tau shape
    (GOOD, GOOD, "deep"),
    (GOOD, GOOD, None),
])
def test_argument_errors(origins, directions, tau):
    with pytest.raises(ValueError):
        _no_device().query_free_flight(None, origins, directions, tau)


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().query_free_flight(None, torch.zeros(4, 3), GOOD, 1.0)
    with pytest.raises(ValueError):
        _no_device().query_free_flight(None, GOOD, GOOD, torch.ones(4))


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert '#include "vr/query.h"' in src and "query_free_flight(" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        assert "vr_query_free_flight(" in f.read()
