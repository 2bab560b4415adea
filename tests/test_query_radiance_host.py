"""The radiance query, the parts that need no GPU: the Python surface (Device.radiance, autograd.radiance), the ctypes
signatures against libvr_hip.so, the header, argument checks that must fail before the library is called, and the C++
mirror (include/vr/query.h, MixtureQuery::radiance) in the driver build.

The Python method takes the C++ mirror's name, Device.radiance, as Device.evaluate_features does: tests/test_query_host.py
holds a table that must name every Device.query_* method."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT


def test_device_has_the_method_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.radiance)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "t", "features", "weights", "unit", "return_opacity",
                                    "return_tr", "return_pairs"]
    assert [sig.parameters[k].default for k in ("weights", "unit", "return_opacity", "return_tr", "return_pairs")] == \
        [None, False, False, False, False]
    from vr_amd import autograd
    for fn in (autograd.radiance, autograd.radiance_resident):
        assert list(inspect.signature(fn).parameters) == ["mean", "cov6", "density", "albedo", "feats", "origins", "directions", "t", "q",
                                                          "device"]
    assert "radiance(mean, cov6, density, albedo, feats" in autograd.__doc__ and "positive densities" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_radiance", 14), ("vr_query_radiance_device", 15)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs


def test_header_declares_the_query_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    for decl in ("vr_status vr_query_radiance(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride, const float* q,\n",
                 "vr_status vr_query_radiance_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride, const float* d_q,\n"):
        assert decl in src, decl
    assert src.index("vr_status vr_query_features_grad_device(") < src.index("vr_status vr_query_radiance(") < \
        src.index("vr_status vr_query_radiance_device(") < src.index("vr_status vr_query_events_count_device(")
    assert "does not apply that rule" in src  # the one difference from the composition is stated


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    lib = L.lib()
    r, t, f, out = np.zeros(8, np.float32), np.ones(2, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    assert lib.vr_query_radiance(None, r.ctypes.data, L.fptr(t), 0, None, 0, 1, 2, L.fptr(f), 3, L.fptr(out), None, None, None) == 1
    assert b"NULL ctx" in lib.vr_last_error()
    assert lib.vr_query_radiance_device(None, None, None, 0, None, 0, 1, 2, None, 3, None, None, None, None, None) == 1
    assert lib.vr_query_radiance(None, None, None, 0, None, 0, 0, 2, None, 3, None, None, None, None) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


class _Torch:
    """An argument that is handed over as a torch tensor (built when the test runs)."""

    def __init__(self, a):
        self.a = a


GOOD = np.zeros((4, 3), np.float32)
TS, F2 = np.ones((4, 2), np.float32), np.zeros((6, 2), np.float32)


def _bad_arguments():
    """(class of bad argument, positional arguments after the scene, keyword arguments, message)"""
    F64, TAIL, FIVE = GOOD.astype(np.float64), np.zeros((4, 2), np.float32), np.zeros((5, 3), np.float32)
    return [("dtype", (F64, GOOD, TS, F2), {}, "origins must be float32, not float64"),
            ("shape", (TAIL, GOOD, TS, F2), {}, "origins must have shape (n, 3), not (4, 2)"),
            ("mixed", (_Torch(GOOD), GOOD, TS, F2), {}, "origins and directions must both be numpy arrays or both torch tensors"),
            ("rows", (GOOD, FIVE, TS, F2), {}, "4 origins but 5 directions"),
            ("t-dtype", (GOOD, GOOD, TS.astype(np.float64), F2), {}, "t must be float32, not float64"),
            ("t-shape", (GOOD, GOOD, np.ones((4, 2, 1), np.float32), F2), {}, "t must have shape (K,) or (n, K), not (4, 2, 1)"),
            ("t-mixed", (GOOD, GOOD, _Torch(TS), F2), {}, "t must be of the same kind as origins"),
            ("t-rows", (GOOD, GOOD, np.ones((5, 2), np.float32), F2), {}, "t has 5 rows for 4 rays"),
            ("K=0", (GOOD, GOOD, np.ones((4, 0), np.float32), F2), {}, "t has 0 samples per ray: 1 to 1024 are allowed"),
            ("K=max+1", (GOOD, GOOD, np.ones(1025, np.float32), F2), {}, "t has 1025 samples per ray: 1 to 1024 are allowed"),
            ("features-dtype", (GOOD, GOOD, TS, F2.astype(np.float64)), {}, "features must be float32, not float64"),
            ("features-shape", (GOOD, GOOD, TS, np.ones(4, np.float32)), {}, "features must have shape (N, C), not (4,)"),
            ("features-mixed", (GOOD, GOOD, TS, _Torch(F2)), {}, "features must be of the same kind as points"),
            ("C=0", (GOOD, GOOD, TS, np.zeros((6, 0), np.float32)), {}, "features has 0 channels: 1 to 64 are allowed"),
            ("C=max+1", (GOOD, GOOD, TS, np.zeros((6, 65), np.float32)), {}, "features has 65 channels: 1 to 64 are allowed"),
            ("weights-dtype", (GOOD, GOOD, TS, F2), {"weights": TS.astype(np.float64)}, "weights must be float32, not float64"),
            ("weights-shape", (GOOD, GOOD, TS, F2), {"weights": np.ones((4, 2, 1), np.float32)},
             "weights must have shape (K,) or (n, K), not (4, 2, 1)"),
            ("weights-mixed", (GOOD, GOOD, TS, F2), {"weights": _Torch(TS)}, "weights must be of the same kind as origins"),
            ("weights-rows", (GOOD, GOOD, TS, F2), {"weights": np.ones((5, 2), np.float32)}, "weights has 5 rows for 4 rays"),
            ("weights-columns", (GOOD, GOOD, TS, F2), {"weights": np.ones((4, 3), np.float32)}, "weights has 3 columns for 2 samples"),
            ("weights-shared-columns", (GOOD, GOOD, TS, F2), {"weights": np.ones(3, np.float32)}, "weights has 3 columns for 2 samples")]


@pytest.mark.parametrize("args,kwargs,message", [pytest.param(a, k, msg, id=label) for label, a, k, msg in _bad_arguments()])
def test_bad_argument_raises_its_message_before_the_library(args, kwargs, message):
    import torch
    as_given = lambda x: torch.from_numpy(x.a) if isinstance(x, _Torch) else x  # noqa: E731
    with pytest.raises(ValueError) as err:
        _no_device().radiance(None, *map(as_given, args), **{n: as_given(v) for n, v in kwargs.items()})
    assert str(err.value) == message


def test_feature_rows_must_match_the_scene():
    import vr_amd as vr
    sc = vr.Scene.from_gaussians(np.zeros((2, 3), np.float32), np.tile(np.float32([1, 0, 0, 1, 0, 1]), (2, 1)),
                                 np.ones(2, np.float32), np.ones(2, np.float32))
    with pytest.raises(ValueError) as err:
        _no_device().radiance(sc, GOOD, GOOD, TS, F2)
    assert str(err.value) == "features has 6 rows for 2 Gaussians"


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert ".radiance(" in src and "--query-radiance" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        hdr = f.read()
    assert "std::vector<float> radiance(" in hdr and "vr_query_radiance(" in hdr
