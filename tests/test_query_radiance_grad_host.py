"""The radiance gradient query, the parts that need no GPU: the Python surface (Device.radiance_gradient,
autograd.radiance_fused[_resident]), the ctypes signatures against libvr_hip.so, the header, argument checks that must fail
before the library is called, and the C++ mirror (include/vr/query.h, MixtureQuery::radiance_gradient) in the driver build.

The Python method takes the C++ mirror's name, Device.radiance_gradient, as Device.features_gradient does:
tests/test_query_host.py holds a table that must name every Device.query_* method."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT


def test_device_has_the_method_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.radiance_gradient)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "t", "features", "weights", "weight_opacity", "q", "tr",
                                    "unit", "moving_bounds", "gaussians", "features_grad", "grad_q", "grad_tau"]
    names = ("weights", "weight_opacity", "q", "tr", "unit", "moving_bounds", "gaussians", "features_grad", "grad_q", "grad_tau")
    assert [sig.parameters[k].default for k in names] == [None, None, None, None, False, True, True, True, False, False]
    assert not [m for m in dir(vr.Device) if m.startswith("query_radiance")]
    from vr_amd import autograd
    for fn in (autograd.radiance_fused, autograd.radiance_fused_resident):
        assert inspect.signature(fn) == inspect.signature(autograd.radiance)
        assert [p.default for p in inspect.signature(fn).parameters.values()][-2:] == [None, 0]
    assert "radiance_fused(mean, cov6, density, albedo, feats" in autograd.__doc__
    assert "radiance and radiance_resident stay exactly as they are" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_radiance_grad", 18), ("vr_query_radiance_grad_device", 19)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    host, dev = L.SIGNATURES["vr_query_radiance_grad"][1], L.SIGNATURES["vr_query_radiance_grad_device"][1]
    assert host[13] is ctypes.c_uint32 and dev[13] is ctypes.c_uint32  # flags, after the three optional inputs
    assert host[:10] == L.SIGNATURES["vr_query_radiance"][1][:10] and dev[:10] == L.SIGNATURES["vr_query_radiance_device"][1][:10]


def test_header_declares_the_query_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    for decl in ("vr_status vr_query_radiance_grad(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride, const float* q,\n",
                 "vr_status vr_query_radiance_grad_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride,\n"):
        assert decl in src, decl
    assert src.index("vr_status vr_query_radiance_device(") < src.index("vr_status vr_query_radiance_grad(") < \
        src.index("vr_status vr_query_radiance_grad_device(") < src.index("vr_status vr_query_events_count_device(")
    assert "without a single atomic add" in src and "as rounded to f32" in src


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    lib = L.lib()
    r, t, f, out = np.zeros(8, np.float32), np.ones(2, np.float32), np.zeros(3, np.float32), np.full(2, 7.0, np.float32)
    assert lib.vr_query_radiance_grad(None, r.ctypes.data, L.fptr(t), 0, None, 0, 1, 2, L.fptr(f), 3, None, None, None, 0, None, None,
                                      L.fptr(out), None) == 1
    assert b"NULL ctx" in lib.vr_last_error() and np.all(out == 7.0)
    assert lib.vr_query_radiance_grad_device(None, None, None, 0, None, 0, 1, 2, None, 3, None, None, None, 0, None, None, None, None,
                                             None) == 1
    assert lib.vr_query_radiance_grad(None, None, None, 0, None, 0, 0, 2, None, 3, None, None, None, 0, None, None, None, None) == 1


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
W2, U = np.ones((4, 2), np.float32), np.ones(4, np.float32)


def _bad_arguments():
    """(class of bad argument, positional arguments after the scene, keyword arguments, message)"""
    F64, TAIL, FIVE = GOOD.astype(np.float64), np.zeros((4, 2), np.float32), np.zeros((5, 3), np.float32)
    A = (GOOD, GOOD, TS, F2)
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
            ("nothing", A, {"gaussians": False, "features_grad": False},
             "radiance_gradient: ask for gaussians, features_grad, grad_q, grad_tau or any of them together"),
            ("q-dtype", A, {"q": TS.astype(np.float64)}, "q must be float32, not float64"),
            ("q-shape", A, {"q": np.ones((4, 2, 1), np.float32)}, "q must have shape (K,) or (n, K), not (4, 2, 1)"),
            ("q-mixed", A, {"q": _Torch(TS)}, "q must be of the same kind as origins"),
            ("q-rows", A, {"q": np.ones((5, 2), np.float32)}, "q has 5 rows for 4 rays"),
            ("q-columns", A, {"q": np.ones((4, 3), np.float32)}, "q has 3 columns for 2 samples"),
            ("q-shared-columns", A, {"q": np.ones(3, np.float32)}, "q has 3 columns for 2 samples"),
            ("tr-shared", A, {"tr": np.ones(2, np.float32)}, "tr must have shape (n, K), not (2,)"),
            ("tr-dtype", A, {"tr": TS.astype(np.float64)}, "tr must be float32, not float64"),
            ("tr-mixed", A, {"tr": _Torch(TS)}, "tr must be of the same kind as origins"),
            ("tr-rows", A, {"tr": np.ones((5, 2), np.float32)}, "tr has 5 rows for 4 rays"),
            ("tr-columns", A, {"tr": np.ones((4, 3), np.float32)}, "tr has 3 columns for 2 samples"),
            ("weights-dtype", A, {"weights": W2.astype(np.float64)}, "weights must be float32, not float64"),
            ("weights-shape", A, {"weights": np.ones(4, np.float32)}, "weights must have shape (4, C), not (4,)"),
            ("weights-mixed", A, {"weights": _Torch(W2)}, "weights must be of the same kind as points"),
            ("weights-rows", A, {"weights": np.ones((5, 2), np.float32)}, "weights has 5 rows for 4 rays"),
            ("weights-columns", A, {"weights": np.ones((4, 3), np.float32)}, "weights has 3 columns for 2 channels"),
            ("opacity-dtype", A, {"weight_opacity": U.astype(np.float64)}, "weight_opacity must be float32, not float64"),
            ("opacity-shape", A, {"weight_opacity": np.ones((4, 1), np.float32)}, "weight_opacity must have shape (n), not (4, 1)"),
            ("opacity-mixed", A, {"weight_opacity": _Torch(U)}, "weight_opacity must be of the same kind as origins"),
            ("opacity-rows", A, {"weight_opacity": np.ones(5, np.float32)}, "weight_opacity has 5 entries for 4 rays")]


@pytest.mark.parametrize("args,kwargs,message", [pytest.param(a, k, msg, id=label) for label, a, k, msg in _bad_arguments()])
def test_bad_argument_raises_its_message_before_the_library(args, kwargs, message):
    import torch
    as_given = lambda x: torch.from_numpy(x.a) if isinstance(x, _Torch) else x  # noqa: E731
    with pytest.raises(ValueError) as err:
        _no_device().radiance_gradient(None, *map(as_given, args), **{n: as_given(v) for n, v in kwargs.items()})
    assert str(err.value) == message


def test_feature_rows_must_match_the_scene():
    import vr_amd as vr
    sc = vr.Scene.from_gaussians(np.zeros((2, 3), np.float32), np.tile(np.float32([1, 0, 0, 1, 0, 1]), (2, 1)),
                                 np.ones(2, np.float32), np.ones(2, np.float32))
    with pytest.raises(ValueError) as err:
        _no_device().radiance_gradient(sc, GOOD, GOOD, TS, F2, grad_q=True)
    assert str(err.value) == "features has 6 rows for 2 Gaussians"


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert ".radiance_gradient(" in src and "--query-radiance-grad" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        hdr = f.read()
    assert "std::vector<float> radiance_gradient(" in hdr and "vr_query_radiance_grad(" in hdr
    with open(os.path.join(ROOT, "tools", "query_bench.py")) as f:
        assert "radiance_grad" in f.read()
