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


# ---- every Device.query_* method, every class of bad argument: the ValueError and its message, before the library ----
# The messages were recorded from the package as it stood before the query methods were written once against an
# array-kind object; a Device that owns no context (_no_device) proves that nothing reached the library.
F64, TAIL, FIVE = GOOD.astype(np.float64), np.zeros((4, 2), np.float32), np.zeros((5, 3), np.float32)
ONES, TS = np.ones(4, np.float32), np.ones((4, 2), np.float32)
KMAX = 1024  # VR_PROFILE_MAX_SAMPLES


class _Torch:
    """An argument that is handed over as a torch tensor (built when the test runs)."""

    def __init__(self, a):
        self.a = a


def _bad_arguments():
    """(method, class of bad argument, positional arguments after the scene, keyword arguments, message)"""
    rest = {"query_transmittance_profile": (TS,), "query_transmittance_profile_grad": (TS,), "query_free_flight": (1.0,)}
    out = []
    for m in ("query_transmittance", "query_transmittance_grad", "query_transmittance_ray_grad", "query_transmittance_profile",
              "query_transmittance_profile_grad", "query_events", "query_free_flight"):
        r = rest.get(m, ())
        out += [(m, "dtype", (F64, GOOD) + r, {}, "origins must be float32, not float64"),
                (m, "shape", (TAIL, GOOD) + r, {}, "origins must have shape (n, 3), not (4, 2)"),
                (m, "mixed", (_Torch(GOOD), GOOD) + r, {}, "origins and directions must both be numpy arrays or both torch tensors"),
                (m, "rows", (GOOD, FIVE) + r, {}, "4 origins but 5 directions")]
    for m, kw in (("query_transmittance", "tmax"), ("query_transmittance_grad", "tmax"), ("query_transmittance_ray_grad", "tmax"),
                  ("query_free_flight", "tau")):  # (the targets are checked as a tmax is, and named so)
        out += [(m, kw + "-dtype", (GOOD, GOOD), {kw: ONES.astype(np.float64)}, "tmax must be float32, not float64"),
                (m, kw + "-shape", (GOOD, GOOD), {kw: TS}, "tmax must have shape (n), not (4, 2)"),
                (m, kw + "-mixed", (GOOD, GOOD), {kw: _Torch(ONES)}, "tmax must be a scalar or of the same kind as origins"),
                (m, kw + "-rows", (GOOD, GOOD), {kw: np.ones(3, np.float32)}, "tmax has 3 entries for 4 rays")]
    m = "query_transmittance_grad"
    out += [(m, "weights-dtype", (GOOD, GOOD), {"weights": ONES.astype(np.float64)}, "weights must be float32, not float64"),
            (m, "weights-shape", (GOOD, GOOD), {"weights": TS}, "weights must have shape (n), not (4, 2)"),
            (m, "weights-mixed", (GOOD, GOOD), {"weights": _Torch(ONES)}, "weights must be of the same kind as origins"),
            (m, "weights-rows", (GOOD, GOOD), {"weights": np.ones(5, np.float32)}, "weights has 5 entries for 4 rays")]
    for m in ("query_transmittance_profile", "query_transmittance_profile_grad"):
        out += [(m, "t-dtype", (GOOD, GOOD, TS.astype(np.float64)), {}, "t must be float32, not float64"),
                (m, "t-shape", (GOOD, GOOD, np.ones((4, 2, 1), np.float32)), {}, "t must have shape (K,) or (n, K), not (4, 2, 1)"),
                (m, "t-mixed", (GOOD, GOOD, _Torch(TS)), {}, "t must be of the same kind as origins"),
                (m, "t-rows", (GOOD, GOOD, np.ones((5, 2), np.float32)), {}, "t has 5 rows for 4 rays"),
                (m, "K=0", (GOOD, GOOD, np.ones((4, 0), np.float32)), {}, "t has 0 samples per ray: 1 to 1024 are allowed"),
                (m, "K=max+1", (GOOD, GOOD, np.ones(KMAX + 1, np.float32)), {}, "t has 1025 samples per ray: 1 to 1024 are allowed")]
    m = "query_transmittance_profile_grad"
    out += [(m, "weights-dtype", (GOOD, GOOD, TS), {"weights": TS.astype(np.float64)}, "weights must be float32, not float64"),
            (m, "weights-shape", (GOOD, GOOD, TS), {"weights": ONES}, "weights must have shape (n, K), not (4,)"),
            (m, "weights-mixed", (GOOD, GOOD, TS), {"weights": _Torch(TS)}, "weights must be of the same kind as origins"),
            (m, "weights-rows", (GOOD, GOOD, TS), {"weights": np.ones((5, 2), np.float32)}, "weights has 5 rows for 4 rays"),
            (m, "weights-columns", (GOOD, GOOD, TS), {"weights": np.ones((4, 3), np.float32)}, "weights has 3 columns for 2 samples"),
            (m, "weights-K=max+1", (GOOD, GOOD, np.ones(2, np.float32)), {"weights": np.ones((4, KMAX + 1), np.float32)},
             "weights has 1025 samples per ray: 1 to 1024 are allowed")]
    for m in ("query_sigma", "query_sigma_grad"):
        out += [(m, "dtype", (F64,), {}, "points must be float32, not float64"),
                (m, "shape", (TAIL,), {}, "points must have shape (n, 3), not (4, 2)")]
    m = "query_sigma_grad"
    out += [(m, "weights-dtype", (GOOD,), {"weights": TS.astype(np.float64)}, "weights must be float32, not float64"),
            (m, "weights-shape", (GOOD,), {"weights": GOOD}, "weights must have shape (n, 2), not (4, 3)"),
            (m, "weights-mixed", (GOOD,), {"weights": _Torch(TS)}, "weights must be of the same kind as points"),
            (m, "weights-rows", (GOOD,), {"weights": np.ones((5, 2), np.float32)}, "weights has 5 rows for 4 points"),
            (m, "nothing-asked", (GOOD,), {"gaussians": False, "positions": False},
             "query_sigma_grad: ask for gaussians, positions or both")]
    return out


_BAD = _bad_arguments()


def test_bad_argument_table_covers_every_query_method():
    import vr_amd as vr
    from vr_amd import _lib as L
    assert KMAX == L.VR_PROFILE_MAX_SAMPLES
    assert {m for m, *_ in _BAD} == {name for name in dir(vr.Device) if name.startswith("query_")}


@pytest.mark.parametrize("method,args,kwargs,message", [pytest.param(m, a, k, msg, id=f"{m}-{label}") for m, label, a, k, msg in _BAD])
def test_bad_argument_raises_the_recorded_message_before_the_library(method, args, kwargs, message):
    import torch
    as_given = lambda x: torch.from_numpy(x.a) if isinstance(x, _Torch) else x
    with pytest.raises(ValueError) as err:
        getattr(_no_device(), method)(None, *map(as_given, args), **{n: as_given(v) for n, v in kwargs.items()})
    assert str(err.value) == message
