"""vr_upload_gaussians_device (a Gaussian scene straight from device memory), the parts that need no GPU: the header
and the ctypes signature, the argument checks that must fail before the library is touched, the autograd surface, the
C++ mirror in the driver build, and the rule for the records' `norm` word (tests/upload_device_reference.py) against
the host's on 200 000 seeded covariances per scale band.

Measured here against glibc's powf: 116, 107 and 119 of 200 000 rows differ (0.05 - 0.06 %), by 2 ulp at most."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import upload_device_reference as U
from helpers import ROOT


def test_header_declares_the_entry_point_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    assert "vr_status vr_upload_gaussians_device(vr_ctx* ctx, const float* d_mean, const float* d_cov6" in src
    assert "(float)(K * (double)(float)(1.0 / sqrt((double)det)))" in src  # the norm rule is documented where it is declared


def test_ctypes_signature_resolves():
    from vr_amd import _lib as L
    fn = L.lib().vr_upload_gaussians_device
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES["vr_upload_gaussians_device"][1]
    assert len(fn.argtypes) == 9


def test_null_arguments_are_invalid():
    from vr_amd import _lib as L
    assert L.lib().vr_upload_gaussians_device(None, None, None, None, None, 0, None, 0, None) == L.VR_ERR_INVALID
    assert b"NULL ctx" in L.lib().vr_last_error()


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


def _rows(n=4, dtype=None, kind="torch"):
    import torch
    shapes = ((n, 3), (n, 6), (n,), (n,))
    if kind == "numpy":
        return [np.zeros(s, dtype or np.float32) for s in shapes]
    return [torch.zeros(s, dtype=dtype or torch.float32) for s in shapes]


def _bad_inputs():
    import torch
    yield "cpu tensors", _rows()
    yield "numpy arrays", _rows(kind="numpy")
    yield "float64", _rows(dtype=torch.float64)
    for k, shape in ((0, (4, 2)), (1, (4, 5)), (2, (4, 1)), (3, (2, 2)), (0, (12,))):
        bad = _rows()
        bad[k] = torch.zeros(shape)
        yield f"argument {k} of shape {shape}", bad
    bad = _rows()
    bad[2] = torch.zeros(5)
    yield "counts differ", bad
    bad = _rows()
    bad[1] = torch.zeros(6, 4).t()
    yield "not contiguous", bad
    bad = _rows()
    bad[0] = bad[0].tolist()
    yield "a list", bad


@pytest.mark.parametrize("label,args", list(_bad_inputs()), ids=lambda v: v if isinstance(v, str) else "")
def test_argument_errors(label, args):
    with pytest.raises(ValueError):
        _no_device().upload_gaussians(*args)


def test_each_mistake_is_refused_for_what_it_is():
    """(Without a GPU every tensor here is a CPU one, which alone is refused: dtype, shape, count and contiguity are
    checked first, so their messages show that each check is reached.)"""
    import torch
    import vr_amd as vr
    t = _rows()
    with pytest.raises(ValueError, match="float32"):
        vr.DeviceScene(t[0].double(), *t[1:])
    with pytest.raises(ValueError, match="shape"):
        vr.DeviceScene(t[0], t[1][:, :5], *t[2:])
    with pytest.raises(ValueError, match="5 rows for 4 means"):
        vr.DeviceScene(t[0], t[1], torch.zeros(5), t[3])
    with pytest.raises(ValueError, match="contiguous"):
        vr.DeviceScene(t[0], torch.zeros(6, 4).t(), *t[2:])
    with pytest.raises(ValueError, match="numpy array"):
        vr.DeviceScene(*_rows(kind="numpy"))
    with pytest.raises(ValueError, match="is on cpu"):
        vr.DeviceScene(*t)


def test_python_surface():
    import vr_amd as vr
    from vr_amd import autograd
    sig = inspect.signature(vr.Device.upload_gaussians)
    assert list(sig.parameters) == ["self", "mean", "cov6", "density", "albedo", "lights", "env_color"]
    assert sig.parameters["lights"].default == () and sig.parameters["env_color"].default is None
    for name in ("refresh", "get_num_primitives", "volume_type"):
        assert hasattr(vr.DeviceScene, name), name
    assert "DeviceScene" in vr.__all__
    # the resident form has optical_depth's arguments, and optical_depth keeps the ones its own tests pin
    res = inspect.signature(autograd.optical_depth_resident)
    assert list(res.parameters) == list(inspect.signature(autograd.optical_depth).parameters)
    assert [p.default for p in res.parameters.values()] == [p.default for p in inspect.signature(autograd.optical_depth).parameters.values()]
    assert "upload_gaussians" in autograd.__doc__


def test_resident_parameters_must_be_on_the_rays_device():
    """Refused before a context is asked for: the check compares devices only (the rays stand on torch's meta device
    here, which needs no GPU)."""
    import torch
    from vr_amd import autograd
    rays = torch.zeros(4, 3, device="meta")
    with pytest.raises(ValueError, match="rays' device"):
        autograd.optical_depth_resident(*_rows(), rays, rays)


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert "HipIntegrator::upload_device(" in src and "--upload-device" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "integrator.h")) as f:
        hdr = f.read()
    assert "vr_upload_gaussians_device(" in hdr and "static void upload_device(" in hdr


@pytest.mark.parametrize("band", range(len(U.BANDS)))
def test_norm_rule_against_the_host(band):
    """The numpy restatement of the device's norm against precompute_gaussian's (Scene.records()[:, 10]): never more
    than 2 ulp apart (the bound of upload_device_reference's docstring), and different on fewer than 0.2 % of rows
    (three times the share measured against glibc; evaluating everything in double with one rounding differs on
    25 %, so a wrong formula cannot pass)."""
    import vr_amd as vr
    n = 200_000
    cov = U.band_cov(band, n, 900 + band)
    zeros = np.zeros(n, np.float32)
    host = vr.Scene.from_gaussians(np.zeros((n, 3), np.float32), cov, zeros + 1, zeros).records()[:, 10]
    dev = U.device_norm(cov)
    assert np.isfinite(host).all() and np.isfinite(dev).all() and (host > 0).all()
    apart = U.ulp_apart(dev, host)
    differ = int(np.count_nonzero(apart))
    print(f"band {U.BANDS[band]}: {differ} of {n} rows differ ({100.0 * differ / n:.3f} %), largest {int(apart.max())} ulp")
    assert apart.max() <= 2
    assert differ < 0.002 * n
