"""The transmittance profile query, the parts that need no GPU: the folding rule of its gradient as exact algebra on the
float64 model of tests/grad_reference.py, the Python surfaces (Device.query_transmittance_profile[_grad],
autograd.optical_depth_profile[_resident]), the ctypes signatures against libvr_hip.so, the header, argument checks that
must fail before the library is called, and the C++ mirror (include/vr/query.h) in the driver build."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import grad_reference as R
from helpers import ROOT


# ------------------------------------------------------------------------------------------------
# folding K weighted samples of one (ray, Gaussian) hit is exact algebra
# ------------------------------------------------------------------------------------------------
def folded_contribution(mean, M, norm, rho, o, d, a, t1, ts, ws, moving):
    """The ten numbers of one ray and one Gaussian from the folded moments, as include/vr_hip.h states the rule for
    vr_query_transmittance_profile_grad: float64 throughout, written out independently of R.contributions (staging row
    first, then the conversion to covariance space)."""
    from scipy.special import erf
    p = o - mean
    Md, Mp = M @ d, M @ p
    A, B, C = d @ Md, 2.0 * (p @ Md), p @ Mp
    m = -B / (2.0 * A)
    c = p + m * d
    ua = a - m
    k = np.exp(-0.5 * (C - B * B / (4.0 * A)))
    sA, c0 = np.sqrt(0.5 * A), np.sqrt(np.pi / (2.0 * A))
    erfa, ea = erf(ua * sA), np.exp(-0.5 * A * ua * ua)

    def moments(tb):
        ub = tb - m
        J0 = c0 * (erf(ub * sA) - erfa)
        eb = np.exp(-0.5 * A * ub * ub)
        return np.array([J0, (ea - eb) / A, (ua * ea - ub * eb) / A + J0 / A])

    S, Wf, Wi = np.zeros(3), 0.0, 0.0
    for tk, w in zip(ts, ws):
        if not tk > a:
            continue
        if tk >= t1:
            Wf += w
        else:
            S += w * moments(tk)
            Wi += w
    if Wf != 0.0:
        S += Wf * moments(t1)
    s = rho * norm * k
    gmean = s * (M @ (c * S[0] + d * S[1]))
    GM = -0.5 * s * (S[0] * np.outer(c, c) + S[1] * (np.outer(c, d) + np.outer(d, c)) + S[2] * np.outer(d, d))
    if moving:
        for tb, W in ((t1, Wf), (a, -(Wf + Wi) if a > 0 else 0.0)):
            x = p + tb * d
            wb = W * rho * norm * R.E45 / (2.0 * A * tb + B)
            GM = GM - wb * np.outer(x, x)
            gmean = gmean + 2.0 * wb * (M @ x)
    U = norm * k * S[0]
    GS = -M @ GM @ M - 0.5 * rho * U * M
    return np.array([gmean[0], gmean[1], gmean[2], GS[0, 0], 2 * GS[0, 1], 2 * GS[0, 2], GS[1, 1], 2 * GS[1, 2], GS[2, 2], U])


def fold_case(inside):
    """One Gaussian (default_rng(5)), one ray through it (from outside, or from a point inside its ellipsoid so that the
    entry is clamped), and the chord [a, t1] of the 3-sigma ellipsoid in float64."""
    rng = np.random.default_rng(5)
    L = rng.uniform(-0.3, 0.3, (3, 3))
    cov = L @ L.T + 0.02 * np.eye(3)
    M = np.linalg.inv(cov)
    mean, rho = rng.uniform(-0.2, 0.2, 3), 1.3
    norm = 1.0 / np.sqrt((2 * np.pi) ** 3 * np.linalg.det(cov))
    o = mean + (np.array([0.05, -0.02, 0.03]) if inside else np.array([1.5, 0.4, -2.0]))
    d = (mean + np.array([0.02, 0.01, -0.03])) - o if not inside else np.array([0.3, -0.5, 0.8])
    d = d / np.linalg.norm(d)
    A, B, C, _, _ = R.quadratic(mean[None], M[None], o[None], d[None])
    A, B, C = A[0, 0], B[0, 0], C[0, 0] - 9.0
    disc = B * B - 4 * A * C
    assert disc > 0
    t0, t1 = (-B - np.sqrt(disc)) / (2 * A), (-B + np.sqrt(disc)) / (2 * A)
    assert (t0 < 0) == inside and t1 > 0
    return mean, M, norm, rho, o, d, max(t0, 0.0), t1


@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("inside", [False, True])
@pytest.mark.parametrize("samples", ["in_in_past", "before_in_past", "past_past_in", "all_inside", "all_past"])
def test_folding_is_exact_algebra(samples, inside, moving):
    """K = 3 weighted samples of one ray: sum_k w_k contributions(b_k), b_k = min(t_k, t_exit), from
    grad_reference.contributions against the ten numbers computed once from the folded moments and W_full / W_in. Both
    sides are float64 sums of a handful of terms: 1e-12 relative to the sum of the absolute per-sample contributions."""
    mean, M, norm, rho, o, d, a, t1 = fold_case(inside)
    L = t1 - a
    ts = {"in_in_past": [a + 0.3 * L, a + 0.8 * L, t1 + 1.0], "before_in_past": [0.5 * a - 0.1, a + 0.5 * L, np.inf],
          "past_past_in": [t1, t1 + 0.2, a + 0.1 * L], "all_inside": [a + 0.9 * L, a + 0.2 * L, a + 0.2 * L],
          "all_past": [t1 + 3.0, t1, np.inf]}[samples]
    ws = [0.7, -0.4, 0.9]
    total, scale = np.zeros(10), np.zeros(10)
    for tk, w in zip(ts, ws):
        b = min(tk, t1)
        use = np.array([[b > a]])
        one = R.contributions(mean[None], M[None], np.array([norm]), np.array([rho]), o[None], d[None],
                              np.array([[a]]), np.array([[b if b > a else a + 1.0]]), use,
                              use & (a > 0) & moving, use & (t1 <= tk) & moving)[0, 0]
        total += w * one
        scale += np.abs(w * one)
    fold = folded_contribution(mean, M, norm, rho, o, d, a, t1, ts, ws, moving)
    assert np.all(scale > 0)
    rel = float(np.max(np.abs(fold - total) / scale))
    print(f"{samples} inside={inside} moving={moving}: max |folded - sum| / sum |.| = {rel:.3e}")
    assert rel <= 1e-12


# ------------------------------------------------------------------------------------------------
# the surfaces
# ------------------------------------------------------------------------------------------------
def test_python_surfaces_have_the_documented_arguments():
    import vr_amd as vr
    from vr_amd import autograd
    sig = inspect.signature(vr.Device.query_transmittance_profile)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "t", "return_tau"]
    assert sig.parameters["return_tau"].default is False
    sig = inspect.signature(vr.Device.query_transmittance_profile_grad)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "t", "weights", "moving_bounds"]
    assert [sig.parameters[k].default for k in ("weights", "moving_bounds")] == [None, True]
    for fn in (autograd.optical_depth_profile, autograd.optical_depth_profile_resident):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["mean", "cov6", "density", "albedo", "origins", "directions", "t", "device", "moving_bounds"]
        assert [sig.parameters[k].default for k in ("device", "moving_bounds")] == [0, True]
        assert "origins, directions, t and" in fn.__doc__ and "None" in fn.__doc__
    assert "optical_depth_profile" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_transmittance_profile", 8), ("vr_query_transmittance_profile_device", 9),
                        ("vr_query_transmittance_profile_grad", 9), ("vr_query_transmittance_profile_grad_device", 10)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert L.VR_PROFILE_MAX_SAMPLES == 1024


def test_header_declares_the_queries_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    assert "#define VR_PROFILE_MAX_SAMPLES 1024\n" in src
    names = ["vr_query_transmittance_profile", "vr_query_transmittance_profile_device", "vr_query_transmittance_profile_grad",
             "vr_query_transmittance_profile_grad_device"]
    at = [src.index(f"vr_status {n}(vr_ctx* ctx, const vr_ray* ") for n in names]
    assert at == sorted(at)
    assert src.index("vr_status vr_query_transmittance_ray_grad_device(") < at[0] and at[3] < src.index("vr_status vr_query_sigma(")
    assert "size_t t_stride" in src[at[0]:at[0] + 200] and "uint32_t flags" in src[at[2]:at[2] + 300]


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    lib = L.lib()
    x = np.zeros(8, np.float32)
    assert lib.vr_query_transmittance_profile(None, x.ctypes.data, L.fptr(x), 1, 1, 1, L.fptr(x), None) == 1  # VR_ERR_INVALID
    assert b"NULL ctx" in lib.vr_last_error()
    assert lib.vr_query_transmittance_profile_device(None, None, None, 0, 0, 1, None, None, None) == 1
    assert lib.vr_query_transmittance_profile_grad(None, x.ctypes.data, L.fptr(x), 1, None, 1, 1, 0, L.fptr(x)) == 1
    assert b"NULL ctx" in lib.vr_last_error()
    assert lib.vr_query_transmittance_profile_grad_device(None, None, None, 0, None, 0, 1, 0, None, None) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


O4 = np.zeros((4, 3), np.float32)
T43 = np.ones((4, 3), np.float32)


@pytest.mark.parametrize("origins,t", [
    (np.zeros((4, 2), np.float32), T43),        # rays: wrong trailing shape
    (O4.astype(np.float64), T43),               # rays: dtype
    (O4, T43.astype(np.float64)),               # t: dtype
    (O4, np.ones((3, 3), np.float32)),          # t: a row per ray, or one row
    (O4, np.ones((4, 3, 1), np.float32)),       # t: rank
    (O4, np.float32(1.0)),                      # t: a scalar is no row
    (O4, [1.0, 2.0]),                           # t: not an array
    (O4, np.ones((4, 0), np.float32)),          # K = 0
    (O4, np.ones(0, np.float32)),
    (O4, np.ones(1025, np.float32)),            # K > VR_PROFILE_MAX_SAMPLES
])
def test_argument_errors(origins, t):
    with pytest.raises(ValueError):
        _no_device().query_transmittance_profile(None, origins, O4, t)
    with pytest.raises(ValueError):
        _no_device().query_transmittance_profile_grad(None, origins, O4, t)


@pytest.mark.parametrize("weights", [
    np.ones((4, 2), np.float32),                # one weight per sample
    np.ones((3, 3), np.float32),
    np.ones(3, np.float32),                     # weights are never a shared row
    np.ones((4, 3), np.float64),
    1.0,
])
def test_weight_errors(weights):
    for t in (T43, np.ones(3, np.float32)):
        with pytest.raises(ValueError):
            _no_device().query_transmittance_profile_grad(None, O4, O4, t, weights)


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().query_transmittance_profile(None, O4, O4, torch.ones(4, 3))
    with pytest.raises(ValueError):
        _no_device().query_transmittance_profile(None, torch.zeros(4, 3), torch.zeros(4, 3), T43)
    with pytest.raises(ValueError):
        _no_device().query_transmittance_profile_grad(None, O4, O4, T43, torch.ones(4, 3))


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert "transmittance_profile(" in src and "transmittance_profile_gradient(" in src and "--query-profile" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        hdr = f.read()
    assert "std::vector<float> transmittance_profile(" in hdr and "vr_query_transmittance_profile(" in hdr
    assert "std::vector<float> transmittance_profile_gradient(" in hdr and "vr_query_transmittance_profile_grad(" in hdr
