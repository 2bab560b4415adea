"""The sigma gradient query, the parts that need no GPU: the float64 model of tests/sigma_grad_reference.py against central
differences of its own sigma, the Python surface (Device.query_sigma_grad, autograd.sigma), the ctypes signatures
against libvr_hip.so, the header, argument checks that must fail before the library is called, and the C++ mirror
(include/vr/query.h, MixtureQuery::sigma_gradient) in the driver build.

Measured here: worst |model - central difference| / largest component of the column 7.2e-9 for the Gaussians' eleven columns and 1.4e-10 for the points' three (bound 1e-5)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import sigma_grad_reference as R
from helpers import ROOT


# ------------------------------------------------------------------------------------------------
# the model against central differences (float64 throughout: records and sigma from theta)
# ------------------------------------------------------------------------------------------------
def fd_case():
    """theta (6, 11), points (64, 3), weights (64, 2). default_rng(11): six Gaussians with means U(-0.25, 0.25)^3,
    covariance L L^T + 0.01 I with L's entries U(-0.25, 0.25) (smallest eigenvalue >= 0.01), density U(0.5, 1.5),
    albedo U(0.1, 0.9): they overlap. Points by the recipe of the GPU tests, those within 1e-3 in q of a cut-off
    dropped and the first 64 of the rest kept; weights U(-1, 1)^2."""
    rng = np.random.default_rng(11)
    theta = np.zeros((6, 11))
    for g in range(6):
        L = rng.uniform(-0.25, 0.25, (3, 3))
        cov = L @ L.T + 0.01 * np.eye(3)
        theta[g] = np.concatenate([rng.uniform(-0.25, 0.25, 3), cov[np.triu_indices(3)], [rng.uniform(0.5, 1.5)],
                                   [rng.uniform(0.1, 0.9)]])
    rec = R.records_of(theta)
    x = R.recipe_points(rec, 96).astype(np.float64)
    q = R.quadratic(rec, x)[2]
    x = x[np.all(np.abs(q - 9.0) >= 1e-3, axis=1)][:64]
    assert len(x) == 64
    return theta, x, rng.uniform(-1, 1, (64, 2))


def loss(theta, x, w, active):
    return float((R.sigma(R.records_of(theta), x, active) * w).sum())


def test_model_matches_central_differences():
    """L = sum_i w_i . sigma(x_i). Central differences with step h = 1e-6 max(1, |value|), the active set held (it is
    asserted not to move: every point stays >= 1e-3 - O(h) in q from a cut-off). Bound: 1e-5 of the largest component of
    the column. Truncation is h^2 |L'''| / 6 with |L'''| <= (10 / lambda_min)^2 |L'| = 1e6 |L'| at most (each derivative
    of exp(-q / 2) norm in a covariance entry costs at most a factor (1 + q) / lambda_min, q <= 9, lambda_min >= 0.01),
    i.e. 1.7e-7 |L'|; rounding is 2^-52 |L| n_terms / h < 1e-8 |L|: both far inside the bound."""
    theta, x, w = fd_case()
    rec = R.records_of(theta)
    active = R.quadratic(rec, x)[2] <= 9.0
    assert active.sum(1).max() >= 3 and active.any(0).all()  # overlapping Gaussians, each holding points
    cg, cx = R.contributions(rec, x, w, active)
    G, Gx = cg.sum(0), cx.sum(1)

    def same_set(th, pts):
        return np.array_equal(R.quadratic(R.records_of(th), pts)[2] <= 9.0, active)

    fd = np.zeros_like(G)
    for g in range(theta.shape[0]):
        for k in range(11):
            h = 1e-6 * max(1.0, abs(theta[g, k]))
            tp, tm = theta.copy(), theta.copy()
            tp[g, k] += h
            tm[g, k] -= h
            assert same_set(tp, x) and same_set(tm, x)
            fd[g, k] = (loss(tp, x, w, active) - loss(tm, x, w, active)) / (2 * h)
    fdx = np.zeros_like(Gx)
    for i in range(len(x)):
        for k in range(3):
            h = 1e-6 * max(1.0, abs(x[i, k]))
            xp, xm = x.copy(), x.copy()
            xp[i, k] += h
            xm[i, k] -= h
            assert same_set(theta, xp) and same_set(theta, xm)
            fdx[i, k] = (loss(theta, xp, w, active) - loss(theta, xm, w, active)) / (2 * h)
    worst = 0.0
    for name, a, b in (("gaussians", G, fd), ("points", Gx, fdx)):
        scale = np.abs(a).max(0)
        assert np.all(scale > 0)
        rel = float((np.abs(a - b) / scale).max())
        print(f"{name}: worst |model - central difference| / largest component of the column = {rel:.3e}")
        worst = max(worst, rel)
    assert worst <= 1e-5
    # the (1, 1) weights differentiate sigma_t: no albedo in it
    assert not np.any(R.contributions(rec, x, np.ones((64, 2)), active)[0][..., 10])


def test_sums_and_bound_terms_of_the_model_class():
    """Model.both is `contributions` summed block by block, with S the sums of absolute values."""
    theta, x, w = fd_case()
    rec = R.records_of(theta)
    mdl = R.Model(rec, x.astype(np.float32))
    cg, cx = R.contributions(rec, mdl.x, w)
    (G, S), (Gx, Sx) = mdl.both(w)
    assert np.allclose(G, cg.sum(0), rtol=1e-12, atol=0) and np.allclose(S, np.abs(cg).sum(0), rtol=1e-12, atol=0)
    assert np.array_equal(Gx, cx.sum(1)) and np.array_equal(Sx, np.abs(cx).sum(1))
    assert np.array_equal(mdl.n_active, (R.quadratic(rec, mdl.x)[2] <= 9.0).sum(1))


# ------------------------------------------------------------------------------------------------
# the surfaces
# ------------------------------------------------------------------------------------------------
def test_device_has_the_method_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.query_sigma_grad)
    assert list(sig.parameters) == ["self", "scene", "points", "weights", "gaussians", "positions"]
    assert [sig.parameters[k].default for k in ("weights", "gaussians", "positions")] == [None, True, False]
    from vr_amd import autograd
    for fn in (autograd.sigma, autograd.sigma_resident):
        assert list(inspect.signature(fn).parameters) == ["mean", "cov6", "density", "albedo", "points", "device"]
    assert "no gradient flows to albedo" not in autograd.__doc__ and "albedo.grad" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_sigma_grad", 6), ("vr_query_sigma_grad_device", 7)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs


def test_header_declares_the_query_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    assert "vr_status vr_query_sigma_grad(vr_ctx* ctx, const float* xyz, const float* weight_as, size_t n, float* grad,\n" in src
    assert "vr_status vr_query_sigma_grad_device(vr_ctx* ctx, const float* d_xyz, const float* d_weight_as, size_t n, float* d_grad,\n" in src
    assert src.index("vr_status vr_query_sigma_device(") < src.index("vr_status vr_query_sigma_grad(") < src.index("vr_status vr_query_events_count_device(")


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    g, gx = np.zeros(11, np.float32), np.zeros(3, np.float32)
    x, w = np.zeros(3, np.float32), np.ones(2, np.float32)
    assert L.lib().vr_query_sigma_grad(None, L.fptr(x), L.fptr(w), 1, L.fptr(g), L.fptr(gx)) == 1  # VR_ERR_INVALID
    assert b"NULL ctx" in L.lib().vr_last_error()
    assert L.lib().vr_query_sigma_grad(None, None, None, 0, None, None) == 1
    assert L.lib().vr_query_sigma_grad_device(None, None, None, 1, None, None, None) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


GOOD = np.zeros((4, 3), np.float32)
W4 = np.ones((4, 2), np.float32)


@pytest.mark.parametrize("points,weights,gaussians,positions", [
    (np.zeros((4, 2), np.float32), None, True, False),          # wrong trailing shape
    (np.zeros(12, np.float32), None, True, False),              # flat
    (GOOD.astype(np.float64), None, True, False),               # dtype
    (GOOD.tolist(), None, True, False),                         # not an array
    (GOOD, np.ones((3, 2), np.float32), True, False),           # two weights per point
    (GOOD, np.ones((4, 2), np.float64), True, False),           # weights dtype
    (GOOD, np.ones(4, np.float32), True, False),                # weights shape
    (GOOD, np.ones((4, 1), np.float32), True, True),
    (GOOD, 1.0, True, False),                                   # weights: an array or None
    (GOOD, W4, False, False),                                   # nothing asked for
])
def test_argument_errors(points, weights, gaussians, positions):
    with pytest.raises(ValueError):
        _no_device().query_sigma_grad(None, points, weights, gaussians, positions)


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().query_sigma_grad(None, torch.zeros(4, 3), W4)
    with pytest.raises(ValueError):
        _no_device().query_sigma_grad(None, GOOD, torch.ones(4, 2))


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert "sigma_gradient(" in src and "--query-sigma-grad" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        hdr = f.read()
    assert "std::vector<float> sigma_gradient(" in hdr and "vr_query_sigma_grad(" in hdr
