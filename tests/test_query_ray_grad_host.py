"""The ray gradient of the optical depth, the parts that need no GPU: the float64 model of tests/ray_grad_reference.py
against central differences of its own closed-form tau, the identity d tau / d origin = -sum_g d tau / d mean_g against
the Gaussian gradient's model, the pose step of tests/test_gpu_query_ray_grad.py on the model, the Python surface
(Device.query_transmittance_ray_grad, autograd.optical_depth), the ctypes signatures against libvr_hip.so, argument
checks that must fail before the library is called, and the C++ mirror (include/vr/query.h,
MixtureQuery::transmittance_ray_gradient) in the driver build.

Measured here: worst |model - central difference| / largest component of the row over the 80 rays, 1.6e-8 .. 1.9e-8
for the four (unit, flag) combinations (bound 1e-5); the identity holds to 2.0e-16; the pose step's ratio is 0.9979."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import grad_reference as R
import ray_grad_reference as RR
from helpers import ROOT

INF = np.inf


# ------------------------------------------------------------------------------------------------
# the float64 side: records from theta, intersect_direct and tau in float64
# ------------------------------------------------------------------------------------------------
def records_of(theta):
    """mean (N, 3), M (N, 3, 3), norm (N,), rho (N,) of theta rows mean[3], cov6[6], density (gaussian.h:50-55)."""
    cov = R.sym(theta[:, 3:9])
    return theta[:, 0:3], np.linalg.inv(cov), (2.0 * np.pi) ** -1.5 * np.linalg.det(cov) ** -0.5, theta[:, 9]


def bounds_of(rec, o, d):
    """intersect_direct in float64: (hit, t0, t1) (n, N), t0 not yet clamped."""
    A, B, C, _, _ = R.quadratic(rec[0], rec[1], o, d)
    disc = B * B - 4.0 * A * (C - 9.0)
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
    t0, t1 = (-B - sq) / (2 * A), (-B + sq) / (2 * A)
    hit = (disc >= 0) & (t1 >= 0)
    return hit, np.where(hit, t0, 0.0), np.where(hit, t1, 0.0)


def walked(v, unit):
    return v if unit else v / np.linalg.norm(v, axis=1, keepdims=True)


def tau_of(rec, o, v, tmax, unit, held=None):
    """(n,) tau of the rays; `held`: the ellipsoids' own (hit, t0, t1) are these, not re-intersected (frozen bounds);
    tmax clips either way, being the caller's bound."""
    d = walked(v, unit)
    hit, t0, t1 = held if held is not None else bounds_of(rec, o, d)
    a, b = np.maximum(t0, 0.0), np.minimum(tmax[:, None], t1)
    return R.tau_terms(*rec, o, d, a, b, hit & (b > a)).sum(1)


def model_rows(rec, o, v, tmax, unit, moving):
    """(rows (n, 7), per-Gaussian |contribution| sums (n, 7), use (n, N)) of the model, float64 bounds."""
    d = walked(v, unit)
    hit, t0, t1 = bounds_of(rec, o, d)
    a, b = np.maximum(t0, 0.0), np.minimum(tmax[:, None], t1)
    use = hit & (b > a)
    a, b = np.where(use, a, 0.0), np.where(use, b, 1.0)
    no = np.zeros_like(use)
    c, _ = RR.ray_contributions(*rec, o, d, a, b, use, use & (t0 > 0) if moving else no,
                                use & (t1 <= tmax[:, None]) if moving else no, use & (t1 > tmax[:, None]))
    c = RR.row_form(c, d, None if unit else np.linalg.norm(v, axis=1))
    return c.sum(1), np.abs(c).sum(1), use


def cloud_case():
    """12 random Gaussians (default_rng(7): mean U(-0.6, 0.6)^3, covariance L L^T + 0.01 I with L's entries
    U(-0.25, 0.25), density U(0.5, 1.5)) and 80 rays: ray k starts on the radius-4 sphere and aims at a point of
    U(-0.5, 0.5)^3 for k % 2 == 0, else starts at a point of U(-0.6, 0.6)^3 inside the cloud with a random direction.
    The stored directions have lengths U(0.5, 2). tmax is infinite for k % 4 < 2, else clips inside the cloud (the
    distance to the target for an outside ray, U(0.3, 1) for an inside one)."""
    rng = np.random.default_rng(7)
    theta = np.zeros((12, 10))
    for g in range(12):
        L = rng.uniform(-0.25, 0.25, (3, 3))
        cov = L @ L.T + 0.01 * np.eye(3)
        theta[g] = np.concatenate([rng.uniform(-0.6, 0.6, 3), cov[np.triu_indices(3)], [rng.uniform(0.5, 1.5)]])
    n = 80
    o, v, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, INF)
    for k in range(n):
        if k % 2 == 0:
            u = rng.normal(size=3)
            o[k] = 4.0 * u / np.linalg.norm(u)
            v[k] = rng.uniform(-0.5, 0.5, 3) - o[k]
            clip = np.linalg.norm(v[k])
        else:
            o[k] = rng.uniform(-0.6, 0.6, 3)
            v[k] = rng.normal(size=3)
            clip = rng.uniform(0.3, 1.0)
        v[k] *= rng.uniform(0.5, 2.0) / np.linalg.norm(v[k])
        if k % 4 >= 2:
            tmax[k] = clip
    return theta, o, v, tmax


@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_model_matches_central_differences(unit, moving):
    """|model row - central difference| <= 1e-5 of the row's largest component, step 1e-6 max(1, |x|), over origin,
    tmax and the stored direction. unit=False differentiates through v / |v|; unit=True takes the three components
    of a unit vector as free (the perturbed vector is walked as it stands). Moving bounds: tau is re-intersected at
    x +- h; frozen bounds: the ellipsoids' entry / exit distances of x are held and only tmax clips anew."""
    theta, o, v, tmax = cloud_case()
    rec = records_of(theta)
    if unit:
        v = walked(v, False)
    G, _, use = model_rows(rec, o, v, tmax, unit, moving)
    held = None if moving else bounds_of(rec, o, walked(v, unit))
    x0 = np.concatenate([o, tmax[:, None], v], 1)
    fd = np.zeros_like(G)
    for i in range(7):
        if i == 3:  # tmax: only the finite ones move
            h = np.where(np.isfinite(tmax), 1e-6 * np.maximum(1.0, np.abs(x0[:, 3])), 0.0)
        else:
            h = 1e-6 * np.maximum(1.0, np.abs(x0[:, i]))
        xp, xm = x0.copy(), x0.copy()
        xp[:, i] += h
        xm[:, i] -= h
        tp = tau_of(rec, xp[:, 0:3], xp[:, 4:7], xp[:, 3], unit, held)
        tm = tau_of(rec, xm[:, 0:3], xm[:, 4:7], xm[:, 3], unit, held)
        with np.errstate(invalid="ignore"):
            fd[:, i] = np.where(h > 0, (tp - tm) / (2 * h), 0.0)
    hits = use.any(1)
    inside = (np.arange(len(o)) % 2 == 1)
    finite = np.isfinite(tmax)
    rel = np.abs(G - fd)[hits].max(1) / np.abs(G)[hits].max(1)
    print(f"unit={unit} moving={moving}: {int(hits.sum())} rays with hits ({int((hits & inside).sum())} from inside, "
          f"{int((hits & finite).sum())} with a finite tmax, {int((G[:, 3] != 0).sum())} with a tmax term), "
          f"worst distance / largest component {rel.max():.3e}")
    assert hits.sum() >= 60 and (hits & inside).sum() >= 25 and (hits & ~inside).sum() >= 25
    assert (hits & finite).sum() >= 25 and (hits & ~finite).sum() >= 25 and (G[:, 3] != 0).sum() >= 20
    assert np.all(G[~finite, 3] == 0) and np.all(G[~hits] == 0)
    assert rel.max() <= 1e-5


def test_origin_gradient_is_minus_the_sum_of_the_mean_gradients():
    """tau depends on o and mean_g through p = o - mean_g only: per ray and Gaussian, d tau / d origin of the ray
    model equals -d tau / d mean of the Gaussian model (grad_reference.contributions), and so do the sums; 1e-12 of
    the largest entry, both flags."""
    theta, o, v, tmax = cloud_case()
    rec = records_of(theta)
    d = walked(v, False)
    hit, t0, t1 = bounds_of(rec, o, d)
    a, b = np.maximum(t0, 0.0), np.minimum(tmax[:, None], t1)
    use = hit & (b > a)
    a, b = np.where(use, a, 0.0), np.where(use, b, 1.0)
    for moving in (True, False):
        mv_in = use & (t0 > 0) & moving
        mv_out = use & (t1 <= tmax[:, None]) & moving
        cr, _ = RR.ray_contributions(*rec, o, d, a, b, use, mv_in, mv_out, use & (t1 > tmax[:, None]))
        cg = R.contributions(*rec, o, d, a, b, use, mv_in, mv_out)
        scale = np.abs(cg[..., 0:3]).max()
        per_hit = np.abs(cr[..., 0:3] + cg[..., 0:3]).max() / scale
        summed = np.abs(cr[..., 0:3].sum(1) + cg[..., 0:3].sum(1)).max() / np.abs(cg[..., 0:3].sum(1)).max()
        print(f"moving={moving}: |d_origin + d_mean| / largest: per hit {per_hit:.3e}, summed over Gaussians {summed:.3e}")
        assert use.sum() > 200 and per_hit <= 1e-12 and summed <= 1e-12


# ------------------------------------------------------------------------------------------------
# the pose step of tests/test_gpu_query_ray_grad.py, on the model: its own first-order ratio
# ------------------------------------------------------------------------------------------------
POSE_OFFSET = 0.05 * np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)


def test_pose_step_of_the_model_is_first_order():
    """The GPU test's pose step in the float64 model with float64 bounds: the 64 rays of grad_reference.descent_case
    through its 8 Gaussians, all translated by a common offset of length 0.05; tau* are the untranslated rays' optical
    depths. One gradient step on the offset, sized for a predicted 1 % drop of sum (tau - tau*)^2, lowers it by
    0.9 .. 1.1 of the prediction. Measured: 0.9979."""
    theta0, _, o, d, frac = R.descent_case()
    rec = records_of(theta0)
    tmax = np.full(len(o), INF)
    target = tau_of(rec, o, d, tmax, True)

    def loss_and_grad(off):
        t = tau_of(rec, o + off, d, tmax, True)
        G, _, _ = model_rows(rec, o + off, d, tmax, True, True)
        return float(np.sum((t - target) ** 2)), (2.0 * (t - target)[:, None] * G[:, 0:3]).sum(0)

    loss0, g = loss_and_grad(POSE_OFFSET)
    eta = frac * loss0 / float(g @ g)
    loss1, _ = loss_and_grad(POSE_OFFSET - eta * g)
    ratio = (loss0 - loss1) / (frac * loss0)
    print(f"pose step (model): loss {loss0:.6e} -> {loss1:.6e}, predicted drop {frac * loss0:.3e}, ratio {ratio:.4f}")
    assert loss0 > 0 and 0.9 <= ratio <= 1.1


# ------------------------------------------------------------------------------------------------
# the surfaces
# ------------------------------------------------------------------------------------------------
def test_device_has_the_method_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.query_transmittance_ray_grad)
    assert list(sig.parameters) == ["self", "scene", "origins", "directions", "tmax", "unit", "moving_bounds"]
    assert [sig.parameters[k].default for k in ("tmax", "unit", "moving_bounds")] == [float("inf"), False, True]
    from vr_amd import autograd
    sig = inspect.signature(autograd.optical_depth)
    assert list(sig.parameters) == ["mean", "cov6", "density", "albedo", "origins", "directions", "tmax", "device",
                                    "moving_bounds"]
    assert "no gradient flows to the rays" not in autograd.__doc__
    assert "query_transmittance_ray_grad" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_transmittance_ray_grad", 5), ("vr_query_transmittance_ray_grad_device", 6)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert L.VR_GRAD_FROZEN_BOUNDS == 1


def test_header_declares_the_query_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    assert "typedef struct vr_ray_grad {" in src and "} vr_ray_grad;" in src
    assert "vr_status vr_query_transmittance_ray_grad(vr_ctx* ctx" in src
    assert "vr_status vr_query_transmittance_ray_grad_device(vr_ctx* ctx" in src
    assert "gradients with respect to the rays are not computed" not in src


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    out = np.zeros(8, np.float32)
    rays = np.zeros(8, np.float32)
    assert L.lib().vr_query_transmittance_ray_grad(None, rays.ctypes.data, 1, 0, out.ctypes.data) == 1  # VR_ERR_INVALID
    assert b"NULL ctx" in L.lib().vr_last_error()
    assert L.lib().vr_query_transmittance_ray_grad(None, None, 0, 0, None) == 1
    assert L.lib().vr_query_transmittance_ray_grad_device(None, None, 1, 0, None, None) == 1
    assert not np.any(out)


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


GOOD = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("origins,directions,tmax", [
    (np.zeros((4, 2), np.float32), GOOD, INF),          # wrong trailing shape
    (np.zeros(12, np.float32), GOOD, INF),              # flat
    (GOOD, np.zeros((5, 3), np.float32), INF),          # counts differ
    (GOOD.astype(np.float64), GOOD, INF),               # dtype
    (GOOD, GOOD.astype(np.float64), INF),
    (GOOD.tolist(), GOOD, INF),                         # not an array
    (GOOD, GOOD, np.zeros(3, np.float32)),              # tmax does not broadcast
    (GOOD, GOOD, np.zeros(4, np.float64)),              # tmax dtype
    (GOOD, GOOD, "far"),
])
def test_argument_errors(origins, directions, tmax):
    with pytest.raises(ValueError):
        _no_device().query_transmittance_ray_grad(None, origins, directions, tmax)


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().query_transmittance_ray_grad(None, torch.zeros(4, 3), GOOD)
    with pytest.raises(ValueError):
        _no_device().query_transmittance_ray_grad(None, GOOD, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        _no_device().query_transmittance_ray_grad(None, GOOD, GOOD, torch.ones(4))


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert '#include "vr/query.h"' in src and "transmittance_ray_gradient(" in src and "--query-ray-grad" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        assert "vr_query_transmittance_ray_grad(" in f.read()
