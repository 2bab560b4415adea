"""The optical-depth gradient query (Device.query_transmittance_grad over vr_query_transmittance_grad[_device]) against
the float64 model of tests/grad_reference.py: hit flags and f32 clip bounds from the oracle's probe, records from the
oracle scene, the formulas of include/vr_hip.h in float64.

The bound everywhere: |G_dev - G64| <= 2^-21 S per component, S the sum of the absolute per-ray contributions, and
exact zeros where S = 0. It is derived, not measured: the only f32 step is the final rounding (<= 2^-24 |G| <= 2^-24 S),
everything before it is double on both sides from the same f32 inputs and bounds, which leaves 8x for the device's
double erf / exp. Every test prints its measured maximum before it asserts. Measured on an MI355X: between 4.3e-9
(1_gaussian) and 5.9e-8 = 2^-24 (every other case, the 600 001-ray batch included) of S, i.e. the final rounding alone;
the descent step's ratio is 1.006.

Rays ("sphere" sets): default_rng(7); origins on the radius-4 sphere about the centre of the records' means, targets
uniform in the middle 0.7 of their bounds; the finite tmax of ray i is its distance to its target, inside the cloud.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import grad_reference as R
from helpers import CAM_POS, FOV, ROOT, main_view_dir, scene_path

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)


def device():
    import vr_amd as vr
    return vr.Device.get(0)


@functools.lru_cache(maxsize=None)
def vr_scene(name):
    import vr_amd as vr
    return vr.Scene.load_GMM(scene_path(name + ".txt"))


@functools.lru_cache(maxsize=None)
def sphere_rays(name, n=256):
    """(origins, directions, finite tmax) f32, read-only."""
    m = R.oracle_scene(name).records()[:, :3].astype(np.float64)
    lo, hi = m.min(0), m.max(0)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(n, 3))
    o = (c + 4.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    tgt = rng.uniform(c - 0.7 * h - 1e-3, c + 0.7 * h + 1e-3, (n, 3)).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    tmax = np.linalg.norm(d.astype(np.float64), axis=1).astype(np.float32)
    for a in (o, d, tmax):
        a.setflags(write=False)
    return o, d, tmax


@functools.lru_cache(maxsize=None)
def sphere_model(name, finite):
    o, d, tmax = sphere_rays(name)
    return R.Model(R.oracle_scene(name), o, d, tmax if finite else INF)


@functools.lru_cache(maxsize=None)
def signed_weights(n):
    w = np.random.default_rng(7).uniform(-1, 1, n).astype(np.float32)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------------------------------------
# 1. one Gaussian: every lane adds to the same ten words; a partial wave
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_gaussian_case():
    name, n = "1_gaussian", 257
    rec = R.oracle_scene(name).records()[0].astype(np.float64)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(n, 3))
    o = (rec[:3] + rng.uniform(2, 5, (n, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = ((rec[:3] + rng.uniform(-0.1, 0.1, (n, 3))) - o).astype(np.float32)
    return o, d, R.Model(R.oracle_scene(name), o, d, INF)


@pytest.mark.parametrize("moving", [True, False])
def test_one_gaussian_257_rays_signed_weights(moving):
    """All 257 lanes add to the same ten words. Measured on an MI355X: 5.3e-9 (moving), 4.3e-9 (frozen) of S."""
    o, d, mdl = one_gaussian_case()
    w = signed_weights(257)
    assert mdl.use.sum() >= 250
    g = device().query_transmittance_grad(vr_scene("1_gaussian"), o, d, w, moving_bounds=moving)
    assert g.shape == (1, 10) and g.dtype == np.float32
    R.judge(f"1_gaussian moving={moving}", g, *mdl.grad(w, moving))


# ------------------------------------------------------------------------------------------------
# 2. random scenes, infinite and clipping tmax, both flags; weights=None is all ones
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("name", ["250_random", "1000_random"])
def test_random_scene(name, finite, moving):
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, finite)
    tm = tmax if finite else INF
    w = signed_weights(256)
    dev, sc = device(), vr_scene(name)
    if finite:  # the clip is inside the cloud: some Gaussians are cut short, some never reached
        assert mdl.use.sum() < sphere_model(name, False).use.sum()
    g = dev.query_transmittance_grad(sc, o, d, w, tmax=tm, moving_bounds=moving)
    assert g.shape == (mdl.N, 10)
    R.judge(f"{name} finite={finite} moving={moving} signed", g, *mdl.grad(w, moving))
    G1, S1 = mdl.grad(None, moving)
    g_none = dev.query_transmittance_grad(sc, o, d, None, tmax=tm, moving_bounds=moving)
    g_ones = dev.query_transmittance_grad(sc, o, d, np.ones(256, np.float32), tmax=tm, moving_bounds=moving)
    R.judge(f"{name} finite={finite} moving={moving} weights=None", g_none, G1, S1)
    R.judge(f"{name} finite={finite} moving={moving} ones", g_ones, G1, S1)
    assert np.all(np.abs(g_none.astype(np.float64) - g_ones) <= 2 * R.BOUND * S1)


# ------------------------------------------------------------------------------------------------
# 3. origins at and near Gaussian centres: the entry is clamped, no entry term
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def centre_case():
    name, n = "50_random", 128
    rec = R.oracle_scene(name).records().astype(np.float64)
    rng = np.random.default_rng(7)
    o = rec[np.arange(n) % len(rec), :3].copy()
    o[64:] += rng.normal(size=(64, 3)) * 0.02
    d = rng.normal(size=(n, 3))
    o, d = o.astype(np.float32), d.astype(np.float32)
    return o, d, R.Model(R.oracle_scene(name), o, d, INF)


@pytest.mark.parametrize("moving", [True, False])
def test_origins_at_gaussian_centres(moving):
    o, d, mdl = centre_case()
    w = signed_weights(128)
    g = device().query_transmittance_grad(vr_scene("50_random"), o, d, w, moving_bounds=moving)
    R.judge(f"50_random centres moving={moving}", g, *mdl.grad(w, moving))


# ------------------------------------------------------------------------------------------------
# 4.-6. zero weights, invalid rays, linearity
# ------------------------------------------------------------------------------------------------
def test_zero_weights_give_zeros():
    o, d, _ = sphere_rays("250_random")
    g = device().query_transmittance_grad(vr_scene("250_random"), o, d, np.zeros(256, np.float32))
    assert g.shape == (250, 10) and not np.any(g)
    import torch
    g = device().query_transmittance_grad(vr_scene("250_random"), torch.from_numpy(o.copy()).cuda(),
                                          torch.from_numpy(d.copy()).cuda(), torch.zeros(256, device="cuda"))
    assert not bool(torch.any(g != 0))


def test_invalid_rays_contribute_nothing():
    """A NaN origin, a zero direction, tmax = 0, < 0 and NaN among the 256 rays: the batch without them, within the
    bound (they are dropped from the model's sums too)."""
    name = "250_random"
    o, d, _ = sphere_rays(name)
    mdl = sphere_model(name, False)
    w = signed_weights(256)
    o2, d2, tm = o.copy(), d.copy(), np.full(256, INF, np.float32)
    o2[3, 1] = np.nan
    o2[70] = np.inf
    d2[11] = 0.0
    d2[130, 2] = np.nan
    tm[17], tm[64], tm[200] = 0.0, -1.0, np.nan
    bad = [3, 70, 11, 130, 17, 64, 200]
    keep = np.setdiff1d(np.arange(256), bad)
    dev, sc = device(), vr_scene(name)
    g = dev.query_transmittance_grad(sc, o2, d2, w, tmax=tm)
    G, S = mdl.grad(w, True, rows=keep)
    R.judge("250_random with 7 invalid rays", g, G, S)
    g_keep = dev.query_transmittance_grad(sc, np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep]),
                                          np.ascontiguousarray(w[keep]))
    assert np.all(np.abs(g.astype(np.float64) - g_keep) <= 2 * R.BOUND * S)


def test_linearity_in_the_weights():
    name = "250_random"
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, True)
    rng = np.random.default_rng(11)
    # multiples of 2^-10 in [-1, 1]: w1 + w2 is exact in f32
    w1, w2 = (rng.integers(-1024, 1025, 256) / 1024.0).astype(np.float32), (rng.integers(-1024, 1025, 256) / 1024.0).astype(np.float32)
    w12 = w1 + w2
    dev, sc = device(), vr_scene(name)
    g1, g2, g12 = (dev.query_transmittance_grad(sc, o, d, w, tmax=tmax).astype(np.float64) for w in (w1, w2, w12))
    S = mdl.grad(w1)[1] + mdl.grad(w2)[1] + mdl.grad(w12)[1]
    # each of the three is within the bound of its own model sum, and the model is exactly linear
    err = np.abs(g1 + g2 - g12)
    with np.errstate(all="ignore"):
        print(f"linearity: max |g(w1) + g(w2) - g(w1 + w2)| / S = {np.nanmax(np.where(S > 0, err / S, 0)):.3e}")
    assert np.all(err <= R.BOUND * S)


# ------------------------------------------------------------------------------------------------
# 7. tree options: the 4-wide walk, the pair-tree redo, host and device builders
# ------------------------------------------------------------------------------------------------
def test_tree_options_change_nothing_beyond_rounding():
    import vr_amd as vr
    name = "1000_random"
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, True)
    w = signed_weights(256)
    G, S = mdl.grad(w, True)
    dev = vr.Device(0)
    out = {}
    for half in (0, 1):
        for dbvh in (0, 1):
            dev.set_option("half_nodes", half)
            dev.set_option("device_bvh", dbvh)
            g = dev.query_transmittance_grad(vr_scene(name), o, d, w, tmax=tmax)
            R.judge(f"1000_random half_nodes={half} device_bvh={dbvh}", g, G, S)
            out[half, dbvh] = g.astype(np.float64)
    ref = out[1, 0]
    for g in out.values():
        assert np.all(np.abs(g - ref) <= 2 * R.BOUND * S)


# ------------------------------------------------------------------------------------------------
# 8. 600 001 rays: queue claims and refills at scale
# ------------------------------------------------------------------------------------------------
def test_600001_rays():
    name = "250_random"
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, True)
    n = 600001
    idx = np.arange(n) % 256
    Ga, Sa = mdl.grad(None, True)
    Gb, Sb = mdl.grad(None, True, rows=np.arange(193))
    assert n == 2343 * 256 + 193
    g = device().query_transmittance_grad(vr_scene(name), o[idx], d[idx], None, tmax=tmax[idx])
    R.judge("250_random x 600001", g, 2343 * Ga + Gb, 2343 * Sa + Sb)


# ------------------------------------------------------------------------------------------------
# 9. host form / device form, numpy / torch, the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree():
    import torch
    name = "250_random"
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, True)
    w = signed_weights(256)
    dev, sc = device(), vr_scene(name)
    for moving in (True, False):
        G, S = mdl.grad(w, moving)
        g_np = dev.query_transmittance_grad(sc, o, d, w, tmax=tmax, moving_bounds=moving)
        to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
        g_t = dev.query_transmittance_grad(sc, to(o), to(d), to(w), tmax=to(tmax), moving_bounds=moving)
        assert g_t.is_cuda and g_t.dtype == torch.float32 and tuple(g_t.shape) == (250, 10)
        R.judge(f"host form moving={moving}", g_np, G, S)
        R.judge(f"device form moving={moving}", g_t.cpu().numpy(), G, S)


def test_cpp_mirror_matches(tmp_path):
    name = "250_random"
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d, tmax = sphere_rays(name)
    path = tmp_path / "rays.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 256, 0))
        f.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-grad", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("tg ")]
    assert [int(x[1]) for x in lines] == list(range(250)) and all(len(x) == 12 for x in lines)
    g = np.array([[int(h, 16) for h in x[2:]] for x in lines], np.uint32).view(np.float32)
    G, S = sphere_model(name, True).grad(None, True)
    R.judge("C++ mirror (--query-grad)", g, G, S)
    g_py = device().query_transmittance_grad(vr_scene(name), o, d, None, tmax=tmax)
    assert np.all(np.abs(g.astype(np.float64) - g_py) <= 2 * R.BOUND * S)


# ------------------------------------------------------------------------------------------------
# 10. a frame's statistics are the frame's
# ------------------------------------------------------------------------------------------------
def test_gradient_query_leaves_the_last_frame_alone():
    import torch
    import vr_amd as vr
    name = "many_gaussians"
    sc = vr_scene(name)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), env_samples=8)
    img = vr.Image(48, 48)
    integ.render(sc, img)
    dev = device()
    before = dev.stats()
    first = img.pixels.copy()
    o = np.tile(CAM_POS, (63, 1)).astype(np.float32)
    d = (np.random.default_rng(7).uniform(-0.5, 0.5, (63, 3)) + [0, 0, -3]).astype(np.float32)
    g = dev.query_transmittance_grad(sc, o, d)
    assert np.any(g != 0)
    dev.query_transmittance_grad(sc, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    dev.synchronize()
    assert dev.stats() == before
    integ.render(sc, img)
    assert np.array_equal(img.pixels.view(np.uint32), first.view(np.uint32))


def test_errors():
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    o, d, _ = sphere_rays("250_random")
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    g = np.full((250, 10), 7.0, np.float32)
    call = lambda r, w, n, fl, out: L.lib().vr_query_transmittance_grad(fresh._h, r, w, n, fl, out)  # noqa: E731
    assert call(rows.ctypes.data, None, 256, 0, L.fptr(g)) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call(rows.ctypes.data, None, 256, 0, L.fptr(g)) == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene("250_random"))
    assert call(None, None, 256, 0, L.fptr(g)) == 1  # VR_ERR_INVALID
    assert call(rows.ctypes.data, None, 256, 0, None) == 1
    assert call(rows.ctypes.data, None, 256, 2, L.fptr(g)) == 1 and b"flag" in L.lib().vr_last_error()
    assert call(rows.ctypes.data, None, 1 << 31, 0, L.fptr(g)) == 1
    assert np.all(g == 7.0)
    assert call(None, None, 0, 0, L.fptr(g)) == 0 and not np.any(g)  # n == 0 zeroes grad
    import torch
    buf = torch.zeros(256 * 8 + 4, dtype=torch.float32, device="cuda")
    out = torch.full((250, 10), 7.0, device="cuda")
    dcall = L.lib().vr_query_transmittance_grad_device
    assert dcall(fresh._h, buf.data_ptr() + 4, None, 256, 0, out.data_ptr(), None) == 1  # not 16-byte aligned
    assert dcall(fresh._h, buf.data_ptr(), None, 0, 0, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out != 0))


# ------------------------------------------------------------------------------------------------
# 11. torch autograd
# ------------------------------------------------------------------------------------------------
def test_autograd_backward_is_the_gradient_query():
    import torch
    import vr_amd as vr
    from vr_amd import autograd
    name = "50_random"
    gs = vr_scene(name).gaussians()  # (N, 14): mean, cov6, density, albedo, emission
    o, d, tmax = sphere_rays(name)
    w = signed_weights(256)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    mean, cov6, dens = (to(gs[:, 0:3]).requires_grad_(), to(gs[:, 3:9]).requires_grad_(), to(gs[:, 9]).requires_grad_())
    alb = to(gs[:, 10])
    tau = autograd.optical_depth(mean, cov6, dens, alb, to(o), to(d), tmax=to(tmax))
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    _, tau_q = dev.query_transmittance(sc, o, d, tmax=tmax, return_tau=True)
    assert np.array_equal(tau.detach().cpu().numpy().view(np.uint32), tau_q.view(np.uint32))
    (tau * to(w)).sum().backward()
    got = torch.cat([mean.grad, cov6.grad, dens.grad[:, None]], 1).cpu().numpy()
    mdl = R.Model(R.oracle_scene(name), o, d, tmax)
    G, S = mdl.grad(w, True)
    R.judge("autograd backward", got, G, S)
    g_q = dev.query_transmittance_grad(sc, o, d, w, tmax=tmax)
    assert np.all(np.abs(got.astype(np.float64) - g_q) <= 2 * R.BOUND * S)
    assert autograd.optical_depth(mean, cov6, dens, alb, to(o), to(d)).requires_grad


def test_autograd_descent_step():
    """One gradient step on sum (tau - tau*)^2 sized for a first-order drop of 1 % lowers the loss by 0.5 .. 1.5 of that
    (the float64 model's own ratio for this case is 0.993 at the full step: test_query_grad_host.py)."""
    import torch
    from vr_amd import autograd
    theta0, star, o, d, frac = R.descent_case()
    to = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()  # noqa: E731
    alb = torch.full((8,), 0.5, device="cuda")
    ro, rd = to(o), to(d)
    with torch.no_grad():
        target = autograd.optical_depth(to(star[:, 0:3]), to(star[:, 3:9]), to(star[:, 9]), alb, ro, rd)
    p = [to(theta0[:, 0:3]).requires_grad_(), to(theta0[:, 3:9]).requires_grad_(), to(theta0[:, 9]).requires_grad_()]
    loss0 = (autograd.optical_depth(*p, alb, ro, rd).double() - target.double()).square().sum()
    loss0.backward()
    loss0 = loss0.detach()
    g2 = sum(float(x.grad.double().square().sum()) for x in p)
    eta = frac * float(loss0) / g2
    with torch.no_grad():
        q = [x - eta * x.grad for x in p]
        loss1 = (autograd.optical_depth(*q, alb, ro, rd).double() - target.double()).square().sum()
    ratio = (float(loss0) - float(loss1)) / (frac * float(loss0))
    print(f"descent: loss {float(loss0):.6e} -> {float(loss1):.6e}, predicted drop {frac * float(loss0):.3e}, ratio {ratio:.4f}")
    assert 0.5 <= ratio <= 1.5
