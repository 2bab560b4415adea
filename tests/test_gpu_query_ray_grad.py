"""The ray gradient of the optical depth (Device.query_transmittance_ray_grad over
vr_query_transmittance_ray_grad[_device]) against the float64 model of tests/ray_grad_reference.py: hit flags and f32
clip bounds from the oracle's probe, records from the oracle scene, the formulas of include/vr_hip.h in float64.

The bound everywhere: |row_dev - G64| <= 2^-21 S per component, S the sum over Gaussians of the absolute contributions
in the row's own form, and exact zeros where S = 0. It is derived, not measured: the only f32 step is the final
rounding (<= 2^-24 |G| <= 2^-24 S), everything before it is double on both sides from the same f32 inputs and bounds,
which leaves 8x for the device's double erf / exp. Every test prints its measured maximum before it asserts. The tau
column is the transmittance query's tau bit for bit, on every case.

Rays ("sphere" sets, the recipe of tests/test_gpu_query_grad.py): default_rng(7); origins on the radius-4 sphere about
the centre of the records' means, targets uniform in the middle 0.7 of their bounds; the finite tmax of ray i is its
distance to its target, inside the cloud. unit=False runs on those directions scaled by 1.7 (the library normalises
them), unit=True on their f32 normalisation (used as it stands).

Measured on an MI355X, maxima of |row_dev - G64| / S: 1_gaussian 5.6e-8 (moving) / 5.7e-8 (frozen); 250_random and
1000_random over finite x unit x moving 2.3e-8 .. 5.6e-8; 50_random centres 5.7e-8 / 5.8e-8; the batch with six edge
cases 4.7e-8; after half_nodes=0 and after device_bvh=1 5.6e-8 each; device form and C++ mirror 5.6e-8 (the host form's
bits); autograd (w_i times the row, two roundings) 9.9e-8. That is 2^-24 = 6.0e-8, the final rounding. The identity
across the two gradient queries: 0.042 of the two bounds added. The pose step's ratio: 0.992.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import grad_reference as R
import ray_grad_reference as RR
from helpers import ROOT, scene_path

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


def stored(d, unit):
    """What the device gets as directions, and what the Ray constructor normalises to the direction it walks."""
    d_raw = d if unit else (np.float32(1.7) * d).astype(np.float32)
    return (R.normalized_f32(d_raw) if unit else d_raw), d_raw


@functools.lru_cache(maxsize=None)
def sphere_probe(name, unit):
    o, d, _ = sphere_rays(name)
    return R.probe(R.oracle_scene(name), o, stored(d, unit)[1])


@functools.lru_cache(maxsize=None)
def sphere_model(name, finite, unit):
    o, d, tmax = sphere_rays(name)
    return RR.RayModel(R.oracle_scene(name), o, stored(d, unit)[1], tmax if finite else INF, unit, sphere_probe(name, unit))


def forward_tau(dev, scene, o, d, tmax, unit):
    """vr_query_transmittance's tau for the same vr_ray rows."""
    from vr_amd import _lib as L
    if not unit:
        return dev.query_transmittance(scene, o, d, tmax=tmax, return_tau=True)[1]
    dev.upload(scene)
    rays = dev._pack_rays_numpy(o, d, tmax)
    rays[:, 7] = 1.0
    tr, tau = np.empty(len(o), np.float32), np.empty(len(o), np.float32)
    assert L.lib().vr_query_transmittance(dev._h, rays.ctypes.data, len(o), L.fptr(tr), L.fptr(tau)) == 0
    return tau


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def run_and_judge(label, scene_name, o, d_dev, tmax, unit, moving, mdl):
    """The query on numpy inputs: rows within the bound of the model, tau the forward query's bit for bit."""
    dev, sc = device(), vr_scene(scene_name)
    g_o, g_d, g_t, tau = dev.query_transmittance_ray_grad(sc, o, d_dev, tmax=tmax, unit=unit, moving_bounds=moving)
    n = len(o)
    assert g_o.shape == (n, 3) and g_d.shape == (n, 3) and g_t.shape == (n,) and tau.shape == (n,)
    assert all(x.dtype == np.float32 for x in (g_o, g_d, g_t, tau))
    rows = RR.pack_rows(g_o, g_d, g_t)
    RR.judge(label, rows, *mdl.rows(moving))
    assert same_bits(tau, forward_tau(dev, sc, o, d_dev, tmax, unit)), label + ": tau differs from query_transmittance's"
    return rows, tau


# ------------------------------------------------------------------------------------------------
# 1. one Gaussian, a partial wave
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_gaussian_case():
    name, n = "1_gaussian", 257
    rec = R.oracle_scene(name).records()[0].astype(np.float64)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(n, 3))
    o = (rec[:3] + rng.uniform(2, 5, (n, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = ((rec[:3] + rng.uniform(-0.1, 0.1, (n, 3))) - o).astype(np.float32)
    return o, d, RR.RayModel(R.oracle_scene(name), o, d, INF, False)


@pytest.mark.parametrize("moving", [True, False])
def test_one_gaussian_257_rays(moving):
    o, d, mdl = one_gaussian_case()
    assert mdl.use.sum() >= 250
    rows, _ = run_and_judge(f"1_gaussian moving={moving}", "1_gaussian", o, d, INF, False, moving, mdl)
    assert not np.any(rows[:, 3])  # tmax = inf: no tmax term


# ------------------------------------------------------------------------------------------------
# 2. random scenes, infinite and clipping tmax, both flags, both unit modes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("name", ["250_random", "1000_random"])
def test_random_scene(name, finite, unit, moving):
    o, d, tmax = sphere_rays(name)
    mdl = sphere_model(name, finite, unit)
    if finite:  # both branches of g_tmax: Gaussians cut short by tmax, and Gaussians that end before it
        assert mdl.clipped.any() and mdl.moved_out.any()
        assert mdl.use.sum() < sphere_model(name, False, unit).use.sum()
    else:
        assert not mdl.clipped.any()
    rows, _ = run_and_judge(f"{name} finite={finite} unit={unit} moving={moving}", name, o, stored(d, unit)[0],
                            tmax if finite else INF, unit, moving, mdl)
    assert np.any(rows[:, 3] != 0) == finite


# ------------------------------------------------------------------------------------------------
# 3. origins at and near Gaussian centres: the entry is clamped to a = 0 and has no entry term
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
    return o, d, RR.RayModel(R.oracle_scene(name), o, d, INF, False)


@pytest.mark.parametrize("moving", [True, False])
def test_origins_at_gaussian_centres(moving):
    o, d, mdl = centre_case()
    assert (mdl.use & ~mdl.moved_in).any(1).all()  # every ray starts inside a Gaussian
    run_and_judge(f"50_random centres moving={moving}", "50_random", o, d, INF, False, moving, mdl)


# ------------------------------------------------------------------------------------------------
# 4. a batch mixing valid rays with the edge cases
# ------------------------------------------------------------------------------------------------
def test_edge_cases_leave_their_neighbours_alone():
    """64 rays of 250_random: a NaN origin, a zero direction and an infinite direction give eight NaNs; tmax = 0, -1 and
    NaN give eight zeros; every other ray's row has the bits it has in the batch without them (a ray's sums are its
    own lane's, in its own walk's order) and lies within the bound of the model."""
    name = "250_random"
    o, d, tmax = (x[:64] for x in sphere_rays(name))
    o2, d2, tm = o.copy(), d.copy(), tmax.copy()
    o2[3, 1] = np.nan
    d2[11] = 0.0
    d2[40, 0] = np.inf
    tm[17], tm[33], tm[62] = 0.0, -1.0, np.nan
    nan_rows, zero_rows = [3, 11, 40], [17, 33, 62]
    keep = np.setdiff1d(np.arange(64), nan_rows + zero_rows)
    dev, sc = device(), vr_scene(name)
    out = dev.query_transmittance_ray_grad(sc, o2, d2, tmax=tm)
    full = np.concatenate([RR.pack_rows(out[0], out[1], out[2]), out[3][:, None]], 1)
    assert np.all(np.isnan(full[nan_rows])) and full[nan_rows].shape == (3, 8)
    assert not np.any(full[zero_rows]) and not np.any(np.isnan(full[zero_rows]))
    clean = dev.query_transmittance_ray_grad(sc, o, d, tmax=tmax)
    clean = np.concatenate([RR.pack_rows(clean[0], clean[1], clean[2]), clean[3][:, None]], 1)
    assert same_bits(full[keep], clean[keep])
    mdl = RR.RayModel(R.oracle_scene(name), o2, d2, tm, False)
    assert not mdl.valid[nan_rows].any() and mdl.valid[zero_rows].all() and not mdl.walked[zero_rows].any()
    G, S = mdl.rows(True)
    RR.judge("250_random, 64 rays with 6 edge cases", full[keep, :7], G[keep], S[keep])
    tr, tau = dev.query_transmittance(sc, o2, d2, tmax=tm, return_tau=True)
    assert same_bits(full[:, 7], tau)  # NaN and zero rows included


# ------------------------------------------------------------------------------------------------
# 5. tree options: every walk through redo (the pair tree), then the device-built tree
# ------------------------------------------------------------------------------------------------
def test_tree_options_change_nothing_beyond_rounding():
    import vr_amd as vr
    name = "250_random"
    o, d, tmax = sphere_rays(name)
    unit = False
    mdl = sphere_model(name, True, unit)
    G, S = mdl.rows(True)
    dev = vr.Device(0)
    saved = {k: dev.get_option(k) for k in ("half_nodes", "device_bvh")}
    ask = lambda: dev.query_transmittance_ray_grad(vr_scene(name), o, stored(d, unit)[0], tmax=tmax)  # noqa: E731
    try:
        a = ask()
        ref = RR.pack_rows(*a[:3]).astype(np.float64)
        RR.judge("250_random default options", ref, G, S)
        for opt, val in (("half_nodes", 0), ("device_bvh", 1)):
            dev.set_option(opt, val)
            b = ask()
            rows = RR.pack_rows(*b[:3]).astype(np.float64)
            RR.judge(f"250_random after {opt}={val}", rows, G, S)
            assert np.all(np.abs(rows - ref) <= 2 * RR.BOUND * S)
            assert same_bits(b[3], a[3])
    finally:
        for k, v in saved.items():
            dev.set_option(k, v)
    assert {k: dev.get_option(k) for k in saved} == saved


# ------------------------------------------------------------------------------------------------
# 6. host form / device form, the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_device_form_on_a_side_stream_has_the_host_form_bits():
    import torch
    name = "250_random"
    o, d, tmax = sphere_rays(name)
    dev, sc = device(), vr_scene(name)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    for unit, moving in ((False, True), (True, False)):
        dd = stored(d, unit)[0]
        host = dev.query_transmittance_ray_grad(sc, o, dd, tmax=tmax, unit=unit, moving_bounds=moving)
        to_o, to_d, to_t = to(o), to(dd), to(tmax)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = dev.query_transmittance_ray_grad(sc, to_o, to_d, tmax=to_t, unit=unit, moving_bounds=moving)
        side.synchronize()
        assert all(x.is_cuda and x.dtype == torch.float32 for x in got)
        assert [tuple(x.shape) for x in got] == [(256, 3), (256, 3), (256,), (256,)]
        for h, g in zip(host, got):
            assert same_bits(h, g.cpu().numpy())
        RR.judge(f"device form unit={unit} moving={moving}", RR.pack_rows(*[g.cpu().numpy() for g in got[:3]]),
                 *sphere_model(name, True, unit).rows(moving))


def test_cpp_mirror_matches(tmp_path):
    """vol_render --query-ray-grad: Ray's constructor normalises, so the rows are the unit=True ones."""
    name = "250_random"
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d, tmax = sphere_rays(name)
    path = tmp_path / "rays.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 256, 0))
        f.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-ray-grad", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rg ")]
    assert [int(x[1]) for x in lines] == list(range(256)) and all(len(x) == 10 for x in lines)
    g = np.array([[int(h, 16) for h in x[2:]] for x in lines], np.uint32).view(np.float32)
    RR.judge("C++ mirror (--query-ray-grad)", g[:, :7], *sphere_model(name, True, True).rows(True))
    py = device().query_transmittance_ray_grad(vr_scene(name), o, stored(d, True)[0], tmax=tmax, unit=True)
    assert same_bits(g[:, :7], RR.pack_rows(*py[:3])) and same_bits(g[:, 7], py[3])


# ------------------------------------------------------------------------------------------------
# 7. the two gradient queries agree: d tau_i / d origin = -sum_g d tau_i / d mean_g
# ------------------------------------------------------------------------------------------------
def test_origin_row_is_minus_the_summed_mean_gradient():
    """For 8 rays of 250_random: minus the sum over Gaussians of query_transmittance_grad's mean columns for the
    one-hot weight of ray i equals row i's origin, within the two queries' bounds added (the sum of f32 numbers in
    float64 adds nothing)."""
    name = "250_random"
    o, d, tmax = (np.ascontiguousarray(x[:8]) for x in sphere_rays(name))
    dev, sc = device(), vr_scene(name)
    probed = tuple(x[:8] for x in sphere_probe(name, True))  # (d itself: what both queries normalise)
    ray_mdl = RR.RayModel(R.oracle_scene(name), o, d, tmax, False, probed)
    gauss_mdl = R.Model(R.oracle_scene(name), o, d, tmax)
    worst = 0.0
    for moving in (True, False):
        g_o = dev.query_transmittance_ray_grad(sc, o, d, tmax=tmax, moving_bounds=moving)[0].astype(np.float64)
        S_ray = ray_mdl.rows(moving)[1][:, 0:3]
        for i in range(8):
            w = np.zeros(8, np.float32)
            w[i] = 1.0
            gg = dev.query_transmittance_grad(sc, o, d, w, tmax=tmax, moving_bounds=moving).astype(np.float64)
            S_g = gauss_mdl.grad(w, moving)[1][:, 0:3].sum(0)
            err = np.abs(g_o[i] + gg[:, 0:3].sum(0))
            tol = RR.BOUND * S_ray[i] + R.BOUND * S_g
            assert np.all(S_ray[i] > 0)
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), (moving, i, err, tol)
    print(f"identity across the two gradient queries: worst error / (the two bounds added) = {worst:.3e}")


# ------------------------------------------------------------------------------------------------
# 8. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    o, d, _ = sphere_rays("250_random")
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    out = np.full((256, 8), 7.0, np.float32)
    call = lambda r, n, fl, res: L.lib().vr_query_transmittance_ray_grad(fresh._h, r, n, fl, res)  # noqa: E731
    assert call(rows.ctypes.data, 256, 0, out.ctypes.data) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call(rows.ctypes.data, 256, 0, out.ctypes.data) == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene("250_random"))
    assert call(None, 256, 0, out.ctypes.data) == 1  # VR_ERR_INVALID
    assert call(rows.ctypes.data, 256, 0, None) == 1
    assert call(rows.ctypes.data, 256, 2, out.ctypes.data) == 1 and b"flag" in L.lib().vr_last_error()
    assert call(rows.ctypes.data, 1 << 31, 0, out.ctypes.data) == 1
    assert call(None, 0, 0, None) == 0  # n == 0 touches nothing
    assert np.all(out == 7.0)
    buf = torch.zeros(256 * 8 + 4, dtype=torch.float32, device="cuda")
    res = torch.full((256 * 8 + 4,), 7.0, device="cuda")
    dcall = L.lib().vr_query_transmittance_ray_grad_device
    assert dcall(fresh._h, buf.data_ptr() + 4, 256, 0, res.data_ptr(), None) == 1  # rays not 16-byte aligned
    assert dcall(fresh._h, buf.data_ptr(), 256, 0, res.data_ptr() + 4, None) == 1  # rows not 16-byte aligned
    assert dcall(fresh._h, buf.data_ptr(), 256, 4, res.data_ptr(), None) == 1
    assert dcall(fresh._h, buf.data_ptr(), 0, 0, res.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(res == 7.0))
    assert call(rows.ctypes.data, 256, 1, out.ctypes.data) == 0 and not np.any(out == 7.0)


# ------------------------------------------------------------------------------------------------
# 9. torch autograd
# ------------------------------------------------------------------------------------------------
def test_autograd_ray_gradients_are_the_rows():
    import torch
    import vr_amd as vr
    from vr_amd import autograd
    name = "50_random"
    gs = vr_scene(name).gaussians()  # (N, 14): mean, cov6, density, albedo, emission
    o, d, tmax = sphere_rays(name)
    d = stored(d, False)[0]
    w = np.random.default_rng(7).uniform(-1, 1, 256).astype(np.float32)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    mean, cov6, dens = (to(gs[:, 0:3]).requires_grad_(), to(gs[:, 3:9]).requires_grad_(), to(gs[:, 9]).requires_grad_())
    alb = to(gs[:, 10])
    ro, rd, rt = to(o).requires_grad_(), to(d).requires_grad_(), to(tmax).requires_grad_()
    tau = autograd.optical_depth(mean, cov6, dens, alb, ro, rd, tmax=rt)
    assert tau.requires_grad
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    _, tau_q = dev.query_transmittance(sc, o, d, tmax=tmax, return_tau=True)
    assert same_bits(tau.detach().cpu().numpy(), tau_q)
    (tau * to(w)).sum().backward()
    # the rays: w_i times the rows
    g_o, g_d, g_t, _ = dev.query_transmittance_ray_grad(sc, o, d, tmax=tmax)
    assert same_bits(ro.grad.cpu().numpy(), g_o * w[:, None])
    assert same_bits(rd.grad.cpu().numpy(), g_d * w[:, None])
    assert same_bits(rt.grad.cpu().numpy(), g_t * w)
    mdl = RR.RayModel(R.oracle_scene(name), o, d, tmax, False)
    G, S = mdl.rows(True)
    got = RR.pack_rows(ro.grad.cpu().numpy(), rd.grad.cpu().numpy(), rt.grad.cpu().numpy())
    RR.judge("autograd ray gradients", got, G * w[:, None].astype(np.float64), S * np.abs(w[:, None]).astype(np.float64))
    assert np.any(got[:, 3] != 0)
    # the Gaussians: what the gradient query gives for these weights, as without ray gradients
    gm = R.Model(R.oracle_scene(name), o, d, tmax)
    Gg, Sg = gm.grad(w, True)
    got_g = torch.cat([mean.grad, cov6.grad, dens.grad[:, None]], 1).cpu().numpy()
    R.judge("autograd Gaussian gradients beside ray gradients", got_g, Gg, Sg)
    g_q = dev.query_transmittance_grad(sc, o, d, w, tmax=tmax)
    assert np.all(np.abs(got_g.astype(np.float64) - g_q) <= 2 * R.BOUND * Sg)
    # one tmax for all rays: its gradient is the sum
    t1 = torch.tensor([float(np.median(tmax))], device="cuda", requires_grad=True)
    (autograd.optical_depth(mean, cov6, dens, alb, to(o), to(d), tmax=t1) * to(w)).sum().backward()
    g_t1 = dev.query_transmittance_ray_grad(sc, o, d, tmax=float(t1.detach()))[2].astype(np.float64)
    # (256 f32 products summed in f32 in whatever order: at most 256 * 2^-24 of the sum of their absolute values)
    assert t1.grad.shape == (1,) and abs(float(t1.grad) - float((g_t1 * w).sum())) <= 2.0 ** -16 * float(np.abs(g_t1 * w).sum())
    # no ray input requires grad: none gets one
    o3 = to(o)
    m2 = to(gs[:, 0:3]).requires_grad_()
    autograd.optical_depth(m2, cov6.detach(), dens.detach(), alb, o3, to(d), tmax=to(tmax)).sum().backward()
    assert o3.grad is None and m2.grad is not None
    # only a ray input requires grad
    o4 = to(o).requires_grad_()
    autograd.optical_depth(mean.detach(), cov6.detach(), dens.detach(), alb, o4, to(d), tmax=to(tmax)).sum().backward()
    assert same_bits(o4.grad.cpu().numpy(), g_o)


def test_autograd_pose_step():
    """The 64 rays of grad_reference.descent_case through its 8 Gaussians, translated by a common offset of length
    0.05; tau* are the untranslated rays' optical depths. One gradient step on the offset sized for a first-order drop
    of 1 % of sum (tau - tau*)^2 lowers the loss by 0.5 .. 1.5 of that, the interval of the Gaussian descent test (the
    float64 model's own ratio for this case is 0.9979: test_query_ray_grad_host.py)."""
    import torch
    from vr_amd import autograd
    theta0, _, o, d, frac = R.descent_case()
    to = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()  # noqa: E731
    alb = torch.full((8,), 0.5, device="cuda")
    p = [to(theta0[:, 0:3]), to(theta0[:, 3:9]), to(theta0[:, 9])]
    ro, rd = to(o), to(d)
    with torch.no_grad():
        target = autograd.optical_depth(*p, alb, ro, rd).double()
    off = to(0.05 * np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)).requires_grad_()
    loss0 = (autograd.optical_depth(*p, alb, ro + off, rd).double() - target).square().sum()
    loss0.backward()
    loss0 = loss0.detach()
    g = off.grad.double()
    eta = frac * float(loss0) / float(g.square().sum())
    with torch.no_grad():
        off1 = (off.double() - eta * g).float()
        loss1 = (autograd.optical_depth(*p, alb, ro + off1, rd).double() - target).square().sum()
    ratio = (float(loss0) - float(loss1)) / (frac * float(loss0))
    print(f"pose step: loss {float(loss0):.6e} -> {float(loss1):.6e}, predicted drop {frac * float(loss0):.3e}, "
          f"ratio {ratio:.4f} (the float64 model's: 0.9979)")
    assert float(loss0) > 0 and 0.5 <= ratio <= 1.5
