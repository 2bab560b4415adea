"""The sigma gradient query (Device.query_sigma_grad over vr_query_sigma_grad[_device], autograd.sigma[_resident]) against
the float64 model of tests/sigma_grad_reference.py: records from the oracle scene read as doubles, the formulas of
include/vr_hip.h in float64.

The bound everywhere: |dev - model| <= 2^-21 S per component, S the sum of the absolute per-(point, Gaussian) terms, and
exact zeros where S = 0. It is derived, not measured: the only f32 step is the final rounding (<= 2^-24 S), both sides
are double before that from the same f32 inputs and the same active set, which leaves 8x for the device's double exp.
Every test prints its measured maximum before it asserts. Measured on an MI355X (Gaussians' rows / points' rows):
1_gaussian 5.3e-9 / 5.6e-8, 50_random 3.7e-8 / 5.9e-8, 250_random 5.5e-8 / 5.8e-8 (the same under every tree option),
65 537 points 4.3e-9 / 5.9e-8, autograd 3.7e-8 / 5.9e-8, the C++ mirror 5.8e-8 / 5.7e-8: at or below 2^-24 = 6.0e-8,
the final rounding alone.

Points: the recipe of sigma_grad_reference.recipe_points (default_rng(7); point i in or just outside Gaussian i mod N),
those within 9e-4 in q of a cut-off dropped before the query (at most 1 %, asserted); on the kept points the forward
query's active count equals the model's at every point, which ties the gradient's active set to the forward's.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import grad_reference as GR
import sigma_grad_reference as R
import upload_device_reference as U
from helpers import ROOT, scene_path

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device():
    import vr_amd as vr
    return vr.Device.get(0)


@functools.lru_cache(maxsize=None)
def vr_scene(name):
    import vr_amd as vr
    return vr.Scene.load_GMM(scene_path(name + ".txt"))


@functools.lru_cache(maxsize=None)
def scene_records(name):
    return R.records_of_oracle(GR.oracle_scene(name).records())


@functools.lru_cache(maxsize=None)
def case(name, n_draw, n_keep=None):
    """The shared model of scene `name` at the recipe's kept points; the forward's active counts are checked once."""
    mdl = R.kept_recipe(scene_records(name), n_draw, n_keep)
    _, act = device().query_sigma(vr_scene(name), mdl.x, return_active=True)
    assert np.array_equal(act, mdl.n_active)
    print(f"{name}: {mdl.n} points kept, {mdl.dropped} of {n_draw} dropped, active per point up to {int(mdl.n_active.max())}, "
          f"{int((mdl.n_active == 0).sum())} in no ellipsoid")
    return mdl


@functools.lru_cache(maxsize=None)
def expected(name, n_draw, n_keep=None, signed=True):
    mdl = case(name, n_draw, n_keep)
    return mdl.both(R.signed_weights(mdl.n) if signed else None)


# ------------------------------------------------------------------------------------------------
# 1. one Gaussian: every lane adds to the same eleven words; a partial wave
# ------------------------------------------------------------------------------------------------
def test_one_gaussian_257_points_signed_weights():
    mdl = case("1_gaussian", 264, 257)
    assert mdl.n == 257 and mdl.n_active.sum() >= 200
    w = R.signed_weights(257)
    g, gx = device().query_sigma_grad(vr_scene("1_gaussian"), mdl.x, w, gaussians=True, positions=True)
    assert g.shape == (1, 11) and g.dtype == np.float32 and gx.shape == (257, 3) and gx.dtype == np.float32
    (G, S), (Gx, Sx) = expected("1_gaussian", 264, 257)
    R.judge("1_gaussian grad", g, G, S)
    R.judge("1_gaussian grad_xyz", gx, Gx, Sx)


# ------------------------------------------------------------------------------------------------
# 2. random scenes: signed weights, weights=None, the three forms of the call, numpy and torch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["50_random", "250_random"])
def test_random_scene(name):
    import torch
    mdl = case(name, 1024)
    dev, sc = device(), vr_scene(name)
    N = mdl.N
    assert mdl.active.any(0).all() and mdl.n_active.max() >= 2 and (mdl.n_active == 0).any()
    w = R.signed_weights(mdl.n)
    (G, S), (Gx, Sx) = expected(name, 1024)
    g, gx = dev.query_sigma_grad(sc, mdl.x, w, gaussians=True, positions=True)
    assert g.shape == (N, 11) and gx.shape == (mdl.n, 3)
    R.judge(f"{name} grad", g, G, S)
    R.judge(f"{name} grad_xyz", gx, Gx, Sx)
    # Gaussians only, positions only, both at once; the device form
    g_only = dev.query_sigma_grad(sc, mdl.x, w)
    x_only = dev.query_sigma_grad(sc, mdl.x, w, gaussians=False, positions=True)
    assert g_only.shape == (N, 11) and x_only.shape == (mdl.n, 3)
    assert np.array_equal(bits(x_only), bits(gx))
    assert np.all(np.abs(g_only.astype(np.float64) - g) <= 2 * R.BOUND * S)
    R.judge(f"{name} grad (Gaussians only)", g_only, G, S)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    g_t, gx_t = dev.query_sigma_grad(sc, to(mdl.x), to(w), gaussians=True, positions=True)
    assert g_t.is_cuda and g_t.dtype == torch.float32 and tuple(g_t.shape) == (N, 11) and tuple(gx_t.shape) == (mdl.n, 3)
    assert np.array_equal(bits(gx_t.cpu().numpy()), bits(gx))
    R.judge(f"{name} grad (device form)", g_t.cpu().numpy(), G, S)
    assert np.array_equal(bits(dev.query_sigma_grad(sc, to(mdl.x), to(w), gaussians=False, positions=True).cpu().numpy()), bits(gx))
    # weights=None is (1, 1) everywhere: the gradient of sigma_t, no albedo in it
    (G1, S1), (Gx1, Sx1) = expected(name, 1024, None, False)
    ones = np.ones((mdl.n, 2), np.float32)
    g_none, gx_none = dev.query_sigma_grad(sc, mdl.x, None, gaussians=True, positions=True)
    g_ones, gx_ones = dev.query_sigma_grad(sc, mdl.x, ones, gaussians=True, positions=True)
    R.judge(f"{name} grad (weights=None)", g_none, G1, S1)
    R.judge(f"{name} grad_xyz (weights=None)", gx_none, Gx1, Sx1)
    assert np.all(np.abs(g_none.astype(np.float64) - g_ones) <= 2 * R.BOUND * S1)
    assert np.all(np.abs(gx_none.astype(np.float64) - gx_ones) <= 2 * R.BOUND * Sx1)
    assert not np.any(bits(g_none[:, 10])) and not np.any(S1[:, 10])


# ------------------------------------------------------------------------------------------------
# 3. 65 537 points: 256 blocks and one lane
# ------------------------------------------------------------------------------------------------
def test_65537_points():
    name = "50_random"
    mdl = case(name, 66200, 65537)
    assert mdl.n == 65537 == 256 * 256 + 1
    w = R.signed_weights(mdl.n)
    g, gx = device().query_sigma_grad(vr_scene(name), mdl.x, w, gaussians=True, positions=True)
    (G, S), (Gx, Sx) = expected(name, 66200, 65537)
    R.judge("50_random x 65537 grad", g, G, S)
    R.judge("50_random x 65537 grad_xyz", gx, Gx, Sx)


# ------------------------------------------------------------------------------------------------
# 4. tree options: the 4-wide walk, the child-pair walk, host and device builders
# ------------------------------------------------------------------------------------------------
def test_tree_options_change_nothing_beyond_rounding():
    import vr_amd as vr
    name = "250_random"
    mdl = case(name, 1024)
    w = R.signed_weights(mdl.n)
    (G, S), (Gx, Sx) = expected(name, 1024)
    dev = vr.Device(0)
    out = {}
    for half in (0, 1):
        for dbvh in (0, 1):
            dev.set_option("half_nodes", half)
            dev.set_option("device_bvh", dbvh)
            g, gx = dev.query_sigma_grad(vr_scene(name), mdl.x, w, gaussians=True, positions=True)
            R.judge(f"250_random half_nodes={half} device_bvh={dbvh} grad", g, G, S)
            R.judge(f"250_random half_nodes={half} device_bvh={dbvh} grad_xyz", gx, Gx, Sx)
            out[half, dbvh] = (g.astype(np.float64), gx.astype(np.float64))
    ref = out[1, 0]
    for g, gx in out.values():
        assert np.all(np.abs(g - ref[0]) <= 2 * R.BOUND * S) and np.all(np.abs(gx - ref[1]) <= 2 * R.BOUND * Sx)


# ------------------------------------------------------------------------------------------------
# 5. points that contribute nothing
# ------------------------------------------------------------------------------------------------
def test_points_that_contribute_nothing():
    name = "50_random"
    rec = scene_records(name)
    base = case(name, 1024)
    lonely = int(np.argmin(base.active.sum(0)))  # the Gaussian holding the fewest points: here it holds none
    inside = base.x[~base.active[:, lonely] & (base.n_active > 0)][:40]
    mdl = R.Model(rec, inside)
    assert mdl.n == 40 and not mdl.near.any() and not mdl.active[:, lonely].any()
    far = (rec[0][0] + 100.0).astype(np.float32)
    bad = inside[0].copy()
    bad[1] = np.nan
    pts = np.ascontiguousarray(np.concatenate([inside[:20], far[None], bad[None], inside[20:]]))
    w = R.signed_weights(len(pts))
    keep = np.r_[0:20, 22:len(pts)]
    g, gx = device().query_sigma_grad(vr_scene(name), pts, w, gaussians=True, positions=True)
    (G, S), (Gx, Sx) = mdl.both(w[keep])
    R.judge("with a far and a NaN point: grad", g, G, S)
    R.judge("with a far and a NaN point: grad_xyz", gx[keep], Gx, Sx)
    assert not np.any(bits(gx[20:22]))  # +0 rows
    empty = ~(S > 0).any(1)
    assert empty.any() and not np.any(bits(g[empty]))  # eleven zero bit patterns
    assert not np.any(bits(device().query_sigma_grad(vr_scene(name), pts[20:22], None)))
    assert device().query_sigma_grad(vr_scene(name), pts[:0]).shape == (50, 11)
    assert device().query_sigma_grad(vr_scene(name), pts[:0], gaussians=False, positions=True).shape == (0, 3)


def test_points_of_non_positive_mass_are_taken_back():
    """A Gaussian of negative density inside a positive one: near the centre the summed m is < 0, the forward gives
    (0, 0), and the gradient takes such a point's adds back (rows: to the rounding of a double sum; its own row: +0)."""
    import vr_amd as vr
    F = np.float32
    mean = np.zeros((2, 3), F)
    cov6 = np.array([[0.04, 0, 0, 0.04, 0, 0.04], [0.01, 0, 0, 0.01, 0, 0.01]], F)
    density, albedo = np.array([1.0, -0.5], F), np.array([0.3, 0.8], F)
    rec = R.records_of_oracle(GR.oracle_from_gaussians(mean, cov6, density, albedo).records())
    x = R.recipe_points(rec, 300)
    m, q = R.mass(rec, x)
    ok = ~np.any(np.abs(q - 9.0) <= R.Q_MARGIN, axis=1) & (np.abs(m.sum(1)) >= 1e-3 * np.abs(m).sum(1))
    x = np.ascontiguousarray(x[ok][:257])
    assert len(x) == 257
    mdl = R.Model(rec, x)
    dead = (R.mass(rec, x)[0].sum(1) <= 0) & (mdl.n_active > 0)
    live = (R.mass(rec, x)[0].sum(1) > 0) & (mdl.n_active == 2)
    assert dead.sum() >= 30 and live.sum() >= 30
    sc = vr.Scene.from_gaussians(mean, cov6, density, albedo)
    sig, act = device().query_sigma(sc, x, return_active=True)
    assert np.array_equal(act, mdl.n_active) and not np.any(bits(sig[dead])) and np.all(sig[live].sum(1) > 0)
    w = R.signed_weights(257)
    g, gx = device().query_sigma_grad(sc, x, w, gaussians=True, positions=True)
    (G, S), (Gx, Sx) = mdl.both(w)
    assert not np.any(Sx[dead]) and not np.any(bits(gx[dead]))
    R.judge("negative density: grad", g, G, S)
    R.judge("negative density: grad_xyz", gx, Gx, Sx)
    assert np.array_equal(bits(device().query_sigma_grad(sc, x, w, gaussians=False, positions=True)), bits(gx))


def test_walks_at_the_stack_limit_are_taken_back(device_options):
    """The mirrored comb of tests/wide_walk_reference.py under the device builder's 4-wide tree: every point's containment
    walk reaches sp + 4 > kStackSize (simulated on the tree read back, as tests/test_gpu_wide_stack.py does for the
    forward), so whatever the broken-off walk added is taken back and the child-pair walk adds the whole active set.
    The plain comb, whose walks stay under the limit, must give the same to the rounding of a double sum."""
    import tree_reference as T
    import vr_amd as vr
    import wide_walk_reference as W
    leaf_max = T.limits()["leaf_max"]
    device_options("device_bvh", 1)
    device_options("half_nodes", 1)
    dev = vr.Device.get(0)
    p = (W.CENTRE + np.random.default_rng(74).uniform(-0.4, 0.4, (256, 3)) * W.EXTENT).astype(np.float32)
    w = R.signed_weights(256)
    for mirrored in (True, False):
        sc = W.comb_scene(leaf_max, mirrored)
        dev.upload(sc, force=True)
        sim = W.walk_sigma(dev.debug_tree(), p, 32)
        assert sum(r["fire"] is not None for r in sim) == (256 if mirrored else 0)
        mdl = R.Model(R.records_of_oracle(W.comb_oracle(leaf_max, mirrored).records()), p)
        assert not mdl.near.any() and np.all(mdl.n_active == W.comb_count(leaf_max))
        g, gx = dev.query_sigma_grad(sc, p, w, gaussians=True, positions=True)
        (G, S), (Gx, Sx) = mdl.both(w)
        assert not (S[W.comb_count(leaf_max):] > 0).any()  # the ballast holds no point: exact zeros
        R.judge(f"comb mirrored={mirrored} grad", g, G, S)
        R.judge(f"comb mirrored={mirrored} grad_xyz", gx, Gx, Sx)


# ------------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    x = np.ascontiguousarray(case("250_random", 1024).x[:256])
    g = np.full((250, 11), 7.0, np.float32)
    gx = np.full((256, 3), 7.0, np.float32)
    call = lambda p, w, n, a, b: L.lib().vr_query_sigma_grad(fresh._h, p, w, n, a, b)  # noqa: E731
    assert call(L.fptr(x), None, 256, L.fptr(g), L.fptr(gx)) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call(L.fptr(x), None, 256, L.fptr(g), L.fptr(gx)) == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene("250_random"))
    assert call(L.fptr(x), None, 256, None, None) == 1 and b"both outputs" in L.lib().vr_last_error()  # VR_ERR_INVALID
    assert call(None, None, 256, L.fptr(g), L.fptr(gx)) == 1
    assert call(L.fptr(x), None, 1 << 31, L.fptr(g), L.fptr(gx)) == 1
    assert np.all(g == 7.0) and np.all(gx == 7.0)
    assert call(None, None, 0, L.fptr(g), L.fptr(gx)) == 0 and not np.any(bits(g)) and np.all(gx == 7.0)  # n == 0 zeroes grad
    assert call(None, None, 0, None, None) == 0
    out = torch.full((250, 11), 7.0, device="cuda")
    dcall = L.lib().vr_query_sigma_grad_device
    xt = torch.from_numpy(np.array(x)).cuda()
    assert dcall(fresh._h, xt.data_ptr(), None, 256, None, None, None) == 1
    assert dcall(fresh._h, None, None, 256, out.data_ptr(), None, None) == 1
    assert dcall(fresh._h, None, None, 0, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out != 0))


# ------------------------------------------------------------------------------------------------
# 7. torch autograd
# ------------------------------------------------------------------------------------------------
def autograd_run(fn, gs, x, w, param_device="cuda"):
    import torch
    to = lambda a, d="cuda": torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    p = [to(a, param_device).requires_grad_() for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])]
    pts = to(x).requires_grad_()
    sig = fn(*p, pts)
    assert tuple(sig.shape) == (len(x), 2) and sig.dtype == torch.float32 and sig.requires_grad
    (sig * to(w)).sum().backward()
    assert p[3].grad is not None
    got = torch.cat([p[0].grad, p[1].grad, p[2].grad[:, None], p[3].grad[:, None]], 1).cpu().numpy()
    return sig.detach().cpu().numpy(), got, pts.grad.cpu().numpy()


def test_autograd_backward_is_the_gradient_query():
    import vr_amd as vr
    from vr_amd import autograd
    name = "50_random"
    gs = vr_scene(name).gaussians()  # (N, 14): mean, cov6, density, albedo, emission
    mdl = case(name, 1024)
    w = R.signed_weights(mdl.n)
    sig, got, got_x = autograd_run(autograd.sigma, gs, mdl.x, w)
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    assert np.array_equal(bits(sig), bits(dev.query_sigma(sc, mdl.x)))
    (G, S), (Gx, Sx) = expected(name, 1024)
    R.judge("autograd.sigma parameters", got, G, S)
    R.judge("autograd.sigma points", got_x, Gx, Sx)
    g_q, gx_q = dev.query_sigma_grad(sc, mdl.x, w, gaussians=True, positions=True)
    assert np.all(np.abs(got.astype(np.float64) - g_q) <= 2 * R.BOUND * S) and np.array_equal(bits(got_x), bits(gx_q))


def test_autograd_resident():
    """sigma_resident: the model's records carry the norm word of the device upload (upload_device_reference.device_norm)."""
    import torch
    from vr_amd import autograd
    name = "50_random"
    gs = vr_scene(name).gaussians()
    rec = GR.oracle_from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10]).records()
    rec[:, 10] = U.device_norm(np.ascontiguousarray(gs[:, 3:9], np.float32))
    rec = R.records_of_oracle(rec)
    x = case(name, 1024).x
    mdl = R.Model(rec, x)
    assert not mdl.near.any()
    w = R.signed_weights(mdl.n)
    sig, got, got_x = autograd_run(autograd.sigma_resident, gs, x, w)
    (G, S), (Gx, Sx) = mdl.both(w)
    R.judge("autograd.sigma_resident parameters", got, G, S)
    R.judge("autograd.sigma_resident points", got_x, Gx, Sx)
    with pytest.raises(ValueError):
        autograd_run(autograd.sigma_resident, gs, x, w, param_device="cpu")
    # only what requires grad is asked for
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    alb = to(gs[:, 10]).requires_grad_()
    s = autograd.sigma_resident(to(gs[:, 0:3]), to(gs[:, 3:9]), to(gs[:, 9]), alb, to(x))
    (s * to(w)).sum().backward()
    assert np.all(np.abs(alb.grad.cpu().numpy().astype(np.float64) - G[:, 10]) <= R.BOUND * S[:, 10])


# ------------------------------------------------------------------------------------------------
# 8. the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches(tmp_path):
    name = "250_random"
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    mdl = case(name, 1024)
    path = tmp_path / "points.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0, mdl.n))
        f.write(mdl.x.astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-sigma-grad", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("sg ")]
    assert [int(v[1]) for v in rows] == list(range(250)) and all(len(v) == 13 for v in rows)
    g = np.array([[int(h, 16) for h in v[2:]] for v in rows], np.uint32).view(np.float32)
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("sx ")]
    assert [int(v[1]) for v in rows] == list(range(mdl.n)) and all(len(v) == 5 for v in rows)
    gx = np.array([[int(h, 16) for h in v[2:]] for v in rows], np.uint32).view(np.float32)
    (G, S), (Gx, Sx) = expected(name, 1024, None, False)
    R.judge("C++ mirror (--query-sigma-grad) grad", g, G, S)
    R.judge("C++ mirror (--query-sigma-grad) grad_xyz", gx, Gx, Sx)
    g_py, gx_py = device().query_sigma_grad(vr_scene(name), mdl.x, None, gaussians=True, positions=True)
    assert np.all(np.abs(g.astype(np.float64) - g_py) <= 2 * R.BOUND * S) and np.array_equal(bits(gx), bits(gx_py))
