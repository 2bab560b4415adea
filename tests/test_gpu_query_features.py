"""The feature query (Device.evaluate_features / Device.features_gradient over vr_query_features[_grad][_device],
autograd.features[_resident], MixtureQuery::evaluate_features / features_gradient) against the float64 model of
tests/features_reference.py: records from the oracle scene read as doubles, the formulas of include/vr_hip.h in float64.

Forward: |F - model| <= FEAT_RTOL * S per entry, S = sum_g |m_g f_gc| (for mass: sum_g |m_g|), and exact +0 where S = 0.
FEAT_RTOL is 4 x the largest such ratio measured on an MI355X, the protocol of SIGMA_RTOL in tests/test_gpu_query.py: the
error is the same f32 mu_t's (its exponent of up to -4.5 carries a few ulp into expf) against float64, plus one f32
multiply per term. Measured: MEASURED_FORWARD below. The ties are exact: a channel of ones has the bits of mass;
channel 0 (the albedo) and mass give query_sigma's bits through a = F / mass, sigma_s = a * mass, sigma_a = (1 - a) * mass;
a channel's bits depend neither on C nor on its place.

Gradients: sigma_grad_reference's bound as it stands, |dev - model| <= 2^-21 S per component and exact zeros where S = 0:
both sides are double from the same f32 inputs and the same active set, the only f32 step is the final rounding
(<= 2^-24 S), which leaves 8x for the device's double exp. Every test prints its measured maximum before it asserts.
Measured on an MI355X: MEASURED_GRAD below.

Points: sigma_grad_reference.kept_recipe, the scenes and draw counts of tests/test_gpu_query_sigma_grad.py. Features:
features_reference.features_of (default_rng(7), U(-1, 1) f32; channel 0 the albedo, channel 1 ones).
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import features_reference as FR
import grad_reference as GR
import sigma_grad_reference as R
import upload_device_reference as U
from helpers import ROOT, scene_path

pytestmark = pytest.mark.gpu

# Largest |F - model| / S and |mass - model| / S_mass measured on an MI355X per case (see the module docstring).
MEASURED_FORWARD = ("1_gaussian 6.2e-7, 50_random 1.08e-6, 250_random 6.5e-7 (the same under every tree option), 65 537 points "
                    "1.66e-6 (the largest), negative densities 3.5e-7, the combs 6.2e-8, features_resident 1.04e-6")
MEASURED_GRAD = ("Gaussians' / features' / points' rows: 1_gaussian 1.0e-8 / 1.2e-9 / 5.8e-8, 50_random 5.3e-8 / 5.4e-8 / 5.9e-8, "
                 "250_random 5.7e-8 / 5.5e-8 / 6.0e-8 (the same under every tree option), 65 537 points 5.2e-9 / 3.5e-9 / 6.0e-8, "
                 "the combs 1.1e-8 / 1.6e-9 / 5.5e-8, autograd 3.0e-8 / 3.1e-8 / 5.8e-8: at or below 2^-24 = 6.0e-8, the final "
                 "rounding alone")
FEAT_RTOL = 6.7e-6  # 4 x 1.66e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device():
    import vr_amd as vr
    return vr.Device.get(0)


def to_cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def vr_scene(name):
    import vr_amd as vr
    return vr.Scene.load_GMM(scene_path(name + ".txt"))


@functools.lru_cache(maxsize=None)
def scene_records(name):
    return R.records_of_oracle(GR.oracle_scene(name).records())


@functools.lru_cache(maxsize=None)
def case(name, n_draw, n_keep, C):
    """The shared model of scene `name` at the recipe's kept points with C feature channels."""
    rec = scene_records(name)
    mdl = R.kept_recipe(rec, n_draw, n_keep)
    print(f"{name}: {mdl.n} points kept, {mdl.dropped} of {n_draw} dropped, active per point up to {int(mdl.n_active.max())}, "
          f"{int((mdl.n_active == 0).sum())} in no ellipsoid")
    return FR.FeatureModel(mdl, FR.features_of(rec, C))


@functools.lru_cache(maxsize=None)
def expected(name, n_draw, n_keep, C, signed=True):
    fm = case(name, n_draw, n_keep, C)
    return fm.grads(*(FR.signed_weights(fm.mdl.n, C) if signed else (None, None)))


def judge_forward(label, F, mass, act, fm, rows=None):
    """Prints the measured maxima, then asserts the forward's bound, the exact zeros and the active counts."""
    rows = slice(None) if rows is None else rows
    assert FEAT_RTOL <= 1e-4
    assert F.dtype == np.float32 and mass.dtype == np.float32
    assert np.array_equal(act, fm.mdl.n_active[rows])
    worst = 0.0
    for what, dev, ref, S in (("F", F, fm.F[rows], fm.S[rows]), ("mass", mass, fm.mass[rows], fm.S_mass[rows])):
        assert dev.shape == ref.shape, (dev.shape, ref.shape)
        err = np.abs(dev.astype(np.float64) - ref)
        with np.errstate(all="ignore"):
            rel = np.where(S > 0, err / S, 0.0)
        print(f"{label} {what}: max |dev - model| / S = {rel.max() if rel.size else 0.0:.3e} (FEAT_RTOL {FEAT_RTOL:.1e}), "
              f"entries with S = 0: {int((S == 0).sum())}")
        assert np.all(np.isfinite(dev)) and not np.any(bits(dev)[S == 0])
        assert np.all(err <= FEAT_RTOL * S), float(rel.max())
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
    return worst


def judge_grads(label, got, exp):
    for what, dev, (G, S) in zip(("grad", "grad_features", "grad_xyz"), got, exp):
        assert dev.dtype == np.float32
        R.judge(f"{label} {what}", dev, G, S)


def sigma_from(F0, mass):
    """gmm.h:115-125 in f32 from channel 0 (the albedo) and the mass: (sigma_a, sigma_s), (0, 0) where mass is not > 0."""
    F0, mass = np.ascontiguousarray(F0, np.float32), np.ascontiguousarray(mass, np.float32)
    with np.errstate(all="ignore"):
        a = F0 / mass
        ss, sa = a * mass, (np.float32(1.0) - a) * mass
    live = mass > 0
    return np.stack([np.where(live, sa, np.float32(0)), np.where(live, ss, np.float32(0))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# 1. one Gaussian: every lane adds to the same words; a partial wave
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_one_gaussian_257_points(C):
    fm = case("1_gaussian", 264, 257, C)
    mdl = fm.mdl
    assert mdl.n == 257 and mdl.n_active.sum() >= 200
    dev, sc = device(), vr_scene("1_gaussian")
    F, mass, act = dev.evaluate_features(sc, mdl.x, fm.f, return_mass=True, return_active=True)
    assert F.shape == (257, C) and mass.shape == (257,) and act.shape == (257,)
    judge_forward(f"1_gaussian C={C}", F, mass, act, fm)
    w, u = FR.signed_weights(257, C)
    got = dev.features_gradient(sc, mdl.x, fm.f, w, u, gaussians=True, features_grad=True, positions=True)
    assert got[0].shape == (1, 10) and got[1].shape == (1, C) and got[2].shape == (257, 3)
    judge_grads(f"1_gaussian C={C}", got, expected("1_gaussian", 264, 257, C))


# ------------------------------------------------------------------------------------------------
# 2. random scenes, C = 19 (two full chunks and three channels): the forward and its exact ties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["50_random", "250_random"])
def test_random_scene_forward(name):
    fm = case(name, 1024, None, 19)
    mdl = fm.mdl
    dev, sc = device(), vr_scene(name)
    assert mdl.active.any(0).all() and mdl.n_active.max() >= 2 and (mdl.n_active == 0).any()
    F, mass, act = dev.evaluate_features(sc, mdl.x, fm.f, return_mass=True, return_active=True)
    assert F.shape == (mdl.n, 19)
    judge_forward(f"{name} C=19", F, mass, act, fm)
    # a channel of ones has the bits of mass; the albedo channel and mass give query_sigma's bits
    assert np.array_equal(bits(F[:, 1]), bits(mass))
    sig, sig_act = dev.query_sigma(sc, mdl.x, return_active=True)
    assert np.array_equal(sig_act, act)
    assert np.array_equal(bits(sigma_from(F[:, 0], mass)), bits(sig))
    # a channel's bits depend neither on C nor on its place among the C
    col = np.ascontiguousarray(fm.f[:, 10:11])
    alone = dev.evaluate_features(sc, mdl.x, col)
    assert alone.shape == (mdl.n, 1) and np.array_equal(bits(alone[:, 0]), bits(F[:, 10]))
    for C, at in ((8, 7), (9, 8), (9, 0)):
        f = np.array(FR.features_of(mdl.rec, C, seed=C))
        f[:, at] = col[:, 0]
        got, m2 = dev.evaluate_features(sc, mdl.x, f, return_mass=True)
        assert np.array_equal(bits(got[:, at]), bits(F[:, 10])) and np.array_equal(bits(m2), bits(mass)), (C, at)
    # only the mass, only the counts; numpy and torch forms
    assert np.array_equal(dev.evaluate_features(sc, mdl.x, fm.f, return_active=True)[1], act)
    F_t, mass_t, act_t = dev.evaluate_features(sc, to_cuda(mdl.x), to_cuda(fm.f), return_mass=True, return_active=True)
    assert F_t.is_cuda and tuple(F_t.shape) == (mdl.n, 19) and tuple(mass_t.shape) == (mdl.n,)
    assert np.array_equal(bits(F_t.cpu().numpy()), bits(F)) and np.array_equal(bits(mass_t.cpu().numpy()), bits(mass))
    assert np.array_equal(act_t.cpu().numpy(), act)
    only = dev.evaluate_features(sc, to_cuda(mdl.x), to_cuda(fm.f))
    assert np.array_equal(bits(only.cpu().numpy()), bits(F))


# ------------------------------------------------------------------------------------------------
# 3. random scenes: the gradients, every form of the call, numpy and torch, the sigma gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["50_random", "250_random"])
def test_random_scene_gradients(name):
    C = 19
    fm = case(name, 1024, None, C)
    mdl = fm.mdl
    dev, sc = device(), vr_scene(name)
    N, n = mdl.N, mdl.n
    w, u = FR.signed_weights(n, C)
    exp = expected(name, 1024, None, C)
    (G, S), (Gf, Sf), (Gx, Sx) = exp
    g, gf, gx = dev.features_gradient(sc, mdl.x, fm.f, w, u, positions=True)
    assert g.shape == (N, 10) and gf.shape == (N, C) and gx.shape == (n, 3)
    judge_grads(f"{name} all three", (g, gf, gx), exp)
    ask = lambda a, b, c, kind=lambda v: v: dev.features_gradient(  # noqa: E731
        sc, kind(mdl.x), kind(fm.f), kind(w), kind(u), gaussians=a, features_grad=b, positions=c)
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v  # noqa: E731
    for kind in (lambda v: v, to_cuda):
        for a, b, c in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
            got = ask(a, b, c, kind)
            got = list(got) if isinstance(got, tuple) else [got]
            assert len(got) == a + b + c
            label = f"{name} {'torch' if kind is to_cuda else 'numpy'} gaussians={a} features={b} positions={c}"
            if a:
                one = host(got.pop(0))
                R.judge(label + " grad", one, G, S)
                assert np.all(np.abs(one.astype(np.float64) - g) <= 2 * R.BOUND * S)
            if b:
                one = host(got.pop(0))
                R.judge(label + " grad_features", one, Gf, Sf)
                assert np.all(np.abs(one.astype(np.float64) - gf) <= 2 * R.BOUND * Sf)
            if c:
                one = host(got.pop(0))
                assert one.shape == (n, 3) and np.array_equal(bits(one), bits(gx))
    # weights=None is ones, weight_mass=None zeros
    exp1 = expected(name, 1024, None, C, False)
    none = dev.features_gradient(sc, mdl.x, fm.f, positions=True)
    ones = dev.features_gradient(sc, mdl.x, fm.f, np.ones((n, C), np.float32), np.zeros(n, np.float32), positions=True)
    judge_grads(f"{name} weights=None", none, exp1)
    for a, b, (_, S1) in zip(none[:2], ones[:2], exp1[:2]):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * R.BOUND * S1)
    assert np.array_equal(bits(none[2]), bits(ones[2]))
    # one channel of albedo with (w, u) = (w_s - w_a, w_a) is the sigma gradient (weights on a grid of 2^-12, so that
    # w_s = u + w is exact in f32 and both queries get the same numbers)
    grid = np.round(R.signed_weights(n).astype(np.float64) * 4096.0) / 4096.0
    ws, ua = grid[:, 1:2].astype(np.float32), np.ascontiguousarray(grid[:, 0].astype(np.float32))
    w2 = np.ascontiguousarray(np.stack([grid[:, 0], grid[:, 0] + grid[:, 1]], 1).astype(np.float32))
    assert np.array_equal(w2.astype(np.float64)[:, 1] - w2[:, 0], ws[:, 0].astype(np.float64))
    alb = np.ascontiguousarray(fm.f[:, 0:1])
    g1, gf1, gx1 = dev.features_gradient(sc, mdl.x, alb, ws, ua, positions=True)
    sg, sx = dev.query_sigma_grad(sc, mdl.x, w2, gaussians=True, positions=True)
    (Gs, Ss), (Gsx, Ssx) = mdl.both(w2)
    R.judge(f"{name} C=1 albedo: grad against the sigma model", g1, Gs[:, :10], Ss[:, :10])
    R.judge(f"{name} C=1 albedo: grad_features against the sigma model's albedo column", gf1, Gs[:, 10:11], Ss[:, 10:11])
    R.judge(f"{name} C=1 albedo: grad_xyz against the sigma model", gx1, Gsx, Ssx)
    assert np.all(np.abs(g1.astype(np.float64) - sg[:, :10]) <= 2 * R.BOUND * Ss[:, :10])
    assert np.all(np.abs(gf1[:, 0].astype(np.float64) - sg[:, 10]) <= 2 * R.BOUND * Ss[:, 10])
    assert np.all(np.abs(gx1.astype(np.float64) - sx) <= 2 * R.BOUND * Ssx)


# ------------------------------------------------------------------------------------------------
# 4. 65 537 points: 256 blocks and one lane
# ------------------------------------------------------------------------------------------------
def test_65537_points():
    name, C = "50_random", 3
    fm = case(name, 66200, 65537, C)
    mdl = fm.mdl
    assert mdl.n == 65537 == 256 * 256 + 1
    dev, sc = device(), vr_scene(name)
    F, mass, act = dev.evaluate_features(sc, mdl.x, fm.f, return_mass=True, return_active=True)
    judge_forward("50_random x 65537", F, mass, act, fm)
    assert np.array_equal(bits(F[:, 1]), bits(mass))
    w, u = FR.signed_weights(mdl.n, C)
    got = dev.features_gradient(sc, mdl.x, fm.f, w, u, positions=True)
    judge_grads("50_random x 65537", got, expected(name, 66200, 65537, C))


# ------------------------------------------------------------------------------------------------
# 5. tree options: the 4-wide walk, the child-pair walk, host and device builders
# ------------------------------------------------------------------------------------------------
def test_tree_options_change_nothing_beyond_rounding():
    import vr_amd as vr
    name, C = "250_random", 19
    fm = case(name, 1024, None, C)
    mdl = fm.mdl
    w, u = FR.signed_weights(mdl.n, C)
    exp = expected(name, 1024, None, C)
    dev = vr.Device(0)
    out, fwd = {}, {}
    for half in (0, 1):
        for dbvh in (0, 1):
            dev.set_option("half_nodes", half)
            dev.set_option("device_bvh", dbvh)
            F, mass, act = dev.evaluate_features(vr_scene(name), mdl.x, fm.f, return_mass=True, return_active=True)
            judge_forward(f"250_random half_nodes={half} device_bvh={dbvh}", F, mass, act, fm)
            got = dev.features_gradient(vr_scene(name), mdl.x, fm.f, w, u, positions=True)
            judge_grads(f"250_random half_nodes={half} device_bvh={dbvh}", got, exp)
            out[half, dbvh], fwd[half, dbvh] = got, (F, mass)
    for key in out:
        assert np.array_equal(bits(fwd[key][0]), bits(fwd[1, 0][0])) and np.array_equal(bits(fwd[key][1]), bits(fwd[1, 0][1]))
        for a, b, (_, S) in zip(out[key], out[1, 0], exp):
            assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * R.BOUND * S)


# ------------------------------------------------------------------------------------------------
# 6. points that contribute nothing
# ------------------------------------------------------------------------------------------------
def test_far_and_nan_points_get_zero_rows():
    name, C = "50_random", 3
    rec = scene_records(name)
    base = case(name, 1024, None, C).mdl
    lonely = int(np.argmin(base.active.sum(0)))  # the Gaussian holding the fewest points: here it holds none
    inside = base.x[~base.active[:, lonely] & (base.n_active > 0)][:40]
    mdl = R.Model(rec, inside)
    assert mdl.n == 40 and not mdl.near.any() and not mdl.active[:, lonely].any()
    fm = FR.FeatureModel(mdl, FR.features_of(rec, C))
    far = (rec[0][0] + 100.0).astype(np.float32)
    bad = inside[0].copy()
    bad[1] = np.nan
    pts = np.ascontiguousarray(np.concatenate([inside[:20], far[None], bad[None], inside[20:]]))
    w, u = FR.signed_weights(len(pts), C)
    keep = np.r_[0:20, 22:len(pts)]
    dev, sc = device(), vr_scene(name)
    F, mass, act = dev.evaluate_features(sc, pts, fm.f, return_mass=True, return_active=True)
    judge_forward("with a far and a NaN point", F[keep], mass[keep], act[keep], fm)
    assert not np.any(bits(F[20:22])) and not np.any(bits(mass[20:22])) and not np.any(act[20:22])
    g, gf, gx = dev.features_gradient(sc, pts, fm.f, w, u, positions=True)
    exp = fm.grads(w[keep], u[keep])
    judge_grads("with a far and a NaN point", (g, gf, gx[keep]), exp)
    assert not np.any(bits(gx[20:22]))  # +0 rows
    empty = ~(exp[0][1] > 0).any(1)
    assert empty.any() and not np.any(bits(g[empty])) and not np.any(bits(gf[empty]))
    for got in dev.features_gradient(sc, pts[20:22], fm.f, None, None, positions=True):
        assert not np.any(bits(got))
    none = dev.features_gradient(sc, pts[:0], fm.f, positions=True)
    assert [a.shape for a in none] == [(50, 10), (50, C), (0, 3)] and not any(np.any(bits(a)) for a in none)
    assert dev.evaluate_features(sc, pts[:0], fm.f).shape == (0, C)


def test_points_of_non_positive_mass_are_taken_back():
    """The two-Gaussian scene of tests/test_gpu_query_sigma_grad.py: a Gaussian of negative density inside a positive one. Near
    the centre the summed m is < 0: the forward gives +0 everywhere and the gradient takes such a point's adds back."""
    import vr_amd as vr
    F32 = np.float32
    C = 3
    mean = np.zeros((2, 3), F32)
    cov6 = np.array([[0.04, 0, 0, 0.04, 0, 0.04], [0.01, 0, 0, 0.01, 0, 0.01]], F32)
    density, albedo = np.array([1.0, -0.5], F32), np.array([0.3, 0.8], F32)
    rec = R.records_of_oracle(GR.oracle_from_gaussians(mean, cov6, density, albedo).records())
    x = R.recipe_points(rec, 300)
    m, q = R.mass(rec, x)
    ok = ~np.any(np.abs(q - 9.0) <= R.Q_MARGIN, axis=1) & (np.abs(m.sum(1)) >= 1e-3 * np.abs(m).sum(1))
    x = np.ascontiguousarray(x[ok][:257])
    assert len(x) == 257
    mdl = R.Model(rec, x)
    fm = FR.FeatureModel(mdl, FR.features_of(rec, C))
    tot = R.mass(rec, x)[0].sum(1)
    dead, live = (tot <= 0) & (mdl.n_active > 0), (tot > 0) & (mdl.n_active == 2)
    assert dead.sum() >= 30 and live.sum() >= 30
    sc = vr.Scene.from_gaussians(mean, cov6, density, albedo)
    dev = device()
    F, mass, act = dev.evaluate_features(sc, x, fm.f, return_mass=True, return_active=True)
    judge_forward("negative density", F, mass, act, fm)
    assert not np.any(bits(F[dead])) and not np.any(bits(mass[dead])) and np.all(mass[live] > 0)
    assert np.array_equal(bits(sigma_from(F[:, 0], mass)), bits(dev.query_sigma(sc, x)))
    w, u = FR.signed_weights(257, C)
    got = dev.features_gradient(sc, x, fm.f, w, u, positions=True)
    exp = fm.grads(w, u)
    assert not np.any(exp[2][1][dead]) and not np.any(bits(got[2][dead]))
    judge_grads("negative density", got, exp)
    assert np.array_equal(bits(dev.features_gradient(sc, x, fm.f, w, u, gaussians=False, features_grad=False, positions=True)),
                          bits(got[2]))


def test_walks_at_the_stack_limit_are_taken_back(device_options):
    """The mirrored comb of tests/wide_walk_reference.py under the device builder's 4-wide tree: every point's containment
    walk reaches sp + 4 > kStackSize, so whatever the broken-off walk added is taken back and the child-pair walk adds the
    whole active set. The plain comb's walks stay under the limit. The ballast holds no point: exact zeros."""
    import tree_reference as T
    import vr_amd as vr
    import wide_walk_reference as W
    C = 3
    leaf_max = T.limits()["leaf_max"]
    device_options("device_bvh", 1)
    device_options("half_nodes", 1)
    dev = vr.Device.get(0)
    p = (W.CENTRE + np.random.default_rng(74).uniform(-0.4, 0.4, (256, 3)) * W.EXTENT).astype(np.float32)
    w, u = FR.signed_weights(256, C)
    for mirrored in (True, False):
        sc = W.comb_scene(leaf_max, mirrored)
        dev.upload(sc, force=True)
        sim = W.walk_sigma(dev.debug_tree(), p, 32)
        assert sum(r["fire"] is not None for r in sim) == (256 if mirrored else 0)
        rec = R.records_of_oracle(W.comb_oracle(leaf_max, mirrored).records())
        mdl = R.Model(rec, p)
        assert not mdl.near.any() and np.all(mdl.n_active == W.comb_count(leaf_max))
        fm = FR.FeatureModel(mdl, FR.features_of(rec, C))
        F, mass, act = dev.evaluate_features(sc, p, fm.f, return_mass=True, return_active=True)
        judge_forward(f"comb mirrored={mirrored}", F, mass, act, fm)
        got = dev.features_gradient(sc, p, fm.f, w, u, positions=True)
        exp = fm.grads(w, u)
        assert not (exp[0][1][W.comb_count(leaf_max):] > 0).any() and not (exp[1][1][W.comb_count(leaf_max):] > 0).any()
        judge_grads(f"comb mirrored={mirrored}", got, exp)


# ------------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    lib = L.lib()
    C = 3
    fm = case("250_random", 1024, None, 19)
    x = np.ascontiguousarray(fm.mdl.x[:256])
    f = np.ascontiguousarray(fm.f[:, :C])
    out, mass = np.full((256, C), 7.0, np.float32), np.full(256, 7.0, np.float32)
    act = np.full(256, 7, np.uint32)
    g, gf, gx = np.full((250, 10), 7.0, np.float32), np.full((250, C), 7.0, np.float32), np.full((256, 3), 7.0, np.float32)
    P, up = L.fptr, lambda a: a.ctypes.data_as(L.U32P)  # noqa: E731
    fwd = lambda p, n, ft, c, o: lib.vr_query_features(fresh._h, p, n, ft, c, o, P(mass), up(act))  # noqa: E731
    grd = lambda p, n, ft, c, a, b, d: lib.vr_query_features_grad(fresh._h, p, n, ft, c, None, None, a, b, d)  # noqa: E731
    assert fwd(P(x), 256, P(f), C, P(out)) == 5 and grd(P(x), 256, P(f), C, P(g), P(gf), P(gx)) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert fwd(P(x), 256, P(f), C, P(out)) == 7 and grd(P(x), 256, P(f), C, P(g), P(gf), P(gx)) == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene("250_random"))
    for bad_c in (0, 65):  # VR_ERR_INVALID
        assert fwd(P(x), 256, P(f), bad_c, P(out)) == 1 and b"C must lie in [1, 64]" in lib.vr_last_error()
        assert grd(P(x), 256, P(f), bad_c, P(g), P(gf), P(gx)) == 1 and b"C must lie in [1, 64]" in lib.vr_last_error()
        assert grd(None, 0, None, bad_c, P(g), P(gf), None) == 1
    assert fwd(None, 256, P(f), C, P(out)) == 1 and fwd(P(x), 256, None, C, P(out)) == 1 and fwd(P(x), 256, P(f), C, None) == 1
    assert grd(None, 256, P(f), C, P(g), P(gf), P(gx)) == 1 and grd(P(x), 256, None, C, P(g), P(gf), P(gx)) == 1
    assert grd(P(x), 256, P(f), C, None, None, None) == 1 and b"all three outputs" in lib.vr_last_error()
    assert fwd(P(x), 1 << 31, P(f), C, P(out)) == 1 and grd(P(x), 1 << 31, P(f), C, P(g), P(gf), P(gx)) == 1
    assert fwd(P(x), 1 << 30, P(f), 2, P(out)) == 1 and grd(P(x), 1 << 30, P(f), 2, P(g), P(gf), P(gx)) == 1  # n * C = 2^31
    for a in (out, mass, g, gf, gx):
        assert np.all(a == 7.0)
    assert np.all(act == 7)
    # n == 0: nothing is launched, the gradients are zeroed
    assert fwd(None, 0, None, C, None) == 0 and np.all(out == 7.0)
    assert grd(None, 0, None, C, P(g), P(gf), P(gx)) == 0
    assert not np.any(bits(g)) and not np.any(bits(gf)) and np.all(gx == 7.0)
    assert grd(None, 0, None, C, None, None, None) == 0
    # an empty scene gives zeros
    hollow = vr.Scene.from_gaussians(np.zeros((0, 3)), np.zeros((0, 6)), [], [], [vr.Light([0, 1, 0], [1, 1, 1])])
    fresh.upload(hollow)
    none = np.zeros((0, C), np.float32)
    assert fwd(P(x), 256, P(none), C, P(out)) == 0 and not np.any(bits(out)) and not np.any(bits(mass)) and not np.any(act)
    assert grd(P(x), 256, P(none), C, None, None, P(gx)) == 0 and not np.any(bits(gx))
    assert fresh.evaluate_features(hollow, x, none).shape == (256, C)
    # the _device forms with torch pointers
    fresh.upload(vr_scene("250_random"))
    xt, ft = to_cuda(x), to_cuda(f)
    o_t, g_t, gf_t = (torch.full(s, 7.0, device="cuda") for s in ((256, C), (250, 10), (250, C)))
    dfw, dgr = lib.vr_query_features_device, lib.vr_query_features_grad_device
    assert dfw(fresh._h, xt.data_ptr(), 256, ft.data_ptr(), 0, o_t.data_ptr(), None, None, None) == 1
    assert dfw(fresh._h, xt.data_ptr(), 256, None, C, o_t.data_ptr(), None, None, None) == 1
    assert dgr(fresh._h, xt.data_ptr(), 256, ft.data_ptr(), C, None, None, None, None, None, None) == 1
    assert dgr(fresh._h, None, 256, ft.data_ptr(), C, None, None, g_t.data_ptr(), None, None, None) == 1
    assert dgr(fresh._h, xt.data_ptr(), 256, ft.data_ptr(), 65, None, None, g_t.data_ptr(), None, None, None) == 1
    torch.cuda.synchronize()
    assert bool(torch.all(o_t == 7.0)) and bool(torch.all(g_t == 7.0))
    assert dgr(fresh._h, None, 0, None, C, None, None, g_t.data_ptr(), gf_t.data_ptr(), None, None) == 0
    assert dfw(fresh._h, xt.data_ptr(), 256, ft.data_ptr(), C, o_t.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(g_t != 0)) and not bool(torch.any(gf_t != 0))
    assert np.array_equal(bits(o_t.cpu().numpy()), bits(device().evaluate_features(vr_scene("250_random"), x, f)))


# ------------------------------------------------------------------------------------------------
# 8. torch autograd
# ------------------------------------------------------------------------------------------------
def autograd_run(fn, gs, f, x, w, u, param_device="cuda"):
    import torch
    to = lambda a, d="cuda": torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    p = [to(a, param_device).requires_grad_() for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10], f)]
    pts = to(x).requires_grad_()
    F, mass = fn(*p, pts)
    assert tuple(F.shape) == (len(x), f.shape[1]) and tuple(mass.shape) == (len(x),) and F.dtype == torch.float32
    assert F.requires_grad and mass.requires_grad
    ((F * to(w)).sum() + (mass * to(u)).sum()).backward()
    assert p[3].grad is None  # albedo
    got = torch.cat([p[0].grad, p[1].grad, p[2].grad[:, None]], 1).cpu().numpy()
    return F.detach().cpu().numpy(), mass.detach().cpu().numpy(), (got, p[4].grad.cpu().numpy(), pts.grad.cpu().numpy())


def test_autograd_backward_is_the_gradient_query():
    import vr_amd as vr
    from vr_amd import autograd
    name, C = "50_random", 3
    gs = vr_scene(name).gaussians()  # (N, 14): mean, cov6, density, albedo, emission
    fm = case(name, 1024, None, C)
    mdl = fm.mdl
    w, u = FR.signed_weights(mdl.n, C)
    F, mass, got = autograd_run(autograd.features, gs, fm.f, mdl.x, w, u)
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    F_q, mass_q = dev.evaluate_features(sc, mdl.x, fm.f, return_mass=True)
    assert np.array_equal(bits(F), bits(F_q)) and np.array_equal(bits(mass), bits(mass_q))
    exp = expected(name, 1024, None, C)
    judge_grads("autograd.features", got, exp)
    q = dev.features_gradient(sc, mdl.x, fm.f, w, u, positions=True)
    for a, b, (_, S) in zip(got[:2], q[:2], exp[:2]):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * R.BOUND * S)
    assert np.array_equal(bits(got[2]), bits(q[2]))


def test_autograd_resident_and_only_what_is_needed(monkeypatch):
    """features_resident: the model's records carry the norm word of the device upload (upload_device_reference.device_norm).
    Backward asks Device.features_gradient only for the outputs some input needs (a counting wrapper sees the flags)."""
    import vr_amd as vr
    from vr_amd import autograd
    name, C = "50_random", 3
    gs = vr_scene(name).gaussians()
    rec = GR.oracle_from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10]).records()
    rec[:, 10] = U.device_norm(np.ascontiguousarray(gs[:, 3:9], np.float32))
    rec = R.records_of_oracle(rec)
    base = case(name, 1024, None, C)
    mdl = R.Model(rec, base.mdl.x)
    assert not mdl.near.any()
    fm = FR.FeatureModel(mdl, base.f)
    w, u = FR.signed_weights(mdl.n, C)
    calls = []
    real = vr.Device.features_gradient

    def counting(self, scene, points, features, weights=None, weight_mass=None, gaussians=True, features_grad=True, positions=False):
        calls.append((bool(gaussians), bool(features_grad), bool(positions)))
        return real(self, scene, points, features, weights, weight_mass, gaussians, features_grad, positions)

    monkeypatch.setattr(vr.Device, "features_gradient", counting)
    F, mass, got = autograd_run(autograd.features_resident, gs, fm.f, mdl.x, w, u)
    assert calls == [(True, True, True)]
    judge_forward("autograd.features_resident", F, mass, mdl.n_active, fm)
    exp = fm.grads(w, u)
    judge_grads("autograd.features_resident", got, exp)
    with pytest.raises(ValueError):
        autograd_run(autograd.features_resident, gs, fm.f, mdl.x, w, u, param_device="cpu")
    # one input at a time
    x_t, w_t, u_t = to_cuda(mdl.x), to_cuda(w), to_cuda(u)
    for which, flags in ((2, (True, False, False)), (4, (False, True, False)), (5, (False, False, True))):
        del calls[:]
        args = [to_cuda(a) for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10], fm.f)] + [x_t.clone()]
        args[which].requires_grad_()
        F_t, mass_t = autograd.features_resident(*args)
        ((F_t * w_t).sum() + (mass_t * u_t).sum()).backward()
        assert calls == [flags], (which, calls)
        grad = args[which].grad.cpu().numpy()
        G, S = (exp[0][0][:, 9], exp[0][1][:, 9]) if which == 2 else exp[1] if which == 4 else exp[2]
        assert np.all(np.abs(grad.astype(np.float64) - G) <= R.BOUND * S)
    # albedo alone needs nothing: no call at all
    del calls[:]
    args = [to_cuda(a) for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10], fm.f)] + [x_t]
    args[3].requires_grad_()
    F_t, mass_t = autograd.features_resident(*args)
    ((F_t * w_t).sum() + (mass_t * u_t).sum()).backward()
    assert not calls and args[3].grad is None


# ------------------------------------------------------------------------------------------------
# 9. the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches(tmp_path):
    name, C = "250_random", 5
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    fm = case(name, 1024, None, C)
    mdl = fm.mdl
    path, fpath = tmp_path / "points.bin", tmp_path / "features.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0, mdl.n))
        f.write(mdl.x.astype("<f4").tobytes())
    with open(fpath, "wb") as f:
        f.write(struct.pack("<II", mdl.N, C))
        f.write(fm.f.astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-features", str(path), str(fpath)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def rows(tag, count, width, skip=2):
        got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(tag + " ")]
        assert [int(v[1]) for v in got] == list(range(count)) and all(len(v) == skip + width for v in got), tag
        return got, np.array([[int(h, 16) for h in v[skip:]] for v in got], np.uint32).view(np.float32)

    raw, fq = rows("fq", mdl.n, 1 + C, skip=3)
    act = np.array([int(v[2]) for v in raw])
    F_py, mass_py, act_py = device().evaluate_features(vr_scene(name), mdl.x, fm.f, return_mass=True, return_active=True)
    assert np.array_equal(bits(fq[:, 1:]), bits(F_py)) and np.array_equal(bits(fq[:, 0]), bits(mass_py)) and np.array_equal(act, act_py)
    got = (rows("fg", mdl.N, 10)[1], rows("fr", mdl.N, C)[1], rows("fx", mdl.n, 3)[1])
    exp = expected(name, 1024, None, C, False)
    judge_grads("C++ mirror (--query-features)", got, exp)
    py = device().features_gradient(vr_scene(name), mdl.x, fm.f, positions=True)
    for a, b, (_, S) in zip(got[:2], py[:2], exp[:2]):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * R.BOUND * S)
    assert np.array_equal(bits(got[2]), bits(py[2]))
