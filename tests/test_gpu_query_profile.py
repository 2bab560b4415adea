"""The transmittance profile query (Device.query_transmittance_profile[_grad] over vr_query_transmittance_profile*):
tau and Tr at K distances per ray from one walk, and the gradient of a weighted sum of those optical depths.

Forward: column k must have the bits of Device.query_transmittance(..., tmax=t[:, k], return_tau=True), whatever K, the
order of the samples and the tree. KC = 16 is the number of samples of one work item of the forward walk
(kernels/vr_query_profile.hip), so K runs over 1, KC - 1, KC, KC + 1 and 2 KC + 3.

Gradient: the float64 model of tests/grad_reference.py on the n * K expanded rays (tests/profile_reference.py), under
that model's own bound |G_dev - G64| <= 2^-21 S per component (R.judge), and within 2 * 2^-21 S of
Device.query_transmittance_grad on the expanded rays, as the existing tests compare two device results.

Rays: the sphere sets of test_gpu_query_grad.py plus one ray, so that the last wave is partial (257)."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import grad_reference as R
import profile_reference as PR
from helpers import CAM_POS, FOV, ROOT, main_view_dir, scene_path
from test_gpu_query_grad import one_gaussian_case, sphere_rays, vr_scene

pytestmark = pytest.mark.gpu
KC = 16
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def device():
    import vr_amd as vr
    return vr.Device.get(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rays257(name):
    """The 256 sphere rays and one more (ray 5's origin moved a little, aimed as ray 9): (o, d, centre), read-only."""
    o, d, _ = sphere_rays(name)
    m = R.oracle_scene(name).records()[:, :3].astype(np.float64)
    c = 0.5 * (m.min(0) + m.max(0))
    o = np.concatenate([o, o[5:6] + np.float32([0.05, -0.03, 0.02])]).astype(np.float32)
    d = np.concatenate([d, d[9:10]]).astype(np.float32)
    for a in (o, d):
        a.setflags(write=False)
    return o, d, c


@functools.lru_cache(maxsize=None)
def samples(name, K):
    """(257, K) f32: per ray K distances U(0, 2 |centre - o|), unsorted. default_rng(13)."""
    o, _, c = rays257(name)
    reach = 2.0 * np.linalg.norm(c - o.astype(np.float64), axis=1)
    t = (np.random.default_rng(13).uniform(0, 1, (len(o), K)) * reach[:, None]).astype(np.float32)
    t.setflags(write=False)
    return t


def single_queries(dev, sc, o, d, t):
    """(tr, tau), each (n, K): one Device.query_transmittance call per column."""
    cols = [dev.query_transmittance(sc, o, d, tmax=np.ascontiguousarray(t[:, k]), return_tau=True) for k in range(t.shape[1])]
    return np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)


@functools.lru_cache(maxsize=None)
def single_reference(name):
    """The single query at every one of the 2 KC + 3 sample columns, on the default tree. Read-only."""
    o, d, _ = rays257(name)
    tr, tau = single_queries(device(), vr_scene(name), o, d, samples(name, 2 * KC + 3))
    tr.setflags(write=False)
    tau.setflags(write=False)
    return tr, tau


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------------------------
# 1. bit equality with the single query
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, KC - 1, KC, KC + 1, 2 * KC + 3])
@pytest.mark.parametrize("name", ["250_random", "1000_random"])
def test_profile_has_the_bits_of_the_single_query(name, K):
    o, d, _ = rays257(name)
    t = np.ascontiguousarray(samples(name, 2 * KC + 3)[:, :K])
    tr, tau = device().query_transmittance_profile(vr_scene(name), o, d, t, return_tau=True)
    assert tr.shape == tau.shape == (257, K) and tr.dtype == tau.dtype == np.float32
    ref_tr, ref_tau = single_reference(name)
    print(f"{name} K={K}: tau {tau.min():.3e} .. {tau.max():.3e}, {int((tau > 0).sum())} of {tau.size} samples see the cloud")
    assert (tau > 0).mean() > 0.5
    same_bits(tau, ref_tau[:, :K], "tau")
    same_bits(tr, ref_tr[:, :K], "tr")
    # from the oracle's probe: (ray, sample, Gaussian) triples of all three classes are among what was compared
    mdl = profile_model(name, 1)
    a = np.maximum(np.float32(0), mdl.te)[:, None, :]
    h, tk, tx = mdl.hit[:, None, :], t[:, :, None], mdl.tx[:, None, :]
    before, inside, past = (h & ~(tk > a)).sum(), (h & (tk > a) & (tk < tx)).sum(), (h & (tk >= tx)).sum()
    print(f"  before the entry {before}, inside the chord {inside}, past the exit {past}")
    assert before > 0 and inside > 0 and past > 0


# ------------------------------------------------------------------------------------------------
# 2. special samples, invalid rays, unit, shared rows, numpy / torch, the outputs asked for
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_case():
    name, K = "250_random", KC + 4
    o, d, _ = rays257(name)
    o = o.copy()
    t = samples(name, K).copy()
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = 0.0, -1.0, NAN, INF
    t[:, 4] = t[:, 5]                       # a duplicate
    t[:, KC + 1] = t[:, KC - 1]             # and one across the chunks
    t[7] = np.resize(np.float32([0.0, -1.0, NAN]), K)  # no sample > 0
    t[200, KC:] = np.float32([NAN, -2.0, 0.0, -0.0])  # nor in this ray's second chunk
    o[11, 1] = NAN                          # an invalid ray
    for a in (o, t):
        a.setflags(write=False)
    return name, o, d, t


def test_special_samples():
    name, o, d, t = special_case()
    dev, sc = device(), vr_scene(name)
    tr, tau = dev.query_transmittance_profile(sc, o, d, t, return_tau=True)
    ref_tr, ref_tau = single_queries(dev, sc, o, d, t)
    same_bits(tau, ref_tau, "tau")
    same_bits(tr, ref_tr, "tr")
    ok = np.arange(257) != 11
    assert np.all(np.isnan(tr[11])) and np.all(np.isnan(tau[11]))
    for col in (0, 1, 2):
        assert np.all(tau[ok, col] == 0.0) and np.all(tr[ok, col] == 1.0)
    assert np.all(tau[7] == 0.0) and np.all(tr[7] == 1.0) and np.all(tau[200, KC:] == 0.0) and np.all(tr[200, KC:] == 1.0)
    assert np.all(tau[ok, 3] >= tau[ok].max(1)) and np.any(tau[ok, 3] > 0)  # +inf: the whole ray
    rest = ok & (np.arange(257) != 200)  # (ray 200's second chunk was overwritten after the duplicate was made)
    assert np.array_equal(bits(tau[ok, 4]), bits(tau[ok, 5])) and np.array_equal(bits(tau[rest, KC + 1]), bits(tau[rest, KC - 1]))
    # the outputs asked for
    same_bits(dev.query_transmittance_profile(sc, o, d, t), tr, "tr alone")
    from vr_amd import _lib as L
    rows = dev._pack_rays_numpy(o, d, np.inf)
    only_tau, only_tr = np.full_like(tau, 7.0), np.full_like(tr, 7.0)
    L.check(L.lib().vr_query_transmittance_profile(dev._h, rows.ctypes.data, L.fptr(t), t.shape[1], 257, t.shape[1], None, L.fptr(only_tau)))
    L.check(L.lib().vr_query_transmittance_profile(dev._h, rows.ctypes.data, L.fptr(t), t.shape[1], 257, t.shape[1], L.fptr(only_tr), None))
    same_bits(only_tau, tau, "tau alone")
    same_bits(only_tr, tr, "tr alone (C ABI)")


def test_unit_directions_are_used_as_they_stand():
    from vr_amd import _lib as L
    name = "250_random"
    o, d, _ = rays257(name)
    t = samples(name, KC + 1)
    dev, sc = device(), vr_scene(name)
    dev.upload(sc)
    rows = dev._pack_rays_numpy(o, R.normalized_f32(d), np.inf)
    rows[:, 7] = 1.0
    tr, tau = np.empty_like(t), np.empty_like(t)
    L.check(L.lib().vr_query_transmittance_profile(dev._h, rows.ctypes.data, L.fptr(t), t.shape[1], 257, t.shape[1], L.fptr(tr), L.fptr(tau)))
    for k in range(t.shape[1]):
        rows[:, 3] = t[:, k]
        r_tr, r_tau = np.empty(257, np.float32), np.empty(257, np.float32)
        L.check(L.lib().vr_query_transmittance(dev._h, rows.ctypes.data, 257, L.fptr(r_tr), L.fptr(r_tau)))
        same_bits(tau[:, k], r_tau, f"tau column {k}")
        same_bits(tr[:, k], r_tr, f"tr column {k}")
    rows[:, 7] = 0.0  # the rows' own tmax (the last column's sample) is not read
    tr0, tau0 = np.empty_like(t), np.empty_like(t)
    L.check(L.lib().vr_query_transmittance_profile(dev._h, rows.ctypes.data, L.fptr(t), t.shape[1], 257, t.shape[1], L.fptr(tr0), L.fptr(tau0)))
    same_bits(tau0, dev.query_transmittance_profile(sc, o, R.normalized_f32(d), t, return_tau=True)[1], "tmax field")


def test_shared_row_and_torch_input():
    import torch
    name = "250_random"
    o, d, _ = rays257(name)
    dev, sc = device(), vr_scene(name)
    row = np.sort(samples(name, 2 * KC + 3)[3])[::-1].copy()  # descending
    row[2] = NAN
    tiled = np.ascontiguousarray(np.tile(row, (257, 1)))
    tr_s, tau_s = dev.query_transmittance_profile(sc, o, d, row, return_tau=True)
    tr_t, tau_t = dev.query_transmittance_profile(sc, o, d, tiled, return_tau=True)
    assert tr_s.shape == (257, len(row))
    same_bits(tau_s, tau_t, "shared row tau")
    same_bits(tr_s, tr_t, "shared row tr")
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    for t in (row, np.ascontiguousarray(samples(name, KC + 1))):
        tr_n, tau_n = dev.query_transmittance_profile(sc, o, d, t, return_tau=True)
        tr_g, tau_g = dev.query_transmittance_profile(sc, to(o), to(d), to(t), return_tau=True)
        assert tr_g.is_cuda and tr_g.dtype == torch.float32 and tuple(tr_g.shape) == tr_n.shape
        same_bits(tau_g.cpu().numpy(), tau_n, "torch tau")
        same_bits(tr_g.cpu().numpy(), tr_n, "torch tr")
        only = dev.query_transmittance_profile(sc, to(o), to(d), to(t))
        same_bits(only.cpu().numpy(), tr_n, "torch tr alone")


# ------------------------------------------------------------------------------------------------
# 3. the tree does not matter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half_nodes,device_bvh", [(0, 0), (1, 1), (0, 1)])
def test_results_do_not_depend_on_the_tree(device_options, half_nodes, device_bvh):
    name = "1000_random"
    o, d, _ = rays257(name)
    ref_tr, ref_tau = single_reference(name)  # (on the default tree, 1 / 0)
    device_options("half_nodes", half_nodes)
    device_options("device_bvh", device_bvh)
    tr, tau = device().query_transmittance_profile(vr_scene(name), o, d, samples(name, 2 * KC + 3), return_tau=True)
    same_bits(tau, ref_tau, "tau")
    same_bits(tr, ref_tr, "tr")


# ------------------------------------------------------------------------------------------------
# 5. gradient
# ------------------------------------------------------------------------------------------------
def case_rays(name):
    if name == "1_gaussian":
        o, d, _ = one_gaussian_case()
        return o, d
    return rays257(name)[:2]


@functools.lru_cache(maxsize=None)
def grad_samples(name, K):
    if name != "1_gaussian":
        return samples(name, K)
    o, _ = case_rays(name)
    c = R.oracle_scene(name).records()[0, :3].astype(np.float64)
    reach = 2.0 * np.linalg.norm(c - o.astype(np.float64), axis=1)
    t = (np.random.default_rng(13).uniform(0, 1, (len(o), K)) * reach[:, None]).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def profile_model(name, K):
    o, d = case_rays(name)
    return PR.ProfileModel(R.oracle_scene(name), o, d, grad_samples(name, K))


@functools.lru_cache(maxsize=None)
def signed_weights(n, K):
    w = np.random.default_rng(17).uniform(-1, 1, (n, K)).astype(np.float32)
    w.setflags(write=False)
    return w


def expanded(o, d, t, w=None):
    """The n * K rays (ray i, tmax = t[i, k], weight w[i, k]), row-major."""
    K = t.shape[1]
    rep = lambda a: np.ascontiguousarray(np.repeat(a, K, axis=0))  # noqa: E731
    return rep(o), rep(d), np.ascontiguousarray(t.reshape(-1)), None if w is None else np.ascontiguousarray(w.reshape(-1))


@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("name", ["1_gaussian", "250_random", "1000_random"])
def test_gradient(name, K, moving):
    o, d = case_rays(name)
    t, w = grad_samples(name, K), signed_weights(257, K)
    mdl = profile_model(name, K)
    dev, sc = device(), vr_scene(name)
    print(f"{name} K={K}: (ray, sample, Gaussian) before / inside / past: {mdl.classes()}")
    assert all(c > 0 for c in mdl.classes()[1:])
    G, S = mdl.grad(w, moving)
    if name == "1_gaussian":  # the model (one probe per ray) is grad_reference.Model on the expanded rays (n K probes)
        G2, S2 = R.Model(R.oracle_scene(name), *expanded(o, d, t)[:3]).grad(expanded(o, d, t, w)[3], moving)
        assert np.all(np.abs(G - G2) <= 1e-13 * S2) and np.allclose(S, S2, rtol=1e-12, atol=0)
    g = dev.query_transmittance_profile_grad(sc, o, d, t, w, moving_bounds=moving)
    assert g.shape == (mdl.N, 10) and g.dtype == np.float32
    R.judge(f"{name} K={K} moving={moving} signed", g, G, S)
    eo, ed, et, ew = expanded(o, d, t, w)
    g_exp = dev.query_transmittance_grad(sc, eo, ed, ew, tmax=et, moving_bounds=moving)
    err = np.abs(g.astype(np.float64) - g_exp)
    with np.errstate(all="ignore"):
        print(f"  against the gradient query on {len(eo)} expanded rays: max |dg| / S = {np.nanmax(np.where(S > 0, err / S, 0)):.3e}")
    assert np.all(err <= 2 * R.BOUND * S)
    # weights=None is all ones
    G1, S1 = mdl.grad(None, moving)
    g_none = dev.query_transmittance_profile_grad(sc, o, d, t, None, moving_bounds=moving)
    g_ones = dev.query_transmittance_profile_grad(sc, o, d, t, np.ones((257, K), np.float32), moving_bounds=moving)
    R.judge(f"{name} K={K} moving={moving} weights=None", g_none, G1, S1)
    assert np.all(np.abs(g_none.astype(np.float64) - g_ones) <= 2 * R.BOUND * S1)


@pytest.mark.parametrize("moving", [True, False])
def test_zero_weights_and_special_samples_add_nothing(moving):
    name, K = "250_random", 5
    o, d = case_rays(name)
    t, w = grad_samples(name, K), signed_weights(257, K).copy()
    mdl = profile_model(name, K)
    dev, sc = device(), vr_scene(name)
    # a column of zero weights: the profile without that column
    w[:, 2] = 0.0
    keep = [0, 1, 3, 4]
    G, S = mdl.grad(w, moving, cols=keep)
    g0 = dev.query_transmittance_profile_grad(sc, o, d, t, w, moving_bounds=moving)
    g4 = dev.query_transmittance_profile_grad(sc, o, d, np.ascontiguousarray(t[:, keep]), np.ascontiguousarray(w[:, keep]),
                                              moving_bounds=moving)
    R.judge(f"zero column moving={moving}", g0, G, S)
    assert np.all(np.abs(g0.astype(np.float64) - g4) <= 2 * R.BOUND * S)
    # samples <= 0 or NaN in the place of that column, and two invalid rays: the same again
    t2, o2, d2 = t.copy(), o.copy(), d.copy()
    t2[:, 2] = np.resize(np.float32([0.0, -1.0, NAN, -0.0]), 257)
    w2 = signed_weights(257, K).copy()
    o2[11, 1], d2[30] = NAN, 0.0
    ok = np.setdiff1d(np.arange(257), [11, 30])
    g_sp = dev.query_transmittance_profile_grad(sc, o2, d2, t2, w2, moving_bounds=moving)
    g_ok = dev.query_transmittance_profile_grad(sc, np.ascontiguousarray(o[ok]), np.ascontiguousarray(d[ok]),
                                                np.ascontiguousarray(t[ok][:, keep]), np.ascontiguousarray(w2[ok][:, keep]),
                                                moving_bounds=moving)
    assert np.all(np.isfinite(g_sp))
    assert np.all(np.abs(g_sp.astype(np.float64) - g_ok) <= 2 * R.BOUND * S)
    # nothing but special samples: exact zeros
    t3 = np.resize(np.float32([0.0, -1.0, NAN, -0.0, -INF]), (257, K)).copy()
    g_z = dev.query_transmittance_profile_grad(sc, o, d, t3, signed_weights(257, K), moving_bounds=moving)
    assert g_z.shape == (250, 10) and not np.any(g_z)
    assert not np.any(dev.query_transmittance_profile_grad(sc, o, d, t, np.zeros((257, K), np.float32), moving_bounds=moving))


def test_gradient_of_a_shared_row_and_torch_input():
    import torch
    name, K = "250_random", 5
    o, d = case_rays(name)
    row = np.ascontiguousarray(grad_samples(name, K)[3])
    w = signed_weights(257, K)
    dev, sc = device(), vr_scene(name)
    mdl = PR.ProfileModel(R.oracle_scene(name), o, d, row)
    G, S = mdl.grad(w, True)
    g_s = dev.query_transmittance_profile_grad(sc, o, d, row, w)
    g_t = dev.query_transmittance_profile_grad(sc, o, d, np.ascontiguousarray(np.tile(row, (257, 1))), w)
    R.judge("shared row", g_s, G, S)
    assert np.all(np.abs(g_s.astype(np.float64) - g_t) <= 2 * R.BOUND * S)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    g_g = dev.query_transmittance_profile_grad(sc, to(o), to(d), to(row), to(w))
    assert g_g.is_cuda and g_g.dtype == torch.float32 and tuple(g_g.shape) == (250, 10)
    R.judge("shared row, torch", g_g.cpu().numpy(), G, S)


# ------------------------------------------------------------------------------------------------
# 4. the stack limit: the comb of wide_walk_reference.py, where redo and the take-back run
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def comb_samples(name, K):
    """(n, K) f32: column 0 is the batch's own tmax, the others U(0, 2 |comb centre - o|). default_rng(19)."""
    import wide_walk_reference as W
    from test_gpu_wide_stack import batch
    o, _, tmax, _ = batch(name)
    with np.errstate(invalid="ignore"):
        reach = 2.0 * np.linalg.norm(W.CENTRE - o.astype(np.float64), axis=1)
    reach = np.where(np.isfinite(reach), reach, 1.0)
    t = (np.random.default_rng(19).uniform(0, 1, (len(o), K)) * reach[:, None]).astype(np.float32)
    t[:, 0] = tmax
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def comb_model(name):
    from test_gpu_wide_stack import batch, oracle
    o, d, _, _ = batch(name)
    return PR.ProfileModel(oracle(), o, d, comb_samples(name, KC + 1)[:, :2])  # (the gradient's two columns of the forward's)


@pytest.mark.parametrize("config", ["wide", "pair", "host"])
@pytest.mark.parametrize("name", ["f64", "f257", "shuffled"])
def test_the_stack_limit(name, config, device_options):
    """Under "wide" every F, I and C ray overflows the 4-wide walk's stack (test_gpu_wide_stack.py shows it on the tree
    read back): the forward redoes its chunk on the pair tree, the gradient takes its first leaves' adds back first."""
    from test_gpu_wide_stack import batch, on_device
    dev, sc = on_device(device_options, config)
    o, d, tmax, names = batch(name)
    t = comb_samples(name, KC + 1)
    assert np.array_equal(bits(t[:, 0]), bits(tmax))
    tr, tau = dev.query_transmittance_profile(sc, o, d, t, return_tau=True)
    ref_tr, ref_tau = single_queries(dev, sc, o, d, t)
    same_bits(tau, ref_tau, "tau")
    same_bits(tr, ref_tr, "tr")
    assert np.all(np.isnan(tau[names == "X"])) and (tau[names == "F"] > 0).mean() > 0.5
    mdl = comb_model(name)
    t2 = np.ascontiguousarray(t[:, :2])
    w = signed_weights(len(o), 2)
    for moving in (True, False):
        G, S = mdl.grad(w, moving)
        g = dev.query_transmittance_profile_grad(sc, o, d, t2, w, moving_bounds=moving)
        R.judge(f"{config} {name} moving={moving}", g, G, S)
        eo, ed, et, ew = expanded(o, d, t2, w)
        g_exp = dev.query_transmittance_grad(sc, eo, ed, ew, tmax=et, moving_bounds=moving)
        assert np.all(np.abs(g.astype(np.float64) - g_exp) <= 2 * R.BOUND * S)


# ------------------------------------------------------------------------------------------------
# 6. errors; a frame's statistics are the frame's
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    lib = L.lib()
    name = "250_random"
    o, d, _ = rays257(name)
    K = 3
    t = np.ascontiguousarray(samples(name, K))
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    tr, tau = np.full((257, K), 7.0, np.float32), np.full((257, K), 7.0, np.float32)
    g = np.full((250, 10), 7.0, np.float32)
    big = np.ones(L.VR_PROFILE_MAX_SAMPLES + 1, np.float32)
    fwd = lambda r, ts, stride, n, k, a, b: lib.vr_query_transmittance_profile(fresh._h, r, ts, stride, n, k, a, b)  # noqa: E731
    grd = lambda r, ts, stride, w, n, k, fl, out: lib.vr_query_transmittance_profile_grad(fresh._h, r, ts, stride, w, n, k, fl, out)  # noqa: E731
    R_, T_ = rows.ctypes.data, L.fptr(t)
    assert fwd(R_, T_, K, 257, K, L.fptr(tr), L.fptr(tau)) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert fwd(R_, T_, K, 257, K, L.fptr(tr), L.fptr(tau)) == 7  # VR_ERR_UNSUPPORTED
    assert grd(R_, T_, K, None, 257, K, 0, L.fptr(g)) == 7
    fresh.upload(vr_scene(name))
    good = lambda: fwd(R_, T_, K, 257, K, L.fptr(tr), L.fptr(tau)) == 0 and grd(R_, T_, K, None, 257, K, 0, L.fptr(g)) == 0  # noqa: E731
    bad = [
        lambda: fwd(R_, T_, 0, 257, 0, L.fptr(tr), L.fptr(tau)),                                  # K = 0
        lambda: grd(R_, T_, 0, None, 257, 0, 0, L.fptr(g)),
        lambda: fwd(R_, L.fptr(big), 0, 257, len(big), L.fptr(tr), L.fptr(tau)),                  # K over the limit
        lambda: grd(R_, L.fptr(big), 0, None, 257, len(big), 0, L.fptr(g)),
        lambda: fwd(R_, T_, 1, 257, K, L.fptr(tr), L.fptr(tau)),                                  # a bad t_stride
        lambda: fwd(R_, T_, K + 1, 257, K, L.fptr(tr), L.fptr(tau)),
        lambda: grd(R_, T_, 2 * K, None, 257, K, 0, L.fptr(g)),
        lambda: fwd(R_, T_, K, 257, K, None, None),                                               # both outputs NULL
        lambda: grd(R_, T_, K, None, 257, K, 2, L.fptr(g)),                                       # unknown flags
        lambda: grd(R_, T_, K, None, 257, K, 0, None),                                            # a NULL grad
        lambda: fwd(R_, T_, 1024, 1 << 21, 1024, L.fptr(tr), L.fptr(tau)),                        # n K = 2^31
        lambda: fwd(None, T_, K, 257, K, L.fptr(tr), L.fptr(tau)),
        lambda: fwd(R_, None, K, 257, K, L.fptr(tr), L.fptr(tau)),
    ]
    for i, call in enumerate(bad):
        assert call() == 1, i  # VR_ERR_INVALID
        assert np.all(tr == 7.0) and np.all(tau == 7.0) and np.all(g == 7.0), i
        assert good(), i
        ref = (tr.copy(), tau.copy(), g.copy()) if i == 0 else ref
        same_bits(tr, ref[0], i)
        same_bits(tau, ref[1], i)
        tr[:], tau[:], g[:] = 7.0, 7.0, 7.0
    assert fwd(None, None, 0, 0, K, L.fptr(tr), L.fptr(tau)) == 0 and np.all(tr == 7.0)  # n == 0 touches nothing
    assert grd(None, None, 0, None, 0, K, 0, L.fptr(g)) == 0 and not np.any(g)           # ... and zeroes grad
    buf = torch.zeros(257 * 8 + 4, dtype=torch.float32, device="cuda")
    dt, out = torch.ones(K, device="cuda"), torch.full((257, K), 7.0, device="cuda")
    dg = torch.full((250, 10), 7.0, device="cuda")
    assert lib.vr_query_transmittance_profile_device(fresh._h, buf.data_ptr() + 4, dt.data_ptr(), 0, 257, K, out.data_ptr(), None, None) == 1
    assert lib.vr_query_transmittance_profile_grad_device(fresh._h, buf.data_ptr() + 4, dt.data_ptr(), 0, None, 257, K, 0, dg.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert bool(torch.all(out == 7.0)) and bool(torch.all(dg == 7.0))


def test_profile_queries_leave_the_last_frame_alone():
    import torch
    import vr_amd as vr
    sc = vr_scene("many_gaussians")
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), env_samples=8)
    img = vr.Image(48, 48)
    integ.render(sc, img)
    dev = device()
    before = dev.stats()
    first = img.pixels.copy()
    o = np.tile(CAM_POS, (63, 1)).astype(np.float32)
    d = (np.random.default_rng(7).uniform(-0.5, 0.5, (63, 3)) + [0, 0, -3]).astype(np.float32)
    t = np.linspace(1.0, 12.0, 5, dtype=np.float32)
    assert np.any(dev.query_transmittance_profile(sc, o, d, t) < 1.0)
    assert np.any(dev.query_transmittance_profile_grad(sc, o, d, t) != 0)
    to = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dev.query_transmittance_profile(sc, to(o), to(d), to(t))
    dev.query_transmittance_profile_grad(sc, to(o), to(d), to(t))
    dev.synchronize()
    assert dev.stats() == before
    integ.render(sc, img)
    assert np.array_equal(img.pixels.view(np.uint32), first.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# 7. torch autograd, the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_autograd_profile():
    import torch
    import vr_amd as vr
    from vr_amd import autograd
    theta, _, o, d, _ = R.descent_case()  # 8 Gaussians, 64 rays
    K = 4
    o, d = o.astype(np.float32), d.astype(np.float32)
    t = (np.random.default_rng(23).uniform(0.5, 8.0, (64, K))).astype(np.float32)
    Gw = np.random.default_rng(29).uniform(-1, 1, (64, K)).astype(np.float32)
    th = theta.astype(np.float32)
    alb = np.full(8, 0.5, np.float32)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    dev = device()
    sc = vr.Scene.from_gaussians(th[:, 0:3], th[:, 3:9], th[:, 9], alb)
    _, tau_q = dev.query_transmittance_profile(sc, o, d, t, return_tau=True)
    g_q = dev.query_transmittance_profile_grad(sc, o, d, t, Gw)
    mdl = PR.ProfileModel(R.oracle_from_gaussians(th[:, 0:3], th[:, 3:9], th[:, 9], alb), o, d, t)
    G, S = mdl.grad(Gw, True)
    R.judge("8 Gaussians, the query", g_q, G, S)
    got = {}
    for fn in (autograd.optical_depth_profile, autograd.optical_depth_profile_resident):
        mean, cov6, dens = (to(th[:, 0:3]).requires_grad_(), to(th[:, 3:9]).requires_grad_(), to(th[:, 9]).requires_grad_())
        ro, rt = to(o).requires_grad_(), to(t).requires_grad_()
        tau = fn(mean, cov6, dens, to(alb), ro, to(d), rt)
        assert tau.requires_grad and tuple(tau.shape) == (64, K)
        (tau * to(Gw)).sum().backward()
        assert ro.grad is None and rt.grad is None
        got[fn.__name__] = (tau.detach().cpu().numpy(), torch.cat([mean.grad, cov6.grad, dens.grad[:, None]], 1).cpu().numpy())
    tau_h, g_h = got["optical_depth_profile"]
    tau_r, g_r = got["optical_depth_profile_resident"]
    same_bits(tau_h, tau_q, "optical_depth_profile forward")
    R.judge("optical_depth_profile backward", g_h, G, S)
    assert np.all(np.abs(g_h.astype(np.float64) - g_q) <= 2 * R.BOUND * S)
    # the resident form, under the rule test_gpu_upload_device.py applies to optical_depth_resident: where no record's norm
    # differs between the host's and the device's upload (shown on the CPU), the same tau bit for bit and a gradient
    # under the model's bound and within twice that of the host form's
    import upload_device_reference as U
    host_norm = sc.records()[:, 10]
    assert np.array_equal(bits(host_norm), bits(U.device_norm(np.ascontiguousarray(th[:, 3:9]))))
    same_bits(tau_r, tau_h, "optical_depth_profile_resident forward")
    R.judge("optical_depth_profile_resident backward", g_r, G, S)
    assert np.all(np.abs(g_r.astype(np.float64) - g_h) <= 2 * R.BOUND * S)


def test_cpp_mirror_matches(tmp_path):
    name, K = "250_random", KC + 1
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d, tmax = sphere_rays(name)
    path = tmp_path / "rays.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 256, 0))
        f.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-profile", str(path), str(K)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("tp ")]
    assert [(int(x[1]), int(x[2])) for x in rows] == [(i, k) for i in range(256) for k in range(K)]
    words = np.array([[int(h, 16) for h in x[3:]] for x in rows], np.uint32).reshape(256, K, 3)
    t = (tmax[:, None] * np.arange(1, K + 1, dtype=np.float32)[None]) / np.float32(K)
    assert t.dtype == np.float32 and np.array_equal(words[..., 0], bits(t))
    tr, tau = device().query_transmittance_profile(vr_scene(name), o, d, np.ascontiguousarray(t), return_tau=True)
    assert np.array_equal(words[..., 1], bits(tr)) and np.array_equal(words[..., 2], bits(tau))
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("pg ")]
    assert [int(x[1]) for x in lines] == list(range(250)) and all(len(x) == 12 for x in lines)
    g = np.array([[int(h, 16) for h in x[2:]] for x in lines], np.uint32).view(np.float32)
    G, S = PR.ProfileModel(R.oracle_scene(name), o, d, t).grad(None, True)
    R.judge("C++ mirror (--query-profile)", g, G, S)
