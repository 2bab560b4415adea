"""The radiance query (Device.radiance over vr_query_radiance[_device], autograd.radiance[_resident],
MixtureQuery::radiance) on the device.

Against the device's own composition: query_transmittance_profile x evaluate_features at the numpy-computed f32 points
x = o + t * d, summed in float64. tr has the profile's bits, the pair counts are the summed n_active exactly, and
|out - comp| <= 2^-22 S per entry with exact +0 where S = 0, S = sum_k |q| T F_abs, F_abs the feature query on |f|: one
f32 multiply per term and the rounding of F on the composition's side and the final rounding on the query's cost at
most 2^-24 S each, three in all, and the bound allows four.

Against the float64 model of tests/radiance_reference.py: |dev - model| <= RAD_RTOL * S. RAD_RTOL is 4 x the largest such
ratio measured on an MI355X over the cases of radiance_reference.CASES, the protocol of SIGMA_RTOL and FEAT_RTOL. The
model's T is the oracle's (the reference's own f32 optical depth, which the profile reproduces), so the error is the f32
mu_t against float64 and the device's erff / expf against the model's. Measured: MEASURED below. With the float64 closed
form for T as well the same ratio is MEASURED_T64 (printed by the test, not asserted): that is the distance of the
reference's f32 optical depth from float64 (radiance_reference.py's head), above the 1e-4 cap by itself. Every test prints
its measured maximum before it asserts.

The chord-end and elongated cases go against the composition alone: their samples sit on the cut-off by construction
(the float64 model's exclusion would zero them all), and at a condition number of 10^4 no float64 model is a fair
reference for f32 decisions (tests/aniso_cases.py).
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import features_reference as FR
import grad_reference as GR
import profile_reference as PR
import radiance_reference as RR
import sigma_grad_reference as SR
from helpers import ROOT, scene_path

pytestmark = pytest.mark.gpu

# Largest |dev - model| / S measured on an MI355X per case (L and opacity together).
MEASURED = "1_gaussian K=1 5.7e-7, K=17 3.5e-7 (the same at C = 1 and 3), 50_random 1.39e-6 (the largest), 250_random 9.6e-7"
MEASURED_T64 = "1_gaussian K=1 1.29e-4, K=17 1.59e-4, 50_random 1.04e-3, 250_random 1.55e-3 (|Tr - T64| / T64 up to 8.0e-3)"
RAD_RTOL = 5.6e-6  # 4 x 1.39e-6
NAN, INF = np.float32(np.nan), np.float32(np.inf)


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


def run(dev, sc, o, d, t, f, q, **kw):
    """(L, opacity, tr, pairs) of Device.radiance."""
    return dev.radiance(sc, o, d, t, f, q, return_opacity=True, return_tr=True, return_pairs=True, **kw)


def composition(dev, sc, o, d, t, f, q, unit=False):
    """The same quantities from the profile query and the feature query at the f32 points, summed in float64, and S."""
    n = len(o)
    t2 = np.ascontiguousarray(np.broadcast_to(t, (n, t.shape[-1])))
    K = t2.shape[1]
    q2 = np.ones((n, K)) if q is None else np.broadcast_to(q, (n, K)).astype(np.float64)
    tr = dev.query_transmittance_profile(sc, o, d, t2)
    dn = np.ascontiguousarray(d, np.float32) if unit else GR.normalized_f32(d)
    valid = RR.valid_samples(t2)
    x = np.where(valid[..., None], RR.points_f32(o, dn, t2), NAN).reshape(-1, 3)  # (a NaN point lies in no box)
    x = np.ascontiguousarray(x, np.float32)
    F, mass, act = dev.evaluate_features(sc, x, f, return_mass=True, return_active=True)
    F_abs = dev.evaluate_features(sc, x, np.abs(f))
    with np.errstate(invalid="ignore"):
        w = np.where(valid, q2 * tr.astype(np.float64), 0.0)
    C = f.shape[1]
    L = np.einsum("nk,nkc->nc", w, F.reshape(n, K, C).astype(np.float64))
    S = np.einsum("nk,nkc->nc", np.abs(w), F_abs.reshape(n, K, C).astype(np.float64))
    m = mass.reshape(n, K).astype(np.float64)
    return dict(L=L, S=S, op=(w * m).sum(1), S_op=(np.abs(w) * m).sum(1), tr=tr, pairs=act.reshape(n, K).sum(1))


def judge(label, got, comp, bound=2.0 ** -22, rows=None):
    """Prints the measured maxima, then asserts tr's bits, the pair counts, the bound and the exact zeros."""
    L, op, tr, pairs = got
    rows = np.ones(len(L), bool) if rows is None else rows
    assert L.dtype == op.dtype == tr.dtype == np.float32
    assert np.array_equal(bits(tr), bits(comp["tr"])), np.argwhere(bits(tr) != bits(comp["tr"]))[:5].tolist()
    assert np.array_equal(pairs[rows], comp["pairs"][rows]), np.argwhere(pairs != comp["pairs"])[:5].tolist()
    worst = 0.0
    for what, dev, ref, S in (("L", L[rows], comp["L"][rows], comp["S"][rows]), ("opacity", op[rows], comp["op"][rows], comp["S_op"][rows])):
        assert dev.shape == ref.shape, (dev.shape, ref.shape)
        err = np.abs(dev.astype(np.float64) - ref)
        with np.errstate(all="ignore"):
            rel = np.where(S > 0, err / S, 0.0)
        print(f"{label} {what}: max |dev - ref| / S = {rel.max() if rel.size else 0.0:.3e} (bound {bound:.3e}), entries with S = 0: "
              f"{int((S == 0).sum())}, pairs {int(pairs[rows].sum())}")
        assert np.all(np.isfinite(dev)) and not np.any(bits(dev)[S == 0])
        assert np.all(err <= bound * S), float(rel.max())
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
    return worst


def case_inputs(name, n, K, C):
    o, d = RR.case_rays(name, n)
    mdl = RR.model(name, n, K, C)
    return o, d, np.ascontiguousarray(mdl.t), mdl.f, mdl.weights, mdl


def ties(dev, sc, o, d, t, f, q, got):
    """The definition's exact properties on one case: the ones channel, C and place, layouts, numpy and torch."""
    L, op, tr, pairs = got
    n, C = L.shape
    assert np.array_equal(bits(L[:, 1]), bits(op))  # channel 1 is all 1.0f
    col = np.ascontiguousarray(f[:, 10:11])
    alone, op1 = dev.radiance(sc, o, d, t, col, q, return_opacity=True)
    assert alone.shape == (n, 1) and np.array_equal(bits(alone[:, 0]), bits(L[:, 10])) and np.array_equal(bits(op1), bits(op))
    for Cx, at in ((8, 7), (9, 8), (9, 0)):
        fx = np.array(RR.features_of(len(f), Cx, seed=Cx))
        fx[:, at] = col[:, 0]
        one, opx, prx = dev.radiance(sc, o, d, t, fx, q, return_opacity=True, return_pairs=True)
        assert np.array_equal(bits(one[:, at]), bits(L[:, 10])) and np.array_equal(bits(opx), bits(op)), (Cx, at)
        assert np.array_equal(prx, pairs)
    # a shared row against the same row per ray, for t and for q
    row_t, row_q = np.ascontiguousarray(t[3]), np.ascontiguousarray(q[5])
    a = run(dev, sc, o, d, row_t, f, row_q)
    b = run(dev, sc, o, d, np.ascontiguousarray(np.tile(row_t, (n, 1))), f, np.ascontiguousarray(np.tile(row_q, (n, 1))))
    c = run(dev, sc, o, d, row_t, f, np.ascontiguousarray(np.tile(row_q, (n, 1))))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
    assert a[3].sum() > 0
    # q = None is ones
    a = run(dev, sc, o, d, t, f, None)
    b = run(dev, sc, o, d, t, f, np.ones_like(t))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # numpy and torch forms; only what is asked for
    g = run(dev, sc, to_cuda(o), to_cuda(d), to_cuda(t), to_cuda(f), to_cuda(q))
    assert all(v.is_cuda for v in g) and tuple(g[0].shape) == (n, C) and tuple(g[2].shape) == t.shape
    for x, y in zip(g, got):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))
    only = dev.radiance(sc, to_cuda(o), to_cuda(d), to_cuda(row_t), to_cuda(f), to_cuda(row_q))
    assert np.array_equal(bits(only.cpu().numpy()), bits(c[0]))
    assert np.array_equal(bits(dev.radiance(sc, o, d, t, f, q)), bits(L))


# ------------------------------------------------------------------------------------------------
# 1. against the device's own composition, 4. against the float64 model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,K,C", RR.CASES, ids=[f"{c[0]}-K{c[2]}-C{c[3]}" for c in RR.CASES])
def test_against_the_composition_and_the_model(name, n, K, C):
    o, d, t, f, q, mdl = case_inputs(name, n, K, C)
    dev, sc = device(), vr_scene(name)
    got = run(dev, sc, o, d, t, f, q)
    assert got[0].shape == (n, C) and got[1].shape == (n,) and got[2].shape == (n, K) and got[3].shape == (n,)
    comp = composition(dev, sc, o, d, t, f, q)
    print(f"{name} n={n} K={K} C={C}: {mdl.near.sum()} samples zeroed ({mdl.zeroed:.2%}), rows without a pair {int((got[3] == 0).sum())}")
    judge(f"{name} K={K} C={C} composition", got, comp)
    assert np.array_equal(got[3], mdl.pairs.sum(1))  # (the model's own count: its zeroed samples are counted on both sides)
    if C >= 19:
        assert (got[3] == 0).any() and got[3].max() > 1
        ties(dev, sc, o, d, t, f, q, got)
    # the float64 model
    worst = judge(f"{name} K={K} C={C} float64 model", got,
                  dict(L=mdl.L, S=mdl.S, op=mdl.opacity, S_op=mdl.S_op, tr=got[2], pairs=got[3]), bound=RAD_RTOL or np.inf)
    print(f"{name} K={K} C={C}: measured max |dev - model| / S = {worst:.3e}")
    assert RAD_RTOL is not None and RAD_RTOL <= 1e-4
    with np.errstate(all="ignore"):
        r64 = max(np.nanmax(np.where(mdl.S > 0, np.abs(got[0] - mdl.L64) / mdl.S, 0)),
                  np.nanmax(np.where(mdl.S_op > 0, np.abs(got[1] - mdl.opacity64) / mdl.S_op, 0)))
        print(f"  with the float64 closed form for T as well: max |dev - model| / S = {r64:.3e}; max |Tr - T| / T = "
              f"{np.nanmax(np.abs(got[2] - mdl.T) / mdl.T):.3e} (the oracle's), {np.nanmax(np.abs(got[2] - mdl.T64) / mdl.T64):.3e} (float64)")


# ------------------------------------------------------------------------------------------------
# 2. chord ends: samples at t_enter, t_exit and their f32 neighbours, and t = 0 for origins inside
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chord_case():
    name = "50_random"
    sc = GR.oracle_scene(name)
    o, d = (np.array(a[:256]) for a in RR.case_rays(name, 1024))
    rec = SR.records_of_oracle(sc.records())
    centre = rec[0][np.arange(0, 50, 7)]  # eight rays start inside a Gaussian
    o[:8] = (centre + 0.01).astype(np.float32)
    hit, te, tx = GR.probe(sc, o, d)
    K = 64
    t = np.full((256, K), NAN, np.float32)
    for i in range(256):
        ends = np.concatenate([te[i][hit[i]], tx[i][hit[i]]]).astype(np.float32)
        s = np.unique(np.concatenate([np.nextafter(ends, -INF), ends, np.nextafter(ends, INF)]))
        if SR.Model(rec, o[i:i + 1]).n_active[0] > 0:
            s = np.concatenate([np.float32([0.0]), s])
        t[i, :min(K, len(s))] = s[:K]
    q = np.random.default_rng(29).uniform(-1, 1, t.shape).astype(np.float32)
    return name, o, d, t, q


def test_chord_ends():
    name, o, d, t, q = chord_case()
    f = RR.features_of(50, 19)
    dev, sc = device(), vr_scene(name)
    got = run(dev, sc, o, d, t, f, q)
    comp = composition(dev, sc, o, d, t, f, q)
    valid = RR.valid_samples(t)
    print(f"chord ends: {int(valid.sum())} samples on {int(valid.any(1).sum())} rays, {int((t == 0).sum())} at t = 0, pairs {int(got[3].sum())}")
    assert valid.sum() >= 2000 and (t[:8, 0] == 0).all() and got[3][:8].min() >= 1
    judge("chord ends", got, comp)


# ------------------------------------------------------------------------------------------------
# 3. elongated Gaussians: the ladder's largest condition number (ratio^2 = 10^4)
# ------------------------------------------------------------------------------------------------
def test_elongated_gaussians():
    import aniso_cases as AC
    key = ("disc", 100)
    assert key[1] == max(r for _, r in AC.LADDER)
    o, d, _ = AC.aimed_rays(*key, n=256)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    dist = np.linalg.norm(d.astype(np.float64), axis=1)
    rng = np.random.default_rng(31)
    K = 33
    t = (rng.uniform(0, 2, (256, K)) * dist[:, None]).astype(np.float32)
    t[:, 0] = dist.astype(np.float32)  # the aimed target itself
    q = rng.uniform(-1, 1, t.shape).astype(np.float32)
    N = len(AC.gaussians(*key).mean)
    f = RR.features_of(N, 19)
    dev, sc = device(), AC.device_scene(*key)
    got = run(dev, sc, o, d, t, f, q)
    comp = composition(dev, sc, o, d, t, f, q)
    assert got[3].sum() >= 256
    judge("disc 100", got, comp)


# ------------------------------------------------------------------------------------------------
# 5. 65 537 rays: 256 blocks and one lane
# ------------------------------------------------------------------------------------------------
def test_65537_rays():
    name, n, K, C = "50_random", 65537, 4, 3
    o, d = RR.case_rays(name, n)
    t, q = RR.case_samples(name, n, K)
    f = RR.features_of(50, C)
    dev, sc = device(), vr_scene(name)
    got = run(dev, sc, o, d, t, f, q)
    judge("50_random x 65537", got, composition(dev, sc, o, d, t, f, q))
    assert np.array_equal(bits(got[0][:, 1]), bits(got[1]))


# ------------------------------------------------------------------------------------------------
# 6. tree options
# ------------------------------------------------------------------------------------------------
def test_tree_options_change_nothing_beyond_rounding():
    import vr_amd as vr
    name, n, K, C = "250_random", 1024, 33, 19
    o, d, t, f, q, mdl = case_inputs(name, n, K, C)
    dev = vr.Device(0)
    out = {}
    for half in (0, 1):
        for dbvh in (0, 1):
            dev.set_option("half_nodes", half)
            dev.set_option("device_bvh", dbvh)
            out[half, dbvh] = run(dev, vr_scene(name), o, d, t, f, q)
            if (half, dbvh) == (0, 0):
                comp = composition(dev, vr_scene(name), o, d, t, f, q)
            judge(f"250_random half_nodes={half} device_bvh={dbvh}", out[half, dbvh], comp)
    for key, got in out.items():
        ref = out[1, 0]
        assert np.array_equal(bits(got[2]), bits(ref[2])) and np.array_equal(got[3], ref[3])
        assert np.all(np.abs(got[0].astype(np.float64) - ref[0]) <= 2.0 ** -23 * comp["S"])
        assert np.all(np.abs(got[1].astype(np.float64) - ref[1]) <= 2.0 ** -23 * comp["S_op"])


# ------------------------------------------------------------------------------------------------
# 7. the redo path: the comb of wide_walk_reference.py, where 4-wide ray walks break off
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["wide", "host"])
@pytest.mark.parametrize("name", ["f257", "shuffled"])
def test_the_stack_limit(name, config, device_options):
    """Under "wide" (the device builder's 4-wide tree) every F, I and C ray's walk reaches the stack limit and the whole
    ray is walked again on the child-pair tree after a reset; under "host" the simulators print what the rays do and
    nothing is assumed. Both must equal the composition, whose point walks have their own redo."""
    from test_gpu_query_profile import comb_samples
    from test_gpu_wide_stack import batch, on_device, oracle
    dev, sc = on_device(device_options, config)
    o, d, _, names = batch(name)
    K = 9
    t = np.ascontiguousarray(comb_samples(name, 17)[:, :K])
    q = np.random.default_rng(37).uniform(-1, 1, t.shape).astype(np.float32)
    f = RR.features_of(oracle().num, 11)
    ok = names != "X"
    got = run(dev, sc, o, d, t, f, q)
    comp = composition(dev, sc, o, d, t, f, q)
    assert got[3][names == "F"].sum() > 0
    judge(f"comb {name} {config}", got, comp, rows=ok)
    bad = ~ok
    assert np.all(np.isnan(got[0][bad])) and np.all(np.isnan(got[1][bad])) and np.all(np.isnan(got[2][bad])) and not got[3][bad].any()


# ------------------------------------------------------------------------------------------------
# 8. inputs that contribute nothing
# ------------------------------------------------------------------------------------------------
def test_inputs_that_contribute_nothing():
    import vr_amd as vr
    name, n, K, C = "50_random", 1024, 33, 19
    o, d, t, f, q, mdl = case_inputs(name, n, K, C)
    o, t, q = np.array(o[:64]), np.array(t[:64]), np.array(q[:64])
    d = np.ascontiguousarray(d[:64])
    dev, sc = device(), vr_scene(name)
    base = run(dev, sc, o, d, t, f, q)
    # special samples in three columns: what is left is the query without them; tr keeps the profile's value
    cols = [c for c in range(K) if c not in (4, 9, 20)]
    t2, q2 = t.copy(), q.copy()
    t2[:, 4], t2[:, 9], t2[:, 20] = -1.0, NAN, INF
    t2[1, 4] = -INF
    q2[:, 9] = INF
    got = run(dev, sc, o, d, t2, f, q2)
    rest = run(dev, sc, o, d, np.ascontiguousarray(t[:, cols]), f, np.ascontiguousarray(q[:, cols]))
    for a, b in ((got[0], rest[0]), (got[1], rest[1]), (got[3], rest[3]), (got[2][:, cols], rest[2])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(bits(got[2]), bits(dev.query_transmittance_profile(sc, o, d, t2)))
    assert np.all(got[2][:, 4] == 1.0) and np.all(got[2][:, 9] == 1.0)
    # q = inf on samples in no ellipsoid leaves the rows finite
    comp = composition(dev, sc, o, d, t, f, q)
    x = RR.points_f32(o, GR.normalized_f32(d), t).reshape(-1, 3)
    act = dev.evaluate_features(sc, np.ascontiguousarray(x), f, return_active=True)[1].reshape(t.shape)
    assert (act == 0).sum() > 100
    q3 = np.where(act == 0, INF, q).astype(np.float32)
    got = run(dev, sc, o, d, t, f, q3)
    for a, b in zip(got, base):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a row with nothing but special samples: +0, no pairs, and no walk
    t4 = t.copy()
    t4[7] = np.resize(np.float32([-1.0, NAN, INF, -INF]), K)
    got = run(dev, sc, o, d, t4, f, q)
    assert not np.any(bits(got[0][7])) and not bits(got[1])[7] and got[3][7] == 0
    keep = np.arange(64) != 7
    assert np.array_equal(bits(got[0][keep]), bits(base[0][keep]))
    # invalid rays: NaN rows and 0 pairs
    o5, d5 = o.copy(), np.array(d)
    o5[11, 1], d5[30] = NAN, 0.0
    got = run(dev, sc, o5, d5, t, f, q)
    for r in (11, 30):
        assert np.all(np.isnan(got[0][r])) and np.isnan(got[1][r]) and np.all(np.isnan(got[2][r])) and got[3][r] == 0
    keep = ~np.isin(np.arange(64), (11, 30))
    for a, b in zip(got, base):
        assert np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32))
    # n = 0; an empty scene gives zeros and tr = 1
    none = run(dev, sc, o[:0], d[:0], t[:0], f, q[:0])
    assert [a.shape for a in none] == [(0, C), (0,), (0, K), (0,)]
    hollow = vr.Scene.from_gaussians(np.zeros((0, 3)), np.zeros((0, 6)), [], [], [vr.Light([0, 1, 0], [1, 1, 1])])
    fresh = vr.Device(0)
    for kind in (lambda v: v, to_cuda):
        got = run(fresh, hollow, kind(o), kind(d), kind(t), kind(np.zeros((0, C), np.float32)), kind(q))
        got = [a.cpu().numpy() if hasattr(a, "cpu") else a for a in got]
        assert not np.any(bits(got[0])) and not np.any(bits(got[1])) and np.all(got[2] == 1.0) and not np.any(got[3])


# ------------------------------------------------------------------------------------------------
# 9. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    lib = L.lib()
    name, K, C = "250_random", 3, 3
    o, d = (np.ascontiguousarray(a[:257]) for a in RR.case_rays(name, 1024))
    t, q = (np.ascontiguousarray(a[:257]) for a in RR.case_samples(name, 1024, K))
    f = RR.features_of(250, C)
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    out, op, tr = np.full((257, C), 7.0, np.float32), np.full(257, 7.0, np.float32), np.full((257, K), 7.0, np.float32)
    prs = np.full(257, 7, np.uint32)
    big = np.ones(L.VR_PROFILE_MAX_SAMPLES + 1, np.float32)
    P, up = L.fptr, lambda a: a.ctypes.data_as(L.U32P)  # noqa: E731
    R_ = rows.ctypes.data

    def call(r=R_, ts=P(t), ts_stride=K, qs=P(q), qs_stride=K, n=257, k=K, ft=P(f), c=C, o_=P(out)):
        return lib.vr_query_radiance(fresh._h, r, ts, ts_stride, qs, qs_stride, n, k, ft, c, o_, P(op), P(tr), up(prs))

    assert call() == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call() == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene(name))
    bad = [dict(k=0, ts_stride=0, qs_stride=0), dict(ts=P(big), ts_stride=0, qs=None, qs_stride=0, k=len(big)),  # K
           dict(c=0), dict(c=65),                                                                                  # C
           dict(ts_stride=1), dict(ts_stride=K + 1), dict(qs_stride=1), dict(qs_stride=2 * K),                     # strides
           dict(r=None), dict(ts=None), dict(ft=None), dict(o_=None),                                              # NULL
           dict(n=1 << 31), dict(n=1 << 30, k=2, ts_stride=2, qs_stride=2), dict(n=1 << 30, k=1, ts_stride=1, qs_stride=1, c=2)]
    for i, kw in enumerate(bad):
        assert call(**kw) == 1, (i, kw)  # VR_ERR_INVALID
        assert np.all(out == 7.0) and np.all(op == 7.0) and np.all(tr == 7.0) and np.all(prs == 7), (i, kw)
    assert call(n=0) == 0 and call(r=None, ts=None, qs=None, ft=None, o_=None, n=0) == 0  # n == 0 touches nothing
    assert np.all(out == 7.0) and np.all(op == 7.0) and np.all(tr == 7.0) and np.all(prs == 7)
    assert call(qs=None, qs_stride=99) == 0  # (no q: its stride is not read)
    ones = run(device(), vr_scene(name), o, d, t, f, None)
    assert np.array_equal(bits(out), bits(ones[0])) and np.array_equal(bits(tr), bits(ones[2])) and np.array_equal(prs, ones[3])
    assert call() == 0
    ref = run(device(), vr_scene(name), o, d, t, f, q)
    assert np.array_equal(bits(out), bits(ref[0])) and np.array_equal(bits(op), bits(ref[1])) and np.array_equal(prs, ref[3])
    # the _device form with torch pointers
    buf = torch.zeros(257 * 8 + 4, dtype=torch.float32, device="cuda")
    dt, dq, df = to_cuda(t), to_cuda(q), to_cuda(f)
    o_t = torch.full((257, C), 7.0, device="cuda")
    dcall = lambda r, ts, stride, ft, c, dst: lib.vr_query_radiance_device(  # noqa: E731
        fresh._h, r, ts, stride, dq.data_ptr(), K, 257, K, ft, c, dst, None, None, None, None)
    assert dcall(buf.data_ptr() + 4, dt.data_ptr(), K, df.data_ptr(), C, o_t.data_ptr()) == 1  # a misaligned ray array
    assert dcall(buf.data_ptr(), dt.data_ptr(), K + 1, df.data_ptr(), C, o_t.data_ptr()) == 1
    assert dcall(buf.data_ptr(), None, K, df.data_ptr(), C, o_t.data_ptr()) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, None, C, o_t.data_ptr()) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, df.data_ptr(), 65, o_t.data_ptr()) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, df.data_ptr(), C, None) == 1
    torch.cuda.synchronize()
    assert bool(torch.all(o_t == 7.0))
    rays_t = to_cuda(rows)
    assert dcall(rays_t.data_ptr(), dt.data_ptr(), K, df.data_ptr(), C, o_t.data_ptr()) == 0  # (tr == NULL: the workspace)
    torch.cuda.synchronize()
    assert np.array_equal(bits(o_t.cpu().numpy()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------
# 10. torch autograd
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def autograd_case():
    """Axis-parallel rays through 50_random (their directions are unit vectors whose normalisation changes nothing, so
    the library, torch and the oracle walk the same lines), K = 5 samples, C = 3, signed weights and output gradients."""
    name, n, K, C = "50_random", 192, 5, 3
    sc = GR.oracle_scene(name)
    m = sc.records()[:, :3].astype(np.float64)
    lo, hi = m.min(0), m.max(0)
    rng = np.random.default_rng(41)
    o = rng.uniform(lo, hi, (n, 3))
    d = np.zeros((n, 3))
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    d[np.arange(n), axis] = sign
    o[np.arange(n), axis] = np.where(sign > 0, lo[axis] - 1.0, hi[axis] + 1.0)
    o, d = o.astype(np.float32), d.astype(np.float32)
    reach = (hi - lo)[axis] + 2.0
    t = (rng.uniform(0, 1, (n, K)) * reach[:, None]).astype(np.float32)
    q = (rng.uniform(-1, 1, (n, K)) * (reach / K)[:, None]).astype(np.float32)
    f = RR.features_of(sc.num, C)
    mdl = RR.RadianceModel(sc, o, d, t, q, f)
    gL, gA = FR.signed_weights(n, C)
    return name, o, d, t, mdl.weights, f, mdl, gL, gA


def radiance_backward(fn, gs, f, o, d, t, q, gL, gA, needs=(0, 1, 2, 4), param_device="cuda"):
    import torch
    to = lambda a, dev_="cuda": torch.from_numpy(np.array(a)).to(dev_)  # noqa: E731
    p = [to(a, param_device) for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10], f)]
    for k in needs:
        p[k].requires_grad_()
    ro, rt, rq = to(o).requires_grad_(), to(t).requires_grad_(), to(q).requires_grad_()
    L, op = fn(*p, ro, to(d), rt, rq)
    assert tuple(L.shape) == (len(o), f.shape[1]) and tuple(op.shape) == (len(o),) and L.dtype == torch.float32
    ((L * to(gL)).sum() + (op * to(gA)).sum()).backward()
    assert p[3].grad is None and ro.grad is None and rt.grad is None and rq.grad is None
    return L.detach().cpu().numpy(), op.detach().cpu().numpy(), p


def test_autograd_forward_and_backward(monkeypatch):
    import torch
    import vr_amd as vr
    from vr_amd import autograd
    name, o, d, t, q, f, mdl, gL, gA = autograd_case()
    n, K = t.shape
    C = f.shape[1]
    gs = vr_scene(name).gaussians()
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    calls = []
    for meth in ("features_gradient", "evaluate_features", "query_transmittance_profile_grad", "radiance"):
        def counting(self, *a, _real=getattr(vr.Device, meth), _name=meth, **kw):
            calls.append((_name, bool(kw.get("gaussians", True)), bool(kw.get("features_grad", True))) if _name == "features_gradient" else _name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(vr.Device, meth, counting)
    L, op, p = radiance_backward(autograd.radiance, gs, f, o, d, t, q, gL, gA)
    assert calls == ["radiance", ("features_gradient", True, True), "evaluate_features", "query_transmittance_profile_grad"], calls
    # the forward has the bits of Device.radiance for the same unit directions (here: the directions themselves)
    assert np.array_equal(d, autograd._unit_directions(to_cuda(d)).cpu().numpy())
    L_q, op_q, tr_q = dev.radiance(sc, o, d, t, f, q, unit=True, return_opacity=True, return_tr=True)
    assert np.array_equal(bits(L), bits(L_q)) and np.array_equal(bits(op), bits(op_q))
    assert np.array_equal(bits(L_q), bits(dev.radiance(sc, o, d, t, f, q)))  # (unit or not: the same rays)
    # the backward against the two float64 gradient models, fed the weights formed in float64 from the device's T and F
    x = np.ascontiguousarray(RR.points_f32(o, d, t).reshape(-1, 3))
    F_d, mass_d = dev.evaluate_features(sc, x, f, return_mass=True)
    qt = q.astype(np.float64) * tr_q.astype(np.float64)
    w = (qt[:, :, None] * gL.astype(np.float64)[:, None, :]).reshape(-1, C)
    u = (qt * gA.astype(np.float64)[:, None]).reshape(-1)
    s = (F_d.reshape(n, K, C).astype(np.float64) * gL.astype(np.float64)[:, None, :]).sum(2) + mass_d.reshape(n, K).astype(np.float64) * gA[:, None]
    rec = SR.records_of_oracle(GR.oracle_scene(name).records())
    pts = SR.Model(rec, x)
    assert np.array_equal(pts.near.reshape(n, K), mdl.near) and not np.any(qt[mdl.near])  # (samples on a cut-off weigh 0)
    (Gf, Sf), (Gr, Sr), _ = FR.FeatureModel(pts, f).grads(w, u)
    Gp, Sp = PR.ProfileModel(GR.oracle_scene(name), o, d, t).grad(-qt * s, True)
    got = torch.cat([p[0].grad, p[1].grad, p[2].grad[:, None]], 1).cpu().numpy()
    assert got.dtype == np.float32 and (Sf > 0).any() and (Sp > 0).any()
    bound = (SR.BOUND + 2.0 ** -23) * Sf + (GR.BOUND + 2.0 ** -23) * Sp
    err = np.abs(got.astype(np.float64) - (Gf + Gp))
    with np.errstate(all="ignore"):
        print(f"autograd.radiance backward: max |dev - model| / (S_features + S_profile) = {np.nanmax(np.where(Sf + Sp > 0, err / (Sf + Sp), 0)):.3e}, "
              f"max |model| = {np.abs(Gf + Gp).max():.3e}, feature part {np.abs(Gf).max():.3e}, profile part {np.abs(Gp).max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    gfe = p[4].grad.cpu().numpy()
    errf = np.abs(gfe.astype(np.float64) - Gr)
    with np.errstate(all="ignore"):
        print(f"autograd.radiance feats.grad: max |dev - model| / S = {np.nanmax(np.where(Sr > 0, errf / Sr, 0)):.3e}")
    assert np.all(errf <= (SR.BOUND + 2.0 ** -23) * Sr) and not np.any(gfe[Sr == 0])
    # only the calls some input needs; none for albedo alone
    del calls[:]
    radiance_backward(autograd.radiance_resident, gs, f, o, d, t, q, gL, gA, needs=(4,))
    assert calls == ["radiance", ("features_gradient", False, True)], calls
    del calls[:]
    _, _, p2 = radiance_backward(autograd.radiance_resident, gs, f, o, d, t, q, gL, gA, needs=(2,))
    assert calls == ["radiance", ("features_gradient", True, False), "evaluate_features", "query_transmittance_profile_grad"], calls
    e2 = np.abs(p2[2].grad.cpu().numpy().astype(np.float64) - (Gf + Gp)[:, 9])
    assert np.all(e2 <= 2 * bound[:, 9])  # (the resident upload's norm words may differ by 2 ulp: twice the bound)
    del calls[:]
    radiance_backward(autograd.radiance_resident, gs, f, o, d, t, q, gL, gA, needs=(3,))
    assert calls == ["radiance"], calls
    with pytest.raises(ValueError):
        radiance_backward(autograd.radiance_resident, gs, f, o, d, t, q, gL, gA, param_device="cpu")


# ------------------------------------------------------------------------------------------------
# 11. the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches(tmp_path):
    from test_gpu_query_grad import sphere_rays
    name, K, C = "250_random", 17, 5
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d, tmax = sphere_rays(name)
    f = RR.features_of(250, C)
    path, fpath = tmp_path / "rays.bin", tmp_path / "features.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<II", 256, 0))
        fh.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
    with open(fpath, "wb") as fh:
        fh.write(struct.pack("<II", 250, C))
        fh.write(f.astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-radiance", str(path), str(K),
                        str(fpath)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rq = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rq ")]
    rt = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rt ")]
    assert [int(v[1]) for v in rq] == list(range(256)) and all(len(v) == 4 + C for v in rq)
    assert [int(v[1]) for v in rt] == list(range(256)) and all(len(v) == 2 + K for v in rt)
    words = np.array([[int(h, 16) for h in v[3:]] for v in rq], np.uint32).view(np.float32)
    trw = np.array([[int(h, 16) for h in v[2:]] for v in rt], np.uint32)
    t = np.ascontiguousarray((tmax[:, None] * np.arange(1, K + 1, dtype=np.float32)[None]) / np.float32(K))
    q = np.ascontiguousarray(np.repeat((tmax / np.float32(K))[:, None], K, 1))
    assert t.dtype == q.dtype == np.float32
    L, op, tr, pairs = run(device(), vr_scene(name), o, d, t, f, q)
    assert pairs.sum() > 0
    assert np.array_equal(bits(words[:, 1:]), bits(L)) and np.array_equal(bits(words[:, 0]), bits(op))
    assert np.array_equal(trw, bits(tr)) and np.array_equal(np.array([int(v[2]) for v in rq]), pairs)
