"""Batched mixture queries (Device.query_transmittance / query_events / query_sigma over vr_query_*) against
the line-faithful oracle: OracleScene.probe(i, o, d) is Gaussian::intersect_direct + optical_depth of the
reference in f32 (gaussian.h:126-164, 208-231), and the three queries are gmm.h:517-578, :457-515 and :98-126.

Test rays: the scene's bounds are those of the oracle's records() means; rng = default_rng(7); origins uniform
in the bounding cube grown by 0.5, targets uniform in 0.7 of it. Test points are uniform in the bounds.

Measured on an MI355X (device vs oracle, the inputs below), see each test's docstring.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import pyoracle as O
from helpers import CAM_POS, FOV, ROOT, main_view_dir, scene_path

pytestmark = pytest.mark.gpu

PARITY = 1e-4  # the project's parity bound
INF = np.float32(np.inf)


# ------------------------------------------------------------------------------------------------
# inputs and CPU references (computed once per (scene, n), shared, never modified)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    return O.OracleScene.load_gmm(scene_path(name + ".txt"))


@functools.lru_cache(maxsize=None)
def bounds(name):
    m = oracle_scene(name).records()[:, :3].astype(np.float64)
    return m.min(0), m.max(0)


@functools.lru_cache(maxsize=None)
def rays(name, n):
    lo, hi = bounds(name)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(7)
    o = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(np.float32)
    tgt = rng.uniform(c - 0.7 * h, c + 0.7 * h, (n, 3)).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    for a in (o, d):
        a.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def points(name, n):
    lo, hi = bounds(name)
    p = np.random.default_rng(7).uniform(lo, hi, (n, 3)).astype(np.float32)
    p.setflags(write=False)
    return p


def probe_all(name, o, d):
    """(n_rays, N, 4) f32: hit, t_enter, t_exit, optical_depth(t_enter, t_exit) of every Gaussian."""
    import ctypes
    sc = oracle_scene(name)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    out = np.zeros((len(o), sc.num, 4), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    probe, base = O.lib().orc_gaussian_probe, out.ctypes.data
    for r in range(len(o)):  # (the loop of OracleScene.probe, without a numpy allocation per call)
        po, pd = o[r].ctypes.data_as(fp), d[r].ctypes.data_as(fp)
        for i in range(sc.num):
            probe(sc.h, i, po, pd, ctypes.cast(base + 16 * (r * sc.num + i), fp))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probes(name, n):
    return probe_all(name, *rays(name, n))


def normalized_f32(d):
    """Ray's normalisation (ray.h:11-12) in f32, Eigen's order; only feeds the f64 model below."""
    d = np.asarray(d, np.float32)
    s = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / np.sqrt(s)[:, None]).astype(np.float32)


def tau_f64(name, o, d, a, b):
    """Optical depth of every Gaussian over [a, b] ((n, N) arrays) in float64 from records():
    gaussian.h:208-231's closed form."""
    from scipy.special import erf
    rec = oracle_scene(name).records().astype(np.float64)
    mean, dens, norm = rec[:, :3], rec[:, 3], rec[:, 10]
    m = rec[:, 4:10]
    M = np.stack([np.stack([m[:, 0], m[:, 1], m[:, 2]], -1), np.stack([m[:, 1], m[:, 3], m[:, 4]], -1),
                  np.stack([m[:, 2], m[:, 4], m[:, 5]], -1)], -2)  # (N, 3, 3)
    dn = normalized_f32(d).astype(np.float64)
    p = o.astype(np.float64)[:, None, :] - mean[None]  # (n, N, 3)
    Md = np.einsum("gij,rj->rgi", M, dn)
    A = np.einsum("ri,rgi->rg", dn, Md)
    B = 2.0 * np.einsum("rgi,rgi->rg", p, Md)
    C = np.einsum("rgi,gij,rgj->rg", p, M, p)
    den = 2.0 * np.sqrt(2.0 * A)
    with np.errstate(invalid="ignore", over="ignore"):
        F1, F0 = erf((B + 2.0 * A * b) / den), erf((B + 2.0 * A * a) / den)
        return dens * norm * np.sqrt(np.pi / (2.0 * A)) * np.exp(-0.5 * (C - B * B / (4.0 * A))) * (F1 - F0)


def tau_ref_f32(name, o, d, a, b):
    """The reference's own optical_depth (gaussian.h:208-231) restated in numpy float32, operation for
    operation as vr_march.h's exact form (erf / exp through float64, rounded once): what f32 arithmetic
    can give at all, used to choose inputs on which the float64 integral is a fair reference."""
    from scipy.special import erf
    f = np.float32
    rec = oracle_scene(name).records()
    mean, dens, norm, m = rec[:, :3], rec[:, 3], rec[:, 10], rec[:, 4:10]
    dn = normalized_f32(d)
    px, py, pz = (o[:, None, k] - mean[None, :, k] for k in range(3))
    dx, dy, dz = (dn[:, None, k] for k in range(3))
    mdx = m[:, 0] * dx + (m[:, 1] * dy + m[:, 2] * dz)
    mdy = m[:, 1] * dx + (m[:, 3] * dy + m[:, 4] * dz)
    mdz = m[:, 2] * dx + (m[:, 4] * dy + m[:, 5] * dz)
    mpx = m[:, 0] * px + (m[:, 1] * py + m[:, 2] * pz)
    mpy = m[:, 1] * px + (m[:, 3] * py + m[:, 4] * pz)
    mpz = m[:, 2] * px + (m[:, 4] * py + m[:, 5] * pz)
    A = dx * mdx + (dy * mdy + dz * mdz)
    B = f(2) * (px * mdx + (py * mdy + pz * mdz))
    C = px * mpx + (py * mpy + pz * mpz)
    with np.errstate(all="ignore"):
        twoA = f(2) * A
        pref = (dens * norm) * np.sqrt(f(np.pi) / twoA)
        den = f(2) * np.sqrt(twoA)
        F1 = erf(((B + twoA * b) / den).astype(np.float64)).astype(f)
        F0 = erf(((B + twoA * a) / den).astype(np.float64)).astype(f)
        e = np.exp((f(-0.5) * (C - (B * B) / (f(4) * A))).astype(np.float64)).astype(f)
        out = pref * e * (F1 - F0)
    assert out.dtype == np.float32
    return out


def device():
    import vr_amd as vr
    return vr.Device.get(0)


@functools.lru_cache(maxsize=None)
def vr_scene(name):
    import vr_amd as vr
    return vr.Scene.load_GMM(scene_path(name + ".txt"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# transmittance
# ------------------------------------------------------------------------------------------------
def oracle_tau_inf(pr):
    """gmm.h:517-578 with tmax = inf: the double sum of probe[3] over hits with t_exit > t_enter."""
    use = (pr[..., 0] != 0) & (pr[..., 2] > pr[..., 1])
    return np.where(use, pr[..., 3].astype(np.float64), 0.0).sum(1)


@pytest.mark.parametrize("name,n", [("1_gaussian", 1), ("many_gaussians", 63), ("50_random", 257), ("250_random", 256)])
def test_transmittance_infinite_tmax_matches_oracle(name, n):
    """|Tr - exp(-float32(sum_double probe[3]))| <= 1e-4. Measured maxima on an MI355X: 1_gaussian 4.1e-11,
    many_gaussians 4.6e-8, 50_random 5.7e-8, 250_random 2.5e-9 (libm against the device library)."""
    o, d = rays(name, n)
    ref = np.exp(-oracle_tau_inf(probes(name, n)).astype(np.float32).astype(np.float64))
    tr = device().query_transmittance(vr_scene(name), o, d)
    assert tr.shape == (n,) and tr.dtype == np.float32
    err = float(np.max(np.abs(tr.astype(np.float64) - ref)))
    print(f"transmittance inf {name} x{n}: max |Tr - oracle| = {err:.3e}")
    assert err <= PARITY


# tmax per scene, chosen on the CPU so that the oracle alone (1) puts >= 25 % of the values in (0.01, 0.99) and
# (2) has the reference's own f32 optical depth (tau_ref_f32) within half the bar of the float64 integral,
# so that float64 is a fair reference for f32 code; both are asserted below. Full-length rays saturate in
# these scenes. 250_random and 1000_random: U(r0, r1 * extent) from the origin (62 % / 41 % in the middle,
# f32 against float64 1.2e-6 / 4.2e-7).
# 10k_random's Gaussians are opaque (a chord's optical depth is ~450) and small (2A ~ 1e4 .. 1e5): Tr falls
# from 1 to 0 inside the first Gaussian a ray meets, so no range from the origin reaches 10 % in the middle
# (U(a, b * extent) scanned for a in 0 .. 0.5, b in 0.2 .. 1), and wherever Tr is in the middle the erf
# argument (B + 2A t) / (2 sqrt(2A)) cancels two terms of ~1e5, whose f32 error (~1e-5 in the argument) times
# that optical depth is ~4e-3: with tmax = first entry + U(0, w) the reference's f32 formula is 4.4e-4 (w =
# 0.03), 1.9e-4 (0.001), 8.5e-5 (0.0004), 5.0e-5 (0.0002) from float64. Hence tmax = the ray's first entry
# distance (oracle probe) + U(0, 0.0002): 59 % in the middle (Tr 0.83 .. 0.99), f32 against float64 5.0e-5.
TMAX_RANGE = {"250_random": (0.05, 0.5, False), "1000_random": (0.02, 0.3, False), "10k_random": (0.0, 0.0002, True)}


@functools.lru_cache(maxsize=None)
def finite_case(name, n):
    """(tmax, oracle tau in float64, the reference's f32 formula's largest |dTr| from it): hit set and clip
    bounds from the f32 probe, the clipped erf integral in float64 from records()."""
    o, d = rays(name, n)
    lo, hi = bounds(name)
    ext = float(np.max(hi - lo))
    r0, r1, from_first = TMAX_RANGE[name]
    pr = probes(name, n)
    u = np.random.default_rng(7)
    if from_first:
        first = np.where(pr[..., 0] != 0, pr[..., 1], np.inf).min(1)
        tmax = (np.where(np.isfinite(first), first, 1.0) + u.uniform(r0, r1, n)).astype(np.float32)
    else:
        tmax = u.uniform(r0, r1 * ext, n).astype(np.float32)
    a = np.maximum(np.float32(0.0), pr[..., 1])
    b = np.minimum(tmax[:, None], pr[..., 2])
    use = (pr[..., 0] != 0) & (b > a)
    tau = np.where(use, tau_f64(name, o, d, a.astype(np.float64), b.astype(np.float64)), 0.0).sum(1)
    tau32 = np.where(use, tau_ref_f32(name, o, d, a, b).astype(np.float64), 0.0).sum(1).astype(np.float32)
    tmax.setflags(write=False)
    return tmax, tau, float(np.max(np.abs(np.exp(-tau32.astype(np.float64)) - np.exp(-tau))))


@pytest.mark.parametrize("name,n", [("250_random", 128), ("1000_random", 128), ("10k_random", 32)])
def test_transmittance_finite_tmax_matches_oracle(name, n):
    """Same 1e-4 bar for a per-ray tmax, against the float64 integral over the f32 probe's clip bounds.
    Measured maxima on an MI355X: 250_random 1.2e-6, 1000_random 3.8e-7, 10k_random 4.97e-5: the f32
    arithmetic's own distance from float64 (see TMAX_RANGE), the device library against libm adding < 1e-6."""
    o, d = rays(name, n)
    tmax, tau, own = finite_case(name, n)
    ref = np.exp(-tau)
    mid = float(np.mean((ref > 0.01) & (ref < 0.99)))
    print(f"transmittance tmax {name} x{n}: {100 * mid:.1f} % of the oracle values in (0.01, 0.99), "
          f"the reference's f32 formula {own:.3e} from float64")
    assert mid >= 0.25 and own <= 0.5 * PARITY
    tr = device().query_transmittance(vr_scene(name), o, d, tmax=tmax)
    err = float(np.max(np.abs(tr.astype(np.float64) - ref)))
    print(f"transmittance tmax {name} x{n}: max |Tr - oracle| = {err:.3e}")
    assert err <= PARITY


def test_transmittance_edge_cases():
    """tmax <= 0 and NaN give Tr = 1, tau = 0; +inf mixed into the same batch equals the all-inf batch; an
    origin inside a Gaussian matches the oracle; a zero direction (and a non-finite origin) gives NaN among
    valid neighbours."""
    name, n = "many_gaussians", 63
    o, d = (a.copy() for a in rays(name, n))
    mean0 = oracle_scene(name).records()[0, :3]
    o[5] = mean0  # inside Gaussian 0 (its centre)
    full = probe_all(name, o, d)
    tmax = np.full(n, INF, np.float32)
    tmax[0], tmax[1], tmax[2], tmax[3] = 0.0, -1.0, np.nan, 1e-3
    d[7] = 0.0
    o[9, 1] = np.inf
    tr, tau = device().query_transmittance(vr_scene(name), o, d, tmax=tmax, return_tau=True)
    assert np.all(tr[:3] == 1.0) and np.all(tau[:3] == 0.0)
    assert np.isnan(tr[7]) and np.isnan(tau[7]) and np.isnan(tr[9]) and np.isnan(tau[9])
    ok = np.ones(n, bool)
    ok[[0, 1, 2, 3, 7, 9]] = False
    ref = np.exp(-oracle_tau_inf(full).astype(np.float32).astype(np.float64))
    assert np.all(np.isfinite(tr[ok])) and np.max(np.abs(tr[ok] - ref[ok])) <= PARITY
    assert full[5, 0, 0] == 1.0 and full[5, 0, 1] == 0.0 and tr[5] < 1.0  # the inside origin: entry clamped to 0
    a = np.maximum(np.float32(0.0), full[3, :, 1])
    b = np.minimum(tmax[3], full[3, :, 2])
    use = (full[3, :, 0] != 0) & (b > a)
    t3 = np.where(use, tau_f64(name, o[3:4], d[3:4], a[None].astype(np.float64), b[None].astype(np.float64))[0], 0.0).sum()
    assert abs(tr[3] - np.exp(-t3)) <= PARITY
    # n = 0 and n = 1
    e = device().query_transmittance(vr_scene(name), o[:0], d[:0])
    assert e.shape == (0,)
    one = device().query_transmittance(vr_scene(name), o[10:11], d[10:11])
    assert bits(one)[0] == bits(tr)[10]


# tau: |tau - oracle| <= TAU_RTOL * tau. 4 x the largest relative gap measured on an MI355X over the three
# fixed cases below (2.04e-7: libm against the device library's erf / exp, a few ulp each), far inside the
# loosest the bound may ever be (1e-4).
TAU_RTOL = 8.2e-7


@pytest.mark.parametrize("name,n", [("many_gaussians", 63), ("50_random", 257), ("250_random", 256)])
def test_tau_matches_oracle_and_tr_is_exp_of_it(name, n):
    """tau against the oracle's double sum; Tr == expf(-tau) bit for bit (the device's expf: torch.exp on
    the same GPU is the same library function), and the Tr of a call with tau equals the Tr of one without
    (the call without tau stops at an optical depth of 104, where expf gives 0 either way). Measured
    largest |tau - oracle| / tau on an MI355X: many_gaussians 1.16e-7, 50_random 2.04e-7, 250_random 9.6e-8."""
    import torch
    o, d = rays(name, n)
    ref = oracle_tau_inf(probes(name, n))
    dev = device()
    tr, tau = dev.query_transmittance(vr_scene(name), o, d, return_tau=True)
    pos = ref > 0
    rel = float(np.max(np.abs(tau[pos].astype(np.float64) - ref[pos]) / ref[pos])) if pos.any() else 0.0
    print(f"tau {name} x{n}: max |tau - oracle| / tau = {rel:.3e}")
    assert TAU_RTOL <= 1e-4 and rel <= TAU_RTOL
    assert np.all(tau[~pos] == 0.0)
    expd = torch.exp(-torch.tensor(tau).cuda()).cpu().numpy()
    assert np.array_equal(bits(tr), bits(expd))
    tr_only = dev.query_transmittance(vr_scene(name), o, d)
    assert np.array_equal(bits(tr_only), bits(tr))


# ------------------------------------------------------------------------------------------------
# events
# ------------------------------------------------------------------------------------------------
def expected_events(pr):
    """Per ray the list of (t bits, Gaussian, entering) of every probe hit (gmm.h:482-485; -0 as +0)."""
    out = []
    for r in range(pr.shape[0]):
        ev = []
        for i in np.nonzero(pr[r, :, 0])[0]:
            t0, t1 = np.float32(pr[r, i, 1] + np.float32(0.0)), np.float32(pr[r, i, 2] + np.float32(0.0))
            if t0 >= 0:
                ev.append((int(bits(t0).reshape(-1)[0]), int(i), 1))
            if t1 >= 0:
                ev.append((int(bits(t1).reshape(-1)[0]), int(i), 0))
        out.append(ev)
    return out


def check_events(pr, off, t, g, e):
    exp = expected_events(pr)
    n = len(exp)
    assert off.shape == (n + 1,) and off[0] == 0
    assert np.array_equal(np.diff(off), [len(x) for x in exp])  # offsets equal exactly
    assert len(t) == len(g) == len(e) == off[-1]
    tb = bits(t)
    ties = 0
    for r in range(n):
        s = slice(off[r], off[r + 1])
        tr_, gr, er = t[s], g[s], e[s]
        assert np.all(tr_[1:] >= tr_[:-1])  # non-decreasing
        assert np.array_equal(tb[s], np.sort(np.array([x[0] for x in exp[r]], np.uint32)))  # sorted t bit-equal
        got = sorted(zip(tb[s].tolist(), gr.tolist(), er.astype(int).tolist()))
        # as sets per run of equal t (no order assumed), which also pins each Gaussian's own (t_enter, t_exit)
        assert got == sorted(exp[r])
        ties += len(tr_) - len(np.unique(tb[s]))
    return ties


@pytest.mark.parametrize("name,n", [("many_gaussians", 63), ("250_random", 256)])
def test_events_match_oracle(name, n):
    o, d = rays(name, n)
    off, t, g, e = device().query_events(vr_scene(name), o, d)
    assert t.dtype == np.float32 and e.dtype == bool
    ties = check_events(probes(name, n), off, t, g, e)
    print(f"events {name} x{n}: {off[-1]} events, {off[-1] / n:.1f} per ray, {ties} tied")
    assert off[-1] > 0


def test_events_origins_inside_gaussians():
    """Origins at Gaussian centres: every Gaussian holding the origin enters at t = 0 (many ties)."""
    name, n = "250_random", 64
    _, d = rays(name, n)
    o = np.ascontiguousarray(oracle_scene(name).records()[:n, :3])
    off, t, g, e = device().query_events(vr_scene(name), o, d)
    ties = check_events(probe_all(name, o, d), off, t, g, e)
    zero = int(np.sum(t == 0.0))
    print(f"events inside {name} x{n}: {off[-1]} events, {zero} at t = 0, {ties} tied")
    assert zero >= n and ties > 0


def test_events_capacity_overflow():
    """A cap below the total returns VR_ERR_OVERFLOW with the right total and writes nothing past cap."""
    import ctypes
    import vr_amd as vr
    from vr_amd import _lib as L
    name, n = "many_gaussians", 63
    o, d = rays(name, n)
    dev = device()
    off, t, g, e = dev.query_events(vr_scene(name), o, d)
    want = int(off[-1])
    cap = want // 2
    rows = dev._pack_rays_numpy(o, d, 0.0)
    tbuf = np.full(want, -7.0, np.float32)
    ebuf = np.full(want, 0xdeadbeef, np.uint32)
    offs = np.zeros(n + 1, np.uint32)
    total = ctypes.c_uint64()
    st = L.lib().vr_query_events(dev._h, rows.ctypes.data, n, offs.ctypes.data_as(L.U32P), L.fptr(tbuf),
                                 ebuf.ctypes.data_as(L.U32P), cap, ctypes.byref(total))
    assert st == L.VR_ERR_OVERFLOW and total.value == want
    assert np.all(tbuf[cap:] == -7.0) and np.all(ebuf[cap:] == 0xdeadbeef)
    assert np.array_equal(offs.astype(np.int64), off)
    st = L.lib().vr_query_events(dev._h, rows.ctypes.data, n, None, None, None, 0, ctypes.byref(total))
    assert st == L.VR_OK and total.value == want
    st = L.lib().vr_query_events(dev._h, rows.ctypes.data, n, None, L.fptr(tbuf), ebuf.ctypes.data_as(L.U32P), want,
                                 ctypes.byref(total))
    assert st == L.VR_OK and np.array_equal(bits(tbuf), bits(t))
    with pytest.raises(vr.VRError):
        L.check(L.lib().vr_query_events(dev._h, rows.ctypes.data, n, None, L.fptr(tbuf), ebuf.ctypes.data_as(L.U32P), 1,
                                        ctypes.byref(total)))


# ------------------------------------------------------------------------------------------------
# sigma
# ------------------------------------------------------------------------------------------------
def sigma_model(name, p):
    """float64 evaluate_sigma (gmm.h:98-126) over the Gaussians with q = p.M.p <= 9; also q itself."""
    rec = oracle_scene(name).records().astype(np.float64)
    mean, dens, norm, alb = rec[:, :3], rec[:, 3], rec[:, 10], rec[:, 11]
    m = rec[:, 4:10]
    x = p.astype(np.float64)[:, None, :] - mean[None]
    q = (m[:, 0] * x[..., 0] ** 2 + m[:, 3] * x[..., 1] ** 2 + m[:, 5] * x[..., 2] ** 2 +
         2.0 * (m[:, 1] * x[..., 0] * x[..., 1] + m[:, 2] * x[..., 0] * x[..., 2] + m[:, 4] * x[..., 1] * x[..., 2]))
    act = q <= 9.0
    mu = np.where(act, dens * norm * np.exp(-0.5 * q), 0.0)
    s, sa = mu.sum(1), (mu * alb).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        amix = np.where(s > 0, sa / s, 0.0)
    sig = np.stack([np.where(s > 0, (1.0 - amix) * s, 0.0), np.where(s > 0, amix * s, 0.0)], 1)
    return sig, act.sum(1), q


# |sigma - model| <= SIGMA_RTOL * max(1, sigma): 4 x the largest such ratio measured on an MI355X (6.2e-7 on
# 250_random, 1.32e-6 on 50_random: f32 mu_t, whose exponent of up to -4.5 carries a few ulp into expf, and
# sigma_a = (1 - a_mix) * sum with albedos up to 0.95, against float64), below the cap of 1e-4.
SIGMA_RTOL = 5.3e-6


@pytest.mark.parametrize("name", ["250_random", "50_random"])
def test_sigma_matches_float64_model(name):
    n = 1024
    p = points(name, n)
    ref, ref_act, q = sigma_model(name, p)
    # f32 error of q: a few eps * kappa, kappa <= 12 (beyond: test_gpu_aniso_query.py, whose margin grows with kappa)
    near = np.any(np.abs(q - 9.0) <= 9e-4, axis=1)
    print(f"sigma {name}: {int(near.sum())} points excluded, nearest |q - 9| = {np.min(np.abs(q - 9.0)):.2e}")
    assert near.mean() <= 0.01
    keep = ~near
    sig, act = device().query_sigma(vr_scene(name), p, return_active=True)
    assert sig.shape == (n, 2) and sig.dtype == np.float32
    assert np.array_equal(act[keep], ref_act[keep])  # the active count, exactly
    ratio = float(np.max(np.abs(sig[keep].astype(np.float64) - ref[keep]) / np.maximum(1.0, ref[keep])))
    print(f"sigma {name}: max |sigma - model| / max(1, sigma) = {ratio:.3e}, largest sigma {ref.max():.1f}")
    assert SIGMA_RTOL <= 1e-4 and ratio <= SIGMA_RTOL
    out = keep & (ref_act == 0)  # outside every ellipsoid: exactly 0, 0
    print(f"sigma {name}: {int(out.sum())} points outside every ellipsoid")
    assert out.sum() > 0 and np.all(bits(sig[out]) == 0)
    assert np.array_equal(bits(device().query_sigma(vr_scene(name), p)), bits(sig))
    assert device().query_sigma(vr_scene(name), p[:0]).shape == (0, 2)


def test_queries_on_a_one_gaussian_scene():
    """The root of the tree is a leaf."""
    name = "1_gaussian"
    rec = oracle_scene(name).records()
    o = np.float32([[0, 0, 5], [3, 3, 3], rec[0, :3]]) + np.float32([[0, 0, 0], [0, 0, 0], [0.01, 0, 0]])
    d = (rec[0, :3][None] - o).astype(np.float32)
    d[2] = (1, 0, 0)
    pr = probe_all(name, o, d)
    off, t, g, e = device().query_events(vr_scene(name), o, d)
    check_events(pr, off, t, g, e)
    assert off[-1] == 6
    p = np.ascontiguousarray(np.float32([rec[0, :3], rec[0, :3] + 100.0]))
    sig, act = device().query_sigma(vr_scene(name), p, return_active=True)
    ref, ref_act, _ = sigma_model(name, p)
    assert act.tolist() == [1, 0] == ref_act.tolist() and np.all(sig[1] == 0)
    assert np.max(np.abs(sig - ref) / np.maximum(1.0, ref)) <= SIGMA_RTOL


# ------------------------------------------------------------------------------------------------
# invariance
# ------------------------------------------------------------------------------------------------
def all_queries(dev, sc, o, d, tmax, p, as_torch=False):
    if as_torch:
        import torch
        o, d, tmax, p = (torch.tensor(a).cuda() for a in (o, d, tmax, p))
    res = [*dev.query_transmittance(sc, o, d, tmax=tmax, return_tau=True), dev.query_transmittance(sc, o, d),
           *dev.query_events(sc, o, d), *dev.query_sigma(sc, p, return_active=True)]
    return [r.cpu().numpy() if as_torch else r for r in res]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float32:
            assert np.array_equal(bits(x), bits(y))
        else:
            assert np.array_equal(x, y)


@functools.lru_cache(maxsize=None)
def invariance_inputs():
    name, n = "1000_random", 128  # >= 256 Gaussians: the device builder takes the scene
    o, d = rays(name, n)
    tmax = np.random.default_rng(11).uniform(0.05, 3.0, n).astype(np.float32)
    tmax[::7] = INF
    return name, o, d, tmax, points(name, 512)


@functools.lru_cache(maxsize=None)
def invariance_baseline():
    name, o, d, tmax, p = invariance_inputs()
    return all_queries(device(), vr_scene(name), o, d, tmax, p)


@pytest.mark.parametrize("half_nodes,device_bvh", [(0, 0), (1, 1), (0, 1)])
def test_results_do_not_depend_on_the_tree(device_options, half_nodes, device_bvh):
    """Bit-identical under VR_OPT_HALF_NODES 0 / 1 and VR_OPT_DEVICE_BVH 0 / 1 (the default is 1 / 0)."""
    name, o, d, tmax, p = invariance_inputs()
    base = invariance_baseline()
    device_options("half_nodes", half_nodes)
    device_options("device_bvh", device_bvh)
    same(all_queries(device(), vr_scene(name), o, d, tmax, p), base)


def test_torch_input_equals_numpy_input():
    """Torch tensors take the `_device` entry points on torch's current stream (rays packed on the device),
    numpy arrays the host entry points: the same results bit for bit, of the caller's kind."""
    import torch
    name, o, d, tmax, p = invariance_inputs()
    dev = device()
    tr = dev.query_transmittance(vr_scene(name), torch.tensor(o).cuda(), torch.tensor(d).cuda())
    assert isinstance(tr, torch.Tensor) and tr.is_cuda
    same(all_queries(dev, vr_scene(name), o, d, tmax, p, as_torch=True), invariance_baseline())
    off, t, g, e = dev.query_events(vr_scene(name), torch.tensor(o).cuda(), torch.tensor(d).cuda())
    assert off.dtype == torch.int64 and g.dtype == torch.int32 and e.dtype == torch.bool


def test_queries_leave_the_last_frame_alone():
    """stats() of a rendered frame is unchanged by the three queries and a re-render is bit-equal."""
    import vr_amd as vr
    name = "many_gaussians"
    sc = vr_scene(name)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), env_samples=8)
    img = vr.Image(48, 48)
    integ.render(sc, img)
    dev = device()
    before = dev.stats()
    first = img.pixels.copy()
    o, d = rays(name, 63)
    all_queries(dev, sc, o, d, np.full(63, INF, np.float32), points(name, 100))
    all_queries(dev, sc, o, d, np.full(63, INF, np.float32), points(name, 100), as_torch=True)
    dev.synchronize()
    assert dev.stats() == before
    integ.render(sc, img)
    assert np.array_equal(bits(img.pixels), bits(first))


def test_errors():
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    o, d = rays("many_gaussians", 63)
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    tr = np.zeros(63, np.float32)
    assert L.lib().vr_query_transmittance(fresh._h, rows.ctypes.data, 63, L.fptr(tr), None) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert L.lib().vr_query_transmittance(fresh._h, rows.ctypes.data, 63, L.fptr(tr), None) == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene("many_gaussians"))
    assert L.lib().vr_query_transmittance(fresh._h, None, 63, L.fptr(tr), None) == 1  # VR_ERR_INVALID
    assert L.lib().vr_query_transmittance(fresh._h, None, 0, None, None) == 0
    assert L.lib().vr_query_sigma(fresh._h, None, 5, None, None) == 1
    assert L.lib().vr_query_transmittance(fresh._h, rows.ctypes.data, 63, L.fptr(tr), None) == 0
    assert np.array_equal(bits(tr), bits(device().query_transmittance(vr_scene("many_gaussians"), o, d)))


# ------------------------------------------------------------------------------------------------
# C++ mirror (include/vr/query.h through tools/vol_render --query)
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_python(tmp_path):
    """MixtureQuery (transmittance_up_to, intersect_events, evaluate_sigma) through the driver gives the
    Python results bit for bit."""
    name, n, m = "50_random", 65, 33
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d = rays(name, n)
    tmax = np.random.default_rng(3).uniform(0.1, 4.0, n).astype(np.float32)
    tmax[::5] = INF
    p = points(name, m)
    path = tmp_path / "rays.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", n, m))
        f.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
        f.write(p.astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    dev, sc = device(), vr_scene(name)
    tr, tau = dev.query_transmittance(sc, o, d, tmax=tmax, return_tau=True)
    off, t, g, e = dev.query_events(sc, o, d)
    sig, act = dev.query_sigma(sc, p, return_active=True)
    c_tr = [(int(x[1]), int(x[2], 16), int(x[3], 16)) for x in lines if x[0] == "tr"]
    assert c_tr == [(i, int(bits(tr)[i]), int(bits(tau)[i])) for i in range(n)]
    c_ev = [(int(x[1]), int(x[2], 16), int(x[3]), int(x[4])) for x in lines if x[0] == "ev"]
    ray_of = np.repeat(np.arange(n), np.diff(off))
    assert c_ev == list(zip(ray_of.tolist(), bits(t).tolist(), g.tolist(), e.astype(int).tolist())) and len(c_ev) > 0
    c_sig = [(int(x[1]), int(x[2], 16), int(x[3], 16), int(x[4])) for x in lines if x[0] == "sigma"]
    assert c_sig == [(i, int(bits(sig)[i, 0]), int(bits(sig)[i, 1]), int(act[i])) for i in range(m)]
