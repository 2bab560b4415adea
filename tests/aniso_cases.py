"""Elongated Gaussians: the scene recipe, the aimed rays and points, and the CPU models of the anisotropy tests
(test_aniso_reference.py on the CPU, test_gpu_aniso_*.py on the device). Computed once per case, shared, never
modified. Nothing here touches the GPU, and vr_amd is imported only inside device_scene().

The make_random family of the other tests has a covariance condition number kappa <= 12. Here a Gaussian is a
disc, sigma = (s, s, s / ratio), or a needle, sigma = (s, s / ratio, s / ratio), so kappa(M) = ratio^2, and every
f32 rounding difference in p.M.p is amplified by about kappa. The device's forward queries, primary march, exact
slow path and free-flight sweep state the reference's f32 arithmetic operation for operation, so on these scenes the
fair reference is the oracle's own f32 value, not a float64 model: the oracle itself is up to 0.16 away from
float64 at disc 100 (test_aniso_reference.py prints the table).

The ladder: discs of ratio 3 (the control: kappa 9, inside today's family), 10, 30, 100; needles of ratio 3, 10,
30; and needle 100, where the reference's f32 cofactor inverse by itself produces records whose M is not positive
definite. Ratios of 300 and above are out of scope: at needle 300, 44 of 150 records hold NaN or inf, and at
disc 300 the oracle's hit decisions differ from float64 on more (ray, Gaussian) pairs than there are hits, so
neither the oracle nor float64 is a reference for anything there.

Record layout (OracleScene.records(), (N, 12) f32): mean[3], density, M {00 01 02 11 12 22}, norm, albedo.
"""
import collections
import ctypes
import functools

import numpy as np

import pyoracle as O

F32 = np.float32
LADDER = (("disc", 3), ("disc", 10), ("disc", 30), ("disc", 100), ("needle", 3), ("needle", 10), ("needle", 30),
          ("needle", 100))
CONTROL = ("disc", 3)
SIZES = {("needle", 100): 512}
LIGHT = ((0.0, 3.0, 0.0), (1.0, 1.0, 1.0))
R_AIM = 3.3        # the aimed targets fill the 3.3-sigma ellipsoid: 3 sigma is the cut-off
CAP = 0.05         # either exclusion rule may take at most this share of a case's rays / points
CUT_FACTOR = 4.0   # cut-off points: |q64 - 9| <= 4 x the rung's largest |q32 - q64| (SIGMA_RTOL's own factor)
Q_WINDOW = 30.0    # ... measured over pairs with |q64 - 9| < 30

Case = collections.namedtuple("Case", "shape ratio mean cov6 density albedo rot sigma")


def size(shape, ratio, n=None):
    """The rung's number of Gaussians: 150, and 512 at needle 100, where non-PD records are about 1 in 250."""
    return n if n is not None else SIZES.get((shape, ratio), 150)


def case_id(key):
    return f"{key[0]}{key[1]}"


@functools.lru_cache(maxsize=None)
def gaussians(shape, ratio, n=None, seed=31):
    """n Gaussians, default_rng(seed), drawn in this order: means U(-1, 1)^3, quaternions (4 normals each, the recipe
    of tree_reference.rotated_cov), s U(0.05, 0.15), albedo U(0.1, 0.9). sigma = (s, s, s / ratio) for a disc,
    (s, s / ratio, s / ratio) for a needle; covariance R diag(sigma^2) R^T in float64, rounded to f32. The density
    1 / (norm sqrt(2 pi) sigma_min), norm = (2 pi)^-1.5 / (sigma_0 sigma_1 sigma_2) in float64, gives a central chord
    along the thinnest axis an optical depth of 1."""
    assert shape in ("disc", "needle") and ratio >= 1
    n = size(shape, ratio, n)
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1.0, 1.0, (n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                    np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                    np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    s = rng.uniform(0.05, 0.15, n)
    alb = rng.uniform(0.1, 0.9, n)
    thin = s / float(ratio)
    sigma = np.stack([s, s, thin] if shape == "disc" else [s, thin, thin], 1)
    C = np.einsum("nij,nj,nkj->nik", rot, sigma ** 2, rot)
    cov6 = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], -1)
    norm = (2.0 * np.pi) ** -1.5 / np.prod(sigma, axis=1)
    dens = 1.0 / (norm * np.sqrt(2.0 * np.pi) * sigma.min(1))
    out = Case(shape, ratio, mean.astype(F32), cov6.astype(F32), dens.astype(F32), alb.astype(F32), rot, sigma)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def arrays(case):
    """(mean, cov6, density, albedo): the leading arguments of both from_gaussians."""
    return case.mean, case.cov6, case.density, case.albedo


@functools.lru_cache(maxsize=None)
def oracle_scene(shape, ratio, n=None):
    return O.OracleScene.from_gaussians(*arrays(gaussians(shape, ratio, n)), [LIGHT[0]], [LIGHT[1]])


@functools.lru_cache(maxsize=None)
def device_scene(shape, ratio, n=None):
    import vr_amd as vr
    return vr.Scene.from_gaussians(*arrays(gaussians(shape, ratio, n)), lights=[vr.Light(*LIGHT)])


@functools.lru_cache(maxsize=None)
def records(shape, ratio, n=None):
    rec = oracle_scene(shape, ratio, n).records()
    rec.setflags(write=False)
    return rec


def sym(m6):
    """(..., 6) {00 01 02 11 12 22} -> (..., 3, 3)."""
    m6 = np.asarray(m6)
    return np.stack([np.stack([m6[..., 0], m6[..., 1], m6[..., 2]], -1), np.stack([m6[..., 1], m6[..., 3], m6[..., 4]], -1),
                     np.stack([m6[..., 2], m6[..., 4], m6[..., 5]], -1)], -2)


def record_health(rec):
    """(kappa (N,) of the finite records' M by |eigenvalue|, non-PD mask (N,), non-finite mask (N,))."""
    bad = ~np.isfinite(rec).all(1)
    ev = np.linalg.eigvalsh(sym(np.where(bad[:, None], 1.0, rec[:, 4:10].astype(np.float64))))
    with np.errstate(all="ignore"):
        kappa = np.abs(ev).max(1) / np.abs(ev).min(1)
    return kappa, (ev.min(1) <= 0) & ~bad, bad


# ------------------------------------------------------------------------------------------------
# aimed rays and points
# ------------------------------------------------------------------------------------------------
def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _targets(case, n, rng):
    """Target i lies in Gaussian i % N: mean + V sqrt(Lambda) v with v uniform in the ball of radius R_AIM (the
    radii R_AIM u^(1/3) are drawn first, then the directions)."""
    N = len(case.mean)
    g = np.arange(n) % N
    r = R_AIM * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0)
    v = _unit(rng, n) * r[:, None]
    return case.mean[g].astype(np.float64) + np.einsum("nij,nj->ni", case.rot[g], case.sigma[g] * v), g


@functools.lru_cache(maxsize=None)
def aimed_rays(shape, ratio, n=256, N=None):
    """(origins, directions (n, 3) f32, the aimed Gaussian (n,)): default_rng(7); ray i aims at a point of Gaussian
    i % N (_targets) from that point plus a random unit vector times U(0.5, 2.0). The direction, target - origin, is
    left unnormalised: its length is the distance to the target."""
    rng = np.random.default_rng(7)
    tgt, g = _targets(gaussians(shape, ratio, N), n, rng)
    o = (tgt + _unit(rng, n) * rng.uniform(0.5, 2.0, n)[:, None]).astype(F32)
    d = (tgt.astype(F32) - o).astype(F32)
    for a in (o, d, g):
        a.setflags(write=False)
    return o, d, g


@functools.lru_cache(maxsize=None)
def aimed_points(shape, ratio, n=1024, N=None):
    """(n, 3) f32: the targets of _targets alone, default_rng(7). Uniform points of the scene's box land inside a thin
    disc 3 % of the time, which tests nothing."""
    p = _targets(gaussians(shape, ratio, N), n, np.random.default_rng(7))[0].astype(F32)
    p.setflags(write=False)
    return p


def probe_all(sc, o, d):
    """(n, N, 4) f32: hit, t_enter, t_exit, optical_depth(t_enter, t_exit) of every Gaussian of oracle scene `sc`
    (orc_gaussian_probe: intersect_direct and optical_depth of the reference in f32)."""
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    out = np.zeros((len(o), sc.num, 4), F32)
    fp = ctypes.POINTER(ctypes.c_float)
    probe, base = O.lib().orc_gaussian_probe, out.ctypes.data
    for r in range(len(o)):
        po, pd = o[r].ctypes.data_as(fp), d[r].ctypes.data_as(fp)
        for i in range(sc.num):
            probe(sc.h, i, po, pd, ctypes.cast(base + 16 * (r * sc.num + i), fp))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
def normalized_f32(d):
    """Ray's normalisation (ray.h:11-12) in f32, Eigen's order: the direction both sides walk."""
    d = np.asarray(d, F32)
    s = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / np.sqrt(s)[:, None]).astype(F32)


class Pairs64:
    """float64 model of every (ray, Gaussian) pair on the f32 records: the quadratic, the hit decision and
    unclamped bounds of intersect_direct (gaussian.h:126-164), and the closed-form optical depth (:208-231).
    `unit`: the directions are unit vectors already (an oracle row's), else they are normalised in f32 first."""

    def __init__(self, rec, o, d, unit=False):
        rec = rec.astype(np.float64)
        self.dens, self.norm = rec[:, 3], rec[:, 10]
        M = sym(rec[:, 4:10])
        dn = (np.asarray(d, F32) if unit else normalized_f32(d)).astype(np.float64)
        p = np.asarray(o, F32).astype(np.float64)[:, None, :] - rec[None, :, :3]
        Md = np.einsum("gij,rj->rgi", M, dn)
        self.A = np.einsum("ri,rgi->rg", dn, Md)
        self.B = 2.0 * np.einsum("rgi,rgi->rg", p, Md)
        self.C = np.einsum("rgi,gij,rgj->rg", p, M, p)
        with np.errstate(all="ignore"):
            disc = self.B * self.B - 4.0 * self.A * (self.C - 9.0)
            s = np.sqrt(disc)
            ta, tb = (-self.B - s) / (2.0 * self.A), (-self.B + s) / (2.0 * self.A)
            self.t0, self.t1 = np.minimum(ta, tb), np.maximum(ta, tb)
            self.hit = (disc >= 0) & (self.t1 >= 0)

    def tau(self, a, b):
        """(n, N) float64: each Gaussian's optical depth over [a, b] ((n, N) arrays)."""
        from scipy.special import erf
        A, B = self.A, self.B
        with np.errstate(all="ignore"):
            den = 2.0 * np.sqrt(2.0 * A)
            return (self.dens * self.norm * np.sqrt(np.pi / (2.0 * A)) * np.exp(-0.5 * (self.C - B * B / (4.0 * A))) *
                    (erf((B + 2.0 * A * b) / den) - erf((B + 2.0 * A * a) / den)))


def _mv32(m, x, y, z):
    """M v in the reference's association, rows of M as (N,) columns of the (N, 6) array m."""
    return (m[:, 0] * x + (m[:, 1] * y + m[:, 2] * z), m[:, 1] * x + (m[:, 3] * y + m[:, 4] * z),
            m[:, 2] * x + (m[:, 4] * y + m[:, 5] * z))


def tau_ref_f32(rec, o, d, a, b, unit=False):
    """The reference's own optical_depth (gaussian.h:208-231) restated in numpy float32, operation for operation as
    vr_march.h's exact form (erf / exp through float64, rounded once): (n, N) f32 for clip bounds a, b (n, N) f32."""
    from scipy.special import erf
    f = F32
    mean, dens, norm, m = rec[:, :3], rec[:, 3], rec[:, 10], rec[:, 4:10]
    dn = np.asarray(d, f) if unit else normalized_f32(d)
    o = np.asarray(o, f)
    px, py, pz = (o[:, None, k] - mean[None, :, k] for k in range(3))
    dx, dy, dz = (dn[:, None, k] for k in range(3))
    mdx, mdy, mdz = _mv32(m, dx, dy, dz)
    mpx, mpy, mpz = _mv32(m, px, py, pz)
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
    assert out.dtype == f
    return out


def q_ref_f32(rec, p):
    """(n, N) f32: q = x.(M x), x = p - mean, in the reference's association (intersect_direct's C before the
    - 9, the value vr_query.hip's membership test compares)."""
    p = np.asarray(p, F32)
    px, py, pz = (p[:, None, k] - rec[None, :, k] for k in range(3))
    mpx, mpy, mpz = _mv32(rec[:, 4:10], px, py, pz)
    q = px * mpx + (py * mpy + pz * mpz)
    assert q.dtype == F32
    return q


def q_f64(rec, p):
    rec = rec.astype(np.float64)
    x = np.asarray(p, F32).astype(np.float64)[:, None, :] - rec[None, :, :3]
    return np.einsum("rgi,gij,rgj->rg", x, sym(rec[:, 4:10]), x)


# ------------------------------------------------------------------------------------------------
# per-rung bundles
# ------------------------------------------------------------------------------------------------
def oracle_tau_inf(pr):
    """gmm.h:517-578 with tmax = inf: the double sum of probe[3] over hits with t_exit > t_enter."""
    use = (pr[..., 0] != 0) & (pr[..., 2] > pr[..., 1])
    return np.where(use, pr[..., 3].astype(np.float64), 0.0).sum(1)


RayCase = collections.namedtuple("RayCase", "o d aimed pr pairs keep tau_oracle tr_oracle tr_f64 flips nonpd_rays")


@functools.lru_cache(maxsize=None)
def ray_case(shape, ratio, n=256, N=None):
    """The aimed rays of one rung with the oracle's probe, the float64 pair model and the phantom-ray rule: `keep` is
    False on a ray on which the f32 probe reports a hit on some Gaussian that the float64 model misses entirely. Such a
    chord can lie outside the Gaussian's padded box, so whether a tree walk tests it depends on the tree (the
    reference's own BVH has the same ambiguity). tr_f64: float64 decisions, bounds and depths. flips: pairs whose
    hit decision differs between the two. nonpd_rays: rays the probe reports as hitting a non-PD record."""
    o, d, g = aimed_rays(shape, ratio, n, N)
    rec = records(shape, ratio, N)
    pr = probe_all(oracle_scene(shape, ratio, N), o, d)
    pairs = Pairs64(rec, o, d)
    hit32 = pr[..., 0] != 0
    _, nonpd, _ = record_health(rec)
    pd = ~nonpd[None, :]
    keep = ~np.any(hit32 & ~pairs.hit & pd, axis=1)
    tau_o = oracle_tau_inf(pr)
    t64 = np.where(pairs.hit & pd, pairs.tau(np.maximum(pairs.t0, 0.0), pairs.t1), 0.0).sum(1)
    out = RayCase(o, d, g, pr, pairs, keep, tau_o, np.exp(-tau_o.astype(F32).astype(np.float64)), np.exp(-t64),
                  int(np.sum((hit32 != pairs.hit) & pd)), np.any(hit32 & nonpd[None, :], axis=1))
    for a in (keep, tau_o, out.tr_oracle, out.tr_f64, out.nonpd_rays):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def finite_case(shape, ratio, n=256, N=None):
    """(tmax (n,) f32, the oracle-side tau (n,) float64): tmax = U(0.3, 1.0) x the distance to the target,
    default_rng(11); the reference is tau_ref_f32 summed in double over the probe's hits, each on its clip bounds
    [max(0, t_enter), min(tmax, t_exit)] in f32 (gmm.h:517-578)."""
    rc = ray_case(shape, ratio, n, N)
    dist = np.linalg.norm(rc.d.astype(np.float64), axis=1)
    tmax = (np.random.default_rng(11).uniform(0.3, 1.0, n) * dist).astype(F32)
    a = np.maximum(F32(0.0), rc.pr[..., 1])
    b = np.minimum(tmax[:, None], rc.pr[..., 2])
    use = (rc.pr[..., 0] != 0) & (b > a)
    t32 = tau_ref_f32(records(shape, ratio, N), rc.o, rc.d, a, b)
    tau = np.where(use, t32.astype(np.float64), 0.0).sum(1)
    tmax.setflags(write=False)
    tau.setflags(write=False)
    return tmax, tau


@functools.lru_cache(maxsize=None)
def q_error(shape, ratio, n=1024, N=None):
    """The rung's largest |q32 - q64| over the aimed points' pairs with |q64 - 9| < Q_WINDOW: what the reference's f32
    arithmetic loses on q near the 3-sigma cut-off."""
    rec, p = records(shape, ratio, N), aimed_points(shape, ratio, n, N)
    q64 = q_f64(rec, p)
    _, nonpd, _ = record_health(rec)
    near = (np.abs(q64 - 9.0) < Q_WINDOW) & ~nonpd[None, :]
    return float(np.max(np.abs(q_ref_f32(rec, p).astype(np.float64) - q64)[near]))


def sigma_scale(shape, ratio):
    """SIGMA_RTOL's multiplier at this rung: the rung's q_error over the control rung's, never under 1. mu_t carries
    exp(-q / 2), so its relative f32 error is half the error of q; the control rung is where SIGMA_RTOL was sized."""
    return max(1.0, q_error(shape, ratio) / q_error(*CONTROL))


SigmaCase = collections.namedtuple("SigmaCase", "p sigma active keep q64 sigma_f32")


@functools.lru_cache(maxsize=None)
def sigma_case(shape, ratio, n=1024, N=None):
    """The aimed points of one rung, the float64 evaluate_sigma (gmm.h:98-126) over the Gaussians with q64 <= 9, and the
    cut-off rule: `keep` is False on a point with some |q64 - 9| <= CUT_FACTOR x q_error. sigma_f32 is the same model
    with the f32 restatement's q in the decision and in the exponent: what line-faithful f32 code gives at best."""
    rec, p = records(shape, ratio, N), aimed_points(shape, ratio, n, N)
    r64 = rec.astype(np.float64)
    dens, norm, alb = r64[:, 3], r64[:, 10], r64[:, 11]
    _, nonpd, _ = record_health(rec)
    q64 = q_f64(rec, p)
    keep = ~np.any((np.abs(q64 - 9.0) <= CUT_FACTOR * q_error(shape, ratio, n, N)) & ~nonpd[None, :], axis=1)

    def mix(q):
        act = q <= 9.0
        with np.errstate(all="ignore"):
            mu = np.where(act, dens * norm * np.exp(-0.5 * q), 0.0)
            s, sa = mu.sum(1), (mu * alb).sum(1)
            amix = np.where(s > 0, sa / s, 0.0)
        return np.stack([np.where(s > 0, (1.0 - amix) * s, 0.0), np.where(s > 0, amix * s, 0.0)], 1), act.sum(1)

    sig, act = mix(q64)
    out = SigmaCase(p, sig, act, keep, q64, mix(q_ref_f32(rec, p).astype(np.float64))[0])
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# record-level frames (test_gpu_aniso_records.py): 24 x 24, env_samples 3, the camera of test_gpu_records.py moved to look
# at the origin from 4 units. Six pixels per rung among those with the most rows, found by scanning the frame with
# the oracle; test_aniso_reference.py asserts that each has rows and that at least 25 % of a case's rays are fair.
# ------------------------------------------------------------------------------------------------
RECORD_CAMERA = (np.float32([0.0, 0.0, 4.0]), np.float32([0.0, 0.0, -1.0]))
RECORD_W, RECORD_ENV = 24, 3
RECORD_CASES = {
    ("disc", 10): [(20, 10), (16, 0), (20, 23), (4, 13), (9, 10), (13, 7)],
    ("disc", 30): [(6, 12), (16, 3), (19, 18), (19, 22), (4, 17), (16, 1)],
    ("needle", 10): [(19, 22), (15, 14), (16, 20), (8, 10), (4, 16), (20, 10)],
}
MIN_FAIR_SHARE = 0.25


@functools.lru_cache(maxsize=None)
def record_case(shape, ratio):
    """({pixel: oracle rows}, {pixel: {step: float64 Tr of the row's rays}}) of the rung's six pixels; the float64 ray
    model takes each row's active list from the oracle (records_compare.ray_model_f64)."""
    import records_compare as RC
    osc, rec = oracle_scene(shape, ratio), records(shape, ratio)
    pixels = RECORD_CASES[(shape, ratio)]
    rows = RC.oracle_rows_many(osc, pixels, RECORD_W, RECORD_W, RECORD_ENV, cam=RECORD_CAMERA)
    model = {}
    for p in pixels:
        act = {int(r[0]): RC.record_active(osc, p[0], p[1], RECORD_W, RECORD_W, RECORD_ENV, int(r[0]), cam=RECORD_CAMERA) for r in rows[p]}
        assert all(len(act[int(r[0])]) == int(r[8]) for r in rows[p])
        model[p] = RC.ray_model_f64(rec, rows[p], p[0], p[1], [LIGHT[0]], RECORD_ENV, active=act)
    return rows, model
