"""Reference model of the optical-depth gradient query (Device.query_transmittance_grad, vr_query_transmittance_grad):
the formulas of include/vr_hip.h in float64 numpy / scipy. Computed once per case, shared, never modified.

For a scene: hit flags and the f32 t_enter / t_exit come from the oracle's probe (orc_gaussian_probe: intersect_direct,
gaussian.h:126-164, the decision both sides take in f32), the records (mean, density, inverse covariance, norm in f32)
from the oracle scene. Everything after that is float64. `contributions` is also the model the CPU test checks against
central differences of its own closed-form tau, there with float64 records and bounds.

Row layout (10 per Gaussian): d/d mean[3], d/d cov6 {xx, xy, xz, yy, yz, zz} (off-diagonal: the stored number stands
at (i, j) and (j, i), hence 2 G_Sigma[i][j]), d/d density.
"""
import ctypes
import functools

import numpy as np

E45 = np.exp(-4.5)
BOUND = 2.0 ** -21  # |G_dev - G64| <= BOUND * S per component (the only f32 step is the final rounding, 2^-24 S; 8x for erf / exp)


def sym(m6):
    """(..., 6) {00 01 02 11 12 22} -> (..., 3, 3)."""
    m6 = np.asarray(m6)
    return np.stack([np.stack([m6[..., 0], m6[..., 1], m6[..., 2]], -1), np.stack([m6[..., 1], m6[..., 3], m6[..., 4]], -1),
                     np.stack([m6[..., 2], m6[..., 4], m6[..., 5]], -1)], -2)


def normalized_f32(d):
    """Ray's normalisation (ray.h:11-12) in f32, Eigen's order: the direction the device walks."""
    d = np.asarray(d, np.float32)
    s = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / np.sqrt(s)[:, None]).astype(np.float32)


def quadratic(mean, M, o, d):
    """A, B, C (n, N) and p (n, N, 3), Md (n, N, 3) of q(t) = A t^2 + B t + C for rays (n) and Gaussians (N)."""
    p = o[:, None, :] - mean[None]
    Md = np.einsum("gij,rj->rgi", M, d)
    A = np.einsum("ri,rgi->rg", d, Md)
    B = 2.0 * np.einsum("rgi,rgi->rg", p, Md)
    C = np.einsum("rgi,gij,rgj->rg", p, M, p)
    return A, B, C, p, Md


def tau_terms(mean, M, norm, rho, o, d, a, b, use):
    """(n, N) float64: the closed-form optical depth (gaussian.h:208-231) of each Gaussian over [a, b] where `use`."""
    from scipy.special import erf
    A, B, C, _, _ = quadratic(mean, M, o, d)
    with np.errstate(all="ignore"):
        m = -B / (2.0 * A)
        k = np.exp(-0.5 * (C - B * B / (4.0 * A)))
        sA = np.sqrt(0.5 * A)
        J0 = np.sqrt(np.pi / (2.0 * A)) * (erf((b - m) * sA) - erf((a - m) * sA))
    return np.where(use, rho * norm * k * J0, 0.0)


def contributions(mean, M, norm, rho, o, d, a, b, use, move_in, move_out):
    """(n, N, 10) float64: d tau_i / d theta_g per ray and Gaussian, after the conversion to covariance space.
    mean (N, 3), M (N, 3, 3), norm, rho (N,); o, d (n, 3) with d of unit length; a, b (n, N) the clip bounds; use:
    the hit contributes (b > a); move_in / move_out: the bound lies on the ellipsoid and moves with the parameters."""
    from scipy.special import erf
    A, B, C, p, Md = quadratic(mean, M, o, d)
    dd = np.broadcast_to(d[:, None, :], p.shape)
    with np.errstate(all="ignore"):
        m = -B / (2.0 * A)
        c = p + m[..., None] * dd
        ua, ub = a - m, b - m
        k = np.exp(-0.5 * (C - B * B / (4.0 * A)))
        sA = np.sqrt(0.5 * A)
        J0 = np.sqrt(np.pi / (2.0 * A)) * (erf(ub * sA) - erf(ua * sA))
        ea, eb = np.exp(-0.5 * A * ua * ua), np.exp(-0.5 * A * ub * ub)
        J1 = (ea - eb) / A
        J2 = (ua * ea - ub * eb) / A + J0 / A
        nk = norm * k
        U = nk * J0
        outer = lambda x, y: x[..., :, None] * y[..., None, :]  # noqa: E731
        GM = -0.5 * (rho * nk)[..., None, None] * (J0[..., None, None] * outer(c, c) +
                                                    J1[..., None, None] * (outer(c, dd) + outer(dd, c)) +
                                                    J2[..., None, None] * outer(dd, dd))
        gmean = (rho * nk)[..., None] * np.einsum("gij,rgj->rgi", M, c * J0[..., None] + dd * J1[..., None])
        for t, sg, mv in ((b, 1.0, move_out), (a, -1.0, move_in)):
            x = p + t[..., None] * dd
            w = np.where(mv, sg * rho * norm * E45 / (2.0 * A * t + B), 0.0)
            GM = GM - w[..., None, None] * outer(x, x)
            gmean = gmean + 2.0 * w[..., None] * np.einsum("gij,rgj->rgi", M, x)
        T = rho * U
        GS = -np.einsum("gij,rgjk,gkl->rgil", M, GM, M) - 0.5 * T[..., None, None] * M[None]
    out = np.stack([gmean[..., 0], gmean[..., 1], gmean[..., 2], GS[..., 0, 0], 2.0 * GS[..., 0, 1], 2.0 * GS[..., 0, 2],
                    GS[..., 1, 1], 2.0 * GS[..., 1, 2], GS[..., 2, 2], U], -1)
    return np.where(use[..., None], out, 0.0)


def descent_case():
    """The descent step's case: (theta0 (8, 10), theta* (8, 10), origins (64, 3), unit directions (64, 3), fraction).
    8 Gaussians, default_rng(7): mean U(-0.6, 0.6)^3, covariance L L^T + 0.01 I with L's entries U(-0.25, 0.25), density
    U(0.5, 1.5); theta* = theta0 (1 + 0.1 U(-1, 1)) per number (10 %); 64 rays from the radius-4 sphere toward points
    U(-0.5, 0.5)^3. Every number is a float32 value, so the device and the float64 model see the same parameters. The
    step is sized for a first-order drop of `fraction` = 1 % of the loss sum (tau - tau*)^2."""
    rng = np.random.default_rng(7)
    theta = np.zeros((8, 10))
    for g in range(8):
        L = rng.uniform(-0.25, 0.25, (3, 3))
        cov = L @ L.T + 0.01 * np.eye(3)
        theta[g] = np.concatenate([rng.uniform(-0.6, 0.6, 3), cov[np.triu_indices(3)], [rng.uniform(0.5, 1.5)]])
    star = theta * (1.0 + 0.1 * rng.uniform(-1, 1, theta.shape))
    u = rng.normal(size=(64, 3))
    o = 4.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    d = rng.uniform(-0.5, 0.5, (64, 3)) - o
    o, d = o.astype(np.float32), normalized_f32(d.astype(np.float32))
    theta, star = theta.astype(np.float32).astype(np.float64), star.astype(np.float32).astype(np.float64)
    for t in (theta, star):
        assert np.all(np.linalg.eigvalsh(sym(t[:, 3:9])) > 1e-3)
    return theta, star, o.astype(np.float64), d.astype(np.float64), 0.01


# ---- scenes: the oracle's records and probe ----
@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    import pyoracle as O
    from helpers import scene_path
    return O.OracleScene.load_gmm(scene_path(name + ".txt"))


def oracle_from_gaussians(mean, cov6, density, albedo):
    import pyoracle as O
    return O.OracleScene.from_gaussians(mean, cov6, density, albedo, [(0.0, 4.0, 0.0)], [(1.0, 1.0, 1.0)])


def probe(sc, o, d):
    """(hit (n, N) bool, t_enter, t_exit (n, N) f32) of oracle scene `sc` for rays o, d ((n, 3) f32; the Ray
    constructor normalises d): t_enter is clamped to 0 for an origin inside (intersect_direct)."""
    import pyoracle as O
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    out = np.zeros((len(o), sc.num, 4), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    fn, base = O.lib().orc_gaussian_probe, out.ctypes.data
    for r in range(len(o)):
        po, pd = o[r].ctypes.data_as(fp), d[r].ctypes.data_as(fp)
        for i in range(sc.num):
            fn(sc.h, i, po, pd, ctypes.cast(base + 16 * (r * sc.num + i), fp))
    return out[..., 0] != 0, out[..., 1].copy(), out[..., 2].copy()


class Model:
    """The float64 model of one scene along one batch of rays: per-ray, per-Gaussian contributions for either flag."""

    def __init__(self, sc, o, d, tmax):
        n = len(o)
        self.tmax = np.broadcast_to(np.asarray(tmax, np.float32), (n,)).copy()
        hit, te, tx = probe(sc, o, d)
        rec = sc.records().astype(np.float64)
        self.N = rec.shape[0]
        mean, rho, norm, M = rec[:, :3], rec[:, 3], rec[:, 10], sym(rec[:, 4:10])
        with np.errstate(invalid="ignore"):
            a = np.maximum(np.float32(0), te)           # f32, as the device clips
            b = np.minimum(self.tmax[:, None], tx)
            valid = np.isfinite(o).all(1) & (self.tmax > 0)
            dn = normalized_f32(d)
        valid &= np.isfinite(dn).all(1)
        use = hit & (b > a) & valid[:, None]
        o64 = np.where(valid[:, None], o, 0.0).astype(np.float64)
        d64 = np.where(valid[:, None], dn, np.float32([1, 0, 0])).astype(np.float64)
        a64, b64 = np.where(use, a, 0.0).astype(np.float64), np.where(use, b, 1.0).astype(np.float64)
        args = (mean, M, norm, rho, o64, d64, a64, b64, use)
        self.use = use
        self.tau = tau_terms(*args).sum(1)
        self._frozen = contributions(*args, np.zeros_like(use), np.zeros_like(use))
        self._moving = contributions(*args, use & (te > 0), use & (tx <= self.tmax[:, None]))
        for x in (self._frozen, self._moving, self.tau):
            x.setflags(write=False)

    def grad(self, weights=None, moving=True, rows=None):
        """(G64, S), each (N, 10): sum_i w_i contribution_i and sum_i |w_i contribution_i| over rays `rows` (all)."""
        c = self._moving if moving else self._frozen
        w = np.ones(c.shape[0]) if weights is None else np.asarray(weights, np.float64)
        if rows is not None:
            c, w = c[rows], w[rows]
        t = c * w[:, None, None]
        return t.sum(0), np.abs(t).sum(0)


def judge(label, dev, G64, S, bound=BOUND):
    """Prints the measured maxima, then asserts |dev - G64| <= bound * S per component and exact zeros where S = 0."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == G64.shape, (dev.shape, G64.shape)
    err = np.abs(dev - G64)
    with np.errstate(all="ignore"):
        rel = np.where(S > 0, err / S, 0.0)
    nz = int(np.count_nonzero(dev[S == 0]))
    print(f"{label}: max |G_dev - G64| / S = {rel.max():.3e} (bound {bound:.3e}), max |G64| = {np.abs(G64).max():.3e}, "
          f"rows hit {int((S[:, 9] > 0).sum())} of {len(S)}, non-zeros where S = 0: {nz}")
    assert np.all(np.isfinite(dev))
    assert nz == 0
    assert np.all(err <= bound * S), (float(rel.max()), np.argwhere(err > bound * S)[:5].tolist())
    return float(rel.max())
