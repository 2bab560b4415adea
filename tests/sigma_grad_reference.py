"""Reference model of the sigma gradient query (Device.query_sigma_grad, vr_query_sigma_grad): the formulas of
include/vr_hip.h in float64 numpy. Computed once per case, shared, never modified.

The function differentiated: sigma_s(x) = sum alpha_g m_g(x), sigma_a(x) = sum (1 - alpha_g) m_g(x) over the active set
{g : q_g(x) <= 9}, with p = x - mean, q = p.Mp, e = norm exp(-q / 2), m = rho e. For a scene the records (mean, rho, M,
norm, alpha in f32) come from the oracle scene and are read as doubles, as the device reads its own; the active set is
the model's own float64 decision, which is the device's f32 one for every point the tests keep (`near` drops the points
within 9e-4 of a cut-off, the f32 error of q, as the forward sigma test does). The CPU test checks the same functions
against central differences of `sigma`, there with float64 records built from the parameters.

Row layout per Gaussian (11): d/d mean[3], d/d cov6 {xx, xy, xz, yy, yz, zz} (off-diagonal: the stored number stands
at (i, j) and (j, i), hence 2 G_Sigma[i][j]), d/d density, d/d albedo. Per point (3): d/d x.
With weights w = (w_a, w_s) per point and c = w_a (1 - alpha) + w_s alpha, per active (point, Gaussian):
  mean: c m M p;   G_Sigma = -M G_M M - T M / 2 with G_M = -c m p p^T / 2 and T = c m, i.e. c m ((Mp)(Mp)^T - M) / 2;
  density: c e;   albedo: (w_s - w_a) m;   x: -c m M p.
A point whose sum of m is <= 0 contributes nothing (the forward's (0, 0)).
"""
import functools

import numpy as np

BOUND = 2.0 ** -21  # |dev - model| <= BOUND * S per component: the final f32 rounding is 2^-24 S; 8x for the device's double exp
Q_MARGIN = 9e-4     # the forward sigma test's margin for the f32 error of q
CHUNK = 4096        # points per block of the (point, Gaussian) arrays


def sym(m6):
    """(..., 6) {00 01 02 11 12 22} -> (..., 3, 3)."""
    m6 = np.asarray(m6)
    return np.stack([np.stack([m6[..., 0], m6[..., 1], m6[..., 2]], -1), np.stack([m6[..., 1], m6[..., 3], m6[..., 4]], -1),
                     np.stack([m6[..., 2], m6[..., 4], m6[..., 5]], -1)], -2)


def records_of(theta):
    """(mean (N, 3), M (N, 3, 3), norm, rho, alpha (N,)) float64 of theta rows mean[3], cov6[6], density, albedo
    (gaussian.h:50-55)."""
    cov = sym(theta[:, 3:9])
    return theta[:, 0:3], np.linalg.inv(cov), (2.0 * np.pi) ** -1.5 * np.linalg.det(cov) ** -0.5, theta[:, 9], theta[:, 10]


def records_of_oracle(rec):
    """The same tuple from the oracle's (N, 12) f32 rows: mean[3], rho, M6, norm, alpha."""
    rec = np.asarray(rec).astype(np.float64)
    return rec[:, :3], sym(rec[:, 4:10]), rec[:, 10], rec[:, 3], rec[:, 11]


def quadratic(rec, x):
    """p (n, N, 3), Mp (n, N, 3), q (n, N) for points x (n, 3)."""
    mean, M = rec[0], rec[1]
    p = np.asarray(x, np.float64)[:, None, :] - mean[None]
    Mp = np.einsum("gij,ngj->ngi", M, p)
    return p, Mp, np.einsum("ngi,ngi->ng", p, Mp)


def mass(rec, x, active=None):
    """m (n, N) float64 over the active set (q <= 9 unless given), 0 elsewhere; also q."""
    _, _, q = quadratic(rec, x)
    act = q <= 9.0 if active is None else active
    return np.where(act, rec[3] * rec[2] * np.exp(-0.5 * q), 0.0), q


def sigma(rec, x, active=None):
    """(n, 2) float64 (sigma_a, sigma_s): the function the gradient is of."""
    m, _ = mass(rec, x, active)
    live = (m.sum(1) > 0)[:, None]
    return np.where(live, np.stack([(m * (1.0 - rec[4])).sum(1), (m * rec[4]).sum(1)], 1), 0.0)


def contributions(rec, x, w, active=None):
    """(per Gaussian (n, N, 11), per point (n, N, 3)) float64: the weighted gradient's terms per (point, Gaussian), after
    the conversion to covariance space. w (n, 2) = (w_a, w_s)."""
    mean, M, norm, rho, alpha = rec
    p, Mp, q = quadratic(rec, x)
    act = q <= 9.0 if active is None else active
    e = norm * np.exp(-0.5 * q)
    m = rho * e
    act = act & (np.where(act, m, 0.0).sum(1) > 0)[:, None]
    w = np.asarray(w, np.float64)
    c = w[:, 0:1] * (1.0 - alpha) + w[:, 1:2] * alpha
    cm = c * m
    GS = 0.5 * cm[..., None, None] * (Mp[..., :, None] * Mp[..., None, :] - M[None])
    gmean = cm[..., None] * Mp
    g = np.stack([gmean[..., 0], gmean[..., 1], gmean[..., 2], GS[..., 0, 0], 2.0 * GS[..., 0, 1], 2.0 * GS[..., 0, 2],
                  GS[..., 1, 1], 2.0 * GS[..., 1, 2], GS[..., 2, 2], c * e, (w[:, 1:2] - w[:, 0:1]) * m], -1)
    return np.where(act[..., None], g, 0.0), np.where(act[..., None], -gmean, 0.0)


def recipe_points(rec, n, seed=7):
    """The tests' points, (n, 3) f32: point i belongs to Gaussian g = i mod N, x = mean_g + chol(M_g^-1) (r u) with u a
    uniform direction and r uniform in [0, 3.3], in float64, rounded to f32. Every Gaussian holds points, some 9 % lie
    just outside their own ellipsoid, and overlaps give several active Gaussians per point."""
    mean, M = rec[0], rec[1]
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = rng.uniform(0.0, 3.3, n)
    g = np.arange(n) % len(mean)
    L = np.linalg.cholesky(np.linalg.inv(M))
    return (mean[g] + np.einsum("nij,nj->ni", L[g], r[:, None] * u)).astype(np.float32)


class Model:
    """The float64 model of one set of records at one batch of points. Holds q, the active set and `near`; the
    (point, Gaussian) terms are formed block by block for each set of weights."""

    def __init__(self, rec, x):
        self.rec = rec
        self.x = np.ascontiguousarray(x, np.float32)
        self.n, self.N = len(self.x), len(rec[0])
        q = np.concatenate([quadratic(rec, self.x[k:k + CHUNK])[2] for k in range(0, self.n, CHUNK)]) if self.n else np.zeros((0, self.N))
        self.q = q
        self.active = q <= 9.0
        self.n_active = self.active.sum(1)
        self.near = np.any(np.abs(q - 9.0) <= Q_MARGIN, axis=1)
        for a in (self.x, self.q, self.active, self.n_active, self.near):
            a.setflags(write=False)

    def _weights(self, weights):
        return np.ones((self.n, 2)) if weights is None else np.asarray(weights, np.float64)

    def both(self, weights=None):
        """((G, S) (N, 11), (Gx, Sx) (n, 3)): the sums of the terms and of their absolute values, per Gaussian over
        the points and per point over the Gaussians."""
        w = self._weights(weights)
        G, S = np.zeros((self.N, 11)), np.zeros((self.N, 11))
        Gx, Sx = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        for k in range(0, self.n, CHUNK):
            s = slice(k, k + CHUNK)
            cg, cx = contributions(self.rec, self.x[s], w[s], self.active[s])
            G += cg.sum(0)
            S += np.abs(cg).sum(0)
            Gx[s], Sx[s] = cx.sum(1), np.abs(cx).sum(1)
        return (G, S), (Gx, Sx)

    def grad(self, weights=None):
        return self.both(weights)[0]

    def grad_xyz(self, weights=None):
        return self.both(weights)[1]


def kept_recipe(rec, n_draw, n_keep=None):
    """A Model at the recipe's points after the boundary exclusion: n_draw points are drawn, those within Q_MARGIN of a
    cut-off dropped (at most 1 %, asserted) and, if n_keep is given, the first n_keep of the rest kept."""
    x = recipe_points(rec, n_draw)
    near = Model(rec, x).near
    assert near.mean() <= 0.01, (int(near.sum()), n_draw)
    x = x[~near]
    if n_keep is not None:
        assert len(x) >= n_keep
        x = x[:n_keep]
    mdl = Model(rec, x)
    assert not mdl.near.any()
    mdl.dropped = int(near.sum())
    return mdl


@functools.lru_cache(maxsize=None)
def signed_weights(n):
    """(n, 2) f32 uniform in (-1, 1)^2, read-only."""
    w = np.random.default_rng(7).uniform(-1, 1, (n, 2)).astype(np.float32)
    w.setflags(write=False)
    return w


def judge(label, dev, G64, S, bound=BOUND):
    """Prints the measured maximum, then asserts |dev - G64| <= bound * S per component and exact zeros where S = 0."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == G64.shape, (dev.shape, G64.shape)
    err = np.abs(dev - G64)
    with np.errstate(all="ignore"):
        rel = np.where(S > 0, err / S, 0.0)
    nz = int(np.count_nonzero(dev[S == 0]))
    print(f"{label}: max |dev - model| / S = {rel.max() if rel.size else 0.0:.3e} (bound {bound:.3e}), max |model| = "
          f"{np.abs(G64).max() if G64.size else 0.0:.3e}, rows with S > 0: {int((S > 0).any(1).sum())} of {len(S)}, "
          f"non-zeros where S = 0: {nz}")
    assert np.all(np.isfinite(dev))
    assert nz == 0
    assert np.all(err <= bound * S), (float(rel.max()), np.argwhere(err > bound * S)[:5].tolist())
    return float(rel.max()) if rel.size else 0.0
