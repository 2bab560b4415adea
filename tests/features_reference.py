"""Reference model of the feature query (Device.evaluate_features / Device.features_gradient, vr_query_features[_grad]): the
formulas of include/vr_hip.h in float64 numpy, built on tests/sigma_grad_reference.py (records, active set, the recipe's
points, the bound and `judge` are its own, unmodified). Computed once per case, shared, never modified.

Forward, over the active set {g : q_g(x) <= 9} with m = rho norm exp(-q / 2):
  mass(x) = sum_g m_g(x),   F_c(x) = sum_g m_g(x) f_gc,   both 0 where mass is not > 0.
Gradient of L = sum_i (sum_c w_ic F_ic + u_i mass_i): with c_ig = u_i + sum_c w_ic f_gc, per active (point, Gaussian) of a
point with mass > 0:
  Gaussians (10): mean: c m M p;  cov6: c m ((Mp)(Mp)^T - M) / 2, off-diagonal twice;  density: c e
  features (C):   w_ic m
  points (3):     -c m M p
S is the sum of the absolute values of the same terms (for F: sum_g |m_g f_gc|).
"""
import functools

import numpy as np

from sigma_grad_reference import BOUND, CHUNK, Model, judge, kept_recipe, mass, quadratic, records_of, records_of_oracle  # noqa: F401


def features_of(rec, C, seed=7):
    """(N, C) f32, read-only: uniform in (-1, 1) by default_rng(seed); channel 0 is the records' albedo, channel 1 is 1."""
    f = np.random.default_rng(seed).uniform(-1, 1, (len(rec[0]), C)).astype(np.float32)
    f[:, 0] = rec[4].astype(np.float32)
    if C > 1:
        f[:, 1] = 1.0
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def signed_weights(n, C):
    """(w (n, C), u (n,)) f32 uniform in (-1, 1), read-only."""
    a = np.random.default_rng(7).uniform(-1, 1, (n, C + 1)).astype(np.float32)
    w, u = np.ascontiguousarray(a[:, :C]), np.ascontiguousarray(a[:, C])
    w.setflags(write=False)
    u.setflags(write=False)
    return w, u


def forward(rec, x, f, active=None):
    """(F (n, C), S (n, C), mass (n,), S_mass (n,)) float64."""
    m, _ = mass(rec, x, active)
    f = np.asarray(f, np.float64)
    tot = m.sum(1)
    live = tot > 0
    return (np.where(live[:, None], m @ f, 0.0), np.where(live[:, None], np.abs(m) @ np.abs(f), 0.0), np.where(live, tot, 0.0),
            np.where(live, np.abs(m).sum(1), 0.0))


def loss(rec, x, f, w, u, active=None):
    """L = sum_i (sum_c w_ic F_ic + u_i mass_i), the function the gradient is of."""
    F, _, tot, _ = forward(rec, x, f, active)
    return float((F * w).sum() + (tot * u).sum())


def contributions(rec, x, f, w, u, active=None):
    """(per Gaussian (n, N, 10), per feature (n, N, C), per point (n, N, 3)) float64: the gradient's terms per
    (point, Gaussian), the Gaussians' after the conversion to covariance space."""
    mean, M, norm, rho, _ = rec
    p, Mp, q = quadratic(rec, x)
    act = q <= 9.0 if active is None else active
    e = norm * np.exp(-0.5 * q)
    m = rho * e
    act = act & (np.where(act, m, 0.0).sum(1) > 0)[:, None]
    f, w, u = np.asarray(f, np.float64), np.asarray(w, np.float64), np.asarray(u, np.float64)
    c = u[:, None] + w @ f.T
    cm = c * m
    GS = 0.5 * cm[..., None, None] * (Mp[..., :, None] * Mp[..., None, :] - M[None])
    gmean = cm[..., None] * Mp
    g = np.stack([gmean[..., 0], gmean[..., 1], gmean[..., 2], GS[..., 0, 0], 2.0 * GS[..., 0, 1], 2.0 * GS[..., 0, 2],
                  GS[..., 1, 1], 2.0 * GS[..., 1, 2], GS[..., 2, 2], c * e], -1)
    gf = w[:, None, :] * m[..., None]
    a = act[..., None]
    return np.where(a, g, 0.0), np.where(a, gf, 0.0), np.where(a, -gmean, 0.0)


class FeatureModel:
    """The feature query's float64 model over a sigma_grad_reference.Model (its points, records and active set)."""

    def __init__(self, mdl, f):
        self.mdl, self.f = mdl, f
        self.C = f.shape[1]
        parts = [forward(mdl.rec, mdl.x[k:k + CHUNK], f, mdl.active[k:k + CHUNK]) for k in range(0, mdl.n, CHUNK)]
        if not parts:
            parts = [(np.zeros((0, self.C)), np.zeros((0, self.C)), np.zeros(0), np.zeros(0))]
        self.F, self.S, self.mass, self.S_mass = (np.concatenate([p[i] for p in parts]) for i in range(4))
        for a in (self.F, self.S, self.mass, self.S_mass):
            a.setflags(write=False)

    def weights(self, w, u):
        n = self.mdl.n
        return (np.ones((n, self.C)) if w is None else np.asarray(w, np.float64), np.zeros(n) if u is None else np.asarray(u, np.float64))

    def grads(self, w=None, u=None):
        """((G, S) (N, 10), (Gf, Sf) (N, C), (Gx, Sx) (n, 3)): the sums of the terms and of their absolute values."""
        mdl = self.mdl
        w, u = self.weights(w, u)
        G, S = np.zeros((mdl.N, 10)), np.zeros((mdl.N, 10))
        Gf, Sf = np.zeros((mdl.N, self.C)), np.zeros((mdl.N, self.C))
        Gx, Sx = np.zeros((mdl.n, 3)), np.zeros((mdl.n, 3))
        for k in range(0, mdl.n, CHUNK):
            s = slice(k, k + CHUNK)
            cg, cf, cx = contributions(mdl.rec, mdl.x[s], self.f, w[s], u[s], mdl.active[s])
            G += cg.sum(0)
            S += np.abs(cg).sum(0)
            Gf += cf.sum(0)
            Sf += np.abs(cf).sum(0)
            Gx[s], Sx[s] = cx.sum(1), np.abs(cx).sum(1)
        return (G, S), (Gf, Sf), (Gx, Sx)
