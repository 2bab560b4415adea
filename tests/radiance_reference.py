"""Reference model of the radiance query (Device.radiance, vr_query_radiance) in float64 numpy, and the cases its tests share.
Computed once per case, shared, never modified.

  L[i, c]    = sum_{k valid} q_ik T_ik sum_{g active at x_ik} m_g(x_ik) f_gc
  opacity[i] = the same without f
  S, S_op    = the sums of the absolute values of the same terms

The sample points are the definition's f32 points: d = grad_reference.normalized_f32(directions), x = o + t * d with one
f32 multiply and one f32 add per component. At those points q_g(x), the active set {q <= 9} and m are
sigma_grad_reference's (records from the oracle scene read as doubles). T is the oracle's: the reference's own f32
optical depth (aniso_cases.tau_ref_f32, gaussian.h:208-231 operation for operation) over the oracle's f32 chord clipped
to [max(0, t_enter), min(t, t_exit)], summed in double, rounded to f32 and put through exp(-tau) in f32 (gmm.h:517-578),
the protocol of the finite-tmax tests: vr_query_transmittance is defined as that arithmetic and the profile has its bits.
The float64 closed form (grad_reference.tau_terms, `transmittance`) is kept beside it as T64, L64 and opacity64: the
reference's f32 optical depth itself lies up to 1.8e-4 (relative, in T) from it on 1_gaussian, through the cancellation in
C - B^2 / 4A for origins 2 to 5 units away, so a bound on the query against an all-float64 model would be a bound on the
reference's arithmetic. A sample is valid iff t is finite and >= 0; a sample that is not > 0 has T = 1.

A sample whose point lies within Q_MARGIN of any ellipsoid (|q - 9| <= 9e-4, the f32 error of q) gets q = 0 on both
sides: `weights` is the caller's q with those entries zeroed, the array the device is given, so the pairs of such a
sample contribute exactly 0 whatever either side decides. At most 1 % of a case's samples may be zeroed (asserted here).
"""
import functools

import numpy as np

import grad_reference as GR
import sigma_grad_reference as SR

CAP = 0.01
ROWS = 64  # rays per block of the (sample, Gaussian) arrays


def points_f32(o, dn, t):
    """(n, K, 3) f32: o + t * dn, per component one f32 multiply and then one f32 add."""
    o, dn, t = np.asarray(o, np.float32), np.asarray(dn, np.float32), np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        prod = (t[:, :, None] * dn[:, None, :]).astype(np.float32)
        return (o[:, None, :] + prod).astype(np.float32)


def valid_samples(t):
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & (t >= 0)


def features_of(N, C, seed=7):
    """(N, C) f32, read-only: uniform in (-1, 1) by default_rng(seed); channel 1 (if there is one) is 1."""
    f = np.random.default_rng(seed).uniform(-1, 1, (N, C)).astype(np.float32)
    if C > 1:
        f[:, 1] = 1.0
    f.setflags(write=False)
    return f


def transmittance(sc, o, d, t):
    """(n, K) float64: exp(-tau) at the samples, tau in closed form over the oracle's chords."""
    rec = sc.records().astype(np.float64)
    mean, rho, norm, M = rec[:, :3], rec[:, 3], rec[:, 10], GR.sym(rec[:, 4:10])
    hit, te, tx = GR.probe(sc, o, d)
    dn = GR.normalized_f32(d)
    o64, d64 = np.asarray(o, np.float64), dn.astype(np.float64)
    T = np.ones(t.shape)
    for k in range(t.shape[1]):
        tk = t[:, k]
        with np.errstate(invalid="ignore"):
            a = np.maximum(np.float32(0), te)
            b = np.minimum(tk[:, None], tx)
            use = hit & (b > a) & (tk > 0)[:, None]
        a64, b64 = np.where(use, a, 0.0).astype(np.float64), np.where(use, b, 1.0).astype(np.float64)
        T[:, k] = np.exp(-GR.tau_terms(mean, M, norm, rho, o64, d64, a64, b64, use).sum(1))
    return T


def transmittance_f32(sc, o, d, t):
    """(n, K) float64 holding f32 values: the reference's own f32 transmittance at the samples (see the module's head)."""
    import aniso_cases as AC
    rec = sc.records()
    hit, te, tx = GR.probe(sc, o, d)
    T = np.ones(t.shape)
    for k in range(t.shape[1]):
        tk = t[:, k]
        with np.errstate(invalid="ignore"):
            a = np.maximum(np.float32(0), te)
            b = np.minimum(tk[:, None], tx)
            use = hit & (b > a) & (tk > 0)[:, None]
        with np.errstate(all="ignore"):
            terms = AC.tau_ref_f32(rec, o, d, np.where(use, a, np.float32(0)), np.where(use, b, np.float32(1)))
        tau = np.where(use, terms.astype(np.float64), 0.0).sum(1).astype(np.float32)
        T[:, k] = np.exp(-tau).astype(np.float32)
    return T


class RadianceModel:
    def __init__(self, sc, o, d, t, q, f):
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = len(o)
        t = np.asarray(t, np.float32)
        self.t = np.ascontiguousarray(np.broadcast_to(t, (n, t.shape[-1])))
        self.K = K = self.t.shape[1]
        q = np.ones((n, K), np.float32) if q is None else np.broadcast_to(np.asarray(q, np.float32), (n, K))
        self.f = f = np.asarray(f, np.float32)
        self.C = C = f.shape[1]
        rec = SR.records_of_oracle(sc.records())
        self.N = len(rec[0])
        assert np.isfinite(o).all() and np.isfinite(GR.normalized_f32(d)).all()  # (the model's rays are valid)
        self.x = points_f32(o, GR.normalized_f32(d), self.t)
        self.valid = valid_samples(self.t)
        self.T, self.T64 = transmittance_f32(sc, o, d, self.t), transmittance(sc, o, d, self.t)
        f64, fabs = f.astype(np.float64), np.abs(f.astype(np.float64))
        mf, mabs, ms, msabs = np.zeros((n, K, C)), np.zeros((n, K, C)), np.zeros((n, K)), np.zeros((n, K))
        near, pairs = np.zeros((n, K), bool), np.zeros((n, K), np.int64)
        for r in range(0, n, ROWS):
            s = slice(r, r + ROWS)
            ok = self.valid[s].reshape(-1)
            x = np.where(ok[:, None], self.x[s].reshape(-1, 3), 0.0)
            m, qg = SR.mass(rec, x)
            m = np.where(ok[:, None], m, 0.0)
            shape = self.t[s].shape
            mf[s], mabs[s] = (m @ f64).reshape(shape + (C,)), (np.abs(m) @ fabs).reshape(shape + (C,))
            ms[s], msabs[s] = m.sum(1).reshape(shape), np.abs(m).sum(1).reshape(shape)
            near[s] = (ok & np.any(np.abs(qg - 9.0) <= SR.Q_MARGIN, axis=1)).reshape(shape)
            pairs[s] = (ok[:, None] & (qg <= 9.0)).sum(1).reshape(shape)
        self.near, self.pairs = near, pairs
        self.zeroed = float(near.sum()) / max(1, int(self.valid.sum()))
        assert self.zeroed <= CAP, (int(near.sum()), int(self.valid.sum()))
        self.weights = np.ascontiguousarray(np.where(near, np.float32(0), q).astype(np.float32))
        w = np.where(self.valid, self.weights.astype(np.float64), 0.0) * self.T
        self.L, self.S = np.einsum("nk,nkc->nc", w, mf), np.einsum("nk,nkc->nc", np.abs(w), mabs)
        self.opacity, self.S_op = (w * ms).sum(1), (np.abs(w) * msabs).sum(1)
        w64 = np.where(self.valid, self.weights.astype(np.float64), 0.0) * self.T64
        self.L64, self.opacity64 = np.einsum("nk,nkc->nc", w64, mf), (w64 * ms).sum(1)
        for a in (self.t, self.x, self.valid, self.T, self.T64, self.L64, self.opacity64, self.near, self.pairs, self.weights, self.L, self.S, self.opacity, self.S_op):
            a.setflags(write=False)


def literal(sc, o, d, t, q, f):
    """(L, opacity, S) by a per-sample, per-Gaussian loop, for small cases: the definition read line by line."""
    rec = sc.records().astype(np.float64)
    dn = GR.normalized_f32(d)
    n, K = t.shape
    T = transmittance_f32(sc, o, d, t)
    L, A, S = np.zeros((n, f.shape[1])), np.zeros(n), np.zeros((n, f.shape[1]))
    for i in range(n):
        for k in range(K):
            tk = t[i, k]
            if not (np.isfinite(tk) and tk >= 0):
                continue
            x = (o[i] + (tk * dn[i]).astype(np.float32)).astype(np.float32).astype(np.float64)
            for g in range(len(rec)):
                p = x - rec[g, :3]
                M = GR.sym(rec[g, 4:10])
                qg = p @ M @ p
                if qg <= 9.0:
                    term = float(q[i, k]) * T[i, k] * rec[g, 3] * rec[g, 10] * np.exp(-0.5 * qg)
                    L[i] += term * f[g].astype(np.float64)
                    S[i] += abs(term) * np.abs(f[g].astype(np.float64))
                    A[i] += term
    return L, A, S


# ---- the cases: rays by the profile tests' recipe, samples in random order with repeats, signed weights ----
@functools.lru_cache(maxsize=None)
def case_rays(name, n):
    """(origins, directions) f32, read-only: 1_gaussian: one_gaussian_case's 257 rays; else sphere_rays(name, n)."""
    from test_gpu_query_grad import one_gaussian_case, sphere_rays
    if name == "1_gaussian":
        o, d, _ = one_gaussian_case()
        assert n == len(o)
    else:
        o, d, _ = sphere_rays(name, n)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    for a in (o, d):
        a.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def case_samples(name, n, K):
    """(t, q), each (n, K) f32, read-only. default_rng(23): t = U(0, 1) x 2 |centre - o| per ray, unsorted, with column 2
    repeated in column 0 when K >= 3; q = U(-1, 1) x the ray's mean spacing."""
    o, _ = case_rays(name, n)
    m = GR.oracle_scene(name).records()[:, :3].astype(np.float64)
    c = 0.5 * (m.min(0) + m.max(0))
    reach = 2.0 * np.linalg.norm(c - o.astype(np.float64), axis=1)
    rng = np.random.default_rng(23)
    t = (rng.uniform(0, 1, (n, K)) * reach[:, None]).astype(np.float32)
    if K >= 3:
        t[:, 0] = t[:, 2]
    q = (rng.uniform(-1, 1, (n, K)) * (reach / K)[:, None]).astype(np.float32)
    for a in (t, q):
        a.setflags(write=False)
    return t, q


CASES = (("1_gaussian", 257, 1, 1), ("1_gaussian", 257, 1, 3), ("1_gaussian", 257, 17, 1), ("1_gaussian", 257, 17, 3),
         ("50_random", 1024, 33, 19), ("250_random", 1024, 33, 19))


@functools.lru_cache(maxsize=None)
def model(name, n, K, C):
    sc = GR.oracle_scene(name)
    o, d = case_rays(name, n)
    t, q = case_samples(name, n, K)
    return RadianceModel(sc, o, d, t, q, features_of(sc.num, C))
