"""Reference model of the radiance gradient query (Device.radiance_gradient, vr_query_radiance_grad) in float64 numpy,
composed from the models that exist: features_reference.FeatureModel at the n K sample points for the emission part and
profile_reference.ProfileModel for the part through the transmittances. Computed once per case, shared, never modified.

  l = sum_i (sum_c gL_ic L_ic + gA_i opacity_i),  L_ic = sum_k q_ik T_ik sum_{g active at x_ik} m_g(x_ik) f_gc, opacity without f.

With a_ik = q_ik T_ik (0 for an invalid sample), phi_ig = gA_i + sum_c gL_ic f_gc and s_ik = sum_g m_g(x_ik) phi_ig:
  grad_q = T s,  grad_tau = -q T s,  s_abs = sum_g m |phi|
  s_slack = sum m |phi| over the pairs within Q_MARGIN of a cut-off, which either side of an f32 decision may count: such a
            sample has q = 0 in the cases, so it moves nothing but its own grad_q, by at most T s_slack
  features (N, C):  FeatureModel.grads(w, u)'s, with w = a (x) gL and u = a gA formed in float64 and not rounded
  Gaussians (N, 10): FeatureModel.grads(w, u)'s ten columns (Gf, Sf), plus ProfileModel.grad(weights, moving) (Gp, Sp) for
                     the weights the caller hands over: the model's own grad_tau, or the device's (which the device's
                     second pass used, rounded to f32)
T is passed in: the device's tr, which has the profile's bits (or radiance_reference.transmittance for an all-float64
forward). The points, the validity of a sample and the records are radiance_reference's. `reach` widens the set the sums
run over from q <= 9 to q <= reach: a scale (S, s_abs) for samples that sit on a cut-off by construction, where either
side of an f32 decision may be taken (radiance_interval's own chord is q <= 13.5); the gradients themselves are only
meaningful with reach = 9.

`profile_sums`, `sparse_model` and `scales` are the same sums taken Gaussian by Gaussian over the rays that hit it (the samples that are
active for it) through the same functions, grad_reference.contributions and features_reference.contributions: what
ProfileModel and FeatureModel form for every (ray, Gaussian), they form for the pairs that contribute. They serve where
the dense models cost too much (65 537 rays, the comb's 256 Gaussians) and as the absolute-sum scales of the comparisons
against the device's own composition; tests/test_radiance_grad_reference.py holds them to the dense models.
"""
import functools
import types

import numpy as np

import features_reference as FR
import grad_reference as GR
import profile_reference as PR
import radiance_reference as RR
import sigma_grad_reference as SR

FAR = 1.0e6  # an invalid sample's stand-in point: in no ellipsoid, with weight 0


class RadianceGradModel:
    def __init__(self, sc, o, d, t, q, f, T, gL, gA, unit=False, reach=9.0):
        self.sc = sc
        self.o, self.d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = len(self.o)
        t = np.asarray(t, np.float32)
        self.t = np.ascontiguousarray(np.broadcast_to(t, (n, t.shape[-1])))
        self.K = K = self.t.shape[1]
        self.q = np.ones((n, K)) if q is None else np.broadcast_to(np.asarray(q, np.float64), (n, K))
        self.f = np.asarray(f, np.float32)
        self.C = C = self.f.shape[1]
        self.T = np.asarray(T, np.float64)
        gL = np.ones((n, C)) if gL is None else np.asarray(gL, np.float64)
        gA = np.zeros(n) if gA is None else np.asarray(gA, np.float64)
        self.valid = RR.valid_samples(self.t)
        dn = self.d if unit else GR.normalized_f32(self.d)
        x = np.where(self.valid[..., None], RR.points_f32(self.o, dn, np.where(self.valid, self.t, 0)), np.float32(FAR))
        rec = SR.records_of_oracle(sc.records())
        self.N = len(rec[0])
        pts = SR.Model(rec, x.reshape(-1, 3))
        self.near = pts.near.reshape(n, K) & self.valid
        if reach != 9.0:
            pts = types.SimpleNamespace(rec=rec, x=pts.x, n=pts.n, N=pts.N, active=pts.q <= reach)
        self.pairs = int(pts.active.sum())
        self.a = np.where(self.valid, self.q * self.T, 0.0)
        w = (self.a[:, :, None] * gL[:, None, :]).reshape(-1, C)
        u = (self.a * gA[:, None]).reshape(-1)
        fm = FR.FeatureModel(pts, self.f)
        (self.Gf, self.Sf), (self.Gr, self.Sr), _ = fm.grads(w, u)
        # s = gL . F + gA mass; s_abs = sum_g m |phi|, block by block
        phi = gA[:, None] + gL @ self.f.astype(np.float64).T  # (n, N)
        s64, s_abs, slack = np.zeros(n * K), np.zeros(n * K), np.zeros(n * K)
        ray = np.repeat(np.arange(n), K)
        for k in range(0, n * K, SR.CHUNK):
            sl = slice(k, k + SR.CHUNK)
            m, qg = SR.mass(rec, pts.x[sl], pts.active[sl])
            s64[sl], s_abs[sl] = (m * phi[ray[sl]]).sum(1), (np.abs(m) * np.abs(phi[ray[sl]])).sum(1)
            edge = np.where(np.abs(qg - 9.0) <= SR.Q_MARGIN, np.abs(rec[3] * rec[2] * np.exp(-0.5 * np.minimum(qg, 700.0))), 0.0)
            slack[sl] = (edge * np.abs(phi[ray[sl]])).sum(1)
        self.s64 = np.where(self.valid, s64.reshape(n, K), 0.0)
        self.s_abs = np.where(self.valid, s_abs.reshape(n, K), 0.0)
        self.s_slack = np.where(self.valid, slack.reshape(n, K), 0.0)  # what the pairs within Q_MARGIN of a cut-off could add to s
        self.grad_q = self.T * self.s64
        self.grad_tau = -self.a * self.s64
        self._profile = None
        for a in (self.t, self.valid, self.near, self.a, self.Gf, self.Sf, self.Gr, self.Sr, self.s64, self.s_abs, self.grad_q,
                  self.grad_tau):
            a.setflags(write=False)

    def profile(self, weights=None, moving=True):
        """(Gp, Sp), each (N, 10): ProfileModel.grad for `weights` (None: the model's own grad_tau)."""
        if self._profile is None:
            self._profile = PR.ProfileModel(self.sc, self.o, self.d, self.t)
        w = self.grad_tau if weights is None else np.where(self.valid, np.asarray(weights, np.float64), 0.0)
        return self._profile.grad(w, moving)


def case_inputs(name, n, K, C, rows=None):
    """(o, d, t, q, f, gL, gA) of a radiance_reference case: its rays, samples and features, the radiance model's weights
    (a sample within Q_MARGIN of a cut-off has q = 0; at most 1 % of them, asserted when that model is built) and
    features_reference's signed output weights. rows: the first `rows` rays of the case."""
    o, d = RR.case_rays(name, n)
    mdl = RR.model(name, n, K, C)
    gL, gA = FR.signed_weights(n, C)
    r = slice(0, n if rows is None else rows)
    return tuple(np.ascontiguousarray(a[r]) for a in (o, d, mdl.t, mdl.weights)) + (mdl.f,) + tuple(np.ascontiguousarray(a[r]) for a in (gL, gA))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return GR.oracle_scene(name)


def model(name, n, K, C, T, rows=None):
    """The model of a case for the device's T (not cached: T is the caller's)."""
    o, d, t, q, f, gL, gA = case_inputs(name, n, K, C, rows)
    return RadianceGradModel(_oracle(name), o, d, t, q, f, T, gL, gA)


def _chords(sc, o, d, unit, chords):
    """(hit (n, N), t0 (unclamped entry or the clamped one), te = max(0, entry), tx): the oracle's f32 probe, or the
    roots of q(t) = 9 in float64 (a scale needs no f32 decision, and the probe costs a call per (ray, Gaussian))."""
    if chords == "oracle":
        assert not unit
        if len(o) * sc.num <= 1 << 19:
            hit, te, tx = GR.probe(sc, o, d)
        else:  # the probe of the pairs whose line comes near the ellipsoid in float64 (q_min <= 9.01); the others miss
            import ctypes
            import pyoracle as O
            rec = sc.records().astype(np.float64)
            A, B, C, _, _ = GR.quadratic(rec[:, :3], GR.sym(rec[:, 4:10]), np.asarray(o, np.float64), GR.normalized_f32(d).astype(np.float64))
            o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
            out = np.zeros((len(o), sc.num, 4), np.float32)
            fp = ctypes.POINTER(ctypes.c_float)
            fn, base = O.lib().orc_gaussian_probe, out.ctypes.data
            for r, i in np.argwhere(C - B * B / (4.0 * A) <= 9.01):
                fn(sc.h, int(i), o[r].ctypes.data_as(fp), d[r].ctypes.data_as(fp), ctypes.cast(base + 16 * (int(r) * sc.num + int(i)), fp))
            hit, te, tx = out[..., 0] != 0, out[..., 1].copy(), out[..., 2].copy()
        return hit, te, np.maximum(np.float32(0), te), tx
    rec = sc.records().astype(np.float64)
    dn = (np.asarray(d, np.float32) if unit else GR.normalized_f32(d)).astype(np.float64)
    A, B, C, _, _ = GR.quadratic(rec[:, :3], GR.sym(rec[:, 4:10]), np.asarray(o, np.float64), dn)
    with np.errstate(all="ignore"):
        disc = B * B - 4.0 * A * (C - 9.0)
        root = np.sqrt(np.where(disc > 0, disc, 0.0))
        t0, t1 = (-B - root) / (2.0 * A), (-B + root) / (2.0 * A)
        hit = (disc > 0) & (t1 > 0)
    return hit, t0, np.maximum(0.0, t0), t1


def profile_sums(sc, o, d, t, weights, moving=True, unit=False, chords="oracle"):
    """(G, S), each (N, 10): ProfileModel.grad(weights, moving)'s sums, Gaussian by Gaussian over the rays that hit it."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    n = len(o)
    t = np.broadcast_to(np.asarray(t, np.float32), (n, np.shape(t)[-1]))
    K = t.shape[1]
    w = np.asarray(weights, np.float64)
    rec = sc.records().astype(np.float64)
    mean, rho, norm, M = rec[:, :3], rec[:, 3], rec[:, 10], GR.sym(rec[:, 4:10])
    with np.errstate(all="ignore"):
        dn = d if unit else GR.normalized_f32(d)
        ray_ok = np.isfinite(o).all(1) & np.isfinite(dn).all(1)
    hit, t0, te, tx = _chords(sc, np.where(ray_ok[:, None], o, 0), np.where(ray_ok[:, None], d, np.float32([1, 0, 0])), unit, chords)
    hit = hit & ray_ok[:, None]
    G, S = np.zeros((len(rec), 10)), np.zeros((len(rec), 10))
    for g in range(len(rec)):
        rows = np.nonzero(hit[:, g])[0]
        if not len(rows):
            continue
        tk = t[rows]
        with np.errstate(invalid="ignore"):
            a = np.broadcast_to(te[rows, g, None], tk.shape)
            b = np.minimum(tk, tx[rows, g, None])
            use = (b > a) & (tk > 0)
            mv_in = use & (t0[rows, g, None] > 0) & moving
            mv_out = use & (tx[rows, g, None] <= tk) & moving
        flat = lambda v: np.ascontiguousarray(v).reshape(-1, 1)  # noqa: E731
        c = GR.contributions(mean[g:g + 1], M[g:g + 1], norm[g:g + 1], rho[g:g + 1], np.repeat(o[rows].astype(np.float64), K, 0),
                             np.repeat(dn[rows].astype(np.float64), K, 0), flat(np.where(use, a, 0.0).astype(np.float64)),
                             flat(np.where(use, b, 1.0).astype(np.float64)), flat(use), flat(mv_in), flat(mv_out))
        term = c[:, 0, :] * np.where(use, w[rows], 0.0).reshape(-1, 1)
        G[g], S[g] = term.sum(0), np.abs(term).sum(0)
    return G, S


def near_samples(sc, o, d, t, unit=False, margin=SR.Q_MARGIN):
    """(n, K) bool: the valid samples with some |q - 9| <= margin, the ones a case gives q = 0 (radiance_reference's rule)."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float32), (len(o), np.shape(t)[-1])))
    with np.errstate(all="ignore"):
        dn = d if unit else GR.normalized_f32(d)
        ok = RR.valid_samples(t) & (np.isfinite(o).all(1) & np.isfinite(dn).all(1))[:, None]
        x = np.where(ok[..., None], RR.points_f32(np.where(np.isfinite(o), o, 0), np.where(np.isfinite(dn), dn, 0), np.where(ok, t, 0)),
                     np.float32(FAR)).reshape(-1, 3).astype(np.float64)
    rec = SR.records_of_oracle(sc.records())
    near = np.concatenate([np.any(np.abs(SR.quadratic(rec, x[k:k + SR.CHUNK])[2] - 9.0) <= margin, axis=1) for k in range(0, len(x), SR.CHUNK)])
    return near.reshape(t.shape) & ok


def sparse_model(sc, o, d, t, q, f, T, gL, gA, unit=False, margin=SR.Q_MARGIN, reach=9.0):
    """RadianceGradModel's sums taken pair by pair, as a namespace: Gf, Sf (N, 10), Gr, Sr (N, C), s64, s_abs, s_slack (n, K),
    grad_q, grad_tau, near (n, K) (a sample with a pair within `margin` of the cut-off), T, q, valid, N, C. An invalid ray
    has no valid sample. reach: the sums run over q <= reach (9: the model; more: a scale only)."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = len(o)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float32), (n, np.shape(t)[-1])))
    K = t.shape[1]
    f = np.asarray(f, np.float32)
    C = f.shape[1]
    qq = np.ones((n, K)) if q is None else np.broadcast_to(np.asarray(q, np.float64), (n, K))
    gL = np.ones((n, C)) if gL is None else np.asarray(gL, np.float64)
    gA = np.zeros(n) if gA is None else np.asarray(gA, np.float64)
    with np.errstate(all="ignore"):
        dn = d if unit else GR.normalized_f32(d)
        ok = RR.valid_samples(t) & (np.isfinite(o).all(1) & np.isfinite(dn).all(1))[:, None]
        T = np.where(ok, np.asarray(T, np.float64), 0.0)
        a = np.where(ok, qq * T, 0.0).reshape(-1)
        x = np.where(ok[..., None], RR.points_f32(np.where(np.isfinite(o), o, 0), np.where(np.isfinite(dn), dn, 0), np.where(ok, t, 0)),
                     np.float32(FAR)).reshape(-1, 3).astype(np.float64)
    rec = SR.records_of_oracle(sc.records())
    N = len(rec[0])
    active, edge = [], []
    for k in range(0, len(x), SR.CHUNK):
        p, _, v = SR.quadratic(rec, x[k:k + SR.CHUNK])
        active.append(v <= reach)
        # margin None: the pair's own bound on an f32 evaluation of q, 2^-20 sum_ij |M_ij| |p_i| |p_j| (vr_radiance_interval.h has
        # the count), where that is more than Q_MARGIN: for samples that sit on cut-offs, where any error decides
        width = margin if margin is not None else np.maximum(SR.Q_MARGIN, 2.0 ** -20 * np.einsum("ngi,gij,ngj->ng", np.abs(p), np.abs(rec[1]), np.abs(p)))
        edge.append(np.abs(v - 9.0) <= width)
    active, edge = np.concatenate(active), np.concatenate(edge)
    ray = np.repeat(np.arange(n), K)
    Sf, Sr, s_abs, slack = np.zeros((N, 10)), np.zeros((N, C)), np.zeros(n * K), np.zeros(n * K)
    Gf, Gr, s64 = np.zeros((N, 10)), np.zeros((N, C)), np.zeros(n * K)
    for g in range(N):
        rec_g = tuple(r[g:g + 1] for r in rec)
        idx = np.nonzero(edge[:, g])[0]
        if len(idx):
            phi = gA[ray[idx]] + gL[ray[idx]] @ f[g].astype(np.float64)
            slack[idx] += np.abs(SR.mass(rec_g, x[idx], np.ones((len(idx), 1), bool))[0][:, 0] * phi)
        idx = np.nonzero(active[:, g])[0]
        if not len(idx):
            continue
        on = np.ones((len(idx), 1), bool)
        cg, cf, _ = FR.contributions(rec_g, x[idx], f[g:g + 1], a[idx, None] * gL[ray[idx]], a[idx] * gA[ray[idx]], on)
        Sf[g], Sr[g] = np.abs(cg).sum((0, 1)), np.abs(cf).sum((0, 1))
        Gf[g], Gr[g] = cg.sum((0, 1)), cf.sum((0, 1))
        phi = gA[ray[idx]] + gL[ray[idx]] @ f[g].astype(np.float64)
        m = SR.mass(rec_g, x[idx], on)[0][:, 0]
        s_abs[idx] += np.abs(m * phi)
        s64[idx] += m * phi
    s64, s_abs, slack = s64.reshape(n, K), s_abs.reshape(n, K), slack.reshape(n, K)
    return types.SimpleNamespace(Gf=Gf, Sf=Sf, Gr=Gr, Sr=Sr, s64=s64, s_abs=s_abs, s_slack=slack, near=edge.any(1).reshape(n, K) & ok,
                                 grad_q=T * s64, grad_tau=-a.reshape(n, K) * s64, T=T, q=np.where(ok, qq, 0.0), valid=ok, N=N, C=C,
                                 pairs=int(active.sum()))


def scales(sc, o, d, t, q, f, T, gL, gA, grad_tau, unit=False, reach=9.0, moving=True):
    """(Sf (N, 10), Sr (N, C), Sp (N, 10), s_abs (n, K)): the absolute sums of RadianceGradModel and of
    ProfileModel.grad(grad_tau), over the pairs with q <= reach and float64 chords: scales, not references."""
    m = sparse_model(sc, o, d, t, q, f, np.nan_to_num(np.asarray(T, np.float64)), gL, gA, unit, reach=reach)
    gt = np.where(m.valid, np.nan_to_num(np.asarray(grad_tau, np.float64)), 0.0)
    return m.Sf, m.Sr, profile_sums(sc, o, d, t, gt, moving, unit, chords="float64")[1], m.s_abs
