"""The float64 model of the radiance gradient query (tests/radiance_grad_reference.py), on the CPU: its Gaussian, feature and
q gradients against central differences of an all-float64 forward.

The forward is l(theta, f, q) = sum_i (sum_c gL_ic L_ic + gA_i opacity_i) on 1_gaussian with a handful of rays, K = 3 and C = 2:
T = radiance_reference.transmittance (the closed form over the oracle's chords, which are probed once at theta_0 and held:
frozen bounds), m from sigma_grad_reference.mass over the active set held at theta_0's. theta = (mean, cov6, density) in
float64, its records by sigma_grad_reference.records_of; theta_0 is the oracle's record read back (cov = M^-1), so the model
and the forward see the same float64 numbers. The recipe is the other models' (tests/test_query_features_host.py,
tests/test_query_sigma_grad_host.py): step h = 1e-6 max(1, |value|), the active set asserted not to move, and
|model - central difference| <= 1e-5 of the largest component of the column.

Measured here: worst ratio 2.3e-8 for the Gaussians' ten columns, 1.9e-10 for the features' two, 2.8e-9 for q."""
import numpy as np

import features_reference as FR
import grad_reference as GR
import radiance_grad_reference as RG
import radiance_reference as RR
import sigma_grad_reference as SR

NAME, N_RAYS, K, C, ROWS = "1_gaussian", 257, 3, 2, 12


class _Theta:
    """The oracle scene with the records of theta: the probe (the chords) stays the oracle's own."""

    def __init__(self, sc, theta):
        self._sc, self.num, self.h = sc, sc.num, sc.h
        mean, M, norm, rho, _ = SR.records_of(np.concatenate([theta, np.zeros((len(theta), 1))], 1))
        rec = np.zeros((len(theta), 12))
        rec[:, :3], rec[:, 3], rec[:, 10] = mean, rho, norm
        rec[:, 4:10] = np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)
        self._rec = rec

    def records(self):
        return self._rec


def theta_of(sc):
    rec = SR.records_of_oracle(sc.records())
    cov = np.linalg.inv(rec[1])
    return np.concatenate([rec[0], np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1),
                           rec[3][:, None]], 1)


def test_model_matches_central_differences():
    sc = GR.oracle_scene(NAME)
    o, d, t, q, f, gL, gA = RG.case_inputs(NAME, N_RAYS, K, C, rows=ROWS)
    theta0, f0, q0 = theta_of(sc), f.astype(np.float64), q.astype(np.float64)
    at0 = _Theta(sc, theta0)
    mdl = RG.RadianceGradModel(at0, o, d, t, q0, f, RR.transmittance(at0, o, d, t), gL, gA)
    Gp, _ = mdl.profile(None, moving=False)
    G, Gr, Gq = mdl.Gf + Gp, mdl.Gr, mdl.grad_q
    x = RR.points_f32(o, GR.normalized_f32(d), t).reshape(-1, 3)
    active = SR.quadratic(SR.records_of_oracle(at0.records()), x)[2] <= 9.0
    assert active.sum() >= 6 and not mdl.near.any()
    gL64, gA64 = gL.astype(np.float64), gA.astype(np.float64)

    def loss(theta, ft, qs):
        th = _Theta(sc, theta)
        rec = SR.records_of_oracle(th.records())
        assert np.array_equal(SR.quadratic(rec, x)[2] <= 9.0, active)
        m, _ = SR.mass(rec, x, active)
        a = (qs * RR.transmittance(th, o, d, t)).reshape(-1)
        L = ((a[:, None] * (m @ ft)).reshape(len(o), K, C)).sum(1)
        op = (a * m.sum(1)).reshape(len(o), K).sum(1)
        return float((L * gL64).sum() + (op * gA64).sum())

    def central(which, base, idx):
        h = 1e-6 * max(1.0, abs(base[idx]))
        up, dn = base.copy(), base.copy()
        up[idx] += h
        dn[idx] -= h
        args = {"theta": (theta0, f0, q0), "f": (theta0, f0, q0), "q": (theta0, f0, q0)}[which]
        at = {"theta": 0, "f": 1, "q": 2}[which]
        hi, lo = list(args), list(args)
        hi[at], lo[at] = up, dn
        return (loss(*hi) - loss(*lo)) / (2 * h)

    fd = np.array([[central("theta", theta0, (g, k)) for k in range(10)] for g in range(len(theta0))])
    fdf = np.array([[central("f", f0, (g, k)) for k in range(C)] for g in range(len(theta0))])
    fdq = np.array([[central("q", q0, (i, k)) for k in range(K)] for i in range(len(o))])
    worst = 0.0
    for name, a, b in (("gaussians", G, fd), ("features", Gr, fdf), ("q", Gq, fdq)):
        scale = np.abs(a).max(0)
        assert np.all(scale > 0), name
        rel = float((np.abs(a - b) / scale).max())
        print(f"{name}: worst |model - central difference| / largest component of the column = {rel:.3e}")
        worst = max(worst, rel)
    assert worst <= 1e-5


def test_the_model_is_the_two_models_it_is_composed_from():
    """The emission part is FeatureModel.grads for w = a (x) gL, u = a gA; s is gL . F + gA mass of the same model; and the
    cases keep the radiance model's cap on zeroed samples."""
    sc = GR.oracle_scene(NAME)
    o, d, t, q, f, gL, gA = RG.case_inputs(NAME, N_RAYS, 17, 3)
    T = RR.transmittance_f32(sc, o, d, t)
    mdl = RG.RadianceGradModel(sc, o, d, t, q, f, T, gL, gA)
    assert RR.model(NAME, N_RAYS, 17, 3).zeroed <= RR.CAP
    x = RR.points_f32(o, GR.normalized_f32(d), t).reshape(-1, 3)
    fm = FR.FeatureModel(SR.Model(SR.records_of_oracle(sc.records()), x), f)
    a = q.astype(np.float64) * T
    (Gf, Sf), (Gr, Sr), _ = fm.grads((a[:, :, None] * gL.astype(np.float64)[:, None, :]).reshape(-1, 3), (a * gA[:, None]).reshape(-1))
    assert np.array_equal(Gf, mdl.Gf) and np.array_equal(Sr, mdl.Sr)
    s = (fm.F.reshape(257, 17, 3) * gL.astype(np.float64)[:, None, :]).sum(2) + fm.mass.reshape(257, 17) * gA[:, None]
    assert np.allclose(s, mdl.s64, rtol=1e-12, atol=1e-15 * np.abs(mdl.s_abs).max())
    assert np.all(np.abs(mdl.s64) <= mdl.s_abs * (1 + 1e-12)) and (mdl.s_abs > 0).sum() > 100
    assert np.array_equal(mdl.grad_tau, -a * mdl.s64) and np.array_equal(mdl.grad_q, T * mdl.s64)


def test_the_sparse_sums_are_the_dense_models_sums():
    """profile_sums with the oracle's chords is ProfileModel.grad; scales (float64 chords) gives the models' absolute sums."""
    import profile_reference as PR
    name, n, K_, C_, rows = "50_random", 1024, 33, 19, 96
    sc = GR.oracle_scene(name)
    o, d, t, q, f, gL, gA = RG.case_inputs(name, n, K_, C_, rows=rows)
    T = RR.transmittance_f32(sc, o, d, t)
    mdl = RG.RadianceGradModel(sc, o, d, t, q, f, T, gL, gA)
    for moving in (True, False):
        G, S = PR.ProfileModel(sc, o, d, t).grad(mdl.grad_tau, moving)
        G2, S2 = RG.profile_sums(sc, o, d, t, mdl.grad_tau, moving)
        assert np.allclose(G, G2, rtol=1e-12, atol=1e-12 * S.max()) and np.allclose(S, S2, rtol=1e-12, atol=0) and (S > 0).any()
    sm = RG.sparse_model(sc, o, d, t, q, f, T, gL, gA)
    for a, b in ((sm.Gf, mdl.Gf), (sm.Gr, mdl.Gr), (sm.s64, mdl.s64)):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max())
    for a, b in ((sm.Sf, mdl.Sf), (sm.Sr, mdl.Sr), (sm.s_abs, mdl.s_abs), (sm.s_slack, mdl.s_slack)):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert np.array_equal(sm.near, mdl.near) and np.array_equal(sm.grad_tau, -sm.q * sm.T * sm.s64)
    Sf, Sr, Sp, s_abs = RG.scales(sc, o, d, t, q, f, T, gL, gA, mdl.grad_tau)
    assert np.array_equal(Sf, sm.Sf) and np.array_equal(s_abs, sm.s_abs)
    S = mdl.profile(None, True)[1]
    print(f"float64 chords against the oracle's: max |Sp - Sp'| / max Sp = {(np.abs(Sp - S) / S.max(0)).max():.3e}")
    assert np.all(np.abs(Sp - S) <= 1e-3 * S.max(0))  # (a scale: the boundary terms feel the f32 rounding of the chord ends)
