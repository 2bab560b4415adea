"""CPU: parameter maps and Adam of the inverse loop (gmm.h:583-706, optimizer.h:13-55)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dg-vol-renderer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pytest  # noqa: E402
import sfd_replay as R  # noqa: E402
from vr_amd import inverse as inv  # noqa: E402


def test_pack_apply_round_trip_reproduces_covariance():
    rng = np.random.default_rng(0)
    rows = []
    for _ in range(16):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        d = rng.uniform(0.01, 0.2, 3) ** 2
        C = Q @ np.diag(d) @ Q.T
        rows.append([*rng.uniform(-1, 1, 3), C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2],
                     rng.uniform(0.2, 3), rng.uniform(0.1, 0.9)])
    g = np.array(rows, np.float32)
    p = inv.pack_parameters(g)
    assert p.shape == (16 * 11,)
    back = inv.apply_params(p, [], (0.5, 0.5, 0.5)).gaussians()[:, :11]
    np.testing.assert_allclose(back, g, rtol=2e-5, atol=2e-6)


def test_adam_first_steps_follow_the_reference_formula():
    a = inv.AdamOptimizer(2, lr=0.1)
    x = np.array([1.0, -2.0], np.float32)
    g = np.array([0.5, -4.0], np.float32)
    assert a.step(x, g)
    # t = 1: m = 0.1 g, v = 0.001 g^2, a = lr sqrt(1-0.999)/(1-0.9) -> step = lr * sign(g) (eps aside)
    np.testing.assert_allclose(x, [0.9, -1.9], rtol=1e-5)
    assert not a.step(np.zeros(3, np.float32), np.zeros(3, np.float32))


def test_default_eps_layout():
    e = inv.make_default_eps_for_params(np.zeros(22, np.float32))
    np.testing.assert_array_equal(e[:11], np.float32([0.02] * 3 + [0.1] * 3 + [0.05] * 3 + [0.25, 0.5]))
    np.testing.assert_array_equal(e[11:], e[:11])


def test_sigmoid_pair():
    y = np.float32([0.1, 0.5, 0.9])
    np.testing.assert_allclose(inv.sigmoidf_safe(inv.inv_sigmoidf(y)), y, rtol=1e-6)


def test_sign_vectors_are_balanced_and_keyed():
    a = inv.sign_vector(7, 0, 20000)
    b = inv.sign_vector(7, 1, 20000)
    assert set(np.unique(a)) == {-1.0, 1.0} and abs(a.mean()) < 0.03
    assert not np.array_equal(a, b) and np.array_equal(a, inv.sign_vector(7, 0, 20000))


def test_pack_matches_numpy_eigh_up_to_rotation_sign():
    """The native eigenbasis (Jacobi) gives the LAPACK eigenvalues; apply(pack) is the identity on
    covariances, so any sign choice of the eigenvectors is equivalent."""
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    d = np.array([0.01, 0.02, 0.05]) ** 2
    C = Q @ np.diag(d) @ Q.T
    g = np.array([[0, 0, 0, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2], 1.0, 0.5]], np.float32)
    p = inv.pack_parameters(g)
    np.testing.assert_allclose(np.exp(p[6:9]), np.sqrt(np.linalg.eigvalsh(C.astype(np.float32))), rtol=1e-4)


# ---- against the float64 models of tests/sfd_replay.py ------------------------------------------
def _native_adam(p, g, m, v, t, lr):
    import ctypes
    fp = ctypes.POINTER(ctypes.c_float)
    inv.check(inv.lib().vr_adam_step(p.ctypes.data_as(fp), g.ctypes.data_as(fp), m.ctypes.data_as(fp), v.ctypes.data_as(fp),
                                     p.size, int(t), float(lr), 0.9, 0.999, 1e-8))


def test_adam_seven_steps_follow_the_float64_model():
    """vr_adam_step, steps 1..7 on 1000 parameters: every step against adam64 on the step's own f32 inputs
    (parameters, gradient, carried moments), parameters within adam_margin, moments to their f32 roundings."""
    rng = np.random.default_rng(11)
    n, lr = 1000, 0.05
    p = rng.uniform(-3, 3, n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for t in range(1, 8):
        g = (10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if t == 1:
            g[:40] = 0.0  # zero gradient on zero moments: 0 / (0 + eps)
        if t == 4:
            g[20:80] = 0.0  # zero gradient on carried moments
        p0, m0, v0 = p.copy(), m.copy(), v.copy()
        _native_adam(p, g, m, v, t, lr)
        p64, m64, v64 = R.adam64(p0, g, m0, v0, t, lr)
        assert np.all(np.abs(p - p64) <= R.adam_margin(p0, p64)), t
        worst = max(worst, float(np.abs(p - p64).max()) / R.ulp32(np.abs(p0).max()))
        b1 = float(np.float32(0.9))
        assert np.all(np.abs(m - m64) <= 3 * 2.0 ** -24 * (np.abs(b1 * m0.astype(np.float64)) + np.abs((1 - b1) * g.astype(np.float64)))), t
        np.testing.assert_allclose(v, v64, rtol=4e-7, atol=0)
    print(f"vr_adam_step vs adam64 over 7 steps: max |dp| = {worst:.2f} ulp_f32(max |p|)")
    assert not np.array_equal(m, np.zeros(n)) and np.all(np.isfinite(p))


def _apply_rows():
    rng = np.random.default_rng(5)
    n = 2000
    p = np.zeros((n, 11), np.float64)
    p[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0, np.pi, n)
    angle[0:50] = 0.0
    angle[50:100] = 1e-6
    angle[100:150] = np.pi
    angle[150:250] = rng.uniform(np.pi, 7.0, 100)
    angle[250] = 7.0
    p[:, 3:6] = axis * angle[:, None]
    p[:, 6:9] = rng.uniform(np.log(0.005), np.log(0.5), (n, 3))
    p[0, 6:9] = np.log(0.005)
    p[1, 6:9] = np.log(0.5)
    p[2, 6:9] = np.log([0.005, 0.5, 0.005])
    p[:, 9] = rng.uniform(-3, 2, n)
    p[:, 10] = rng.uniform(-6, 6, n)
    p[0::7, 10] = 20.0
    p[1::7, 10] = -20.0
    return p.astype(np.float32)


def test_apply_parameters_follows_the_float64_model():
    """vr_gmm_apply_parameters on 2000 rows against apply64 (one-sided: no pack in the loop). Rotation angles 0,
    1e-6, pi and (pi, 7] are present, log scales span log 0.005 .. log 0.5, logits reach +-20."""
    p = _apply_rows()
    ang = np.linalg.norm(p[:, 3:6].astype(np.float64), axis=1)
    assert (ang == 0).any() and (np.abs(ang - 1e-6) < 1e-9).any() and (np.abs(ang - np.pi) < 1e-6).any() and (ang > 3.2).any()
    got = inv.apply_params(p.reshape(-1), [], (0.5, 0.5, 0.5)).gaussians()[:, :11]
    ref = R.apply64(p.reshape(-1))
    assert np.array_equal(got[:, 0:3], p[:, 0:3])
    lam = np.exp(2.0 * p[:, 6:9].astype(np.float64)).max(axis=1)
    cerr = np.abs(got[:, 3:9] - ref[:, 3:9]).max(axis=1) / lam
    derr = np.abs(got[:, 9] - ref[:, 9]) / ref[:, 9]
    aerr = np.abs(got[:, 10] - ref[:, 10])
    print(f"apply vs apply64: covariance {cerr.max():.2e} of the largest eigenvalue, density {derr.max():.2e} relative, "
          f"albedo {aerr.max():.2e}")
    assert cerr.max() <= 2e-6
    assert derr.max() <= 1e-6
    assert aerr.max() <= 1e-6


def _rot(angle, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * np.outer(a, a)


_Q0 = _rot(0.7, (0.3, -0.5, 0.8))
_ASC = np.array([0.02, 0.05, 0.11]) ** 2
# name -> (eigenbasis Q, eigenvalues d): covariance Q diag(d) Q^T
PACK_CASES = {
    "isotropic": (np.eye(3), np.array([0.07, 0.07, 0.07]) ** 2),
    "axis_aligned": (np.eye(3), _ASC),
    "two_equal_eigenvalues": (_Q0, np.array([0.03, 0.03, 0.12]) ** 2),
    "two_equal_largest": (_Q0, np.array([0.03, 0.12, 0.12]) ** 2),
    "pi_about_x": (np.diag([1.0, -1.0, -1.0]), _ASC),
    "pi_about_x_general": (_rot(np.pi, (1, 0, 0)) @ _Q0, _ASC),
    "pi_about_111": (_rot(np.pi, (1, 1, 1)), _ASC),
    "pi_about_111_general": (_rot(np.pi, (1, 1, 1)) @ _Q0, _ASC),
    "pi_minus_1e-4": (_rot(np.pi - 1e-4, (0.2, 0.9, -0.4)), _ASC),
    "cyclic_permutation": (np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), _ASC),
    "ratio_1e6": (_Q0, 0.04 * np.array([1e-6, 1e-3, 1.0])),
}
# the covariance is diagonal with ascending entries: the eigenbasis is the identity, the rotation zero
PACK_DIAGONAL = ("isotropic", "axis_aligned", "pi_about_x")


@pytest.mark.parametrize("name", list(PACK_CASES))
def test_pack_parameters_named_covariances(name):
    """vr_gmm_pack_parameters on a named covariance, then apply64 (the float64 model, not the native apply:
    an error shared by the two native maps cannot cancel): the covariance comes back to 1e-6 of its largest
    entry. A diagonal covariance whose entries ascend packs as rotation 0; in another order (the cyclic
    permutation) it packs as the axis permutation that sorts the eigenvalues, as the reference's ascending
    eigen-solver does."""
    Q, d = PACK_CASES[name]
    C = Q @ np.diag(d) @ Q.T
    g = np.array([[0.1, -0.2, 0.3, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2], 0.7, 0.4]], np.float32)
    p = inv.pack_parameters(g)
    assert np.all(np.isfinite(p))
    if name in PACK_DIAGONAL:
        assert np.array_equal(p[3:6], np.zeros(3, np.float32))
    if name == "cyclic_permutation":
        assert abs(float(np.linalg.norm(p[3:6].astype(np.float64))) - 2 * np.pi / 3) < 1e-6
    back = R.apply64(p)[0]
    err = np.abs(back[3:9] - g[0, 3:9].astype(np.float64)).max() / np.abs(g[0, 3:9]).max()
    print(f"{name}: rotation {p[3:6]}, pack -> apply64 covariance error {err:.2e} of the largest entry")
    assert err <= 1e-6
    assert np.array_equal(p[0:3], g[0, 0:3])
    np.testing.assert_allclose(np.exp(2.0 * p[6:9].astype(np.float64)), np.sort(np.linalg.eigvalsh(R.cov3(g[0, 3:9]))),
                               rtol=1e-5 if name != "ratio_1e6" else 1e-3)


def test_pack_parameters_clamps_density_and_albedo():
    g = np.array([[0, 0, 0, 0.01, 0, 0, 0.01, 0, 0.01, 0.0, 0.0],
                  [0, 0, 0, 0.01, 0, 0, 0.01, 0, 0.01, 2.0, 1.0]], np.float32)
    p = inv.pack_parameters(g).reshape(2, 11)
    lo, hi = np.float32(1e-7), np.float32(1) - np.float32(1e-7)
    logit = lambda y: np.log(float(np.float32(y / (np.float32(1) - y))))  # noqa: E731
    np.testing.assert_allclose(p[0, 9], np.log(float(np.float32(1e-12))), rtol=1e-6)
    np.testing.assert_allclose(p[1, 9], np.log(2.0), rtol=1e-6)
    np.testing.assert_allclose(p[0, 10], logit(lo), rtol=1e-6)
    np.testing.assert_allclose(p[1, 10], logit(hi), rtol=1e-6)
    assert p[0, 10] < -16.0 and p[1, 10] > 15.9


@pytest.mark.parametrize("seed", [0, 7, 2 ** 63])
def test_sign_vectors_equal_the_integer_restatement(seed):
    for k in (0, 1, 5):
        assert np.array_equal(inv.sign_vector(seed, k, 5000), R.sign_vector_py(seed, k, 5000)), (seed, k)


def test_union_sum_equals_a_literal_set_union():
    """The helper against inverse_integrator.h:166-179 as written: per Gaussian the set of pixels of either
    recording, then the sum of loss_plus - loss_base over that set."""
    rng = np.random.default_rng(9)
    n, npix = 70, 200
    words = (n + 31) // 32
    b0 = (rng.integers(0, 2 ** 32, (words, npix), dtype=np.uint64) & rng.integers(0, 2 ** 32, (words, npix), dtype=np.uint64)
          ).astype(np.uint32)
    b1 = (rng.integers(0, 2 ** 32, (words, npix), dtype=np.uint64) & rng.integers(0, 2 ** 32, (words, npix), dtype=np.uint64)
          ).astype(np.uint32)
    b0[:, 50:60] = 0
    lb, lp = rng.random(npix).astype(np.float32), rng.random(npix).astype(np.float32)
    pixels = [set() for _ in range(n)]
    for bits in (b0, b1):
        for p in range(npix):
            for g in range(n):
                if (int(bits[g // 32, p]) >> (g % 32)) & 1:
                    pixels[g].add(p)
    ref = np.array([sum(float(lp[p]) - float(lb[p]) for p in sorted(s)) for s in pixels])
    got = R.union_sum(b0, b1, lb, lp, n)
    assert got.shape == (n,)
    np.testing.assert_allclose(got, ref, rtol=0, atol=npix * 2.0 ** -52)
    ints = R.union_sum(b0, b1, np.zeros(npix, np.float32), np.arange(1, npix + 1, dtype=np.float32), n)
    assert np.array_equal(ints, np.array([sum(p + 1 for p in s) for s in pixels], np.float64))
