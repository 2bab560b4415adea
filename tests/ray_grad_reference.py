"""Reference model of the ray gradient of the optical depth (Device.query_transmittance_ray_grad,
vr_query_transmittance_ray_grad): the formulas of include/vr_hip.h in float64 numpy / scipy. Computed once per case,
shared, never modified.

For a scene: hit flags and the f32 t_enter / t_exit come from the oracle's probe (grad_reference.probe), the records
from the oracle scene; everything after that is float64. `ray_contributions` is also the model the CPU test checks
against central differences of its own closed-form tau, there with float64 records and bounds.

Row layout (7 per ray, the vr_ray_grad row without its tau): d/d origin[3], d/d tmax, d/d direction[3].
"""
import numpy as np

from grad_reference import normalized_f32, oracle_scene, probe, quadratic, sym  # noqa: F401 (re-exported to the tests)

E45 = np.exp(-4.5)
BOUND = 2.0 ** -21  # |row_dev - G64| <= BOUND * S per component (the only f32 step is the final rounding, 2^-24 S; 8x for erf / exp)


def ray_contributions(mean, M, norm, rho, o, d, a, b, use, move_in, move_out, clipped):
    """((n, N, 7), (n, N)) float64: d tau_i / d (o[3], tmax, d[3]) of ray i through Gaussian g, d's three components
    taken as free, and the Gaussian's closed-form optical depth. mean (N, 3), M (N, 3, 3), norm, rho (N,); o, d (n, 3);
    a, b (n, N) the clip bounds; use: the hit contributes (b > a); move_in / move_out: the bound lies on the ellipsoid
    and moves with the ray; clipped: the upper bound is tmax itself."""
    from scipy.special import erf
    A, B, C, p, _ = quadratic(mean, M, o, d)
    dd = np.broadcast_to(d[:, None, :], p.shape)
    Mv = lambda x: np.einsum("gij,rgj->rgi", M, x)  # noqa: E731
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
        s = rho * norm * k
        go = -s[..., None] * Mv(c * J0[..., None] + dd * J1[..., None])
        gd = -s[..., None] * Mv(m[..., None] * c * J0[..., None] + (c + m[..., None] * dd) * J1[..., None] + dd * J2[..., None])
        for t, sg, mv in ((b, 1.0, move_out), (a, -1.0, move_in)):
            w = np.where(mv, sg * rho * norm * E45 / (2.0 * A * t + B), 0.0)
            Mx = Mv(p + t[..., None] * dd)
            go = go - 2.0 * w[..., None] * Mx
            gd = gd - 2.0 * (w * t)[..., None] * Mx
        gt = np.where(clipped, s * eb, 0.0)
        tau = s * J0
    out = np.concatenate([go, gt[..., None], gd], -1)
    return np.where(use[..., None], out, 0.0), np.where(use, tau, 0.0)


def row_form(c, d, vlen):
    """Per-Gaussian contributions c (n, N, 7) in the row's own form: for unit == 0 (vlen (n,), the length of the stored
    direction) the direction part becomes (g_d - d (d.g_d)) / |v|; vlen None (unit != 0): as it stands."""
    if vlen is None:
        return c
    gd = c[..., 4:7]
    dd = d[:, None, :]
    proj = (gd - dd * np.sum(dd * gd, -1, keepdims=True)) / vlen[:, None, None]
    return np.concatenate([c[..., 0:4], proj], -1)


class RayModel:
    """The float64 model of one scene along one batch of rays, for either flag. `d_raw` (n, 3) f32 is what the Ray
    constructor normalises: with unit=False the device gets d_raw itself, with unit=True normalized_f32(d_raw); the
    direction walked is the same. Invalid rays and rays with tmax <= 0 / NaN have zero rows here (`valid`, `walked`
    tell them apart: the device gives NaN for the first kind)."""

    def __init__(self, sc, o, d_raw, tmax, unit, probed=None):
        n = len(o)
        o, d_raw = np.asarray(o, np.float32), np.asarray(d_raw, np.float32)
        self.tmax = np.broadcast_to(np.asarray(tmax, np.float32), (n,)).copy()
        hit, te, tx = probed if probed is not None else probe(sc, o, d_raw)
        rec = sc.records().astype(np.float64)
        self.N = rec.shape[0]
        mean, rho, norm, M = rec[:, :3], rec[:, 3], rec[:, 10], sym(rec[:, 4:10])
        with np.errstate(all="ignore"):
            s32 = d_raw[:, 0] * d_raw[:, 0] + (d_raw[:, 1] * d_raw[:, 1] + d_raw[:, 2] * d_raw[:, 2])  # the loader's f32 sum
            dn = normalized_f32(d_raw)
            self.valid = np.isfinite(o).all(1) & np.isfinite(s32) & (s32 > 0) & np.isfinite(dn).all(1)
            self.walked = self.valid & (self.tmax > 0)
            a = np.maximum(np.float32(0), te)           # f32, as the device clips
            b = np.minimum(self.tmax[:, None], tx)
            use = hit & (b > a) & self.walked[:, None]
            clipped = use & (tx > self.tmax[:, None])
        ok = self.walked[:, None]
        o64 = np.where(ok, o, 0.0).astype(np.float64)
        d64 = np.where(ok, dn, np.float32([1, 0, 0])).astype(np.float64)
        a64, b64 = np.where(use, a, 0.0).astype(np.float64), np.where(use, b, 1.0).astype(np.float64)
        vlen = None if unit else np.where(self.walked, np.sqrt(np.where(self.walked, s32, 1).astype(np.float64)), 1.0)
        args = (mean, M, norm, rho, o64, d64, a64, b64, use)
        self.use, self.clipped, self.moved_out, self.moved_in = use, clipped, use & (tx <= self.tmax[:, None]), use & (te > 0)
        none = np.zeros_like(use)
        frozen, tau = ray_contributions(*args, none, none, clipped)
        moving, _ = ray_contributions(*args, self.moved_in, self.moved_out, clipped)
        self.tau = tau.sum(1)
        self._rows = {}
        for key, c in ((False, frozen), (True, moving)):
            c = row_form(c, d64, vlen)
            self._rows[key] = (c.sum(1), np.abs(c).sum(1))
            for x in self._rows[key]:
                x.setflags(write=False)
        self.tau.setflags(write=False)

    def rows(self, moving=True):
        """(G64, S), each (n, 7): the row of each ray and the sum over Gaussians of its absolute contributions."""
        return self._rows[bool(moving)]


def judge(label, dev, G64, S, bound=BOUND):
    """Prints the measured maximum, then asserts |dev - G64| <= bound * S per component and exact zeros where S = 0."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == G64.shape, (dev.shape, G64.shape)
    err = np.abs(dev - G64)
    with np.errstate(all="ignore"):
        rel = np.where(S > 0, err / S, 0.0)
    nz = int(np.count_nonzero(dev[S == 0]))
    print(f"{label}: max |row_dev - G64| / S = {rel.max():.3e} (bound {bound:.3e}), max |G64| = {np.abs(G64).max():.3e}, "
          f"rays with hits {int((S[:, :3].sum(1) > 0).sum())} of {len(S)}, non-zeros where S = 0: {nz}")
    assert np.all(np.isfinite(dev))
    assert nz == 0
    assert np.all(err <= bound * S), (float(rel.max()), np.argwhere(err > bound * S)[:5].tolist())
    return float(rel.max())


def pack_rows(d_origin, d_direction, d_tmax):
    """The method's three gradient outputs as (n, 7) rows in the model's layout."""
    return np.concatenate([np.asarray(d_origin), np.asarray(d_tmax)[:, None], np.asarray(d_direction)], 1)
