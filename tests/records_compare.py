"""Record-level comparison of RayMarchingGaussians: a pixel's scattering steps as `vr_debug_pixel_records`
(device) and `orc_debug_pixel_records` (oracle) return them, row against row.

A row is (k, pos xyz, T sigma_s, Li + Le rgb, active-list length, then every secondary ray's Tr: lights first,
then the environment samples in sample order). The pixel bar of test_gpu_parity.py (L-inf < 1e-4) sees a ray's
error only through two sums (a record's rays, a pixel's records); compare_rows holds every ray to that bar.

Shared by tests/test_gpu_records.py (device against oracle), tests/test_records_reference.py (the checker
against mutated oracle rows, no GPU) and tools/pixel_records_cmp.py.
"""
from collections import namedtuple

import numpy as np

import pyoracle as O
from helpers import CAM_POS, FOV, main_view_dir, scene_path

TR_TOL = 1e-4      # per ray: the project's parity bar (test_gpu_parity.TOL)
TS_RTOL = 1e-5     # T sigma_s, relative
S_RTOL = 1e-5      # Li + Le recomputed from the row's own Tr, relative to its all-Tr-one value
TS_TINY = 1e-30    # a step on one side only is a sigma_s > 0 decision on an underflowing density below this
TINY_SHARE = 0.01  # ... and at most this share of a pixel's rows
SPREAD = (0.05, 0.95)
MIN_SPREAD_SHARE = 0.25
BUDGET = 1.2e-6    # test_secondary_cut_off_stays_within_its_pixel_budget's figure
FAIR_E_REF = 0.5e-4  # a ray whose oracle Tr is this close to the float64 model's is a fair one (compare_rows' tr_f64)
STEP = 0.01
ENV = (0.53, 0.81, 0.92)

K4PI = float(np.float32(4.0 * np.pi))
INV4PI = float(np.float32(1.0 / (4.0 * np.pi)))

# kind: step_only_dev, step_only_orc, tiny_steps, width, position, active, ts, tr, s_self, s_oracle, budget
Finding = namedtuple("Finding", "kind k ray dev orc")


class Report:
    def __init__(self):
        self.findings = []
        self.rows = 0
        self.rays = 0
        self.max_dtr = 0.0
        self.max_rel_dts = 0.0
        self.spread_rays = 0  # compared rays whose oracle Tr lies in SPREAD
        self.tr_min = 1.0
        self.budget = 0.0
        self.one_sided = 0  # steps on one side only that pass as underflow decisions
        # with a float64 ray model (compare_rows' tr_f64): fair rays, and the two rules' largest figures
        self.fair_rays = 0
        self.max_fair = 0.0    # |Tr_dev - Tr_oracle| over the fair rays
        self.max_other = 0.0   # |Tr_dev - Tr_f64| - e_ref over the other rays
        self.max_e_ref = 0.0   # the oracle's own distance from float64

    def kinds(self):
        return {f.kind for f in self.findings}

    def named(self, kind, k=None, ray=None):
        return [f for f in self.findings if f.kind == kind and (k is None or f.k == k) and (ray is None or f.ray == ray)]

    def merge(self, other):
        self.findings += other.findings
        self.rows += other.rows
        self.rays += other.rays
        self.max_dtr = max(self.max_dtr, other.max_dtr)
        self.max_rel_dts = max(self.max_rel_dts, other.max_rel_dts)
        self.spread_rays += other.spread_rays
        self.tr_min = min(self.tr_min, other.tr_min)
        self.budget = max(self.budget, other.budget)
        self.one_sided += other.one_sided
        self.fair_rays += other.fair_rays
        self.max_fair = max(self.max_fair, other.max_fair)
        self.max_other = max(self.max_other, other.max_other)
        self.max_e_ref = max(self.max_e_ref, other.max_e_ref)
        return self

    @property
    def fair_share(self):
        return self.fair_rays / self.rays if self.rays else 0.0

    @property
    def spread_share(self):
        return self.spread_rays / self.rays if self.rays else 0.0

    def summary(self):
        return (f"{self.rows} rows, {self.rays} rays, max |dTr| {self.max_dtr:.3e}, max rel dTs {self.max_rel_dts:.3e}, "
                f"{self.one_sided} one-sided steps, oracle Tr min {self.tr_min:.3f}, {100 * self.spread_share:.0f} % of rays with Tr in "
                f"[{SPREAD[0]}, {SPREAD[1]}]")

    def describe(self, limit=12):
        out = [f"{len(self.findings)} findings"]
        for f in self.findings[:limit]:
            out.append(f"  {f.kind}: step {f.k} ray {f.ray}: device {f.dev!r} oracle {f.orc!r}")
        return "\n".join(out)


def ray_weights(pos, light_pos, light_int, env, n_env):
    """(lights + n_env, 3) float64: what a ray with Tr = 1 adds to the row's Li + Le. Lights: I / d^2 with d the
    f32 distance from the row's position (the reference squares the rounded norm); environment: 4 pi env / n_env."""
    lp = np.asarray(light_pos, np.float32).reshape(-1, 3)
    li = np.asarray(light_int, np.float64).reshape(-1, 3)
    d = lp - np.asarray(pos, np.float32)
    dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32))
    d2 = (dist * dist).astype(np.float64)
    w_env = np.tile(K4PI * np.asarray(env, np.float64) / max(n_env, 1), (n_env, 1))
    return np.concatenate([li / d2[:, None], w_env]) if len(lp) else w_env


def compare_rows(dev, orc, light_pos, light_int, env, budget=False, tr_f64=None):
    """Device rows against oracle rows of one pixel, matched by step index. Returns a Report whose findings name
    every row, column and ray over its bar. budget=True is the t_eps > 0 form: rows up to the device's last
    step, every ray's |dTr| weighted into the pixel budget instead of held to TR_TOL.

    tr_f64 ({step: float64 Tr of the row's rays}, ray_model_f64) is for scenes on which the oracle's own f32 Tr is far
    from float64 (elongated Gaussians): with e_ref = |Tr_oracle - Tr_f64|, a fair ray (e_ref <= FAIR_E_REF) is held to
    |Tr_dev - Tr_oracle| <= TR_TOL as ever, any other ray to |Tr_dev - Tr_f64| <= e_ref + TR_TOL (the device is never
    further from the truth than the reference, plus the bar; finding kind "tr_f64"). Li + Le against the oracle's
    then gets what the two rules leave a ray: TR_TOL, plus 2 e_ref where the ray is not fair."""
    dev = np.asarray(dev, np.float32)
    orc = np.asarray(orc, np.float32)
    rep = Report()
    nl = len(np.asarray(light_pos).reshape(-1, 3))
    if dev.ndim != 2 or orc.ndim != 2 or dev.shape[1] != orc.shape[1] or dev.shape[1] < 9 + nl:
        rep.findings.append(Finding("width", None, None, dev.shape, orc.shape))
        return rep
    n_env = dev.shape[1] - 9 - nl
    kd = {int(r[0]): r for r in dev}
    ko = {int(r[0]): r for r in orc}
    if len(kd) != len(dev) or len(ko) != len(orc):
        rep.findings.append(Finding("step_only_dev" if len(kd) != len(dev) else "step_only_orc", None, None,
                                    "repeated step index", None))
    if budget and kd:
        last = max(kd)
        ko = {k: r for k, r in ko.items() if k <= last}
    tiny = 0
    for k in sorted(set(kd) ^ set(ko)):
        row, kind = (kd[k], "step_only_dev") if k in kd else (ko[k], "step_only_orc")
        if abs(float(row[4])) < TS_TINY:
            tiny += 1
        else:
            rep.findings.append(Finding(kind, k, None, float(row[4]) if k in kd else None, float(row[4]) if k in ko else None))
    rep.one_sided = tiny
    if tiny > TINY_SHARE * max(len(kd), len(ko)):
        rep.findings.append(Finding("tiny_steps", None, None, tiny, max(len(kd), len(ko))))
    for k in sorted(set(kd) & set(ko)):
        a, b = kd[k], ko[k]
        rep.rows += 1
        if not np.array_equal(a[1:4].view(np.uint32), b[1:4].view(np.uint32)):
            rep.findings.append(Finding("position", k, None, a[1:4].tolist(), b[1:4].tolist()))
        if a[8] != b[8]:
            rep.findings.append(Finding("active", k, None, int(a[8]), int(b[8])))
        ts_d, ts_o = float(a[4]), float(b[4])
        rel = abs(ts_d - ts_o) / max(abs(ts_o), TS_TINY)
        rep.max_rel_dts = max(rep.max_rel_dts, rel)
        if not rel <= TS_RTOL:
            rep.findings.append(Finding("ts", k, None, ts_d, ts_o))
        tr_d, tr_o = a[9:].astype(np.float64), b[9:].astype(np.float64)
        dtr = np.abs(tr_d - tr_o)
        rep.rays += len(dtr)
        rep.spread_rays += int(np.sum((tr_o >= SPREAD[0]) & (tr_o <= SPREAD[1])))
        if len(dtr):
            rep.tr_min = min(rep.tr_min, float(tr_o.min()))
        # Li + Le from the device's own Tr row, in float64 (the shading kernel, independently of the oracle)
        w = ray_weights(a[1:4], light_pos, light_int, env, n_env)
        s_one = w.sum(axis=0)
        s_own = (tr_d[:, None] * w).sum(axis=0)
        for c in range(3):
            if not abs(float(a[5 + c]) - s_own[c]) <= S_RTOL * s_one[c]:
                rep.findings.append(Finding("s_self", k, c, float(a[5 + c]), float(s_own[c])))
        if budget:
            rep.budget += ts_o * STEP * INV4PI * float((w.max(axis=1) * np.nan_to_num(dtr, nan=np.inf)).sum())
            continue
        rep.max_dtr = max(rep.max_dtr, float(np.nanmax(dtr)) if len(dtr) else 0.0)
        slack = np.zeros(3)
        if tr_f64 is None:
            for s in np.nonzero(~(dtr < TR_TOL))[0]:
                rep.findings.append(Finding("tr", k, int(s), float(tr_d[s]), float(tr_o[s])))
        else:
            t64 = np.asarray(tr_f64[k], np.float64)
            e_ref = np.abs(tr_o - t64)
            fair = e_ref <= FAIR_E_REF
            over = np.abs(tr_d - t64) - e_ref
            rep.fair_rays += int(fair.sum())
            rep.max_e_ref = max(rep.max_e_ref, float(e_ref.max()) if len(e_ref) else 0.0)
            rep.max_fair = max(rep.max_fair, float(np.nanmax(dtr[fair])) if fair.any() else 0.0)
            rep.max_other = max(rep.max_other, float(np.nanmax(over[~fair])) if (~fair).any() else 0.0)
            for s in np.nonzero(fair & ~(dtr < TR_TOL))[0]:
                rep.findings.append(Finding("tr", k, int(s), float(tr_d[s]), float(tr_o[s])))
            for s in np.nonzero(~fair & ~(over <= TR_TOL))[0]:
                rep.findings.append(Finding("tr_f64", k, int(s), float(tr_d[s]), (float(tr_o[s]), float(t64[s]))))
            slack = (np.where(fair, 0.0, 2.0 * e_ref)[:, None] * w).sum(axis=0)
        for c in range(3):
            if not abs(float(a[5 + c]) - float(b[5 + c])) <= TR_TOL * s_one[c] + slack[c]:
                rep.findings.append(Finding("s_oracle", k, c, float(a[5 + c]), float(b[5 + c])))
    if budget and not rep.budget <= BUDGET:
        rep.findings.append(Finding("budget", None, None, rep.budget, BUDGET))
    return rep


def pixel_from_rows(rows, step=STEP):
    """(float64 rgb sum of the rows' Ts S step / 4 pi, its f32 accumulation bound n_rows 2^-23 sum |terms|)."""
    rows = np.asarray(rows, np.float64)
    terms = rows[:, 4:5] * rows[:, 5:8] * float(np.float32(step)) * INV4PI
    return terms.sum(axis=0), len(rows) * 2.0 ** -23 * np.abs(terms).sum(axis=0)


def oracle_rows(osc, x, y, W, H, env_samples, step=STEP, cam=None):
    """The oracle's rows of pixel (x, y) under the device's tie rule (stable event order). cam: (position, view
    direction) of the pinhole camera, the main view's by default."""
    pos, view = cam if cam is not None else (CAM_POS, main_view_dir())
    with O.stable_ties():
        return O.debug_pixel_records(osc, pos, view, FOV, x, y, W, H, step, env_samples)


def oracle_rows_many(osc, pixels, W, H, env_samples, step=STEP, cam=None):
    """oracle_rows of several pixels, one thread each (the trace buffer is per thread; a pixel of the 200-deep
    nested scene costs seconds)."""
    from concurrent.futures import ThreadPoolExecutor
    O.lib()
    pos, view = cam if cam is not None else (CAM_POS, main_view_dir())
    pixels = [(int(x), int(y)) for x, y in pixels]
    with O.stable_ties(), ThreadPoolExecutor(max_workers=max(1, min(8, len(pixels)))) as pool:
        rows = list(pool.map(lambda p: O.debug_pixel_records(osc, pos, view, FOV, p[0], p[1], W, H, step,
                                                             env_samples), pixels))
    return dict(zip(pixels, rows))


def record_active(osc, x, y, W, H, env_samples, k, step=STEP, cam=None):
    """orc_debug_record_active: the scene indices active at scattering step k of pixel (x, y) (None: no such
    step), for a failure message and for ray_model_f64."""
    pos, view = cam if cam is not None else (CAM_POS, main_view_dir())
    with O.stable_ties():
        return O.debug_record_active(osc, pos, view, FOV, x, y, W, H, k, step, env_samples)


# ---- the cases of test_gpu_records.py; test_records_reference.py evaluates their oracle side without a GPU ----
def six_pixels(W):
    return [(W // 2, W // 2), (W // 3, W // 2), (W // 2, W // 3), (2 * W // 3, 2 * W // 3), (W // 4, 3 * W // 4),
            (W // 2 + 1, W // 2 - 3)]


# name: (scene file, W, env_samples, pixels). The dense 250_random and 1000_random are opaque at six_pixels
# (15 % and 6 % of those rays have Tr in SPREAD: the rest is 0 or 1), so they keep the centre (250_random also
# (W/4, 3W/4)) and take pixels at the cloud's rim, found by scanning the frame with the oracle (shares in DESIGN.md
# section 5); the two fallback pixels the GPU test adds at 1000_random are opaque ones again.
FIXTURE_CASES = {
    "50_random": ("50_random.txt", 32, 5, six_pixels(32)),
    "many_gaussians": ("many_gaussians.txt", 32, 5, six_pixels(32)),
    "2_gaussian": ("2_gaussian.txt", 32, 5, six_pixels(32)),
    "250_random": ("250_random.txt", 48, 3, [(24, 24), (12, 36), (4, 2), (31, 1), (17, 0), (5, 4)]),
    "1000_random": ("1000_random.txt", 64, 3, [(32, 32), (54, 4), (60, 4), (52, 2), (6, 0), (62, 8)]),
}
NESTED_PIXELS = [(8, 8), (7, 9), (5, 8), (8, 4), (10, 10), (3, 3)]
NESTED_CASES = [(60, 1e-2), (80, 1e-2), (200, 3e-3), (60, 3e-2)]  # 16 x 16, env_samples 3
NESTED_LIGHT = ([0.0, 5.0, 0.0], [1.0, 1.0, 1.0])
# 48 x 48, env_samples 8: every first-light ray of these pixels is one of the slow ones
LIGHT_INSIDE_PIXELS = [(24, 3), (27, 3), (21, 6), (21, 15)]
# 32 x 32, env_samples 8: each has three environment rays with a chord in the f32 error band (band_chords)
BAND_PIXELS = [(15, 17), (14, 16), (16, 18), (14, 13), (14, 12), (17, 9)]
CHORD_BAND = 8.0 * 2.0 ** -23  # vr_gauss_common.h kChordBand
# (scene file, W, env_samples, pixels) at t_eps = 1e-6
CUTOFF_CASES = {
    "many_gaussians": ("many_gaussians.txt", 96, 5, six_pixels(96)),
    "1000_random": ("1000_random.txt", 64, 3, FIXTURE_CASES["1000_random"][3]),
}


def nested_gaussians(n, density):
    """test_gpu_parity._nested_scene's construction: n concentric Gaussians (sigma 0.3 .. 0.4) around (0, 1, 0),
    all n active at once on the central rays. Arrays (mean, cov6, density, albedo, light positions, intensities)."""
    mean = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (n, 1))
    sig = np.linspace(0.3, 0.4, n)
    cov = np.stack([sig ** 2, 0 * sig, 0 * sig, sig ** 2, 0 * sig, sig ** 2], 1).astype(np.float32)
    dens = np.full(n, density, np.float32)
    alb = np.full(n, 0.5, np.float32)
    return mean, cov, dens, alb, np.float32([NESTED_LIGHT[0]]), np.float32([NESTED_LIGHT[1]])


def light_inside_gaussians(big_density=(1.0, 0.2)):
    """test_gpu_parity._light_inside_scene: the first light lies inside a Gaussian's 3-sigma ellipsoid, so every ray
    towards it takes the exact slow path. Its two large Gaussians (the one around the light, the one around the
    camera) have densities 0.05 and 0.02 there, which leaves 10 % of the rays with Tr in SPREAD (19 % at the best
    pixel); with `big_density` the rays towards the light cross a medium that matters (Tr 0.05 .. 0.95 on all of
    them at LIGHT_INSIDE_PIXELS). big_density=(0.05, 0.02) is the parity test's scene."""
    rng = np.random.default_rng(3)
    n, spread = 12, 1.0
    mean = np.stack([rng.uniform(-spread, spread, n), rng.uniform(1 - spread, 1 + spread, n),
                     rng.uniform(-spread, spread, n)], 1).astype(np.float32)
    s = rng.uniform(0.05, 0.175, size=(n, 3))
    cov = []
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        c = q @ np.diag(s[i] ** 2) @ q.T
        cov.append([c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]])
    cov = np.asarray(cov, np.float32)
    dens = rng.uniform(0.2, 2.5, n).astype(np.float32)
    alb = rng.uniform(0.0, 1.0, n).astype(np.float32)
    mean = np.vstack([mean, [[0.0, 3.0, 0.0], [0.0, 1.0, 5.0]]]).astype(np.float32)
    cov = np.vstack([cov, [[0.5, 0, 0, 0.5, 0, 0.5], [0.3, 0.0, 0.0, 0.3, 0.0, 0.6]]]).astype(np.float32)
    dens = np.append(dens, big_density).astype(np.float32)
    alb = np.append(alb, [0.7, 0.9]).astype(np.float32)
    lpos = np.array([[0.0, 3.1, 0.1], [2.0, 2.0, 2.0]], np.float32)
    lint = np.array([[40, 40, 40], [10, 20, 30]], np.float32)
    return mean, cov, dens, alb, lpos, lint


def band_shell_gaussians(n_shell=1500, sigma=0.02, radius=2.5):
    """A scattering Gaussian (sigma 0.3) at (0, 1, 0) inside a shell of small dense ones at `radius`: seen from a
    record at whitened distance sqrt(c) ~ radius / sigma = 125, a grazing chord's 9 - e2 lies within the
    reference's f32 error band (|9 - e2| < kChordBand c = 0.015, the grazing-chord construction of
    test_oracle_golden.test_reference_f32_quadratic_collapses_a_grazing_chord_seen_from_far) for about one
    environment ray in 800: the device leaves that chord to its band fix-up queue (band_rays)."""
    rng = np.random.default_rng(11)
    v = rng.normal(size=(n_shell, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    mean = np.vstack([[[0.0, 1.0, 0.0]], np.array([0.0, 1.0, 0.0]) + radius * v]).astype(np.float32)
    sig = np.concatenate([[0.3], np.full(n_shell, sigma)])
    cov = np.stack([sig ** 2, 0 * sig, 0 * sig, sig ** 2, 0 * sig, sig ** 2], 1).astype(np.float32)
    dens = np.concatenate([[1.0], np.full(n_shell, 30.0)]).astype(np.float32)
    alb = np.full(n_shell + 1, 0.6, np.float32)
    return mean, cov, dens, alb, np.float32([[0.0, 5.0, 0.5]]), np.float32([[20, 20, 20]])


def _pcg32_textbook(seed, seq, n):
    """n outputs of PCG32(seed, seq) with the textbook output function (a rotation by the top five state bits): the
    oracle's uniform_env. O.pcg32 returns next_u32's outputs, whose rotation differs (the path sampler's)."""
    m64 = (1 << 64) - 1
    inc = ((seq << 1) | 1) & m64
    state = inc  # the constructor: one step from state 0, add the seed, one more step
    state = ((state + seed) * 6364136223846793005 + inc) & m64
    out = np.zeros(n, np.uint32)
    for i in range(n):
        old = state
        state = (old * 6364136223846793005 + inc) & m64
        shifted = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        out[i] = ((shifted >> rot) | (shifted << ((-rot) & 31))) & 0xFFFFFFFF
    return out


def env_directions(x, y, k, env_samples):
    """The environment directions of step k of pixel (x, y), as the oracle draws them (PCG32 keyed by pixel and
    step, its textbook output, 24-bit uniforms): secondary_rays' float64 model reproduces the oracle's own Tr along
    them to 5e-5 at kappa 9 (test_aniso_reference.py), which pins them."""
    xi = (_pcg32_textbook(O.derive_path_seed(x, y, k), 1, 2 * env_samples) >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.array([O.env_dir(xi[2 * i], xi[2 * i + 1]) for i in range(env_samples)], np.float64)


def secondary_rays(row, x, y, light_pos, env_samples):
    """(origins, unit directions (m, 3) f32, ends (m,) f32) of the secondary rays of one oracle row of pixel (x, y), in
    the row's order, as the reference forms them in f32: towards light l, Ray(pos, normalized(l - pos)) up to
    norm(l - pos) (the Ray constructor normalises once more); then Ray(pos, env_dir(xi1, xi2)) without end."""
    f = np.float32
    pos = np.asarray(row[1:4], f)
    lp = np.asarray(light_pos, f).reshape(-1, 3)

    def unit(v):
        s = v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return (v / np.sqrt(s)[:, None]).astype(f), np.sqrt(s)

    v = (lp - pos[None]).astype(f)
    wi, dist = unit(v) if len(lp) else (v, np.zeros(0, f))
    env = np.asarray(env_directions(x, y, int(row[0]), env_samples), f).reshape(-1, 3)
    d = unit(np.concatenate([wi, env]).astype(f))[0]
    end = np.concatenate([dist.astype(f), np.full(len(env), np.inf, f)])
    return np.tile(pos, (len(d), 1)), d, end


def ray_model_f64(rec, rows, x, y, light_pos, env_samples, active=None):
    """{step: float64 Tr of the row's rays}: aniso_cases.Pairs64 (float64 decisions, bounds and closed-form optical depth
    on the f32 records `rec`) along secondary_rays of every oracle row of pixel (x, y), each ray cut at its end.
    active ({step: scene indices}, record_active) is the row's active list, a decision the primary march took in f32
    from the camera's distance: the reference pre-activates those Gaussians at t = 0 whatever p.M.p says at the row's
    position (test_integrators.h:209-211), so a member the ray crosses counts over [0, t_exit] and a member it misses
    stays active to the ray's end, the light's distance or an environment ray's last event (:220-235, :258-271).
    Without it the float64 p.M.p <= 9 at the origin decides, which is the same set but for members within the
    march's f32 error of their 3-sigma surface."""
    import aniso_cases as A
    out = {}
    for row in rows:
        o, d, end = secondary_rays(row, x, y, light_pos, env_samples)
        pairs = A.Pairs64(rec, o, d, unit=True)
        end = end.astype(np.float64)[:, None]
        a, b = np.maximum(pairs.t0, 0.0), np.minimum(pairs.t1, end)
        use = pairs.hit & (b > a)
        if active is not None:
            member = np.zeros(len(rec), bool)
            member[np.asarray(active[int(row[0])], np.int64)] = True
            last = np.where(pairs.hit, pairs.t1, 0.0).max(1, keepdims=True)  # an environment ray's last event
            stop = np.where(np.isfinite(end), end, last)
            a = np.where(member[None, :], 0.0, a)
            b = np.where(member[None, :] & ~pairs.hit, stop, b)
            use = np.where(member[None, :], b > a, use)
        tau = np.where(use, pairs.tau(a, b), 0.0).sum(1)
        out[int(row[0])] = np.exp(-tau)
    return out


def band_chords(arrays, rows, x, y, env_samples):
    """[(k, environment sample, Gaussian)] of the rows' environment rays that meet an isotropic Gaussian of
    `arrays` ahead of them with |9 - e2| < CHORD_BAND c (float64 model of the device's whitened test)."""
    mean, s2 = arrays[0].astype(np.float64), arrays[1][:, 0].astype(np.float64)
    hits = []
    for r in rows:
        d = env_directions(x, y, int(r[0]), env_samples)
        v = mean[None, :, :] - r[1:4].astype(np.float64)[None, None, :]
        vv = (v * v).sum(-1)
        vd = (v * d[:, None, :]).sum(-1)
        inb = (np.abs(9.0 - (vv - vd * vd) / s2) < CHORD_BAND * vv / s2) & (vd > 0)
        hits += [(int(r[0]), int(e), int(j)) for e, j in zip(*np.nonzero(inb))]
    return hits


# test_gpu_parity.test_non_positive_definite_record_uses_the_m_forms: its f32 inverse is not positive definite, so
# the scene's secondary rays run the persistent kernel's M-form variant
DEGENERATE_COV = np.float32([0.009235004894435406, 0.06374555826187134, -0.06935998797416687, 0.5371712446212769,
                             -0.32841256260871887, 0.7535938024520874]) * np.float32(2.0 ** -14)


def write_m_form_scene(directory):
    """50_random.txt plus the degenerate Gaussian far outside every ray; returns the new file's path."""
    import os
    src = open(scene_path("50_random.txt")).read().rstrip("\n")
    path = os.path.join(str(directory), "50_random_plus_degenerate.txt")
    with open(path, "w") as f:
        f.write(src + "\ng 0.0 -30.0 0.0  " + " ".join(f"{c:.9g}" for c in DEGENERATE_COV) + "  0.3 0.7  0.1 0.1 0.1\n")
    return path


def lights_of(scene):
    """(positions, intensities) of a vr_amd Scene's lights."""
    ls = scene.lights
    return (np.float32([l.position for l in ls]).reshape(-1, 3), np.float32([l.intensity for l in ls]).reshape(-1, 3))


def oracle_scene(arrays, env=None):
    osc = O.OracleScene.from_gaussians(*arrays)
    if env is not None:
        osc.set_env(env)
    return osc


def oracle_fixture(name, env=None):
    osc = O.OracleScene.load_gmm(scene_path(name))
    if env is not None:
        osc.set_env(env)
    return osc
