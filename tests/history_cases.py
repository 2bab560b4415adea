"""Scenes, probe inputs, probes and histories of the context-history tests (test_history_cases.py checks the inputs on
the CPU, test_gpu_history.py runs the histories on the device).

A device context carries capacity hints, per-scene picks, lazily grown tables and some sixty workspaces from one call
to the next, and the library claims that none of it changes a result. A *history* is a scripted sequence of uploads,
frames and queries on one context; after each of its *check* steps every *probe* of the current scene is compared
with the same probe on a fresh context that got the same options, that one upload and that one probe, and nothing else.

Nothing here touches the device when it is imported: the probes are functions of a context that the GPU test passes in.
Every input is seeded, computed once per key (lru_cache), shared and read-only.
"""
import collections
import functools

import numpy as np

from helpers import CAM_POS, FOV, main_view_dir, render, render_rays, scene_path

F32 = np.float32
N_RAYS = 256   # rays and points of a probe batch (also the 16 x 16 ray grid)
K_PROFILE = 5  # samples per ray of the profile probes
PROFILE_FRACTIONS = F32([0.5, 0.75, 1.0, 1.5, 3.0])  # of the ray's tmax: before it, at it and past it

# ------------------------------------------------------------------------------------------------
# scenes: each one is there for a piece of context state
# ------------------------------------------------------------------------------------------------
GAUSSIAN_SCENES = ("A", "Aenv", "B", "C", "D", "E", "F", "G", "R")
SPHERE_SCENES = ("S2", "S3")
NOTES = {
    "A": "1000_random.txt: translucent (median chord depth 4.5): window 16, refill 24, the phase-scheduled path kernel; "
         "fallback pixels, light rays on the slow path, the list filter switches itself off",
    "Aenv": "A with another environment colour",
    "B": "many_gaussians.txt: 7 Gaussians, the host builder whatever VR_OPT_DEVICE_BVH says",
    "C": "Scene.add_random_gaussians(300): opaque (median chord depth in the hundreds): window 4, refill 56, the bounce "
         "kernel; no lights",
    "D": "aniso_cases needle 100 (512 Gaussians): records that are not positive definite, no tight tree, the M forms",
    "E": "the scene of test_device_tree_without_half_nodes: boxes below the half-node rule, no hnodes",
    "F": "test_gpu_parity._nested_scene(80, 1e-2): the deep march, march_big switches on after the first frame",
    "G": "an empty Gaussian scene",
    "S2": "sph_2_lights.txt (two lights)",
    "S3": "sph_3_spheres.txt",
    "R": "513 Gaussians uploaded from torch tensors (test_gpu_upload_device.agreeing_case)",
}
ENV_OTHER = (0.9, 0.2, 0.1)  # Aenv's environment colour


@functools.lru_cache(maxsize=None)
def scene(name):
    """The vr_amd scene `name` (for R: the host scene of the same floats; resident_scene() is what a context gets)."""
    import vr_amd as vr
    if name in ("A", "Aenv"):
        sc = vr.Scene.load_GMM(scene_path("1000_random.txt"))
        if name == "Aenv":
            sc.env_color = ENV_OTHER
        return sc
    if name == "B":
        return vr.Scene.load_GMM(scene_path("many_gaussians.txt"))
    if name == "C":
        sc = vr.Scene(vr.Scene.GAUSSIANS)
        sc.add_random_gaussians(300)
        return sc
    if name == "D":
        import aniso_cases
        return aniso_cases.device_scene("needle", 100)
    if name == "E":
        import test_gpu_tree
        return test_gpu_tree.scene_of(test_gpu_tree.random_rows(300, 46, 1e-3, 2e-3))
    if name == "F":
        import test_gpu_parity
        return test_gpu_parity._nested_scene(80, 1e-2)[0]
    if name == "G":
        return vr.Scene.from_gaussians(np.zeros((0, 3)), np.zeros((0, 6)), [], [], [vr.Light([0, 1, 0], [1, 1, 1])])
    if name == "R":
        import test_gpu_upload_device as U
        return U.host_scene(U.agreeing_case(), U.LIGHT)
    if name in SPHERE_SCENES:
        return vr.Scene.load_SMM(scene_path({"S2": "sph_2_lights.txt", "S3": "sph_3_spheres.txt"}[name]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def resident_scene():
    """R as a context gets it: a DeviceScene of torch tensors on cuda:0 (needs the GPU)."""
    import torch
    import test_gpu_upload_device as U
    import vr_amd as vr
    return vr.DeviceScene(*(torch.from_numpy(np.array(a)).cuda() for a in U.agreeing_case()), lights=U.LIGHT, env_color=U.ENV)


def is_gaussian(name):
    return name in GAUSSIAN_SCENES


@functools.lru_cache(maxsize=None)
def gaussians(name):
    """(mean (N, 3), cov6 (N, 6), density, albedo (N,)) f32 of Gaussian scene `name`, read-only."""
    g = scene(name).gaussians()
    out = tuple(np.ascontiguousarray(a) for a in (g[:, 0:3], g[:, 3:9], g[:, 9], g[:, 10]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    """The oracle's scene of the same floats (its records and probe are the CPU reference of the preconditions and of
    the float64 gradient models)."""
    import pyoracle as O
    if name in ("A", "Aenv"):
        return O.OracleScene.load_gmm(scene_path("1000_random.txt"))
    if name == "B":
        return O.OracleScene.load_gmm(scene_path("many_gaussians.txt"))
    return O.OracleScene.from_gaussians(*gaussians(name), [(0.0, 4.0, 0.0)], [(1.0, 1.0, 1.0)])


def num_gaussians(name):
    return len(gaussians(name)[0]) if is_gaussian(name) else 0


# ------------------------------------------------------------------------------------------------
# probe inputs
# ------------------------------------------------------------------------------------------------
# tmax per scene, picked as test_gpu_query.py's TMAX_RANGE picks it: (r0, r1, from_first). from_first = False: tmax =
# U(r0, r1 * extent) from the origin; True: the ray's first entry distance (oracle probe) + U(r0, r1), for scenes whose
# Gaussians are opaque (Tr falls from 1 to 0 inside the first one). test_history_cases.py asserts what they are for:
# the oracle's Tr in (0.01, 0.99) on a quarter of the rays at least.
TMAX_RULE = {
    "A": (0.02, 0.3, False), "Aenv": (0.02, 0.3, False), "B": (0.2, 1.0, False), "C": (0.0, 0.004, True),
    "D": (0.0, 0.1, True), "E": (0.0, 4e-6, True), "F": (0.2, 1.0, False), "G": (0.2, 1.0, False), "R": (0.0, 0.06, True),
}

Inputs = collections.namedtuple("Inputs", "cur prev n o d tmax t p w wk w2 tau_target grad_rows")


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _aimed(name, idx, rng):
    """Targets inside the Gaussians idx % N of `name`: mean + chol(cov) (r u), u a uniform direction, r in [0, 2]."""
    mean, cov6, _, _ = gaussians(name)
    g = idx % len(mean)
    c = cov6[g].astype(np.float64)
    cov = np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], -1), np.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                    np.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], -2)
    w, v = np.linalg.eigh(cov)
    root = v * np.sqrt(np.maximum(w, 0.0))[:, None, :]  # cov = root root^T (a covariance rounded to f32 may not be PD)
    r = rng.uniform(0.0, 2.0, len(idx))
    return mean[g].astype(np.float64) + np.einsum("nij,nj->ni", root, r[:, None] * _unit(rng, len(idx)))


def extent(name):
    """The largest edge of the scene's bounding box (of the Gaussians' 3-sigma boxes)."""
    info = scene(name).info()
    return float(np.max(np.array(list(info.bounds_max), np.float64) - np.array(list(info.bounds_min), np.float64)))


def _bounds(names):
    m = np.concatenate([gaussians(s)[0].astype(np.float64) for s in names])
    return m.min(0), m.max(0)


@functools.lru_cache(maxsize=None)
def rays(cur, prev, n=N_RAYS):
    """The common ray batch of two scenes that follow each other in a history (prev may be cur, or None at a history's
    start): default_rng(7); a quarter by test_gpu_query.py's recipe on the union of the two scenes' bounds (origins
    around the box, aimed into its inner 70 %), the rest aimed at points inside the Gaussians of cur and of prev in
    turn from 0.5 to 2 away. Directions are left unnormalised. An empty scene adds nothing to aim at."""
    names = [s for s in dict.fromkeys((cur, prev)) if s is not None and is_gaussian(s) and num_gaussians(s) > 0]
    rng = np.random.default_rng(7)
    if not names:
        names = ["B"]  # (the empty scene at a history's start: any rays will do)
    lo, hi = _bounds(names)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    nbox = n // 4
    o = rng.uniform(lo - 0.5, hi + 0.5, (n, 3))
    tgt = rng.uniform(c - 0.7 * h, c + 0.7 * h, (n, 3))
    k = np.arange(n - nbox)
    for j, s in enumerate(names):
        sel = k[k % len(names) == j]
        tgt[nbox + sel] = _aimed(s, sel // len(names), rng)
    o[nbox:] = tgt[nbox:] + _unit(rng, n - nbox) * rng.uniform(0.5, 2.0, n - nbox)[:, None]
    o = o.astype(F32)
    d = (tgt.astype(F32) - o).astype(F32)
    for a in (o, d):
        a.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def oracle_probe(name, cur, prev, n=N_RAYS):
    """(hit (n, N) bool, t_enter, t_exit (n, N) f32) of scene `name` along rays(cur, prev, n)."""
    import grad_reference as R
    out = R.probe(oracle_scene(name), *rays(cur, prev, n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tmax_of(cur, prev, n=N_RAYS):
    """(n,) f32 by cur's TMAX_RULE."""
    r0, r1, from_first = TMAX_RULE[cur]
    u = np.random.default_rng(7)
    if from_first:
        hit, te, _ = oracle_probe(cur, cur, prev, n)
        first = np.where(hit, te, np.inf).min(1)
        tmax = (np.where(np.isfinite(first), first, 1.0) + u.uniform(r0, r1, n)).astype(F32)
    else:
        tmax = u.uniform(r0, r1 * extent(cur if num_gaussians(cur) else "B"), n).astype(F32)
    tmax.setflags(write=False)
    return tmax


@functools.lru_cache(maxsize=None)
def oracle_tau(name, cur, prev, n=N_RAYS):
    """(n,) float64: the optical depth of scene `name` along rays(cur, prev) up to tmax_of(cur, prev), by
    grad_reference's model (the f32 probe's hit set and clip bounds, the closed form in float64)."""
    import grad_reference as R
    if num_gaussians(name) == 0:
        return np.zeros(n)
    o, d = rays(cur, prev, n)
    tmax = tmax_of(cur, prev, n)
    hit, te, tx = oracle_probe(name, cur, prev, n)
    rec = oracle_scene(name).records().astype(np.float64)
    a = np.maximum(F32(0), te)
    b = np.minimum(tmax[:, None], tx)
    use = hit & (b > a)
    a64, b64 = np.where(use, a, 0.0).astype(np.float64), np.where(use, b, 1.0).astype(np.float64)
    with np.errstate(all="ignore"):  # (terms outside `use` are formed and dropped)
        tau = R.tau_terms(rec[:, :3], R.sym(rec[:, 4:10]), rec[:, 10], rec[:, 3], o.astype(np.float64),
                          R.normalized_f32(d).astype(np.float64), a64, b64, use).sum(1)
    tau.setflags(write=False)
    return tau


@functools.lru_cache(maxsize=None)
def sigma_points(cur, n=N_RAYS):
    """(n, 3) f32 points of the sigma probes: sigma_grad_reference's recipe (point i in Gaussian i % N, up to 3.3 sigma
    from its mean) without the points within Q_MARGIN of a cut-off, where f32 and float64 may pick another active set
    (kept_recipe's rule; 1.5 n are drawn, the first n of the rest kept). An empty scene gets points of the unit box."""
    import sigma_grad_reference as SR
    if num_gaussians(cur) == 0:
        p = np.random.default_rng(7).uniform(-1.0, 1.0, (n, 3)).astype(F32)
    elif cur == "D":  # (records that are not positive definite have no Cholesky factor: the rung's own aimed points)
        import aniso_cases
        case = aniso_cases.sigma_case("needle", 100)
        p = case.p[case.keep][:n]
        assert len(p) == n
    else:
        rec = SR.records_of_oracle(oracle_scene(cur).records())
        x = SR.recipe_points(rec, n + n // 2)
        x = x[np.isfinite(x).all(1)]
        p = x[~SR.Model(rec, x).near][:n]
        assert len(p) == n, (cur, len(p))
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


# The two ray gradients take N_GRAD rays of the batch: their float64 models hold every (ray, Gaussian) term of both
# bound rules in memory and take seconds per 256 rays of a 1000-Gaussian scene on the CPU; the atomics, the staging
# and its zeroing are the same for 64 rays. The sigma gradient's model is cheap and takes all the points.
N_GRAD = 64


@functools.lru_cache(maxsize=None)
def gradient_rows(cur, prev, n=N_RAYS):
    """The rows of rays(cur, prev) that the two ray-gradient probes take: the first N_GRAD on which the oracle's probe
    hits no record whose M is not positive definite. The closed form's sqrt(d^T M d) has no float64 counterpart on
    such a record, so the float64 model is no reference there (Elongated Gaussians: needle 100 is
    measured on the rays on no such record). Only D has such records."""
    import aniso_cases
    if num_gaussians(cur) == 0:
        return np.arange(min(n, N_GRAD))
    not_pd = aniso_cases.record_health(oracle_scene(cur).records())[1]
    rows = np.arange(n)
    if not_pd.any():
        rows = rows[~oracle_probe(cur, cur, prev, n)[0][:, not_pd].any(1)]
    assert len(rows) >= N_GRAD, (cur, prev, len(rows))
    rows = rows[:N_GRAD]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def inputs(cur, prev, n=N_RAYS):
    """Everything the probes of scene `cur` read when it follows `prev`."""
    o, d = rays(cur, prev, n)
    tmax = tmax_of(cur, prev, n)
    rng = np.random.default_rng(11)
    t = np.ascontiguousarray(tmax[:, None] * PROFILE_FRACTIONS[None, :])
    w = rng.uniform(-1, 1, n).astype(F32)
    wk = rng.uniform(-1, 1, (n, K_PROFILE)).astype(F32)
    w2 = rng.uniform(-1, 1, (n, 2)).astype(F32)
    tau_target = rng.uniform(0.05, 2.0, n).astype(F32)
    for a in (t, w, wk, w2, tau_target):
        a.setflags(write=False)
    return Inputs(cur, prev, n, o, d, tmax, t, sigma_points(cur, n), w, wk, w2, tau_target, gradient_rows(cur, prev, n))


@functools.lru_cache(maxsize=None)
def warm_inputs(cur, n):
    """A larger or smaller batch for the steps that only give a context its history (no oracle behind it: tmax by the
    from-the-origin rule whatever the scene)."""
    o, d = rays(cur, None, n)
    rng = np.random.default_rng(13)
    lo, hi = _bounds([cur])
    tmax = rng.uniform(0.05, 0.5 * extent(cur), n).astype(F32)
    t = np.ascontiguousarray(tmax[:, None] * PROFILE_FRACTIONS[None, :])
    p = rng.uniform(lo, hi, (n, 3)).astype(F32)
    return Inputs(cur, None, n, o, d, tmax, t, p, rng.uniform(-1, 1, n).astype(F32), rng.uniform(-1, 1, (n, K_PROFILE)).astype(F32),
                  rng.uniform(-1, 1, (n, 2)).astype(F32), rng.uniform(0.05, 2.0, n).astype(F32), np.arange(n))  # (no model behind a warm-up: every ray)


# ------------------------------------------------------------------------------------------------
# the scene heuristics, restated (vr_upload.cpp)
# ------------------------------------------------------------------------------------------------
def median_chord_depth(rec):
    """scene_median_chord_depth of vr_upload.cpp in numpy from Scene.records() rows (mean3, density, inv_cov 00 01 02 11
    12 22, norm, albedo): the median (element of rank n / 2) over up to 4096 sampled Gaussians of density * norm *
    sqrt(2 pi / d^T M d) along one of four fixed directions in turn."""
    rec = np.asarray(rec)
    N = len(rec)
    if N == 0:
        return 0.0
    step = max(1, N // 4096)
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [F32(0.57735027)] * 3], np.float64)
    r = rec[::step].astype(np.float64)
    d = dirs[np.arange(len(r)) & 3]
    m = r[:, 4:10]
    a = (m[:, 0] * d[:, 0] * d[:, 0] + m[:, 3] * d[:, 1] * d[:, 1] + m[:, 5] * d[:, 2] * d[:, 2]
         + 2.0 * (m[:, 1] * d[:, 0] * d[:, 1] + m[:, 2] * d[:, 0] * d[:, 2] + m[:, 4] * d[:, 1] * d[:, 2]))
    ok = (a > 0.0) & np.isfinite(a)
    with np.errstate(all="ignore"):
        tau = (r[:, 3] * r[:, 10] * np.sqrt(2.0 * np.pi / a))[ok]
    if len(tau) == 0:
        return 0.0
    return float(np.sort(tau)[len(tau) // 2])


def half_node_rule(name):
    """(median box extent, 3 % of the scene's half extent): half_tree_rule of vr_upload.cpp on the primitive boxes, the
    device builder's input (tree_reference.prim_boxes restates gaussian_bounds bit for bit)."""
    import tree_reference as T
    pb = T.prim_boxes(scene(name).gaussians()).astype(np.float64)
    half = float(np.max(0.5 * (pb[:, 3:6].max(0) - pb[:, 0:3].min(0))))
    ext = np.sort(np.max(pb[:, 3:6] - pb[:, 0:3], axis=1).astype(F32))
    return float(ext[len(ext) // 2]), 0.03 * half


# ------------------------------------------------------------------------------------------------
# probes: a named call on a context with its current scene; each returns a dict of arrays
# ------------------------------------------------------------------------------------------------
def camera(pos=None):
    import vr_amd as vr
    return vr.Pinhole_Camera(CAM_POS if pos is None else pos, main_view_dir(), FOV)


FAR_CAMERA = F32([0.0, 1.0, 60.0])  # 60 units away on the main camera's axis: a long step table
STAT_KEYS = ("pixels", "fallback_pixels", "error_pixels", "scatter_records", "deep_pixels")


def _march(dev, sc, inp, t_eps=0.0, first=True, W=32):
    import vr_amd as vr
    out = {"frame": render(dev, vr.RayMarchingGaussians(camera(), env_samples=4, t_eps=t_eps), W, W)}
    st = dev.stats()
    if first:  # the counts that belong to a context's first ray-march frame of a scene (compare() has the rule)
        out["stats"] = np.array([st[k] for k in STAT_KEYS], np.int64)
    out["filtered_rays"] = np.array([st["filtered_rays"], st["scatter_records"] * 4], np.int64)  # (of the environment rays)
    out["records_centre"] = dev.debug_pixel_records(W // 2, W // 2)
    out["records_rim"] = dev.debug_pixel_records(1, W // 2)
    return out


def probe_march(dev, sc, inp):
    """RayMarchingGaussians 32 x 32, 4 environment samples, t_eps 0; then the frame's counts and two pixels' records."""
    return _march(dev, sc, inp)


def probe_march_eps(dev, sc, inp):
    """The same at t_eps 1e-3 (the rec_cut path, and the list filter has rays to cut), without the counts."""
    return _march(dev, sc, inp, t_eps=1e-3, first=False)


def probe_march_second(dev, sc, inp):
    """The march probe's frame rendered twice: the counts of the second rendering. A fresh context's second frame of a
    scene is what a context reports whose march_big was switched on by an earlier frame (compare() has the rule)."""
    _march(dev, sc, inp)
    return _march(dev, sc, inp)


def probe_march_far(dev, sc, inp):
    """The march frame alone from FAR_CAMERA (its step table is ten times the main camera's)."""
    import vr_amd as vr
    return {"frame": render(dev, vr.RayMarchingGaussians(camera(FAR_CAMERA), env_samples=4), 32, 32)}


def probe_march_frame(dev, sc, inp):
    """The march frames alone, t_eps 0 and 1e-3 (a multi-GPU context: the records and counts are per rank)."""
    import vr_amd as vr
    return {"frame": render(dev, vr.RayMarchingGaussians(camera(), env_samples=4), 32, 32),
            "frame_eps": render(dev, vr.RayMarchingGaussians(camera(), env_samples=4, t_eps=1e-3), 32, 32)}


def probe_pure(dev, sc, inp):
    import vr_amd as vr
    return {"frame": render(dev, vr.PureRayMarching(camera(), env_samples=4), 24, 24)}


def probe_freeflight(dev, sc, inp):
    import vr_amd as vr
    return {"frame": render(dev, vr.FreeFlightGaussians(camera(), 4), 24, 24)}


def probe_multi(dev, sc, inp):
    """MultiScatterGaussians 24 x 24, 4 spp, recorded into slots 0 and 1, with the two bitsets."""
    import ctypes
    import vr_amd as vr
    from vr_amd import _lib as L
    integ = vr.MultiScatterGaussians(camera(), 4)
    out = {}
    for slot in (0, 1):
        out[f"frame{slot}"] = render(dev, integ, 24, 24, slot=slot)
    N = num_gaussians(inp.cur)
    for slot in (0, 1):
        b = np.zeros(((N + 31) // 32, 24 * 24), np.uint32)
        if b.size:
            L.check(L.lib().vr_get_pixel_gaussians(dev._h, slot, b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), b.size))
        out[f"bits{slot}"] = b
    return out


def probe_raygrid(dev, sc, inp):
    """The first 256 rays of the batch as a 16 x 16 grid through vr_render_rays, with its transmittance."""
    import vr_amd as vr
    rgb, tr = render_rays(dev, vr.RayMarchingGaussians(camera(), env_samples=4), inp.o[:256].reshape(16, 16, 3),
                          inp.d[:256].reshape(16, 16, 3))
    return {"rgb": rgb, "tr": tr}


def probe_spheres(dev, sc, inp):
    import vr_amd as vr
    return {"frame": render(dev, vr.RayMarchingSpheres(camera()), 24, 24)}


def probe_hitmask(dev, sc, inp):
    import vr_amd as vr
    return {"frame": render(dev, vr.TestIntegrator(camera()), 24, 24)}


def probe_tree(dev, sc, inp):
    tree = dev.debug_tree()
    info = tree.pop("info")
    for k, v in info.items():
        tree["info." + k] = np.asarray(v)
    return tree


def _kind(as_torch):
    if not as_torch:
        return (lambda a: a), (lambda a: np.asarray(a))
    import torch
    return (lambda a: torch.from_numpy(np.array(a)).cuda()), (lambda a: a.cpu().numpy())


def _q_transmittance(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    tr, tau = dev.query_transmittance(sc, to(inp.o), to(inp.d), tmax=to(inp.tmax), return_tau=True)
    return {"tr": back(tr), "tau": back(tau)}


def _q_events(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    off, t, g, entering = dev.query_events(sc, to(inp.o), to(inp.d))
    return {"off": back(off).astype(np.int64), "t": back(t), "g": back(g).astype(np.int32), "in": back(entering).astype(np.uint8)}


def _q_sigma(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    sig, act = dev.query_sigma(sc, to(inp.p), return_active=True)
    return {"sigma": back(sig), "active": back(act).astype(np.int32)}


def _q_free_flight(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    t, alb, act = dev.query_free_flight(sc, to(inp.o), to(inp.d), to(inp.tau_target), return_albedo=True, return_active=True)
    return {"t": back(t), "albedo": back(alb), "active": back(act).astype(np.int32)}


def _q_ray_grad(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    go, gd, gt, tau = dev.query_transmittance_ray_grad(sc, to(inp.o), to(inp.d), tmax=to(inp.tmax))
    return {"d_origin": back(go), "d_direction": back(gd), "d_tmax": back(gt), "tau": back(tau)}


def _q_profile(dev, sc, inp, as_torch):
    to, back = _kind(as_torch)
    tr, tau = dev.query_transmittance_profile(sc, to(inp.o), to(inp.d), to(inp.t), return_tau=True)
    return {"tr": back(tr), "tau": back(tau)}


def _g_transmittance(dev, sc, inp, as_torch=False):
    k = inp.grad_rows
    return {"grad": dev.query_transmittance_grad(sc, inp.o[k], inp.d[k], inp.w[k], tmax=inp.tmax[k])}


def _g_profile(dev, sc, inp, as_torch=False):
    k = inp.grad_rows
    return {"grad": dev.query_transmittance_profile_grad(sc, inp.o[k], inp.d[k], inp.t[k], inp.wk[k])}


def _g_sigma(dev, sc, inp, as_torch=False):
    g, gx = dev.query_sigma_grad(sc, inp.p, inp.w2, gaussians=True, positions=True)
    return {"grad": g, "grad_xyz": gx}


FORWARD_QUERIES = {"transmittance": _q_transmittance, "events": _q_events, "sigma": _q_sigma, "free_flight": _q_free_flight,
                   "ray_grad": _q_ray_grad, "profile": _q_profile}
ATOMIC_GRADIENTS = {"grad": _g_transmittance, "profile_grad": _g_profile, "sigma_grad": _g_sigma}

PROBES = {"march": probe_march, "march_eps": probe_march_eps, "pure": probe_pure, "freeflight": probe_freeflight,
          "multi": probe_multi, "raygrid": probe_raygrid, "march_far": probe_march_far, "march_second": probe_march_second,
          "march_frame": probe_march_frame, "spheres": probe_spheres, "hitmask": probe_hitmask, "tree": probe_tree}
for _name, _fn in FORWARD_QUERIES.items():
    PROBES[_name + ".numpy"] = functools.partial(_fn, as_torch=False)
    PROBES[_name + ".torch"] = functools.partial(_fn, as_torch=True)
for _name, _fn in ATOMIC_GRADIENTS.items():
    PROBES[_name] = _fn

FRAME_PROBES = ("march", "march_eps", "pure", "freeflight", "multi", "raygrid")  # a fresh context each, always
FREE_FLIGHT_PROBES = ("freeflight", "multi")
MARCH_PROBES = ("march", "march_eps", "pure", "raygrid")
GROUP_PROBES = ("march_frame", "pure", "freeflight")  # the frame probes of a two-rank group
BATCH_FREE = ("tree", "march", "march_second", "march_eps", "pure", "freeflight", "multi", "march_far", "march_frame", "spheres", "hitmask")
SPHERE_PROBES = ("spheres", "hitmask")
QUERY_PROBES = tuple(k for k in PROBES if "." in k)
GRADIENT_PROBES = tuple(ATOMIC_GRADIENTS)
# atomic gradients: the key that is summed with atomics (every other key of these probes is bit-equal like the rest)
ATOMIC_KEYS = {("grad", "grad"), ("profile_grad", "grad"), ("sigma_grad", "grad")}


def probes_of(name):
    """The probes of a scene, in the order a check runs them."""
    if name in SPHERE_SCENES:
        return SPHERE_PROBES
    return ("tree",) + FRAME_PROBES + QUERY_PROBES + GRADIENT_PROBES


# ------------------------------------------------------------------------------------------------
# float64 models of the three atomic gradients (grad_reference, profile_reference, sigma_grad_reference)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradient_model(probe, cur, prev):
    """(G64, S) of an atomic-gradient probe on inputs(cur, prev), from the module that owns the query's model."""
    inp = inputs(cur, prev)
    k = inp.grad_rows
    if probe == "grad":
        import grad_reference as R
        with np.errstate(all="ignore"):  # (terms outside the hit set are formed and dropped)
            return R.Model(oracle_scene(cur), inp.o[k], inp.d[k], inp.tmax[k]).grad(inp.w[k], True)
    if probe == "profile_grad":
        import profile_reference as P
        return P.ProfileModel(oracle_scene(cur), inp.o[k], inp.d[k], inp.t[k]).grad(inp.wk[k], True)
    import sigma_grad_reference as SR
    return SR.Model(SR.records_of_oracle(oracle_scene(cur).records()), inp.p).grad(inp.w2)


# ------------------------------------------------------------------------------------------------
# histories (the generators of test_gpu_history.py): the batches their check steps read
# ------------------------------------------------------------------------------------------------
# The check steps of each history, which its generator in test_gpu_history.py walks: (scene, the Gaussian scene whose
# common batch with it the probes read, or None for the scene's own batch).
SEQUENCES = {
    "1-large-then-small": (("B", "A"), ("G", "B"), ("B", "G")),
    "2-small-then-large": (("A", "B"),),
    "3-kinds-lights-environment": (("S2", None), ("B", None), ("S3", None), ("Aenv", "B"), ("S2", None)),
    "4-trees": (("A", None), ("D", "A"), ("E", "D"), ("R", "E"), ("A", "R")),
    "5-heuristic-state": (("F", None), ("B", "F"), ("A", "B"), ("C", "A"), ("A", "C")),
    "6-tables": (("B", None),),
    "7-option-round-trip": (("A", None),),
    "8-queries-between-frames": (("A", None),),
}
# Every (Gaussian scene, previous scene) batch that a check reads; test_history_cases.py checks each of them.
PAIRS = tuple(dict.fromkeys(pair for seq in SEQUENCES.values() for pair in seq if pair[0] in GAUSSIAN_SCENES))
