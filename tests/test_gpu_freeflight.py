"""GPU parity of the free-flight integrators through the C ABI:
FreeFlightGaussians (integrator.h:300-408) and MultiScatterGaussians (integrator.h:532-717) vs the
oracle's restatement (oracle/vr_oracle.cpp free_flight_pixel).

Both sides follow each path (pixel, sample) with the same PCG32 stream, bit-identical camera rays
and ellipsoid distances, and the same solver; libm (log, erf, acos, sin, cos) differs from the
device library by a few ulp, so a path whose discrete decision (scatter-or-not in a segment,
Russian roulette, light choice) lands within an ulp can diverge. Bar: at least 99.9 % of pixels
within 1e-4 L-inf, mean |diff| < 1e-4, image means within 0.5 % (measured on MI355X: 100 % of
pixels within 1e-4, mean |diff| ~1e-8).
"""
import ctypes

import numpy as np
import pytest

import pyoracle as O
import vr_amd as vr
from helpers import CAM_POS, FOV, main_view_dir, scene_path

pytestmark = pytest.mark.gpu


def _gpu(scene, W, H, multi, spp, min_bounces=5, cam=None, stats=None):
    camera = cam or vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    integ = vr.MultiScatterGaussians(camera, spp, min_bounces) if multi else vr.FreeFlightGaussians(camera, spp)
    img = vr.Image(W, H)
    integ.render(scene, img)
    if stats is not None:
        stats.update(integ.last_stats)
    return img.pixels.copy()


def _check(g, r, frac_min=0.999, mean_max=1e-4):
    g = np.asarray(g, np.float64)
    r = np.asarray(r, np.float64)
    assert not np.isnan(g).any()
    d = np.abs(g - r).max(axis=-1)
    frac = float(np.mean(d <= 1e-4))
    mean = float(d.mean())
    rel = abs(g.mean() - r.mean()) / max(abs(r.mean()), 1e-12)
    print(f"frac<=1e-4 {frac:.4f} mean|d| {mean:.2e} image-mean rel {rel:.2e}")
    assert frac >= frac_min, frac
    assert mean <= mean_max, mean
    assert rel <= 5e-3, rel


@pytest.mark.parametrize("name,W,spp", [
    ("1_gaussian.txt", 48, 4),
    ("2_gaussian.txt", 48, 16),
    ("many_gaussians.txt", 48, 16),
    ("50_random.txt", 40, 4),
    ("god_ray.txt", 40, 4),
])
@pytest.mark.parametrize("multi", [False, True])
def test_free_flight_matches_oracle(name, W, spp, multi):
    path = scene_path(name)
    g = _gpu(vr.Scene.load_GMM(path), W, W, multi, spp)
    r = O.render_ff(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, W, W, multi=multi,
                    num_samples=spp)
    _check(g, r)


def test_multi_scatter_orthographic_and_min_bounces():
    path = scene_path("many_gaussians.txt")
    vd = main_view_dir()
    cam = vr.Orthographic_Camera(CAM_POS, vd)
    g = _gpu(vr.Scene.load_GMM(path), 40, 40, True, 4, min_bounces=1, cam=cam)
    r = O.render_ff(O.OracleScene.load_gmm(path), O.ORTHO, CAM_POS, vd, 0.0, 40, 40, multi=True, num_samples=4,
                    min_bounces=1)
    _check(g, r)


def test_many_overlapping_hits_use_several_windows():
    # 400 Gaussians strung along the central ray: > 128 hits per ray forces the bounded hit buffer to
    # cut the event sweep into windows; results must still follow the sorted-event reference.
    rng = np.random.default_rng(7)
    n = 400
    z = np.linspace(-1.5, 1.5, n).astype(np.float32)
    mean = np.stack([rng.uniform(-0.05, 0.05, n), 1.0 + rng.uniform(-0.05, 0.05, n), z], 1).astype(np.float32)
    s2 = rng.uniform(0.02, 0.05, n).astype(np.float32) ** 2
    cov6 = np.stack([s2, np.zeros(n), np.zeros(n), s2, np.zeros(n), s2], 1).astype(np.float32)
    dens = np.full(n, 0.02, np.float32)
    alb = rng.uniform(0.5, 0.9, n).astype(np.float32)
    lights = [vr.Light((0.0, 4.0, 0.0), (30.0, 30.0, 30.0))]
    scene = vr.Scene.from_gaussians(mean, cov6, dens, alb, lights=lights)
    oscene = O.OracleScene.from_gaussians(mean, cov6, dens, alb, np.array([[0, 4, 0]], np.float32),
                                          np.array([[30, 30, 30]], np.float32))
    W = 24
    for multi in (False, True):
        g = _gpu(scene, W, W, multi, 4)
        r = O.render_ff(oscene, O.PINHOLE, CAM_POS, main_view_dir(), FOV, W, W, multi=multi, num_samples=4)
        _check(g, r)


def test_free_flight_is_deterministic_and_tiles_agree():
    path = scene_path("many_gaussians.txt")
    scene = vr.Scene.load_GMM(path)
    a = _gpu(scene, 40, 40, True, 4)
    b = _gpu(scene, 40, 40, True, 4)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("multi", [False, True])
def test_free_flight_tile_slabs_unshuffle_bitwise(multi):
    """The multi-GPU building block with the free-flight integrators: rank r of 3 renders tiles
    r, r+3, ... into a packed slab (its own sample batches and running sums); the unshuffled frame
    equals the single-call frame bit for bit (paths depend only on (x, y, si))."""
    torch = pytest.importorskip("torch")
    path = scene_path("50_random.txt")
    W, H = 70, 50
    scene = vr.Scene.load_GMM(path)
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    integ = vr.MultiScatterGaussians(cam, 4) if multi else vr.FreeFlightGaussians(cam, 4)
    full = vr.Image(W, H)
    integ.render(scene, full)
    dev = vr.Device.get(0)
    dev.upload(scene)
    nt = vr.num_tiles(W, H)
    R = 3
    per = (nt + R - 1) // R
    slabs = torch.zeros((R, per * 256 * 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for r in range(R):
        cnt = len(range(r, nt, R))
        for _ in range(4):  # each share's outcome is checked before the next share's call (finish_local's rule)
            dev.render_tiles_device(cam, integ.params, W, H, r, R, cnt, True, slabs[r].data_ptr(), stream)
            try:
                dev.synchronize()
                break
            except vr.VRError as e:
                assert e.status == vr._lib.VR_ERR_RETRY
    img = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    dev.unshuffle_tiles_device(slabs.data_ptr(), R, per, W, H, img.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), full.pixels)


def test_free_flight_needs_a_gaussian_scene():
    scene = vr.Scene.load_SMM(scene_path("sph_1_spheres.txt"))
    with pytest.raises(vr.VRError):
        _gpu(scene, 16, 16, True, 1)


def test_empty_scene_free_flight_is_env():
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.env_color = (0.25, 0.5, 0.75)
    g = _gpu(scene, 16, 16, True, 4)
    s = np.float32(0.0)
    for _ in range(4):
        s = np.float32(s + np.float32(0.25))
    assert np.all(g[..., 0] == np.float32(s / np.float32(4)))


def _coincident_scene(n):
    """n coincident Gaussians at (0, 1, 0) (sigma 0.2): all n overlap every point of the central rays."""
    mean = np.tile(np.float32([0.0, 1.0, 0.0]), (n, 1))
    cov6 = np.tile(np.float32([0.04, 0, 0, 0.04, 0, 0.04]), (n, 1))
    dens = np.full(n, 0.01, np.float32)
    alb = np.full(n, 0.8, np.float32)
    light = ((0.0, 4.0, 0.0), (30.0, 30.0, 30.0))
    dev = vr.Scene.from_gaussians(mean, cov6, dens, alb, lights=[vr.Light(*light)])
    orc = O.OracleScene.from_gaussians(mean, cov6, dens, alb, [light[0]], [light[1]])
    return dev, orc


@pytest.mark.parametrize("multi", [False, True])
def test_overlap_beyond_the_hit_buffer_matches_oracle(multi):
    """200 coincident Gaussians: more than the path kernel's 128-entry rows overlap at one point. Those
    paths re-run whole in ff_fallback_kernel (1024-entry rows, inline shadow rays); the reference's
    event lists are unbounded (integrator.h:422-498), so the image must match the oracle."""
    scene, orc = _coincident_scene(200)
    st = {}
    g = _gpu(scene, 16, 16, multi, 4, stats=st)
    r = O.render_ff(orc, O.PINHOLE, CAM_POS, main_view_dir(), FOV, 16, 16, multi=multi, num_samples=4)
    assert st["fallback_pixels"] > 0 and st["error_pixels"] == 0  # paths re-run with the large rows
    _check(g, r)


def test_overlap_beyond_every_capacity_fails_loudly():
    # more Gaussians overlapping one point than even the fallback's rows hold (kFFBigCap = 1024): the
    # render must fail (VR_ERR_OVERFLOW), not return garbage
    scene, _ = _coincident_scene(1100)
    with pytest.raises(vr.VRError):
        _gpu(scene, 8, 8, True, 1)


@pytest.mark.parametrize("cap0", ["1", "128"])
def test_window_capacity_does_not_change_results(cap0, device_options):
    # first-window capacity 1 (a window per event) vs 128 (one window): the event sweep must be the
    # reference's either way
    device_options("ff_window0", int(cap0))
    path = scene_path("50_random.txt")
    g = _gpu(vr.Scene.load_GMM(path), 32, 32, True, 4)
    r = O.render_ff(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, 32, 32, multi=True,
                    num_samples=4)
    _check(g, r)


@pytest.mark.parametrize("name", ["20k_bias.txt", "5000_random.txt", "10k_random.txt"])
def test_dense_reference_scenes_stay_within_the_hit_capacity(name):
    """The per-path hit buffer holds 128 Gaussians overlapping one point (the only capacity a path
    can exceed, test_overlap_beyond_capacity_fails_loudly). The reference's densest scenes (20k_bias:
    y-skewed, 20k Gaussians) render at the C5 settings without reaching it, and match the oracle
    (stable tie order, the device's rule for tangent hits)."""
    path = scene_path(name)
    g = _gpu(vr.Scene.load_GMM(path), 64, 64, True, 4)
    with O.stable_ties():
        r = O.render_ff(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, 64, 64, multi=True,
                        num_samples=4)
    # (the densest scenes give libm-ulp divergences the most chances: 10k_random measured 99.80 % of pixels
    # within 1e-4 on MI355X, mean |diff| 8.9e-7; the other scenes 100 %)
    _check(g, r, frac_min=0.995)


def test_reference_driver_default_render_matches_oracle():
    """The reference driver's own forward workload (tests/main.cpp:17-45): MultiScatterGaussians on
    2g_altered.txt at 512x512, here at 64 paths per pixel (the driver uses 256; bench.py --config main
    times that), full frame. Every path follows the oracle's (same PCG32 stream per pixel and sample)."""
    path = scene_path("2g_altered.txt")
    W = H = 512
    g = _gpu(vr.Scene.load_GMM(path), W, H, True, 64)
    r = O.render_ff(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, W, H, multi=True,
                    num_samples=64)
    _check(g, r)


@pytest.mark.parametrize("multi,kernel", [(False, 0), (True, 0), (False, 2), (True, 2)],
                         ids=["False", "True", "False-phase", "True-phase"])
def test_deferred_shadow_rays_equal_inline(multi, kernel, device_options):
    """VR_OPT_FF_NEE_QUEUE: the path kernel queues each bounce's shadow ray for ff_nee_kernel (the same
    walk and double sum as an inline transmittance_up_to), linked per path, and the accumulation adds a
    path's contributions in bounce order, so frames equal inline NEE bit for bit while the queue has
    room. A queue of 1 ray per path fills in every launch (its paths would switch to inline NEE mid-path
    and add those contributions as one partial sum): the frame is rendered again with every shadow ray
    inline, so it is the same frame bit for bit too (round 5; until then float association only).
    kernel: VR_OPT_FF_KERNEL, the scene's default kernel (0) and the phase-scheduled kernel forced (2)."""
    scene = vr.Scene.load_GMM(scene_path("50_random.txt"))
    device_options("ff_kernel", kernel)
    frames = {}
    for q in (0, 16, 1):
        device_options("ff_nee_queue", q)
        frames[q] = _gpu(scene, 40, 40, multi, 16)
    for q in (16, 1):
        assert np.array_equal(frames[q], frames[0]), f"queue {q}: max|d| {np.abs(frames[q] - frames[0]).max():.2e}"


def _fresh_render(scene, integ, W, H, **opts):
    """vr_render on a context of its own (no capacity hints from earlier frames)."""
    dev = vr.Device(0)
    for k, v in opts.items():
        dev.set_option(k, v)
    dev.upload(scene)
    out = np.empty((H, W, 3), np.float32)
    vr.check(vr.lib().vr_render(dev._h, ctypes.byref(integ.camera.struct), ctypes.byref(integ.params), W, H, vr.fptr(out)))
    return out, dev


def test_first_frame_queue_sizing_equals_queue_at_its_bound():
    """A fresh context sizes the shadow-ray queue of its first frame from the integrator (one ray per
    bounce up to min_bounces + 1), so a MultiScatter frame with min_bounces = 1 outgrows it: the frame is
    rendered again with a grown queue (up to 3 doublings, then inline) and equals the frame rendered with
    the queue at its bound from the start (VR_OPT_FF_NEE_QUEUE = 16) bit for bit."""
    scene = vr.Scene.load_GMM(scene_path("50_random.txt"))
    integ = vr.MultiScatterGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), 16, 1)
    a, _ = _fresh_render(scene, integ, 48, 40)
    b, _ = _fresh_render(scene, integ, 48, 40, ff_nee_queue=16)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("window0", [0, 2])
def test_multiscatter_frame_is_deterministic(window0):
    """The same frame from three fresh contexts, bit for bit, on the C2
    scene with many hit windows. A window's cut once depended on whether the walk had skipped a subtree
    while the hit buffer was full, which depends on the wave's NODE/PRIM schedule (so on which paths
    shared the wave): about 100 of the C2 bench frame's 262k pixels then differed by an ulp from run to
    run (round 5). A full buffer now always ends its window at its largest kept key."""
    scene = vr.Scene.load_GMM(scene_path("1000_random.txt"))
    integ = vr.MultiScatterGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), 4, 5)
    opts = {"ff_window0": window0} if window0 else {}
    frames = [_fresh_render(scene, integ, 160, 160, **opts)[0] for _ in range(3)]
    for k, f in enumerate(frames[1:], 1):
        d = np.abs(f - frames[0])
        assert np.array_equal(f, frames[0], equal_nan=True), f"frame {k}: {int((d.max(-1) > 0).sum())} pixels differ, max {np.nanmax(d):.2e}"


@pytest.mark.parametrize("name,multi,tree", [("1000_random.txt", True, {}), ("1000_random.txt", False, {}),
                                             ("50_random.txt", True, {}), ("many_gaussians.txt", True, {}),
                                             ("2g_altered.txt", True, {}), ("1000_random.txt", True, {"half_nodes": 0}),
                                             ("1000_random.txt", True, {"device_bvh": 1})])
def test_phase_scheduled_kernel_equals_bounce_kernel(name, multi, tree):
    """VR_OPT_FF_KERNEL: the phase-scheduled path kernel (each wave iteration runs the collection, sweep or
    shading phase most of its lanes are in) and the bounce kernel run every path's operations in the same
    order, so their frames are equal bit for bit, with a small first window (many windows) too, without
    the half-precision trees (VR_OPT_HALF_NODES = 0: every walk on the f32 pair tree) and on the device
    linear BVH; a ragged frame (90 x 70: tiles with pixels outside it)."""
    scene = vr.Scene.load_GMM(scene_path(name))
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    integ = vr.MultiScatterGaussians(cam, 4, 5) if multi else vr.FreeFlightGaussians(cam, 4)
    for w0 in (0, 2):
        opts = dict(tree, **({"ff_window0": w0} if w0 else {}))
        a, _ = _fresh_render(scene, integ, 90, 70, ff_kernel=1, **opts)
        b, _ = _fresh_render(scene, integ, 90, 70, ff_kernel=2, **opts)
        assert np.array_equal(a, b, equal_nan=True), f"window0 {w0}: max|d| {np.nanmax(np.abs(a - b)):.2e}"


@pytest.mark.parametrize("multi", [False, True])
def test_phase_scheduled_kernel_equals_bounce_kernel_through_the_fallback(multi):
    """200 coincident Gaussians exceed the 128-entry rows on every path that hits them: both kernels hand
    those paths to ff_fallback_kernel, and the frames are equal bit for bit."""
    scene, _ = _coincident_scene(200)
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    integ = vr.MultiScatterGaussians(cam, 4, 5) if multi else vr.FreeFlightGaussians(cam, 4)
    frames = {}
    for k in (1, 2):
        frames[k], dev = _fresh_render(scene, integ, 16, 16, ff_kernel=k)
        st = dev.stats()
        print(f"kernel {k}: {st}")
        assert st["fallback_pixels"] > 0 and st["error_pixels"] == 0
    assert np.array_equal(frames[1], frames[2], equal_nan=True)


def test_phase_scheduled_kernel_fails_loudly_beyond_every_capacity(device_options):
    # test_overlap_beyond_every_capacity_fails_loudly with the phase-scheduled kernel forced
    scene, _ = _coincident_scene(1100)
    device_options("ff_kernel", 2)
    with pytest.raises(vr.VRError):
        _gpu(scene, 8, 8, True, 1)


@pytest.mark.parametrize("solver", ["bisection", "uniform"])
def test_phase_scheduled_kernel_equals_bounce_kernel_with_other_solvers(solver, device_options):
    """The solvers that read the cached F rows (bisection: od_to / ph) and the path's seed (uniform:
    ff_path_seed) give the same frame under both kernels, bit for bit."""
    scene = vr.Scene.load_GMM(scene_path("250_random.txt"))
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    frames = {}
    try:
        for k in (1, 2):
            device_options("ff_kernel", k)
            img = vr.Image(32, 32)
            vr.MultiScatterGaussians(cam, 4, 5, solver=solver).render(scene, img)
            frames[k] = img.pixels.copy()
    finally:
        vr.Device.get(0).set_option("ff_solver", 0)
    assert np.array_equal(frames[1], frames[2], equal_nan=True), f"max|d| {np.nanmax(np.abs(frames[1] - frames[2])):.2e}"


def test_phase_scheduled_kernel_records_what_the_bounce_kernel_records(device_options):
    """RECORD_PIXEL_GAUSSIANS under both kernels: the same per-pixel Gaussian sets and the same image."""
    scene = vr.Scene.load_GMM(scene_path("50_random.txt"))
    integ = vr.MultiScatterGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), 4)
    bits, imgs = {}, {}
    for k in (1, 2):
        device_options("ff_kernel", k)
        img = vr.Image(32, 32)
        integ.record(scene, img, slot=0)
        bits[k] = integ.pixel_gaussian_bits(0)
        imgs[k] = img.pixels.copy()
    assert bits[1].any()
    assert np.array_equal(bits[1], bits[2])
    assert np.array_equal(imgs[1], imgs[2], equal_nan=True)


@pytest.mark.parametrize("queue", [1, 2])
def test_small_nee_queue_through_tiles_is_reported_then_equal(queue):
    """The asynchronous tile path (vr_render_tiles_device, the multi-GPU building block) with a shadow-ray
    queue forced small: a frame that meets the queue full is never silently returned — vr_synchronize
    reports VR_ERR_RETRY even after vr_get_stats collected the frame first (the r4a red run: the 3-way
    slab test lost such a report to the next call's collect) — and the frame rendered again equals the
    full frame of a default context bit for bit."""
    torch = pytest.importorskip("torch")
    scene = vr.Scene.load_GMM(scene_path("50_random.txt"))
    W, H = 40, 40
    integ = vr.MultiScatterGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), 16, 5)
    full, _ = _fresh_render(scene, integ, W, H)
    dev = vr.Device(0)
    dev.set_option("ff_nee_queue", queue)
    dev.upload(scene)
    nt = vr.num_tiles(W, H)
    img = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    retries = 0
    for attempt in range(4):
        dev.render_tiles_device(integ.camera, integ.params, W, H, 0, 1, nt, False, img.data_ptr(), stream)
        st = dev.stats()  # collects the frame's report before vr_synchronize does
        try:
            dev.synchronize()
        except vr.VRError as e:
            assert e.status == vr._lib.VR_ERR_RETRY and st["record_overflow"]
            retries += 1
            continue
        break
    else:
        pytest.fail("the frame was reported over capacity 4 times")
    print(f"queue {queue}: {retries} re-render(s)")
    if queue == 1:
        assert retries >= 1  # a 1-ray-per-path queue fills (test_deferred_shadow_rays_equal_inline's setting)
    assert np.array_equal(img.cpu().numpy(), full)
    # the context now traces inline: the next frame fits at once and is the same frame
    dev.render_tiles_device(integ.camera, integ.params, W, H, 0, 1, nt, False, img.data_ptr(), stream)
    dev.synchronize()
    assert np.array_equal(img.cpu().numpy(), full)


SOLVERS = {"analytic_newton": 0, "bisection": 1, "newton": 2, "analytic_bisection": 3, "uniform": 4}


@pytest.mark.parametrize("solver", ["bisection", "newton", "analytic_bisection", "uniform"])
@pytest.mark.parametrize("multi", [False, True])
def test_distance_solver_modes_match_oracle(solver, multi):
    """VR_OPT_FF_SOLVER: the reference's compile-time solver choice (distance_solvers.h:143-187) at run
    time. Every mode follows the oracle's restatement of the same solver path by path; the oracle's
    BISECTION / NEWTON / UNIFORM renders are pinned to the reference's own 250_rand_{bisection,newton,
    uniform}_big.ppm (tests/test_oracle_freeflight.py). UNIFORM draws its rand01() from the seeded
    PCG32 stream 2 + bounce of the path on both sides (documented deviation: the reference seeds
    mt19937 from random_device)."""
    L = O.lib()
    L.orc_set_solver.argtypes = [ctypes.c_int]
    path = scene_path("250_random.txt")
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    kw = {"solver": solver}
    integ = vr.MultiScatterGaussians(cam, 4, 5, **kw) if multi else vr.FreeFlightGaussians(cam, 4, **kw)
    img = vr.Image(40, 40)
    try:
        integ.render(vr.Scene.load_GMM(path), img)
    finally:
        vr.Device.get(0).set_option("ff_solver", 0)
    L.orc_set_solver(SOLVERS[solver])
    try:
        r = O.render_ff(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, 40, 40, multi=multi,
                        num_samples=4)
    finally:
        L.orc_set_solver(0)
    _check(img.pixels, r)


def test_solver_modes_change_the_frame():
    """The modes really switch the device solver: UNIFORM (a uniform point of the critical segment)
    renders a different frame than the default ANALYTIC_PLUS_NEWTON on the same paths."""
    path = scene_path("250_random.txt")
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    frames = {}
    try:
        for s in ("analytic_newton", "uniform"):
            img = vr.Image(32, 32)
            vr.MultiScatterGaussians(cam, 4, 5, solver=s).render(vr.Scene.load_GMM(path), img)
            frames[s] = img.pixels.copy()
    finally:
        vr.Device.get(0).set_option("ff_solver", 0)
    assert not np.array_equal(frames["analytic_newton"], frames["uniform"])
