"""Ray grids on the GPU (vr_render_rays / Integrator.render_rays): a W x H image of the caller's own rays is rendered
by the ray-march integrators exactly as a frame is. The yardstick needs no oracle: a grid filled with a camera's
own rays (Camera.sample_ray at ((x + 0.5f) / W, (y + 0.5f) / H) in f32, which
test_host_abi.py::test_camera_and_primary_rays_bit_identical proves equal to the device's rays; passed with
unit = 1) must reproduce that camera's frame bit for bit, statistics included. Equality below is always
np.array_equal on the uint32 views.
"""
import ctypes

import numpy as np
import pytest

import vr_amd as vr
from vr_amd import _lib as L
from helpers import CAM_POS, FOV, main_view_dir, scene_path

pytestmark = pytest.mark.gpu

F = np.float32


def beq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def camera_rays(cam, W, H):
    """(origins, directions), each (H, W, 3): the camera's own primary rays."""
    o = np.zeros((H, W, 3), np.float32)
    d = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            r = cam.sample_ray(((x + F(0.5)) / F(W), (y + F(0.5)) / F(H)))
            o[y, x], d[y, x] = r.origin, r.direction
    return o, d


def pinhole():
    return vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)


def ortho():
    return vr.Orthographic_Camera(CAM_POS, main_view_dir())


_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = vr.Scene.load_SMM(scene_path(name)) if name.startswith("sph_") else vr.Scene.load_GMM(scene_path(name))
    return _scenes[name]


def frame(integ, sc, W, H):
    img = vr.Image(W, H)
    integ.render(sc, img)
    return img.pixels.copy(), integ.last_stats


# The cases of test 1: name -> (integrator factory, camera factory, scene, W, H). The frame and the camera's rays
# of each are computed once and shared by the tests below.
CASES = {
    "rmg": (lambda c: vr.RayMarchingGaussians(c, env_samples=4, t_eps=0.0), pinhole, "250_random.txt", 40, 24),
    "rmg_eps": (lambda c: vr.RayMarchingGaussians(c, env_samples=4, t_eps=1e-6), pinhole, "250_random.txt", 40, 24),
    "rmg_ortho": (lambda c: vr.RayMarchingGaussians(c, env_samples=4, t_eps=0.0), ortho, "250_random.txt", 40, 24),
    "rmg_ortho_eps": (lambda c: vr.RayMarchingGaussians(c, env_samples=4, t_eps=1e-6), ortho, "250_random.txt", 40, 24),
    "pure": (lambda c: vr.PureRayMarching(c, env_samples=4, t_eps=0.0), pinhole, "many_gaussians.txt", 24, 24),
    "pure_eps": (lambda c: vr.PureRayMarching(c, env_samples=4, t_eps=1e-6), pinhole, "many_gaussians.txt", 24, 24),
    "pure_ortho": (lambda c: vr.PureRayMarching(c, env_samples=4, t_eps=0.0), ortho, "many_gaussians.txt", 24, 24),
    "spheres": (lambda c: vr.RayMarchingSpheres(c, env_samples=4), pinhole, "sph_3_spheres.txt", 40, 24),
    "spheres_ortho": (lambda c: vr.RayMarchingSpheres(c, env_samples=4), ortho, "sph_3_spheres.txt", 40, 24),
    "hitmask_spheres": (lambda c: vr.TestIntegrator(c), pinhole, "sph_3_spheres.txt", 40, 24),
    "hitmask_spheres_ortho": (lambda c: vr.TestIntegrator(c), ortho, "sph_3_spheres.txt", 40, 24),
    "hitmask_gaussians": (lambda c: vr.TestIntegrator(c), pinhole, "250_random.txt", 40, 24),
}
_refs = {}


def case(name):
    """(integrator, scene, origins, directions, frame pixels, frame stats) of a CASES entry."""
    if name not in _refs:
        make, cam, sc, W, H = CASES[name]
        c = cam()
        integ = make(c)
        o, d = camera_rays(c, W, H)
        px, st = frame(integ, scene(sc), W, H)
        _refs[name] = (integ, scene(sc), o, d, px, st)
    return _refs[name]


# ---- 1. a camera's grid is its frame ----
@pytest.mark.parametrize("name", list(CASES))
def test_camera_grid_is_the_frame(name):
    integ, sc, o, d, px, st = case(name)
    rgb = integ.render_rays(sc, o, d, unit=True)
    gs = integ.last_stats
    assert rgb.shape == px.shape and rgb.dtype == np.float32
    assert beq(rgb, px), int(np.sum(rgb.view(np.uint32) != px.view(np.uint32)))
    assert gs["scatter_records"] == st["scatter_records"] and gs["secondary_rays"] == st["secondary_rays"]
    assert gs["error_pixels"] == 0 and gs["pixels"] == st["pixels"]
    if name.startswith("rmg") or name.startswith("pure"):
        assert gs["scatter_records"] > 0 and gs["secondary_rays"] > 0


# ---- 2. rays are read per pixel ----
def test_rays_are_read_per_pixel():
    W = H = 32
    sc = scene("250_random.txt")
    cp, co = pinhole(), ortho()
    ip, io = vr.RayMarchingGaussians(cp, env_samples=3), vr.RayMarchingGaussians(co, env_samples=3)
    fp, _ = frame(ip, sc, W, H)
    fo, _ = frame(io, sc, W, H)
    (op, dp), (oo, do) = camera_rays(cp, W, H), camera_rays(co, W, H)
    o, d = op.copy(), dp.copy()
    o[1::2], d[1::2] = oo[1::2], do[1::2]
    rgb = ip.render_rays(sc, o, d, unit=True)
    assert not beq(fp, fo)
    for y in range(H):
        assert beq(rgb[y], (fp if y % 2 == 0 else fo)[y]), y


# ---- 3. arbitrary rays, origins inside the cloud ----
def test_arbitrary_rays_with_origins_inside_the_cloud():
    sc = scene("50_random.txt")
    info = sc.info()
    lo, hi = np.float32(list(info.bounds_min)), np.float32(list(info.bounds_max))
    rng = np.random.default_rng(7)
    origins = rng.uniform(lo, hi, (16, 3)).astype(np.float32)
    dirs = rng.normal(size=(16, 3)).astype(np.float32)
    lit = 0
    for o, d in zip(origins, dirs):
        cam = vr.Orthographic_Camera(o, d)  # its 1 x 1 frame marches exactly the ray (o, forward) at pixel (0, 0)
        integ = vr.RayMarchingGaussians(cam, env_samples=3)
        px, st = frame(integ, sc, 1, 1)
        r = cam.sample_ray((0.5, 0.5))
        assert np.array_equal(r.origin, o)
        rgb = integ.render_rays(sc, r.origin.reshape(1, 1, 3), r.direction.reshape(1, 1, 3), unit=True)
        assert beq(rgb, px), (o, d, rgb, px)
        assert integ.last_stats["scatter_records"] == st["scatter_records"]
        lit += st["scatter_records"] > 0
    assert lit >= 4  # (most of these rays cross Gaussians)


# ---- 4. the fallback passes ----
def _dense_overlap_scene():
    n = 40
    rng = np.random.default_rng(7)
    mean = (np.array([0.0, 1.0, 0.0]) + rng.normal(scale=0.02, size=(n, 3))).astype(np.float32)
    sig = rng.uniform(0.2, 0.35, n)
    cov = np.stack([sig ** 2, 0 * sig, 0 * sig, sig ** 2, 0 * sig, sig ** 2], 1).astype(np.float32)
    dens = np.full(n, 0.002, np.float32)
    alb = rng.uniform(0.2, 0.9, n).astype(np.float32)
    return vr.Scene.from_gaussians(mean, cov, dens, alb, [vr.Light([0.0, 5.0, 0.1], [50, 50, 50])])


def _nested_scene(n, density=1e-4):
    mean = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (n, 1))
    sig = np.linspace(0.3, 0.4, n)
    cov = np.stack([sig ** 2, 0 * sig, 0 * sig, sig ** 2, 0 * sig, sig ** 2], 1).astype(np.float32)
    dens = np.full(n, density, np.float32)
    alb = np.full(n, 0.5, np.float32)
    return vr.Scene.from_gaussians(mean, cov, dens, alb, [vr.Light([0.0, 5.0, 0.0], [1.0, 1.0, 1.0])])


@pytest.mark.parametrize("which", ["fallback", "deep"])
def test_fallback_passes(which):
    if which == "fallback":
        sc, W, H, env = _dense_overlap_scene(), 32, 32, 2
    else:
        sc, W, H, env = _nested_scene(80), 16, 16, 1
    cam = pinhole()
    integ = vr.RayMarchingGaussians(cam, env_samples=env)
    px, _ = frame(integ, sc, W, H)
    # After a frame with many fallback pixels the context's primary march takes more active-list slots, so fewer
    # pixels overflow it (and leave fewer orphaned records behind): the counts are compared with a second frame's,
    # which marches as the grid does. The pixels do not depend on the pass.
    px2, st = frame(integ, sc, W, H)
    o, d = camera_rays(cam, W, H)
    rgb = integ.render_rays(sc, o, d, unit=True)
    gs = integ.last_stats
    assert beq(rgb, px) and beq(px2, px)
    assert gs["error_pixels"] == 0 and gs["fallback_pixels"] > 0
    if which == "deep":
        assert gs["deep_pixels"] > 0
    for k in ("fallback_pixels", "deep_pixels", "scatter_records", "secondary_rays"):
        assert gs[k] == st[k], k


# ---- 5. transmittance ----
@pytest.mark.parametrize("name", ["rmg", "rmg_eps", "pure", "spheres", "hitmask_spheres", "hitmask_gaussians"])
def test_transmittance_leaves_rgb_unchanged_and_is_bounded(name):
    integ, sc, o, d, px, st = case(name)
    rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    assert beq(rgb, px)  # (a)
    assert tr.shape == px.shape[:2] and tr.dtype == np.float32
    assert np.all((tr >= 0) & (tr <= 1))  # (d)
    if name.startswith("hitmask"):  # 1 where the ray hits nothing (the environment colour shows), 0 where it hits
        env = sc.env_color
        miss = np.all(px.view(np.uint32) == env.view(np.uint32), axis=-1)
        assert np.array_equal(tr, miss.astype(np.float32)) and 0 < miss.sum() < miss.size


def test_transmittance_of_a_purely_absorbing_cloud_is_the_image():
    g = scene("250_random.txt").gaussians()
    sc = vr.Scene.from_gaussians(g[:, 0:3], g[:, 3:9], g[:, 9], np.zeros(len(g), np.float32), env_color=[1.0, 1.0, 1.0])
    cam = pinhole()
    o, d = camera_rays(cam, 40, 24)
    integ = vr.RayMarchingGaussians(cam, env_samples=4)
    rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    assert integ.last_stats["scatter_records"] == 0  # no sigma_s: no records
    for c in range(3):
        assert beq(rgb[..., c], tr)  # (b)
    assert np.any(tr < 1) and np.any(tr == 1)


def test_rays_without_events_get_the_environment_exactly():
    integ, sc, o, d, px, st = case("rmg")
    rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    env = sc.env_color
    off, _, _, _ = vr.Device.get(0).query_events(sc, o.reshape(-1, 3), d.reshape(-1, 3))
    no_events = (np.diff(off) == 0).reshape(px.shape[:2])
    is_env = np.all(px.view(np.uint32) == env.view(np.uint32), axis=-1)
    clear = no_events & is_env
    assert clear.sum() > 0 and (~clear).sum() > 0  # (the cloud fills most of this frame: a few corner rays are clear)
    assert np.all(tr[clear] == 1.0)  # (c)
    assert np.all(rgb[clear].view(np.uint32) == env.view(np.uint32))
    assert np.all((tr[~clear] >= 0) & (tr[~clear] <= 1))  # (d)


# ---- 6. invalid rays ----
@pytest.mark.parametrize("name", ["rmg", "spheres", "hitmask_gaussians"])
def test_invalid_rays_give_nan_and_nothing_else_changes(name):
    integ, sc, o, d, px, st = case(name)
    o, d = o.copy(), d.copy()
    bad = [(3, 5), (17, 20), (23, 39)]  # (y, x)
    o[bad[0]] = [np.nan, 0, 0]
    d[bad[1]] = 0
    d[bad[2]] = [np.inf, 0, 0]
    with np.errstate(all="ignore"):
        rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    assert integ.last_stats["error_pixels"] == 0
    ok = np.ones(px.shape[:2], bool)
    for b in bad:
        ok[b] = False
        assert np.all(np.isnan(rgb[b])) and np.isnan(tr[b])
    assert beq(rgb[ok], px[ok])
    assert not np.any(np.isnan(tr[ok]))


# ---- 7. unit ----
def test_unit_flag():
    integ, sc, o, d, px, st = case("rmg")
    d_un = (d * F(0.37)).astype(np.float32)  # un-normalised
    a = integ.render_rays(sc, o, d_un, unit=False)
    b = integ.render_rays(sc, o, (d_un * F(4.0)).astype(np.float32), unit=False)  # a power of two: the same bits after normalising
    assert beq(a, b)
    # (not the frame bit for bit: normalising the camera's direction once more moves it by an ulp, which can move a
    # Gaussian's entry across a step; no bound on that is asserted)
    assert not np.any(np.isnan(a)) and np.all(np.isfinite(a))
    assert beq(integ.render_rays(sc, o, d, unit=True), px)  # normalised already and used as they stand: test 1


# ---- 8. entry points agree ----
def test_numpy_and_torch_inputs_agree():
    import torch
    for name in ("rmg", "spheres"):
        integ, sc, o, d, px, st = case(name)
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        rgb, tr = integ.render_rays(sc, to, td, unit=True, return_transmittance=True)
        assert isinstance(rgb, torch.Tensor) and rgb.is_cuda and tuple(rgb.shape) == px.shape and tuple(tr.shape) == px.shape[:2]
        nrgb, ntr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
        assert beq(rgb.cpu().numpy(), px) and beq(nrgb, px) and beq(tr.cpu().numpy(), ntr)
        # un-normalised directions, normalised on the device
        d_un = (d * F(0.37)).astype(np.float32)
        assert beq(integ.render_rays(sc, to, torch.from_numpy(d_un).cuda()).cpu().numpy(), integ.render_rays(sc, o, d_un))


def test_flat_batch_is_the_padded_grid():
    import torch
    integ, sc, _, _, _, _ = case("rmg")
    o, d = camera_rays(pinhole(), 40, 25)
    o, d = o.reshape(1000, 3), d.reshape(1000, 3)
    go, gd = np.zeros((4, 256, 3), np.float32), np.zeros((4, 256, 3), np.float32)
    go.reshape(-1, 3)[:1000], gd.reshape(-1, 3)[:1000] = o, d  # the pad: zero directions
    with np.errstate(all="ignore"):
        grgb, gtr = integ.render_rays(sc, go, gd, unit=True, return_transmittance=True)
    assert np.all(np.isnan(grgb.reshape(-1, 3)[1000:])) and np.all(np.isnan(gtr.reshape(-1)[1000:]))
    rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    assert rgb.shape == (1000, 3) and tr.shape == (1000,)
    assert beq(rgb, grgb.reshape(-1, 3)[:1000]) and beq(tr, gtr.reshape(-1)[:1000])
    assert not np.any(np.isnan(rgb)) and len(np.unique(rgb, axis=0)) > 10
    trgb = integ.render_rays(sc, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), unit=True)
    assert tuple(trgb.shape) == (1000, 3) and beq(trgb.cpu().numpy(), rgb)


# ---- 9. limits and options ----
def _raw(dev, rays, W, H, params, rgb, tr=None):
    return L.lib().vr_render_rays(dev._h, rays.ctypes.data if rays is not None else None, W, H, ctypes.byref(params),
                                  L.fptr(rgb), L.fptr(tr) if tr is not None else None)


def test_far_origins_and_argument_errors():
    import torch
    integ, sc, o, d, px, st = case("rmg")
    dev = vr.Device.get(0)
    dev.upload(sc)
    W, H = 40, 24
    far_o, far_d = o.copy(), d.copy()
    far_o[2, 3] = [0.0, 1.0, 1.0e7]  # 10^7 away, aimed at the scene: a table of 10^9 steps
    far_d[2, 3] = [0.0, 0.0, -1.0]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(vr.VRError) as e:
        integ.render_rays(sc, far_o, far_d, unit=True)
    assert e.value.status == L.VR_ERR_OVERFLOW
    with pytest.raises(vr.VRError) as e:
        integ.render_rays(sc, torch.from_numpy(far_o).cuda(), torch.from_numpy(far_d).cuda(), unit=True)
    assert e.value.status == L.VR_ERR_OVERFLOW
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 30)  # (that table would take 4 GB)
    assert beq(integ.render_rays(sc, o, d, unit=True), px)  # the context is as it was
    # the same far origin aimed away from the bounds does not count: it sees the environment
    far_d[2, 3] = [0.0, 0.0, 1.0]
    rgb, tr = integ.render_rays(sc, far_o, far_d, unit=True, return_transmittance=True)
    ok = np.ones((H, W), bool)
    ok[2, 3] = False
    assert beq(rgb[ok], px[ok]) and tr[2, 3] == 1.0 and beq(rgb[2, 3], sc.env_color)
    assert integ.last_stats["error_pixels"] == 0
    # argument errors
    rays = vr._pack_ray_grid_numpy(o, d, True, W, H, W * H)
    out = np.zeros((H, W, 3), np.float32)
    assert _raw(dev, rays, 0, H, integ.params, out) == L.VR_ERR_INVALID
    assert _raw(dev, rays, 65536, 1, integ.params, out) == L.VR_ERR_INVALID
    assert _raw(dev, rays, W, 0, integ.params, out) == L.VR_ERR_INVALID
    assert _raw(dev, None, W, H, integ.params, out) == L.VR_ERR_INVALID
    t = torch.zeros(W * H * 8 + 1, dtype=torch.float32, device="cuda")
    trgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    assert L.lib().vr_render_rays_device(dev._h, t.data_ptr() + 4, W, H, ctypes.byref(integ.params), trgb.data_ptr(), None,
                                         None) == L.VR_ERR_INVALID  # not 16-byte aligned
    assert L.lib().vr_render_rays_device(dev._h, None, W, H, ctypes.byref(integ.params), trgb.data_ptr(), None,
                                         None) == L.VR_ERR_INVALID
    for ff in (vr.FreeFlightGaussians(pinhole(), 4), vr.MultiScatterGaussians(pinhole(), 4)):
        assert _raw(dev, rays, W, H, ff.params, out) == L.VR_ERR_UNSUPPORTED
    sph = vr.RayMarchingSpheres(pinhole())
    assert _raw(dev, rays, W, H, sph.params, out) == L.VR_ERR_INVALID  # a frame's own check: needs a sphere scene
    assert beq(integ.render_rays(sc, o, d, unit=True), px)


def test_options_do_not_change_a_grid(device_options):
    integ, sc, o, d, px, st = case("rmg")
    device_options("march_binned", 1)  # ignored by grids; the binned frame equals the unbinned one anyway
    assert beq(integ.render_rays(sc, o, d, unit=True), px)
    device_options("march_binned", 0)
    device_options("half_nodes", 0)
    f0, s0 = frame(integ, sc, 40, 24)
    # (pixels only: scatter_records also counts the records a pixel wrote before it overflowed a pass, and after a
    # frame with many fallback pixels the context's primary march takes more slots; see test_fallback_passes)
    assert beq(integ.render_rays(sc, o, d, unit=True), f0)
    device_options("half_nodes", 1)
    device_options("device_bvh", 1)  # (the device builder takes scenes of at least 256 Gaussians)
    big = scene("1000_random.txt")
    f1, s1 = frame(integ, big, 40, 24)
    assert beq(integ.render_rays(big, o, d, unit=True), f1)
    assert vr.Device.get(0).debug_tree(arrays=())["info"]["built_on_device"]


def test_multi_gpu_rehearsal_context_renders_the_grid():
    _, sc, o, d, px, st = case("rmg")
    integ = vr.RayMarchingGaussians(pinhole(), env_samples=4, device=(0, 0))  # the same GPU listed twice
    rgb, tr = integ.render_rays(sc, o, d, unit=True, return_transmittance=True)
    assert beq(rgb, px) and np.all((tr >= 0) & (tr <= 1))


# ---- 10. a frame after a grid, and a grid after a frame ----
def test_frames_and_grids_alternate_on_one_context():
    integ, sc, o, d, px, st = case("rmg")
    dense = _dense_overlap_scene()
    cam = pinhole()
    i2 = vr.RayMarchingGaussians(cam, env_samples=2)
    o2, d2 = camera_rays(cam, 32, 32)
    first = None
    for _ in range(2):
        a = integ.render_rays(sc, o, d, unit=True)  # a grid after a frame (of another size, scene and record count)
        b, _ = frame(integ, sc, 40, 24)
        c = i2.render_rays(dense, o2, d2, unit=True)
        e, _ = frame(i2, dense, 32, 32)
        assert beq(a, px) and beq(b, px) and beq(c, e)
        if first is None:
            first = (a, c)
        assert beq(a, first[0]) and beq(c, first[1])
