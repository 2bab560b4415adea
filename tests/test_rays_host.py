"""CPU-only tests of the ray-grid entry points (vr_render_rays, include/vr_hip.h): no GPU calls.

* the Python shape handling of Integrator.render_rays: (H, W, 3) grids pass through, flat (n, 3) batches are laid
  out RAY_BATCH_WIDTH wide with a zero-direction pad, everything else is refused before the library is called;
* the host extent function that sizes a grid's step table (vr_ray_grid_extent) equals a numpy restatement of
  its arithmetic bit for bit on random rays, invalid rays and rays that miss the bounds included;
* the ctypes prototypes of the new entry points load against the built library, and argument errors surface
  as VR_ERR_INVALID / VR_ERR_UNSUPPORTED / VR_ERR_NOSCENE before any device work.
"""
import ctypes

import numpy as np
import pytest

import vr_amd as vr
from vr_amd import _lib as L
from helpers import CAM_POS, FOV, main_view_dir, scene_path


# ---- shape handling ----
def test_grid_shape_passes_through():
    o = np.zeros((5, 7, 3), np.float32)
    assert vr._ray_grid_layout(o, o) == (False, 7, 5, 35, (5, 7))
    rays = vr._pack_ray_grid_numpy(o + 2, o + 3, True, 7, 5, 35)
    assert rays.shape == (35, 8) and rays.dtype == np.float32
    assert np.all(rays[:, 0:3] == 2) and np.all(rays[:, 3] == 0) and np.all(rays[:, 4:7] == 3) and np.all(rays[:, 7] == 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_flat_batch_layout_and_padding(n):
    assert vr.RAY_BATCH_WIDTH == 256
    rng = np.random.default_rng(n)
    o = rng.normal(size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    torch_in, W, H, cnt, lead = vr._ray_grid_layout(o, d)
    assert (torch_in, W, H, cnt, lead) == (False, 256, -(-n // 256), n, (n,))
    rays = vr._pack_ray_grid_numpy(o, d, False, W, H, cnt).reshape(H, W, 8)
    for i in (0, n // 2, n - 1):  # ray i sits at (x, y) = (i % 256, i // 256)
        assert np.array_equal(rays[i // 256, i % 256, 0:3], o[i]) and np.array_equal(rays[i // 256, i % 256, 4:7], d[i])
    flat = rays.reshape(-1, 8)
    assert np.all(flat[:n, 7] == 0)
    assert np.all(flat[n:] == 0)  # the pad: zero direction (an invalid ray: NaN, dropped)


def test_shape_and_type_rejections():
    f = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="float32"):
        vr._ray_grid_layout(f.astype(np.float64), f)
    with pytest.raises(ValueError, match="shape"):
        vr._ray_grid_layout(np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        vr._ray_grid_layout(np.zeros((2, 2, 2, 3), np.float32), np.zeros((2, 2, 2, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        vr._ray_grid_layout(np.zeros(3, np.float32), np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="directions"):
        vr._ray_grid_layout(f, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        vr._ray_grid_layout([[0, 0, 0]], f)
    with pytest.raises(ValueError, match="width and height"):
        vr._ray_grid_layout(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="width and height"):
        vr._ray_grid_layout(np.zeros((1, 65536, 3), np.float32), np.zeros((1, 65536, 3), np.float32))

    # a flat batch of more than 256 * 65535 rays (a broadcast view: nothing that large is allocated)
    most = np.broadcast_to(np.zeros((1, 3), np.float32), (256 * 65535, 3))
    assert vr._ray_grid_layout(most, most)[1:4] == (256, 65535, 256 * 65535)
    huge = np.broadcast_to(np.zeros((1, 3), np.float32), (256 * 65535 + 1, 3))
    with pytest.raises(ValueError, match="at most 16776960"):
        vr._ray_grid_layout(huge, huge)


def test_mixed_numpy_and_torch_is_refused():
    torch = pytest.importorskip("torch")
    f = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="both"):
        vr._ray_grid_layout(f, torch.zeros((4, 3)))


def test_free_flight_classes_refuse_render_rays():
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    f = np.zeros((4, 3), np.float32)
    for integ in (vr.FreeFlightGaussians(cam, 4), vr.MultiScatterGaussians(cam, 4)):
        with pytest.raises(vr.VRError, match="VR_ERR_UNSUPPORTED.*free-flight") as e:
            integ.render_rays(vr.Scene.load_GMM(scene_path("1_gaussian.txt")), f, f)
        assert e.value.status == 7


# ---- the extent that sizes the step table ----
def _extent_numpy(rays, bmin, bmax):
    """vr_ray_grid_extent restated: f32 validity and slab test (a hit iff tmax >= max(tmin, 0), NaNs dropped by
    min / max), the farthest corner's distance from f32 differences squared and summed in double."""
    f = np.float32
    best = f(0)
    for r in rays:
        o, d = r[0:3], r[4:7]
        s = f(d[0] * d[0]) + f(f(d[1] * d[1]) + f(d[2] * d[2]))
        if not (np.all(np.isfinite(o)) and s > 0 and np.isfinite(s)):
            continue
        tmin, tmax = f(-np.inf), f(np.inf)
        for k in range(3):
            inv = f(1) / d[k]
            t1, t2 = f(f(bmin[k] - o[k]) * inv), f(f(bmax[k] - o[k]) * inv)
            tmin, tmax = np.fmax(tmin, np.fmin(t1, t2)), np.fmin(tmax, np.fmax(t1, t2))
        if not (tmax >= np.fmax(tmin, f(0))):
            continue
        e = np.maximum(np.abs(bmin - o), np.abs(bmax - o)).astype(np.float32)
        best = max(best, f(np.sqrt(np.sum(e.astype(np.float64) ** 2))))
    return best


def _extent_lib(rays, bmin, bmax):
    out = ctypes.c_float(-1.0)
    rays = np.ascontiguousarray(rays, np.float32)
    L.check(L.lib().vr_ray_grid_extent(rays.ctypes.data, len(rays), L.fptr(bmin), L.fptr(bmax), ctypes.byref(out)))
    return np.float32(out.value)


def test_extent_equals_numpy_restatement_on_random_rays():
    rng = np.random.default_rng(11)
    bmin, bmax = np.float32([-1.2, -0.1, -1.1]), np.float32([1.3, 2.2, 1.0])
    n = 400
    rays = np.zeros((n, 8), np.float32)
    with np.errstate(all="ignore"):
        rays[:, 0:3] = rng.uniform(-6, 6, (n, 3))
        rays[:, 4:7] = rng.normal(size=(n, 3)) * rng.choice([0.25, 1.0, 7.0], (n, 1))
        rays[::7, 0:3] = rng.uniform(bmin, bmax, (len(rays[::7]), 3))  # origins inside the bounds always hit
        rays[5, 4:7] = 0  # invalid rays are skipped
        rays[6, 0] = np.nan
        rays[8, 5] = np.inf
        rays[9, 4:7] = [0, 0, -1]  # axis-parallel (1 / 0 in the slab test)
        rays[9, 0:3] = [0.1, 1.0, 5.0]
        hits = 0
        for lo in range(0, n, 40):  # subsets, so that rays other than the farthest decide too
            sub = rays[lo:lo + 40]
            ref = _extent_numpy(sub, bmin, bmax)
            got = _extent_lib(sub, bmin, bmax)
            assert got.view(np.uint32) == ref.view(np.uint32), (lo, got, ref)
            hits += ref > 0
        assert hits >= 8
        # a far ray that hits decides the extent; the same origin aimed away is not counted
        far = np.zeros((2, 8), np.float32)
        far[:, 0:3] = [0.0, 1.0, 1.0e7]
        far[0, 4:7] = [0, 0, -1]
        far[1, 4:7] = [0, 0, 1]
        assert _extent_lib(far[:1], bmin, bmax) > 9.9e6
        assert _extent_lib(far[1:], bmin, bmax) == 0
        assert _extent_lib(far[:0], bmin, bmax) == 0


# ---- prototypes and argument errors (no device work) ----
def test_prototypes_load_and_argument_errors():
    lib = L.lib()
    for name in ("vr_render_rays", "vr_render_rays_device", "vr_ray_grid_extent"):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1]
    p = L.vr_render_params()
    p.integrator, p.step_size, p.env_samples = L.VR_RAYMARCH_GAUSSIANS, 0.01, 1
    rays = np.zeros((4, 8), np.float32)
    rgb = np.zeros((4, 3), np.float32)
    # NULL context: VR_ERR_INVALID before anything else
    assert lib.vr_render_rays(None, rays.ctypes.data, 2, 2, ctypes.byref(p), L.fptr(rgb), None) == 1
    assert lib.vr_render_rays_device(None, rays.ctypes.data, 2, 2, ctypes.byref(p), rgb.ctypes.data, None, None) == 1
    out = ctypes.c_float()
    b = np.zeros(3, np.float32)
    assert lib.vr_ray_grid_extent(None, 3, L.fptr(b), L.fptr(b), ctypes.byref(out)) == 1
    assert lib.vr_ray_grid_extent(rays.ctypes.data, 4, L.fptr(b), L.fptr(b), None) == 1
