"""The environment rays' list filter (VR_OPT_SEC_FILTER, `sec_filter`): the pass that orders a record chunk's
environment rays runs each ray's list phase and keeps the rays that reach their optical-depth cut-off there out of
the persistent kernel. The filter's decision is the persistent kernel's own, so everything a frame computes is the
same with the option on and off, bit for bit: the frame, every secondary ray's Tr, and the per-ray work counts."""
import functools

import numpy as np
import pytest

import vr_amd as vr
from helpers import CAM_POS, FOV, main_view_dir, scene_path

pytestmark = pytest.mark.gpu

BENCH_LIGHTS = [((0.0, 5.0, 0.1), (50.0, 0.0, 0.0)), ((-3.0, 3.0, 0.3), (0.0, 30.0, 0.0)),
                ((3.0, 3.0, -0.2), (0.0, 0.0, 30.0))]  # bench.py LIGHTS


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "blobs" or name == "blobs_dark":  # 20 000 nearly opaque blobs; dark: no lights (environment rays only)
        scene = vr.Scene(vr.Scene.GAUSSIANS)
        scene.add_random_gaussians(20000, seed=7, variant=0)
        if name == "blobs":
            for p, i in BENCH_LIGHTS:
                scene.add_light(vr.Light(p, i))
        return scene
    return vr.Scene.load_GMM(scene_path(name))


def _camera():
    return vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)


def _frame(device_options, name, W, H, env_samples, t_eps, on):
    device_options("sec_filter", on)
    img = vr.Image(W, H)
    integ = vr.RayMarchingGaussians(_camera(), env_samples=env_samples, t_eps=t_eps)
    integ.render(_scene(name), img)
    return img.pixels.copy(), integ.last_stats


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# 70 x 50 is no multiple of the 16 x 16 tile, and a frame's record count is one of the 32-record chunk only by chance;
# frames this small have few chunks per resident wave: the persistent kernel cuts each into 8 claim units (split = 3)
SHAPES = {"1000_random.txt": (70, 50), "10k_random.txt": (64, 64), "blobs": (96, 96)}


@pytest.mark.parametrize("env_samples", [20, 1])
@pytest.mark.parametrize("t_eps", [1e-6, 0.0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_frame_is_bit_identical_with_the_filter_on_and_off(name, t_eps, env_samples, device_options):
    W, H = SHAPES[name]
    on, st_on = _frame(device_options, name, W, H, env_samples, t_eps, 1)
    off, st_off = _frame(device_options, name, W, H, env_samples, t_eps, 0)
    print(f"{name} {W}x{H} t_eps={t_eps} env={env_samples}: records {st_on['scatter_records']} / "
          f"{st_off['scatter_records']}, secondary rays {st_on['secondary_rays']}, filtered {st_on['filtered_rays']}")
    # (no record count compared: a context's first frame of a scene with many fallback pixels leaves their first
    # march's records behind as orphans, later frames march those pixels with the larger active list at once)
    assert st_on["scatter_records"] > 0 and st_off["scatter_records"] > 0
    assert st_off["filtered_rays"] == 0
    assert np.array_equal(_bits(on), _bits(off))


@pytest.mark.parametrize("env_samples", [20, 1])
def test_frame_without_lights_is_bit_identical(env_samples, device_options):
    """No light rays: a chunk whose environment rays are all cut on their lists is an empty claim unit."""
    on, st_on = _frame(device_options, "blobs_dark", 96, 96, env_samples, 1e-6, 1)
    off, st_off = _frame(device_options, "blobs_dark", 96, 96, env_samples, 1e-6, 0)
    print(f"no lights, env={env_samples}: secondary rays {st_on['secondary_rays']}, filtered {st_on['filtered_rays']}")
    assert st_on["filtered_rays"] > 0 and st_off["filtered_rays"] == 0
    assert st_on["secondary_rays"] == st_on["scatter_records"] * env_samples
    assert np.array_equal(_bits(on), _bits(off))


def test_interleaved_tile_shares_are_bit_identical(device_options):
    """Three interleaved shares of the frame's tiles (tile_stride 3, packed slabs), as a 3-GPU split renders them."""
    torch = pytest.importorskip("torch")
    W = H = 96
    cam = _camera()
    integ = vr.RayMarchingGaussians(cam, env_samples=20, t_eps=1e-6)
    dev = vr.Device.get(0)
    _frame(device_options, "blobs", W, H, 20, 1e-6, 1)  # (the whole frame first: it sizes the context's record buffers)
    nt, R = vr.num_tiles(W, H), 3
    per = (nt + R - 1) // R
    stream = torch.cuda.current_stream().cuda_stream
    got = {}
    for on in (1, 0):
        device_options("sec_filter", on)
        slabs = torch.zeros((R, per * 256 * 3), dtype=torch.float32, device="cuda")
        filtered = 0
        for r in range(R):
            dev.render_tiles_device(cam, integ.params, W, H, r, R, len(range(r, nt, R)), True, slabs[r].data_ptr(), stream)
            torch.cuda.synchronize()
            filtered += dev.stats()["filtered_rays"]
        got[on] = (slabs.cpu().numpy(), filtered)
    assert got[1][1] > 0 and got[0][1] == 0
    assert np.array_equal(_bits(got[1][0]), _bits(got[0][0]))


def test_filtered_ray_counts(device_options):
    """The blobs are opaque: an inward environment ray from a record at a blob's fringe is cut by its member."""
    _, on = _frame(device_options, "blobs", 96, 96, 20, 1e-6, 1)
    _, off = _frame(device_options, "blobs", 96, 96, 20, 1e-6, 0)
    print(f"blobs 96x96: secondary rays {on['secondary_rays']}, filtered {on['filtered_rays']}")
    assert off["filtered_rays"] == 0
    assert on["filtered_rays"] > 0
    assert on["filtered_rays"] <= on["secondary_rays"] - on["scatter_records"] * len(BENCH_LIGHTS)


def test_per_ray_rows_are_bit_identical(device_options):
    """Every secondary ray's Tr at four pixels of the blob scene (Device.debug_pixel_records)."""
    pixels = [(48, 48), (40, 55), (57, 42), (30, 62)]
    dev = vr.Device.get(0)
    rows = {}
    for on in (1, 0):
        _frame(device_options, "blobs", 96, 96, 20, 0.0, on)  # (exact mode: every pixel's records to the end)
        rows[on] = [dev.debug_pixel_records(x, y) for x, y in pixels]
    n = sum(len(r) for r in rows[1])
    print(f"{n} records, {n * 23} secondary rays at {pixels}")
    assert n > 0
    for a, b in zip(rows[1], rows[0]):
        assert a.shape == b.shape
        assert np.array_equal(_bits(a), _bits(b))


def test_per_ray_work_counts_are_equal(device_options):
    """The instrumented build: the filter counts the rays it keeps back as secondary rays and cut rays (of no
    node steps), so the per-ray counts are those of a frame that hands every ray out."""
    dev = vr.Device.get(0)
    dev.upload(_scene("blobs"))
    integ = vr.RayMarchingGaussians(_camera(), env_samples=20, t_eps=1e-6)
    work = {}
    for on in (1, 0):
        device_options("sec_filter", on)
        work[on] = dev.count_work(integ.camera, integ.params, 96, 96)["secondary"]
    print(f"filter on: {work[1]}\nfilter off: {work[0]}")
    for key in ("secondary_rays", "cut_rays", "full_ray_node_steps"):
        assert work[1][key] == work[0][key] > 0, key
    assert work[1]["list_tests"] >= work[0]["list_tests"]  # the survivors' list phase runs twice


def test_filter_is_left_out_while_it_filters_too_little(device_options):
    """A frame that filters less than the break-even share of its environment rays (a third) switches the filter
    off for the context's later frames of the scene; setting the option asks again. The translucent 1000_random
    filters a few percent, the opaque blobs nearly half. Frames are the same either way."""
    first, st1 = _frame(device_options, "1000_random.txt", 70, 50, 20, 1e-6, 1)
    env_rays = st1["scatter_records"] * 20
    print(f"1000_random: filtered {st1['filtered_rays']} of {env_rays} environment rays")
    assert 0 < st1["filtered_rays"] * 3 < env_rays
    img = vr.Image(70, 50)
    integ = vr.RayMarchingGaussians(_camera(), env_samples=20, t_eps=1e-6)
    integ.render(_scene("1000_random.txt"), img)  # (the option is not set again)
    assert integ.last_stats["filtered_rays"] == 0
    assert np.array_equal(_bits(img.pixels), _bits(first))
    _, st3 = _frame(device_options, "1000_random.txt", 70, 50, 20, 1e-6, 1)
    assert st3["filtered_rays"] > 0

    _, st1 = _frame(device_options, "blobs", 96, 96, 20, 1e-6, 1)
    assert st1["filtered_rays"] * 3 >= st1["scatter_records"] * 20
    img = vr.Image(96, 96)
    integ.render(_scene("blobs"), img)
    assert integ.last_stats["filtered_rays"] == st1["filtered_rays"]
