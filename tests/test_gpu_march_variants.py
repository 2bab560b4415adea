"""Every variant of the primary march that a scene can reach (vr_gauss_march.hip): the four passes (tile, one pixel
per wave, one pixel per lane, deep), each on the tree the scene gives it (the 4-wide f16 tree of the default options,
under which the deep pass walks the f16 child-pair tree, or the f32 child-pair tree of VR_OPT_HALF_NODES = 0), the
tile pass's two choices (16 or 32 active-list slots on the 4-wide tree, a 24- or 32-entry stack on the pair tree),
and the tile pass of a ray grid on both trees.

Every case renders on a fresh context with one light, a non-zero environment colour and 2 environment samples,
checks through debug_tree()'s info and the frame's statistics that the variant it names is the one that ran, and
compares the frame's bytes (the product build) and the eight march counts of the same frame (count_work: the
instrumented build) with tests/golden/march_variants.json. A ray grid has no instrumented build (vr_count_work takes
a camera): its cases compare the frame and the per-ray transmittance. The fixture was recorded on an MI355X from the
library of the commit before the march's template parameters became the pass and the tree, in separate processes
that agreed bit for bit in every frame and every count (UNSTABLE is empty), so it pins what each variant computes
and how much work it does.

Scenes: aniso_cases' disc 3 with 150 Gaussians (the tile pass); the chain scene of secondary_chain_cases, whose tree
has the deepest level count the device builder keeps (the 32-entry stack; VR_OPT_DEVICE_BVH = 1, since the host
builder's median splits give the same Gaussians 16 levels); n concentric Gaussians, all active at once on the
central rays (records_compare.nested_gaussians): 24 overflow the tile pass's 16 slots but not 32, 60 overflow both
but not the fallback passes' 64, 80 reach the deep pass."""
import base64
import json
import os
import zlib

import numpy as np
import pytest

import aniso_cases as A
import records_compare as RC
import secondary_chain_cases as SC
import vr_amd as vr
from helpers import CAM_POS, FOV, main_view_dir, render, render_rays

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "march_variants.json")
ENV_SAMPLES = 2
ENV_COLOR = (0.3, 0.5, 0.7)
NESTED_DENSITY = 1e-2
SHALLOW_DEPTH = 25  # kShallowStack + 1 (vr_internal.h): the deepest pair tree that marches with the 24-entry stack
WAVE, LANE = 1 << 31, 0  # march_wide_min: the fallback queue's length from which the lane pass takes it
MAIN = (CAM_POS, main_view_dir(), FOV)
DISC = (*A.RECORD_CAMERA, FOV)
# id -> (scene, camera, frame width, 4-wide tree, march_wide_min or None, what the case proves)
CASES = {
    "tile-wide4-16": ("disc", DISC, 16, True, None, "tile"),
    "tile-pair_f32-stack24": ("disc", DISC, 16, False, None, "tile"),
    "tile-pair_f32-stack32": ("chain", SC.CHAIN_CAMERA, 16, False, None, "tile-tall"),
    "tile-wide4-32": ("nested24", MAIN, 16, True, None, "tile-big"),
    "wave-wide4": ("nested60", MAIN, 16, True, WAVE, "fallback"),
    "wave-pair_f32": ("nested60", MAIN, 16, False, WAVE, "fallback"),
    "lane-wide4": ("nested60", MAIN, 16, True, LANE, "fallback"),
    "lane-pair_f32": ("nested60", MAIN, 16, False, LANE, "fallback"),
    "deep-pair_f16": ("nested80", MAIN, 16, True, None, "deep"),
    "deep-pair_f32": ("nested80", MAIN, 16, False, None, "deep"),
    "rays-wide4": ("disc", DISC, 16, True, None, "rays"),
    "rays-pair_f32": ("disc", DISC, 16, False, None, "rays"),
}
# Counts that differed between recordings of one library would be named here, case -> names, and left out of the
# comparison (at most two of a case's eight). None did: at t_eps = 0 the march's work does not depend on timing.
UNSTABLE = {}


def scene(name):
    if name == "disc":
        arrays, light = A.arrays(A.gaussians("disc", 3)), A.LIGHT
    else:
        a = SC.chain_gaussians(1.2e-5) if name == "chain" else RC.nested_gaussians(int(name[6:]), NESTED_DENSITY)
        arrays, light = a[:4], (a[4][0], a[5][0])
    sc = vr.Scene.from_gaussians(*arrays, lights=[vr.Light(*light)], env_color=ENV_COLOR)
    assert len(sc.lights) == 1
    return sc


def camera_rays(cam, W):
    o, d = np.zeros((W, W, 3), np.float32), np.zeros((W, W, 3), np.float32)
    for y in range(W):
        for x in range(W):
            r = cam.sample_ray(((x + np.float32(0.5)) / np.float32(W), (y + np.float32(0.5)) / np.float32(W)))
            o[y, x], d[y, x] = r.origin, r.direction
    return o, d


def run_case(case):
    """One case on a fresh context: {"frame": (W, W, 3) f32, "tr": (W, W) f32 for a ray grid, "counts": the eight
    march counts (None for a ray grid), "info": debug_tree()'s info, "stats": the compared frame's statistics,
    "first": the statistics of the frame before it (tile-big)}."""
    name, camera, W, wide, wide_min, proves = CASES[case]
    dev = vr.Device(0)
    if not wide:
        dev.set_option("half_nodes", 0)  # (before the upload: the scene gets its f32 child-pair tree alone)
    if name == "chain":  # (the host builder splits at the median: 16 levels; the device builder keeps the chain's own)
        dev.set_option("device_bvh", 1)
    if wide_min is not None:
        dev.set_option("march_wide_min", wide_min)
    dev.upload(scene(name))
    cam = vr.Pinhole_Camera(*camera)
    integ = vr.RayMarchingGaussians(cam, env_samples=ENV_SAMPLES, t_eps=0.0)
    out = {"tr": None, "counts": None, "first": None}
    if proves == "rays":
        out["frame"], out["tr"] = render_rays(dev, integ, *camera_rays(cam, W), unit=True)
        out["stats"] = dev.stats()
    else:
        if proves == "tile-big":  # the frame that switches the context's later frames to 32 slots
            first = render(dev, integ, W, W)
            out["first"] = dev.stats()
        out["frame"] = render(dev, integ, W, W)
        out["stats"] = dev.stats()
        if proves == "tile-big":
            assert first.tobytes() == out["frame"].tobytes()  # (no frame is left out of the comparison)
        work = dev.count_work(cam, integ.params, W, W)
        out["counts"] = {k: work["march"][k] for k in vr.Device.WORK_NAMES["march"]}
    out["info"] = dev.debug_tree([])["info"]
    return out


def encode(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a, "<f4").tobytes(), 9)).decode("ascii")


def decode(text, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), "<f4").reshape(shape)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def same_bytes(case, what, got, ref):
    if got.tobytes() != ref.tobytes():
        d = np.abs(got.astype(np.float64) - ref)
        pytest.fail(f"{case}: {int(np.count_nonzero(d.reshape(len(d), -1).max(-1)))} rows of the {what} differ from the "
                    f"fixture, max {np.nanmax(d):.3e}")


@pytest.mark.parametrize("case", list(CASES))
def test_variant_frame_and_work(case, golden):
    _, _, W, wide, _, proves = CASES[case]
    out = run_case(case)
    frame, info, st, counts = out["frame"], out["info"], out["stats"], out["counts"]
    print(f"{case}: num_nodes4 {info['num_nodes4']}, bvh_depth {info['bvh_depth']}, fallback {st['fallback_pixels']}, "
          f"deep {st['deep_pixels']}, first {out['first'] and out['first']['fallback_pixels']}, march {counts}")
    # the variant the case names is the one that ran: the tree by the scene's 4-wide nodes, the pass by the statistics
    assert (info["num_nodes4"] > 0) if wide else (info["num_nodes4"] == 0)
    assert st["error_pixels"] == 0
    if proves in ("tile", "rays"):
        assert st["fallback_pixels"] == 0
        assert wide or info["bvh_depth"] <= SHALLOW_DEPTH
    elif proves == "tile-tall":
        assert info["bvh_depth"] > SHALLOW_DEPTH and counts["node_tests"] > 0
    elif proves == "tile-big":
        assert out["first"]["fallback_pixels"] * 20 >= W * W and st["fallback_pixels"] == 0
    elif proves == "fallback":
        assert st["fallback_pixels"] > 0 and st["deep_pixels"] == 0
    else:
        assert st["deep_pixels"] > 0
    want = golden[case]
    assert np.isfinite(frame).all() and float(frame.max()) > 0.0
    same_bytes(case, "frame", frame, decode(want["frame"], (W, W, 3)))
    if case.startswith("lane-"):  # the lane pass's frame is the wave pass's
        same_bytes(case, "frame (against the wave pass's)", frame, decode(golden["wave-" + case[5:]]["frame"], (W, W, 3)))
    if proves == "rays":
        same_bytes(case, "transmittance", out["tr"], decode(want["tr"], (W, W)))
        same_bytes(case, "frame (against the camera's)", frame, decode(golden["tile-" + ("wide4-16" if wide else "pair_f32-stack24")]["frame"], (W, W, 3)))
    else:
        assert counts["pixels"] > 0 and counts["primary_queries"] > 0
        for name in UNSTABLE.get(case, ()):
            del counts[name]
        assert counts == want["counts"]
