"""The six variants of the persistent secondary-ray kernel that a scene can reach (vr_gauss_secondary.hip,
secondary_ww_kernel<S, SecForm, SecTree>), each in both builds: the tree (the 4-wide f16 tree of the default options, or
the f32 child-pair tree of VR_OPT_HALF_NODES = 0) crossed with the form (whitened records, M forms, PureRayMarching),
and a seventh case, whitened on the 4-wide tree at t_eps = 1e-3, for the per-record cut-offs (rec_cut).

Every case renders one 32 x 32 frame with one light, a non-zero environment colour and 2 environment samples on a
fresh context, checks through debug_tree()'s info that the variant it names is the one that ran, and compares the
frame's bytes (the product build) and the 16 work counts of the same frame (count_work: the instrumented build)
with tests/golden/secondary_variants.json. The fixture was recorded on an MI355X from the library of the commit
before the kernel's template parameters became the two enums, in six separate processes (the issue asks for two)
that agreed bit for bit in every frame and in every count but the four of UNSTABLE, so it pins what each variant
computes and how much work its schedule does.

Scenes (aniso_cases.py): the whitened and PureRayMarching cases use disc 3 with 150 Gaussians; the M-form cases use
needle 100 at its 512 Gaussians, where the reference's f32 cofactor inverse leaves records without a Cholesky factor
(wrec_pd false)."""
import base64
import json
import os
import zlib

import numpy as np
import pytest

import aniso_cases as A
import vr_amd as vr
from helpers import FOV, render

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secondary_variants.json")
W = 32
ENV_SAMPLES = 2
ENV_COLOR = (0.3, 0.5, 0.7)
SCENES = {"whitened": ("disc", 3), "mform": ("needle", 100), "pure": ("disc", 3)}
# id -> (form, 4-wide tree, t_eps)
CASES = {f"{form}-{'wide4' if wide else 'pair_f32'}": (form, wide, 0.0) for form in SCENES for wide in (True, False)}
CASES["whitened-wide4-t_eps"] = ("whitened", True, 1e-3)
# Counts that differed between recordings of one library and are left out of the fixture (pipeline step
# 3, *Variants*): with a finite cut-off, how many list members and node steps a ray takes before its cut-off is seen
# is not the same from run to run. Over six recordings: node_tests 4581430 .. 4581800, cut_ray_node_steps 173853 ..
# 174223, list_tests 599884 .. 599914, optical_depths 2519725 .. 2519755; the other twelve counts and the frame agreed.
UNSTABLE = {"whitened-wide4-t_eps": ("node_tests", "cut_ray_node_steps", "list_tests", "optical_depths")}


def scene(form):
    sc = vr.Scene.from_gaussians(*A.arrays(A.gaussians(*SCENES[form])), lights=[vr.Light(*A.LIGHT)], env_color=ENV_COLOR)
    assert sc.get_num_primitives() == (512 if form == "mform" else 150) and len(sc.lights) == 1
    return sc


def run_case(case):
    """(frame (32, 32, 3) f32, {stage: {counter: count}} of count_work's 16 counts, debug_tree()'s info) of one case on
    a fresh context."""
    form, wide, t_eps = CASES[case]
    dev = vr.Device(0)
    if not wide:
        dev.set_option("half_nodes", 0)  # (before the upload: the scene gets its f32 child-pair tree alone)
    sc = scene(form)
    dev.upload(sc)
    cam = vr.Pinhole_Camera(*A.RECORD_CAMERA, FOV)
    cls = vr.PureRayMarching if form == "pure" else vr.RayMarchingGaussians
    integ = cls(cam, env_samples=ENV_SAMPLES, t_eps=t_eps)
    frame = render(dev, integ, W, W)
    work = dev.count_work(cam, integ.params, W, W)
    counts = {stage: {k: work[stage][k] for k in vr.Device.WORK_NAMES[stage]} for stage in ("march", "secondary")}
    return frame, counts, dev.debug_tree([])["info"]


def encode(frame):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(frame, "<f4").tobytes(), 9)).decode("ascii")


def decode(text):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), "<f4").reshape(W, W, 3)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_variant_frame_and_work(case, golden):
    form, wide, _ = CASES[case]
    frame, counts, info = run_case(case)
    print(f"{case}: wrec_pd {info['wrec_pd']}, num_nodes4 {info['num_nodes4']}, secondary {counts['secondary']}")
    # the variant the case names is the one that ran: the form by the scene's records (and the integrator), the tree
    # by the scene's 4-wide nodes
    assert info["wrec_pd"] == (form != "mform")
    assert (info["num_nodes4"] > 0) if wide else (info["num_nodes4"] == 0)
    assert counts["secondary"]["secondary_rays"] > 0 and counts["secondary"]["node_tests"] > 0
    want = golden[case]
    ref = decode(want["frame"])
    assert np.isfinite(frame).all() and float(frame.max()) > 0.0
    if frame.tobytes() != ref.tobytes():
        d = np.abs(frame.astype(np.float64) - ref)
        pytest.fail(f"{case}: {int(np.count_nonzero(d.max(-1)))} of {W * W} pixels differ from the fixture, max {d.max():.3e}")
    for name in UNSTABLE.get(case, ()):
        del counts["secondary"][name]
    assert counts == want["counts"]
