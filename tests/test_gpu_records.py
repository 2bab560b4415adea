"""GPU parity at record level: every scatter record and every secondary ray of chosen pixels against the oracle.

test_gpu_parity.py compares whole pixels at L-inf < 1e-4. A pixel is a sum over its scatter records of
Ts S step / 4 pi, and S is a sum over the record's light and environment rays, so that bar dilutes one ray's
error by two sums: on the nested scenes of test_gpu_parity.py (density 1e-4) a secondary stage that met no
Gaussian at all would move the central pixel by 2.6e-5 (n = 60) or 4.0e-5 (n = 80). Here the rows of
vr_debug_pixel_records are matched with the oracle's (tests/records_compare.py): positions and active counts
bit for bit, T sigma_s to 1e-5, every ray's Tr to 1e-4, Li + Le against the row's own Tr and against the oracle's,
and, with the environment at 0, the pixel against its own rows. Every case's rays spread over (0, 1): at least
25 % of them have an oracle Tr in [0.05, 0.95] (tests/test_records_reference.py checks that without a GPU).
"""
import numpy as np
import pytest

import vr_amd as vr
import records_compare as RC
from helpers import CAM_POS, FOV, main_view_dir, scene_path

pytestmark = pytest.mark.gpu

ID_COLUMNS = [0, 1, 2, 3, 8]  # step, position, active count (with T sigma_s, column 4: the march's part of a row)


def _render(scene, W, env_samples, t_eps=0.0):
    img = vr.Image(W, W)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV), step_size=RC.STEP,
                                    env_samples=env_samples, t_eps=t_eps)
    integ.render(scene, img)
    st = dict(integ.last_stats)
    assert st["error_pixels"] == 0
    return img.pixels, st


def _device_rows(pixels):
    dev = vr.Device.get(0)
    return {(int(x), int(y)): dev.debug_pixel_records(int(x), int(y)) for x, y in pixels}


def _fallback_sample(pixels, n=2):
    """Up to n pixels the last frame re-ran on its fallback path, besides `pixels` (the queue's order varies run
    to run: the first and the middle one in (y, x) order)."""
    fb = vr.Device.get(0).fallback_pixels()
    have = {(int(x), int(y)) for x, y in pixels}
    fb = [(int(p[0]), int(p[1])) for p in fb[np.lexsort((fb[:, 0], fb[:, 1]))] if (int(p[0]), int(p[1])) not in have]
    return [fb[i] for i in sorted({0, len(fb) // 2})][:n] if fb else []


def _compare(tag, scene, osc, W, env_samples, dev_rows, budget=False, spread=True):
    """Every pixel of dev_rows against the oracle; asserts the bars and the spread condition, returns the report."""
    lp, li = RC.lights_of(scene)
    orc_rows = RC.oracle_rows_many(osc, list(dev_rows), W, W, env_samples)
    total, msgs = RC.Report(), []
    for p, rows in dev_rows.items():
        rep = RC.compare_rows(rows, orc_rows[p], lp, li, scene.env_color, budget=budget)
        if rep.findings:
            msgs.append(f"pixel {p}: {rep.describe()}")
            f = rep.findings[0]
            if f.k is not None:
                msgs.append(f"  oracle active list at step {f.k}: {RC.record_active(osc, p[0], p[1], W, W, env_samples, f.k)}")
        total.merge(rep)
    what = f"pixel budget sum {total.budget:.3e}, " if budget else ""
    print(f"{tag}: {len(dev_rows)} pixels, {what}{total.summary()}")
    assert not msgs, "\n".join(msgs)
    assert total.one_sided == 0  # (these scenes have no step that exists on one side only)
    assert total.rows > 0
    if spread:
        assert total.spread_share >= RC.MIN_SPREAD_SHARE
    return total


@pytest.mark.parametrize("name", list(RC.FIXTURE_CASES))
def test_fixture_scene_records_match_the_oracle(name):
    f, W, es, pixels = RC.FIXTURE_CASES[name]
    scene = vr.Scene.load_GMM(scene_path(f))
    _, st = _render(scene, W, es)
    rows = _device_rows(pixels + _fallback_sample(pixels))
    rep = _compare(f"{name} {W}x{W} (fallback pixels {st['fallback_pixels']})", scene, RC.oracle_fixture(f), W, es, rows)
    assert sum(len(r) > 0 for r in rows.values()) >= 5 and rep.rows >= 489


@pytest.mark.parametrize("n,density", RC.NESTED_CASES)
def test_nested_scene_records_match_the_oracle(n, density):
    """The nested scenes of test_gpu_parity.py with densities at which the secondary rays matter: the 64-slot
    fallback march (n = 60), the deep march and the re-intersected lists (n >= 80), and the rays' list phase over
    60 to 200 members, each ray held to the bar."""
    arr = RC.nested_gaussians(n, density)
    scene = vr.Scene.from_gaussians(*arr[:4], [vr.Light(arr[4][0], arr[5][0])])
    _, st = _render(scene, 16, 3)
    assert st["fallback_pixels"] > 0
    assert (st["deep_pixels"] > 0) == (n >= 80)
    rep = _compare(f"nested n={n} density={density}", scene, RC.oracle_scene(arr), 16, 3, _device_rows(RC.NESTED_PIXELS))
    assert (rep.rows, rep.rays) == (1181, 4724)


@pytest.mark.parametrize("half_nodes", [1, 0])
def test_slow_path_records_match_the_oracle(half_nodes, device_options):
    """The rays towards a light inside a Gaussian take the exact slow path: secondary_slow_coop_kernel with the
    4-wide half tree, secondary_slow_kernel without it."""
    device_options("half_nodes", half_nodes)
    arr = RC.light_inside_gaussians()
    scene = vr.Scene.from_gaussians(*arr[:4], [vr.Light(p, i) for p, i in zip(arr[4], arr[5])])
    _, st = _render(scene, 48, 8)
    assert st["slow_rays"] > 0
    _compare(f"light inside, half_nodes {half_nodes} (slow rays {st['slow_rays']})", scene, RC.oracle_scene(arr), 48, 8,
             _device_rows(RC.LIGHT_INSIDE_PIXELS))


def test_band_ray_records_match_the_oracle():
    """Environment rays with a chord in the reference's f32 error band go through the band fix-up queue; the
    pixels are those where a float64 model of the band test finds such rays (RC.band_chords)."""
    arr = RC.band_shell_gaussians()
    scene = vr.Scene.from_gaussians(*arr[:4], [vr.Light(arr[4][0], arr[5][0])])
    _, st = _render(scene, 32, 8)
    print(f"band shell: band rays {st['band_rays']}, slow rays {st['slow_rays']}")
    assert st["band_rays"] > 0
    _compare("band shell 32x32", scene, RC.oracle_scene(arr), 32, 8, _device_rows(RC.BAND_PIXELS))


def test_m_form_records_match_the_oracle(tmp_path):
    """A scene with a non-positive-definite record: its secondary rays run the M-form variant."""
    path = RC.write_m_form_scene(tmp_path)
    scene = vr.Scene.load_GMM(path)
    _render(scene, 32, 5)
    _compare("50_random + degenerate 32x32", scene, RC.oracle_fixture(path), 32, 5, _device_rows(RC.six_pixels(32)))


OPTION_VALUES = {"half_nodes": (0, 1), "sec_tight": (0, 1), "start_subtree": (0, 1), "device_bvh": (0, 1),
                 "march_wide_min": (0, 1 << 31), "march_binned": (0, 1)}


@pytest.mark.parametrize("option,values", list(OPTION_VALUES.items()), ids=list(OPTION_VALUES))
def test_tree_and_schedule_options_keep_the_records(option, values, device_options):
    """Both values of every tree and schedule option against the oracle at the same bars; between the two, the
    march's part of every row (step, position, T sigma_s, active count) is bit-equal.

    device_bvh: the march keeps a pixel's active list sorted by scene index (RenderArgs::gauss_order) and sums a
    step's densities in that order, the reference's. While it sorted by the position in the tree's primitive array,
    which the host builder (SAH order) and the device builder (Morton order) permute differently, T sigma_s
    differed between the two trees on 136 of these 857 rows, by at most 5.0e-7 relative."""
    f, W, es, pixels = RC.FIXTURE_CASES["1000_random"]
    osc = RC.oracle_fixture(f)
    got = []
    for v in values:
        device_options(option, v)
        scene = vr.Scene.load_GMM(scene_path(f))  # a new scene: the tree options apply at the next upload
        _render(scene, W, es)
        rows = _device_rows(pixels)
        _compare(f"1000_random {option}={v}", scene, osc, W, es, rows)
        got.append(rows)
    differ, rel = 0, 0.0
    for p in got[0]:
        a, b = got[0][p], got[1][p]
        assert a.shape == b.shape, (option, p)
        assert np.array_equal(a[:, ID_COLUMNS].view(np.uint32), b[:, ID_COLUMNS].view(np.uint32)), (option, p)
        differ += int(np.sum(a[:, 4] != b[:, 4]))
        if len(a):
            rel = max(rel, float(np.max(np.abs(a[:, 4].astype(np.float64) - b[:, 4]) / np.maximum(np.abs(b[:, 4]), RC.TS_TINY))))
    print(f"1000_random {option}: T sigma_s differs between the two values on {differ} rows, max relative {rel:.3e}")
    assert differ == 0, (option, differ, rel)


@pytest.mark.parametrize("name", list(RC.CUTOFF_CASES))
def test_cut_off_stays_within_the_pixel_budget_at_record_level(name):
    """t_eps = 1e-6: a pixel's secondary rays stop at its cut-off, so single rays may miss the oracle's Tr by more
    than 1e-4; what they change of the pixel, sum_rows Ts step / 4 pi sum_rays c_s |dTr| (c_s the ray's channel-max
    weight), stays within the budget of test_secondary_cut_off_stays_within_its_pixel_budget. Rows up to the
    device's last step (the primary early-out drops the tail)."""
    f, W, es, pixels = RC.CUTOFF_CASES[name]
    scene = vr.Scene.load_GMM(scene_path(f))
    _render(scene, W, es, t_eps=1e-6)
    rep = _compare(f"{name} {W}x{W} t_eps=1e-6", scene, RC.oracle_fixture(f), W, es, _device_rows(pixels), budget=True)
    assert rep.budget <= RC.BUDGET


@pytest.mark.parametrize("case", ["many_gaussians", "50_random", "nested60"])
def test_pixel_is_the_sum_of_its_rows_without_environment(case):
    """env_color = 0: the device pixel is the float64 sum of its own rows' Ts S step / 4 pi within the f32
    accumulation bound n_rows 2^-23 sum |terms| (the accumulate kernel at row level); the rows match the oracle's."""
    if case == "nested60":
        arr = RC.nested_gaussians(60, 3e-2)
        scene = vr.Scene.from_gaussians(*arr[:4], [vr.Light(arr[4][0], arr[5][0])], env_color=(0, 0, 0))
        osc, W, es, pixels = RC.oracle_scene(arr, env=(0, 0, 0)), 16, 3, RC.NESTED_PIXELS
    else:
        f, W, es, pixels = RC.FIXTURE_CASES[case]
        scene = vr.Scene.load_GMM(scene_path(f))
        scene.env_color = (0, 0, 0)
        osc = RC.oracle_fixture(f, env=(0, 0, 0))
    img, _ = _render(scene, W, es)
    rows = _device_rows(pixels)
    _compare(f"{case} without environment", scene, osc, W, es, rows)
    for (x, y), r in rows.items():
        s, bound = RC.pixel_from_rows(r)
        err = np.abs(img[y, x].astype(np.float64) - s)
        assert np.all(err <= bound), ((x, y), err.tolist(), bound.tolist())
