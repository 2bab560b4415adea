"""CPU tests of the record-level checker (tests/records_compare.py) and of the oracle side of every case of
tests/test_gpu_records.py: the comparator names each kind of mutation, the oracle's rows have the layout the GPU
test relies on, and the cases' secondary rays really spread over (0, 1) — all known before a GPU is used.
"""
import functools

import numpy as np
import pytest

import pyoracle as O
import vr_amd as vr
import records_compare as RC
from helpers import CAM_POS, FOV, main_view_dir, scene_path


@functools.lru_cache(maxsize=None)
def _mutation_rows():
    """The oracle's rows of the central pixel of 50_random (32 x 32, 5 environment samples) and its lights."""
    rows = RC.oracle_rows(RC.oracle_fixture("50_random.txt"), 16, 16, 32, 32, 5)
    lp, li = RC.lights_of(vr.Scene.load_GMM(scene_path("50_random.txt")))
    rows.setflags(write=False)
    return rows, lp, li


def _cmp(dev, rows, lp, li):
    return RC.compare_rows(dev, rows, lp, li, RC.ENV)


def _row_with_spread(rows, nl):
    """A row whose first light ray and first environment ray both lie inside (0.05, 0.95) and differ."""
    for i, r in enumerate(rows):
        a, b = float(r[9]), float(r[9 + nl])
        if 0.05 < a < 0.95 and 0.05 < b < 0.95 and abs(a - b) > 0.01:
            return i
    raise AssertionError("no such row")


def test_identical_rows_have_no_findings():
    rows, lp, li = _mutation_rows()
    rep = _cmp(rows, rows, lp, li)
    assert len(rows) == 94 and rep.rows == 94 and rep.rays == 94 * 8
    assert rep.findings == [] and rep.max_dtr == 0.0 and rep.max_rel_dts == 0.0


def test_comparator_names_a_shifted_tr():
    rows, lp, li = _mutation_rows()
    i = _row_with_spread(rows, len(lp))
    for ray in (0, len(lp), rows.shape[1] - 10):  # a light ray, the first and the last environment ray
        dev = rows.copy()
        dev[i, 9 + ray] += np.float32(2e-4)
        rep = _cmp(dev, rows, lp, li)
        assert [(f.k, f.ray) for f in rep.named("tr")] == [(int(rows[i, 0]), ray)], rep.describe()
        assert 1.9e-4 < rep.max_dtr < 2.1e-4
        # the row's Li + Le no longer follows from its Tr: 2e-4 of one ray's weight
        assert {f.k for f in rep.named("s_self")} <= {int(rows[i, 0])}


def test_comparator_names_a_tr_set_to_one():
    rows, lp, li = _mutation_rows()
    i = _row_with_spread(rows, len(lp))
    dev = rows.copy()
    dev[i, 9 + len(lp)] = 1.0
    rep = _cmp(dev, rows, lp, li)
    assert [(f.k, f.ray, f.dev) for f in rep.named("tr")] == [(int(rows[i, 0]), len(lp), 1.0)], rep.describe()
    assert rep.named("s_self", k=int(rows[i, 0]))


def test_comparator_names_a_dropped_row():
    rows, lp, li = _mutation_rows()
    dev = np.delete(rows, 7, axis=0)
    rep = _cmp(dev, rows, lp, li)
    assert [(f.kind, f.k) for f in rep.findings] == [("step_only_orc", int(rows[7, 0]))], rep.describe()
    rep = _cmp(rows, dev, lp, li)
    assert [(f.kind, f.k) for f in rep.findings] == [("step_only_dev", int(rows[7, 0]))], rep.describe()


def test_comparator_tolerates_only_underflowing_one_sided_steps():
    """A step on one side only passes if its T sigma_s is below 1e-30 there, and only for 1 % of the rows."""
    _, lp, li = _mutation_rows()
    rows = RC.oracle_rows(RC.oracle_fixture("50_random.txt"), 21, 21, 32, 32, 5)
    assert len(rows) == 122
    extra = rows[-1:].copy()
    extra[0, 0] += 1
    extra[0, 4] = 1e-38
    assert _cmp(np.vstack([rows, extra]), rows, lp, li).findings == []  # 1 of 123 rows
    more = np.repeat(extra, 2, axis=0)
    more[1, 0] += 1
    assert _cmp(np.vstack([rows, more]), rows, lp, li).kinds() == {"tiny_steps"}
    extra[0, 4] = 1e-29
    assert _cmp(np.vstack([rows, extra]), rows, lp, li).kinds() == {"step_only_dev"}


def test_comparator_names_an_active_count_off_by_one():
    rows, lp, li = _mutation_rows()
    dev = rows.copy()
    dev[11, 8] += 1
    rep = _cmp(dev, rows, lp, li)
    assert [(f.kind, f.k, f.dev, f.orc) for f in rep.findings] == [
        ("active", int(rows[11, 0]), int(rows[11, 8]) + 1, int(rows[11, 8]))], rep.describe()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_comparator_names_a_position_off_by_one_ulp(axis):
    rows, lp, li = _mutation_rows()
    dev = rows.copy()
    dev[20, 1 + axis] = np.nextafter(dev[20, 1 + axis], np.float32(np.inf))
    rep = _cmp(dev, rows, lp, li)
    assert [(f.kind, f.k) for f in rep.findings] == [("position", int(rows[20, 0]))], rep.describe()


def test_comparator_names_a_scaled_ts():
    rows, lp, li = _mutation_rows()
    dev = rows.copy()
    dev[30, 4] *= np.float32(1 + 3e-5)
    rep = _cmp(dev, rows, lp, li)
    assert [(f.kind, f.k) for f in rep.findings] == [("ts", int(rows[30, 0]))], rep.describe()
    assert 2.9e-5 < rep.max_rel_dts < 3.1e-5
    dev[30, 4] = rows[30, 4] * np.float32(1 + 5e-6)  # inside the bar
    assert _cmp(dev, rows, lp, li).findings == []


def test_comparator_names_swapped_light_and_environment_columns():
    """Tr columns in another order than lights first, then environment samples: the rays disagree with the
    oracle's, and the row's Li + Le no longer follows from its own Tr."""
    rows, lp, li = _mutation_rows()
    nl = len(lp)
    i = _row_with_spread(rows, nl)
    dev = rows.copy()
    dev[:, [9, 9 + nl]] = dev[:, [9 + nl, 9]]
    rep = _cmp(dev, rows, lp, li)
    k = int(rows[i, 0])
    assert rep.named("tr", k=k, ray=0) and rep.named("tr", k=k, ray=nl) and rep.named("s_self", k=k), rep.describe()
    assert {f.ray for f in rep.named("tr")} == {0, nl}


def test_comparator_refuses_rows_of_another_width():
    rows, lp, li = _mutation_rows()
    assert _cmp(rows[:, :-1], rows, lp, li).kinds() == {"width"}


def test_budget_form_sums_weighted_ray_errors_up_to_the_device_s_last_step():
    rows, lp, li = _mutation_rows()
    dev = rows[:60].copy()  # the primary early-out drops the tail
    rep = RC.compare_rows(dev, rows, lp, li, RC.ENV, budget=True)
    assert rep.findings == [] and rep.rows == 60 and rep.budget == 0.0
    i = int(np.argmax(dev[:, 4]))
    dev[i, 9] += np.float32(1e-3)  # one ray over the per-ray bar: the budget is the assertion here
    rep = RC.compare_rows(dev, rows, lp, li, RC.ENV, budget=True)
    w = RC.ray_weights(rows[i, 1:4], lp, li, RC.ENV, 5)[0].max()
    want = float(rows[i, 4]) * RC.STEP * RC.INV4PI * w * 1e-3
    assert rep.budget == pytest.approx(want, rel=1e-3)
    assert ("budget" in rep.kinds()) == (want > RC.BUDGET)
    assert "tr" not in rep.kinds()


# ---- the oracle side of the GPU cases --------------------------------------------------------------------------
def _oracle_case(osc, lights, W, env_samples, pixels, env=RC.ENV):
    rep = RC.Report()
    with_rows = 0
    for rows in RC.oracle_rows_many(osc, pixels, W, W, env_samples).values():
        with_rows += len(rows) > 0
        rep.merge(RC.compare_rows(rows, rows, lights[0], lights[1], env))
    assert rep.findings == [], rep.describe()  # (Li + Le follows from the oracle's own Tr too)
    return rep, with_rows


@pytest.mark.parametrize("name", ["50_random.txt", "2_gaussian.txt", "many_gaussians.txt"])
def test_oracle_pixel_is_the_sum_of_its_rows(name):
    """With the environment at 0 a pixel is sum_k Ts_k S_k step / 4 pi and nothing else: the oracle's pixel equals
    the float64 sum of its own rows, which pins the row layout (k, position, Ts, Li + Le, active, Tr ...)."""
    osc = RC.oracle_fixture(name, env=(0.0, 0.0, 0.0))
    pix = np.array(RC.six_pixels(32), np.int32)
    with O.stable_ties():
        got = O.render(osc, O.PINHOLE, CAM_POS, main_view_dir(), FOV, 32, 32, O.RAYMARCH_GAUSSIANS_LISTS, RC.STEP, 5,
                       pixels=pix)
    n = 0
    for (x, y), px in zip(pix, got):
        rows = RC.oracle_rows(osc, x, y, 32, 32, 5)
        if len(rows):
            s, _ = RC.pixel_from_rows(rows)
            assert np.abs(s - px).max() < 1e-6, (x, y)
            assert np.all(rows[:, 0] == np.round(rows[:, 0])) and np.all(np.diff(rows[:, 0]) > 0)
            n += 1
        else:
            assert np.all(px == 0.0)
    assert n >= 5


@pytest.mark.parametrize("name", list(RC.FIXTURE_CASES))
def test_fixture_cases_spread(name):
    f, W, es, pixels = RC.FIXTURE_CASES[name]
    rep, with_rows = _oracle_case(RC.oracle_fixture(f), RC.lights_of(vr.Scene.load_GMM(scene_path(f))), W, es, pixels)
    print(f"{name} {W}x{W}: {rep.summary()}")
    assert with_rows >= 5 and 489 <= rep.rows <= 1573
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE


@pytest.mark.parametrize("n,density,lo,share", [(60, 1e-2, 0.46, 0.49), (80, 1e-2, 0.35, 0.53),
                                                (200, 3e-3, 0.46, 0.49), (60, 3e-2, 0.096, 0.67)])
def test_nested_cases_spread(n, density, lo, share):
    arr = RC.nested_gaussians(n, density)
    rep, _ = _oracle_case(RC.oracle_scene(arr), arr[4:], 16, 3, RC.NESTED_PIXELS)
    print(f"nested n={n} density={density}: {rep.summary()}")
    assert (rep.rows, rep.rays) == (1181, 4724)
    assert abs(rep.tr_min - lo) < 0.01 and abs(rep.spread_share - share) < 0.01
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE


def test_light_inside_case_spread():
    arr = RC.light_inside_gaussians()
    osc = RC.oracle_scene(arr)
    rep, with_rows = _oracle_case(osc, arr[4:], 48, 8, RC.LIGHT_INSIDE_PIXELS)
    print(f"light inside 48x48: {rep.summary()}")
    assert with_rows == len(RC.LIGHT_INSIDE_PIXELS)
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE
    # the rays towards the first light (the slow ones) are among the spread ones
    first = np.concatenate([RC.oracle_rows(osc, x, y, 48, 48, 8)[:, 9] for x, y in RC.LIGHT_INSIDE_PIXELS])
    assert np.mean((first >= RC.SPREAD[0]) & (first <= RC.SPREAD[1])) > 0.9


def test_band_case_spread_and_predicted_band_chords():
    arr = RC.band_shell_gaussians()
    osc = RC.oracle_scene(arr)
    rep, with_rows = _oracle_case(osc, arr[4:], 32, 8, RC.BAND_PIXELS)
    print(f"band shell 32x32: {rep.summary()}")
    assert with_rows == len(RC.BAND_PIXELS)
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE
    for x, y in RC.BAND_PIXELS:
        assert len(RC.band_chords(arr, RC.oracle_rows(osc, x, y, 32, 32, 8), x, y, 8)) >= 2, (x, y)


def test_m_form_case_spread(tmp_path):
    path = RC.write_m_form_scene(tmp_path)
    scene = vr.Scene.load_GMM(path)
    rec = scene.records()[-1, 4:10].astype(np.float64)
    M = np.array([[rec[0], rec[1], rec[2]], [rec[1], rec[3], rec[4]], [rec[2], rec[4], rec[5]]])
    assert np.linalg.eigvalsh(M).min() < 0.0
    rep, _ = _oracle_case(RC.oracle_fixture(path), RC.lights_of(scene), 32, 5, RC.six_pixels(32))
    print(f"50_random + degenerate 32x32: {rep.summary()}")
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE


@pytest.mark.parametrize("name", list(RC.CUTOFF_CASES))
def test_cut_off_cases_spread(name):
    f, W, es, pixels = RC.CUTOFF_CASES[name]
    rep, with_rows = _oracle_case(RC.oracle_fixture(f), RC.lights_of(vr.Scene.load_GMM(scene_path(f))), W, es, pixels)
    print(f"{name} {W}x{W}: {rep.summary()}")
    assert with_rows >= 5
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE


def test_record_active_binding_lists_the_active_ids():
    osc = RC.oracle_fixture("2_gaussian.txt")
    rows = RC.oracle_rows(osc, 16, 16, 32, 32, 5)
    k = int(rows[len(rows) // 2, 0])
    act = RC.record_active(osc, 16, 16, 32, 32, 5, k)
    assert act is not None and len(act) == int(rows[len(rows) // 2, 8]) and set(act) <= {0, 1}
    assert RC.record_active(osc, 16, 16, 32, 32, 5, 1 << 20) is None
