"""Preconditions of the context-history tests (history_cases.py, test_gpu_history.py), checked with the oracle and
numpy alone: the probe inputs show something of every scene, they tell consecutive scenes apart, and each scene has
the piece of state it was chosen for. Without them a history could pass emptily: a batch whose rays all miss gives
Tr = 1 on every context, and a stale answer from the previous scene could pass where the two scenes agree."""
import numpy as np
import pytest

import history_cases as H


def transmittance(name, cur, prev):
    return np.exp(-H.oracle_tau(name, cur, prev))


@pytest.mark.parametrize("cur,prev", H.PAIRS, ids=[f"{c}-after-{p}" for c, p in H.PAIRS])
def test_batches_show_the_scene_and_tell_it_from_the_previous_one(cur, prev):
    """test_gpu_query.py's rule: at the finite tmax the oracle's Tr lies in (0.01, 0.99) on a quarter of the rays at
    least. And the previous scene's Tr along the same rays differs from this one's by more than 1e-3 on a quarter of
    them, so the previous scene's answer cannot pass for this one's. (The empty scene's Tr is 1.)"""
    inp = H.inputs(cur, prev)
    assert inp.o.shape == inp.d.shape == (H.N_RAYS, 3) and inp.tmax.shape == (H.N_RAYS,) and inp.t.shape == (H.N_RAYS, H.K_PROFILE)
    assert np.all(np.isfinite(inp.tmax)) and np.all(inp.tmax > 0)
    tr = transmittance(cur, cur, prev)
    if H.num_gaussians(cur) > 0:
        mid = float(np.mean((tr > 0.01) & (tr < 0.99)))
        print(f"{cur} after {prev}: {100 * mid:.0f} % of the oracle's Tr in (0.01, 0.99)")
        assert mid >= 0.25
    if prev is not None:
        apart = float(np.mean(np.abs(tr - transmittance(prev, cur, prev)) > 1e-3))
        print(f"{cur} after {prev}: Tr differs from the previous scene's on {100 * apart:.0f} % of the rays")
        assert apart >= 0.25


@pytest.mark.parametrize("name", [s for s in H.GAUSSIAN_SCENES if s != "G"])
def test_sigma_points_lie_in_the_mixture(name):
    import sigma_grad_reference as SR
    p = H.sigma_points(name)
    assert p.shape == (H.N_RAYS, 3) and np.isfinite(p).all()
    rec = SR.records_of_oracle(H.oracle_scene(name).records())
    positive = float(np.mean(SR.sigma(rec, p).sum(1) > 0))
    print(f"{name}: sigma > 0 at {100 * positive:.0f} % of the points")
    assert positive >= 0.25


def test_every_batch_of_the_histories_has_a_rule():
    """PAIRS is derived from SEQUENCES, the check steps that test_gpu_history.py's generators walk."""
    assert len(H.PAIRS) == 15 and ("A", "B") in H.PAIRS and ("B", None) in H.PAIRS
    for cur, prev in H.PAIRS:
        assert cur in H.TMAX_RULE and (prev is None or prev in H.GAUSSIAN_SCENES)


def test_a_queue_of_one_ray_per_path_must_fill():
    """History 5's ff_nee_queue = 1 step: a MultiScatter path queues one shadow ray per bounce and is not ended by
    Russian roulette before min_bounces + 1 bounces, so a path that scatters twice needs two slots of a queue that has
    one per path (test_gpu_history.py then reads the inline and queued ray counts from the instrumented render)."""
    import vr_amd as vr
    assert vr.MultiScatterGaussians(H.camera(), 4).params.min_bounces + 1 > 1


def test_scenes_have_the_state_they_were_chosen_for():
    """Median chord depth (scene_median_chord_depth of vr_upload.cpp, restated): A and C fall on opposite sides of 16
    (auto_ff_sm: the phase-scheduled kernel below it) and of 50 (auto_nee_refill: 56 from there on), and
    scene_window0's `w * median < 64` doubling gives 16 for A and 4 for C. D holds records that are not positive
    definite. E's median box is below the half-node rule's 3 % of the scene's half extent, A's above it."""
    import aniso_cases
    med_a, med_c = (H.median_chord_depth(H.scene(s).records()) for s in ("A", "C"))
    print(f"median chord depth: A {med_a:.3f}, C {med_c:.1f}")
    assert 0 < med_a < 16 and med_c >= 50
    assert H.num_gaussians("A") >= 256  # auto_ff_sm's other condition

    def window0(med):  # scene_window0 for a mean overlap under 8
        w = 4
        while w < 32 and w * med < 64.0:
            w *= 2
        return w
    assert window0(med_a) == 16 and window0(med_c) == 4
    _, not_pd, not_finite = aniso_cases.record_health(H.scene("D").records())
    print(f"D: {int(not_pd.sum())} of {len(not_pd)} records are not positive definite")
    assert not_pd.sum() >= 1 and not not_finite.any()
    assert not aniso_cases.record_health(H.scene("A").records())[1].any()
    med, bar = H.half_node_rule("E")
    assert med < bar
    med, bar = H.half_node_rule("A")
    assert med >= bar
    assert H.num_gaussians("B") < 256 <= H.num_gaussians("R")  # B takes the host builder, R the device builder
    assert H.num_gaussians("G") == 0
    lights = {s: len(H.scene(s).lights) for s in ("S2", "B", "S3", "Aenv", "C")}
    print(f"lights: {lights}")
    assert lights["S2"] == 2 and lights["C"] == 0 and len(set(lights.values())) >= 3
    assert not np.array_equal(H.scene("A").env_color, H.scene("Aenv").env_color)


def test_the_gradient_bounds_are_the_modules_own():
    import grad_reference as R
    import sigma_grad_reference as SR
    assert R.BOUND == SR.BOUND == 2.0 ** -21
    assert set(H.PROBES) >= set(H.FRAME_PROBES + H.SPHERE_PROBES + H.QUERY_PROBES + H.GRADIENT_PROBES + H.GROUP_PROBES + H.BATCH_FREE)
