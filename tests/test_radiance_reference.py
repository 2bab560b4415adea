"""The float64 model of the radiance query (tests/radiance_reference.py), on the CPU: the exclusion's cap on every case the
GPU tests hold against the model, the model against a literal per-sample loop, and what its pieces are made of."""
import numpy as np
import pytest

import grad_reference as GR
import radiance_reference as RR


@pytest.mark.parametrize("case", RR.CASES, ids=[f"{c[0]}-K{c[2]}-C{c[3]}" for c in RR.CASES])
def test_the_exclusion_zeroes_at_most_one_percent(case):
    mdl = RR.model(*case)  # (the constructor asserts the cap)
    print(f"{case}: {int(mdl.near.sum())} of {int(mdl.valid.sum())} samples zeroed ({mdl.zeroed:.3%}), {int(mdl.pairs.sum())} pairs, "
          f"rows with S > 0: {int((mdl.S > 0).any(1).sum())}")
    assert mdl.zeroed <= RR.CAP == 0.01
    assert np.array_equal(mdl.weights == 0, mdl.near | (RR.case_samples(*case[:3])[1] == 0))
    assert mdl.pairs.sum() > 0 and (mdl.S > 0).any()
    if case[3] > 1:  # a channel of ones is the opacity
        assert np.allclose(mdl.L[:, 1], mdl.opacity, rtol=1e-12, atol=0) and np.allclose(mdl.S[:, 1], mdl.S_op, rtol=1e-12, atol=0)


def test_the_autograd_case_keeps_the_cap_too():
    from test_gpu_query_radiance import autograd_case, chord_case
    mdl = autograd_case()[6]
    assert mdl.zeroed <= RR.CAP and mdl.pairs.sum() > 100
    name, o, d, t, q = chord_case()
    valid = RR.valid_samples(t)
    assert t.shape == (256, 64) and valid.sum() >= 2000 and (t[:8, 0] == 0).all() and (t[8:] == 0).sum() == 0


def test_model_equals_a_literal_loop_on_one_gaussian():
    name, n, K, C = "1_gaussian", 257, 17, 3
    mdl = RR.model(name, n, K, C)
    o, d = RR.case_rays(name, n)
    L, A, S = RR.literal(GR.oracle_scene(name), o, d, mdl.t, mdl.weights, mdl.f)
    scale = np.abs(mdl.S).max()
    print(f"max |model - loop| = {np.abs(L - mdl.L).max():.3e}, {np.abs(A - mdl.opacity).max():.3e}, {np.abs(S - mdl.S).max():.3e} of {scale:.3e}")
    assert np.abs(mdl.L).max() > 0.1
    assert np.all(np.abs(L - mdl.L) <= 1e-13 * scale) and np.all(np.abs(A - mdl.opacity) <= 1e-13 * scale)
    assert np.all(np.abs(S - mdl.S) <= 1e-13 * scale)


def test_points_are_one_f32_multiply_and_one_f32_add():
    rng = np.random.default_rng(3)
    o, d = rng.normal(size=(64, 3)).astype(np.float32), GR.normalized_f32(rng.normal(size=(64, 3)).astype(np.float32))
    t = rng.uniform(0, 9, (64, 5)).astype(np.float32)
    x = RR.points_f32(o, d, t)
    assert x.dtype == np.float32 and x.shape == (64, 5, 3)
    prod = (t[:, :, None].astype(np.float64) * d[:, None, :].astype(np.float64)).astype(np.float32)
    want = (o[:, None, :].astype(np.float64) + prod.astype(np.float64)).astype(np.float32)
    assert np.array_equal(x.view(np.uint32), want.view(np.uint32))
    fused = (o[:, None, :].astype(np.float64) + t[:, :, None].astype(np.float64) * d[:, None, :].astype(np.float64)).astype(np.float32)
    assert (fused.view(np.uint32) != x.view(np.uint32)).any()  # (a fused multiply-add gives other points)


def test_valid_samples_and_the_transmittance_of_special_samples():
    t = np.float32([[0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf]])
    assert RR.valid_samples(t).tolist() == [[True, True, True, False, False, False, False]]
    sc = GR.oracle_scene("1_gaussian")
    o, d = (a[:1] for a in RR.case_rays("1_gaussian", 257))
    T = RR.transmittance(sc, o, d, np.float32([[0.0, -1.0, np.nan, 1e3, np.inf]]))
    assert T[0, 0] == T[0, 1] == T[0, 2] == 1.0 and 0 < T[0, 3] < 1 and T[0, 3] == T[0, 4]
