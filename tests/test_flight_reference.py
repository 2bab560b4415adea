"""The free-flight query's reference data (tests/flight_reference.py) on its own, against the oracle's per-path
record: the rebuilt rays are the oracle's, the cases have the properties test_gpu_query_flight.py relies on, and
the float64 model agrees with the oracle's own f32 answers. No GPU."""
import numpy as np
import pytest

import flight_reference as R

CASES = list(R.CASES)


@pytest.mark.parametrize("name", CASES)
def test_rebuilt_rays_reproduce_the_oracle_positions_bit_for_bit(name):
    """pos = origin + t_scatter * direction in f32 (integrator.h:600) equals the record's slots 4-6 exactly, on
    every scattering ray; the case scatters as often as its table entry says."""
    rec = R.record(name)
    o, d, tgt = R.rays(name)
    sc = ~np.isnan(rec[:, 1])
    assert int(sc.sum()) == R.SCATTERING[name]
    pos = o + rec[:, 1:2] * d
    assert pos.dtype == np.float32
    assert np.array_equal(pos[sc], rec[sc, 4:7])
    assert np.array_equal(tgt[sc], rec[sc, 0]) and np.all(np.isfinite(tgt)) and np.all(tgt >= 0)
    nrm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    assert np.max(np.abs(nrm - 1.0)) < 1e-6  # unit directions: the query gets them with unit = 1


@pytest.mark.parametrize("name", CASES)
def test_model_agrees_with_the_oracle_record(name):
    """Escape: the float64 optical depth of the whole ray is below the target exactly on the rays the oracle lets
    escape, by the case's margin (thousands of f32 ulps). Scatter: the model's optical depth at the oracle's t is the
    target within the reference's own f32 residual (1.7e-3 in optical depth measured over these cases, every solver:
    the Newton / bisection tolerance 1e-6 is on an f32 sum of up to 200 terms), here 2e-3; the oracle's albedo is the
    model's within 1e-5 (measured 4e-6) and at most one ray's t lies within 1e-5 of an event."""
    rec, m = R.record(name), R.model(name)
    _, _, tgt = R.rays(name)
    esc = np.isnan(rec[:, 1])
    total = m.tau(np.full(len(tgt), np.inf))
    has = m.hit.any(1)
    margin = np.abs(total - tgt)[has]
    print(f"{name}: {int((~esc).sum())} scatter, smallest |tau_total - target| {margin.min():.2e}")
    assert np.array_equal(total < tgt, esc)
    sc = ~esc
    if name != "250_random_ortho":
        assert margin.min() > 1e-3
    t = np.where(sc, rec[:, 1], 0.0)
    res = np.abs(m.tau(t) - tgt)[sc]
    near = m.near_event(t) & sc
    use = sc & ~near
    da = np.abs(m.albedo(t) - rec[:, 2])[use]
    print(f"{name}: max |tau64(t_orc) - target| {res.max():.2e}, max |albedo_orc - model| {da.max():.2e}, near an event {int(near.sum())}")
    assert res.max() <= 2e-3
    assert da.max() <= 1e-5
    assert near.sum() <= 1


def test_cases_exercise_windows_and_the_big_rows():
    """The slab's rays cross 29-349 Gaussians (median 145: more than a 128-entry window) with up to 86 active at
    once; the coincident case has all 200 active at every collision (over the 128-entry rows)."""
    m = R.model("slab")
    hits = m.hit.sum(1)
    assert hits.min() == 29 and hits.max() == 349 and int(np.median(hits)) == 145
    rec = R.record("coincident200")
    sc = ~np.isnan(rec[:, 1])
    assert np.all(R.model("coincident200").active(np.where(sc, rec[:, 1], 0.0)).sum(1)[sc] == 200)


@pytest.mark.parametrize("solver", [1, 2, 3])
def test_solver_modes_change_the_record_not_the_rays(solver):
    a, b = R.record("250_random"), R.record("250_random", solver)
    assert np.array_equal(np.isnan(a[:, 1]), np.isnan(b[:, 1]))
    sc = ~np.isnan(a[:, 1])
    assert np.array_equal(a[sc, 0], b[sc, 0]) and not np.array_equal(a[sc, 1], b[sc, 1])
