"""The elongated-Gaussian recipe of aniso_cases.py, pinned on the CPU: what the GPU tests of test_gpu_aniso_*.py rely
on is asserted here of the oracle and the float64 models alone. Each test prints its rung's row of the table in
DESIGN.md ("Elongated Gaussians"): run with -s to regenerate it.
"""
import numpy as np
import pytest

import aniso_cases as A

SIGMA_RTOL = 5.3e-6  # test_gpu_query.py's, restated here so that this file imports nothing that needs a GPU
RUNGS = [pytest.param(k, id=A.case_id(k)) for k in A.LADDER]


@pytest.mark.parametrize("key", RUNGS)
def test_records(key):
    """kappa(M) of the oracle's f32 records is within 2x of ratio^2, and every M is positive definite, on every rung
    below needle 100. At needle 100 the cofactor inverse's cancellation leaves an M that is not positive definite
    on at least one record, and kappa of the others spreads over a decade (measured 4.7e3 .. 4.2e4), so only the
    median is held to the factor 2 there."""
    shape, ratio = key
    kappa, nonpd, bad = A.record_health(A.records(*key))
    print(f"{A.case_id(key)}: N = {len(kappa)}, kappa(M) {kappa[~nonpd].min():.4g} .. {kappa[~nonpd].max():.4g} (median "
          f"{np.median(kappa):.4g}), ratio^2 = {ratio ** 2}, non-PD records {int(nonpd.sum())}, non-finite {int(bad.sum())}")
    assert not bad.any()  # no NaN-record scene goes to the GPU
    if key == ("needle", 100):
        assert nonpd.sum() >= 1
        assert 0.5 * ratio ** 2 <= np.median(kappa) <= 2.0 * ratio ** 2
    else:
        assert nonpd.sum() == 0
        assert np.all((kappa >= 0.5 * ratio ** 2) & (kappa <= 2.0 * ratio ** 2))


@pytest.mark.parametrize("key", RUNGS)
def test_aimed_rays(key):
    """The phantom-ray rule takes at most 5 % of the rays, at least 25 % of the kept rays have an oracle Tr in
    (0.01, 0.99), and the oracle hits the Gaussian a ray aims at on most rays. Prints the oracle against float64."""
    rc = A.ray_case(*key)
    n = len(rc.o)
    hit32 = rc.pr[..., 0] != 0
    e = np.abs(rc.tr_oracle - rc.tr_f64)
    mid = float(np.mean((rc.tr_oracle[rc.keep] > 0.01) & (rc.tr_oracle[rc.keep] < 0.99)))
    aimed = float(hit32[np.arange(n), rc.aimed].mean())
    print(f"| {key[0]} {key[1]} | {key[1] ** 2:.0e} | {e.max():.1e} | {int((e > 5e-5).sum())} / {n} | {rc.flips} |  "
          f"phantom rays {int((~rc.keep).sum())}, rays on a non-PD record {int(rc.nonpd_rays.sum())}, aimed Gaussian hit "
          f"{100 * aimed:.0f} %, {hit32.sum(1).mean():.1f} hits per ray, Tr in (0.01, 0.99) on {100 * mid:.0f} % of the kept rays")
    assert (~rc.keep).mean() <= A.CAP
    assert mid >= 0.25
    assert aimed >= 0.85
    if key == A.CONTROL:
        assert rc.flips == 0 and e.max() <= 1e-4  # inside today's family float64 still is a fair reference


@pytest.mark.parametrize("key", RUNGS)
def test_aimed_points(key):
    """The cut-off rule takes at most 5 % of the points, at least 50 % of them lie inside one or more ellipsoids, on
    the kept points the f32 restatement takes the float64 decisions, and its sigma is within the scaled SIGMA_RTOL
    of the float64 model: the bar test_gpu_aniso_query.py sets the device is one that line-faithful f32 code meets."""
    sc = A.sigma_case(*key)
    rec = A.records(*key)
    _, nonpd, _ = A.record_health(rec)
    qerr, scale = A.q_error(*key), A.sigma_scale(*key)
    inside = float(np.mean(sc.active > 0))
    act32 = ((A.q_ref_f32(rec, sc.p) <= np.float32(9.0)) & ~nonpd[None, :]).sum(1)
    act64 = ((sc.q64 <= 9.0) & ~nonpd[None, :]).sum(1)
    rel = np.abs(sc.sigma_f32 - sc.sigma) / np.maximum(1.0, sc.sigma)
    print(f"{A.case_id(key)}: max |q32 - q64| near the cut-off {qerr:.2e}, SIGMA_RTOL x {scale:.1f} = {SIGMA_RTOL * scale:.2e}, "
          f"cut-off points {int((~sc.keep).sum())} / {len(sc.p)}, inside an ellipsoid {100 * inside:.0f} %, up to "
          f"{int(sc.active.max())} active, f32 restatement against float64 {rel[sc.keep].max():.2e}, largest sigma {sc.sigma.max():.0f}")
    assert (~sc.keep).mean() <= A.CAP
    assert inside >= 0.5
    assert np.array_equal(act32[sc.keep], act64[sc.keep])
    if not nonpd.any():
        assert rel[sc.keep].max() <= SIGMA_RTOL * scale


@pytest.mark.parametrize("key", RUNGS)
def test_finite_tmax_cuts_inside_the_cloud(key):
    """tmax = U(0.3, 1) x the distance to the target clips some hit of at least a quarter of the rays."""
    rc = A.ray_case(*key)
    tmax, tau = A.finite_case(*key)
    cut = np.any((rc.pr[..., 0] != 0) & (rc.pr[..., 2] > tmax[:, None]), axis=1)
    print(f"{A.case_id(key)}: tmax clips or drops a hit on {100 * cut.mean():.0f} % of the rays, largest tau {tau.max():.2f}")
    assert cut.mean() >= 0.25 and np.all(np.isfinite(tau))


@pytest.mark.parametrize("name", ["disc10", "disc30"])
def test_free_flight_reference_meets_its_own_conditions(name):
    """flight_reference.judge's conditions, which test_gpu_aniso_query.py sets the device, hold of the oracle's own
    answers at disc 10 and disc 30: the rebuilt rays reproduce its positions bit for bit, and its albedo is the
    float64 model's within 1e-4 with at most 2 collisions within 1e-5 of an event. The float64 optical depth at
    the oracle's t is printed, not asserted: it is 1.6e-2 (disc 10) and 0.15 (disc 30) from the target where the
    kappa <= 12 cases are within 2e-3, which is why the oracle's t, not float64, is the reference for t."""
    import flight_reference as R
    rec, m = R.record(name), R.model(name)
    o, d, tgt = R.rays(name)
    sc = ~np.isnan(rec[:, 1])
    assert int(sc.sum()) == R.SCATTERING[name]
    assert np.array_equal((o + rec[:, 1:2] * d)[sc], rec[sc, 4:7])
    t = np.where(sc, rec[:, 1], np.float32(-1.0)).astype(np.float32)
    res = np.abs(m.tau(np.where(sc, t, 0.0)) - tgt)[sc]
    print(f"{name}: max |tau64(t_orc) - target| {res.max():.2e}, up to {int(m.hit.sum(1).max())} hits per ray")
    fig = R.judge(name, t, np.where(sc, rec[:, 2], 0.0).astype(np.float32), None, label=name + " oracle")
    assert fig["dTr"] == 0.0


@pytest.mark.parametrize("key", [pytest.param(k, id=A.case_id(k)) for k in A.RECORD_CASES])
def test_record_pixels_have_rows_and_fair_rays(key):
    """Each of the rung's six pixels has oracle rows; at least 25 % of the case's secondary rays are fair (the oracle's
    f32 Tr within 0.5e-4 of the float64 ray model's), so the 1e-4 bar against the oracle is applied on real ground, at
    the recipe's own density (no rung needed a lower one); at least 25 % of the rays have a Tr in [0.05, 0.95]."""
    import records_compare as RC
    rows, model = A.record_case(*key)
    tr_o = np.concatenate([r[:, 9:].astype(np.float64) for r in rows.values()])
    t64 = np.concatenate([np.array([model[p][int(r[0])] for r in rows[p]]).reshape(-1, tr_o.shape[1]) for p in rows])
    e = np.abs(tr_o - t64)
    fair = float(np.mean(e <= RC.FAIR_E_REF))
    spread = float(np.mean((tr_o >= RC.SPREAD[0]) & (tr_o <= RC.SPREAD[1])))
    print(f"{A.case_id(key)} records: {len(tr_o)} rows, {tr_o.size} rays, fair {100 * fair:.0f} %, max |Tr_oracle - Tr_f64| {e.max():.2e}, "
          f"{100 * spread:.0f} % of the rays with Tr in [{RC.SPREAD[0]}, {RC.SPREAD[1]}]")
    assert all(len(r) > 0 for r in rows.values())
    assert fair >= A.MIN_FAIR_SHARE
    assert spread >= RC.MIN_SPREAD_SHARE


def test_float64_ray_model_reproduces_the_oracle_inside_todays_family():
    """At disc 3 (kappa 9) the float64 ray model of records_compare agrees with the oracle's own Tr to 1e-4 on every
    secondary ray of two pixels: the rays it rebuilds (light distance, environment directions, their order) are the
    oracle's."""
    import records_compare as RC
    osc, rec = A.oracle_scene(*A.CONTROL), A.records(*A.CONTROL)
    worst = 0.0
    for x, y in [(11, 8), (20, 10)]:
        rows = RC.oracle_rows(osc, x, y, A.RECORD_W, A.RECORD_W, A.RECORD_ENV, cam=A.RECORD_CAMERA)
        model = RC.ray_model_f64(rec, rows, x, y, [A.LIGHT[0]], A.RECORD_ENV)
        assert len(rows) > 100
        worst = max(worst, max(float(np.abs(r[9:] - model[int(r[0])]).max()) for r in rows))
    print(f"disc3: max |Tr_oracle - Tr_f64| over two pixels' rays {worst:.2e}")
    assert worst <= 1e-4
