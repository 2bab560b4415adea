"""The frame at record level on elongated Gaussians (aniso_cases.py): disc 10, disc 30 and needle 10 rendered 24 x 24 with
env_samples 3, six pixels each through records_compare, plus one free-flight frame at disc 10.

The march columns keep their rules: step, position and active count bit for bit, T sigma_s to 1e-5 (the primary march
is line-faithful). The secondary rays' whitened forms (wquad / wintersect, kChordBand, kMemberAmb in
vr_gauss_common.h) compute differently from the reference on purpose and were sized at kappa <= 12, so each ray is
judged with the float64 ray model of records_compare.compare_rows(tr_f64=...): a fair ray (the oracle itself within
0.5e-4 of float64) to |Tr_dev - Tr_oracle| <= 1e-4, any other to |Tr_dev - Tr_f64| <= e_ref + 1e-4.

Measured on an MI355X (rays, fair share, max |Tr_dev - Tr_oracle| on the fair rays, max |Tr_dev - Tr_f64| - e_ref on the
others, max e_ref): disc 10: 2592, 94 %, 4.9e-5, <= 0, 3.3e-4; disc 30: 1244, 64 %, 4.9e-5, 1.5e-8, 3.0e-3; needle 10:
532, 97 %, 4.7e-5, <= 0, 3.8e-4. No ray fails either rule, so the bands of vr_gauss_common.h stay unscaled.
"""
import pytest

import aniso_cases as A
import records_compare as RC
import vr_amd as vr
from helpers import FOV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", [pytest.param(k, id=A.case_id(k)) for k in A.RECORD_CASES])
def test_records_match_the_oracle(key):
    scene = A.device_scene(*key)
    img = vr.Image(A.RECORD_W, A.RECORD_W)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(*A.RECORD_CAMERA, FOV), step_size=RC.STEP, env_samples=A.RECORD_ENV)
    integ.render(scene, img)
    st = dict(integ.last_stats)
    assert st["error_pixels"] == 0
    dev = vr.Device.get(0)
    orc_rows, model = A.record_case(*key)
    lp, li = RC.lights_of(scene)
    total, msgs = RC.Report(), []
    for p in A.RECORD_CASES[key]:
        rep = RC.compare_rows(dev.debug_pixel_records(*p), orc_rows[p], lp, li, scene.env_color, tr_f64=model[p])
        if rep.findings:
            msgs.append(f"pixel {p}: {rep.describe()}")
        total.merge(rep)
    print(f"aniso records {A.case_id(key)}: slow rays {st['slow_rays']}, band rays {st['band_rays']}, fallback pixels "
          f"{st['fallback_pixels']}; {total.summary()}; fair rays {100 * total.fair_share:.0f} %, max |Tr_dev - Tr_oracle| on them "
          f"{total.max_fair:.3e}, max |Tr_dev - Tr_f64| - e_ref on the others {total.max_other:.3e}, max e_ref {total.max_e_ref:.3e}")
    assert not msgs, "\n".join(msgs)
    assert total.one_sided == 0 and total.rows > 0
    assert total.fair_share >= A.MIN_FAIR_SHARE
    assert total.spread_share >= RC.MIN_SPREAD_SHARE


def test_free_flight_frame_matches_the_oracle():
    """MultiScatterGaussians, 16 x 16 at 4 samples per pixel through the disc 10 scene, under test_gpu_freeflight.py's
    bars (99.9 % of the pixels within 1e-4, mean |diff| <= 1e-4, image means within 0.5 %)."""
    import pyoracle as O
    from test_gpu_freeflight import _check, _gpu
    key = ("disc", 10)
    g = _gpu(A.device_scene(*key), 16, 16, True, 4, cam=vr.Pinhole_Camera(*A.RECORD_CAMERA, FOV))
    r = O.render_ff(A.oracle_scene(*key), O.PINHOLE, *A.RECORD_CAMERA, FOV, 16, 16, multi=True, num_samples=4)
    _check(g, r)
