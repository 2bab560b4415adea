"""Both uploads and the trees on elongated Gaussians (aniso_cases.py, 512 of them): disc 100 and needle 30, whose
cofactor sums cancel to a part in 1e4 and 1e3, and needle 100, where the cancellation leaves records whose M is not
positive definite. The assertions are test_gpu_upload_device.py's (Device.upload_gaussians against the host upload
with VR_OPT_DEVICE_BVH = 1: every tree array and every record word but `norm` bit-equal, a NaN or inf word included,
`norm` within 2 ulp) and tree_reference's validators, here on boxes a hundred times thinner than they are wide."""
import numpy as np
import pytest

import aniso_cases as A
import tree_reference as T
import vr_amd as vr
from test_gpu_query import PARITY, check_events
from test_gpu_upload_device import assert_same_upload, both_trees, records_by_rule

pytestmark = pytest.mark.gpu

CASES = [pytest.param(k, id=A.case_id(k)) for k in (("disc", 100), ("needle", 30), ("needle", 100))]


@pytest.mark.parametrize("key", CASES)
def test_trees_and_records(key, device_options):
    """The device-array upload equals the host upload word for word; both trees pass the validators, which hold each
    tight box of the secondary tree to the float64 3-sigma extent of its record's M and to an infinite box where M
    is not positive definite; needle 100 reports the M-form route (wrec_pd false), the others the whitened one.
    Measured on an MI355X: no row's norm differs from the host's at any of the three; 12 levels, 157 4-wide nodes; the
    thinnest box is 3.4e-2, 3.3e-2 and 1.0e-2 of its width; needle 100 has 2 non-PD records and no tight tree."""
    arrs = A.arrays(A.gaussians(*key, 512))
    got, want, sc = both_trees(arrs, device_options)
    assert got["info"]["built_on_device"] and want["info"]["built_on_device"]
    assert_same_upload(got, want, arrs)
    _, nonpd, bad = A.record_health(got["records"])
    assert not bad.any()
    pb = T.prim_boxes(sc.gaussians())
    for tree in (got, want):
        levels = T.validate(tree, pb, records_by_rule(sc, arrs))
    T.check_against_reference(got, pb)
    thin = (pb[:, 3:6] - pb[:, 0:3]).min(1) / (pb[:, 3:6] - pb[:, 0:3]).max(1)
    print(f"{A.case_id(key)}: {levels} levels, {len(got['hnodes4'])} 4-wide nodes, tight {len(got['hnodes4s'])}, non-PD records "
          f"{int(nonpd.sum())}, wrec_pd {got['info']['wrec_pd']}, thinnest box {thin.min():.1e} of its width")
    assert bool(got["info"]["wrec_pd"]) == (not nonpd.any())
    assert nonpd.any() == (key == ("needle", 100))


def test_forward_queries_beside_non_pd_records():
    """needle 100: on the kept rays that the probe reports on no non-PD record, transmittance and tau are within
    1e-4 of the oracle and the events are the oracle's exactly, with the scene on the M-form route. Measured on an
    MI355X: 255 of 256 rays kept, |dTr| 6.1e-8, |dtau| / max(1, tau) 1.2e-7, the oracle 0.16 from float64."""
    key = ("needle", 100)
    rc = A.ray_case(*key)
    k = rc.keep & ~rc.nonpd_rays
    assert k.mean() >= 0.9
    dev, sc = vr.Device.get(0), A.device_scene(*key)
    o, d = np.ascontiguousarray(rc.o[k]), np.ascontiguousarray(rc.d[k])
    tr, tau = dev.query_transmittance(sc, o, d, return_tau=True)
    assert not dev.debug_tree()["info"]["wrec_pd"]
    e_tr = np.abs(tr.astype(np.float64) - rc.tr_oracle[k])
    e_tau = np.abs(tau.astype(np.float64) - rc.tau_oracle[k]) / np.maximum(1.0, rc.tau_oracle[k])
    print(f"aniso needle100: kept {int(k.sum())} of {len(k)} rays, max |Tr - oracle| = {e_tr.max():.3e}, max |tau - oracle| / "
          f"max(1, tau) = {e_tau.max():.3e}, oracle against float64 {np.abs(rc.tr_oracle - rc.tr_f64)[k].max():.3e}")
    assert e_tr.max() <= PARITY and e_tau.max() <= PARITY
    check_events(rc.pr[k], *dev.query_events(sc, o, d))
