"""The secondary rays' start entries and climbs at the smallest trees and lists at which they can go wrong, every
ray against the oracle.

A secondary ray takes its start node and that node's parent entry from one per-record entry (record_start_kernel)
and, when it climbs out of a finished subtree, steps to the parent entry it loaded one climb earlier while it
issues the load of the next one (sec_node4v); the list phase carries the start node in `node`. The cases of
tests/secondary_chain_cases.py are the shapes at which an entry, a look-ahead or the phase switch is at its edge:
a tree of one node (the entry is the root, nothing to climb to), lists of one to three members, a root with leaf
children only, one climb to the root (whose look-ahead entry is -1), and climbs over every level of the deepest tree
the builder keeps; then the walks from the root (no entries) and on the device-built tree (another parent table).

Every case: 16 x 16, one light, 3 environment samples, t_eps 0; the rows of Device.debug_pixel_records against the
oracle's at records_compare's bars (positions and active counts bit for bit, every ray's Tr to 1e-4). A case counts
only with RC.MIN_SPREAD_SHARE of its rays at an oracle Tr in [0.05, 0.95]; tests/test_secondary_chain_reference.py
asserts that of the oracle alone, without a GPU.

(Whether the chain case's walks reach the traversal stack's global overflow is not observable from here: its 4-wide
nodes have mostly leaf children, so its stack stays shallow; what the case does exercise is a climb at every level.)
"""
import pytest

import vr_amd as vr
import records_compare as RC
import secondary_chain_cases as C

pytestmark = pytest.mark.gpu


def _device_rows(arrays, camera, pixels):
    scene = vr.Scene.from_gaussians(*arrays[:4], [vr.Light(p, i) for p, i in zip(arrays[4], arrays[5])])
    img = vr.Image(C.W, C.W)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(*camera), step_size=RC.STEP, env_samples=C.ENV_SAMPLES, t_eps=0.0)
    integ.render(scene, img)
    st = dict(integ.last_stats)
    assert st["error_pixels"] == 0
    dev = vr.Device.get(0)
    return scene, st, {(int(x), int(y)): dev.debug_pixel_records(int(x), int(y)) for x, y in pixels}


def _check(tag, name):
    arrays, camera, pixels, orc_rows = C.reference(name)
    scene, st, dev_rows = _device_rows(arrays, camera, pixels)
    total, msgs = RC.Report(), []
    for p in orc_rows:
        rep = RC.compare_rows(dev_rows[p], orc_rows[p], arrays[4], arrays[5], scene.env_color)
        if rep.findings:
            msgs.append(f"pixel {p}: {rep.describe()}")
        total.merge(rep)
    print(f"{tag}: {len(dev_rows)} pixels, {total.summary()}; secondary rays {st['secondary_rays']}, "
          f"slow {st['slow_rays']}, deep pixels {st['deep_pixels']}")
    assert not msgs, "\n".join(msgs)
    assert total.one_sided == 0 and total.rows > 0
    assert total.spread_share >= RC.MIN_SPREAD_SHARE
    return total


@pytest.mark.parametrize("name", list(C.CASES))
def test_secondary_rays_match_the_oracle(name):
    rep = _check(name, name)
    assert rep.rows == sum(len(r) for r in C.reference(name)[3].values())


@pytest.mark.parametrize("name,option,value", C.OPTION_CASES, ids=[f"{n}-{o}={v}" for n, o, v in C.OPTION_CASES])
def test_secondary_rays_match_the_oracle_under_tree_options(name, option, value, device_options):
    device_options(option, value)  # (before the scene is made: the tree options apply at its upload)
    _check(f"{name} {option}={value}", name)
