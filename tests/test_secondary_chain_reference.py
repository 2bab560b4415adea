"""The oracle side of tests/test_gpu_secondary_chain.py, without a GPU: every case's secondary rays spread over
(0, 1), its active lists have the lengths the case is about, and the reference tree of each scene has the shape
the case names (tests/tree_reference.py, the device builder's tree)."""
import numpy as np
import pytest

import records_compare as RC
import secondary_chain_cases as C
import tree_reference as T

# name: the active-list lengths the case's rows must show (a subset of what they do show)
LIST_LENGTHS = {"single-1": {1}, "single-2": {1, 2}, "nested-3": {1, 2, 3}, "scattered-6": {1, 2, 3},
                "scattered-24": {1, 2, 3, 8}, "chain": {1, 2, 65}}


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_spreads_over_the_unit_interval(name):
    rep, rows = C.oracle_report(name)
    print(f"{name}: {rep.summary()}")
    assert rep.findings == [], rep.describe()  # (Li + Le follows from the oracle's own Tr)
    assert rep.rows >= 100 and sum(len(r) > 0 for r in rows.values()) >= 5
    assert rep.spread_share >= RC.MIN_SPREAD_SHARE
    lengths = {int(a) for r in rows.values() for a in r[:, 8]}
    want = LIST_LENGTHS[name]
    assert {n for n in want if n < 65} <= lengths, lengths
    if 65 in want:  # the lists sec_finish re-intersects
        assert max(lengths) > 64


def _levels4(parent4):
    """Depth of the deepest 4-wide node (root: 1)."""
    deepest = 0
    for i in range(len(parent4)):
        d, x = 1, i
        while x > 0:
            x = int(parent4[x]) & T.PARENT_MASK
            d += 1
        deepest = max(deepest, d)
    return deepest


def _tree(name):
    import vr_amd as vr
    arrays = C.reference(name)[0]
    scene = vr.Scene.from_gaussians(*arrays[:4])
    return T.assemble(scene.gaussians(), scene.records(), T.limits())


def test_reference_trees_have_the_shapes_the_cases_name():
    for name in ("single-2", "nested-3"):  # a single node: its parent entry is -1, nothing to climb to
        t = _tree(name)                    # (the reference tree needs two Gaussians: single-1 has no other shape)
        assert len(t["hnodes4"]) == 1 and int(t["parent4"][0]) == -1
    six = _tree("scattered-6")  # the root with leaf children only
    assert len(six["hnodes4"]) == 1 and np.all(six["hnodes4"]["c"][0] < 0)
    # climbs that end in the root, whose own parent entry is -1 (8 nodes on 3 levels: no seed of this scene gives 2)
    t24 = _tree("scattered-24")
    assert _levels4(t24["parent4"]) == 3 and int(t24["parent4"][0]) == -1
    chain = _tree("chain")  # more 4-wide levels than the 14 entries of the LDS traversal stack
    assert C.chain_levels() == T.limits()["max_depth"] + 1
    assert _levels4(chain["parent4"]) > 14
