"""The stack-limit scene and the walk simulators of tests/wide_walk_reference.py on the host reference tree
(tree_reference.assemble): the comb has the properties tests/test_gpu_wide_stack.py relies on, before any of it
runs on a device. No GPU.

Figures on the reference tree (kLeafMax 2, kStackSize 32): 256 Gaussians, 102 of them the comb, 28 pair levels,
74 4-wide nodes. Every F, I and C ray of the three batches reaches its 14th node with 30 entries on the stack
and 7 leaves queued; B rays peak at 24, passing rays at 0; the smallest decision margin is 4.9e-5 of t (floor
2^-18, 64 float32 ulps). Points in the mirrored comb fire the sigma check with 30 entries; rays from the comb
to the test light peak at 33 entries in the secondary walk (VR_WW_STACK is 14).
"""
import functools

import numpy as np
import pytest

import grad_reference as R
import tree_reference as T
import wide_walk_reference as W

MARGIN_FLOOR = 2.0 ** -18  # of t: 64 float32 ulps, where the simulators' arithmetic is the kernels' to the last bit


@functools.lru_cache(maxsize=None)
def lim():
    return T.limits()


@functools.lru_cache(maxsize=None)
def reference_tree(mirrored=False):
    sc = W.comb_scene(lim()["leaf_max"], mirrored)
    return T.assemble(sc.gaussians(), sc.records(), lim()), T.prim_boxes(sc.gaussians()), sc.records()


def cap():
    return 32  # kStackSize (vr_internal.h:91); tree_reference.limits() exports kMaxDepth = 30, and kStackSize >= kMaxDepth + 1


def test_the_comb_is_a_scene_the_device_builder_keeps_with_the_half_trees():
    """256 Gaussians (the device builder's minimum), at most 120 of them over one another, kMaxDepth + 1 levels at the
    most, and a median box extent over 3 % of the scene's half extent (half_tree_rule)."""
    for mirrored in (False, True):
        tree, pb, rec = reference_tree(mirrored)
        n = tree["info"]["num_prims"]
        comb = W.comb_count(lim()["leaf_max"])
        assert n >= 256 and comb <= 120
        assert T.validate(tree, pb, rec) == tree["info"]["bvh_depth"] <= lim()["max_depth"] + 1
        ext = np.sort((pb[:, 3:6] - pb[:, 0:3]).max(axis=1))
        half = float(np.max(0.5 * (tree["info"]["bounds_max"].astype(np.float64) - tree["info"]["bounds_min"])))
        assert ext[n // 2] >= 0.03 * half
        # the ballast is clear of the comb: no ballast ellipsoid reaches within 0.2 of the comb's centre
        mean = rec[:, 0:3][comb:]
        assert np.min(np.linalg.norm(mean - W.CENTRE, axis=1)) - 3.0 * W.BALLAST_SIGMA > 0.2
        # at most 120 Gaussians over one another anywhere: the comb's, and the ballast ellipsoids that can share a point
        # (their centres lie in a ball of one radius, so within two radii along x)
        x = np.sort(mean[:, 0].astype(np.float64))
        crowd = int(max(np.searchsorted(x, xi + 6.0 * W.BALLAST_SIGMA, side="right") - i for i, xi in enumerate(x)))
        print(f"at most {comb} + {crowd} Gaussians share a point")
        assert comb + crowd <= 120
        print(f"mirrored {mirrored}: {n} Gaussians, {comb} in the comb, {tree['info']['bvh_depth']} levels, "
              f"{len(tree['hnodes4'])} 4-wide nodes")


@pytest.mark.parametrize("batch", ["shuffled", "forward64", "forward257"])
def test_every_family_is_on_its_side_of_the_stack_limit(batch):
    tree, _, _ = reference_tree()
    if batch == "shuffled":
        o, d, tmax, names = W.shuffled_batch()
        for k in range(0, len(o), 64):  # every wave holds every family
            assert set(names[k:k + 64]) == set("FBICPX"), k
    else:
        o, d, tmax = W.forward_batch(int(batch[7:]))
        names = np.array(["F"] * len(o))
    for prune in (True, False):  # transmittance and gradients prune at tmax; events do not
        fig = W.family_verdict(W.classify(tree, o, d, tmax, names, cap(), prune), names, cap())
        print(f"{batch} prune {prune}: {fig}")
        assert fig["margin"] > MARGIN_FLOOR
        assert fig["fired"] == int(np.isin(names, list("FIC")).sum())


def test_the_walk_hands_gaussians_out_in_the_order_of_a_recursive_traversal():
    """What GradOp::redo rests on: the Gaussians a walk had queued when its stack filled are the first of the
    plain recursive near-first order of the same tree, for every ray that fires."""
    tree, _, _ = reference_tree()
    o, d, tmax, names = W.shuffled_batch()
    pick = np.nonzero(np.isin(names, list("FIC")))[0][:96]
    S = W.slabs(tree, o[pick], d[pick])
    for k, i in enumerate(pick):
        fired = W.walk_wide(S, k, cap(), float(tmax[i]))
        whole = W.walk_wide(S, k, 10 ** 9, float(tmax[i]))
        rec = W.recursive_order(S, k, float(tmax[i]))
        assert whole["fire"] is None and whole["order"] == rec, i
        assert 0 < len(fired["order"]) < len(rec) and fired["order"] == rec[:len(fired["order"])], i
        assert sorted(rec) == list(range(W.comb_count(lim()["leaf_max"])))  # tree positions: the comb sorts first


def test_points_in_the_mirrored_comb_fire_the_sigma_check():
    pts = sigma_points()
    mirrored, _, _ = reference_tree(True)
    res = W.walk_sigma(mirrored, pts, cap())
    assert all(r["fire"] is not None for r in res)
    plain, _, _ = reference_tree(False)
    quiet = W.walk_sigma(plain, pts, cap())
    assert all(r["fire"] is None and r["peak"] <= 8 for r in quiet)
    m = min(r["margin"] for r in res + quiet)
    print(f"sigma: mirrored peak {max(r['peak'] for r in res)}, plain peak {max(r['peak'] for r in quiet)}, margin {m:.3f}")
    assert m > 1e-3  # of the nodes' normalised coordinates (float32 resolution there: 6e-8)


def sigma_points(n=256, seed=74):
    return (W.CENTRE + np.random.default_rng(seed).uniform(-0.4, 0.4, (n, 3)) * W.EXTENT).astype(np.float32)


def test_rays_to_the_light_overflow_the_secondary_stack():
    """Rays from points in the comb to the test light, walked from the root of the tight tree as sec_node4v does,
    need more than the VR_WW_STACK = 14 entries the kernel keeps in LDS (vr_gauss_secondary.hip:37; the
    library does not export it): the rest goes to stack_ovf."""
    tree, _, _ = reference_tree()
    o = sigma_points(64)
    light = W.light_position().astype(np.float32)
    d = (light[None] - o).astype(np.float32)
    dist = np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.all(W.normalise(d) >= 0.3)
    S = W.slabs(tree, o, d, which="hnodes4s")
    res = [W.walk_secondary(S, r, float(dist[r])) for r in range(len(o))]
    peaks = [p for p, _, _ in res]
    print(f"secondary walk: peak {min(peaks)} .. {max(peaks)}, margin {min(m for _, m, _ in res):.2e}, "
          f"largest index of an unconditional store {max(t for _, _, t in res)}")
    assert min(peaks) > W.WW_STACK
    assert min(m for _, m, _ in res) > MARGIN_FLOOR


@pytest.mark.parametrize("plan", ["TFFFF", "EEETFFFF"])
def test_light_rays_in_the_threshold_combs_store_at_the_first_row_past_the_stack(plan):
    """The mirrored combs of test_secondary_walk_where_its_branch_free_pushes_end: a level that pushes two, then
    full levels, so that a light ray enters a node with VR_WW_STACK - 3 entries, its nearest child in the last slot.
    The branch-free form's store for that slot is then at row VR_WW_STACK (on the shared tree, walked from the
    root); on the plain comb (nearest child first) such a step never stores past row VR_WW_STACK - 1."""
    arr = W.comb_arrays(lim()["leaf_max"], True, plan=plan)
    import vr_amd as vr
    sc = vr.Scene.from_gaussians(*arr)
    tree = T.assemble(sc.gaussians(), sc.records(), lim())
    T.validate(tree, T.prim_boxes(sc.gaussians()), sc.records())
    o = sigma_points(64)
    light = W.light_position(True).astype(np.float32)
    d = (light[None] - o).astype(np.float32)
    dist = np.linalg.norm(d.astype(np.float64), axis=1)
    S = W.slabs(tree, o, d, which="hnodes4")
    res = [W.walk_secondary(S, r, float(dist[r])) for r in range(len(o))]
    assert {t for _, _, t in res} == {W.WW_STACK}
    assert min(m for _, m, _ in res) > MARGIN_FLOOR


def test_the_density_leaves_half_of_the_forward_rays_translucent():
    """Chosen with the oracle alone: Tr of the 64 forward rays."""
    sc = W.comb_oracle(lim()["leaf_max"])
    o, d, _ = W.forward_batch(64)
    tr = np.exp(-R.Model(sc, o, d, np.inf).tau)
    mid = float(np.mean((tr >= 0.05) & (tr <= 0.95)))
    print(f"Tr {tr.min():.3f} .. {tr.max():.3f}, {100 * mid:.0f} % in [0.05, 0.95]")
    assert mid >= 0.5


def test_the_flight_cases_are_forward_and_backward_rays():
    """flight_reference's comb cases: every ray of the forward camera fires, no ray of the backward one; the rays
    keep every component of their direction over 0.3. Their targets are the oracle's own, and the model's share
    of rays left out (within 1e-5 of an event) is 0 of 256 in both, inside the 2 that judge allows
    (test_flight_reference.py asserts the model's side of it for every case, these two included)."""
    import flight_reference as F
    tree, _, _ = reference_tree()
    for name, fires in (("comb", True), ("comb_back", False)):
        o, d, _ = F.rays(name)
        assert np.all(np.abs(d) >= 0.3) and np.all((d > 0) == fires)
        S = W.slabs(tree, o, d, unit=True)
        res = [W.walk_wide(S, r, cap(), prune=False) for r in range(len(o))]
        assert all((r["fire"] is not None) == fires for r in res), name
        assert min(r["margin"] for r in res) > MARGIN_FLOOR
        if fires:
            assert min(r["leaves_before"] for r in res) >= 6
        else:
            assert max(r["peak"] for r in res) < cap() - 2
        rec = F.record(name)
        sc = ~np.isnan(rec[:, 1])
        near = F.model(name).near_event(np.where(sc, rec[:, 1], 0.0)) & sc
        print(f"{name}: {int(sc.sum())} scatter, {int(near.sum())} near an event")
        assert near.sum() <= 2
