"""The host tree reference (tests/tree_reference.py) on its own: its validator accepts a complete tree
assembled from the reference and reports each kind of damage by name, and the scenes of test_gpu_tree.py
have, on the reference, the properties those tests rely on. No GPU."""
import copy
import functools

import numpy as np
import pytest

import tree_reference as T
import vr_amd as vr


@functools.lru_cache(maxsize=None)
def lim():
    return T.limits()


def random_scene(n, seed):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    return vr.Scene.from_gaussians(mean, T.rotated_cov(rng, n), rng.uniform(0.5, 2.0, n), rng.uniform(0.2, 0.9, n))


@functools.lru_cache(maxsize=None)
def assembled():
    """(tree dict from the reference alone, primitive boxes, scene records) of a 300-Gaussian random scene."""
    sc = random_scene(300, 5)
    g = sc.gaussians()
    return T.assemble(g, sc.records(), lim()), T.prim_boxes(g), sc.records()


def fresh():
    tree, pb, rec = assembled()
    return copy.deepcopy(tree), pb, rec


def first_leaf(tree, count):
    """(node, side) of a leaf child with `count` primitives."""
    for i in range(len(tree["nodes"])):
        for s in range(2):
            r = int(tree["nodes"]["c"][i, s])
            if r < 0 and T.leaf_range(r)[1] == count:
                return i, s
    raise AssertionError(f"no leaf of {count}")


def test_validator_accepts_the_reference_tree():
    tree, pb, rec = fresh()
    assert T.validate(tree, pb, rec) == tree["info"]["bvh_depth"]
    assert T.validate(tree, None, rec) == tree["info"]["bvh_depth"]
    assert tree["info"]["num_nodes4"] > 50 and len(tree["hnodes"]) == len(tree["nodes"]) > 100
    tighter = tree["hnodes4s"]["h"] != tree["hnodes4"]["h"]
    assert len(tree["hnodes4s"]) == len(tree["hnodes4"]) and tighter.mean() > 0.5  # the refit is tighter on most bounds
    assert T.same_pair_tree(tree, T.radix_tree(T.morton_keys(pb), lim()["leaf_max"]), pb[tree["order"]]) == len(tree["nodes"])


def ulp_down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def mutate_f32_max(tree):
    tree["nodes"]["f"][7, 3] = ulp_down(tree["nodes"]["f"][7, 3])
    return 7


def mutate_half_min_inward(tree):
    h = tree["hnodes"]["h"][9:10, 0:1].view(np.float16)
    h[...] = np.nextafter(h, np.float16(np.inf))
    return 9


def mutate_half_max_outward(tree):
    h = tree["hnodes"]["h"][11:12, 9:10].view(np.float16)
    h[...] = np.nextafter(np.nextafter(h, np.float16(np.inf)), np.float16(np.inf))
    return 11


def mutate_order_swap(tree):
    tree["order"][[3, 200]] = tree["order"][[200, 3]]
    return None


def mutate_leaf_count(tree):
    assert lim()["leaf_max"] >= 2
    i, s = first_leaf(tree, 2)
    first, _ = T.leaf_range(tree["nodes"]["c"][i, s])
    for name in ("nodes", "hnodes"):
        tree[name]["c"][i, s] = T.make_leaf(first, 1)
    return None


def mutate_prim_node(tree):
    for j in range(len(tree["prim_node4"])):  # the first record whose leaf's node has a sibling node
        i = int(tree["prim_node4"][j])
        p = int(tree["parent4"][i]) & T.PARENT_MASK if i else 0
        siblings = [int(r) for r in tree["hnodes4"]["c"][p] if r > 0 and r != i]
        if i and siblings:
            tree["prim_node4"][j] = siblings[0]
            return i
    raise AssertionError("no node with a sibling")


def mutate_parent_slot(tree):
    r = 5
    p = int(tree["parent4"][r])
    slot = (p >> 28) - 1
    tree["parent4"][r] = (p & T.PARENT_MASK) | (((slot + 1) % 4 + 1) << 28)
    return 5


def mutate_depth(tree):
    tree["info"] = dict(tree["info"], bvh_depth=tree["info"]["bvh_depth"] - 1)
    return None


def step16(bits, up):
    h = np.array([bits], np.uint16).view(np.float16)
    return np.nextafter(h, np.float16(np.inf if up else -np.inf)).view(np.uint16)[0]


def mutate_wide_box(tree):
    tree["hnodes4"]["h"][4, 0, 3] = step16(tree["hnodes4"]["h"][4, 0, 3], True)  # still conservative, no longer the pair tree's
    return 4


def mutate_wide_empty(tree):
    i = int(np.nonzero(tree["hnodes4"]["c"][:, 3] == 0)[0][0])
    tree["hnodes4"]["h"][i, 3] = 0
    return i


def mutate_per_axis(tree):
    tree["hnodes4w"][6, 5] ^= 1 << 16
    return 6


def mutate_tight_inward(tree):
    """A tight minimum that is the refit's own (not the shared box's) stepped inward by one half ulp."""
    t, h = tree["hnodes4s"]["h"], tree["hnodes4"]["h"]
    i, s, k = [int(v[0]) for v in np.nonzero((t != h) & (np.arange(6) < 3))]
    t[i, s, k] = step16(t[i, s, k], True)
    tree["hnodes4t"] = T.soa_words(tree["hnodes4s"])
    return i


def mutate_tight_outside(tree):
    t, h = tree["hnodes4s"]["h"], tree["hnodes4"]["h"]
    t[2, 0, 4] = step16(h[2, 0, 4], True)
    tree["hnodes4t"] = T.soa_words(tree["hnodes4s"])
    return 2


@pytest.mark.parametrize("mutation,invariant", [
    (mutate_wide_box, "wide-box"),
    (mutate_wide_empty, "wide-empty"),
    (mutate_per_axis, "per-axis"),
    (mutate_tight_inward, "tight-contain"),
    (mutate_tight_outside, "tight-outside"),
    (mutate_f32_max, "pair-box"),
    (mutate_half_min_inward, "half-min"),
    (mutate_half_max_outward, "half-max"),
    (mutate_order_swap, "order-records"),
    (mutate_leaf_count, "pair-coverage"),
    (mutate_prim_node, "prim-node"),
    (mutate_parent_slot, "parent"),
    (mutate_depth, "pair-depth"),
])
def test_validator_reports_each_mutation(mutation, invariant):
    tree, pb, rec = fresh()
    node = mutation(tree)
    with pytest.raises(T.TreeError) as e:
        T.validate(tree, pb, rec)
    assert e.value.invariant == invariant, str(e.value)
    if node is not None:
        assert e.value.node == node, str(e.value)
    assert invariant in str(e.value)


def test_order_swap_is_caught_by_the_boxes_too():
    """Without the scene's records, swapped order entries show as a leaf box that is not its primitives' union."""
    tree, pb, _ = fresh()
    mutate_order_swap(tree)
    with pytest.raises(T.TreeError) as e:
        T.validate(tree, pb)
    assert e.value.invariant == "pair-box"


def test_f32_box_damage_is_caught_without_primitive_boxes():
    """Without primitive boxes an inner child's box is still held to the union of that child's own two boxes."""
    tree, _, rec = fresh()
    i = int(np.nonzero(tree["nodes"]["c"][:, 0] > 0)[0][0])
    tree["nodes"]["f"][i, 3] = ulp_down(tree["nodes"]["f"][i, 3])
    with pytest.raises(T.TreeError) as e:
        T.validate(tree, None, rec)
    assert e.value.invariant == "pair-box" and e.value.node == i


def test_prim_boxes_are_float32_operations():
    g = T.gaussian_rows(np.float32([[0.1, -0.2, 0.3]]), np.float32([[0.01, 0.0, 0.0, 0.0, 0.0, -1.0]]))
    b = T.prim_boxes(g)
    h = np.float32(np.float32(np.float32(3) * np.sqrt(np.float32(0.01))) * np.float32(1.05)) + np.float32(1e-6)
    assert b.dtype == np.float32 and b[0, 0] == np.float32(0.1) - h and b[0, 3] == np.float32(0.1) + h
    assert b[0, 1] == np.float32(-0.2) - np.float32(1e-6)  # zero variance: the 1e-6 pad alone
    assert b[0, 2] == np.float32(0.3) - np.float32(1e-6)   # negative variance clamps to 0


def test_morton_keys_interleave_from_the_high_bit():
    boxes = np.float32([[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 0, 0, 1, 0, 0], [0, 0, 0.5, 0, 0, 0.5]])
    k = T.morton_keys(boxes)
    assert k[0] == 0 and k[1] == (1 << 63) - 1
    assert k[2] == int("100" * 21, 2)
    assert k[3] == 1 << 60  # z = 2^20 of 2^21 cells: its top bit, the lowest of the top triple


# ---- what the GPU scenes rely on ----
def test_chain_scenes_have_31_and_32_levels():
    """The stack-limit scenes: the deepest tree the device builder keeps (kMaxDepth + 1 levels) and the
    shallowest it hands to the host builder, unchanged over twelve decades of variance."""
    L = lim()
    deep = L["max_depth"] + 1
    k_keep, k_fall = T.chain_k_for(deep, L["leaf_max"]), T.chain_k_for(deep + 1, L["leaf_max"])
    assert k_fall == k_keep + 1
    if L["leaf_max"] == 2 and L["max_depth"] == 30:
        assert (k_keep, k_fall) == (23, 24)
    for var in (1e-14, 1e-10, 1e-6, 2.5e-4, 1e-2):
        assert T.chain_levels(k_keep, L["leaf_max"], var) == deep, var
        assert T.chain_levels(k_fall, L["leaf_max"], var) == deep + 1, var
    keys = T.morton_keys(T.prim_boxes(T.chain_gaussians(k_keep)))
    assert sorted(keys[:k_keep], reverse=True) == [1 << (62 - i) for i in range(k_keep)]
    assert keys[k_keep] == (1 << 63) - 1 and set(keys[k_keep + 1:]) == {0}


def test_coincident_scene_has_one_key():
    boxes = T.prim_boxes(T.coincident_gaussians())
    keys = T.morton_keys(boxes)
    assert len(keys) == 256 and set(keys) == {0}
    c = np.float32(0.5) * (boxes[:, 0:3] + boxes[:, 3:6])
    assert np.all(c.max(axis=0) - c.min(axis=0) == 0)  # zero extent on every axis
    assert len(np.unique(boxes, axis=0)) == 256        # ... of boxes that all differ


def test_cluster_scene_has_one_key_per_centre():
    keys = T.morton_keys(T.prim_boxes(T.cluster_gaussians()))
    assert len(set(keys)) == 37
    assert all(keys[i] == keys[i % 37] for i in range(len(keys)))
    order = T.radix_tree(keys, lim()["leaf_max"])["order"]
    # a stable sort keeps the copies of a centre in scene order
    for j in range(0, len(order), 8):
        run = order[j:j + 8].astype(int)
        assert len(set(run % 37)) == 1 and list(run) == sorted(run)
