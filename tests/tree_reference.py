"""Host reference of the trees vr_upload_scene puts on the device, and a validator for what
Device.debug_tree() reads back. numpy and Python integers only.

Reference (a formulation of its own, not the device builder's):
    prim_boxes(gaussians)   gaussian_bounds in float32: mean -+ (3 sqrt(max(d, 0)) * 1.05 + 1e-6)
    morton_keys(boxes)      63-bit Morton code of every box centroid in the centroid bounds
    radix_tree(keys)        stable argsort, then the binary radix tree over the augmented keys
                            (key << 32 | sorted position), built top-down: a range splits at the highest bit
                            in which its first and last augmented keys differ. The radix tree over distinct
                            keys is unique, so Karras's per-node searches must arrive at the same tree.
    assemble(...)           a complete debug_tree()-shaped dict from a radix tree (half nodes, the
                            depth-parity 4-wide collapse, parents, record map, per-axis copies)

validate(tree, prim_boxes=None, records=None) checks every invariant the traversal kernels rely on, for any
builder and any collapse, and returns the measured depth; a violation raises TreeError naming the invariant
and the node.

Levels: the pair tree is a binary tree whose leaves count as nodes. Node 0 is the root (level 1), a child of
a level-L node is on level L + 1, leaves included; a scene that is a single leaf (node 0 holds that leaf and
an empty slot) has one level, an empty scene none.
"""
import bisect

import numpy as np

F32 = np.float32
NODE_DT = np.dtype([("f", "<f4", (12,)), ("c", "<i4", (4,))])
HNODE_DT = np.dtype([("h", "<u2", (12,)), ("c", "<i4", (2,))])
HNODE4_DT = np.dtype([("h", "<u2", (4, 6)), ("c", "<i4", (4,))])
PARENT_MASK = 0x0FFFFFFF  # parent4: node | (slot + 1) << 28
NAN16 = 0x7E00


class TreeError(AssertionError):
    def __init__(self, invariant, node, detail=""):
        super().__init__(f"{invariant}: node {node}" + (f": {detail}" if detail else ""))
        self.invariant = invariant
        self.node = node


def limits():
    """kLeafMax, kMaxDepth and kWideStackMax of the built library (vr_tree_limits)."""
    import ctypes
    from vr_amd import _lib as L
    v = [ctypes.c_int32() for _ in range(3)]
    L.check(L.lib().vr_tree_limits(*[ctypes.byref(x) for x in v]))
    return {"leaf_max": v[0].value, "max_depth": v[1].value, "wide_stack_max": v[2].value}


# ---- leaf refs (vr_internal.h) ----
def make_leaf(first, count):
    r = 0x80000000 | (int(first) << 4) | (int(count) - 1)
    return r - (1 << 32)


def leaf_range(ref):
    r = int(ref) & 0x7FFFFFFF
    return r >> 4, (r & 15) + 1


# ---- reference ----
def prim_boxes(gaussians):
    """(n, 6) float32 boxes [min xyz, max xyz] of Scene.gaussians() rows (mean 0:3, covariance 3:9 as
    xx xy xz yy yz zz): every operation rounded to float32 on its own."""
    g = np.asarray(gaussians, F32)
    d = np.maximum(g[:, [3, 6, 8]], F32(0))
    h = F32(3) * np.sqrt(d)
    h = h * F32(1.05)
    h = h + F32(1e-6)
    assert h.dtype == F32
    return np.concatenate([g[:, 0:3] - h, g[:, 0:3] + h], axis=1).astype(F32)


def morton_keys(boxes):
    """Python-int Morton keys (x, y, z interleaved from the high bit, 21 bits each) of the box centroids."""
    b = np.asarray(boxes, F32)
    c = F32(0.5) * (b[:, 0:3] + b[:, 3:6])
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = hi - lo
    inv = np.where(ext > 0, F32(1) / np.where(ext > 0, ext, F32(1)), F32(0)).astype(F32)
    u = (c - lo) * inv
    u = np.minimum(np.maximum(u, F32(0)), F32(1))
    q = np.minimum(u * F32(2097152.0), F32(2097151.0)).astype(np.int64)  # truncation (all values >= 0)
    keys = []
    for qx, qy, qz in q.tolist():
        k = 0
        for bit in range(20, -1, -1):
            k = (k << 3) | (((qx >> bit) & 1) << 2) | (((qy >> bit) & 1) << 1) | ((qz >> bit) & 1)
        keys.append(k)
    return keys


def radix_tree(keys, leaf_max):
    """The binary radix tree over `keys` (Python ints) in stable sorted order, ranges of <= leaf_max primitives
    as leaves (the root is always a node; at least two keys). Returns a dict: order (sorted position -> index
    into keys), c ((m, 2) child refs: node index or leaf ref), rng ((m, 2, 2) first and count of each child's
    range), level ((m,) node level, root 1) and levels (of the whole tree, leaves included). Nodes are
    numbered in depth-first order, root 0."""
    n = len(keys)
    assert n >= 2
    order = sorted(range(n), key=lambda i: keys[i])  # sorted() is stable
    aug = [(keys[order[j]] << 32) | j for j in range(n)]
    c, rng, level = [], [], []
    todo = [(0, n - 1, 1, -1, 0)]  # first, last, level, parent node, side in it
    levels = 0
    while todo:
        a, b, lv, par, side = todo.pop()
        me = len(c)
        if par >= 0:
            c[par][side] = me
        top = (aug[a] ^ aug[b]).bit_length() - 1  # highest differing bit: every key of the range agrees above it
        # first position of the range whose bit `top` is set
        first_hi = bisect.bisect_left(aug, (aug[b] >> top) << top, a, b + 1)
        kids = [(a, first_hi - 1), (first_hi, b)]
        c.append([0, 0])
        rng.append([[x, y - x + 1] for x, y in kids])
        level.append(lv)
        for s in (1, 0):  # left subtree numbered first
            x, y = kids[s]
            if y - x + 1 <= leaf_max:
                c[me][s] = make_leaf(x, y - x + 1)
                levels = max(levels, lv + 1)
            else:
                todo.append((x, y, lv + 1, me, s))
    return {"order": np.array(order, np.uint32), "c": np.array(c, np.int64).astype(np.int32),
            "rng": np.array(rng, np.int64), "level": np.array(level, np.int32), "levels": levels}


def range_boxes(sorted_boxes, rng):
    """(m, 2, 6) float32: the union of sorted_boxes over each child range of radix_tree's rng."""
    out = np.empty(rng.shape[:2] + (6,), F32)
    for i in range(rng.shape[0]):
        for s in range(2):
            a, k = int(rng[i, s, 0]), int(rng[i, s, 1])
            out[i, s, 0:3] = sorted_boxes[a:a + k, 0:3].min(axis=0)
            out[i, s, 3:6] = sorted_boxes[a:a + k, 3:6].max(axis=0)
    return out


def outward_half(u):
    """Half bits of float64 values u (..., 6) [min xyz, max xyz] rounded outward: to nearest, then one step
    down (minima) or up (maxima) where that fell inside."""
    with np.errstate(over="ignore"):
        h = u.astype(np.float16)
    dn = np.nextafter(h, np.float16(-np.inf))
    up = np.nextafter(h, np.float16(np.inf))
    is_min = np.arange(6) < 3
    fix_min = is_min & (h.astype(np.float64) > u)
    fix_max = ~is_min & (h.astype(np.float64) < u)
    return np.where(fix_min, dn, np.where(fix_max, up, h)).view(np.uint16)


def half_bounds(f, hc, hs):
    """Outward-rounded half bits of float32 bounds f (..., 6) in the normalisation u = (x - hc) * hs
    evaluated in float64; infinities stay infinities."""
    f = np.asarray(f, F32)
    u = (f.astype(np.float64) - np.tile(np.asarray(hc, np.float64), 2)) * np.float64(hs)
    return outward_half(np.where(np.isinf(f), f.astype(np.float64), u))


def ellipsoid_boxes(records):
    """(positive definite (n,), lo (n, 3), hi (n, 3)) in float64: the exact box mean -+ 3 sqrt((M^-1)_kk) of
    x^T M x <= 9 from each record's M; infinite where M is not positive definite."""
    rec = np.asarray(records, np.float64)
    n = len(rec)
    M = np.empty((n, 3, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = (rec[:, k] for k in (4, 5, 6, 7, 8, 9))
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    pd = np.linalg.eigvalsh(M).min(axis=1) > 0 if n else np.zeros(0, bool)
    ext = np.full((n, 3), np.inf)
    if pd.any():
        ext[pd] = 3.0 * np.sqrt(np.diagonal(np.linalg.inv(M[pd]), axis1=1, axis2=2))
    return pd, rec[:, 0:3] - ext, rec[:, 0:3] + ext


def soa_words(h4):
    """(n, 16) uint32 per-axis copy of HNode4 records: words 4a .. 4a+3 hold axis a's bounds as f16 pairs
    {min of children 0, 1}, {min 2, 3}, {max 0, 1}, {max 2, 3}; words 12-15 the child refs."""
    h = h4["h"].astype(np.uint32)
    w = np.zeros((len(h4), 16), np.uint32)
    for a in range(3):
        w[:, 4 * a + 0] = h[:, 0, a] | (h[:, 1, a] << 16)
        w[:, 4 * a + 1] = h[:, 2, a] | (h[:, 3, a] << 16)
        w[:, 4 * a + 2] = h[:, 0, 3 + a] | (h[:, 1, 3 + a] << 16)
        w[:, 4 * a + 3] = h[:, 2, 3 + a] | (h[:, 3, 3 + a] << 16)
    w[:, 12:16] = h4["c"].view(np.uint32)
    return w


def scene_box(boxes):
    b = np.asarray(boxes, F32)
    return b[:, 0:3].min(axis=0), b[:, 3:6].max(axis=0)


def half_normalisation(bmin, bmax):
    hc = (F32(0.5) * (bmin + bmax)).astype(F32)
    half = float(np.max(0.5 * (bmax.astype(np.float64) - bmin.astype(np.float64))))
    return hc, F32(1.0 / half)


def assemble(gaussians, records, lim):
    """A complete tree dict (the shape of Device.debug_tree()) for `gaussians` from the reference alone: the radix
    tree of their Morton keys, half nodes, a 4-wide collapse of the nodes on odd levels (each holds its
    children's children), parents, record map and per-axis copies."""
    pb = prim_boxes(gaussians)
    rt = radix_tree(morton_keys(pb), lim["leaf_max"])
    order = rt["order"]
    m = len(rt["c"])
    nodes = np.zeros(m, NODE_DT)
    nodes["f"] = range_boxes(pb[order], rt["rng"]).reshape(m, 12)
    nodes["c"][:, 0:2] = rt["c"]
    bmin, bmax = scene_box(pb)
    hc, hs = half_normalisation(bmin, bmax)
    hnodes = np.zeros(m, HNODE_DT)
    hnodes["h"] = half_bounds(nodes["f"].reshape(m, 2, 6), hc, hs).reshape(m, 12)
    hnodes["c"] = rt["c"]
    # 4-wide: pair nodes on odd levels, numbered in pair-node order
    wide_of = {int(i): k for k, i in enumerate(np.nonzero(rt["level"] & 1)[0])}
    h4 = np.zeros(len(wide_of), HNODE4_DT)
    h4["h"][:] = NAN16
    slot_rng = np.zeros((len(wide_of), 4, 2), np.int64)  # first, count of every slot's primitives
    for i, k in wide_of.items():
        slot = 0
        for s in range(2):
            r = int(hnodes["c"][i, s])
            if r < 0:
                h4["h"][k, slot] = hnodes["h"][i, 6 * s:6 * s + 6]
                h4["c"][k, slot] = r
                slot_rng[k, slot] = rt["rng"][i, s]
                slot += 1
                continue
            for s2 in range(2):
                r2 = int(hnodes["c"][r, s2])
                h4["h"][k, slot] = hnodes["h"][r, 6 * s2:6 * s2 + 6]
                h4["c"][k, slot] = r2 if r2 < 0 else wide_of[r2]
                slot_rng[k, slot] = rt["rng"][r, s2]
                slot += 1
    # the tight refit: the exact ellipsoid boxes' union per slot, rounded outward, kept where tighter than the shared box
    sorted_rec = np.asarray(records, F32)[order]
    _, elo, ehi = ellipsoid_boxes(sorted_rec)
    t4 = h4.copy()
    for k in range(len(h4)):
        for slot in range(4):
            if h4["c"][k, slot] == 0:
                continue
            a, cnt = slot_rng[k, slot]
            x = np.concatenate([elo[a:a + cnt].min(axis=0), ehi[a:a + cnt].max(axis=0)])
            tight = outward_half((x - np.tile(hc.astype(np.float64), 2)) * np.float64(hs))
            tv, sv = tight.view(np.float16).astype(np.float64), h4["h"][k, slot].view(np.float16).astype(np.float64)
            keep = np.where(np.arange(6) < 3, tv > sv, tv < sv)
            t4["h"][k, slot] = np.where(keep, tight, h4["h"][k, slot])
    n = len(order)
    parent4 = np.full(len(h4), -1, np.int32)
    prim_node4 = np.full(n, -1, np.int32)
    for k in range(len(h4)):
        for s in range(4):
            r = int(h4["c"][k, s])
            if r > 0:
                parent4[r] = k | ((s + 1) << 28)
            elif r < 0:
                a, cnt = leaf_range(r)
                prim_node4[a:a + cnt] = k
    info = {"num_prims": n, "num_nodes": m, "num_nodes4": len(h4), "bvh_depth": rt["levels"], "built_on_device": True,
            "wrec_pd": True, "hn_center": hc, "hn_scale": hs, "bounds_min": bmin, "bounds_max": bmax, **lim}
    return {"order": order, "records": sorted_rec, "nodes": nodes, "hnodes": hnodes, "hnodes4": h4,
            "hnodes4s": t4, "hnodes4w": soa_words(h4), "hnodes4t": soa_words(t4),
            "parent4": parent4, "prim_node4": prim_node4, "info": info}


# ---- validator ----
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _walk_pair(nodes, n, info):
    """Depth-first walk of the pair tree from node 0. Returns (reached node list in visiting order, level of each,
    leaves as (node, side, first, count, level), measured levels)."""
    m = len(nodes)
    c = nodes["c"]
    if m == 0:
        raise TreeError("pair-root", 0, "no nodes")
    leaf_max = info["leaf_max"]
    seen = np.zeros(m, bool)
    covered = np.zeros(n, np.int32)
    reached, level, leaves = [], {}, []
    todo = [(0, 1)]
    seen[0] = True
    while todo:
        i, lv = todo.pop()
        reached.append(i)
        level[i] = lv
        for s in (1, 0):
            r = int(c[i, s])
            if r == 0:
                if i != 0:
                    raise TreeError("pair-node-twice", i, f"side {s} references node 0")
                if not (np.all(np.isposinf(nodes["f"][i, 6 * s:6 * s + 3])) and np.all(np.isneginf(nodes["f"][i, 6 * s + 3:6 * s + 6]))):
                    raise TreeError("pair-empty", i, f"empty side {s} without an inverted box")
                continue
            if r < 0:
                a, k = leaf_range(r)
                if not 1 <= k <= leaf_max:
                    raise TreeError("pair-leaf-count", i, f"side {s}: {k} primitives, kLeafMax {leaf_max}")
                if a + k > n:
                    raise TreeError("pair-coverage", i, f"side {s}: leaf [{a}, {a + k}) past {n} primitives")
                covered[a:a + k] += 1
                leaves.append((i, s, a, k, lv + 1))
                continue
            if r >= m:
                raise TreeError("pair-ref", i, f"side {s}: node {r} of {m}")
            if seen[r]:
                raise TreeError("pair-node-twice", i, f"side {s}: node {r} is referenced twice")
            seen[r] = True
            todo.append((r, lv + 1))
    if n and not np.all(covered == 1):
        j = int(np.nonzero(covered != 1)[0][0])
        raise TreeError("pair-coverage", 0, f"primitive position {j} lies in {int(covered[j])} leaves")
    if n == 0:
        levels = 0
    elif len(leaves) == 1 and (int(c[0, 0]) == 0 or int(c[0, 1]) == 0):
        levels = 1  # the scene is one leaf
    else:
        levels = max(lf[4] for lf in leaves)
    return reached, level, leaves, levels


def validate(tree, prim_boxes=None, records=None):
    """Checks a debug_tree() dict; returns the measured number of levels. prim_boxes: the scene's primitive
    boxes in scene order (every child box must then be the union of its primitives' boxes bit for bit; without
    them an inner child's box must be the union of that child's own two boxes). records: Scene.records() in
    scene order (the records read back must be those, in tree order)."""
    info = tree["info"]
    n = int(info["num_prims"])
    order, nodes = tree["order"], tree["nodes"]

    # ---- order ----
    if len(order) != n or not np.array_equal(np.sort(order), np.arange(n, dtype=order.dtype)):
        raise TreeError("order-permutation", 0, "order is not a permutation of the scene indices")
    if records is not None:
        want = np.asarray(records, F32)[order]
        if tree["records"].shape != want.shape or not np.array_equal(_bits(tree["records"]), _bits(want)):
            bad = np.nonzero(np.any(_bits(tree["records"]) != _bits(want), axis=1))[0] if tree["records"].shape == want.shape else [0]
            raise TreeError("order-records", int(bad[0]), "the record at this position is not the scene's record order[position]")

    # ---- pair tree ----
    if len(nodes) != info["num_nodes"]:
        raise TreeError("pair-root", 0, f"{len(nodes)} nodes read back, num_nodes {info['num_nodes']}")
    reached, level, leaves, levels = _walk_pair(nodes, n, info)
    f = nodes["f"].reshape(-1, 2, 6)
    fb = _bits(f)
    span = {}  # node -> (first, count) of its subtree, filled bottom-up
    pair_child = {}  # (first, count) -> (node, side)
    sb = None if prim_boxes is None else np.asarray(prim_boxes, F32)[order]
    true_box = {}  # node -> union of its primitives' boxes (with prim_boxes)
    for i in reversed(reached):
        lo_hi, boxes = [], []
        for s in range(2):
            r = int(nodes["c"][i, s])
            if r == 0:
                continue
            if r < 0:
                a, k = leaf_range(r)
                want = None if sb is None else np.concatenate([sb[a:a + k, 0:3].min(axis=0), sb[a:a + k, 3:6].max(axis=0)])
            else:
                a, k = span[r]
                if sb is None:
                    want = np.concatenate([np.minimum(f[r, 0, 0:3], f[r, 1, 0:3]), np.maximum(f[r, 0, 3:6], f[r, 1, 3:6])])
                else:
                    want = true_box[r]
            if want is not None:
                if not np.array_equal(_bits(want.astype(F32)), fb[i, s]):
                    k6 = int(np.nonzero(_bits(want.astype(F32)) != fb[i, s])[0][0])
                    raise TreeError("pair-box", i, f"side {s} bound {k6}: stored {f[i, s, k6]!r}, union {want[k6]!r}")
                boxes.append(want)
            lo_hi.append((a, k))
            if (a, k) in pair_child:
                raise TreeError("pair-coverage", i, f"side {s}: range {(a, k)} is covered twice")
            pair_child[(a, k)] = (i, s)
        if len(lo_hi) == 2:
            (a0, k0), (a1, k1) = sorted(lo_hi)
            if a0 + k0 != a1:
                raise TreeError("pair-coverage", i, f"children ranges {(a0, k0)} and {(a1, k1)} are not adjacent")
            span[i] = (a0, k0 + k1)
        elif lo_hi:
            span[i] = lo_hi[0]
        if sb is not None and boxes:
            bx = np.stack(boxes)
            true_box[i] = np.concatenate([bx[:, 0:3].min(axis=0), bx[:, 3:6].max(axis=0)])
    if levels != info["bvh_depth"]:
        deepest = max(leaves, key=lambda lf: lf[4])[0] if leaves else 0
        raise TreeError("pair-depth", deepest, f"{levels} levels, bvh_depth {info['bvh_depth']}")
    if info["bvh_depth"] > info["max_depth"] + 1:
        raise TreeError("pair-depth-bound", 0, f"bvh_depth {info['bvh_depth']} > kMaxDepth + 1 = {info['max_depth'] + 1}")

    # ---- half nodes ----
    hn = tree["hnodes"]
    if len(hn) == 0:
        for name in ("hnodes4", "hnodes4s", "hnodes4w", "hnodes4t", "parent4"):
            if len(tree[name]):
                raise TreeError("half-absent", 0, f"{name} without half nodes")
        return levels
    if len(hn) != len(nodes):
        raise TreeError("half-refs", 0, f"{len(hn)} half nodes for {len(nodes)} nodes")
    ridx = np.array(sorted(reached))
    if not np.array_equal(hn["c"][ridx], nodes["c"][ridx, 0:2]):
        bad = ridx[np.nonzero(np.any(hn["c"][ridx] != nodes["c"][ridx, 0:2], axis=1))[0][0]]
        raise TreeError("half-refs", int(bad), "half node refs differ from the float32 node's")
    hc, hs = np.asarray(info["hn_center"], np.float64), np.float64(info["hn_scale"])
    x = f[ridx]                                            # (r, 2, 6) float32
    hv16 = hn["h"][ridx].reshape(-1, 2, 6).view(np.float16)
    hv = hv16.astype(np.float64)
    u = (x.astype(np.float64) - np.tile(hc, 2)) * hs
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        inward_up = np.nextafter(hv16, np.float16(np.inf)).astype(np.float64)    # the next half above
        inward_dn = np.nextafter(hv16, np.float16(-np.inf)).astype(np.float64)   # the next half below
        is_min = np.broadcast_to(np.arange(6) < 3, x.shape)
        ok_min = np.where(fin, (hv <= u) & (inward_up > u), hv == x.astype(np.float64))
        ok_max = np.where(fin, (hv >= u) & (inward_dn < u), hv == x.astype(np.float64))
    for name, bad in (("half-min", is_min & ~ok_min), ("half-max", ~is_min & ~ok_max)):
        if bad.any():
            r, s, k = [int(v[0]) for v in np.nonzero(bad)]
            raise TreeError(name, int(ridx[r]), f"side {s} bound {k}: half {hv[r, s, k]!r} for u = {u[r, s, k]!r}")

    # ---- 4-wide tree ----
    h4 = tree["hnodes4"]
    n4 = len(h4)
    if n4 != info["num_nodes4"] or n4 == 0:
        raise TreeError("wide-root", 0, f"{n4} 4-wide nodes read back, num_nodes4 {info['num_nodes4']}")
    refs = np.zeros(n4, np.int32)
    order4, lvl4 = [], {}
    holder = {}  # node -> (parent, slot)
    todo = [(0, 1)]
    wide_leaves = []
    while todo:
        i, lv = todo.pop()
        order4.append(i)
        lvl4[i] = lv
        for s in range(4):
            r = int(h4["c"][i, s])
            if r == 0:
                if not np.all(np.isnan(h4["h"][i, s].view(np.float16))):
                    raise TreeError("wide-empty", i, f"empty slot {s} with a box that is not NaN")
            elif r < 0:
                wide_leaves.append((r, i, s))
            else:
                if r >= n4:
                    raise TreeError("wide-ref", i, f"slot {s}: node {r} of {n4}")
                refs[r] += 1
                if refs[r] > 1:
                    raise TreeError("wide-ref", i, f"slot {s}: node {r} is referenced twice")
                holder[r] = (i, s)
                todo.append((r, lv + 1))
    if not np.all(refs[1:] == 1):
        raise TreeError("wide-ref", int(np.nonzero(refs[1:] != 1)[0][0]) + 1, "node is never referenced")
    pair_leaf_refs = sorted(int(nodes["c"][i, s]) for i, s, _, _, _ in leaves)
    if sorted(r for r, _, _ in wide_leaves) != pair_leaf_refs:
        missing = set(pair_leaf_refs) ^ set(r for r, _, _ in wide_leaves)
        raise TreeError("wide-leaves", 0, f"leaves differ from the pair tree's, e.g. {[leaf_range(r) for r in sorted(missing)[:3]]}")
    span4 = {}
    for i in reversed(order4):
        parts = []
        for s in range(4):
            r = int(h4["c"][i, s])
            if r == 0:
                continue
            a, k = leaf_range(r) if r < 0 else span4[r]
            parts.append((a, k))
            src = pair_child.get((a, k))
            if src is None:
                raise TreeError("wide-box", i, f"slot {s}: no pair-tree child covers primitives [{a}, {a + k})")
            pi, ps = src
            if not np.array_equal(h4["h"][i, s], hn["h"][pi, 6 * ps:6 * ps + 6]):
                raise TreeError("wide-box", i, f"slot {s}: box differs from half node {pi} side {ps}")
        parts.sort()
        for (a0, k0), (a1, _) in zip(parts, parts[1:]):
            if a0 + k0 != a1:
                raise TreeError("wide-box", i, "slots do not cover one contiguous range")
        span4[i] = (parts[0][0], sum(k for _, k in parts)) if parts else (0, 0)
    need = 3 * max(lvl4.values())
    if need > info["wide_stack_max"]:
        raise TreeError("wide-stack", 0, f"{max(lvl4.values())} levels need {need} stack entries, kWideStackMax {info['wide_stack_max']}")

    # ---- parents and record map ----
    p4, pn4 = tree["parent4"], tree["prim_node4"]
    if len(p4) != n4 or int(p4[0]) != -1:
        raise TreeError("parent-root", 0, "parent4[0] is not -1")
    for r in range(1, n4):
        par, slot = int(p4[r]) & PARENT_MASK, (int(p4[r]) >> 28) - 1
        if int(p4[r]) < 0 or (par, slot) != holder[r]:
            raise TreeError("parent", r, f"parent4 names node {par} slot {slot}, referenced from {holder[r]}")
    if len(pn4) != n:
        raise TreeError("prim-node", 0, f"{len(pn4)} entries for {n} records")
    for r, i, s in wide_leaves:
        a, k = leaf_range(r)
        if not np.all(pn4[a:a + k] == i):
            j = a + int(np.nonzero(pn4[a:a + k] != i)[0][0])
            raise TreeError("prim-node", i, f"prim_node4[{j}] = {int(pn4[j])}, its leaf is in node {i}")

    # ---- per-axis copies ----
    for name, src in (("hnodes4w", h4), ("hnodes4t", tree["hnodes4s"])):
        got = tree[name]
        if name == "hnodes4t" and len(got) == 0:
            continue
        want = soa_words(src)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = int(np.nonzero(np.any(got != want, axis=1))[0][0]) if got.shape == want.shape else 0
            raise TreeError("per-axis", bad, f"{name} is not the per-axis rearrangement of its tree")

    # ---- tight tree ----
    t4 = tree["hnodes4s"]
    if len(t4) == 0:
        return levels
    if len(t4) != n4 or not np.array_equal(t4["c"], h4["c"]):
        raise TreeError("tight-refs", 0, "the tight tree's refs differ from the shared tree's")
    pd, lo, hi = ellipsoid_boxes(tree["records"])
    ulo, uhi = (lo - hc) * hs, (hi - hc) * hs  # the ellipsoids' exact boxes in the half nodes' normalisation
    tv, sv = t4["h"].view(np.float16).astype(np.float64), h4["h"].view(np.float16).astype(np.float64)
    for i in order4:
        for s in range(4):
            r = int(h4["c"][i, s])
            if r == 0:
                if not np.array_equal(t4["h"][i, s], h4["h"][i, s]):
                    raise TreeError("tight-outside", i, f"empty slot {s} changed")
                continue
            if np.any(tv[i, s, 0:3] < sv[i, s, 0:3]) or np.any(tv[i, s, 3:6] > sv[i, s, 3:6]):
                raise TreeError("tight-outside", i, f"slot {s}: a bound lies outside the shared tree's")
            a, k = leaf_range(r) if r < 0 else span4[r]
            if not pd[a:a + k].all():
                if not np.array_equal(t4["h"][i, s], h4["h"][i, s]):
                    raise TreeError("tight-nonpd", i, f"slot {s} holds a record that is not positive definite and was refit")
                continue
            if np.any(tv[i, s, 0:3] > ulo[a:a + k].min(axis=0)) or np.any(tv[i, s, 3:6] < uhi[a:a + k].max(axis=0)):
                raise TreeError("tight-contain", i, f"slot {s}: an ellipsoid of records [{a}, {a + k}) reaches outside the box")
    return levels


def same_pair_tree(tree, rt, sorted_boxes):
    """Lockstep walk of a read-back pair tree and radix_tree's from their roots: same leaf ranges and
    bit-equal child boxes, whatever the node numbering. Raises TreeError("lockstep", node)."""
    want = range_boxes(sorted_boxes, rt["rng"])
    nodes = tree["nodes"]
    todo = [(0, 0)]
    visited = 0
    while todo:
        i, j = todo.pop()
        visited += 1
        for s in range(2):
            a, b = int(nodes["c"][i, s]), int(rt["c"][j, s])
            if (a < 0) != (b < 0) or (a < 0 and a != b):
                raise TreeError("lockstep", i, f"side {s}: ref {a}, the reference has {b} (its node {j})")
            if not np.array_equal(_bits(nodes["f"][i, 6 * s:6 * s + 6]), _bits(want[j, s])):
                raise TreeError("lockstep", i, f"side {s}: box differs from the reference's node {j}")
            if a > 0:
                todo.append((a, b))
            elif a == 0:
                raise TreeError("lockstep", i, f"side {s} is empty")
    if visited != len(rt["c"]):
        raise TreeError("lockstep", 0, f"{visited} nodes walked, the reference has {len(rt['c'])}")
    return visited


def check_against_reference(tree, pb):
    """The device builder's order and pair tree are the reference's: stable argsort, unique radix tree."""
    rt = radix_tree(morton_keys(pb), tree["info"]["leaf_max"])
    assert np.array_equal(tree["order"], rt["order"])
    assert same_pair_tree(tree, rt, pb[rt["order"]]) == len(rt["c"])
    assert tree["info"]["bvh_depth"] == rt["levels"]


# ---- the scenes both test files use ----
def rotated_cov(rng, n, lo=0.02, hi=0.12):
    """(n, 6) anisotropic covariances R diag(s^2) R^T with random rotations, as xx xy xz yy yz zz."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    s2 = rng.uniform(lo, hi, (n, 3)) ** 2
    C = np.einsum("nij,nj,nkj->nik", R, s2, R)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], -1).astype(F32)


def gaussian_rows(mean, cov6):
    """(n, 14) rows in Scene.gaussians() layout for prim_boxes (density, albedo, emission left 0)."""
    g = np.zeros((len(mean), 14), F32)
    g[:, 0:3] = mean
    g[:, 3:9] = cov6
    return g


def coincident_gaussians(n=256, seed=21):
    """n Gaussians of different covariances with one mean, the origin: every box is symmetric about it, so
    every centroid 0.5f * (lo + hi) is exactly 0."""
    return gaussian_rows(np.zeros((n, 3), F32), rotated_cov(np.random.default_rng(seed), n))


def cluster_gaussians(centres=37, copies=8, seed=22):
    """centres x copies Gaussians, copy c of every centre before copy c + 1 of any (interleaved in scene
    order). The copies of a centre share its covariance, so their box centroids coincide bit for bit."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1.0, 1.0, (centres, 3)).astype(F32)
    return gaussian_rows(np.tile(mean, (copies, 1)), np.tile(rotated_cov(rng, centres), (copies, 1)))


def chain_means(k):
    """The stack-limit scene's means: one at the cell centre of each of the first k single-bit Morton codes
    (bit b = 62 - i on axis 2 - b mod 3, coordinate (2^(b // 3) + 0.5) / 2^21, the other axes in cell 0), one at
    (1, 1, 1), and 256 inside cell 0, the first of them at the origin."""
    cell = 1.0 / 2097152.0
    m = []
    for i in range(k):
        b = 62 - i
        p = [0.5 * cell] * 3
        p[2 - b % 3] = (2.0 ** (b // 3) + 0.5) * cell
        m.append(p)
    m.append([1.0, 1.0, 1.0])
    inside = np.random.default_rng(62).uniform(0.1, 0.9, (256, 3)) * cell
    inside[0] = 0.0
    return np.concatenate([np.array(m), inside]).astype(F32)


def chain_gaussians(k, variance=2.5e-4):
    mean = chain_means(k)
    cov = np.zeros((len(mean), 6), F32)
    cov[:, [0, 3, 5]] = F32(variance)
    return gaussian_rows(mean, cov)


def chain_levels(k, leaf_max, variance=2.5e-4):
    return radix_tree(morton_keys(prim_boxes(chain_gaussians(k, variance))), leaf_max)["levels"]


def chain_k_for(levels, leaf_max):
    """The k whose chain scene has exactly `levels` levels."""
    for k in range(1, 63):
        if chain_levels(k, leaf_max) == levels:
            return k
    raise ValueError(f"no chain scene with {levels} levels")
