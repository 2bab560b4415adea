"""A scene that drives every walk of the 4-wide tree to its stack limit, and host simulators of those walks'
stacks. numpy, Python integers and fractions only; the library is needed for tree_reference.limits() alone.

comb_gaussians(leaf_max)   a "comb": a spine of child-pair nodes towards the cloud's minimum corner whose sibling
                           at every level is itself an inner node, so that a walk that descends the spine first
                           leaves three entries on its stack per 4-wide level. With isotropic Gaussians far
                           wider than the cloud every box is about as large as the scene: a ray through the cloud
                           hits every child of every node, and a point in the cloud lies in all of them.
walk_wide / walk_sigma / walk_secondary
                           the stacks of traverse_wide and WideWalk::node_step (vr_march.h, vr_walk.h), of
                           query_sigma_kernel's containment walk (vr_query.hip) and of sec_node4v
                           (vr_gauss_secondary.hip) on a tree dict (tree_reference.assemble's or
                           Device.debug_tree()'s), in the kernels' own float32 arithmetic.
rays(...)                  the ray families of the tests.

Arithmetic. wide_slab's constants are float32 operations rounded one by one (numpy float32; the reciprocal is
correctly rounded, as __frcp_rn is). fmaf(bound, 1/d, -o/d) is exact: bound is a half, so the product has at most
35 significant bits and is exact in float64; the sum is taken in float64 with its rounding error (TwoSum), and
where that error is not zero the sum is redone in rational arithmetic and rounded to float32 once.
The direction is normalised as make_ray does (dot3, sqrtf, three divisions) without contraction of the dot
product; a last-bit difference in it cannot change a result below: an exact tie counted here is one of equal
half bounds on the axis that decides both keys (so both keys move together), and every other decision holds
with the margin the simulators report.
"""
from fractions import Fraction

import numpy as np

import tree_reference as T

F32 = np.float32
K_TPAD = F32(1e-5)   # kTPad, vr_dev_common.h
WW_STACK = 14        # VR_WW_STACK, vr_gauss_secondary.hip:37 (not exported by the library)
CENTRE = np.array([0.25, -0.5, 0.125])
EXTENT = 0.05
SIGMA = 0.3
PLAN = "EE" + 10 * "F"  # the spine's 4-wide levels: two with leaf siblings (E), then ten with inner siblings (F)
STRETCH = 5          # the centroid bounds are 2^STRETCH comb extents long in x
BALLAST_SIGMA = 0.009


# ---- the scene ----
def _deinterleave(key):
    q = [0, 0, 0]
    for bit in range(62, -1, -1):
        if (key >> bit) & 1:
            q[2 - bit % 3] |= 1 << (bit // 3)
    return q


def comb_keys(leaf_max, plan=PLAN, stretch=STRETCH, ballast=None):
    """(Morton keys of the comb, of the ballast, the lowest key bit the comb uses).

    The device builder takes scenes of 256 Gaussians or more, and at most 120 Gaussians may overlap a point (the
    free-flight rows hold 128). So the scene is the comb, which fills the cell [0, 2^-stretch) x [0, 1) x [0, 1)
    of the centroid bounds, and a ballast of narrower Gaussians in the half x >= 1/2 (key bit 62), spread over
    8 more bits, most of them x's: the root splits the two, and the comb's keys use every bit but x's first `stretch`.
    With b(p) the p-th usable bit from the top, the spine node on pair level l >= 2 splits on b(l - 2):
      level 2:            its sibling is one leaf of one key
      early 4-wide level: an inner node of a 1-leaf and a leaf_max-leaf, then a 1-leaf     (3 leaves, 0 pushes)
      full 4-wide level:  an inner node of two ranges of leaf_max + 1, then leaf_max + 1   (0 leaves, 3 pushes)
      "T" level:          an inner node of a 1-leaf and leaf_max + 1, then leaf_max + 1    (1 leaf, 2 pushes)
    in the order of `plan` (E, F, T), and the spine ends in leaf_max + 1 keys, one of them 0."""
    usable = [b for b in range(61, -1, -1) if not (b % 3 == 2 and b // 3 >= 21 - stretch)]
    jb = int(leaf_max).bit_length()  # bits that number leaf_max + 1 keys
    keys, lowest = [], [0]

    def number(j, pos):  # j in jb bits from position pos, most significant first
        k = 0
        for i in range(jb):
            if (j >> (jb - 1 - i)) & 1:
                k |= 1 << usable[pos + i]
        lowest[0] = max(lowest[0], pos + jb - 1)
        return k

    def group(pos, counts):
        if len(counts) == 1:
            keys.extend((1 << usable[pos]) | number(j, pos + 1) for j in range(counts[0]))
        else:
            for h, cnt in enumerate(counts):
                keys.extend((1 << usable[pos]) | (h << usable[pos + 1]) | number(j, pos + 2) for j in range(cnt))

    group(0, (1,))
    level = 3
    for kind in plan:
        if kind == "E":
            group(level - 2, (1, leaf_max))
            group(level - 1, (1,))
        elif kind == "T":
            group(level - 2, (1, leaf_max + 1))
            group(level - 1, (leaf_max + 1,))
        else:
            group(level - 2, (leaf_max + 1, leaf_max + 1))
            group(level - 1, (leaf_max + 1,))
        level += 2
    keys.extend(number(j, level - 2) for j in range(leaf_max + 1))
    if ballast is None:
        ballast = max(0, 256 - len(keys))
    assert ballast <= 256
    # (the index's low five bits go to x, so that the ballast is a thin row along x: few of it at any one point)
    spread = [59, 56, 53, 50, 47, 58, 57, 55]
    extra = [(1 << 62) | sum(((i >> k) & 1) << b for k, b in enumerate(spread)) for i in range(ballast)]
    if extra:
        extra[-1] = (1 << 63) - 1  # the maximum corner
    return keys, extra, usable[lowest[0]]


def comb_gaussians(leaf_max, mirrored=False, plan=PLAN, centre=CENTRE, extent=EXTENT, sigma=SIGMA,
                   stretch=STRETCH, ballast_sigma=BALLAST_SIGMA):
    """(n, 14) rows in Scene.gaussians() layout (density, albedo and emission 0): the comb's Gaussians first.
    Every key sits in the middle of the coarsest Morton cell that tells it from the others (the float32 box
    centroids move it by a small part of that cell), except key 0 at the minimum corner and the ballast's last
    key at the maximum corner: they pin the centroid bounds the device normalises by. The comb is a cube of
    `extent` around `centre`; the ballast lies 2^(stretch - 1) to 2^stretch extents along +x, clear of every ray
    through the comb whose direction components are all >= 0.3 (comb_count() tells the two apart).
    mirrored: the same scene reflected through `centre` (the spine towards the high keys and the last slot)."""
    keys, extra, low = comb_keys(leaf_max, plan, stretch)
    assert low // 3 >= 6, "the comb needs more Morton bits than the centroids' float32 rounding leaves"
    mid = 1 << (low // 3 - 1)  # half a coarse cell on every axis
    allk = keys + extra
    P = np.array([[(q | mid) / 2097152.0 for q in _deinterleave(k)] for k in allk])
    P[allk.index(0)] = 0.0
    if extra:
        P[len(allk) - 1] = 1.0
    P[:, 0] *= 2.0 ** stretch  # in units of the comb's extent
    if mirrored:
        P = 1.0 - P
    assert len(keys) <= 120, f"{len(keys)} Gaussians overlap: more than the free-flight rows hold (leaf_max {leaf_max})"
    cov = np.zeros((len(P), 6), F32)
    cov[:len(keys), [0, 3, 5]] = F32(sigma * sigma)
    cov[len(keys):, [0, 3, 5]] = F32(ballast_sigma * ballast_sigma)
    return T.gaussian_rows(np.asarray(centre) + extent * (P - 0.5), cov)


def comb_count(leaf_max, plan=PLAN):
    """The comb's own Gaussians (the first rows of comb_gaussians)."""
    return len(comb_keys(leaf_max, plan)[0])


# ---- exact float32 pieces ----
def _round32(fr):
    """A Fraction rounded to the nearest float32, ties to even (normal range)."""
    if fr == 0:
        return 0.0
    s = -1 if fr < 0 else 1
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    q = Fraction(2) ** (e - 23)
    n = fr / q
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (lo & 1)):
        lo += 1
    return s * float(lo * q)


def fma32(a, b, c):
    """fmaf(a, b, c) of float64 arrays holding a half, a float32 and a float32: rounded once."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        out = s.astype(F32).astype(np.float64)
    bad = np.isfinite(s) & (err != 0.0)
    if bad.any():
        pb, cb = np.broadcast_to(p, s.shape), np.broadcast_to(c, s.shape)
        for idx in zip(*np.nonzero(bad)):
            out[idx] = _round32(Fraction(float(pb[idx])) + Fraction(float(cb[idx])))
    return out


def normalise(d):
    """make_ray's direction in float32."""
    d = np.asarray(d, F32)
    s = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    r = np.sqrt(s)
    return (d / r[:, None]).astype(F32)


def decode(h4):
    """(n4, 4, 6) float64 bounds of HNode4 records (min xyz, max xyz per slot; NaN in empty slots)."""
    return h4["h"].view(np.float16).astype(np.float64)


def slabs(tree, origins, directions, which="hnodes4", unit=False):
    """wide_slab and the slab distances of every (ray, node, slot): a dict with tn, tf ((rays, n4, 4, 3): the
    near and far bound's distance per axis), tmin, tmax ((rays, n4, 4)), near ((rays, n4, 4, 3): the near
    bound's half value) and refs (n4, 4)."""
    info = tree["info"]
    hc, hs = np.asarray(info["hn_center"], F32), F32(info["hn_scale"])
    o = np.asarray(origins, F32)
    d = np.asarray(directions, F32) if unit else normalise(directions)
    on = ((o - hc) * hs).astype(F32)
    dd = (d * hs).astype(F32)
    dd = np.where(np.abs(dd) > F32(1e-30), dd, np.copysign(F32(1e-30), dd)).astype(F32)
    inv = (F32(1) / dd).astype(F32)
    oi = (on * inv).astype(F32)
    b = decode(tree[which])                                 # (n4, 4, 6)
    neg = (inv < 0)[:, None, None, :]                       # (rays, 1, 1, 3)
    near = np.where(neg, b[None, :, :, 3:6], b[None, :, :, 0:3])
    far = np.where(neg, b[None, :, :, 0:3], b[None, :, :, 3:6])
    i64, o64 = inv.astype(np.float64)[:, None, None, :], -oi.astype(np.float64)[:, None, None, :]
    tn, tf = fma32(near, i64, o64), fma32(far, i64, o64)
    with np.errstate(invalid="ignore"):
        # fmaxf / fminf chains from axis 0: a NaN (empty slot) stays out of the way of nothing that is used
        tmin = np.fmax(np.fmax(tn[..., 0], tn[..., 1]), tn[..., 2])
        tmax = np.fmin(np.fmin(tf[..., 0], tf[..., 1]), tf[..., 2])
    return {"tn": tn, "tf": tf, "tmin": tmin, "tmax": tmax, "near": near, "refs": tree[which]["c"].astype(np.int64),
            "d": d}


def prune_lim(tmax):
    """shadow_prune_lim in float32 (with or without contraction it differs by an ulp of a bound no comb ray is near)."""
    t = F32(tmax)
    return float(t + K_TPAD * (F32(1) + np.minimum(t, F32(1e30)))) if np.isfinite(t) else float("inf")


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1.0)


class _Margin:
    def __init__(self):
        self.m = float("inf")

    def add(self, v):
        self.m = min(self.m, v)


def _children(S, r, node, lim, mg):
    """wide_children for ray r: [(key, ref)] * 4 after the sorting network, misses as (inf, 0)."""
    refs, tmin, tmax = S["refs"][node], S["tmin"][r, node], S["tmax"][r, node]
    key, kr, slot = [], [], []
    for i in range(4):
        ref = int(refs[i])
        h = False
        if ref != 0:
            a, b = float(tmin[i]), float(tmax[i])
            lo = max(a, 0.0)
            h = b >= lo and a <= lim
            mg.add(_rel(b, lo))
            if lim != float("inf"):
                mg.add(_rel(a, lim))
        key.append(float(tmin[i]) if h else float("inf"))
        kr.append(ref if h else 0)
        slot.append(i)

    def cswap(x, y):
        ka, kb = key[x], key[y]
        if ka != float("inf") and kb != float("inf"):
            if ka == kb:
                # an exact tie must be structural: the same axis decides both keys with equal half bounds,
                # and the runner-up axis is a margin away
                tn, nb = S["tn"][r, node], S["near"][r, node]
                ax, ay = int(np.argmax(tn[slot[x]])), int(np.argmax(tn[slot[y]]))
                if ax != ay or nb[slot[x], ax] != nb[slot[y], ay]:
                    mg.add(0.0)
                for s_ in (slot[x], slot[y]):
                    others = np.delete(tn[s_], ax)
                    mg.add(_rel(float(tn[s_, ax]), float(others.max())) if others.max() != tn[s_, ax] else float("inf"))
            else:
                mg.add(_rel(ka, kb))
        if kb < ka:
            key[x], key[y] = kb, ka
            kr[x], kr[y] = kr[y], kr[x]
            slot[x], slot[y] = slot[y], slot[x]

    cswap(0, 1), cswap(2, 3), cswap(0, 2), cswap(1, 3), cswap(1, 2)
    return key, kr


def _leaf_prims(ref):
    a, k = T.leaf_range(ref)
    return list(range(a, a + k))


def walk_wide(S, r, cap, tmax=float("inf"), prune=True):
    """traverse_wide<cap> / WideWalk::node_step for ray r of slabs S. Returns a dict: peak (the largest sp), fire
    (the node at which sp + 3 > cap held, or None; the walk ends there), fire_depth (how many nodes the walk
    had visited before it), leaves_before (leaves queued before that node), order (tree positions of the
    Gaussians in the order the walk hands them out, the firing node's leaves included, as node_step queues
    them before its check), margin (the smallest relative margin of a decision)."""
    lim = prune_lim(tmax) if prune else float("inf")
    mg = _Margin()
    stack, node, peak, visited, nleaves, order = [], 0, 0, 0, 0, []
    while True:
        key, kr = _children(S, r, node, lim, mg)
        here = [ref for ref in kr if ref < 0]
        for ref in here:
            order += _leaf_prims(ref)
        inner = [ref for ref in kr if ref > 0]
        if len(stack) + 3 > cap:
            return {"peak": peak, "fire": node, "fire_depth": visited, "leaves_before": nleaves, "order": order,
                    "margin": mg.m}
        nleaves += len(here)
        visited += 1
        for ref in reversed(inner[1:]):  # far first
            stack.append(ref)
        peak = max(peak, len(stack))
        if inner:
            node = inner[0]
        elif stack:
            node = stack.pop()
        else:
            return {"peak": peak, "fire": None, "fire_depth": visited, "leaves_before": nleaves, "order": order,
                    "margin": mg.m}


def recursive_order(S, r, tmax=float("inf"), prune=True):
    """The Gaussians of a plain recursive near-first traversal: a node's leaf children near first, then its
    inner children near first, each to its end before the next."""
    lim = prune_lim(tmax) if prune else float("inf")
    mg = _Margin()
    out = []

    def visit(node):
        _, kr = _children(S, r, node, lim, mg)
        for ref in kr:
            if ref < 0:
                out.extend(_leaf_prims(ref))
        for ref in kr:
            if ref > 0:
                visit(ref)

    visit(0)
    return out


def walk_sigma(tree, points, cap):
    """query_sigma_kernel's containment walk of hnodes4 for every point: a list of dicts peak, fire (node at
    which sp + 4 > cap held, or None), margin (how far the closest containment decision is from turning: the
    smallest slack of a child holding the point, the largest excess of one that does not, in the nodes'
    normalised coordinates)."""
    info = tree["info"]
    hc, hs = np.asarray(info["hn_center"], F32), F32(info["hn_scale"])
    u = ((np.asarray(points, F32) - hc) * hs).astype(F32).astype(np.float64)
    b, refs = decode(tree["hnodes4"]), tree["hnodes4"]["c"]
    out = []
    for p in u:
        stack, node, peak, fire, margin = [], 0, 0, None, float("inf")
        while True:
            if len(stack) + 4 > cap:
                fire = node
                break
            for c in range(4):
                ref = int(refs[node, c])
                if ref == 0:
                    continue
                lo, hi = b[node, c, 0:3], b[node, c, 3:6]
                slack = np.concatenate([p - lo, hi - p])  # all >= 0: inside
                margin = min(margin, float(slack.min()) if slack.min() >= 0 else float(-slack.min()))
                if np.all(p >= lo) and np.all(p <= hi) and ref > 0:
                    stack.append(ref)
            peak = max(peak, len(stack))
            if not stack:
                break
            node = stack.pop()
        out.append({"peak": peak, "fire": fire, "margin": margin})
    return out


def walk_secondary(S, r, lim=float("inf")):
    """sec_node4v's walk of slabs S (of the tight tree, hnodes4s) from the root for ray r, a light ray ending at
    lim or an environment ray: the nearest inner child by a strict min-reduction in child order is walked
    next, the other inner children are pushed in child order. Returns (peak sp, the smallest relative margin,
    the largest stack index a node step wrote with sp <= WW_STACK - 3 on entry: its unconditional stores)."""
    plim = float(F32(lim) + K_TPAD * (F32(1) + F32(lim))) if np.isfinite(lim) else float("inf")
    mg = _Margin()
    stack, node, peak, top = [], 0, 0, -1
    while True:
        refs, tmin, tmax = S["refs"][node], S["tmin"][r, node], S["tmax"][r, node]
        best, nxt, inner = float("inf"), 0, []
        for i in range(4):
            a, b = float(tmin[i]), float(tmax[i])
            ref = int(refs[i])
            hit = ref != 0 and a <= min(b, plim) and b >= 0.0
            if ref != 0:
                mg.add(min(_rel(a, min(b, plim)), _rel(b, 0.0)))
            if hit and ref > 0:
                if best != float("inf") and a != best:
                    mg.add(_rel(a, best))
                if a < best:
                    best, nxt = a, ref
                inner.append(ref)
        sp = len(stack)
        if sp <= WW_STACK - 3:  # the branch-free form: a store per slot at the running sp
            k = sp
            for i in range(4):
                top = max(top, k)
                k += int(int(refs[i]) in inner and int(refs[i]) != nxt)
        stack += [ref for ref in inner if ref != nxt]
        peak = max(peak, len(stack))
        if nxt:
            node = nxt
        elif stack:
            node = stack.pop()
        else:
            return peak, mg.m, top


# ---- rays ----
def octant_dirs(rng, n, floor=0.3):
    """Unit directions with every component >= floor."""
    out = []
    while len(out) < n:
        v = np.abs(rng.normal(size=3))
        v /= np.linalg.norm(v)
        if v.min() >= floor:
            out.append(v)
    return np.array(out)


def family(name, n, rng, centre=CENTRE, extent=EXTENT):
    """(origins, directions, tmax) float32 of n rays of family F, B, I, C, P (passing the scene by) around the
    cloud's centre."""
    u = octant_dirs(rng, n)
    c = np.asarray(centre)
    tmax = np.full(n, np.inf)
    if name == "F" or name == "C":
        o, d = c - 3.0 * u, u
        if name == "C":
            tmax = 3.0 + rng.uniform(-0.4, 0.4, n) * extent  # ends inside the cloud
    elif name == "B":
        o, d = c + 3.0 * u, -u
    elif name == "I":
        o, d = c + rng.uniform(-0.4, 0.4, (n, 3)) * extent, u
    elif name == "P":
        # parallel to an F ray, moved sideways by more than the scene's half diagonal (3 sigma 1.05 sqrt 3 < 1.7)
        side = np.cross([0.0, 0.0, 1.0], u)  # towards -x, away from the ballast
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        o, d = c - 3.0 * u + 4.0 * side, u
    else:
        raise ValueError(name)
    return o.astype(F32), d.astype(F32), tmax.astype(F32)


WAVE = {"F": 22, "B": 14, "I": 10, "C": 10, "P": 6, "X": 2}  # rays of each family in every 64


def shuffled_batch(seed=71, n=1024):
    """n rays: every wave of 64 holds every family and the API's two invalid rays (X: a NaN origin, a zero
    direction) in a seeded order of its own, so that lanes that redo sit beside lanes that do not. Returns
    (origins, directions, tmax, family letter per ray)."""
    assert n % 64 == 0 and sum(WAVE.values()) == 64
    rng = np.random.default_rng(seed)
    waves = n // 64
    fam = {name: family("F" if name == "X" else name, k * waves, rng) for name, k in WAVE.items()}
    fam["X"][0][0::2, 0] = np.nan
    fam["X"][1][1::2] = 0.0
    o, d, t, names = [], [], [], []
    for w in range(waves):
        part = [tuple(a[k * w:k * (w + 1)] for a in fam[name]) for name, k in WAVE.items()]
        letters = np.array([name for name, k in WAVE.items() for _ in range(k)])
        perm = rng.permutation(64)
        for i, dst in enumerate((o, d, t)):
            dst.append(np.concatenate([p[i] for p in part])[perm])
        names.append(letters[perm])
    return np.concatenate(o), np.concatenate(d), np.concatenate(t), np.concatenate(names)


def forward_batch(n, seed=72):
    return family("F", n, np.random.default_rng(seed + n))


def classify(tree, o, d, tmax, names, cap, prune=True):
    """walk_wide of every valid ray of a batch: a list of results (None for invalid rays)."""
    ok = names != "X"
    S = slabs(tree, o[ok], d[ok])
    res, k = [], 0
    for i in range(len(o)):
        if not ok[i]:
            res.append(None)
            continue
        res.append(walk_wide(S, k, cap, float(tmax[i]), prune))
        k += 1
    return res


def family_verdict(res, names, cap):
    """What the tests assert of a classified batch, as a dict of figures; raises AssertionError naming the ray."""
    fig = {"min_leaves_before": 10 ** 9, "max_quiet_peak": 0, "margin": float("inf"), "fired": 0}
    for i, (r, nm) in enumerate(zip(res, names)):
        if r is None:
            continue
        fig["margin"] = min(fig["margin"], r["margin"])
        if nm in "FIC":
            assert r["fire"] is not None, f"ray {i} ({nm}) does not reach the stack limit: peak {r['peak']}"
            assert r["leaves_before"] >= 6, f"ray {i} ({nm}): {r['leaves_before']} leaves queued before the firing node"
            fig["min_leaves_before"] = min(fig["min_leaves_before"], r["leaves_before"])
            fig["fired"] += 1
        else:
            assert r["fire"] is None and r["peak"] < cap - 2, f"ray {i} ({nm}) reaches the stack limit: peak {r['peak']}"
            fig["max_quiet_peak"] = max(fig["max_quiet_peak"], r["peak"])
    return fig


# ---- the scenes the tests render and query ----
DENSITY = (0.004, 0.016)  # the comb's optical depth through its centre is 180 x the mean density: Tr about 0.17
LIGHT_OFFSET = np.array([1.5, 2.0, 1.8])  # the test light, from the cloud's centre: a positive-octant direction
LIGHT_INTENSITY = (30.0, 30.0, 30.0)
ENV = (0.4, 0.5, 0.6)


def comb_arrays(leaf_max, mirrored=False, seed=73, plan=PLAN):
    """(mean, cov6, density, albedo) float32 of the comb scene with seeded densities and albedos."""
    rows = comb_gaussians(leaf_max, mirrored, plan)
    rng = np.random.default_rng(seed)
    n = len(rows)
    return (rows[:, 0:3].copy(), rows[:, 3:9].copy(), rng.uniform(*DENSITY, n).astype(F32),
            rng.uniform(0.2, 0.9, n).astype(F32))


def light_position(mirrored=False):
    return CENTRE + (-LIGHT_OFFSET if mirrored else LIGHT_OFFSET)


def comb_scene(leaf_max, mirrored=False, extra_lights=()):
    import vr_amd as vr
    lights = [vr.Light(light_position(mirrored), LIGHT_INTENSITY)] + [vr.Light(p, i) for p, i in extra_lights]
    return vr.Scene.from_gaussians(*comb_arrays(leaf_max, mirrored), lights=lights, env_color=ENV)


def comb_oracle(leaf_max, mirrored=False, extra_lights=()):
    import pyoracle as O
    pos = [light_position(mirrored)] + [p for p, _ in extra_lights]
    inten = [LIGHT_INTENSITY] + [i for _, i in extra_lights]
    sc = O.OracleScene.from_gaussians(*comb_arrays(leaf_max, mirrored), pos, inten)
    sc.set_env(ENV)
    return sc
