"""Every tree vr_upload_scene puts on the device, read back with Device.debug_tree() and checked exactly
against the host reference of tests/tree_reference.py: the child-pair tree of either builder, its
half-precision copy, the 4-wide collapse, parents, record map, per-axis copies and the secondary rays'
tight refit. Every comparison is bitwise or an exact float64 inequality; the one frame bar (2e-6) is that
of test_device_bvh_renders_like_host_bvh. Scenes are a few hundred seeded Gaussians, frames 32 x 32."""
import ctypes
import functools

import numpy as np
import pytest

import tree_reference as T
import vr_amd as vr
from helpers import FOV, scene_path

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scene_of(rows, seed=1, density=(0.5, 2.0), lights=()):
    """A Scene of tree_reference Gaussian rows (means and covariances) with seeded densities and albedos."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    return vr.Scene.from_gaussians(rows[:, 0:3], rows[:, 3:9], rng.uniform(*density, n), rng.uniform(0.2, 0.9, n),
                                   lights=lights, env_color=[0.4, 0.5, 0.6])


def random_rows(n, seed, lo=0.02, hi=0.12):
    rng = np.random.default_rng(seed)
    return T.gaussian_rows(rng.uniform(-1.0, 1.0, (n, 3)), T.rotated_cov(rng, n, lo, hi))


def read_back(scene, set_opt, device_bvh, **options):
    """Uploads `scene` on the shared context with the given builder and returns (tree, primitive boxes,
    scene records)."""
    set_opt("device_bvh", device_bvh)
    for name, value in options.items():
        set_opt(name, value)
    dev = vr.Device.get(0)
    dev.upload(scene, force=True)  # (a failed upload raises: every upload here returned VR_OK)
    return dev.debug_tree(), T.prim_boxes(scene.gaussians()), scene.records()


check_against_reference = T.check_against_reference  # (shared with test_gpu_wide_stack.py)


# ---- host builder ---------------------------------------------------------------------------------
def test_host_leaf_boxes_are_the_restated_primitive_boxes(device_options):
    """prim_boxes is gaussian_bounds bit for bit: every leaf box of a host-built tree is the union of the
    restated boxes of its primitives. Everything below that passes prim_boxes to the validator rests on this."""
    scene = vr.Scene.load_GMM(scene_path("1000_random.txt"))
    tree, pb, _ = read_back(scene, device_options, 0)
    assert not tree["info"]["built_on_device"] and tree["info"]["num_prims"] == 1000
    sb, leaves = pb[tree["order"]], 0
    for node in tree["nodes"]:
        for s in range(2):
            if node["c"][s] < 0:
                a, k = T.leaf_range(node["c"][s])
                want = np.concatenate([sb[a:a + k, 0:3].min(axis=0), sb[a:a + k, 3:6].max(axis=0)])
                assert np.array_equal(bits(node["f"][6 * s:6 * s + 6]), bits(want)), (a, k)
                leaves += 1
    assert leaves >= 1000 // tree["info"]["leaf_max"]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 50, "1000_random.txt"])
def test_host_built_trees(n, device_options):
    """N = 1 and 2 are single leaves (with kLeafMax 2): the empty-child forms of the collapse and parents_kernel."""
    scene = vr.Scene.load_GMM(scene_path(n)) if isinstance(n, str) else scene_of(random_rows(n, 100 + n, 0.1, 0.3))
    tree, pb, rec = read_back(scene, device_options, 0)
    assert not tree["info"]["built_on_device"]
    levels = T.validate(tree, pb, rec)
    print(f"host tree of {n}: {levels} levels, {len(tree['nodes'])} nodes, {len(tree['hnodes4'])} 4-wide, "
          f"tight {len(tree['hnodes4s'])}")
    assert len(tree["hnodes"]) == len(tree["nodes"]) and len(tree["hnodes4"]) > 0  # the half trees are under test
    assert len(tree["hnodes4s"]) == len(tree["hnodes4"]) == len(tree["hnodes4t"])  # ... and the tight refit
    if not isinstance(n, str) and n <= tree["info"]["leaf_max"]:
        assert levels == 1 and tree["nodes"]["c"][0, 1] == 0 and list(tree["hnodes4"]["c"][0, 1:]) == [0, 0, 0]


# ---- device builder -------------------------------------------------------------------------------
def coplanar_rows(n, seed, flat_axes):
    rows = random_rows(n, seed)
    rows[:, flat_axes] = 0.0  # a box symmetric about 0 has the centroid exactly 0: zero extent on the axis
    return rows


def outlier_rows(seed=33):
    rng = np.random.default_rng(seed)
    rows = T.gaussian_rows(rng.uniform(0.0, 1.0, (300, 3)), T.rotated_cov(rng, 300))
    rows[299, 0:3] = 1e4
    return rows


DEVICE_SCENES = {
    "random-256": lambda: random_rows(256, 41),   # the builder's minimum: one block, 255 internal nodes
    "random-257": lambda: random_rows(257, 42),   # 256 internal nodes fill a block; the primitives spill into a second
    "random-513": lambda: random_rows(513, 43),
    "coincident-256": T.coincident_gaussians,     # every key equal, every axis of zero extent
    "coplanar-300": lambda: coplanar_rows(300, 44, [2]),
    "collinear-300": lambda: coplanar_rows(300, 45, [1, 2]),
    "clusters-37x8": T.cluster_gaussians,         # stable sort and the index tie-break decide
    "outlier-300": outlier_rows,                  # all but one in a few cells
}


@pytest.mark.parametrize("name", list(DEVICE_SCENES))
def test_device_built_trees(name, device_options):
    scene = scene_of(DEVICE_SCENES[name]())
    tree, pb, rec = read_back(scene, device_options, 1)
    assert tree["info"]["built_on_device"]
    levels = T.validate(tree, pb, rec)
    check_against_reference(tree, pb)
    print(f"{name}: {levels} levels, {len(tree['hnodes4'])} 4-wide nodes, tight {len(tree['hnodes4s'])}")
    if name.startswith("random"):
        assert len(tree["hnodes4s"]) == len(tree["hnodes4"]) > 0  # the half, 4-wide and tight trees are under test


def test_device_tree_without_half_nodes(device_options):
    """Gaussians small against the scene (median box extent under 3 % of its half extent): half_tree_rule
    declines, nothing half-precision exists, and the float32 tree is the reference's all the same."""
    scene = scene_of(random_rows(300, 46, 1e-3, 2e-3))
    tree, pb, rec = read_back(scene, device_options, 1)
    assert tree["info"]["built_on_device"]
    for name in ("hnodes", "hnodes4", "hnodes4s", "hnodes4w", "hnodes4t", "parent4", "prim_node4"):
        assert len(tree[name]) == 0, name
    assert tree["info"]["num_nodes4"] == 0
    T.validate(tree, pb, rec)
    check_against_reference(tree, pb)


# ---- the stack limit ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_scene(levels):
    lim = T.limits()
    rows = T.chain_gaussians(T.chain_k_for(levels, lim["leaf_max"]))
    # 257 Gaussians overlap at the origin: ~0.013 of optical depth each through the centre
    return scene_of(rows, seed=7, density=(1e-5, 3e-5))


def origin_rays(n=256, seed=8):
    """Rays aimed through the origin from a sphere of radius 3 around the scene (the unit cube)."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    o = (3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return o, (-o).astype(np.float32)


def queries_and_frame(scene):
    dev = vr.Device.get(0)
    o, d = origin_rays()
    tr, tau = dev.query_transmittance(scene, o, d, return_tau=True)
    off, t, g, entering = dev.query_events(scene, o, d)
    img = vr.Image(32, 32)
    cam = vr.Pinhole_Camera([0.0, 0.0, 0.5], [0.0, 0.0, -1.0], FOV)  # the cluster at the origin spans ~7 pixels
    vr.RayMarchingGaussians(cam, env_samples=4).render(scene, img)
    return {"tr": tr, "tau": tau, "off": off.astype(np.int32), "t": t, "g": g, "in": entering.astype(np.uint32)}, img.pixels.copy()


@pytest.mark.parametrize("over", [0, 1])
def test_stack_limit_chain(over, device_options):
    """A radix tree of kMaxDepth + 1 levels is the deepest the device builder keeps; one level more falls back
    to the host builder (its first execution under test). Rays through the origin descend the chain."""
    lim = T.limits()
    levels = lim["max_depth"] + 1 + over
    scene = chain_scene(levels)
    tree, pb, rec = read_back(scene, device_options, 1)  # VR_OK on both
    info = tree["info"]
    print(f"chain scene of {levels} reference levels, {info['num_prims']} Gaussians: built_on_device "
          f"{info['built_on_device']}, bvh_depth {info['bvh_depth']}")
    measured = T.validate(tree, pb, rec)
    if over == 0:
        assert info["built_on_device"]
        assert info["bvh_depth"] == levels == measured
        check_against_reference(tree, pb)
    else:
        assert not info["built_on_device"]
        assert measured == info["bvh_depth"] <= lim["max_depth"] + 1
    got, frame = queries_and_frame(scene)
    host_tree, _, _ = read_back(scene, device_options, 0)
    assert not host_tree["info"]["built_on_device"]
    T.validate(host_tree, pb, rec)
    want, host_frame = queries_and_frame(scene)
    assert int(want["off"][-1]) > 256 and np.all(want["tr"] < 1.0)  # the rays meet the cluster at the origin
    for name in want:
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    d = float(np.max(np.abs(frame.astype(np.float64) - host_frame)))
    print(f"|frame on this tree - frame on the host tree| max {d:.3e}; frame range {host_frame.min():.3f} .. "
          f"{host_frame.max():.3f}; events {int(want['off'][-1])}, Tr {want['tr'].min():.3f} .. {want['tr'].max():.3f}")
    assert np.isfinite(frame).all()
    assert np.abs(host_frame - np.float32([0.4, 0.5, 0.6])).max() > 0.01  # the frame sees the cluster, not the environment alone
    assert d < 2e-6


# ---- tight tree and a record that is not positive definite ------------------------------------------
def test_non_positive_definite_scene_keeps_the_shared_boxes(tmp_path, device_options):
    """The scene of test_non_positive_definite_record_uses_the_m_forms: no whitened records, so no tight refit."""
    cov = np.float32([0.009235004894435406, 0.06374555826187134, -0.06935998797416687, 0.5371712446212769,
                      -0.32841256260871887, 0.7535938024520874]) * np.float32(2.0 ** -14)
    src = open(scene_path("50_random.txt")).read().rstrip("\n")
    path = tmp_path / "50_random_plus_degenerate.txt"
    path.write_text(src + "\ng 0.0 -30.0 0.0  " + " ".join(f"{c:.9g}" for c in cov) + "  0.3 0.7  0.1 0.1 0.1\n")
    scene = vr.Scene.load_GMM(str(path))
    tree, pb, rec = read_back(scene, device_options, 0)
    assert not tree["info"]["wrec_pd"]
    assert len(tree["hnodes4"]) > 0
    assert len(tree["hnodes4s"]) == 0 or tree["hnodes4s"].tobytes() == tree["hnodes4"].tobytes()
    T.validate(tree, pb, rec)


# ---- after the inverse loop -----------------------------------------------------------------------
def test_tree_after_the_inverse_loop(device_options):
    """vr_sfd_optimize re-uploads Adam-updated Gaussians through the device builder on every iteration: the
    tree it leaves behind is that of the parameters it returns."""
    from vr_amd import inverse as inv
    device_options("device_bvh", 0)  # the loop forces the device builder on itself
    cam = vr.Pinhole_Camera([0.0, 0.0, 4.0], [0.0, 0.0, -1.0], FOV)
    target = scene_of(random_rows(256, 51), lights=[vr.Light([0.0, 3.0, 3.0], [20.0, 20.0, 20.0])])
    I_ref = vr.Image(32, 32)
    vr.MultiScatterGaussians(cam, 4).render(target, I_ref)
    p0 = inv.pack_parameters(target.gaussians())
    p0[9::11] += np.float32(np.log(0.5))
    start = inv.apply_params(p0, target.lights, target.env_color)
    cfg = inv.SFDConfig(max_iters=2, save_every=0, num_stoch_samples=2, lr=1e-2, seed=3, final_samples=0)
    opt = inv.StochasticFiniteDiffInverseIntegrator(cam, vr.MultiScatterGaussians(cam, 4), cfg)
    assert opt.optimize(start, I_ref)
    tree = vr.Device.get(0).debug_tree()
    assert tree["info"]["built_on_device"] and tree["info"]["num_prims"] == 256
    assert not np.array_equal(opt.params, p0)
    pb = T.prim_boxes(opt.scene.gaussians())  # the loop's last upload is apply_params of the parameters it returns
    T.validate(tree, pb, opt.scene.records())
    check_against_reference(tree, pb)


# ---- state ----------------------------------------------------------------------------------------
def test_read_back_leaves_the_context_alone(device_options):
    scene = scene_of(random_rows(300, 61))
    device_options("device_bvh", 1)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera([0.0, 0.0, 4.0], [0.0, 0.0, -1.0], FOV), env_samples=4)
    img = vr.Image(32, 32)
    integ.render(scene, img)
    dev = vr.Device.get(0)
    before, first = dev.stats(), img.pixels.copy()
    a = dev.debug_tree()
    b = dev.debug_tree()
    for name in a:
        if name != "info":
            assert a[name].tobytes() == b[name].tobytes() and a[name].shape == b[name].shape, name
    assert len(a["nodes"]) == 299 and first.std() > 0
    dev.synchronize()
    assert dev.stats() == before
    integ.render(scene, img)
    assert np.array_equal(bits(img.pixels), bits(first))


def test_read_back_refuses_contexts_without_a_gaussian_tree():
    from vr_amd import _lib as L
    n = ctypes.c_size_t()

    def status(dev):
        return L.lib().vr_debug_tree(dev._h, 0, None, 0, ctypes.byref(n), None, None)

    fresh = vr.Device(0)
    assert status(fresh) == 1  # VR_ERR_INVALID: no scene
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert status(fresh) == 1  # a sphere scene
    fresh.upload(vr.Scene.load_GMM(scene_path("2_gaussian.txt")))
    assert status(fresh) == 0 and n.value == 2
    assert L.lib().vr_debug_tree(fresh._h, 99, None, 0, ctypes.byref(n), None, None) == 1  # unknown array
    group = vr.Device((0, 0))
    group.upload(vr.Scene.load_GMM(scene_path("2_gaussian.txt")))
    assert status(group) == 1  # a multi-device group context
