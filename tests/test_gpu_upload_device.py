"""vr_upload_gaussians_device (Device.upload_gaussians, DeviceScene, autograd.optical_depth_resident): a Gaussian
scene uploaded straight from torch tensors on the GPU against the same floats uploaded as a host Scene with
VR_OPT_DEVICE_BVH = 1. The contract (include/vr_hip.h) is bitwise: every tree array and every record word but `norm`
is the host upload's, and `norm` is the numpy restatement of tests/upload_device_reference.py, at most 2 ulp from the
host's. Queries and frames are therefore compared bit for bit on scenes whose seed was chosen, on the CPU, so that no
row's norm differs (asserted), and a scene built around a row whose norm does differ checks the 2-ulp case.
Scenes are the few-hundred-Gaussian ones of tests/test_gpu_tree.py, rebuilt here from tree_reference."""
import functools

import numpy as np
import pytest

import grad_reference as R
import tree_reference as T
import upload_device_reference as U
import vr_amd as vr
from helpers import FOV

pytestmark = pytest.mark.gpu
F32 = np.float32
ENV = [0.4, 0.5, 0.6]
TREE_ARRAYS = ("order", "nodes", "hnodes", "hnodes4", "hnodes4s", "hnodes4w", "hnodes4t", "parent4", "prim_node4")
DEGENERATE = np.float32([0.009235004894435406, 0.06374555826187134, -0.06935998797416687, 0.5371712446212769,
                         -0.32841256260871887, 0.7535938024520874]) * np.float32(2.0 ** -14)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_rows(n, seed, lo=0.02, hi=0.12):
    rng = np.random.default_rng(seed)
    return T.gaussian_rows(rng.uniform(-1.0, 1.0, (n, 3)), T.rotated_cov(rng, n, lo, hi))


def coplanar_rows(n, seed, flat_axes):
    rows = random_rows(n, seed)
    rows[:, flat_axes] = 0.0
    return rows


def outlier_rows(seed=33):
    rng = np.random.default_rng(seed)
    rows = T.gaussian_rows(rng.uniform(0.0, 1.0, (300, 3)), T.rotated_cov(rng, 300))
    rows[299, 0:3] = 1e4
    return rows


def arrays_of(rows, seed=1, density=(0.5, 2.0)):
    """mean, cov6, density, albedo (float32) of tree_reference rows with seeded densities and albedos (scene_of)."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    return (np.ascontiguousarray(rows[:, 0:3], F32), np.ascontiguousarray(rows[:, 3:9], F32),
            rng.uniform(*density, n).astype(F32), rng.uniform(0.2, 0.9, n).astype(F32))


def host_scene(arrs, lights=()):
    return vr.Scene.from_gaussians(*arrs, lights=lights, env_color=ENV)


def device_scene(arrs, lights=()):
    """Device.upload_gaussians of the same floats as torch tensors on cuda:0."""
    import torch
    return vr.Device.get(0).upload_gaussians(*(torch.from_numpy(np.array(a)).cuda() for a in arrs), lights=lights, env_color=ENV)


def host_norm(arrs):
    return host_scene(arrs).records()[:, 10]


def norms_agree(arrs):
    """No row's device norm differs from the host's (both NaN counts as agreeing: neither side can use the row)."""
    h, d = host_norm(arrs), U.device_norm(arrs[1])
    return bool(np.all((bits(h) == bits(d)) | (np.isnan(h) & np.isnan(d))))


def both_trees(arrs, set_opt, lights=(), **options):
    """(tree after upload_gaussians, tree after the host upload with device_bvh = 1, host scene)."""
    for name, value in options.items():
        set_opt(name, value)
    dev = vr.Device.get(0)
    set_opt("device_bvh", 0)  # not consulted by the device-array upload
    device_scene(arrs, lights)
    got = dev.debug_tree()
    set_opt("device_bvh", 1)
    sc = host_scene(arrs, lights)
    dev.upload(sc, force=True)
    return got, dev.debug_tree(), sc


def assert_same_upload(got, want, arrs, exact_norm=False):
    """Test 1's rules: trees byte-identical, info equal, records equal but for word 10, which is the numpy restatement
    (exact_norm: the host's own, the host path ran) and within 2 ulp of the host's."""
    for name in TREE_ARRAYS:
        assert got[name].shape == want[name].shape and got[name].tobytes() == want[name].tobytes(), name
    gi, wi = got["info"], want["info"]
    for k in ("num_prims", "num_nodes", "num_nodes4", "bvh_depth", "built_on_device", "wrec_pd"):
        assert gi[k] == wi[k], (k, gi[k], wi[k])
    for k in ("bounds_min", "bounds_max", "hn_center"):
        assert np.array_equal(bits(gi[k]), bits(wi[k])), (k, gi[k], wi[k])
    assert bits(gi["hn_scale"]) == bits(wi["hn_scale"])
    g, w = got["records"], want["records"]
    assert g.shape == w.shape
    rest = [k for k in range(12) if k != 10]
    assert np.array_equal(bits(g[:, rest]), bits(w[:, rest]))
    if exact_norm:
        assert np.array_equal(bits(g[:, 10]), bits(w[:, 10]))
        return
    rule = U.device_norm(arrs[1])[got["order"]]
    nan = np.isnan(rule)
    assert np.array_equal(np.isnan(g[:, 10]), nan) and np.array_equal(bits(g[~nan, 10]), bits(rule[~nan]))
    ok = np.isfinite(w[:, 10]) & ~nan
    apart = U.ulp_apart(g[ok, 10], w[ok, 10])
    print(f"norm: {int(np.count_nonzero(apart))} of {len(apart)} rows differ from the host's, largest "
          f"{int(apart.max()) if len(apart) else 0} ulp")
    assert len(apart) == 0 or apart.max() <= 2


def records_by_rule(sc, arrs):
    rec = sc.records()
    rec[:, 10] = U.device_norm(arrs[1])
    return rec


# ---- 1. trees and records -------------------------------------------------------------------------
DEVICE_SCENES = {
    "random-256": lambda: random_rows(256, 41),
    "random-257": lambda: random_rows(257, 42),
    "random-513": lambda: random_rows(513, 43),
    "coincident-256": T.coincident_gaussians,
    "clusters-37x8": T.cluster_gaussians,
    "outlier-300": outlier_rows,
    "coplanar-300": lambda: coplanar_rows(300, 44, [2]),
    "tiny-300": lambda: random_rows(300, 46, 1e-3, 2e-3),  # half_tree_rule declines: the f32 tree only
}


@pytest.mark.parametrize("name", list(DEVICE_SCENES))
def test_trees_and_records(name, device_options):
    arrs = arrays_of(DEVICE_SCENES[name]())
    got, want, sc = both_trees(arrs, device_options)
    assert got["info"]["built_on_device"] and want["info"]["built_on_device"]
    assert_same_upload(got, want, arrs)
    pb = T.prim_boxes(sc.gaussians())
    levels = T.validate(got, pb, records_by_rule(sc, arrs))
    T.check_against_reference(got, pb)
    print(f"{name}: {levels} levels, {len(got['hnodes4'])} 4-wide nodes, tight {len(got['hnodes4s'])}")
    if name == "tiny-300":
        assert len(got["hnodes"]) == 0 and got["info"]["num_nodes4"] == 0
    if name.startswith("random"):
        assert len(got["hnodes4s"]) == len(got["hnodes4"]) > 0


def test_options_apply_as_at_any_upload(device_options):
    """VR_OPT_HALF_NODES = 0 and VR_OPT_SEC_TIGHT = 0 shape this upload as they shape the host's."""
    arrs = arrays_of(random_rows(300, 47))
    got, want, _ = both_trees(arrs, device_options, half_nodes=0)
    assert len(got["hnodes"]) == 0 and len(got["hnodes4"]) == 0
    assert_same_upload(got, want, arrs)
    device_options("half_nodes", 1)
    got, want, _ = both_trees(arrs, device_options, sec_tight=0)
    assert len(got["hnodes4"]) > 0 and len(got["hnodes4s"]) == 0
    assert_same_upload(got, want, arrs)


# ---- 2. small N: the host path ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255])
def test_small_scenes_take_the_host_path(n, device_options):
    arrs = arrays_of(random_rows(n, 100 + n, 0.1, 0.3))
    got, want, sc = both_trees(arrs, device_options)
    assert not got["info"]["built_on_device"] and not want["info"]["built_on_device"]
    assert got["info"]["num_prims"] == n
    assert_same_upload(got, want, arrs, exact_norm=True)
    T.validate(got, T.prim_boxes(sc.gaussians()), sc.records())


def test_empty_scene(device_options):
    import torch
    dev = vr.Device.get(0)
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    ds = dev.upload_gaussians(z(0, 3), z(0, 6), z(0), z(0), env_color=ENV)
    assert ds.get_num_primitives() == 0
    o, d = origin_rays(8)
    assert np.array_equal(dev.query_transmittance(ds, o, d), np.ones(8, F32))


# ---- 3. the stack limit ----------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1])
def test_stack_limit_chain(over, device_options):
    lim = T.limits()
    levels = lim["max_depth"] + 1 + over
    arrs = arrays_of(T.chain_gaussians(T.chain_k_for(levels, lim["leaf_max"])), seed=7, density=(1e-5, 3e-5))
    got, want, sc = both_trees(arrs, device_options)
    print(f"chain of {levels} levels: built_on_device {got['info']['built_on_device']}, bvh_depth {got['info']['bvh_depth']}")
    assert got["info"]["built_on_device"] == (over == 0)
    assert_same_upload(got, want, arrs, exact_norm=(over == 1))
    if over == 0:
        assert got["info"]["bvh_depth"] == levels
        T.check_against_reference(got, T.prim_boxes(sc.gaussians()))


# ---- 4. same answers -------------------------------------------------------------------------------
def origin_rays(n=256, seed=8):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    o = (3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return o, (-o).astype(F32)


LIGHT = [vr.Light([0.0, 3.0, 3.0], [20.0, 20.0, 20.0])]


@functools.lru_cache(maxsize=None)
def agreeing_case():
    """513 Gaussians, the first seed from 43 on at which no row's norm differs (about three seeds in four do)."""
    for seed in range(43, 63):
        arrs = arrays_of(random_rows(513, seed))
        if norms_agree(arrs):
            for a in arrs:
                a.setflags(write=False)
            return arrs
    raise AssertionError("no seed in 43..62 qualifies")


@functools.lru_cache(maxsize=None)
def agreeing_model():
    """The float64 model of agreeing_case along the first 64 origin rays (computed once, read-only)."""
    arrs = agreeing_case()
    o, d = origin_rays()
    return R.Model(R.oracle_from_gaussians(*arrs), o[:64], d[:64], np.float32(np.inf))


def answers(scene):
    dev = vr.Device.get(0)
    o, d = origin_rays()
    out = {}
    out["tr"], out["tau"] = dev.query_transmittance(scene, o, d, return_tau=True)
    off, t, g, entering = dev.query_events(scene, o, d)
    out["off"], out["t"], out["g"], out["in"] = off.astype(np.int32), t, g.astype(np.int32), entering.astype(np.uint32)
    pts = (0.5 * np.random.default_rng(9).uniform(-1.0, 1.0, (256, 3))).astype(F32)
    out["sigma"], active = dev.query_sigma(scene, pts, return_active=True)
    out["active"] = active.astype(np.uint32)
    ft, alb, act = dev.query_free_flight(scene, o, d, (0.5 * out["tau"]).astype(F32), return_albedo=True, return_active=True)
    out["ff_t"], out["ff_albedo"], out["ff_active"] = ft, alb, act.astype(np.uint32)
    g_o, g_d, g_t, tau2 = dev.query_transmittance_ray_grad(scene, o, d)
    out["g_o"], out["g_d"], out["g_t"], out["tau2"] = g_o, g_d, g_t, tau2
    cam = vr.Pinhole_Camera([0.0, 0.0, 4.0], [0.0, 0.0, -1.0], FOV)
    img = vr.Image(32, 32)
    vr.RayMarchingGaussians(cam, env_samples=4).render(scene, img)
    out["march"] = img.pixels.copy()
    vr.MultiScatterGaussians(cam, 4).render(scene, img)
    out["multiscatter"] = img.pixels.copy()
    grad = dev.query_transmittance_grad(scene, o[:64], d[:64])
    return out, grad


def test_same_answers(device_options):
    arrs = agreeing_case()
    assert norms_agree(arrs)  # the precondition of every bitwise comparison below
    device_options("device_bvh", 0)
    ds = device_scene(arrs, LIGHT)
    assert vr.Device.get(0).debug_tree(["order"])["info"]["built_on_device"]
    got, g_grad = answers(ds)
    device_options("device_bvh", 1)
    want, w_grad = answers(host_scene(arrs, LIGHT))
    assert np.all(want["tr"] < 1.0) and int(want["off"][-1]) > 256 and want["sigma"].max() > 0
    assert np.isfinite(want["march"]).all() and np.abs(want["march"] - F32(ENV)).max() > 0.01
    assert np.isfinite(want["ff_t"]).any()
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(bits(got[name]), bits(want[name])), name
    G, S = agreeing_model().grad(None, True)
    R.judge("gradient after upload_gaussians", g_grad, G, S)
    assert np.all(np.abs(g_grad.astype(np.float64) - w_grad) <= 2 * R.BOUND * S)


# ---- 5. a row whose norm differs -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def differing_row():
    """(cov6, host norm, device norm) of the first seeded covariance whose two norms differ (about 6 in 10 000 do)."""
    for seed in range(950, 960):
        cov = U.band_cov(1, 20_000, seed)
        n = len(cov)
        one = np.ones(n, F32)
        host = vr.Scene.from_gaussians(np.zeros((n, 3), F32), cov, one, one).records()[:, 10]
        k = np.flatnonzero(bits(host) != bits(U.device_norm(cov)))
        if len(k):
            return cov[k[0]].copy(), host[k[0]], U.device_norm(cov[k[0]:k[0] + 1])[0]
    raise AssertionError("no differing row among 200 000 covariances")


def test_a_differing_norm(device_options):
    """A row whose norm is not the host's, in a translucent scene with rays aimed through it. tau moves by at most
    2^-21 of itself against the host upload. The float64 model of grad_reference is that of the gradient query: the
    gradient after the device upload meets it at the module's own bound (the model takes the oracle's norm, the
    host's: 2 ulp on that row is 2^-22 S, half of the bound). The tau query itself adds f32 terms
    (optical_depth() per hit), so it stands some 1e-5 of tau from the model's float64 tau whichever upload ran; that
    figure is printed for both uploads, not bounded here."""
    cov, hn, dn = differing_row()
    assert 1 <= U.ulp_apart([dn], [hn])[0] <= 2
    mean, cov6, density, albedo = arrays_of(random_rows(256, 48), density=(0.005, 0.02))
    mean[0], cov6[0], density[0] = 0.0, cov, 0.02  # the row sits at the origin, where the rays are aimed
    arrs = (mean, cov6, density, albedo)
    o, d = origin_rays(64)
    dev = vr.Device.get(0)
    ds = device_scene(arrs)
    tree = dev.debug_tree(["order", "records"])
    assert tree["info"]["built_on_device"]
    assert bits(tree["records"][np.flatnonzero(tree["order"] == 0)[0], 10]) == bits(dn)
    _, tau_dev = dev.query_transmittance(ds, o, d, return_tau=True)
    grad_dev = dev.query_transmittance_grad(ds, o, d)
    device_options("device_bvh", 1)
    _, tau_host = dev.query_transmittance(host_scene(arrs), o, d, return_tau=True)
    mdl = R.Model(R.oracle_from_gaussians(*arrs), o, d, np.float32(np.inf))
    assert mdl.use[:, 0].all() and np.all(tau_host > 0) and np.all(tau_host < 50)  # every ray crosses the row
    rel = np.abs(tau_dev.astype(np.float64) - tau_host) / tau_host
    print(f"differing norm ({int(U.ulp_apart([dn], [hn])[0])} ulp): |tau_dev - tau_host| / tau max {rel.max():.3e} "
          f"(bound {2.0 ** -21:.3e}), rays whose tau differs {int(np.count_nonzero(rel))} of 64; |tau - model| / tau max "
          f"{(np.abs(tau_dev - mdl.tau) / mdl.tau).max():.3e} (device upload), {(np.abs(tau_host - mdl.tau) / mdl.tau).max():.3e} (host)")
    # 2 ulp on one factor of every term (2^-22 of tau at most) and the one final rounding on each side (2 * 2^-24)
    assert np.all(np.abs(tau_dev.astype(np.float64) - tau_host) <= 2.0 ** -21 * tau_host)
    R.judge("gradient with a differing norm", grad_dev, *mdl.grad(None, True))


# ---- 6. a covariance that is not positive definite -------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_case():
    for seed in range(70, 90):
        rows = random_rows(300, seed)
        extra = T.gaussian_rows(np.float32([[0.0, -30.0, 0.0]]), DEGENERATE[None])
        mean, cov6, density, albedo = arrays_of(np.concatenate([rows, extra]))
        density[-1], albedo[-1] = 0.3, 0.7
        if norms_agree((mean, cov6, density, albedo)):
            return mean, cov6, density, albedo
    raise AssertionError("no seed in 70..89 qualifies")


def test_not_positive_definite(device_options):
    arrs = degenerate_case()
    assert norms_agree(arrs)
    got, want, sc = both_trees(arrs, device_options)
    assert got["info"]["built_on_device"] and not got["info"]["wrec_pd"] and not want["info"]["wrec_pd"]
    assert_same_upload(got, want, arrs)
    dev = vr.Device.get(0)
    o, d = origin_rays()
    o = np.concatenate([o, np.float32([[0.0, -27.0, 0.0]])])  # and one ray at the degenerate Gaussian
    d = np.concatenate([d, np.float32([[0.0, -1.0, 0.0]])])
    _, tau_host = dev.query_transmittance(sc, o, d, return_tau=True)
    _, tau_dev = dev.query_transmittance(device_scene(arrs), o, d, return_tau=True)
    assert np.count_nonzero(tau_host) > 128
    assert np.array_equal(bits(tau_dev), bits(tau_host))


# ---- 7. lifecycle ----------------------------------------------------------------------------------
def test_lifecycle(device_options):
    import torch
    dev = vr.Device.get(0)
    arrs = agreeing_case()
    o, d = origin_rays()
    mean, cov6, density, albedo = (torch.from_numpy(np.array(a)).cuda() for a in arrs)
    ds = dev.upload_gaussians(mean, cov6, density, albedo, lights=LIGHT, env_color=ENV)
    assert isinstance(ds, vr.DeviceScene) and ds.get_num_primitives() == 513 and ds.volume_type == vr.Scene.GAUSSIANS
    assert len(ds.lights) == 1 and np.array_equal(ds.env_color, F32(ENV))
    _, tau0 = dev.query_transmittance(ds, o, d, return_tau=True)
    key = dev._scene_key
    dev.upload(ds)
    assert dev._scene_key == key  # the current scene: nothing to do
    dev.upload(host_scene(arrays_of(random_rows(50, 5))))
    assert dev.debug_tree(["order"])["info"]["num_prims"] == 50
    _, tau1 = dev.query_transmittance(ds, o, d, return_tau=True)  # displaced: uploaded again from the held tensors
    assert dev.debug_tree(["order"])["info"]["num_prims"] == 513
    assert np.array_equal(bits(tau1), bits(tau0)) and np.all(tau0 > 0)
    density.mul_(2.0)  # the optimiser case: the held tensors change in place
    _, stale = dev.query_transmittance(ds, o, d, return_tau=True)
    assert np.array_equal(bits(stale), bits(tau0))
    ds.refresh()
    _, tau2 = dev.query_transmittance(ds, o, d, return_tau=True)
    # tau is linear in the density and doubling is exact in every term: only the summation's roundings remain
    assert np.all(np.abs(tau2.astype(np.float64) - 2.0 * tau0) <= 2.0 ** -22 * tau2)
    img = vr.Image(32, 32)
    vr.RayMarchingGaussians(vr.Pinhole_Camera([0.0, 0.0, 4.0], [0.0, 0.0, -1.0], FOV), env_samples=4).render(ds, img)
    assert np.isfinite(img.pixels).all() and np.abs(img.pixels - F32(ENV)).max() > 0.01
    from vr_amd import _lib as L
    with pytest.raises(vr.VRError) as e:
        dev.upload_gaussians(mean, cov6, density, albedo, lights=LIGHT * 17)
    assert e.value.status == L.VR_ERR_UNSUPPORTED
    group = vr.Device((0, 0))
    with pytest.raises(vr.VRError) as e:
        group.upload_gaussians(mean, cov6, density, albedo)
    assert e.value.status == L.VR_ERR_UNSUPPORTED


# ---- 8. autograd -----------------------------------------------------------------------------------
def test_autograd_resident_is_optical_depth(device_options):
    import torch
    from vr_amd import autograd
    arrs = agreeing_case()
    assert norms_agree(arrs)
    o, d = origin_rays()
    o, d = o[:64], d[:64]
    w = np.random.default_rng(7).uniform(-1, 1, 64).astype(F32)
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    out = {}
    for resident in (False, True):
        fn = autograd.optical_depth_resident if resident else autograd.optical_depth
        p = [to(a).requires_grad_() for a in arrs[:3]]
        ro, rd = to(o).requires_grad_(), to(d).requires_grad_()
        tau = fn(*p, to(arrs[3]), ro, rd)
        (tau * to(w)).sum().backward()
        out[resident] = (tau.detach().cpu().numpy(), torch.cat([p[0].grad, p[1].grad, p[2].grad[:, None]], 1).cpu().numpy(),
                         ro.grad.cpu().numpy(), rd.grad.cpu().numpy())
        assert vr.Device.get(0).debug_tree(["order"])["info"]["built_on_device"] == resident
    a, b = out[False], out[True]
    assert np.all(a[0] > 0) and np.array_equal(bits(a[0]), bits(b[0]))
    G, S = agreeing_model().grad(w, True)
    R.judge("resident backward", b[1], G, S)
    assert np.all(np.abs(b[1].astype(np.float64) - a[1]) <= 2 * R.BOUND * S)
    assert np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3]))
    with pytest.raises(ValueError):
        autograd.optical_depth_resident(to(arrs[0]).cpu(), *(to(x) for x in arrs[1:]), to(o), to(d))


def test_autograd_resident_descent_step():
    """test_autograd_descent_step on 300 Gaussians whose parameters never leave the GPU: targets from parameters
    perturbed by 10 % (means and densities per number, each covariance by one factor, so it stays positive definite),
    a step sized for a first-order drop of 1 %, and a drop between 0.5 and 1.5 of that."""
    import torch
    from vr_amd import autograd
    frac = 0.01
    mean, cov6, density, albedo = (torch.from_numpy(a).cuda() for a in arrays_of(random_rows(300, 49), density=(0.01, 0.04)))
    gen = torch.Generator(device="cuda").manual_seed(7)
    pert = lambda x, shape: x * (1.0 + 0.1 * (2.0 * torch.rand(shape, device="cuda", generator=gen) - 1.0))  # noqa: E731
    star = [pert(mean, mean.shape), pert(cov6, (300, 1)), pert(density, density.shape)]
    o, d = origin_rays()
    ro, rd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    with torch.no_grad():
        target = autograd.optical_depth_resident(*star, albedo, ro, rd)
    p = [mean.requires_grad_(), cov6.requires_grad_(), density.requires_grad_()]
    loss0 = (autograd.optical_depth_resident(*p, albedo, ro, rd).double() - target.double()).square().sum()
    loss0.backward()
    assert vr.Device.get(0).debug_tree(["order"])["info"]["built_on_device"]
    assert all(x.grad.is_cuda for x in p)
    loss0 = loss0.detach()
    g2 = sum(float(x.grad.double().square().sum()) for x in p)
    eta = frac * float(loss0) / g2
    with torch.no_grad():
        q = [x - eta * x.grad for x in p]
        loss1 = (autograd.optical_depth_resident(*q, albedo, ro, rd).double() - target.double()).square().sum()
    ratio = (float(loss0) - float(loss1)) / (frac * float(loss0))
    print(f"resident descent: loss {float(loss0):.6e} -> {float(loss1):.6e}, predicted drop {frac * float(loss0):.3e}, ratio {ratio:.4f}")
    assert float(loss0) > 0 and 0.5 <= ratio <= 1.5
