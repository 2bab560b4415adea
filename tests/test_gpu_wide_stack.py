"""Every walk of the 4-wide tree at its stack limit: the comb scene of tests/wide_walk_reference.py on the
device builder's tree, each query and frame against the reference and under the bound of that query's own
test, unchanged (test_gpu_query.py, test_gpu_query_grad.py, test_gpu_query_ray_grad.py,
test_gpu_query_flight.py / flight_reference.py, test_gpu_freeflight.py, the smoke frame's 1e-4).

Proof that the second paths run: the simulators of wide_walk_reference.py on the tree read back from the device
(`on_device`; every test goes through it). Under "wide" (device_bvh 1, half_nodes 1) every F, I and C ray
reaches sp + 3 > kStackSize at its 14th node with 7 leaves queued, so at least two leaves' Gaussians have been
tested (WideWalk's FIFO lets a lane step on with 4 leaves at the most) and GradOp::redo has adds to take back;
no B or passing ray comes within 2 of the limit. "pair" (half_nodes 0: every walk a plain redo) and "host" (the
host builder's tree, which no ray overflows) are the controls: same calls, same bounds.

The comb has 256 Gaussians, not the 120 at most its first sketch had: the device builder takes no fewer. 102
of them are the comb and lie over one another; the other 154 are a ballast clear of every ray through the comb.
"""
import functools

import numpy as np
import pytest

import flight_reference as F
import grad_reference as R
import pyoracle as O
import ray_grad_reference as RR
import tree_reference as T
import vr_amd as vr
import wide_walk_reference as W

pytestmark = pytest.mark.gpu

CAP = 32  # kStackSize
INF = np.float32(np.inf)
PARITY = 1e-4        # test_gpu_query.py
TAU_RTOL = 8.2e-7    # test_gpu_query.py
SIGMA_RTOL = 5.3e-6  # test_gpu_query.py
CONFIGS = {"wide": (1, 1), "pair": (1, 0), "host": (0, 1)}  # device_bvh, half_nodes
STEP = 0.1  # the ray-march frame's step: about 20 scatter records per pixel, and an oracle frame in seconds
INSIDE_LIGHT = ((W.CENTRE + np.array([0.1, 0.05, -0.08])).tolist(), (5.0, 5.0, 5.0))  # within the comb's 3 sigma


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def leaf_max():
    return T.limits()["leaf_max"]


@functools.lru_cache(maxsize=None)
def scene(mirrored=False, inside_light=False):
    return W.comb_scene(leaf_max(), mirrored, (INSIDE_LIGHT,) if inside_light else ())


@functools.lru_cache(maxsize=None)
def oracle(mirrored=False, inside_light=False):
    return W.comb_oracle(leaf_max(), mirrored, (INSIDE_LIGHT,) if inside_light else ())


@functools.lru_cache(maxsize=None)
def batch(name):
    """(origins, directions, tmax, family letters), read-only: "shuffled" (1024 rays, every family in every wave, the C
    rays clipped), "shuffled_inf" (the same rays unclipped), "f64" (one whole wave that redoes), "f257" (a partial wave)."""
    if name.startswith("shuffled"):
        o, d, tmax, names = W.shuffled_batch()
        if name == "shuffled_inf":
            tmax = np.full(len(o), INF, np.float32)
    else:
        o, d, tmax = W.forward_batch(int(name[1:]))
        names = np.array(["F"] * len(o))
    for a in (o, d, tmax, names):
        a.setflags(write=False)
    return o, d, tmax, names


_verdicts = {}


def verdict(tree, strict):
    """The simulators' classification of the shuffled batch (pruned and not) and the two forward batches on
    `tree`, computed once per tree. strict: assert the families' sides of the limit."""
    key = (tree["hnodes4"].tobytes(), np.asarray(tree["info"]["hn_center"]).tobytes(), float(tree["info"]["hn_scale"]))
    if key not in _verdicts:
        out = {}
        for name, prune in (("shuffled", True), ("shuffled", False), ("f64", True), ("f257", True)):
            o, d, tmax, names = batch(name)
            res = W.classify(tree, o, d, tmax, names, CAP, prune)
            fired = {f: sum(r is not None and r["fire"] is not None for r, nm in zip(res, names) if nm == f) for f in "FBICP"}
            peaks = {f: max([r["peak"] for r, nm in zip(res, names) if nm == f and r is not None], default=0) for f in "FBICP"}
            out[(name, prune)] = (res, names, fired, peaks)
        _verdicts[key] = out
    for (name, prune), (res, names, fired, peaks) in _verdicts[key].items():
        print(f"simulated on this tree, {name} prune {prune}: rays that reach the limit {fired}, peaks {peaks}")
        if strict:
            fig = W.family_verdict(res, names, CAP)
            print(f"  {fig}")
            assert fig["margin"] > 2.0 ** -18
    return _verdicts[key]


def on_device(set_opt, config, mirrored=False, inside_light=False, sc=None):
    """Uploads the comb under `config` and shows, on the tree read back, what its rays do. Returns (device, scene)."""
    device_bvh, half_nodes = CONFIGS[config]
    set_opt("device_bvh", device_bvh)
    set_opt("half_nodes", half_nodes)
    dev = vr.Device.get(0)
    sc = sc or scene(mirrored, inside_light)
    dev.upload(sc, force=True)
    check_tree(dev, sc, config, mirrored)
    return dev, sc


def check_tree(dev, sc, config, mirrored=False):
    tree = dev.debug_tree()
    pb = T.prim_boxes(sc.gaussians())
    levels = T.validate(tree, pb, sc.records())
    info = tree["info"]
    print(f"{config}: built_on_device {info['built_on_device']}, {levels} levels, {len(tree['hnodes4'])} 4-wide nodes")
    if config == "host":
        assert not info["built_on_device"] and len(tree["hnodes4"]) > 0
        if not mirrored:
            verdict(tree, False)  # (printed; nothing is asserted of the host builder's tree)
        return tree
    assert info["built_on_device"]
    T.check_against_reference(tree, pb)
    if config == "pair":
        assert len(tree["hnodes4"]) == 0 and len(tree["hnodes"]) == 0
        return tree
    assert len(tree["hnodes4"]) > 0
    if not mirrored:
        verdict(tree, True)
    return tree


# ---- oracle references, computed once ----
@functools.lru_cache(maxsize=None)
def probes(name):
    """(n, N, 4) f32 oracle probe of every valid ray of the batch (zero rows for invalid rays)."""
    import ctypes
    o, d, _, names = batch(name)
    sc = oracle()
    out = np.zeros((len(o), sc.num, 4), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    probe, base = O.lib().orc_gaussian_probe, out.ctypes.data
    oc, dc = np.ascontiguousarray(o), np.ascontiguousarray(d)
    for r in np.nonzero(names != "X")[0]:
        po, pd = oc[r].ctypes.data_as(fp), dc[r].ctypes.data_as(fp)
        for i in range(sc.num):
            probe(sc.h, i, po, pd, ctypes.cast(base + 16 * (int(r) * sc.num + i), fp))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grad_model(name):
    o, d, tmax, _ = batch(name)
    return R.Model(oracle(), o, d, tmax)


@functools.lru_cache(maxsize=None)
def signed_weights(n):
    w = np.random.default_rng(75).uniform(-1, 1, n).astype(np.float32)
    w.setflags(write=False)
    return w


# ---- tree ----
def test_the_device_tree_is_the_reference_comb(device_options):
    on_device(device_options, "wide")
    on_device(device_options, "wide", mirrored=True)


# ---- transmittance and tau ----
@pytest.mark.parametrize("config", list(CONFIGS))
def test_transmittance_and_tau(config, device_options):
    """Bounds of test_gpu_query.py: |Tr - oracle| <= 1e-4 (the f32 probe's double sum for unclipped rays, the float64
    integral over the probe's clip bounds for the C rays), |tau - oracle| <= 8.2e-7 tau, Tr == expf(-tau) and the
    call without tau bit for bit; NaN for invalid rays. Measured on an MI355X: see DESIGN.md."""
    import torch
    dev, sc = on_device(device_options, config)
    o, d, tmax, names = batch("shuffled")
    pr = probes("shuffled")
    tr, tau = dev.query_transmittance(sc, o, d, tmax=tmax, return_tau=True)
    bad = names == "X"
    assert np.all(np.isnan(tr[bad])) and np.all(np.isnan(tau[bad]))
    full = ~bad & np.isinf(tmax)
    use = (pr[..., 0] != 0) & (pr[..., 2] > pr[..., 1])
    ref = np.where(use, pr[..., 3].astype(np.float64), 0.0).sum(1)
    err = float(np.max(np.abs(tr[full].astype(np.float64) - np.exp(-ref[full].astype(np.float32).astype(np.float64)))))
    pos = full & (ref > 0)
    rel = float(np.max(np.abs(tau[pos].astype(np.float64) - ref[pos]) / ref[pos]))
    clip = names == "C"
    ref_c = grad_model("shuffled").tau[clip]
    err_c = float(np.max(np.abs(tr[clip].astype(np.float64) - np.exp(-ref_c))))
    print(f"{config}: max |Tr - oracle| {err:.3e} unclipped, {err_c:.3e} clipped; max |tau - oracle| / tau {rel:.3e}; "
          f"Tr {np.nanmin(tr):.3f} .. {np.nanmax(tr):.3f}")
    assert pos.sum() >= 600 and np.all(ref[names == "P"] == 0.0)
    assert err <= PARITY and err_c <= PARITY and rel <= TAU_RTOL
    assert np.all(tau[full & (ref == 0)] == 0.0)
    ok = ~bad
    expd = torch.exp(-torch.tensor(tau[ok]).cuda()).cpu().numpy()
    assert np.array_equal(bits(tr[ok]), bits(expd))
    tr_only = dev.query_transmittance(sc, o, d, tmax=tmax)
    assert np.array_equal(bits(tr_only[ok]), bits(tr[ok])) and np.all(np.isnan(tr_only[bad]))


# ---- events ----
_events = {}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_events(config, device_options):
    """Offsets, t, Gaussian and flag equal the oracle's events sorted by (t, scene index, entry first), bit for bit
    (test_gpu_query.check_events), and the three trees give the same arrays."""
    from test_gpu_query import check_events
    dev, sc = on_device(device_options, config)
    o, d, _, names = batch("shuffled")
    off, t, g, e = dev.query_events(sc, o, d)
    ties = check_events(probes("shuffled"), off, t, g, e)
    print(f"{config}: {off[-1]} events, {ties} tied")
    assert off[-1] > 150 * int(np.isin(names, list("FBIC")).sum()) // 2
    _events[config] = (off, bits(t), g, e)
    for other in _events.values():
        for a, b in zip(other, _events[config]):
            assert np.array_equal(a, b)


# ---- gradient ----
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["f64", "f257", "shuffled", "shuffled_inf"])
def test_gradient(name, config, device_options):
    """grad_reference.judge: |G_dev - G64| <= 2^-21 S per component, exact zeros where S = 0, for signed weights and
    both bound modes; weights=None on the partial wave. Under "wide" every F, I and C ray takes back the Gaussians
    of its first leaves before the pair-tree walk adds its whole hit set. Measured on an MI355X: see DESIGN.md."""
    dev, sc = on_device(device_options, config)
    o, d, tmax, _ = batch(name)
    mdl = grad_model(name)
    w = signed_weights(len(o))
    assert mdl.use[:, :W.comb_count(leaf_max())].sum() >= 0.6 * len(o) * 100
    for moving in (True, False):
        g = dev.query_transmittance_grad(sc, o, d, w, tmax=tmax, moving_bounds=moving)
        assert g.shape == (mdl.N, 10)
        R.judge(f"{config} {name} moving={moving} signed", g, *mdl.grad(w, moving))
    if name == "f257":
        g = dev.query_transmittance_grad(sc, o, d, None, tmax=tmax)
        R.judge(f"{config} {name} weights=None", g, *mdl.grad(None, True))


# ---- ray gradient ----
@functools.lru_cache(maxsize=None)
def ray_model(name, unit):
    from test_gpu_query_ray_grad import stored
    o, d, tmax, _ = batch(name)
    d_raw = stored(d, unit)[1]
    return RR.RayModel(oracle(), o, d_raw, tmax, unit, R.probe(oracle(), o, d_raw))


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("name", ["f64", "f257", "shuffled"])
def test_ray_gradient(name, unit, config, device_options):
    """ray_grad_reference.judge (2^-21 S) on the valid rays, NaN rows for the invalid ones, both bound modes; tau is
    the transmittance query's bit for bit. Measured on an MI355X: see DESIGN.md."""
    from test_gpu_query_ray_grad import forward_tau, same_bits, stored
    dev, sc = on_device(device_options, config)
    o, d, tmax, names = batch(name)
    d_dev = stored(d, unit)[0]
    mdl = ray_model(name, unit)
    ok = names != "X"
    assert np.array_equal(mdl.valid, ok)
    for moving in (True, False):
        g_o, g_d, g_t, tau = dev.query_transmittance_ray_grad(sc, o, d_dev, tmax=tmax, unit=unit, moving_bounds=moving)
        rows = RR.pack_rows(g_o, g_d, g_t)
        G64, S = mdl.rows(moving)
        RR.judge(f"{config} {name} unit={unit} moving={moving}", rows[ok], G64[ok], S[ok])
        assert np.all(np.isnan(rows[~ok])) and np.all(np.isnan(tau[~ok]))
        fwd = forward_tau(dev, sc, o, d_dev, tmax, unit)
        assert same_bits(tau[ok], fwd[ok]), "tau differs from query_transmittance's"


# ---- sigma ----
def sigma_model(rec, p):
    """test_gpu_query.sigma_model for given records: float64 evaluate_sigma over the Gaussians with q <= 9."""
    rec = rec.astype(np.float64)
    mean, dens, norm, alb = rec[:, :3], rec[:, 3], rec[:, 10], rec[:, 11]
    m = rec[:, 4:10]
    x = p.astype(np.float64)[:, None, :] - mean[None]
    q = (m[:, 0] * x[..., 0] ** 2 + m[:, 3] * x[..., 1] ** 2 + m[:, 5] * x[..., 2] ** 2 +
         2.0 * (m[:, 1] * x[..., 0] * x[..., 1] + m[:, 2] * x[..., 0] * x[..., 2] + m[:, 4] * x[..., 1] * x[..., 2]))
    act = q <= 9.0
    mu = np.where(act, dens * norm * np.exp(-0.5 * q), 0.0)
    s, sa = mu.sum(1), (mu * alb).sum(1)
    amix = np.where(s > 0, sa / np.where(s > 0, s, 1.0), 0.0)
    return np.stack([(1.0 - amix) * s, amix * s], 1), act.sum(1), q


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("mirrored", [True, False])
def test_sigma(mirrored, config, device_options):
    """Points in the comb. In the mirrored comb the containment walk pops the spine first and reaches
    sp + 4 > kStackSize (simulated on the tree read back); on the plain comb its stack stays under 8. Bound of
    test_gpu_query.py: |sigma - model| <= 5.3e-6 max(1, sigma); the active count is exact."""
    dev, sc = on_device(device_options, config, mirrored=mirrored)
    p = (W.CENTRE + np.random.default_rng(74).uniform(-0.4, 0.4, (256, 3)) * W.EXTENT).astype(np.float32)
    if config == "wide":
        sim = W.walk_sigma(dev.debug_tree(), p, CAP)
        fired = sum(r["fire"] is not None for r in sim)
        print(f"mirrored {mirrored}: {fired} of {len(p)} points reach the limit, peak {max(r['peak'] for r in sim)}")
        assert fired == (len(p) if mirrored else 0) and min(r["margin"] for r in sim) > 1e-3
    ref, ref_act, q = sigma_model(oracle(mirrored).records(), p)
    assert not np.any(np.abs(q - 9.0) <= 9e-4)
    sig, act = dev.query_sigma(sc, p, return_active=True)
    ratio = float(np.max(np.abs(sig.astype(np.float64) - ref) / np.maximum(1.0, ref)))
    print(f"{config} mirrored {mirrored}: max |sigma - model| / max(1, sigma) {ratio:.3e}, active {act.min()} .. {act.max()}")
    assert np.array_equal(act, ref_act) and np.all(act == W.comb_count(leaf_max()))
    assert ratio <= SIGMA_RTOL


# ---- free-flight query ----
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("solver", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["comb", "comb_back"])
def test_free_flight_query(name, solver, config, device_options):
    """flight_reference.judge, every solver: the forward camera's rays all overflow the collection walk's stack
    (test_wide_walk_reference.py), the backward camera's never do."""
    device_bvh, half_nodes = CONFIGS[config]
    device_options("device_bvh", device_bvh)
    device_options("half_nodes", half_nodes)
    device_options("ff_solver", solver)
    dev = vr.Device.get(0)
    dev.upload(F.device_scene(name), force=True)
    check_tree(dev, F.device_scene(name), config)
    fig = F.judge(name, *F.ask(dev, name), solver=solver, label=f"{config} {name} solver {solver}")
    assert fig["scattering"] == F.SCATTERING[name]


# ---- free-flight frames ----
def comb_camera():
    pos, view = F.camera_of("comb")
    return vr.Pinhole_Camera(pos, view, F.COMB_FOV), pos, view


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("multi", [False, True])
def test_free_flight_frames(multi, config, device_options):
    """16 x 16, 4 samples, through the comb's centre along a positive-octant direction, the light in the positive
    octant of the comb: camera and shadow rays overflow. The frames of ff_kernel 1 / 2 x ff_nee_queue 0 / 16 are
    one frame bit for bit and match the oracle under test_gpu_freeflight._check; no path needed the large rows;
    with the 4-wide tree present, pair-tree steps (node2_steps) are the redo's."""
    from test_gpu_freeflight import _check
    dev, sc = on_device(device_options, config)
    cam, pos, view = comb_camera()
    integ = vr.MultiScatterGaussians(cam, 4, 5) if multi else vr.FreeFlightGaussians(cam, 4)
    frames = []
    for kernel in (1, 2):
        for queue in (0, 16):
            device_options("ff_kernel", kernel)
            device_options("ff_nee_queue", queue)
            img = vr.Image(16, 16)
            integ.render(sc, img)
            st = integ.last_stats
            assert st["fallback_pixels"] == 0 and st["error_pixels"] == 0, st
            frames.append(img.pixels.copy())
            work = dev.count_work(integ.camera, integ.params, 16, 16)
            print(f"{config} multi {multi} ff_kernel {kernel} ff_nee_queue {queue}: {work}")
            if config == "wide":
                assert work["path"]["node2_steps"] > 0
    for f in frames[1:]:
        assert np.array_equal(bits(f), bits(frames[0]))
    ref = O.render_ff(oracle(), O.PINHOLE, pos, view, float(F.COMB_FOV), 16, 16, multi=multi, num_samples=4)
    assert np.abs(ref - np.float32(W.ENV)).max() > 0.01  # the frame sees the comb
    _check(frames[0], ref)


# ---- ray-march frame ----
@functools.lru_cache(maxsize=None)
def march_reference():
    _, pos, view = comb_camera()
    return O.render(oracle(False, True), O.PINHOLE, pos, view, float(F.COMB_FOV), 16, 16, O.RAYMARCH_GAUSSIANS, STEP, 3)


@pytest.mark.parametrize("sec_tight", [0, 1])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_ray_march_frame(config, sec_tight, device_options):
    """RayMarchingGaussians 16 x 16, 3 environment samples, t_eps 0, a second light inside the comb (slow rays):
    L-inf against the oracle < 1e-4 (the smoke frame's bound). The secondary walk of a ray from the comb to the first
    light needs 30 stack entries (simulated, test_wide_walk_reference.py): 16 more than VR_WW_STACK keeps in LDS."""
    device_options("sec_tight", sec_tight)
    dev, sc = on_device(device_options, config, inside_light=True)
    cam, _, _ = comb_camera()
    integ = vr.RayMarchingGaussians(cam, step_size=STEP, env_samples=3, t_eps=0.0)
    img = vr.Image(16, 16)
    integ.render(sc, img)
    st = integ.last_stats
    err = float(np.max(np.abs(img.pixels.astype(np.float64) - march_reference())))
    print(f"{config} sec_tight {sec_tight}: L-inf {err:.3e}, slow rays {st['slow_rays']}, secondary rays {st['secondary_rays']}")
    assert st["error_pixels"] == 0 and st["slow_rays"] > 0
    assert np.abs(march_reference() - np.float32(W.ENV)).max() > 0.01
    assert err < 1e-4


# ---- the secondary walk where its branch-free pushes end ----
THRESHOLD_PLANS = ["TFFFF", "EEETFFFF"]  # (the two of five tried whose frames were wrong before the fix)


def threshold_rays(tree, which):
    """walk_secondary of rays from points in the mirrored comb to its light on `tree`: (peaks, largest stack row a
    branch-free node step stores to)."""
    o = (W.CENTRE + np.random.default_rng(74).uniform(-0.4, 0.4, (64, 3)) * W.EXTENT).astype(np.float32)
    light = W.light_position(True).astype(np.float32)
    d = (light[None] - o).astype(np.float32)
    dist = np.linalg.norm(d.astype(np.float64), axis=1)
    S = W.slabs(tree, o, d, which=which)
    res = [W.walk_secondary(S, r, float(dist[r])) for r in range(len(o))]
    assert min(m for _, m, _ in res) > 2.0 ** -18
    return {p for p, _, _ in res}, {t for _, _, t in res}


@pytest.mark.parametrize("sec_tight", [0, 1])
@pytest.mark.parametrize("plan", THRESHOLD_PLANS)
def test_secondary_walk_where_its_branch_free_pushes_end(plan, sec_tight, device_options):
    """sec_node4v pushes branch-free while every lane has room: a store per slot at the running sp. In a mirrored
    comb the nearest child of a ray towards the light is the last slot, so a node entered with VR_WW_STACK - 3
    entries pushes three children and stores the fourth slot's ref at row VR_WW_STACK, which is the leaf
    queue's ring slot 0. Until the branch-free form was limited to lanes with room for 4, a leaf queued there was
    lost: these frames were 8.7e-4 and 1.5e-3 (4.7e-4 with the tight tree) from the oracle at every pixel; now
    1.2e-7 and 1.5e-7 (measured on an MI355X). 8 x 8, one environment sample, step 0.1, bound 1e-4."""
    device_options("device_bvh", 1)
    device_options("half_nodes", 1)
    device_options("sec_tight", sec_tight)
    arr = W.comb_arrays(leaf_max(), True, plan=plan)
    lp = W.light_position(True)
    sc = vr.Scene.from_gaussians(*arr, lights=[vr.Light(lp, W.LIGHT_INTENSITY)], env_color=W.ENV)
    dev = vr.Device.get(0)
    dev.upload(sc, force=True)
    tree = check_tree(dev, sc, "wide", mirrored=True)
    peaks, top = threshold_rays(tree, "hnodes4")
    print(f"{plan}: simulated on the shared tree from the root: peaks {peaks}, last row of a branch-free step {top}")
    assert top == {W.WW_STACK}
    orc = O.OracleScene.from_gaussians(*arr, [lp], [W.LIGHT_INTENSITY])
    orc.set_env(W.ENV)
    pos, view = F.camera_of("comb_back")
    ref = O.render(orc, O.PINHOLE, pos, view, float(F.COMB_FOV), 8, 8, O.RAYMARCH_GAUSSIANS, STEP, 1)
    integ = vr.RayMarchingGaussians(vr.Pinhole_Camera(pos, view, F.COMB_FOV), step_size=STEP, env_samples=1, t_eps=0.0)
    img = vr.Image(8, 8)
    integ.render(sc, img)
    err = float(np.max(np.abs(img.pixels.astype(np.float64) - ref)))
    print(f"{plan} sec_tight {sec_tight}: L-inf {err:.3e}, secondary rays {integ.last_stats['secondary_rays']}")
    assert integ.last_stats["error_pixels"] == 0 and np.abs(ref - np.float32(W.ENV)).max() > 0.01
    assert err < 1e-4
