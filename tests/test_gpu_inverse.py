"""GPU: RECORD_PIXEL_GAUSSIANS recording (integrator.h:616-644) and the stochastic finite-difference
inverse loop (inverse_integrator.h:61-246) on the device, through the C ABI, vs the oracle."""
import numpy as np
import pytest

import pyoracle as O
import sfd_replay as R
import vr_amd as vr
from vr_amd import inverse as inv
from helpers import CAM_POS, FOV, main_view_dir, scene_path

pytestmark = pytest.mark.gpu


def _cam():
    return vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)


@pytest.mark.parametrize("name,W,spp", [("50_random.txt", 32, 4), ("many_gaussians.txt", 32, 4),
                                        ("2_gaussian.txt", 24, 16)])
def test_recorded_pixel_gaussians_match_oracle(name, W, spp):
    path = scene_path(name)
    integ = vr.MultiScatterGaussians(_cam(), spp)
    img = vr.Image(W, W)
    integ.record(vr.Scene.load_GMM(path), img, slot=0)
    bits = integ.pixel_gaussian_bits(0)
    oimg, obits = O.render_ms_record(O.OracleScene.load_gmm(path), O.PINHOLE, CAM_POS, main_view_dir(), FOV, W, W, spp)
    assert bits.shape == obits.shape
    same = np.all(bits == obits, axis=0)
    print(f"pixels with identical Gaussian sets: {same.mean():.4f}, set bits {int(np.unpackbits(bits.view(np.uint8)).sum())}")
    assert same.mean() >= 0.99
    assert np.abs(img.pixels - oimg).max(axis=-1).mean() < 1e-4


def test_per_pixel_lists_and_plain_render_agree():
    path = scene_path("50_random.txt")
    scene = vr.Scene.load_GMM(path)
    integ = vr.MultiScatterGaussians(_cam(), 4)
    a, b = vr.Image(16, 16), vr.Image(16, 16)
    lists = []
    integ.render(scene, a, per_pixel_gaussians=lists)
    integ.render(scene, b)
    assert np.array_equal(a.pixels, b.pixels)  # recording does not change the image
    assert len(lists) == 256 and all(l == sorted(set(l)) for l in lists)
    assert any(len(l) for l in lists)


def test_sfd_loss_diff_matches_host_union_sum():
    path = scene_path("50_random.txt")
    scene = vr.Scene.load_GMM(path)
    n = scene.get_num_primitives()
    W = 32
    integ = vr.MultiScatterGaussians(_cam(), 4)
    ia, ib = vr.Image(W, W), vr.Image(W, W)
    integ.record(scene, ia, slot=0)
    b0 = integ.pixel_gaussian_bits(0)
    params = inv.pack_parameters(scene.gaussians())
    params[0::11] += 0.05
    integ.record(inv.apply_params(params, scene.lights, scene.env_color), ib, slot=1)
    b1 = integ.pixel_gaussian_bits(1)
    rng = np.random.default_rng(3)
    lb = rng.random(W * W).astype(np.float32)
    lp = rng.random(W * W).astype(np.float32)
    out = np.zeros(n, np.float64)
    import ctypes
    vr.check(vr.lib().vr_sfd_loss_diff(vr.Device.get(0)._h, lb.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                       lp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), W, W,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    ref = R.union_sum(b0, b1, lb, lp, n)
    np.testing.assert_allclose(out, ref, rtol=1e-9, atol=1e-9)


def test_sfd_optimize_runs_and_is_reproducible():
    path = scene_path("2_gaussian.txt")
    target = vr.Scene.load_GMM(path)
    W = 24
    I_ref = vr.Image(W, W)
    vr.MultiScatterGaussians(_cam(), 16).render(target, I_ref)
    p = inv.pack_parameters(target.gaussians())
    p[9::11] -= 0.7  # start from thinner Gaussians
    start = inv.apply_params(p, target.lights, target.env_color)
    runs = []
    for _ in range(2):
        opt = inv.StochasticFiniteDiffInverseIntegrator(_cam(), vr.MultiScatterGaussians(_cam(), 4),
                                                        inv.SFDConfig(max_iters=6, num_stoch_samples=2, lr=0.05, seed=1))
        assert opt.optimize(start, I_ref)
        assert np.all(np.isfinite(opt.history)) and np.all(np.isfinite(opt.params))
        assert opt.final_loss is not None and np.isfinite(opt.final_loss)  # final save (:229-238)
        assert opt.fwd.params.num_samples == 16384
        runs.append(opt.params.copy())
    assert np.array_equal(runs[0], runs[1])
    assert not np.array_equal(runs[0], p)


def test_sfd_run_with_grown_scales_does_not_abort():
    """An SFD run on 20k_bias.txt at 64x64 whose Gaussians start 8x wider than the scene's (log scales
    + ln 8): ~200-500 ellipsoids overlap a point, past the path kernel's 128-entry rows, and Adam
    moves the scales further every iteration. The reference's event lists are unbounded
    (gmm.h:457-515, integrator.h:422-498), so the optimisation must run to the end: those paths re-run
    in ff_fallback_kernel instead of failing the render."""
    path = scene_path("20k_bias.txt")
    target = vr.Scene.load_GMM(path)
    W = 64
    I_ref = vr.Image(W, W)
    vr.MultiScatterGaussians(_cam(), 4).render(target, I_ref)
    p = inv.pack_parameters(target.gaussians())
    p[6::11] += np.float32(np.log(8.0))
    p[7::11] += np.float32(np.log(8.0))
    p[8::11] += np.float32(np.log(8.0))
    start = inv.apply_params(p, target.lights, target.env_color)
    probe = vr.MultiScatterGaussians(_cam(), 4)
    probe.render(start, vr.Image(W, W))
    print("paths re-run with the large rows:", probe.last_stats["fallback_pixels"])
    assert probe.last_stats["fallback_pixels"] > 0  # the start scene already needs the large rows
    opt = inv.StochasticFiniteDiffInverseIntegrator(_cam(), vr.MultiScatterGaussians(_cam(), 4),
                                                    inv.SFDConfig(max_iters=4, num_stoch_samples=2, lr=0.05, seed=3,
                                                                  final_samples=16))
    assert opt.optimize(start, I_ref)
    assert len(opt.history) == 4 and np.all(np.isfinite(opt.history))
    assert np.all(np.isfinite(opt.params)) and np.isfinite(opt.final_loss)
    assert not np.array_equal(opt.params[6::11], p[6::11])  # the scales moved


# ---- BASELINE config 5: scenes/gaussians/10k_random.txt at 512x512 ------------------------------
C5_W = 512
C5_SPP = 4


def _oracle_scene(scene):
    g = scene.gaussians()
    return O.OracleScene.from_gaussians(g[:, 0:3], g[:, 3:9], g[:, 9], g[:, 10],
                                        np.array([l.position for l in scene.lights], np.float32),
                                        np.array([l.intensity for l in scene.lights], np.float32))


def _same_sets(bits, obits):
    return np.all(bits == obits, axis=0)


@pytest.mark.timeout(600)
def test_c5_recording_matches_oracle_full_frame():
    """MultiScatterGaussians with RECORD_PIXEL_GAUSSIANS on the C5 scene, whole 512x512 frame: the
    recorded Gaussian set of every pixel and the image against the oracle."""
    path = scene_path("10k_random.txt")
    scene = vr.Scene.load_GMM(path)
    assert scene.get_num_primitives() == 10_000
    integ = vr.MultiScatterGaussians(_cam(), C5_SPP)
    img = vr.Image(C5_W, C5_W)
    integ.record(scene, img, slot=0)
    bits = integ.pixel_gaussian_bits(0)
    osc = O.OracleScene.load_gmm(path)
    res = {}
    for order in ("reference", "stable"):
        if order == "stable":
            with O.stable_ties():  # tangent-hit ties in emission order: the device's rule (see helpers)
                oimg, obits = O.render_ms_record(osc, O.PINHOLE, CAM_POS, main_view_dir(), FOV, C5_W, C5_W, C5_SPP)
        else:
            oimg, obits = O.render_ms_record(osc, O.PINHOLE, CAM_POS, main_view_dir(), FOV, C5_W, C5_W, C5_SPP)
        same = _same_sets(bits, obits)
        d = np.abs(img.pixels.astype(np.float64) - oimg).max(axis=-1).reshape(-1)
        res[order] = (same.mean(), np.mean(d < 1e-4), d.mean())
        print(f"C5 512x512/10k vs the {order}-order oracle: identical Gaussian sets on {same.mean():.5f} of "
              f"{same.size} pixels; pixels within 1e-4 {np.mean(d < 1e-4):.5f}, mean |d| {d.mean():.3e}, "
              f"max {d.max():.3e}")
    # Free-flight paths can part ways on a libm ulp, so the bar is statistical; against the stable tie
    # order (the device's rule for tangent hits, helpers.tie_aware_linf) it is tight.
    for order in res:
        assert res[order][0] >= 0.99 and res[order][1] >= 0.99 and res[order][2] < 1e-4
    assert res["stable"][0] >= 0.9995 and res["stable"][1] >= 0.998 and res["stable"][2] < 1e-5


@pytest.mark.timeout(900)
def test_c5_one_sfd_iteration_matches_oracle():
    """One StochasticFiniteDiffInverseIntegrator iteration (inverse_integrator.h:114-200) on C5: the
    native device loop (vr_sfd_optimize: recorded renders, device losses and union statistic, device
    BVH re-uploads) against the same iteration assembled from the oracle's recorded renders, a host
    union-of-pixels sum and the reference's Adam update (optimizer.h:31-50) — base loss, gradient
    estimate and updated parameters."""
    from vr_amd import inverse as inv
    target = vr.Scene.load_GMM(scene_path("10k_random.txt"))
    I_ref = vr.Image(C5_W, C5_W)
    vr.MultiScatterGaussians(_cam(), C5_SPP).render(target, I_ref)
    p0 = inv.pack_parameters(target.gaussians())
    p0[9::11] += np.float32(np.log(0.5))  # start from half densities
    start = inv.apply_params(p0, target.lights, target.env_color)
    cfg = inv.SFDConfig(max_iters=1, num_stoch_samples=2, lr=1e-2, seed=7, final_samples=0)
    opt = inv.StochasticFiniteDiffInverseIntegrator(_cam(), vr.MultiScatterGaussians(_cam(), C5_SPP), cfg)
    assert opt.optimize(start, I_ref)

    # the same iteration from the oracle
    params = inv.pack_parameters(start)
    eps = inv.make_default_eps_for_params(params)
    n = start.get_num_primitives()

    def rec(scene):
        img, bits = O.render_ms_record(_oracle_scene(scene), O.PINHOLE, CAM_POS, main_view_dir(), FOV, C5_W, C5_W,
                                       C5_SPP)
        im = vr.Image(C5_W, C5_W)
        im.pixels[...] = img
        return inv.compute_pixel_losses(im, I_ref), bits

    with O.stable_ties():  # the device's tie rule (tangent hits in emission order)
        lb, b0 = rec(start)
        grads = np.zeros(params.size, np.float64)
        for k in range(cfg.num_stoch_samples):
            s = inv.sign_vector(cfg.seed, k, params.size)
            lp, b1 = rec(inv.apply_params((params + s * eps).astype(np.float32), start.lights, start.env_color))
            fdiff = R.union_sum(b0, b1, lb, lp, n)
            grads += np.repeat(fdiff, inv.PER) * s.astype(np.float64) / eps.astype(np.float64)
        grads /= cfg.num_stoch_samples
    # Adam's first step (optimizer.h:31-50): m = (1-b1) g, v = (1-b2) g^2, a = lr sqrt(1-b2) / (1-b1)
    g = grads.astype(np.float32)
    m = (np.float32(1) - np.float32(0.9)) * g
    v = (np.float32(1) - np.float32(0.999)) * g * g
    a = np.float32(1e-2) * np.sqrt(np.float32(1) - np.float32(0.999)) / (np.float32(1) - np.float32(0.9))
    p_ref = params - (a * (m / (np.sqrt(v) + np.float32(1e-8)))).astype(np.float32)

    base_rel = abs(opt.history[0] - float(lb.astype(np.float64).mean())) / float(lb.mean())
    gmax = float(np.abs(grads).max())
    gerr = float(np.abs(opt.last_grads - grads).max())
    big = np.abs(grads) > 1e-3 * gmax
    pdiff = np.abs(opt.params - p_ref)
    print(f"C5 SFD iteration: base loss rel diff {base_rel:.2e}; grad max|g| {gmax:.3e}, max|dg| {gerr:.3e}; "
          f"{big.mean():.4f} of parameters with |g| > 1e-3 max; param update identical on "
          f"{np.mean(pdiff[big] <= 1e-6):.5f} of them")
    # a few of the 4 x 262144 paths per render part ways on a libm ulp (see the recording test), so the
    # losses agree to ~1e-5 and the SFD sums to a few 1e-3 of the largest gradient, and Adam's first
    # step (a sign step, |update| = lr) is identical wherever the gradient is not near 0
    assert base_rel < 1e-4
    assert gerr <= 1e-2 * gmax
    assert np.mean(pdiff[big] <= 1e-6) >= 0.999


def test_sfd_on_a_multi_device_context_equals_single_device():
    """vr_sfd_optimize on a multi-device context spreads an iteration's perturbed renders over the ranks
    (each rank uploads its own perturbed scene with the device BVH build, renders and records from a
    host thread of its own; the base render and the union statistic on the first). The result must not
    depend on the number of ranks: parameters, loss history and the last gradient bit-equal to the
    single-device run with the same seed."""
    path = scene_path("2_gaussian.txt")
    target = vr.Scene.load_GMM(path)
    W = 24
    I_ref = vr.Image(W, W)
    vr.MultiScatterGaussians(_cam(), 16).render(target, I_ref)
    p = inv.pack_parameters(target.gaussians())
    p[9::11] -= 0.7
    start = inv.apply_params(p, target.lights, target.env_color)
    runs = {}
    for devices in (0, (0, 0), (0, 0, 0)):
        opt = inv.StochasticFiniteDiffInverseIntegrator(
            _cam(), vr.MultiScatterGaussians(_cam(), 4, device=devices),
            inv.SFDConfig(max_iters=4, num_stoch_samples=3, lr=0.05, seed=5, final_samples=64))
        assert opt.optimize(start, I_ref)
        runs[devices] = (opt.params.copy(), np.array(opt.history), np.array(opt.last_grads))
    base = runs[0]
    for devices in ((0, 0), (0, 0, 0)):
        for a, b in zip(base, runs[devices]):
            assert np.array_equal(a, b), devices


# ---- the loop against its replay (tests/sfd_replay.py) ------------------------------------------
def _camera(pos, lookat, fov):
    d = np.float32(lookat) - np.float32(pos)
    return vr.Pinhole_Camera(np.float32(pos), (d / np.sqrt(np.float32(np.dot(d, d)))).astype(np.float32), np.float32(fov))


MAIN_CAM = (CAM_POS, (0.0, 1.0, 0.0), FOV)


def synthetic_scene(n, seed, wide_first=False):
    """n seeded Gaussians: the first at the main camera's look-at point, the others spread over its frame
    (sigma 0.04 .. 0.25 per axis, rotated by a random angle about a random axis, density 0.5 .. 3, albedo
    0.3 .. 0.95, one white light); for n >= 8 the last one lies at x = 2000, outside every frame and 1e-7 of a
    scattered path's sphere of directions: it is recorded at no pixel. wide_first: the first one has sigma 0.6,
    0.7, 0.4 along x, y, z, so that it is met even by the four paths of a 1 x 1 frame."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform([-2.4, -1.4, -1.0], [2.4, 3.4, 1.0], (n, 3))
    mean[0] = (0.0, 1.0, 0.0)
    if n >= 8:
        mean[-1] = (2000.0, 1.0, 0.0)
    cov6 = np.empty((n, 6))
    for i in range(n):
        a = rng.normal(size=3)
        a /= np.sqrt(a @ a)
        th = rng.uniform(0.0, np.pi)
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        Q = np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(a, a)
        C = Q @ np.diag(rng.uniform(0.04, 0.25, 3) ** 2) @ Q.T
        cov6[i] = C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]
    if wide_first:
        cov6[0] = 0.36, 0, 0, 0.49, 0, 0.16
    return vr.Scene.from_gaussians(mean, cov6, rng.uniform(0.5, 3.0, n), rng.uniform(0.3, 0.95, n),
                                   lights=[vr.Light((0.0, 4.0, 0.0), (1.0, 1.0, 1.0))])


SFD_SEED, SFD_K, SFD_LR = 1, 2, 0.05
SFD_ALL_RECORDED = ("2_gaussian",)
# name -> target scene, log-density offset of the start, frame, paths per pixel, camera (position, look-at, fov).
# The cameras and the synthetic seeds were chosen on the CPU with pyoracle.render_ms_record so that every case
# meets the conditions test_sfd_loop_equals_its_replay asserts from the replay's own bitsets.
SFD_CASES = {
    # n = 2: one word, 30 padding bits. The two Gaussians cross at (0, 1, 0) and every path scattered in one
    # crosses the other, so no camera leaves one of them unrecorded while the other has a gradient (searched on
    # the CPU: aims along both arms, pinholes in front of, inside and behind the pair): this case alone is
    # exempt from the unrecorded-Gaussian condition.
    "2_gaussian": (lambda: vr.Scene.load_GMM(scene_path("2_gaussian.txt")), -0.7, 24, 24, 4, MAIN_CAM),
    # two words, one chunk. The camera looks at the cloud's rim at x = 1.5 with its pinhole at z = 1.5, just in
    # front of the Gaussians: three of them on the far side are recorded at no pixel.
    "50_random": (lambda: vr.Scene.load_GMM(scene_path("50_random.txt")), np.log(0.5), 32, 32, 4,
                  ((1.5, 1.0, 6.0), (1.5, 1.0, 0.0), 2.0 * np.arctan(1.0 / 4.5))),
    # n a multiple of 32; 4680 pixels = two chunks, the second partial, not a multiple of 256
    "synthetic_64": (lambda: synthetic_scene(64, 1), np.log(0.5), 72, 65, 4, MAIN_CAM),
    # four words, the last holds 1 bit; 1 path per pixel gives sparse recordings
    "synthetic_97": (lambda: synthetic_scene(97, 2), np.log(0.5), 72, 65, 1, MAIN_CAM),
}
_SFD_RUNS = {}


def _sfd_setup(name):
    make, dlog, W, H, spp, cam = SFD_CASES[name]
    target = make()
    I_ref = vr.Image(W, H)
    vr.MultiScatterGaussians(_camera(*cam), 16).render(target, I_ref)
    p0 = inv.pack_parameters(target)
    p0[9::11] += np.float32(dlog)
    start = inv.apply_params(p0, None, None, base=target)
    return start, I_ref, _camera(*cam), spp


def _sfd_run(start, I_ref, cam, spp, iters, **kw):
    cfg = inv.SFDConfig(**{"max_iters": iters, "num_stoch_samples": SFD_K, "lr": SFD_LR, "seed": SFD_SEED,
                           "final_samples": 0, **kw})
    opt = inv.StochasticFiniteDiffInverseIntegrator(cam, vr.MultiScatterGaussians(cam, spp), cfg)
    assert opt.optimize(start, I_ref)
    return opt


def _sfd_case(name):
    """The case's start scene and reference image and its three native runs (max_iters = 1, 2, 3), made once."""
    if name not in _SFD_RUNS:
        start, I_ref, cam, spp = _sfd_setup(name)
        runs = {j: _sfd_run(start, I_ref, cam, spp, j) for j in (1, 2, 3)}
        _SFD_RUNS[name] = (start, I_ref, cam, spp, runs)
    return _SFD_RUNS[name]


def _adam(p, g, m, v, t):
    import ctypes
    fp = ctypes.POINTER(ctypes.c_float)
    vr.check(vr.lib().vr_adam_step(p.ctypes.data_as(fp), g.ctypes.data_as(fp), m.ctypes.data_as(fp), v.ctypes.data_as(fp),
                                   p.size, t, SFD_LR, 0.9, 0.999, 1e-8))


@pytest.mark.parametrize("name", list(SFD_CASES))
def test_sfd_loop_equals_its_replay(name, device_options):
    """vr_sfd_optimize with max_iters = 1, 2, 3 (parameters P_j, last gradient G_j, history H_j) against iteration
    j replayed from outside (sfd_replay.replay_iteration) from the native P_{j-1}: the renders are the device's
    own, so no path can part ways and every comparison is exact.
      * the three histories are prefixes of one another bit for bit, and H[j-1] is the sequential double mean of
        the replay's base losses, bit for bit;
      * |G_j - replay gradient| <= sum_k npix 2^-52 sum_p |lp - lb| / (eps K) per parameter: both sides add the
        same doubles, the device in wave / chunk order (derived; nothing measured);
      * P_j is bit-equal to vr_adam_step(P_{j-1}, f32(G_j), m, v, t = j) with m, v carried through
        f32(G_1 .. G_{j-1}), and within adam_margin of the float64 Adam on the same inputs (a wrong t or stale
        moments in the loop fail this)."""
    start, I_ref, cam, spp, runs = _sfd_case(name)
    device_options("device_bvh", 1)  # the loop forces it
    n = start.get_num_primitives()
    W, H = I_ref.get_width(), I_ref.get_height()
    npix = W * H
    integ = vr.MultiScatterGaussians(cam, spp)
    P0 = inv.pack_parameters(start)
    eps = inv.make_default_eps_for_params(P0).astype(np.float64)
    for a, b in ((1, 2), (2, 3)):
        assert runs[a].history == runs[b].history[:a]
    p, m, v = P0.copy(), np.zeros(P0.size, np.float32), np.zeros(P0.size, np.float32)
    worst_g = worst_ulp = 0.0
    for j in (1, 2, 3):
        opt = runs[j]
        cfg = inv.SFDConfig(num_stoch_samples=SFD_K, seed=SFD_SEED)
        lb, grad, per_k = R.replay_iteration(integ, start, None if j == 1 else runs[j - 1].params, I_ref, j - 1, cfg)
        assert len(opt.history) == j and opt.history[j - 1] == R.sequential_mean(lb), j
        # the conditions of the case, from the replay's own bitsets
        rec = np.zeros(n, bool)
        differ = np.zeros(n, bool)
        both_chunks = np.zeros(n, bool)
        bound = np.zeros(P0.size)
        for lp, fd, b0, b1 in per_k:
            u = R.unpack_bits(b0 | b1, n)
            rec |= u.any(axis=0)
            differ |= np.any(R.unpack_bits(b0 ^ b1, n), axis=0)
            both_chunks |= u[:4096].any(axis=0) & u[4096:].any(axis=0)
            assert np.all(fd[~u.any(axis=0)] == 0.0)
            bound += np.repeat(npix * 2.0 ** -52 * R.union_abs_sum(b0, b1, lb, lp, n), 11) / (eps * SFD_K)
        G = opt.last_grads
        assert (~rec).any() or name in SFD_ALL_RECORDED, j
        assert np.all(G[np.repeat(~rec, 11)] == 0.0), j
        assert differ.any(), j
        assert np.mean(np.abs(G) > 1e-3 * np.abs(G).max()) >= 0.10, j
        if npix > 4096:
            assert both_chunks.any(), j
        # gradient
        dG = np.abs(G - grad)
        assert np.all(dG <= bound), (j, float((dG - bound).max()))
        worst_g = max(worst_g, float(np.max(dG[bound > 0] / bound[bound > 0])))
        # Adam: bit-equal to the native step, and within the margin of the float64 step on the same inputs
        assert np.array_equal(p, P0 if j == 1 else runs[j - 1].params), j
        gf = G.astype(np.float32)
        p64, _, _ = R.adam64(p, gf, m, v, j, SFD_LR)
        p_before = p.copy()
        _adam(p, gf, m, v, j)
        assert np.array_equal(opt.params, p), j
        live = p64 != p_before  # (a parameter without a gradient so far does not move: the far Gaussian's mean
        assert np.array_equal(opt.params[~live], p_before[~live]), j  # stays out of the margin's max |p|)
        assert np.all(np.abs(opt.params - p64)[live] <= R.adam_margin(p_before[live], p64[live])), j
        worst_ulp = max(worst_ulp, float(np.abs(opt.params - p64)[live].max()) / R.ulp32(np.abs(p_before[live]).max()))
        assert not np.array_equal(opt.params, p_before)
        print(f"{name} iteration {j}: loss {opt.history[j - 1]:.6e}, {int((~rec).sum())} of {n} Gaussians recorded nowhere, "
              f"{int(differ.sum())} with bits0 != bits1, {int(both_chunks.sum())} in both chunks, "
              f"{np.mean(np.abs(G) > 1e-3 * np.abs(G).max()):.2f} of |G| > 1e-3 max")
    print(f"{name}: max |dG| / bound {worst_g:.3e}, max Adam distance {worst_ulp:.2f} ulp_f32(max |p|)")


def test_sfd_gradient_above_one_chunk_is_the_same_twice():
    """72 x 65 is two pixel chunks of the union-sum kernel: the same run again gives the same last gradient and
    parameters bit for bit (the kernel's partial sums are added in a fixed order)."""
    start, I_ref, cam, spp, runs = _sfd_case("synthetic_64")
    again = _sfd_run(start, I_ref, cam, spp, 1)
    assert np.array_equal(again.last_grads, runs[1].last_grads)
    assert np.array_equal(again.params, runs[1].params) and again.history == runs[1].history


# ---- the union-sum kernel exactly (vr_sfd_loss_diff) --------------------------------------------
def _loss_diff(dev, lb, lp, W, H, n):
    import ctypes
    fp = ctypes.POINTER(ctypes.c_float)
    out = np.full(max(n, 1), -1.0, np.float64)
    lb, lp = np.ascontiguousarray(lb, np.float32), np.ascontiguousarray(lp, np.float32)
    vr.check(vr.lib().vr_sfd_loss_diff(dev._h, lb.ctypes.data_as(fp), lp.ctypes.data_as(fp), W, H,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    return out[:n]


def _record_on(dev, scene, W, H, slot, spp=4):
    """Upload, record into `slot` and read the bitset back on the given context (a fresh vr_init one, or cuda:0's)."""
    import ctypes
    integ = vr.MultiScatterGaussians(_cam(), spp)
    dev.upload(scene, force=True)
    dev.set_option("ff_solver", vr.SOLVERS[integ.solver])
    out = np.empty((H, W, 3), np.float32)
    vr.check(vr.lib().vr_render_record(dev._h, ctypes.byref(integ.camera.struct), ctypes.byref(integ.params), W, H,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), slot))
    n = scene.get_num_primitives()
    bits = np.zeros(((n + 31) // 32, W * H), np.uint32)
    buf = bits if bits.size else np.zeros(1, np.uint32)
    vr.check(vr.lib().vr_get_pixel_gaussians(dev._h, slot, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), bits.size))
    return out, bits


def _shifted(scene, dx=0.05):
    g = scene.gaussians()
    return vr.Scene.from_gaussians(g[:, 0:3] + np.float32([dx, 0, 0]), g[:, 3:9], g[:, 9], g[:, 10], lights=scene.lights)


def _integer_losses(npix):
    return np.zeros(npix, np.float32), np.arange(1, npix + 1, dtype=np.float32)


@pytest.mark.parametrize("n,W,H", [(1, 1, 1), (31, 17, 5), (32, 64, 64), (33, 65, 64), (64, 72, 65), (97, 128, 96),
                                   (1, 128, 96), (97, 1, 1), (33, 17, 5), (64, 64, 64), (31, 72, 65)])
def test_sfd_loss_diff_is_exact_on_integer_losses(n, W, H):
    """sfd_loss_diff_kernel through vr_sfd_loss_diff on recordings of a scene and of its shifted copy, with
    loss_base = 0 and loss_plus[p] = p + 1: integers, exact in f32 and in every double partial sum, so the result
    is bit-equal to the host union sum whatever the order of the additions, and a dropped or doubled pixel shows as
    its own index. 64 x 64 is exactly one 4096-pixel chunk, 65 x 64 and 72 x 65 end in a partial chunk (72 x 65 is
    no multiple of 256), 128 x 96 is three full chunks. Also: the bits at positions >= n of the last word are
    zero, and recording into slot 1 leaves slot 0's words as they were."""
    scene = synthetic_scene(n, 3, wide_first=True)
    dev = vr.Device.get(0)
    _, b0 = _record_on(dev, scene, W, H, 0)
    _, b1 = _record_on(dev, _shifted(scene), W, H, 1)
    integ = vr.MultiScatterGaussians(_cam(), 4)
    integ._rec_shape = (n, W * H)
    assert np.array_equal(integ.pixel_gaussian_bits(0), b0)  # slot 0 after the recording into slot 1
    if n % 32:
        assert not np.any(b0[-1] >> np.uint32(n % 32)) and not np.any(b1[-1] >> np.uint32(n % 32))
    lb, lp = _integer_losses(W * H)
    ref = R.union_sum(b0, b1, lb, lp, n)
    assert ref[0] > 0  # the wide Gaussian is met in every frame
    if n >= 8:
        assert ref[-1] == 0.0  # the last one is recorded nowhere
    if W * H >= 4096:
        assert np.count_nonzero(ref) >= n // 2 and np.any(b0 != b1)
    out = _loss_diff(dev, lb, lp, W, H, n)
    assert np.array_equal(out, ref), np.nonzero(out != ref)[0][:8]
    # the base recording alone (slot 1 a copy of slot 0's render): the union is bits0
    _, b1 = _record_on(dev, scene, W, H, 1)
    assert np.array_equal(b1, b0)
    assert np.array_equal(_loss_diff(dev, lb, lp, W, H, n), R.union_sum(b0, b0, lb, lp, n))


def test_sfd_loss_diff_rounds_the_same_way_in_every_call():
    """Losses from 1e-9 to 1 (their double sums round, unlike the sums of a frame's similar-sized losses, which are
    mostly exact) on three full chunks: sixteen calls give one result bit for bit, since the kernel adds its wave
    and chunk partial sums in a fixed order, and it lies within npix 2^-52 sum |lp - lb| of the host sum. (With one
    atomicAdd per wave in arrival order, 300 calls gave 300 different results on an MI355X.)"""
    n, W, H = 97, 128, 96
    scene = synthetic_scene(n, 3, wide_first=True)
    dev = vr.Device.get(0)
    _, b0 = _record_on(dev, scene, W, H, 0)
    _, b1 = _record_on(dev, _shifted(scene), W, H, 1)
    rng = np.random.default_rng(0)
    lb = (10.0 ** rng.uniform(-9, 0, W * H)).astype(np.float32)
    lp = (10.0 ** rng.uniform(-9, 0, W * H)).astype(np.float32)
    outs = [_loss_diff(dev, lb, lp, W, H, n) for _ in range(16)]
    assert all(np.array_equal(o, outs[0]) for o in outs)
    ref = R.union_sum(b0, b1, lb, lp, n)
    assert np.any(outs[0] != ref)  # the sums do round: the order matters here
    assert np.all(np.abs(outs[0] - ref) <= W * H * 2.0 ** -52 * R.union_abs_sum(b0, b1, lb, lp, n))


def test_rerecording_a_smaller_scene_and_frame_leaves_no_stale_bits():
    """Slots that held n = 97 at 72 x 65 are recorded again with n = 33 at 17 x 5: the words equal a fresh
    context's recording of the same renders, and the union sum of the small recordings is exact."""
    dev = vr.Device.get(0)
    big, small = synthetic_scene(97, 3), synthetic_scene(33, 3)
    for slot, sc in ((0, big), (1, _shifted(big))):
        _record_on(dev, sc, 72, 65, slot)
    img0, b0 = _record_on(dev, small, 17, 5, 0)
    img1, b1 = _record_on(dev, _shifted(small), 17, 5, 1)
    fresh = vr.Device(0)
    fimg0, f0 = _record_on(fresh, small, 17, 5, 0)
    fimg1, f1 = _record_on(fresh, _shifted(small), 17, 5, 1)
    assert np.array_equal(b0, f0) and np.array_equal(b1, f1) and b0.any()
    assert np.array_equal(img0, fimg0) and np.array_equal(img1, fimg1)
    lb, lp = _integer_losses(17 * 5)
    ref = R.union_sum(b0, b1, lb, lp, 33)
    assert np.array_equal(_loss_diff(dev, lb, lp, 17, 5, 33), ref)
    assert np.array_equal(_loss_diff(fresh, lb, lp, 17, 5, 33), ref)


def test_recording_an_empty_scene_sets_no_bits():
    """A scene without Gaussians records zero words and its union sum is empty; a scene whose only Gaussians lie
    outside the frame records no bit at any pixel, and its sums are exactly 0."""
    dev = vr.Device.get(0)
    empty = vr.Scene(vr.Scene.GAUSSIANS)
    for slot in (0, 1):
        img, bits = _record_on(dev, empty, 16, 16, slot)
        assert bits.shape == (0, 256)
        assert np.all(img == img[0, 0])
    lb, lp = _integer_losses(256)
    assert _loss_diff(dev, lb, lp, 16, 16, 0).size == 0
    g = synthetic_scene(40, 3).gaussians()
    away = vr.Scene.from_gaussians(g[:, 0:3] + np.float32([40, 0, 0]), g[:, 3:9], g[:, 9], g[:, 10])
    for slot in (0, 1):
        _, bits = _record_on(dev, away, 16, 16, slot)
        assert bits.shape == (2, 256) and not bits.any()
    assert np.array_equal(_loss_diff(dev, lb, lp, 16, 16, 40), np.zeros(40))


def test_sfd_loss_diff_refuses_mismatched_recordings():
    dev = vr.Device.get(0)
    five, three = synthetic_scene(5, 3), synthetic_scene(3, 3)
    lb, lp = _integer_losses(256)

    def refused(d, W, H, n):
        with pytest.raises(vr.VRError) as e:
            _loss_diff(d, lb[:W * H], lp[:W * H], W, H, n)
        assert e.value.status == vr.L.VR_ERR_INVALID

    _record_on(dev, five, 16, 16, 0)
    _record_on(dev, five, 8, 8, 1)
    refused(dev, 16, 16, 5)  # the slots hold different frame sizes
    refused(dev, 8, 8, 5)
    _record_on(dev, three, 16, 16, 1)
    refused(dev, 16, 16, 5)  # the slots hold different n
    refused(dev, 16, 16, 3)
    _record_on(dev, five, 16, 16, 1)
    refused(dev, 16, 16, 4)  # n is not the recorded count
    refused(dev, 16, 16, 6)
    assert _loss_diff(dev, lb, lp, 16, 16, 5).shape == (5,)  # and the matching call is served
    fresh = vr.Device(0)
    refused(fresh, 16, 16, 5)  # nothing recorded yet
    _record_on(fresh, five, 16, 16, 0)
    refused(fresh, 16, 16, 5)  # slot 1 never recorded


# ---- what the loop leaves behind and writes -----------------------------------------------------
def test_sfd_outputs_final_image_loss_and_saved_frames(tmp_path, device_options):
    """2_gaussian 24 x 24, max_iters 3, save_every 2, final_samples 8: final_image is a plain 8-path render of
    the optimised scene (device BVH), final_loss the sequential double mean of its pixel losses, iter_0000.ppm
    the PPM of a plain render of P_1, iter_0002.ppm the final image (the final save overwrites it,
    inverse_integrator.h:229-232), iter_0001.ppm absent; the device_bvh option is as before afterwards."""
    start, I_ref, cam, spp, runs = _sfd_case("2_gaussian")
    dev = vr.Device.get(0)
    device_options("device_bvh", 0)
    opt = _sfd_run(start, I_ref, cam, spp, 3, save_every=2, final_samples=8, out_dir=str(tmp_path))
    assert dev.get_option("device_bvh") == 0
    assert np.array_equal(opt.params, runs[3].params) and opt.history == runs[3].history
    assert sorted(f.name for f in tmp_path.iterdir()) == ["iter_0000.ppm", "iter_0002.ppm"]
    device_options("device_bvh", 1)
    plain = vr.Image(24, 24)
    vr.MultiScatterGaussians(cam, 8).render(opt.scene, plain)
    assert np.array_equal(opt.final_image.pixels, plain.pixels)
    assert opt.final_loss == R.sequential_mean(inv.compute_pixel_losses(opt.final_image, I_ref))
    assert opt.fwd.params.num_samples == 8
    opt.final_image.make_PPM(tmp_path / "final.ppm")
    assert (tmp_path / "iter_0002.ppm").read_bytes() == (tmp_path / "final.ppm").read_bytes()
    first = vr.Image(24, 24)
    vr.MultiScatterGaussians(cam, spp).render(inv.apply_params(runs[1].params, None, None, base=start), first)
    first.make_PPM(tmp_path / "first.ppm")
    assert (tmp_path / "iter_0000.ppm").read_bytes() == (tmp_path / "first.ppm").read_bytes()
    assert first.to_uint8().any()


def test_sfd_refused_calls_leave_the_device_bvh_option(device_options):
    start, I_ref, cam, spp, _ = _sfd_case("2_gaussian")
    dev = vr.Device.get(0)
    for value in (0, 1):
        device_options("device_bvh", value)
        with pytest.raises(vr.VRError) as e:
            _sfd_run(start, I_ref, cam, spp, 1, num_stoch_samples=0)
        assert e.value.status == vr.L.VR_ERR_INVALID and dev.get_option("device_bvh") == value
        opt = inv.StochasticFiniteDiffInverseIntegrator(cam, vr.MultiScatterGaussians(cam, spp),
                                                        inv.SFDConfig(max_iters=1, num_stoch_samples=SFD_K, final_samples=0))
        opt.fwd.params.integrator = vr.L.VR_FREE_FLIGHT  # the forward integrator is not MultiScatterGaussians
        with pytest.raises(vr.VRError) as e:
            opt.optimize(start, I_ref)
        assert e.value.status == vr.L.VR_ERR_INVALID and dev.get_option("device_bvh") == value


def test_sfd_with_no_iterations_returns_the_initial_parameters(device_options):
    start, I_ref, cam, spp, _ = _sfd_case("2_gaussian")
    opt = _sfd_run(start, I_ref, cam, spp, 0, final_samples=8)
    assert opt.history == [] and opt.last_grads is None
    assert np.array_equal(opt.params, inv.pack_parameters(start))
    device_options("device_bvh", 1)
    plain = vr.Image(24, 24)
    vr.MultiScatterGaussians(cam, 8).render(start, plain)  # the initial scene itself, not apply(pack(initial))
    assert np.array_equal(opt.final_image.pixels, plain.pixels)
    assert opt.final_loss == R.sequential_mean(inv.compute_pixel_losses(opt.final_image, I_ref))
