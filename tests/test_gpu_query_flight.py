"""The free-flight query (Device.query_free_flight over vr_query_free_flight[_device]) against the oracle's
per-path record of a MultiScatterGaussians frame (tests/flight_reference.py: the oracle's exact rays with unit = 1,
its exact targets, and a float64 closed-form model that judges the answers), then the query's structural
properties. Conditions per case (flight_reference.judge):
  1. t == -1 exactly where the oracle's path escapes, on every ray;
  2. |exp(-tau64(t_dev)) - exp(-tau64(t_orc))| <= 1e-4 on the scattering rays, at most one ray per case over it
     (a segment decision within an ulp of libm);
  3. |albedo - albedo64(t_dev)| <= 1e-4 and n_active == the number of Gaussians with max(t0, 0) <= t_dev < t1,
     but for at most 2 rays whose t lies within 1e-5 of an entry or exit distance.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import flight_reference as R
from helpers import CAM_POS, ROOT, scene_path

pytestmark = pytest.mark.gpu

F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def device():
    import vr_amd as vr
    return vr.Device.get(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ask(name):
    return R.ask(device(), name)


@functools.lru_cache(maxsize=None)
def baseline(name):
    """The default-option answer (t, albedo, n_active) to the case's rays, shared by the structural tests."""
    out = ask(name)
    for a in out:
        a.setflags(write=False)
    return out


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------
# against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_matches_the_oracle_record(name):
    """Conditions 1-3 with the reference's solver (ANALYTIC_PLUS_NEWTON). The slab needs several hit windows per
    ray; coincident200 runs every scattering ray through the second, 1024-row launch.
    Measured on an MI355X (max |dTr|, rays over the bound, share of bit-identical t, max |dt|, max |albedo - model|,
    active counts, rays skipped near an event):
      250_random        3.4e-6  0  86.5 %  1.4e-6  4.4e-7  1..9      0
      1000_random       3.5e-6  0  88.2 %  9.5e-7  4.4e-7  1..18     0
      many_gaussians    7.0e-7  0  90.9 %  4.8e-7  4.2e-7  1..3      0
      250_random_ortho  2.8e-6  0  90.6 %  1.4e-6  1.3e-7  1..10     0
      slab              1.0e-6  0  86.8 %  3.3e-6  3.8e-7  10..86    1
      coincident200     4.9e-5  0  67.8 %  1.7e-5  3.8e-6  200..200  0
    (the share and |dt| are records, not assertions: erf / exp / log come from the device library)"""
    t, alb, na = ask(name)
    assert t.dtype == np.float32 and alb.dtype == np.float32 and na.dtype == np.int32 and t.shape == alb.shape == na.shape == (256,)
    R.judge(name, t, alb, na)


@pytest.mark.parametrize("solver", [1, 2, 3])
@pytest.mark.parametrize("name", ["250_random", "many_gaussians"])
def test_solver_modes_match_the_oracle(name, solver, device_options):
    """VR_OPT_FF_SOLVER 1 (bisection), 2 (Newton), 3 (analytic + bisection) against orc_set_solver(mode): conditions
    1-3. Measured on an MI355X (max |dTr|, rays over the bound, share of bit-identical t, max |dt|):
      250_random      1: 9.8e-8 0 99.5 % 1.4e-6   2: 3.4e-6 0 82.0 % 2.9e-6   3: 9.8e-8 0 99.5 % 1.4e-6
      many_gaussians  1: 0      0 100 %  0        2: 9.4e-7 0 50.0 % 2.4e-6   3: 3.8e-8 0 97.7 % 4.8e-7"""
    device_options("ff_solver", solver)
    R.judge(name, *ask(name), solver=solver)


def test_uniform_solver_is_unsupported(device_options):
    import vr_amd as vr
    from vr_amd import _lib as L
    device_options("ff_solver", 4)
    with pytest.raises(vr.VRError) as e:
        ask("many_gaussians")
    assert e.value.status == L.VR_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    same(ask("250_random"), baseline("250_random"))
    same(ask("slab"), baseline("slab"))


def test_a_ray_does_not_depend_on_its_position_or_batch():
    """The 256 rays of 250_random tiled to 600 001 (more than one resident grid of lanes, not a multiple of 64):
    every copy equals the 256-ray call bit for bit."""
    o, d, tgt = R.rays("250_random")
    n = 600_001
    idx = np.arange(n) % 256
    t, alb, na = device().query_free_flight(R.device_scene("250_random"), o[idx], d[idx], tgt[idx], unit=True,
                                            return_albedo=True, return_active=True)
    bt, ba, bn = baseline("250_random")
    assert np.array_equal(bits(t), bits(bt)[idx]) and np.array_equal(bits(alb), bits(ba)[idx]) and np.array_equal(na, bn[idx])


def test_window_capacity_does_not_change_results(device_options):
    """VR_OPT_FF_WINDOW0 = 1 (a window per entry at first, doubling) and = 128 (the slab's rays still need up to three
    windows) are bit-identical, and equal the scene's default: the active list is carried across windows."""
    out = {}
    for window0 in (1, 128):
        device_options("ff_window0", window0)
        out[window0] = ask("slab")
    for x, y in zip(out[1], out[128]):
        print(f"window0 1 vs 128: {int(np.sum(x.view(np.uint32) != y.view(np.uint32)))} of {x.size} values differ")
    same(out[1], out[128])
    same(out[1], baseline("slab"))


def mutual(name, ta, tb):
    """Condition 2 between two device answers."""
    m = R.model(name)
    assert np.array_equal(ta < 0, tb < 0)
    sc = ta >= 0
    a, b = np.where(sc, ta, 0.0), np.where(sc, tb, 0.0)
    dT = np.where(sc, np.abs(np.exp(-m.tau(a)) - np.exp(-m.tau(b))), 0.0)
    print(f"{name}: max |dTr| between the two trees {dT.max():.3e}, bit-identical t {100 * np.mean(bits(ta) == bits(tb)):.1f} %")
    assert int((dT > R.PARITY).sum()) <= 1


@pytest.mark.parametrize("half_nodes,device_bvh", [(0, 0), (1, 1), (0, 1)])
def test_trees_change_the_summation_order_only(device_options, half_nodes, device_bvh):
    """VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH (default 1 / 0): Gaussians that enter at the same distance join the active
    list in walk order, so f32 sums over it may round differently; the answers stay within condition 2 of the
    default tree's and meet conditions 1-3 themselves. 1000_random: the device builder takes >= 256 Gaussians."""
    name = "1000_random"
    base = baseline(name)
    device_options("half_nodes", half_nodes)
    device_options("device_bvh", device_bvh)
    out = ask(name)
    R.judge(name, *out, label=f"{name} half_nodes {half_nodes} device_bvh {device_bvh}")
    mutual(name, out[0], base[0])


def test_optional_outputs_change_no_bit_of_t():
    name = "slab"
    o, d, tgt = R.rays(name)
    dev, sc = device(), R.device_scene(name)
    bt, ba, bn = baseline(name)
    t = dev.query_free_flight(sc, o, d, tgt, unit=True)
    assert isinstance(t, np.ndarray) and np.array_equal(bits(t), bits(bt))
    t, a = dev.query_free_flight(sc, o, d, tgt, unit=True, return_albedo=True)
    assert np.array_equal(bits(t), bits(bt)) and np.array_equal(bits(a), bits(ba))
    t, n = dev.query_free_flight(sc, o, d, tgt, unit=True, return_active=True)
    assert np.array_equal(bits(t), bits(bt)) and np.array_equal(n, bn)


def test_device_form_on_another_stream_equals_host_form():
    import torch
    name = "250_random"
    o, d, tgt = (torch.tensor(a).cuda() for a in R.rays(name))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = device().query_free_flight(R.device_scene(name), o, d, tgt, unit=True, return_albedo=True, return_active=True)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in out) and out[2].dtype == torch.int32
    s.synchronize()
    same([x.cpu().numpy() for x in out], baseline(name))


def test_unit_flag_and_scalar_target():
    """A scalar target broadcasts. unit = False normalises the direction once (ray.h:11-12): scaling a direction by a
    power of two scales its squared norm and the square root exactly, so the normalised direction, and with it the
    answer, is the same bit for bit."""
    name = "250_random"
    o, d, _ = R.rays(name)
    dev, sc = device(), R.device_scene(name)
    a = dev.query_free_flight(sc, o, d, 0.7, unit=True)
    b = dev.query_free_flight(sc, o, d, np.full(256, 0.7, F), unit=True)
    assert np.array_equal(bits(a), bits(b)) and np.sum(a >= 0) > 100
    c = dev.query_free_flight(sc, o, d, 0.7)
    e = dev.query_free_flight(sc, o, (d * F(4.0)).astype(F), 0.7)
    assert np.array_equal(bits(c), bits(e)) and np.sum(c >= 0) > 100


def test_special_targets_and_invalid_rays():
    name = "250_random"
    o, d, tgt = (a.copy() for a in R.rays(name))
    bt, ba, bn = baseline(name)
    tgt[0::8] = INF
    tgt[1::8] = NAN
    o[2::8, 1] = NAN
    o[3::8, 0] = INF
    d[4::8] = 0.0
    t, alb, na = device().query_free_flight(R.device_scene(name), o, d, tgt, unit=True, return_albedo=True, return_active=True)
    assert np.all(t[0::8] == -1.0) and np.all(alb[0::8] == 0.0) and np.all(na[0::8] == 0)
    for k in (1, 2, 3, 4):
        assert np.all(np.isnan(t[k::8])) and np.all(np.isnan(alb[k::8])) and np.all(na[k::8] == 0)
    for k in (5, 6, 7):  # the untouched rays of the batch
        assert np.array_equal(bits(t[k::8]), bits(bt[k::8])) and np.array_equal(bits(alb[k::8]), bits(ba[k::8]))
    # targets <= 0 go through the reference's comparisons: some distance in [0, the first event], never NaN
    t0 = device().query_free_flight(R.device_scene(name), *R.rays(name)[:2], np.float32(0.0), unit=True)
    total = R.model(name).tau(np.full(256, np.inf))
    assert not np.any(np.isnan(t0)) and np.all(t0[~R.model(name).hit.any(1)] == -1.0) and np.all(t0[total > 1e-3] >= 0)


def rows_of(o, d, unit=1.0):
    rows = np.zeros((len(o), 8), F)
    rows[:, 0:3], rows[:, 4:7], rows[:, 7] = o, d, unit
    return rows


def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    lib = L.lib()
    o, d, tgt = R.rays("many_gaussians")
    rows, n = rows_of(o, d), 256
    t = np.zeros(n, F)
    fresh = vr.Device(0)
    call = lambda r, g, k, out: lib.vr_query_free_flight(fresh._h, r, g, k, out, None, None)  # noqa: E731
    assert call(rows.ctypes.data, L.fptr(tgt), n, L.fptr(t)) == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call(rows.ctypes.data, L.fptr(tgt), n, L.fptr(t)) == L.VR_ERR_UNSUPPORTED
    fresh.upload(R.device_scene("many_gaussians"))
    assert call(None, L.fptr(tgt), n, L.fptr(t)) == L.VR_ERR_INVALID
    assert call(rows.ctypes.data, None, n, L.fptr(t)) == L.VR_ERR_INVALID
    assert call(rows.ctypes.data, L.fptr(tgt), n, None) == L.VR_ERR_INVALID
    assert call(None, None, 0, None) == L.VR_OK
    buf = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    tg = torch.tensor(tgt).cuda()
    assert lib.vr_query_free_flight_device(fresh._h, buf.data_ptr() + 4, tg.data_ptr(), n, out.data_ptr(), None, None,
                                           None) == L.VR_ERR_INVALID
    assert b"16-byte" in lib.vr_last_error()
    assert call(rows.ctypes.data, L.fptr(tgt), n, L.fptr(t)) == L.VR_OK
    assert np.array_equal(bits(t), bits(baseline("many_gaussians")[0]))


def test_empty_scene_never_collides():
    import vr_amd as vr
    o, d, tgt = R.rays("many_gaussians")
    t, alb, na = vr.Device(0).query_free_flight(vr.Scene(vr.Scene.GAUSSIANS), o, d, tgt, unit=True, return_albedo=True,
                                                return_active=True)
    assert np.all(t == -1.0) and np.all(alb == 0.0) and np.all(na == 0)


def test_overlap_beyond_every_capacity_is_reported_and_the_batch_still_written():
    """1100 coincident Gaussians (the coincident recipe): more than the second launch's 1024-entry rows hold at one
    point. The 4 x 4 rays through them get NaN / NaN / 0, the host form returns VR_ERR_OVERFLOW, and the other rays
    of the batch (aimed away from the cloud) still get their answers."""
    import vr_amd as vr
    from vr_amd import _lib as L
    dev = vr.Device(0)
    dev.upload(vr.Scene.from_gaussians(*R.coincident_gaussians(1100), lights=[vr.Light(*R.LIGHT)]))
    g = np.linspace(-0.1, 0.1, 4, dtype=F)
    aim = np.stack([np.repeat(g, 4), F(1.0) + np.tile(g, 4), np.zeros(16, F)], 1)
    o = np.tile(CAM_POS, (32, 1)).astype(F)
    d = np.concatenate([aim - CAM_POS, -(aim - CAM_POS)]).astype(F)
    rows = rows_of(o, d, unit=0.0)
    tgt = np.full(32, 0.5, F)
    t, alb = np.full(32, 7.0, F), np.full(32, 7.0, F)
    na = np.full(32, 7, np.uint32)
    st = L.lib().vr_query_free_flight(dev._h, rows.ctypes.data, L.fptr(tgt), 32, L.fptr(t), L.fptr(alb), na.ctypes.data_as(L.U32P))
    assert st == L.VR_ERR_OVERFLOW and b"1024" in L.lib().vr_last_error()
    assert np.all(np.isnan(t[:16])) and np.all(np.isnan(alb[:16])) and np.all(na[:16] == 0)
    assert np.all(t[16:] == -1.0) and np.all(alb[16:] == 0.0) and np.all(na[16:] == 0)


# ------------------------------------------------------------------------------------------------
# C++ mirror (MixtureQuery::query_free_flight through tools/vol_render --query)
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_python(tmp_path):
    name, n = "many_gaussians", 64
    o, d, _ = R.rays(name)
    o, d = o[96:96 + n], d[96:96 + n]
    path = tmp_path / "q.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", n, 0))
        f.write(np.concatenate([o, d, np.full((n, 1), INF, F)], 1).astype("<f4").tobytes())
    r = subprocess.run([os.path.join(ROOT, "tools", "vol_render"), "--scene", scene_path(name + ".txt"), "--query", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ff = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ff ")]
    assert len(ff) == n
    tgt = np.array([int(x[2], 16) for x in ff], np.uint32).view(F)
    # (Ray's constructor normalises the direction again: the driver's rays are the Python call's with unit = False)
    t, alb, na = device().query_free_flight(R.device_scene(name), o, d, tgt, return_albedo=True, return_active=True)
    assert [(int(x[3], 16), int(x[4], 16), int(x[5])) for x in ff] == list(zip(bits(t).tolist(), bits(alb).tolist(), na.tolist()))
    assert np.sum(t >= 0) > 0
