"""The feature query, the parts that need no GPU: the float64 model of tests/features_reference.py against central
differences of its own loss and against the sigma gradient's model, the Python surface (Device.evaluate_features,
Device.features_gradient, autograd.features), the ctypes signatures against libvr_hip.so, the header, argument checks
that must fail before the library is called, and the C++ mirror (include/vr/query.h, MixtureQuery::evaluate_features /
features_gradient) in the driver build.

Measured here: worst |model - central difference| / largest component of the column 6.7e-9 for the Gaussians' ten
columns, 8.0e-10 for the features' five and 1.2e-10 for the points' three (bound 1e-5)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import features_reference as FR
import sigma_grad_reference as R
from helpers import ROOT
from test_query_sigma_grad_host import fd_case

C_FD = 5


def fd_features(theta):
    """(6, 5) float64: channel 0 the albedo, channel 1 ones, the rest U(-1, 1) by default_rng(7), as on the GPU."""
    f = np.random.default_rng(7).uniform(-1, 1, (theta.shape[0], C_FD))
    f[:, 0] = theta[:, 10]
    f[:, 1] = 1.0
    return f


def test_model_matches_central_differences():
    """L = sum_i (sum_c w_ic F_ic + u_i mass_i) on fd_case()'s six Gaussians and 64 points, C = 5. Central differences with
    step h = 1e-6 max(1, |value|), the active set held (asserted not to move). Bound: 1e-5 of the largest component of the
    column; test_query_sigma_grad_host.py derives it (truncation 1.7e-7 |L'|, rounding < 1e-8 |L|), and the derivation
    carries over because the new terms are linear in f: L is the sigma loss with c = u + w . f in place of
    w_a (1 - alpha) + w_s alpha, and d L / d f is m itself."""
    theta, x, w2 = fd_case()
    rng = np.random.default_rng(12)
    w, u = rng.uniform(-1, 1, (64, C_FD)), rng.uniform(-1, 1, 64)
    f = fd_features(theta)
    rec = R.records_of(theta)
    active = R.quadratic(rec, x)[2] <= 9.0
    cg, cf, cx = FR.contributions(rec, x, f, w, u, active)
    G, Gf, Gx = cg.sum(0), cf.sum(0), cx.sum(1)

    def same_set(th, pts):
        return np.array_equal(R.quadratic(R.records_of(th), pts)[2] <= 9.0, active)

    def L(th, ft, pts):
        return FR.loss(R.records_of(th), pts, ft, w, u, active)

    fd = np.zeros_like(G)
    for g in range(theta.shape[0]):
        for k in range(10):
            h = 1e-6 * max(1.0, abs(theta[g, k]))
            tp, tm = theta.copy(), theta.copy()
            tp[g, k] += h
            tm[g, k] -= h
            assert same_set(tp, x) and same_set(tm, x)
            fd[g, k] = (L(tp, f, x) - L(tm, f, x)) / (2 * h)
    fdf = np.zeros_like(Gf)
    for g in range(theta.shape[0]):
        for k in range(C_FD):
            h = 1e-6 * max(1.0, abs(f[g, k]))
            fp, fm = f.copy(), f.copy()
            fp[g, k] += h
            fm[g, k] -= h
            fdf[g, k] = (L(theta, fp, x) - L(theta, fm, x)) / (2 * h)
    fdx = np.zeros_like(Gx)
    for i in range(len(x)):
        for k in range(3):
            h = 1e-6 * max(1.0, abs(x[i, k]))
            xp, xm = x.copy(), x.copy()
            xp[i, k] += h
            xm[i, k] -= h
            assert same_set(theta, xp) and same_set(theta, xm)
            fdx[i, k] = (L(theta, f, xp) - L(theta, f, xm)) / (2 * h)
    worst = 0.0
    for name, a, b in (("gaussians", G, fd), ("features", Gf, fdf), ("points", Gx, fdx)):
        scale = np.abs(a).max(0)
        assert np.all(scale > 0)
        rel = float((np.abs(a - b) / scale).max())
        print(f"{name}: worst |model - central difference| / largest component of the column = {rel:.3e}")
        worst = max(worst, rel)
    assert worst <= 1e-5


def test_one_channel_of_albedo_is_the_sigma_gradient():
    """C = 1, f = albedo, w = w_s - w_a, u = w_a: c = w_a (1 - alpha) + w_s alpha, so the Gaussians' ten columns are the sigma
    gradient's first ten and d L / d f is its albedo column, to 1e-12 relative; and the forward is (sigma_s, sigma_t)."""
    theta, x, w2 = fd_case()
    rec = R.records_of(theta)
    active = R.quadratic(rec, x)[2] <= 9.0
    f = theta[:, 10:11]
    w, u = (w2[:, 1] - w2[:, 0])[:, None], w2[:, 0]
    cg, cf, cx = FR.contributions(rec, x, f, w, u, active)
    sg, sx = R.contributions(rec, x, w2, active)
    assert np.abs(sg).max() > 0
    assert np.allclose(cg, sg[..., :10], rtol=1e-12, atol=0)
    assert np.allclose(cf[..., 0], sg[..., 10], rtol=1e-12, atol=0)
    assert np.allclose(cx, sx, rtol=1e-12, atol=0)
    G, Gs = cg.sum(0), sg.sum(0)
    assert np.allclose(G, Gs[:, :10], rtol=1e-12, atol=1e-12 * np.abs(sg).sum(0)[:, :10].max())
    assert np.allclose(cf.sum(0)[:, 0], Gs[:, 10], rtol=1e-12, atol=1e-12 * np.abs(sg[..., 10]).sum(0).max())
    F, _, tot, _ = FR.forward(rec, x, f, active)
    sig = R.sigma(rec, x, active)
    assert np.allclose(F[:, 0], sig[:, 1], rtol=1e-12, atol=0) and np.allclose(tot, sig.sum(1), rtol=1e-12, atol=0)


def test_sums_and_bound_terms_of_the_model_class():
    """FeatureModel.grads is `contributions` summed block by block, with S the sums of absolute values; channel 0 of
    features_of is the albedo and channel 1 ones."""
    theta, x, _ = fd_case()
    rec = R.records_of(theta)
    mdl = R.Model(rec, x.astype(np.float32))
    f = FR.features_of(rec, C_FD)
    assert f.dtype == np.float32 and np.array_equal(f[:, 0], theta[:, 10].astype(np.float32)) and np.all(f[:, 1] == 1.0)
    assert np.all(np.abs(f[:, 2:]) < 1) and not f.flags.writeable
    w, u = FR.signed_weights(mdl.n, C_FD)
    fm = FR.FeatureModel(mdl, f)
    cg, cf, cx = FR.contributions(rec, mdl.x, f, w, u)
    (G, S), (Gf, Sf), (Gx, Sx) = fm.grads(w, u)
    assert np.allclose(G, cg.sum(0), rtol=1e-12, atol=0) and np.allclose(S, np.abs(cg).sum(0), rtol=1e-12, atol=0)
    assert np.allclose(Gf, cf.sum(0), rtol=1e-12, atol=0) and np.allclose(Sf, np.abs(cf).sum(0), rtol=1e-12, atol=0)
    assert np.array_equal(Gx, cx.sum(1)) and np.array_equal(Sx, np.abs(cx).sum(1))
    F, S_F, tot, S_tot = FR.forward(rec, mdl.x, f)
    assert np.array_equal(fm.F, F) and np.array_equal(fm.mass, tot) and np.array_equal(fm.F[:, 1], tot)
    # weights=None is ones, weight_mass=None zeros
    (G1, _), (Gf1, _), (Gx1, _) = fm.grads()
    (G2, _), (Gf2, _), (Gx2, _) = fm.grads(np.ones((mdl.n, C_FD)), np.zeros(mdl.n))
    assert np.array_equal(G1, G2) and np.array_equal(Gf1, Gf2) and np.array_equal(Gx1, Gx2)


# ------------------------------------------------------------------------------------------------
# the surfaces
# ------------------------------------------------------------------------------------------------
def test_device_has_the_methods_with_the_documented_arguments():
    import vr_amd as vr
    sig = inspect.signature(vr.Device.evaluate_features)
    assert list(sig.parameters) == ["self", "scene", "points", "features", "return_mass", "return_active"]
    assert [sig.parameters[k].default for k in ("return_mass", "return_active")] == [False, False]
    sig = inspect.signature(vr.Device.features_gradient)
    assert list(sig.parameters) == ["self", "scene", "points", "features", "weights", "weight_mass", "gaussians", "features_grad",
                                    "positions"]
    assert [sig.parameters[k].default for k in ("weights", "weight_mass", "gaussians", "features_grad", "positions")] == \
        [None, None, True, True, False]
    from vr_amd import autograd
    for fn in (autograd.features, autograd.features_resident):
        assert list(inspect.signature(fn).parameters) == ["mean", "cov6", "density", "albedo", "feats", "points", "device"]
    assert "features(mean, cov6, density, albedo" in autograd.__doc__


def test_ctypes_signatures_resolve():
    from vr_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("vr_query_features", 8), ("vr_query_features_device", 9), ("vr_query_features_grad", 10),
                        ("vr_query_features_grad_device", 11)):
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert L.VR_FEATURES_MAX_CHANNELS == 64


def test_header_declares_the_queries_and_still_says_abi_11():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        src = f.read()
    assert "#define VR_ABI_VERSION 11\n" in src
    assert "#define VR_FEATURES_MAX_CHANNELS 64 " in src
    for decl in ("vr_status vr_query_features(vr_ctx* ctx, const float* xyz, size_t n, const float* features, uint32_t C, float* out,\n",
                 "vr_status vr_query_features_device(vr_ctx* ctx, const float* d_xyz, size_t n, const float* d_features, uint32_t C,\n",
                 "vr_status vr_query_features_grad(vr_ctx* ctx, const float* xyz, size_t n, const float* features, uint32_t C,\n",
                 "vr_status vr_query_features_grad_device(vr_ctx* ctx, const float* d_xyz, size_t n, const float* d_features, uint32_t C,\n"):
        assert decl in src, decl
    assert src.index("vr_status vr_query_sigma_grad_device(") < src.index("vr_status vr_query_features(") < \
        src.index("vr_status vr_query_features_grad(") < src.index("vr_status vr_query_events_count_device(")


def test_null_context_is_invalid():
    from vr_amd import _lib as L
    x, f, w = np.zeros(3, np.float32), np.zeros(2, np.float32), np.ones(2, np.float32)
    out, m, g = np.zeros(2, np.float32), np.zeros(1, np.float32), np.zeros(10, np.float32)
    na = np.zeros(1, np.uint32)
    lib = L.lib()
    assert lib.vr_query_features(None, L.fptr(x), 1, L.fptr(f), 2, L.fptr(out), L.fptr(m), na.ctypes.data_as(L.U32P)) == 1
    assert b"NULL ctx" in lib.vr_last_error()
    assert lib.vr_query_features_device(None, None, 1, None, 2, None, None, None, None) == 1
    assert lib.vr_query_features_grad(None, L.fptr(x), 1, L.fptr(f), 2, L.fptr(w), L.fptr(m), L.fptr(g), L.fptr(out), L.fptr(x)) == 1
    assert b"NULL ctx" in lib.vr_last_error()
    assert lib.vr_query_features_grad(None, None, 0, None, 1, None, None, None, None, None) == 1
    assert lib.vr_query_features_grad_device(None, None, 1, None, 2, None, None, None, None, None, None) == 1


def _no_device():
    """A Device object that owns no context: argument checks must raise before anything touches it."""
    import vr_amd as vr
    return object.__new__(vr.Device)


GOOD = np.zeros((4, 3), np.float32)
F3 = np.zeros((6, 3), np.float32)


@pytest.mark.parametrize("points,features", [
    (np.zeros((4, 2), np.float32), F3),             # wrong trailing shape
    (np.zeros(12, np.float32), F3),                 # flat
    (GOOD.astype(np.float64), F3),                  # dtype
    (GOOD.tolist(), F3),                            # not an array
    (GOOD, np.zeros(6, np.float32)),                # features: (N, C)
    (GOOD, np.zeros((6, 3, 1), np.float32)),
    (GOOD, F3.astype(np.float64)),                  # features dtype
    (GOOD, F3.tolist()),
    (GOOD, np.zeros((6, 0), np.float32)),           # C = 0
    (GOOD, np.zeros((6, 65), np.float32)),          # C = 65
])
def test_forward_argument_errors(points, features):
    with pytest.raises(ValueError):
        _no_device().evaluate_features(None, points, features)
    with pytest.raises(ValueError):
        _no_device().features_gradient(None, points, features)


@pytest.mark.parametrize("weights,weight_mass,asked", [
    (np.ones((3, 3), np.float32), None, (True, True, False)),       # C weights per point
    (np.ones((4, 2), np.float32), None, (True, True, False)),       # as many columns as channels
    (np.ones((4, 3), np.float64), None, (True, True, False)),       # weights dtype
    (np.ones(4, np.float32), None, (True, True, False)),            # weights shape
    (1.0, None, (True, True, False)),                               # weights: an array or None
    (None, np.ones(3, np.float32), (True, True, False)),            # one mass weight per point
    (None, np.ones((4, 1), np.float32), (True, True, True)),        # mass weights shape
    (None, np.ones(4, np.float64), (True, True, False)),            # mass weights dtype
    (None, 0.5, (True, True, False)),
    (None, None, (False, False, False)),                            # nothing asked for
])
def test_gradient_argument_errors(weights, weight_mass, asked):
    with pytest.raises(ValueError):
        _no_device().features_gradient(None, GOOD, F3, weights, weight_mass, *asked)


class _Torch:
    """An argument that is handed over as a torch tensor (built when the test runs)."""

    def __init__(self, a):
        self.a = a


def _bad_arguments():
    """(method, class of bad argument, positional arguments after the scene, keyword arguments, message): the table of
    tests/test_query_host.py for the two feature methods."""
    F64, TAIL = GOOD.astype(np.float64), np.zeros((4, 2), np.float32)
    ONES, TS = np.ones(4, np.float32), np.ones((4, 2), np.float32)
    feats = np.zeros((6, 2), np.float32)
    out = []
    for m in ("evaluate_features", "features_gradient"):
        out += [(m, "dtype", (F64, feats), {}, "points must be float32, not float64"),
                (m, "shape", (TAIL, feats), {}, "points must have shape (n, 3), not (4, 2)"),
                (m, "features-dtype", (GOOD, feats.astype(np.float64)), {}, "features must be float32, not float64"),
                (m, "features-shape", (GOOD, ONES), {}, "features must have shape (N, C), not (4,)"),
                (m, "features-mixed", (GOOD, _Torch(feats)), {}, "features must be of the same kind as points"),
                (m, "C=0", (GOOD, np.zeros((6, 0), np.float32)), {}, "features has 0 channels: 1 to 64 are allowed"),
                (m, "C=max+1", (GOOD, np.zeros((6, 65), np.float32)), {}, "features has 65 channels: 1 to 64 are allowed")]
    m = "features_gradient"
    out += [(m, "weights-dtype", (GOOD, feats), {"weights": TS.astype(np.float64)}, "weights must be float32, not float64"),
            (m, "weights-shape", (GOOD, feats), {"weights": ONES}, "weights must have shape (4, C), not (4,)"),
            (m, "weights-mixed", (GOOD, feats), {"weights": _Torch(TS)}, "weights must be of the same kind as points"),
            (m, "weights-rows", (GOOD, feats), {"weights": np.ones((5, 2), np.float32)}, "weights has 5 rows for 4 points"),
            (m, "weights-columns", (GOOD, feats), {"weights": np.ones((4, 3), np.float32)}, "weights has 3 columns for 2 channels"),
            (m, "weight_mass-dtype", (GOOD, feats), {"weight_mass": ONES.astype(np.float64)}, "weight_mass must be float32, not float64"),
            (m, "weight_mass-mixed", (GOOD, feats), {"weight_mass": _Torch(ONES)}, "weight_mass must be of the same kind as points"),
            (m, "weight_mass-rows", (GOOD, feats), {"weight_mass": np.ones(5, np.float32)}, "weight_mass has 5 entries for 4 points"),
            (m, "nothing-asked", (GOOD, feats), {"gaussians": False, "features_grad": False, "positions": False},
             "features_gradient: ask for gaussians, features_grad, positions or any of them together")]
    return out


@pytest.mark.parametrize("method,args,kwargs,message", [pytest.param(m, a, k, msg, id=f"{m}-{label}") for m, label, a, k, msg in _bad_arguments()])
def test_bad_argument_raises_its_message_before_the_library(method, args, kwargs, message):
    import torch
    as_given = lambda x: torch.from_numpy(x.a) if isinstance(x, _Torch) else x  # noqa: E731
    with pytest.raises(ValueError) as err:
        getattr(_no_device(), method)(None, *map(as_given, args), **{n: as_given(v) for n, v in kwargs.items()})
    assert str(err.value) == message


def test_numpy_and_torch_may_not_be_mixed():
    import torch
    with pytest.raises(ValueError):
        _no_device().evaluate_features(None, torch.zeros(4, 3), F3)
    with pytest.raises(ValueError):
        _no_device().evaluate_features(None, GOOD, torch.zeros(6, 3))
    with pytest.raises(ValueError):
        _no_device().features_gradient(None, GOOD, F3, torch.ones(4, 3))
    with pytest.raises(ValueError):
        _no_device().features_gradient(None, GOOD, F3, None, torch.ones(4))


def test_feature_rows_must_match_the_scene():
    import vr_amd as vr
    sc = vr.Scene.from_gaussians(np.zeros((2, 3), np.float32), np.tile(np.float32([1, 0, 0, 1, 0, 1]), (2, 1)),
                                 np.ones(2, np.float32), np.ones(2, np.float32))
    with pytest.raises(ValueError):
        _no_device().evaluate_features(sc, GOOD, F3)
    with pytest.raises(ValueError):
        _no_device().features_gradient(sc, GOOD, F3)


def test_cpp_mirror_compiles_in_the_driver_build():
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(tools, "vol_render.cpp")) as f:
        src = f.read()
    assert "evaluate_features(" in src and "features_gradient(" in src and "--query-features" in src
    with open(os.path.join(ROOT, "3dg-vol-renderer_amd", "include", "vr", "query.h")) as f:
        hdr = f.read()
    assert "std::vector<float> evaluate_features(" in hdr and "vr_query_features(" in hdr
    assert "std::vector<float> features_gradient(" in hdr and "vr_query_features_grad(" in hdr
