"""The radiance gradient query (Device.radiance_gradient over vr_query_radiance_grad[_device], autograd.radiance_fused[_resident],
MixtureQuery::radiance_gradient) on the device.

Against the float64 model of tests/radiance_grad_reference.py, with T the device's own tr (the profile's bits), per entry:
  grad_tau        |dev - model| <= (SR.BOUND + 2^-24) |q| T s_abs
  grad_q          |dev - model| <= (SR.BOUND + 2^-24) T s_abs  (+ T s_slack on a sample within Q_MARGIN of a cut-off, where the
                  model cannot say which side the f32 decision takes; such a sample has q = 0, so nothing else feels it)
  grad            |dev - (Gf + Gp)| <= (SR.BOUND + 2^-23) Sf + (GR.BOUND + 2^-23) Sp,  (Gp, Sp) = ProfileModel.grad(the device's grad_tau)
  grad_features   |dev - model| <= (SR.BOUND + 2^-23) Sr, exact zeros where Sr = 0
the bounds tests/test_gpu_query_radiance.py holds the composed backward to. Measured on an MI355X: MEASURED below.

Against the device's own composition, the numpy restatement of autograd._Radiance.backward over Device.features_gradient,
Device.evaluate_features and Device.query_transmittance_profile_grad: grad and grad_features at the same bound plus
2^-23 (Sf + Sp) for the composition's f32 w, u and wp (2^-23 Sr for the rows). The composition's grad_q and wp are printed
beside the fused ones and not asserted: its s comes from the feature query's f32 outputs and lies up to 2.7e-5 of T s_abs from
float64 where the fused one lies 5.5e-8 (DESIGN.md has the figures).

Where no dense model fits (the comb's 256 Gaussians, 65 537 rays, the elongated scene) the same float64 sums are taken pair
by pair (radiance_grad_reference.sparse_model and profile_sums with the oracle's chords, held to the dense models on the
CPU), the samples within the margin of a cut-off get q = 0 as in the model's cases (at most the cap, asserted), and the fused
outputs are held to the four bounds above. On the elongated scene the margin and the cap are aniso_cases' own (CUT_FACTOR x the
rung's f32 error of q, 5 %), and the composition is only printed: at a condition number of 10^4 its f32 s carries an error of
6.6e-4 T s_abs into its profile part. The chord ends' samples sit on cut-offs by construction, so no model can give their
grad and grad_features: those go against the composition, and grad_q and grad_tau against the float64 sums with the slack
T s_slack of the pairs either side of the decision may count (there a pair is in the margin if |q - 9| is within the bound on an
f32 evaluation of q for that pair, 2^-20 |p|.|M| |p|, or within Q_MARGIN).

Every test prints its measured maxima before it asserts.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import features_reference as FR
import grad_reference as GR
import radiance_grad_reference as RG
import radiance_reference as RR
import sigma_grad_reference as SR
from helpers import ROOT, scene_path
from test_gpu_query_radiance import bits, device, to_cuda, vr_scene

pytestmark = pytest.mark.gpu

MEASURED = "|dev - model| over its scale: 5.0e-8 .. 5.9e-8 for grad_q and grad_tau, at most 5.8e-8 for grad and grad_features (DESIGN.md 3e has the table)"
NAN, INF = np.float32(np.nan), np.float32(np.inf)
E23, E24, E40 = 2.0 ** -23, 2.0 ** -24, 2.0 ** -40
CASES = (("1_gaussian", 257, 1, 1, None), ("1_gaussian", 257, 17, 3, None), ("50_random", 1024, 9, 19, 257),
         ("50_random", 1024, 9, 20, 257), ("50_random", 1024, 9, 64, 257))


def run(dev, sc, o, d, t, f, q, gL, gA, tr=None, **kw):
    """(grad, grad_features, grad_q, grad_tau) of Device.radiance_gradient."""
    return dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, grad_q=True, grad_tau=True, **kw)


def host(got):
    return tuple(a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)


def forward_tr(dev, sc, o, d, t, unit=False):
    n = len(o)
    t2 = np.ascontiguousarray(np.broadcast_to(t, (n, t.shape[-1])))
    f1 = np.zeros((sc.get_num_primitives(), 1), np.float32)
    return dev.radiance(sc, o, d, t2, f1, None, unit=unit, return_tr=True)[1]


def composition(dev, sc, o, d, t, f, q, gL, gA, tr, unit=False, moving=True):
    """autograd._Radiance.backward in numpy: (grad (N, 10) float64, grad_features (N, C) f32, grad_q (n, K) float64, wp (n, K) f32)."""
    n, C = len(o), f.shape[1]
    tk = np.ascontiguousarray(np.broadcast_to(t, (n, t.shape[-1])))
    K = tk.shape[1]
    gL64 = np.ones((n, C)) if gL is None else gL.astype(np.float64)
    gA64 = np.zeros(n) if gA is None else gA.astype(np.float64)
    with np.errstate(all="ignore"):
        dn = np.ascontiguousarray(d, np.float32) if unit else GR.normalized_f32(d)
        valid = RR.valid_samples(tk) & np.isfinite(tr)
        qt = tr.astype(np.float64) if q is None else np.broadcast_to(q, (n, K)).astype(np.float64) * tr.astype(np.float64)
        qt = np.where(valid, qt, 0.0)
        x = np.where(valid[..., None], RR.points_f32(o, dn, tk), NAN).reshape(-1, 3)
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray((qt[:, :, None] * gL64[:, None, :]).reshape(-1, C).astype(np.float32))
    u = np.ascontiguousarray((qt * gA64[:, None]).reshape(-1).astype(np.float32))
    g, gf = dev.features_gradient(sc, x, f, w, u)
    F, mass = dev.evaluate_features(sc, x, f, return_mass=True)
    s = (F.reshape(n, K, C).astype(np.float64) * gL64[:, None, :]).sum(2) + mass.reshape(n, K).astype(np.float64) * gA64[:, None]
    wp = np.ascontiguousarray(np.where(valid, -qt * s, 0.0).astype(np.float32))
    gp = dev.query_transmittance_profile_grad(sc, o, d, tk, wp, moving_bounds=moving)
    with np.errstate(invalid="ignore"):
        gq = np.where(valid, tr.astype(np.float64) * s, 0.0)
    return g.astype(np.float64) + gp.astype(np.float64), gf, gq, wp


def ratio(err, S):
    with np.errstate(all="ignore"):
        r = np.where(S > 0, err / S, 0.0)
    return float(r.max()) if r.size else 0.0


def judge_model(label, got, mdl, moving=True, rows=None, grads=True, cap=RR.CAP, profile=None):
    """Prints the measured maxima, then asserts the four bounds of the module's head against the float64 model (dense or
    pair by pair). rows: the valid rays. grads=False: grad_q and grad_tau alone (samples on cut-offs with q != 0)."""
    g, gf, gq, gt = got
    assert g.dtype == gf.dtype == gq.dtype == gt.dtype == np.float32
    assert g.shape == (mdl.N, 10) and gf.shape == (mdl.N, mdl.C) and gq.shape == gt.shape == mdl.T.shape
    rows = np.ones(len(gq), bool) if rows is None else rows
    Ts, absq = (mdl.T * mdl.s_abs)[rows], np.abs(mdl.q)[rows]
    slack = (mdl.T * mdl.s_slack)[rows]
    e_t, e_q = np.abs(gt.astype(np.float64) - mdl.grad_tau)[rows], np.abs(gq.astype(np.float64) - mdl.grad_q)[rows]
    Gp, Sp = (profile or mdl.profile)(np.where(rows[:, None], gt, 0), moving)
    e_g, e_f = np.abs(g.astype(np.float64) - (mdl.Gf + Gp)), np.abs(gf.astype(np.float64) - mdl.Gr)
    near, valid = int(mdl.near.sum()), int(mdl.valid.sum())
    print(f"{label}: max |dev - model| / scale: grad_tau {ratio(np.where(slack > 0, 0, e_t), absq * Ts):.3e}, grad_q "
          f"{ratio(np.where(slack > 0, 0, e_q), Ts):.3e} (bound {SR.BOUND + E24:.3e}), grad {ratio(e_g, mdl.Sf + Sp):.3e}, grad_features "
          f"{ratio(e_f, mdl.Sr):.3e} (bound {SR.BOUND + E23:.3e}{'' if grads else ', not asserted: samples on cut-offs'}); samples near a "
          f"cut-off {near} of {valid}, pairs {mdl.pairs}, max |Gf| {np.abs(mdl.Gf).max():.3e}, max |Gp| {np.abs(Gp).max():.3e}")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gf)) and np.all(np.isfinite(gq[rows])) and np.all(np.isfinite(gt[rows]))
    assert (mdl.Sf > 0).any() and (Sp > 0).any() and (Ts > 0).any()
    # (a pair in the margin that the device counts is rounded with the rest: the relative bound covers the slack too)
    assert np.all(e_t <= (SR.BOUND + E24) * absq * (Ts + slack) + absq * slack)
    assert np.all(e_q <= (SR.BOUND + E24) * (Ts + slack) + slack)
    if grads:  # (every sample near a cut-off has q = 0, and there are at most the cap of them: only grad_q takes the slack)
        assert near <= cap * valid and not np.any(mdl.q[mdl.near])
        assert np.all(e_g <= (SR.BOUND + E23) * mdl.Sf + (GR.BOUND + E23) * Sp)
        assert np.all(e_f <= (SR.BOUND + E23) * mdl.Sr) and not np.any(bits(gf)[mdl.Sr == 0])
    return Sp


def judge_composition(label, got, comp, S, q, tr, rows=None, asserted=True):
    """Prints the measured maxima, then asserts grad and grad_features against the composition's. S = (Sf, Sr, Sp, s_abs)."""
    g, gf, gq, gt = got
    cg, cf, cq, cwp = comp
    Sf, Sr, Sp, s_abs = S
    rows = np.ones(len(gq), bool) if rows is None else rows
    with np.errstate(invalid="ignore"):
        Ts = np.where(np.isfinite(tr), tr.astype(np.float64), 0.0) * s_abs
    absq = np.ones_like(Ts) if q is None else np.abs(np.nan_to_num(np.broadcast_to(q, Ts.shape).astype(np.float64), posinf=0.0, neginf=0.0))
    e_g, e_f = np.abs(g.astype(np.float64) - cg), np.abs(gf.astype(np.float64) - cf.astype(np.float64))
    e_q, e_t = np.abs(gq.astype(np.float64) - cq)[rows], np.abs(gt.astype(np.float64) - cwp.astype(np.float64))[rows]
    print(f"{label}: max |fused - composed| / scale: grad {ratio(e_g, Sf + Sp):.3e} (bound {SR.BOUND + 2 * E23:.3e}{'' if asserted else ', not asserted'}), "
          f"grad_features {ratio(e_f, Sr):.3e}; not asserted: grad_q {ratio(e_q, Ts[rows]):.3e}, grad_tau {ratio(e_t, (absq * Ts)[rows]):.3e}; "
          f"max |grad| {np.abs(cg).max():.3e}, Gaussians with Sf > 0: {int((Sf > 0).any(1).sum())}, with Sp > 0: {int((Sp > 0).any(1).sum())}")
    assert np.all(np.isfinite(cg)) and np.all(np.isfinite(cf))
    if asserted:
        assert np.all(e_g <= (SR.BOUND + E23) * Sf + (GR.BOUND + E23) * Sp + E23 * (Sf + Sp))
        assert np.all(e_f <= (SR.BOUND + 2 * E23) * Sr)


def against_both(label, dev, sc, osc, o, d, t, f, q, gL, gA, rows=None, margin=SR.Q_MARGIN, cap=RR.CAP, zero_near=True, composed=True):
    """The fused outputs against the float64 sums taken pair by pair and against the composition. zero_near: q = 0 on the
    samples within `margin` of a cut-off, then all four outputs are held to the model; otherwise grad_q and grad_tau alone."""
    if zero_near:
        q = np.where(RG.near_samples(osc, o, d, t, margin=margin), np.float32(0), q).astype(np.float32)
    tr = forward_tr(dev, sc, o, d, t)
    got = run(dev, sc, o, d, t, f, q, gL, gA, tr)
    comp = composition(dev, sc, o, d, t, f, q, gL, gA, tr)
    m = RG.sparse_model(osc, o, d, t, q, f, tr, gL, gA, margin=margin)
    Sp = judge_model(label, got, m, rows=rows, grads=zero_near, cap=cap, profile=lambda w, moving: RG.profile_sums(osc, o, d, t, w, moving))
    judge_composition(label, got, comp, (m.Sf, m.Sr, Sp, m.s_abs), q, tr, rows, asserted=composed)
    return got, (m.Sf, m.Sr, Sp, m.s_abs), q


# ------------------------------------------------------------------------------------------------
# 1. the float64 model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,K,C,rows", CASES, ids=[f"{c[0]}-K{c[2]}-C{c[3]}" for c in CASES])
def test_against_the_model(name, n, K, C, rows):
    o, d, t, q, f, gL, gA = RG.case_inputs(name, n, K, C, rows)
    dev, sc = device(), vr_scene(name)
    tr = forward_tr(dev, sc, o, d, t)
    got = run(dev, sc, o, d, t, f, q, gL, gA, tr)
    mdl = RG.RadianceGradModel(GR.oracle_scene(name), o, d, t, q, f, tr, gL, gA)
    judge_model(f"{name} K={K} C={C}", got, mdl)


# ------------------------------------------------------------------------------------------------
# 2. the device's own composition, and autograd
# ------------------------------------------------------------------------------------------------
def test_against_the_composition():
    name, n, K, C, rows = CASES[2]
    o, d, t, q, f, gL, gA = RG.case_inputs(name, n, K, C, rows)
    dev, sc = device(), vr_scene(name)
    tr = forward_tr(dev, sc, o, d, t)
    got = run(dev, sc, o, d, t, f, q, gL, gA, tr)
    comp = composition(dev, sc, o, d, t, f, q, gL, gA, tr)
    mdl = RG.RadianceGradModel(GR.oracle_scene(name), o, d, t, q, f, tr, gL, gA)
    judge_composition(f"{name} K={K} C={C}", got, comp, (mdl.Sf, mdl.Sr, mdl.profile(got[3])[1], mdl.s_abs), q, tr)


def fused_backward(fn, gs, f, o, d, t, q, gL, gA, needs=(0, 1, 2, 4), q_grad=True, param_device="cuda"):
    import torch
    to = lambda a, dev_="cuda": torch.from_numpy(np.array(a)).to(dev_)  # noqa: E731
    p = [to(a, param_device) for a in (gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10], f)]
    for k in needs:
        p[k].requires_grad_()
    ro, rt, rq = to(o).requires_grad_(), to(t).requires_grad_(), to(q).requires_grad_(q_grad)
    L, op = fn(*p, ro, to(d), rt, rq)
    assert tuple(L.shape) == (len(o), f.shape[1]) and tuple(op.shape) == (len(o),) and L.dtype == torch.float32
    ((L * to(gL)).sum() + (op * to(gA)).sum()).backward()
    assert p[3].grad is None and ro.grad is None and rt.grad is None
    return L.detach().cpu().numpy(), op.detach().cpu().numpy(), p, rq.grad


def test_autograd_fused_against_autograd_radiance(monkeypatch):
    import torch
    import vr_amd as vr
    from test_gpu_query_radiance import autograd_case, radiance_backward
    from vr_amd import autograd
    name, o, d, t, q, f, rmdl, gL, gA = autograd_case()
    gs = vr_scene(name).gaussians()
    calls = []
    for meth in ("features_gradient", "evaluate_features", "query_transmittance_profile_grad", "radiance", "radiance_gradient"):
        def counting(self, *a, _real=getattr(vr.Device, meth), _name=meth, **kw):
            calls.append((_name, bool(kw.get("gaussians")), bool(kw.get("features_grad")), bool(kw.get("grad_q")), bool(kw.get("grad_tau")))
                         if _name == "radiance_gradient" else _name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(vr.Device, meth, counting)
    L, op, p, gq = fused_backward(autograd.radiance_fused, gs, f, o, d, t, q, gL, gA)
    assert calls == ["radiance", ("radiance_gradient", True, True, True, False)], calls
    del calls[:]
    L0, op0, p0 = radiance_backward(autograd.radiance, gs, f, o, d, t, q, gL, gA)
    del calls[:]
    assert np.array_equal(bits(L), bits(L0)) and np.array_equal(bits(op), bits(op0))  # the same forward bits
    dev = device()
    sc = vr.Scene.from_gaussians(gs[:, 0:3], gs[:, 3:9], gs[:, 9], gs[:, 10])
    tr = dev.radiance(sc, o, d, t, f, q, unit=True, return_tr=True)[1]
    del calls[:]
    mdl = RG.RadianceGradModel(GR.oracle_scene(name), o, d, t, q, f, tr, gL, gA, unit=True)
    assert np.array_equal(mdl.near, rmdl.near)
    got = torch.cat([p[0].grad, p[1].grad, p[2].grad[:, None]], 1).cpu().numpy()
    ref = torch.cat([p0[0].grad, p0[1].grad, p0[2].grad[:, None]], 1).cpu().numpy()
    gt = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, unit=True, gaussians=False, features_grad=False, grad_tau=True)
    del calls[:]
    Gp, Sp = mdl.profile(gt)
    judge_model("autograd.radiance_fused", (got, p[4].grad.cpu().numpy(), gq.cpu().numpy(), gt), mdl)
    e = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ef = np.abs(p[4].grad.cpu().numpy().astype(np.float64) - p0[4].grad.cpu().numpy())
    print(f"radiance_fused against radiance: max |fused - composed| / (Sf + Sp) = {ratio(e, mdl.Sf + Sp):.3e}, feats {ratio(ef, mdl.Sr):.3e}")
    # (both are f32 here: one more rounding of the composed sum, 2^-24 of it, which the absolute sums bound)
    assert np.all(e <= (SR.BOUND + E23) * mdl.Sf + (GR.BOUND + E23) * Sp + E23 * (mdl.Sf + Sp) + E24 * (mdl.Sf + Sp))
    assert np.all(ef <= (SR.BOUND + 2 * E23) * mdl.Sr)
    assert gq.dtype == torch.float32 and tuple(gq.shape) == t.shape
    # only what some input needs; none at all for albedo alone
    for needs, q_grad, want in (((4,), False, (False, True, False, False)), ((2,), False, (True, False, False, False)),
                                ((), True, (False, False, True, False))):
        del calls[:]
        _, _, p2, gq2 = fused_backward(autograd.radiance_fused_resident, gs, f, o, d, t, q, gL, gA, needs=needs, q_grad=q_grad)
        assert calls == ["radiance", ("radiance_gradient",) + want], calls
        if q_grad:  # (the resident upload's norm words may differ by 2 ulp: twice the bound)
            e2 = np.abs(gq2.cpu().numpy().astype(np.float64) - mdl.grad_q)
            assert np.all(e2 <= 2 * ((SR.BOUND + E24) * mdl.T * mdl.s_abs + mdl.T * mdl.s_slack))
    del calls[:]
    fused_backward(autograd.radiance_fused_resident, gs, f, o, d, t, q, gL, gA, needs=(3,), q_grad=False)
    assert calls == ["radiance"], calls
    with pytest.raises(ValueError):
        fused_backward(autograd.radiance_fused_resident, gs, f, o, d, t, q, gL, gA, param_device="cpu")


# ------------------------------------------------------------------------------------------------
# 3. exact properties
# ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def close_sums(a, b, S):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= E40 * S)


def test_exact_properties():
    name, n, K, C, rows = CASES[2]
    o, d, t, q, f, gL, gA = RG.case_inputs(name, n, K, C, rows)
    dev, sc = device(), vr_scene(name)
    tr = forward_tr(dev, sc, o, d, t)
    got = run(dev, sc, o, d, t, f, q, gL, gA, tr)
    mdl = RG.RadianceGradModel(GR.oracle_scene(name), o, d, t, q, f, tr, gL, gA)
    SG, Sr = mdl.Sf + mdl.profile(got[3])[1], mdl.Sr
    # tr given against tr recomputed: identical bits in all four outputs
    again = run(dev, sc, o, d, t, f, q, gL, gA, None)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    # asked for alone and together
    gq1 = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, gaussians=False, features_grad=False, grad_q=True)
    gt1 = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, gaussians=False, features_grad=False, grad_tau=True)
    both = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, gaussians=False, features_grad=False, grad_q=True, grad_tau=True)
    assert same_bits(gq1, got[2]) and same_bits(gt1, got[3]) and same_bits(both[0], got[2]) and same_bits(both[1], got[3])
    g1 = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, features_grad=False)
    f1 = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr, gaussians=False)
    gf2 = dev.radiance_gradient(sc, o, d, t, f, gL, gA, q, tr)
    assert g1.shape == (50, 10) and f1.shape == (50, C) and len(gf2) == 2
    assert close_sums(g1, got[0], SG) and close_sums(f1, got[1], Sr) and close_sums(gf2[0], got[0], SG) and close_sums(gf2[1], got[1], Sr)
    # a shared row against the same row per ray, for t and for q
    row_t, row_q = np.ascontiguousarray(t[3]), np.ascontiguousarray(q[5])
    tile = lambda r: np.ascontiguousarray(np.tile(r, (len(o), 1)))  # noqa: E731
    a = run(dev, sc, o, d, row_t, f, row_q, gL, gA)
    b = run(dev, sc, o, d, tile(row_t), f, tile(row_q), gL, gA)
    c = run(dev, sc, o, d, row_t, f, tile(row_q), gL, gA)
    trs = forward_tr(dev, sc, o, d, tile(row_t))
    Ss = RG.scales(GR.oracle_scene(name), o, d, tile(row_t), tile(row_q), f, trs, gL, gA, a[3], reach=9.0)
    assert np.abs(a[0]).max() > 0 and np.abs(a[2]).max() > 0
    for x in (b, c):
        assert same_bits(a[2], x[2]) and same_bits(a[3], x[3])
        assert close_sums(a[0], x[0], Ss[0] + Ss[2]) and close_sums(a[1], x[1], Ss[1])
    # q = None is ones
    a = run(dev, sc, o, d, t, f, None, gL, gA, tr)
    b = run(dev, sc, o, d, t, f, np.ones_like(t), gL, gA, tr)
    S1 = RG.scales(GR.oracle_scene(name), o, d, t, None, f, tr, gL, gA, a[3], reach=9.0)
    assert same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and close_sums(a[0], b[0], S1[0] + S1[2]) and close_sums(a[1], b[1], S1[1])
    # weights = None is ones, weight_opacity = None zeros
    a = run(dev, sc, o, d, t, f, q, None, None, tr)
    b = run(dev, sc, o, d, t, f, q, np.ones_like(gL), np.zeros_like(gA), tr)
    S2 = RG.scales(GR.oracle_scene(name), o, d, t, q, f, tr, None, None, a[3], reach=9.0)
    assert same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and close_sums(a[0], b[0], S2[0] + S2[2]) and close_sums(a[1], b[1], S2[1])
    # numpy and torch kinds
    g = run(dev, sc, to_cuda(o), to_cuda(d), to_cuda(t), to_cuda(f), to_cuda(q), to_cuda(gL), to_cuda(gA), to_cuda(tr))
    assert all(v.is_cuda for v in g) and tuple(g[0].shape) == (50, 10) and tuple(g[1].shape) == (50, C) and tuple(g[2].shape) == t.shape
    g = host(g)
    assert same_bits(g[2], got[2]) and same_bits(g[3], got[3]) and close_sums(g[0], got[0], SG) and close_sums(g[1], got[1], Sr)
    only = dev.radiance_gradient(sc, to_cuda(o), to_cuda(d), to_cuda(t), to_cuda(f), to_cuda(gL), to_cuda(gA), to_cuda(q), None,
                                 gaussians=False, features_grad=False, grad_tau=True)
    assert same_bits(only.cpu().numpy(), got[3])
    # grad_tau = f32(-q (T s)) agrees with grad_q = f32(T s) to one rounding each
    ok = np.isfinite(q) & (q != 0)
    lhs = np.abs(got[3].astype(np.float64) + q.astype(np.float64) * got[2].astype(np.float64))
    assert ok.sum() > 1000 and np.all(lhs[ok] <= (E23 + 2.0 ** -45) * np.abs(q.astype(np.float64) * got[2].astype(np.float64))[ok] + 1e-44)
    assert not np.any(bits(got[3])[~ok] & 0x7fffffff)
    # frozen bounds against the model's frozen gradient
    frozen = run(dev, sc, o, d, t, f, q, gL, gA, tr, moving_bounds=False)
    assert same_bits(frozen[2], got[2]) and same_bits(frozen[3], got[3]) and close_sums(frozen[1], got[1], Sr)
    assert np.abs(frozen[0] - got[0]).max() > 0
    judge_model("50_random frozen bounds", frozen, mdl, moving=False)


# ------------------------------------------------------------------------------------------------
# 4. chord ends, 5. elongated Gaussians
# ------------------------------------------------------------------------------------------------
def test_chord_ends():
    from test_gpu_query_radiance import chord_case
    name, o, d, t, q = chord_case()
    f = RR.features_of(50, 19)
    gL, gA = FR.signed_weights(len(o), 19)
    valid = RR.valid_samples(t)
    assert valid.sum() >= 2000 and (t[:8, 0] == 0).all()
    got, S, _ = against_both("chord ends", device(), vr_scene(name), GR.oracle_scene(name), o, d, t, f, q, gL, gA, zero_near=False, margin=None)
    assert not np.any(bits(got[2])[~valid]) and not np.any(bits(got[3])[~valid]) and np.abs(got[2][:8, 0]).min() > 0


def test_elongated_gaussians():
    import aniso_cases as AC
    key = ("disc", 100)
    assert key[1] == max(r for _, r in AC.LADDER)
    o, d, _ = AC.aimed_rays(*key, n=256)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    dist = np.linalg.norm(d.astype(np.float64), axis=1)
    rng = np.random.default_rng(31)
    K = 33
    t = (rng.uniform(0, 2, (256, K)) * dist[:, None]).astype(np.float32)
    t[:, 0] = dist.astype(np.float32)  # the aimed target itself
    q = rng.uniform(-1, 1, t.shape).astype(np.float32)
    N = len(AC.gaussians(*key).mean)
    f = RR.features_of(N, 19)
    gL, gA = FR.signed_weights(256, 19)
    got, S, _ = against_both("disc 100", device(), AC.device_scene(*key), AC.oracle_scene(*key), o, d, t, f, q, gL, gA,
                             margin=AC.CUT_FACTOR * AC.q_error(*key), cap=AC.CAP, composed=False)
    assert (S[0] > 0).any(1).sum() >= N // 2


# ------------------------------------------------------------------------------------------------
# 6. the redo path: the comb of wide_walk_reference.py, where 4-wide ray walks break off
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["wide", "host"])
@pytest.mark.parametrize("name", ["f257", "shuffled"])
def test_the_stack_limit(name, config, device_options):
    """Under "wide" every F, I and C ray's walk reaches the stack limit after it has added Gaussians: the atomics of the
    broken-off walk are taken back, the ray's row of s zeroed again, and the whole ray walked on the child-pair tree."""
    from test_gpu_query_profile import comb_samples
    from test_gpu_wide_stack import batch, on_device, oracle
    dev, sc = on_device(device_options, config)
    o, d, _, names = batch(name)
    K, C = 9, 11
    t = np.ascontiguousarray(comb_samples(name, 17)[:, :K])
    q = np.random.default_rng(37).uniform(-1, 1, t.shape).astype(np.float32)
    f = RR.features_of(oracle().num, C)
    gL, gA = FR.signed_weights(len(o), C)
    ok = names != "X"
    got, S, q = against_both(f"comb {name} {config}", dev, sc, oracle(), o, d, t, f, q, gL, gA, rows=ok)
    assert np.abs(got[2][names == "F"]).max() > 0 and (S[0] > 0).any() and (S[2] > 0).any()
    bad = ~ok
    assert np.all(np.isnan(got[2][bad])) and np.all(np.isnan(got[3][bad]))
    if bad.any():  # the X rays add nothing: the same query without them
        rest = run(dev, sc, np.ascontiguousarray(o[ok]), np.ascontiguousarray(d[ok]), np.ascontiguousarray(t[ok]), f,
                   np.ascontiguousarray(q[ok]), np.ascontiguousarray(gL[ok]), np.ascontiguousarray(gA[ok]))
        assert same_bits(rest[2], got[2][ok]) and same_bits(rest[3], got[3][ok])
        assert close_sums(rest[0], got[0], S[0] + S[2]) and close_sums(rest[1], got[1], S[1])


# ------------------------------------------------------------------------------------------------
# 7. inputs that contribute nothing
# ------------------------------------------------------------------------------------------------
def test_inputs_that_contribute_nothing():
    import vr_amd as vr
    name, n, K, C = "50_random", 1024, 33, 19
    o, d, t, q, f, gL, gA = (np.array(a) for a in RG.case_inputs(name, n, K, C, rows=64))
    dev, sc, osc = device(), vr_scene(name), GR.oracle_scene(name)
    base = run(dev, sc, o, d, t, f, q, gL, gA)
    tr = forward_tr(dev, sc, o, d, t)
    Sf, Sr, Sp, _ = RG.scales(osc, o, d, t, q, f, tr, gL, gA, base[3], reach=9.0)
    SG = Sf + Sp
    # special samples in three columns get +0; what is left is the query without those columns
    cols = [c for c in range(K) if c not in (4, 9, 20)]
    t2, q2 = t.copy(), q.copy()
    t2[:, 4], t2[:, 9], t2[:, 20] = -1.0, NAN, INF
    t2[1, 4] = -INF
    q2[:, 9] = INF
    got = run(dev, sc, o, d, t2, f, q2, gL, gA)
    rest = run(dev, sc, o, d, np.ascontiguousarray(t[:, cols]), f, np.ascontiguousarray(q[:, cols]), gL, gA)
    assert not np.any(bits(got[2][:, (4, 9, 20)])) and not np.any(bits(got[3][:, (4, 9, 20)]))
    assert same_bits(got[2][:, cols], rest[2]) and same_bits(got[3][:, cols], rest[3])
    assert close_sums(got[0], rest[0], SG) and close_sums(got[1], rest[1], Sr) and np.abs(rest[0]).max() > 0
    # q = inf on samples in no ellipsoid leaves everything finite, and as it was
    x = RR.points_f32(o, GR.normalized_f32(d), t).reshape(-1, 3)
    act = dev.evaluate_features(sc, np.ascontiguousarray(x), f, return_active=True)[1].reshape(t.shape)
    assert (act == 0).sum() > 100
    q3 = np.where(act == 0, INF, q).astype(np.float32)
    got = run(dev, sc, o, d, t, f, q3, gL, gA)
    assert all(np.all(np.isfinite(a)) for a in got) and same_bits(got[2], base[2]) and same_bits(got[3], base[3])
    assert close_sums(got[0], base[0], SG) and close_sums(got[1], base[1], Sr)
    # a row with nothing but special samples: +0 and nothing added
    t4 = t.copy()
    t4[7] = np.resize(np.float32([-1.0, NAN, INF, -INF]), K)
    got = run(dev, sc, o, d, t4, f, q, gL, gA)
    keep = np.arange(64) != 7
    rest = run(dev, sc, o[keep], d[keep], t[keep], f, q[keep], gL[keep], gA[keep])
    assert not np.any(bits(got[2][7])) and not np.any(bits(got[3][7]))
    assert same_bits(got[2][keep], rest[2]) and close_sums(got[0], rest[0], SG) and close_sums(got[1], rest[1], Sr)
    # invalid rays: NaN rows and nothing added
    o5, d5 = o.copy(), d.copy()
    o5[11, 1], d5[30] = NAN, 0.0
    got = run(dev, sc, o5, d5, t, f, q, gL, gA)
    keep = ~np.isin(np.arange(64), (11, 30))
    rest = run(dev, sc, o[keep], d[keep], t[keep], f, q[keep], gL[keep], gA[keep])
    for r in (11, 30):
        assert np.all(np.isnan(got[2][r])) and np.all(np.isnan(got[3][r]))
    assert same_bits(got[2][keep], rest[2]) and same_bits(got[3][keep], rest[3])
    assert np.all(np.isfinite(got[0])) and close_sums(got[0], rest[0], SG) and close_sums(got[1], rest[1], Sr)
    # n = 0 zeroes grad and grad_features
    for kind in (lambda v: v, to_cuda):
        none = host(run(dev, sc, kind(o[:0]), kind(d[:0]), kind(t[:0]), kind(f), kind(q[:0]), kind(gL[:0]), kind(gA[:0])))
        assert [a.shape for a in none] == [(50, 10), (50, C), (0, K), (0, K)] and not np.any(bits(none[0])) and not np.any(bits(none[1]))
    # the empty scene gives zeros, in both kinds
    hollow = vr.Scene.from_gaussians(np.zeros((0, 3)), np.zeros((0, 6)), [], [], [vr.Light([0, 1, 0], [1, 1, 1])])
    fresh = vr.Device(0)
    for kind in (lambda v: v, to_cuda):
        got = host(run(fresh, hollow, kind(o5), kind(d5), kind(t), kind(np.zeros((0, C), np.float32)), kind(q), kind(gL), kind(gA)))
        assert [a.shape for a in got] == [(0, 10), (0, C), (64, K), (64, K)]
        assert not np.any(bits(got[2][keep])) and not np.any(bits(got[3][keep])) and np.all(np.isnan(got[2][~keep]))
        only = fresh.radiance_gradient(hollow, kind(o), kind(d), kind(t), kind(np.zeros((0, C), np.float32)))
        assert [tuple(a.shape) for a in only] == [(0, 10), (0, C)]


# ------------------------------------------------------------------------------------------------
# 8. 65 537 rays: 256 blocks and one lane
# ------------------------------------------------------------------------------------------------
def test_65537_rays():
    name, n, K, C = "50_random", 65537, 4, 3
    o, d = RR.case_rays(name, n)
    t, q = RR.case_samples(name, n, K)
    f = RR.features_of(50, C)
    gL, gA = FR.signed_weights(n, C)
    got, S, _ = against_both("50_random x 65537", device(), vr_scene(name), GR.oracle_scene(name), o, d, t, f, q, gL, gA)
    assert np.abs(got[2][-1]).max() > 0 or np.abs(got[2][-64:]).max() > 0


# ------------------------------------------------------------------------------------------------
# 9. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    fresh = vr.Device(0)
    lib = L.lib()
    name, K, C = "250_random", 3, 3
    o, d = (np.ascontiguousarray(a[:257]) for a in RR.case_rays(name, 1024))
    t, q = (np.ascontiguousarray(a[:257]) for a in RR.case_samples(name, 1024, K))
    f = RR.features_of(250, C)
    gL, gA = FR.signed_weights(257, C)
    rows = fresh._pack_rays_numpy(o, d, np.inf)
    outs = [np.full((250, 10), 7.0, np.float32), np.full((250, C), 7.0, np.float32), np.full((257, K), 7.0, np.float32),
            np.full((257, K), 7.0, np.float32)]
    big = np.ones(L.VR_PROFILE_MAX_SAMPLES + 1, np.float32)
    P = L.fptr
    R_ = rows.ctypes.data
    ALL = tuple(P(a) for a in outs)

    def call(r=R_, ts=P(t), ts_stride=K, qs=P(q), qs_stride=K, n=257, k=K, ft=P(f), c=C, flags=0, o_=ALL):
        return lib.vr_query_radiance_grad(fresh._h, r, ts, ts_stride, qs, qs_stride, n, k, ft, c, P(gL), P(gA), None, flags, *o_)

    untouched = lambda: all(np.all(a == 7.0) for a in outs)  # noqa: E731
    assert call() == 5  # VR_ERR_NOSCENE
    fresh.upload(vr.Scene.load_SMM(scene_path("sph_2_spheres.txt")))
    assert call() == 7  # VR_ERR_UNSUPPORTED
    fresh.upload(vr_scene(name))
    bad = [dict(k=0, ts_stride=0, qs_stride=0), dict(ts=P(big), ts_stride=0, qs=None, qs_stride=0, k=len(big)),  # K
           dict(c=0), dict(c=65),                                                                                  # C
           dict(ts_stride=1), dict(ts_stride=K + 1), dict(qs_stride=1), dict(qs_stride=2 * K),                     # strides
           dict(r=None), dict(ts=None), dict(ft=None),                                                             # NULL
           dict(o_=(None, None, None, None)),                                                                      # nothing asked for
           dict(flags=2), dict(flags=0x80000001),                                                                  # unknown flag bits
           dict(n=1 << 31), dict(n=1 << 30, k=2, ts_stride=2, qs_stride=2), dict(n=1 << 30, k=1, ts_stride=1, qs_stride=1, c=2)]
    for i, kw in enumerate(bad):
        assert call(**kw) == 1, (i, kw)  # VR_ERR_INVALID
        assert untouched(), (i, kw)
    assert call(qs=None, qs_stride=99) == 0  # (no q: its stride is not read)
    ones = run(device(), vr_scene(name), o, d, t, f, None, gL, gA)
    assert same_bits(outs[2], ones[2]) and same_bits(outs[3], ones[3])
    assert call(flags=L.VR_GRAD_FROZEN_BOUNDS) == 0 and call() == 0
    ref = run(device(), vr_scene(name), o, d, t, f, q, gL, gA)
    assert same_bits(outs[2], ref[2]) and same_bits(outs[3], ref[3])
    assert np.all(np.abs(outs[0].astype(np.float64) - ref[0]) <= E23 * np.abs(ref[0])) and np.abs(ref[0]).max() > 0
    assert np.all(np.abs(outs[1].astype(np.float64) - ref[1]) <= E23 * np.abs(ref[1]))
    assert call(n=0) == 0 and not np.any(bits(outs[0])) and not np.any(bits(outs[1])) and same_bits(outs[2], ref[2])  # n == 0 zeroes the two
    assert call(r=None, ts=None, qs=None, ft=None, n=0, o_=(None, None, None, None)) == 0
    # the _device form with torch pointers
    buf = torch.zeros(257 * 8 + 4, dtype=torch.float32, device="cuda")
    dt, dq, df = to_cuda(t), to_cuda(q), to_cuda(f)
    o_t = torch.full((257, K), 7.0, device="cuda")
    g_t = torch.full((250, 10), 7.0, device="cuda")
    dcall = lambda r, ts, stride, ft, c, flags, dst, gdst: lib.vr_query_radiance_grad_device(  # noqa: E731
        fresh._h, r, ts, stride, dq.data_ptr(), K, 257, K, ft, c, None, None, None, flags, gdst, None, dst, None, None)
    A_ = (o_t.data_ptr(), g_t.data_ptr())
    assert dcall(buf.data_ptr() + 4, dt.data_ptr(), K, df.data_ptr(), C, 0, *A_) == 1  # a misaligned ray array
    assert dcall(buf.data_ptr(), dt.data_ptr(), K + 1, df.data_ptr(), C, 0, *A_) == 1
    assert dcall(buf.data_ptr(), None, K, df.data_ptr(), C, 0, *A_) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, None, C, 0, *A_) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, df.data_ptr(), 65, 0, *A_) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, df.data_ptr(), C, 4, *A_) == 1
    assert dcall(buf.data_ptr(), dt.data_ptr(), K, df.data_ptr(), C, 0, None, None) == 1
    torch.cuda.synchronize()
    assert bool(torch.all(o_t == 7.0)) and bool(torch.all(g_t == 7.0))
    rays_t = to_cuda(rows)
    assert dcall(rays_t.data_ptr(), dt.data_ptr(), K, df.data_ptr(), C, 0, *A_) == 0  # (tr == NULL: the workspace)
    torch.cuda.synchronize()
    want = device().radiance_gradient(vr_scene(name), o, d, t, f, None, None, q, gaussians=False, features_grad=False, grad_q=True)
    assert same_bits(o_t.cpu().numpy(), want) and bool(torch.all(torch.isfinite(g_t))) and float(g_t.abs().max()) > 0


# ------------------------------------------------------------------------------------------------
# 10. the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches(tmp_path):
    from test_gpu_query_grad import sphere_rays
    name, K, C = "250_random", 17, 5
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run(["make", "-C", tools], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d, tmax = sphere_rays(name)
    f = RR.features_of(250, C)
    path, fpath = tmp_path / "rays.bin", tmp_path / "features.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<II", 256, 0))
        fh.write(np.concatenate([o, d, tmax[:, None]], 1).astype("<f4").tobytes())
    with open(fpath, "wb") as fh:
        fh.write(struct.pack("<II", 250, C))
        fh.write(f.astype("<f4").tobytes())
    r = subprocess.run([os.path.join(tools, "vol_render"), "--scene", scene_path(name + ".txt"), "--query-radiance-grad", str(path), str(K),
                        str(fpath)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = {}
    for tag, count, width in (("Rg", 250, 10), ("Rf", 250, C), ("Rq", 256, K), ("Rt", 256, K)):
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(tag + " ")]
        assert [int(v[1]) for v in lines] == list(range(count)) and all(len(v) == 2 + width for v in lines), tag
        words[tag] = np.array([[int(h, 16) for h in v[2:]] for v in lines], np.uint32).view(np.float32)
    t = np.ascontiguousarray((tmax[:, None] * np.arange(1, K + 1, dtype=np.float32)[None]) / np.float32(K))
    q = np.ascontiguousarray(np.repeat((tmax / np.float32(K))[:, None], K, 1))
    assert t.dtype == q.dtype == np.float32
    dev, sc, osc = device(), vr_scene(name), GR.oracle_scene(name)
    gq, gt = dev.radiance_gradient(sc, o, d, t, f, None, None, q, gaussians=False, features_grad=False, grad_q=True, grad_tau=True)
    assert same_bits(words["Rq"], gq) and same_bits(words["Rt"], gt) and np.abs(gq).max() > 0
    # the rest differ from Device.radiance_gradient's by the order of the atomic adds alone: well inside the bound of test 1
    g, gf = dev.radiance_gradient(sc, o, d, t, f, None, None, q)
    Sf, Sr, Sp, _ = RG.scales(osc, o, d, t, q, f, forward_tr(dev, sc, o, d, t), None, None, gt, reach=9.0)
    e_g, e_f = np.abs(words["Rg"].astype(np.float64) - g), np.abs(words["Rf"].astype(np.float64) - gf)
    print(f"C++ mirror: max |mirror - Device| / scale: grad {ratio(e_g, Sf + Sp):.3e}, grad_features {ratio(e_f, Sr):.3e}")
    assert np.abs(g).max() > 0 and np.abs(gf).max() > 0
    assert np.all(e_g <= (SR.BOUND + E23) * Sf + (GR.BOUND + E23) * Sp) and np.all(e_f <= (SR.BOUND + E23) * Sr)
