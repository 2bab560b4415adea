#!/usr/bin/env python
"""Throughput of the batched mixture queries (Device.query_transmittance / query_events / query_sigma) on the
benchmark's 1M-Gaussian make_random scene: 2^22 camera-like rays with tmax = inf, the same rays for the events,
2^22 points uniform in the scene's bounds. Inputs live on the device (torch tensors: the `_device` entry points,
rays packed on the device), every query is warmed up, and the figure is the median of timed repeats between HIP
events on torch's current stream. Prints one JSON line and, with --out, writes it to a file.

    python tools/query_bench.py [--gaussians 1000000] [--rays 4194304] [--points 4194304] [--repeats 5] [--out F]
                                [--flight-scene FILE] [--only all|mixture|flight|grad|raygrad|upload|sigmagrad|profile|features|radiance|radiance_grad]

--only grad times the optical-depth gradient query (Device.query_transmittance_grad, unit weights, moving and frozen
bounds) beside the tau query on the same rays, on --flight-scene and on the make_random scene (--gaussians 0 skips it).
--only raygrad does the same for the ray gradient (Device.query_transmittance_ray_grad, moving and frozen bounds, and
with unit=True on the same stored directions).
--only sigmagrad times the sigma gradient query (Device.query_sigma_grad, weights None: both outputs, positions only,
Gaussians only) beside query_sigma on the same points, on a make_random scene of --gaussians Gaussians: --points points,
point i in or just outside Gaussian i mod N (mean + chol(cov) r u, u a uniform direction, r uniform in [0, 3.3]).
--only features times the feature query (Device.evaluate_features with the mass and the counts) at C = 1, 3 and 48 channels
and its gradient with all three outputs (Device.features_gradient, signed weights) beside query_sigma and
query_sigma_grad (both outputs) on sigmagrad's points, each both with one call per timed interval and with ten (the device
stays busy, which hides the host's time per call).
--only profile times the transmittance profile (Device.query_transmittance_profile, --profile-k samples per ray, ascending
through the cloud, a row per ray) beside K calls of the tau query on the same rays, and its gradient
(Device.query_transmittance_profile_grad, unit weights) beside the gradient query on the n K expanded rays, on
--flight-scene and on the make_random scene (--gaussians 0 skips it); --profile-forward-only leaves the gradients out.
Each comparison reports the existing query's own spread over the repeats: a difference counts from three times that.
--only radiance times the radiance query (Device.radiance with the opacity: one call) against the composition it replaces
(Device.query_transmittance_profile, Device.evaluate_features with the mass at the n K points, and the torch sum), on a
make_random scene of --gaussians Gaussians with --rays rays, K = 64 samples per ray through the cloud (a row per ray, midpoint
weights) and C = 3 and 48 channels. One process, one warm-up of each side, then the two sides alternate --repeats times; the
medians, each side's spread (max - min), the peak device memory of one call of each side over what is resident before it,
and the largest |fused - composition| over S = sum_k |q| T F_abs beside the tests' bound 2^-22 (the composition summed
again in double for this; entries whose S is below 2^-100, where the f32 result underflows, are counted apart).
--only radiance_grad times the fused backward of that query (Device.radiance_gradient with the forward's Tr: the Gaussians'
and the rows' gradients in one call) against the composed backward it replaces (autograd.radiance's: the n K points, the
weights q T gL, Device.features_gradient, Device.evaluate_features, Device.query_transmittance_profile_grad and the sum of the
two (N, 10) results), on the radiance section's scene, rays, samples and channels and by its rules: one process, a warm-up of
each side, the sides alternating --repeats times, medians and spreads (max - min), torch's peak allocation of one call of each
side, and the library's own workspace sizes of the fused side from the shape. It also times the fused side's parts: the walk
without atomics (grad_q and grad_tau alone), the walk with the rows' adds alone (grad_features), and the profile gradient
query with grad_tau as weights, which is what the second pass runs.
--only upload times getting a scene whose parameters live in torch tensors on the GPU onto the device, on --flight-scene
and on make_random scenes of 100 000 and --gaussians Gaussians: (a) a copy to the host, Scene.from_gaussians and
Device.upload with the host builder, (b) the same with device_bvh = 1, (c) Device.upload_gaussians. A host clock
around each call (every one ends in a synchronise), one warm-up, the median of --repeats; (b) and (c) alternate in
one process. Then autograd's optical depth, forward plus backward on 2^20 of the rays at --gaussians Gaussians, with
the parameters copied to the host (optical_depth) and resident (optical_depth_resident).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dg-vol-renderer_amd"))

import vr_amd as vr  # noqa: E402

CAM_POS = np.array([0.0, 1.0, 6.0], np.float32)  # tests/main.cpp:21-34, as bench.py
CAM_VIEW = np.array([0.0, 0.0, -1.0], np.float32)
FOV = np.float32(0.25 * np.pi)


def camera_rays(n):
    """The primary rays of a square pinhole frame of n pixels (camera.h:45-53), unnormalised directions."""
    side = int(round(n ** 0.5))
    assert side * side == n, "--rays must be a square number"
    cam = vr.Pinhole_Camera(CAM_POS, CAM_VIEW, FOV).basis()
    u = 1.0 - (np.arange(side, dtype=np.float32) + 0.5) / side * 2.0
    v = (np.arange(side, dtype=np.float32) + 0.5) / side * 2.0 - 1.0
    uu, vv = np.meshgrid(u, v)
    o = cam["position"] + uu[..., None] * cam["right"] + vv[..., None] * cam["up"]
    d = cam["pinhole"] - o
    return o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None)
    ap.add_argument("--flight-scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "1000_random.txt"))
    ap.add_argument("--only", choices=("all", "mixture", "flight", "grad", "raygrad", "upload", "sigmagrad", "profile", "features", "radiance", "radiance_grad"),
                    default="all")
    ap.add_argument("--profile-k", default="8,64", help="samples per ray of --only profile, comma-separated")
    ap.add_argument("--profile-forward-only", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("query_bench: no GPU (there is no CPU path to time)")

    o, d = (torch.tensor(a).cuda() for a in camera_rays(args.rays))
    dev = vr.Device.get(0)

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), ms, out

    res = {"rays": args.rays, "repeats": args.repeats}
    if args.only == "grad":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(grad(args, dev, o, d, timed))
    if args.only == "raygrad":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(raygrad(args, dev, o, d, timed))
    if args.only == "sigmagrad":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(sigmagrad(args, dev, timed))
    if args.only == "features":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(features(args, dev, timed))
    if args.only == "radiance":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(radiance(args, dev, o, d))
    if args.only == "radiance_grad":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(radiance_grad(args, dev, o, d))
    if args.only == "profile":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(profile(args, dev, o, d, timed))
    if args.only == "upload":
        res["command"] = "python tools/query_bench.py " + " ".join(sys.argv[1:])
        res.update(upload(args, dev, o, d))
    if args.only in ("all", "mixture"):
        res.update(mixture(args, dev, o, d, timed))
    if args.only in ("all", "flight"):
        res.update(flight(args, dev, o, d, timed))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def grad(args, dev, o, d, timed):
    """The gradient query and the tau query on the same rays, per scene."""
    scenes = [(os.path.basename(args.flight_scene), vr.Scene.load_GMM(args.flight_scene))]
    if args.gaussians > 0:
        big = vr.Scene(vr.Scene.GAUSSIANS)
        big.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
        scenes.append((f"make_random_{args.gaussians}", big))
    out = []
    for name, scene in scenes:
        dev.upload(scene)
        tau_ms, tau_all, tau = timed(lambda: dev.query_transmittance(scene, o, d, return_tau=True))
        g_ms, g_all, g = timed(lambda: dev.query_transmittance_grad(scene, o, d))
        f_ms, f_all, _ = timed(lambda: dev.query_transmittance_grad(scene, o, d, moving_bounds=False))
        out.append({"scene": name, "gaussians": scene.get_num_primitives(), "tau_ms": tau_ms, "grad_ms": g_ms,
                    "grad_frozen_ms": f_ms, "grad_mrays_s": args.rays / g_ms / 1e3, "grad_over_tau": g_ms / tau_ms,
                    "gaussians_hit": int((g[:, 9] != 0).sum()), "mean_tau": float(tau[1].mean()),
                    "all_ms": {"tau": tau_all, "grad": g_all, "grad_frozen": f_all}})
    return {"grad": out, "timing": "median of HIP-event intervals on torch's current stream, inputs on the device"}


def profile(args, dev, o, d, timed):
    """The profile against K calls of the tau query, and its gradient against the gradient query on the expanded rays."""
    import torch
    scenes = [(os.path.basename(args.flight_scene), vr.Scene.load_GMM(args.flight_scene))]
    if args.gaussians > 0:
        big = vr.Scene(vr.Scene.GAUSSIANS)
        big.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
        scenes.append((f"make_random_{args.gaussians}", big))
    n = o.shape[0]
    out = []
    for name, scene in scenes:
        info = scene.info()
        lo, hi = np.array(list(info.bounds_min), np.float64), np.array(list(info.bounds_max), np.float64)
        dist, rad = float(np.linalg.norm(0.5 * (lo + hi) - CAM_POS)), 0.5 * float(np.linalg.norm(hi - lo))
        dev.upload(scene)
        for K in (int(k) for k in args.profile_k.split(",")):
            row = np.linspace(max(dist - rad, 0.0), dist + rad, K + 1)[1:].astype(np.float32)  # ascending, through the cloud
            t = torch.tensor(np.tile(row, (n, 1))).cuda()
            cols = [t[:, k].contiguous() for k in range(K)]
            s_ms, s_all, single = timed(lambda: [dev.query_transmittance(scene, o, d, tmax=c, return_tau=True)[1] for c in cols])
            p_ms, p_all, prof = timed(lambda: dev.query_transmittance_profile(scene, o, d, t, return_tau=True))
            same = bool((torch.stack(single, 1).view(torch.int32) == prof[1].view(torch.int32)).all())
            spread = max(s_all) - min(s_all)
            r = {"scene": name, "gaussians": scene.get_num_primitives(), "K": K, "t_first": float(row[0]), "t_last": float(row[-1]),
                 "single_x_K_ms": s_ms, "profile_ms": p_ms, "single_over_profile": s_ms / p_ms, "single_spread_ms": spread,
                 "profile_not_slower": bool(p_ms <= s_ms + 3.0 * spread), "tau_same_bits": same,
                 "mean_tau_last": float(prof[1][:, -1].mean()), "all_ms": {"single_x_K": s_all, "profile": p_all}}
            if not args.profile_forward_only:
                eo, ed, et = o.repeat_interleave(K, 0), d.repeat_interleave(K, 0), t.reshape(-1).contiguous()
                e_ms, e_all, ge = timed(lambda: dev.query_transmittance_grad(scene, eo, ed, None, tmax=et))
                del eo, ed, et
                g_ms, g_all, gp = timed(lambda: dev.query_transmittance_profile_grad(scene, o, d, t))
                gspread = max(e_all) - min(e_all)
                scale = float(ge.abs().max())
                r.update({"expanded_grad_ms": e_ms, "profile_grad_ms": g_ms, "expanded_over_profile_grad": e_ms / g_ms,
                          "expanded_grad_spread_ms": gspread, "profile_grad_not_slower": bool(g_ms <= e_ms + 3.0 * gspread),
                          "grad_max_abs_difference_over_max": float((ge - gp).abs().max()) / scale if scale > 0 else 0.0})
                r["all_ms"].update({"expanded_grad": e_all, "profile_grad": g_all})
            out.append(r)
    return {"profile": out, "library": os.path.basename(vr._lib.LIB_PATH),
            "timing": "median of HIP-event intervals on torch's current stream after the warm-up, inputs on the device; "
                      "spread = max - min of the existing query's intervals, a difference counts from 3 spreads"}


def radiance(args, dev, o, d):
    """The fused radiance query against profile + features at n K points + the torch sum, alternating in one process."""
    import torch
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
    info = scene.info()
    lo, hi = np.array(list(info.bounds_min), np.float64), np.array(list(info.bounds_max), np.float64)
    dist, rad = float(np.linalg.norm(0.5 * (lo + hi) - CAM_POS)), 0.5 * float(np.linalg.norm(hi - lo))
    dev.upload(scene)
    n, N, K = o.shape[0], scene.get_num_primitives(), 64
    edges = np.linspace(max(dist - rad, 0.0), dist + rad, K + 1)
    t = torch.tensor(np.tile((0.5 * (edges[1:] + edges[:-1])).astype(np.float32), (n, 1))).cuda()
    q = torch.tensor(np.tile(np.diff(edges).astype(np.float32), (n, 1))).cuda()
    # the library's normalisation, for the composition's points (f32 products and sums in its order)
    dn = d / torch.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))[:, None]

    def interval(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), got

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20

    out = []
    for C in (3, 48):
        f = torch.tensor(np.random.default_rng(7).uniform(-1, 1, (N, C)).astype(np.float32)).cuda()

        def fused():
            return dev.radiance(scene, o, d, t, f, q, return_opacity=True)

        def composed(feats=f):
            tr = dev.query_transmittance_profile(scene, o, d, t)
            x = (o[:, None, :] + t[:, :, None] * dn[:, None, :]).reshape(-1, 3)
            F, mass = dev.evaluate_features(scene, x, feats, return_mass=True)
            w = q * tr
            return (w[:, :, None] * F.reshape(n, K, -1)).sum(1), (w * mass.reshape(n, K)).sum(1), w

        for _ in range(max(1, args.warmup)):
            a, b = fused(), composed()
        # the comparison, apart from the timed path: the composition's sums again in double, S = sum_k |q| T F_abs
        def in_double(feats):
            tr = dev.query_transmittance_profile(scene, o, d, t)
            x = (o[:, None, :] + t[:, :, None] * dn[:, None, :]).reshape(-1, 3)
            F = dev.evaluate_features(scene, x, feats).reshape(n, K, -1).double()
            return ((q.double() * tr.double())[:, :, None] * F).sum(1), ((q.double() * tr.double()).abs()[:, :, None] * F).sum(1)
        ref, S = in_double(f)[0], in_double(f.abs())[1]
        err = (a[0].double() - ref).abs()
        # (an entry whose S lies below 2^-100 is counted apart: there the f32 result itself underflows, and its last
        # rounding is no longer 2^-24 of it)
        normal = S >= 2.0 ** -100
        rel = torch.where(normal, err / S, torch.zeros_like(S))
        ratio, over = float(rel.max()), int((normal & (err > 2.0 ** -22 * S)).sum())
        tiny = int(((S > 0) & ~normal).sum())
        del S, err, b, ref, rel, normal
        fm, cm = [], []
        for _ in range(args.repeats):
            fm.append(interval(fused)[0])
            cm.append(interval(composed)[0])
        f_ms, c_ms = statistics.median(fm), statistics.median(cm)
        f_sp, c_sp = max(fm) - min(fm), max(cm) - min(cm)
        out.append({"scene": f"make_random_{args.gaussians}", "gaussians": N, "rays": n, "K": K, "C": C, "fused_ms": f_ms,
                    "composition_ms": c_ms, "composition_over_fused": c_ms / f_ms, "fused_spread_ms": f_sp,
                    "composition_spread_ms": c_sp, "fused_faster_by_more_than_the_spreads": bool(c_ms - f_ms > max(f_sp, c_sp)),
                    "fused_peak_mib": peak(fused), "composition_peak_mib": peak(composed),
                    "max_difference_over_S": ratio, "bound": 2.0 ** -22,
                    "entries_over_the_bound": over, "entries": n * C, "entries_with_S_below_2^-100": tiny, "mean_opacity": float(a[1].mean()),
                    "all_ms": {"fused": fm, "composition": cm}})
    return {"radiance": out, "library": os.path.basename(vr._lib.LIB_PATH),
            "timing": "HIP-event intervals on torch's current stream, the two sides alternating after a warm-up of each, inputs on "
                      "the device; spread = max - min of a side's intervals; peak = torch's peak allocation during one call over "
                      "what was allocated before it (the library's own workspaces, n K floats of Tr for the fused side, are not "
                      "torch's and are not counted on either side)"}


def radiance_grad(args, dev, o, d):
    """The fused radiance backward against the composed one (autograd.radiance's), alternating in one process."""
    import torch
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
    info = scene.info()
    lo, hi = np.array(list(info.bounds_min), np.float64), np.array(list(info.bounds_max), np.float64)
    dist, rad = float(np.linalg.norm(0.5 * (lo + hi) - CAM_POS)), 0.5 * float(np.linalg.norm(hi - lo))
    dev.upload(scene)
    n, N, K = o.shape[0], scene.get_num_primitives(), 64
    edges = np.linspace(max(dist - rad, 0.0), dist + rad, K + 1)
    t = torch.tensor(np.tile((0.5 * (edges[1:] + edges[:-1])).astype(np.float32), (n, 1))).cuda()
    q = torch.tensor(np.tile(np.diff(edges).astype(np.float32), (n, 1))).cuda()
    dn = (d / torch.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))[:, None]).contiguous()

    def interval(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), got

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20

    out = []
    for C in (3, 48):
        rng = np.random.default_rng(7)
        f = torch.tensor(rng.uniform(-1, 1, (N, C)).astype(np.float32)).cuda()
        gL = torch.tensor(rng.uniform(-1, 1, (n, C)).astype(np.float32)).cuda()
        gA = torch.tensor(rng.uniform(-1, 1, n).astype(np.float32)).cuda()
        tr = dev.radiance(scene, o, dn, t, f, q, unit=True, return_tr=True)[1]

        def fused():
            return dev.radiance_gradient(scene, o, dn, t, f, gL, gA, q, tr, unit=True)

        def composed():  # autograd._Radiance.backward, line for line
            gL64, gA64 = gL.to(torch.float64), gA.to(torch.float64)
            x = (o[:, None, :] + t[:, :, None] * dn[:, None, :]).reshape(-1, 3).contiguous()
            valid = torch.isfinite(t) & (t >= 0) & torch.isfinite(tr)
            qt = q.to(torch.float64) * tr.to(torch.float64)
            qt = torch.where(valid, qt, torch.zeros_like(qt))
            x = torch.where(valid.reshape(-1, 1), x, torch.full_like(x, float("nan")))
            w = (qt[:, :, None] * gL64[:, None, :]).reshape(-1, C).to(torch.float32).contiguous()
            u = (qt * gA64[:, None]).reshape(-1).to(torch.float32).contiguous()
            g, gf = dev.features_gradient(scene, x, f, w, u)
            F, mass = dev.evaluate_features(scene, x, f, return_mass=True)
            s = (F.reshape(n, K, C).to(torch.float64) * gL64[:, None, :]).sum(2) + mass.reshape(n, K).to(torch.float64) * gA64[:, None]
            wp = torch.where(valid, -qt * s, torch.zeros_like(s)).to(torch.float32).contiguous()
            gp = dev.query_transmittance_profile_grad(scene, o, dn, t, wp)
            return (g.to(torch.float64) + gp.to(torch.float64)).to(torch.float32), gf

        def rows_only():
            return dev.radiance_gradient(scene, o, dn, t, f, gL, gA, q, tr, unit=True, gaussians=False, features_grad=False, grad_q=True,
                                         grad_tau=True)

        def features_only():
            return dev.radiance_gradient(scene, o, dn, t, f, gL, gA, q, tr, unit=True, gaussians=False)

        for _ in range(max(1, args.warmup)):
            a, b = fused(), composed()
            gt = rows_only()[1]
            features_only()
            dev.query_transmittance_profile_grad(scene, o, dn, t, gt)
        diff = [float((x.double() - y.double()).abs().max() / y.double().abs().max()) for x, y in zip(a, b)]
        del a, b
        fm, cm = [], []
        for _ in range(args.repeats):
            fm.append(interval(fused)[0])
            cm.append(interval(composed)[0])
        parts = {name: statistics.median(interval(fn)[0] for _ in range(args.repeats))
                 for name, fn in (("walk_without_atomics_ms", rows_only), ("walk_with_the_rows_adds_ms", features_only),
                                  ("profile_gradient_of_grad_tau_ms", lambda: dev.query_transmittance_profile_grad(scene, o, dn, t, gt)))}
        f_ms, c_ms = statistics.median(fm), statistics.median(cm)
        f_sp, c_sp = max(fm) - min(fm), max(cm) - min(cm)
        out.append({"scene": f"make_random_{args.gaussians}", "gaussians": N, "rays": n, "K": K, "C": C, "fused_ms": f_ms,
                    "composed_ms": c_ms, "composed_over_fused": c_ms / f_ms, "fused_spread_ms": f_sp, "composed_spread_ms": c_sp,
                    "fused_faster_by_more_than_the_spreads": bool(c_ms - f_ms > max(f_sp, c_sp)), "fused_parts": parts,
                    "fused_torch_peak_mib": peak(fused), "composed_torch_peak_mib": peak(composed),
                    "fused_workspace_mib": {"s": n * K * 8 / 2.0 ** 20, "grad_tau": n * K * 4 / 2.0 ** 20, "tr": 0.0,
                                            "staging": (10 + C) * N * 8 / 2.0 ** 20},
                    "max_difference_over_max": {"grad": diff[0], "grad_features": diff[1]},
                    "all_ms": {"fused": fm, "composed": cm}})
    return {"radiance_grad": out, "library": os.path.basename(vr._lib.LIB_PATH),
            "timing": "HIP-event intervals on torch's current stream, the two sides alternating after a warm-up of each, inputs and the "
                      "forward's Tr on the device; spread = max - min of a side's intervals; torch peak = torch's peak allocation during "
                      "one call over what was allocated before it; the fused side's workspaces are the library's own allocations, which "
                      "torch does not see: their sizes are computed from the shape (vr_query_host.cpp), not measured"}


def sigmagrad(args, dev, timed):
    """The sigma gradient query in its three forms and the sigma query on the same points."""
    import torch
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
    g = scene.gaussians().astype(np.float64)
    c6 = g[:, 3:9]
    cov = np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(args.points, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = rng.uniform(0.0, 3.3, args.points)
    k = np.arange(args.points) % len(g)
    p = torch.tensor((g[k, 0:3] + np.einsum("nij,nj->ni", np.linalg.cholesky(cov)[k], r[:, None] * u)).astype(np.float32)).cuda()
    dev.upload(scene)
    s_ms, s_all, sg = timed(lambda: dev.query_sigma(scene, p, return_active=True))
    b_ms, b_all, both = timed(lambda: dev.query_sigma_grad(scene, p, gaussians=True, positions=True))
    x_ms, x_all, _ = timed(lambda: dev.query_sigma_grad(scene, p, gaussians=False, positions=True))
    g_ms, g_all, _ = timed(lambda: dev.query_sigma_grad(scene, p))
    out = {"scene": f"make_random_{args.gaussians}", "gaussians": scene.get_num_primitives(), "points": args.points,
           "sigma_ms": s_ms, "both_ms": b_ms, "positions_ms": x_ms, "gaussians_ms": g_ms,
           "both_over_sigma": b_ms / s_ms, "positions_over_sigma": x_ms / s_ms, "gaussians_over_sigma": g_ms / s_ms,
           "both_mpoints_s": args.points / b_ms / 1e3, "mean_active": float(sg[1].float().mean()),
           "max_active": int(sg[1].max()), "gaussians_holding_points": int((both[0][:, 9] != 0).sum()),
           "all_ms": {"sigma": s_all, "both": b_all, "positions": x_all, "gaussians": g_all}}
    return {"sigmagrad": out, "timing": "median of HIP-event intervals on torch's current stream, inputs on the device; "
                                        "each call allocates its result tensors"}


def features(args, dev, timed):
    """The feature query at C = 1, 3 and 48 channels and its gradient with all three outputs, beside the sigma query and
    the sigma gradient (both outputs) on the same points: sigmagrad's points on a make_random scene."""
    import torch
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
    g = scene.gaussians().astype(np.float64)
    c6 = g[:, 3:9]
    cov = np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(args.points, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = rng.uniform(0.0, 3.3, args.points)
    k = np.arange(args.points) % len(g)
    p = torch.tensor((g[k, 0:3] + np.einsum("nij,nj->ni", np.linalg.cholesky(cov)[k], r[:, None] * u)).astype(np.float32)).cuda()
    dev.upload(scene)
    out = {"scene": f"make_random_{args.gaussians}", "gaussians": scene.get_num_primitives(), "points": args.points, "all_ms": {}}

    def both(name, fn):
        """(one call per interval, a tenth of ten calls per interval): the second keeps the device busy, so the host's
        time per call (argument checks, result tensors) is hidden where the first includes it."""
        one, one_all, res = timed(fn)
        ten, ten_all, _ = timed(lambda: [fn() for _ in range(10)])
        out["all_ms"][name], out["all_ms"][name + "_x10"] = one_all, ten_all
        return one, ten / 10.0, res

    s1, s10, sg = both("sigma", lambda: dev.query_sigma(scene, p, return_active=True))
    g1, g10, _ = both("sigma_grad", lambda: dev.query_sigma_grad(scene, p, gaussians=True, positions=True))
    out.update({"sigma_ms": s1, "sigma_busy_ms": s10, "sigma_grad_ms": g1, "sigma_grad_busy_ms": g10})
    for C in (1, 3, 48):
        f = torch.tensor(rng.uniform(-1, 1, (len(g), C)).astype(np.float32)).cuda()
        w = torch.tensor(rng.uniform(-1, 1, (args.points, C)).astype(np.float32)).cuda()
        m = torch.tensor(rng.uniform(-1, 1, args.points).astype(np.float32)).cuda()
        fw1, fw10, _ = both(f"features_C{C}", lambda: dev.evaluate_features(scene, p, f, return_mass=True, return_active=True))
        bw1, bw10, _ = both(f"features_grad_C{C}", lambda: dev.features_gradient(scene, p, f, w, m, positions=True))
        out[f"C{C}"] = {"features_ms": fw1, "features_busy_ms": fw10, "features_grad_ms": bw1, "features_grad_busy_ms": bw10,
                        "features_over_sigma": fw1 / s1, "features_busy_over_sigma_busy": fw10 / s10,
                        "features_grad_over_sigma_grad": bw1 / g1, "features_grad_busy_over_sigma_grad_busy": bw10 / g10}
    out["mean_active"], out["max_active"] = float(sg[1].float().mean()), int(sg[1].max())
    return {"features": out, "timing": "median of HIP-event intervals on torch's current stream, inputs on the device; "
                                       "each call allocates its result tensors; *_busy_ms: ten calls per interval, divided by ten"}


def upload(args, dev, o, d):
    """Three ways of getting device-resident parameters onto the device as a scene, and what they cost autograd."""
    import time

    import torch
    from vr_amd import autograd

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def params(scene):
        g = scene.gaussians()
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (g[:, 0:3], g[:, 3:9], g[:, 9], g[:, 10])]

    def from_host(p, device_bvh):
        dev.set_option("device_bvh", device_bvh)
        dev.upload(vr.Scene.from_gaussians(*(t.cpu().numpy() for t in p)), force=True)

    scenes = [(os.path.basename(args.flight_scene), vr.Scene.load_GMM(args.flight_scene))]
    for n in sorted({min(100_000, args.gaussians), args.gaussians} - {0}):
        big = vr.Scene(vr.Scene.GAUSSIANS)
        big.add_random_gaussians(n, seed=args.seed, variant=0)
        scenes.append((f"make_random_{n}", big))
    saved = dev.get_option("device_bvh")
    out = []
    for name, scene in scenes:
        p = params(scene)
        a = [clock(lambda: from_host(p, 0)) for _ in range(args.warmup + args.repeats)][args.warmup:]
        b, c = [], []
        for _ in range(args.warmup + args.repeats):  # alternated: they share the session
            b.append(clock(lambda: from_host(p, 1)))
            c.append(clock(lambda: dev.upload_gaussians(*p)))
        b, c = b[args.warmup:], c[args.warmup:]
        out.append({"scene": name, "gaussians": scene.get_num_primitives(), "host_builder_ms": statistics.median(a),
                    "device_bvh_ms": statistics.median(b), "upload_gaussians_ms": statistics.median(c),
                    "device_bvh_spread_ms": max(b) - min(b), "built_on_device": bool(dev.debug_tree([])["info"]["built_on_device"]),
                    "all_ms": {"host_builder": a, "device_bvh": b, "upload_gaussians": c}})
    dev.set_option("device_bvh", saved)
    res = {"upload": out, "timing": "host clock around each call (each ends in a synchronise), median after one warm-up"}
    if args.gaussians > 0:
        p = params(scenes[-1][1])
        n = min(1 << 20, o.shape[0])
        ro, rd = o[:n].contiguous(), d[:n].contiguous()

        def step(fn):
            q = [t.clone().requires_grad_() for t in p[:3]]
            fn(*q, p[3], ro, rd).sum().backward()

        fb = {}
        for key, fn in (("optical_depth", autograd.optical_depth), ("optical_depth_resident", autograd.optical_depth_resident)):
            ms = [clock(lambda: step(fn)) for _ in range(args.warmup + args.repeats)][args.warmup:]
            fb[key + "_ms"] = statistics.median(ms)
            fb.setdefault("all_ms", {})[key] = ms
        fb.update({"rays": n, "gaussians": scenes[-1][1].get_num_primitives()})
        res["forward_backward"] = fb
    return res


def raygrad(args, dev, o, d, timed):
    """The ray-gradient query and the tau query on the same rays, per scene."""
    import torch
    scenes = [(os.path.basename(args.flight_scene), vr.Scene.load_GMM(args.flight_scene))]
    if args.gaussians > 0:
        big = vr.Scene(vr.Scene.GAUSSIANS)
        big.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
        scenes.append((f"make_random_{args.gaussians}", big))
    out = []
    for name, scene in scenes:
        dev.upload(scene)
        tau_ms, tau_all, tau = timed(lambda: dev.query_transmittance(scene, o, d, return_tau=True))
        g_ms, g_all, g = timed(lambda: dev.query_transmittance_ray_grad(scene, o, d))
        f_ms, f_all, _ = timed(lambda: dev.query_transmittance_ray_grad(scene, o, d, moving_bounds=False))
        u_ms, u_all, _ = timed(lambda: dev.query_transmittance_ray_grad(scene, o, d, unit=True))
        out.append({"scene": name, "gaussians": scene.get_num_primitives(), "tau_ms": tau_ms, "raygrad_ms": g_ms,
                    "raygrad_frozen_ms": f_ms, "raygrad_unit_ms": u_ms, "raygrad_mrays_s": args.rays / g_ms / 1e3,
                    "raygrad_over_tau": g_ms / tau_ms, "rays_hit": int((g[3] != 0).sum()),
                    "tau_same_bits": bool((g[3].view(torch.int32) == tau[1].view(torch.int32)).all()),
                    "mean_tau": float(tau[1].mean()),
                    "all_ms": {"tau": tau_all, "raygrad": g_all, "raygrad_frozen": f_all, "raygrad_unit": u_all}})
    return {"raygrad": out, "timing": "median of HIP-event intervals on torch's current stream, inputs on the device"}


def flight(args, dev, o, d, timed):
    """The free-flight query on --flight-scene, and query_events for the same rays on the same scene."""
    import torch
    scene = vr.Scene.load_GMM(args.flight_scene)
    dev.upload(scene)
    tau = torch.tensor((-np.log1p(-np.random.default_rng(7).random(args.rays))).astype(np.float32)).cuda()
    t_ms, t_all, t = timed(lambda: dev.query_free_flight(scene, o, d, tau))
    f_ms, f_all, _ = timed(lambda: dev.query_free_flight(scene, o, d, tau, return_albedo=True, return_active=True))
    ev_ms, ev_all, ev = timed(lambda: dev.query_events(scene, o, d))
    return {
        "flight_scene": os.path.basename(args.flight_scene), "flight_ms": t_ms, "flight_mrays_s": args.rays / t_ms / 1e3,
        "flight_full_ms": f_ms, "flight_full_mrays_s": args.rays / f_ms / 1e3,
        "flight_scattering_share": float((t >= 0).float().mean()),
        "flight_events_ms": ev_ms, "flight_events_mrays_s": args.rays / ev_ms / 1e3,
        "flight_events_per_ray": int(ev[0][-1]) / args.rays,
        "flight_all_ms": {"t": t_all, "t_albedo_active": f_all, "events": ev_all},
    }


def mixture(args, dev, o, d, timed):
    import torch
    scene = vr.Scene(vr.Scene.GAUSSIANS)
    scene.add_random_gaussians(args.gaussians, seed=args.seed, variant=0)
    info = scene.info()
    lo, hi = np.array(list(info.bounds_min), np.float32), np.array(list(info.bounds_max), np.float32)
    p = torch.tensor(np.random.default_rng(7).uniform(lo, hi, (args.points, 3)).astype(np.float32)).cuda()
    dev.upload(scene)
    tr_ms, tr_all, tr = timed(lambda: dev.query_transmittance(scene, o, d))
    tau_ms, tau_all, _ = timed(lambda: dev.query_transmittance(scene, o, d, return_tau=True))
    ev_ms, ev_all, ev = timed(lambda: dev.query_events(scene, o, d))
    sg_ms, sg_all, sg = timed(lambda: dev.query_sigma(scene, p, return_active=True))
    n_events = int(ev[0][-1])
    return {
        "gaussians": args.gaussians, "points": args.points,
        "transmittance_ms": tr_ms, "transmittance_mrays_s": args.rays / tr_ms / 1e3,
        "transmittance_tau_ms": tau_ms, "transmittance_tau_mrays_s": args.rays / tau_ms / 1e3,
        "events": n_events, "events_per_ray": n_events / args.rays, "events_ms": ev_ms,
        "events_mevents_s": n_events / ev_ms / 1e3, "events_mrays_s": args.rays / ev_ms / 1e3,
        "sigma_ms": sg_ms, "sigma_mpoints_s": args.points / sg_ms / 1e3,
        "mean_active": float(sg[1].float().mean()), "mean_transmittance": float(tr.mean()),
        "all_ms": {"transmittance": tr_all, "transmittance_tau": tau_all, "events": ev_all, "sigma": sg_all},
        "timing": "median of HIP-event intervals on torch's current stream; the events figure spans both passes, "
                  "the count pass's host synchronisation and the allocation of the output tensors",
    }


if __name__ == "__main__":
    main()
