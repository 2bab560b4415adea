#!/usr/bin/env python
"""A ray grid against the frame it restates: the benchmark's C3 workload (1920x1080, 100k Gaussians
of the make_random distribution, 20 environment samples, t_eps 1e-6) rendered by vr_render_tiles_device for the
whole frame and by vr_render_rays_device on the camera's own rays, device-resident, on one context. After one
warm-up of each, the two are timed in alternation: the median of --repeats HIP-event intervals on torch's current
stream (the grid's interval includes its extent reduction and the 4-byte read-back), with the per-stage stage_ms
of both from vr_get_stats. The grid must equal the frame bit for bit. Prints one JSON line; --out writes it too.

    python tools/ray_grid_bench.py [--config c3] [--env-samples 20] [--t-eps 1e-6] [--repeats 5] [--out F]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workloads' scenes and camera; loads torch's HIP runtime first)
import vr_amd as vr  # noqa: E402
from vr_amd import _lib as L  # noqa: E402


def camera_rays(cam, W, H):
    """The pinhole camera's primary rays in the device's own f32 arithmetic (vr_march.h primary_ray: sample_ray's
    normalisation, then the Ray constructor's), vectorised; rows are spot-checked against Camera.sample_ray."""
    f = np.float32
    b = cam.basis()
    uvx = (np.arange(W, dtype=f) + f(0.5)) / f(W)
    uvy = (np.arange(H, dtype=f) + f(0.5)) / f(H)
    u = (f(1.0) - uvx * f(2.0))[None, :, None]
    v = (uvy * f(2.0) - f(1.0))[:, None, None]
    o = ((b["position"] + u * b["right"]) + v * b["up"]).astype(f)
    d = (b["pinhole"] - o).astype(f)
    for _ in range(2):
        s = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        d = (d / np.sqrt(s)[..., None]).astype(f)
    for x, y in ((0, 0), (W - 1, H - 1), (W // 3, H // 2)):
        r = cam.sample_ray(((x + f(0.5)) / f(W), (y + f(0.5)) / f(H)))
        assert np.array_equal(r.origin, o[y, x]) and np.array_equal(r.direction, d[y, x]), (x, y)
    return o, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--env-samples", type=int, default=20)
    ap.add_argument("--t-eps", type=float, default=1e-6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ray_grid_bench: no GPU (there is no CPU path to time)")

    scene, W, H = bench.build_scene(args.config, args.seed)
    cam = vr.Pinhole_Camera(bench.CAM_POS, bench.CAM_VIEW, bench.FOV)
    integ = vr.RayMarchingGaussians(cam, env_samples=args.env_samples, t_eps=args.t_eps)
    dev = vr.Device.get(0)
    dev.upload(scene)
    o, d = camera_rays(cam, W, H)
    rays = torch.from_numpy(vr._pack_ray_grid_numpy(o, d, True, W, H, W * H)).cuda()
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    grid = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    tr = torch.empty((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ntiles = vr.num_tiles(W, H)

    def run_frame():
        dev.render_tiles_device(cam, integ.params, W, H, 0, 1, ntiles, False, frame.data_ptr(), stream)

    def run_grid():
        L.check(L.lib().vr_render_rays_device(dev._h, rays.data_ptr(), W, H, ctypes.byref(integ.params), grid.data_ptr(),
                                              tr.data_ptr(), stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dev.synchronize()  # the frame's outcome (raises if it is invalid)
        return e0.elapsed_time(e1), dev.stats()

    for fn in (run_frame, run_grid):  # warm-up: sizes the record buffers and the step table
        for attempt in range(3):
            try:
                timed(fn)
                break
            except vr.VRError as e:
                if e.status != L.VR_ERR_RETRY or attempt == 2:
                    raise
    ms = {"frame": [], "grid": []}
    stages = {"frame": [], "grid": []}
    for _ in range(args.repeats):  # alternate the two sides
        for name, fn in (("frame", run_frame), ("grid", run_grid)):
            t, st = timed(fn)
            ms[name].append(t)
            stages[name].append(st)
    equal = bool(torch.equal(frame.view(torch.int32), grid.view(torch.int32)))
    med = {k: statistics.median(v) for k, v in ms.items()}

    def stage_median(name):
        return {s: statistics.median(st["stage_ms"][s] for st in stages[name]) for s in vr.Device.STAGES}

    res = {
        "config": args.config, "width": W, "height": H, "gaussians": scene.get_num_primitives(),
        "env_samples": args.env_samples, "t_eps": args.t_eps, "repeats": args.repeats,
        "frame_ms": med["frame"], "grid_ms": med["grid"], "grid_over_frame": med["grid"] / med["frame"],
        "frame_stage_ms": stage_median("frame"), "grid_stage_ms": stage_median("grid"),
        "frame_kernel_ms": statistics.median(st["kernel_ms"] for st in stages["frame"]),
        "grid_kernel_ms": statistics.median(st["kernel_ms"] for st in stages["grid"]),
        "all_ms": ms, "grid_equals_frame": equal,
        "scatter_records": {k: stages[k][-1]["scatter_records"] for k in stages},
        "mean_transmittance": float(tr.mean()),
        "timing": "median of HIP-event intervals on torch's current stream, the two sides alternated after one warm-up "
                  "each; the grid's interval includes the extent reduction and its 4-byte read-back, kernel_ms / "
                  "stage_ms (vr_get_stats) do not",
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        sys.exit("ray_grid_bench: the grid differs from the frame")


if __name__ == "__main__":
    main()
