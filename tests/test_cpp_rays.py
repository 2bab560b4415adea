"""HipIntegrator::render_rays (3dg-vol-renderer_amd/include/vr/integrator.h), the C++ mirror of the ray-grid entry
point, driven through the small program tests/cpp_rays.cpp built against the headers and the in-tree library.

CPU: the program builds and runs up to the render. GPU: the grid it renders along the main camera's own rays
equals the Python mirror's grid, transmittance and frame bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import CAM_POS, FOV, ROOT, main_view_dir, scene_path

PKG = os.path.join(ROOT, "3dg-vol-renderer_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_rays") / "cpp_rays")
    r = subprocess.run(["g++", os.path.join(ROOT, "tests", "cpp_rays.cpp"), "-o", out, "-std=c++20", "-O2", "-Wall",
                        f"-I{PKG}/include", f"-I{ROOT}", f"-L{PKG}", "-lvr_hip", f"-Wl,-rpath,{PKG}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cpp_driver_builds_and_loads(exe, tmp_path):
    r = subprocess.run([exe, scene_path("many_gaussians.txt"), "0", "0", "4", str(tmp_path / "o.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scene: 7 primitives" in r.stdout
    r = subprocess.run([exe, str(tmp_path / "missing.txt"), "0", "0", "4", str(tmp_path / "o.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "cpp_rays:" in r.stderr


@pytest.mark.gpu
def test_cpp_render_rays_equals_python(exe, tmp_path):
    import vr_amd as vr
    W, H, env = 40, 24, 4
    out = tmp_path / "o.bin"
    r = subprocess.run([exe, scene_path("250_random.txt"), str(W), str(H), str(env), str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(out, np.float32)
    assert raw.size == 7 * W * H
    grid, tr, frame = raw[:3 * W * H].reshape(H, W, 3), raw[3 * W * H:4 * W * H].reshape(H, W), raw[4 * W * H:].reshape(H, W, 3)
    cam = vr.Pinhole_Camera(CAM_POS, main_view_dir(), FOV)
    o = np.zeros((H, W, 3), np.float32)
    d = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            ray = cam.sample_ray(((x + np.float32(0.5)) / np.float32(W), (y + np.float32(0.5)) / np.float32(H)))
            o[y, x], d[y, x] = ray.origin, ray.direction
    integ = vr.RayMarchingGaussians(cam, env_samples=env)
    rgb, ptr = integ.render_rays(vr.Scene.load_GMM(scene_path("250_random.txt")), o, d, unit=True, return_transmittance=True)
    assert np.array_equal(grid.view(np.uint32), rgb.view(np.uint32))
    assert np.array_equal(tr.view(np.uint32), ptr.view(np.uint32))
    assert np.array_equal(frame.view(np.uint32), grid.view(np.uint32))
    assert len(np.unique(grid.reshape(-1, 3), axis=0)) > 10
