"""vr_amd — Python mirror of the reference's forward-render API over libvr_hip.so.

Names, argument meaning and error behaviour follow wantonsushi/3DG-vol-renderer:

    scene = Scene.load_GMM("scenes/gaussians/many_gaussians.txt")      # scene.h:72-120
    camera = Pinhole_Camera(position, view_dir, fov)                    # camera.h:31-54
    image = Image(512, 512)                                             # image.h:9-20
    RayMarchingGaussians(camera).render(scene, image)                   # test_integrators.h:143-297
    image.make_PPM("output.ppm")                                        # image.h:62-84

Everything runs through the C ABI (include/vr_hip.h); rendering happens on the GPU only. Errors
are raised as VRError (a RuntimeError), as the reference raises std::runtime_error.
"""
import ctypes
import os

import numpy as np

from . import _lib as L
from ._lib import VRError, check, fptr, lib

__all__ = [
    "VRError", "Light", "Scene", "Camera", "Pinhole_Camera", "Orthographic_Camera", "Ray", "Image",
    "Integrator", "RayMarchingGaussians", "PureRayMarching", "RayMarchingSpheres", "FreeFlightGaussians",
    "MultiScatterGaussians", "bits_to_lists", "TestIntegrator", "Device",
    "DeviceScene", "load_xml",
    "num_tiles", "RAY_BATCH_WIDTH",
]


def _v3(x):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(3))
    return a


class Light:
    """scene.h:12-15"""

    def __init__(self, position, intensity):
        self.position = _v3(position)
        self.intensity = _v3(intensity)

    def __repr__(self):
        return f"Light(position={self.position.tolist()}, intensity={self.intensity.tolist()})"


class Scene:
    """Scene (scene.h:17-205). Owns a native vr_scene handle.

    volume_type: "GAUSSIANS" or "SPHERES". Mutations (add_*, env_color) bump `version` so a
    device context re-uploads before the next render.
    """

    GAUSSIANS = L.VR_VOLUME_GAUSSIANS
    SPHERES = L.VR_VOLUME_SPHERES

    def __init__(self, volume_type=GAUSSIANS, _handle=None):
        if _handle is None:
            h = ctypes.c_void_p()
            check(lib().vr_scene_create(int(volume_type), ctypes.byref(h)))
            _handle = h
        self._h = _handle
        self.version = 0

    # ---- loaders ----
    @classmethod
    def load_GMM(cls, filename):
        h = ctypes.c_void_p()
        check(lib().vr_scene_load_gmm(os.fsencode(str(filename)), ctypes.byref(h)))
        return cls(_handle=h)

    @classmethod
    def load_SMM(cls, filename):
        h = ctypes.c_void_p()
        check(lib().vr_scene_load_smm(os.fsencode(str(filename)), ctypes.byref(h)))
        return cls(_handle=h)

    @classmethod
    def load_XML(cls, filename):
        """Mitsuba-subset XML -> (scene, camera, (width, height), integrator_kwargs)."""
        h = ctypes.c_void_p()
        cam = L.vr_camera()
        w, hh = ctypes.c_uint32(), ctypes.c_uint32()
        p = L.vr_render_params()
        check(lib().vr_scene_load_xml(os.fsencode(str(filename)), ctypes.byref(h), ctypes.byref(cam),
                                      ctypes.byref(w), ctypes.byref(hh), ctypes.byref(p)))
        scene = cls(_handle=h)
        camera = Camera._from_struct(cam)
        kw = {"step_size": p.step_size, "env_samples": p.env_samples}
        return scene, camera, (w.value, hh.value), kw

    @classmethod
    def from_gaussians(cls, mean, cov6, density, albedo, lights=(), env_color=None, emission=None):
        """Build a Gaussian scene from arrays (n,3), (n,6) [xx xy xz yy yz zz], (n,), (n,)."""
        s = cls(cls.GAUSSIANS)
        s.add_gaussians(mean, cov6, density, albedo, emission)
        for l in lights:
            s.add_light(l)
        if env_color is not None:
            s.env_color = env_color
        return s

    # ---- mutation ----
    def add_gaussians(self, mean, cov6, density, albedo, emission=None):
        mean = np.asarray(mean, np.float32).reshape(-1, 3)
        n = mean.shape[0]
        cov6 = np.asarray(cov6, np.float32).reshape(n, 6)
        arr = (L.vr_gaussian * max(n, 1))()
        buf = np.frombuffer(arr, dtype=np.float32).reshape(max(n, 1), 14)
        if n:
            buf[:n, 0:3] = mean
            buf[:n, 3:9] = cov6
            buf[:n, 9] = np.asarray(density, np.float32).reshape(n)
            buf[:n, 10] = np.asarray(albedo, np.float32).reshape(n)
            buf[:n, 11:14] = 0.0 if emission is None else np.asarray(emission, np.float32).reshape(n, 3)
        check(lib().vr_scene_add_gaussians(self._h, arr, n))
        self.version += 1

    def add_random_gaussians(self, n, seed=0, variant=0):
        """Synthetic Gaussians with make_random.py's (variant 0) or make_nonuniform_random.py's
        (variant 1) distribution, generated natively (vr_scene_add_random_gaussians)."""
        check(lib().vr_scene_add_random_gaussians(self._h, int(n), int(seed), int(variant)))
        self.version += 1

    def add_spheres(self, center, radius, sigma_a, sigma_s):
        center = np.asarray(center, np.float32).reshape(-1, 3)
        n = center.shape[0]
        arr = (L.vr_sphere * max(n, 1))()
        buf = np.frombuffer(arr, dtype=np.float32).reshape(max(n, 1), 6)
        if n:
            buf[:n, 0:3] = center
            buf[:n, 3] = np.asarray(radius, np.float32).reshape(n)
            buf[:n, 4] = np.asarray(sigma_a, np.float32).reshape(n)
            buf[:n, 5] = np.asarray(sigma_s, np.float32).reshape(n)
        check(lib().vr_scene_add_spheres(self._h, arr, n))
        self.version += 1

    def add_light(self, light):
        l = L.vr_light()
        l.position[:] = [float(v) for v in light.position]
        l.intensity[:] = [float(v) for v in light.intensity]
        check(lib().vr_scene_add_lights(self._h, ctypes.byref(l), 1))
        self.version += 1

    # ---- queries ----
    def info(self):
        i = L.vr_scene_info()
        check(lib().vr_scene_get_info(self._h, ctypes.byref(i)))
        return i

    @property
    def volume_type(self):
        return self.info().volume_type

    def get_num_primitives(self):
        return int(self.info().num_primitives)

    @property
    def lights(self):
        n = int(self.info().num_lights)
        arr = (L.vr_light * max(n, 1))()
        check(lib().vr_scene_get_lights(self._h, arr, n))
        return [Light(list(arr[i].position), list(arr[i].intensity)) for i in range(n)]

    @property
    def env_color(self):
        return np.array(list(self.info().env_color), np.float32)

    @env_color.setter
    def env_color(self, rgb):
        a = _v3(rgb)
        check(lib().vr_scene_set_env_color(self._h, fptr(a)))
        self.version += 1

    def records(self):
        """Precomputed Gaussian records (n, 12): mean3, density, inv_cov 00 01 02 11 12 22, norm, albedo."""
        n = self.get_num_primitives()
        out = np.zeros((n, 12), np.float32)
        check(lib().vr_scene_get_records(self._h, fptr(out), n))
        return out

    def gaussians(self):
        n = self.get_num_primitives()
        arr = (L.vr_gaussian * max(n, 1))()
        check(lib().vr_scene_get_gaussians(self._h, arr, n))
        return np.frombuffer(arr, dtype=np.float32).reshape(max(n, 1), 14)[:n].copy()

    def spheres(self):
        n = self.get_num_primitives()
        arr = (L.vr_sphere * max(n, 1))()
        check(lib().vr_scene_get_spheres(self._h, arr, n))
        return np.frombuffer(arr, dtype=np.float32).reshape(max(n, 1), 6)[:n].copy()

    def unshuffle_tiles_part_device(self, slabs_ptr, first, nslabs, stride, tiles_per_slab, width, height, image_ptr,
                                    stream_ptr=0):
        """Slabs of ranks first .. first + nslabs - 1 of a stride-way split into the frame
        (vr_unshuffle_tiles_part_device)."""
        check(lib().vr_unshuffle_tiles_part_device(self._h, ctypes.c_void_p(slabs_ptr), first, nslabs, stride,
                                                   tiles_per_slab, width, height, ctypes.c_void_p(image_ptr),
                                                   ctypes.c_void_p(stream_ptr)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and L is not None and L._lib is not None:  # (L is None during interpreter teardown)
            L._lib.vr_scene_destroy(h)
            self._h = None


def load_xml(filename):
    return Scene.load_XML(filename)


class Ray:
    """ray.h:7-16 (direction normalised)."""

    def __init__(self, origin, direction):
        self.origin = _v3(origin)
        self.direction = _v3(direction)

    def __call__(self, t):
        return self.origin + np.float32(t) * self.direction


class Camera:
    """camera.h:7-27; the state a constructor leaves behind is a vr_camera struct."""

    def __init__(self):
        self._c = L.vr_camera()

    @classmethod
    def _from_struct(cls, c):
        obj = Pinhole_Camera.__new__(Pinhole_Camera) if c.type == L.VR_CAMERA_PINHOLE else \
            Orthographic_Camera.__new__(Orthographic_Camera)
        obj._c = c
        return obj

    @property
    def struct(self):
        return self._c

    def sample_ray(self, uv):
        o = np.zeros(3, np.float32)
        d = np.zeros(3, np.float32)
        check(lib().vr_camera_sample_ray(ctypes.byref(self._c), float(uv[0]), float(uv[1]), fptr(o), fptr(d)))
        return Ray(o, d)

    def basis(self):
        c = self._c
        return {k: np.array(list(getattr(c, k)), np.float32) for k in ("position", "view_dir", "right", "up", "pinhole")}


class Pinhole_Camera(Camera):
    """camera.h:31-54: Pinhole_Camera(position, view_dir, fov [radians])."""

    def __init__(self, position, view_dir, fov):
        super().__init__()
        p, v = _v3(position), _v3(view_dir)
        check(lib().vr_camera_pinhole(fptr(p), fptr(v), float(fov), ctypes.byref(self._c)))


class Orthographic_Camera(Camera):
    """camera.h:58-74: Orthographic_Camera(position, forward)."""

    def __init__(self, position, forward):
        super().__init__()
        p, v = _v3(position), _v3(forward)
        check(lib().vr_camera_orthographic(fptr(p), fptr(v), ctypes.byref(self._c)))


class Image:
    """image.h:9-106: float RGB framebuffer, row-major, pixel (i, j) at pixels[j, i]."""

    def __init__(self, width, height=None):
        if isinstance(width, (str, os.PathLike)):  # Image(const std::string&) — P6 reader
            w, h = ctypes.c_uint32(), ctypes.c_uint32()
            path = os.fsencode(str(width))
            check(lib().vr_image_read_ppm(path, None, ctypes.byref(w), ctypes.byref(h)))
            self.pixels = np.zeros((h.value, w.value, 3), np.float32)
            check(lib().vr_image_read_ppm(path, fptr(self.pixels), ctypes.byref(w), ctypes.byref(h)))
        else:
            self.pixels = np.zeros((int(height), int(width), 3), np.float32)

    def get_width(self):
        return self.pixels.shape[1]

    def get_height(self):
        return self.pixels.shape[0]

    def get_pixel(self, i, j):
        return self.pixels[j, i].copy()

    def set_pixel(self, i, j, rgb):
        self.pixels[j, i] = rgb

    def make_PPM(self, filename):
        check(lib().vr_image_write_ppm(os.fsencode(str(filename)), fptr(np.ascontiguousarray(self.pixels)),
                                       self.get_width(), self.get_height()))

    def to_uint8(self):
        """Same quantisation as make_PPM: clamp(v * 255, 0, 255) then truncate (image.h:66)."""
        return np.clip(self.pixels * np.float32(255.0), 0.0, 255.0).astype(np.uint8)

    def get_rgba_buffer(self):
        rgb = self.to_uint8()
        return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)


class Device:
    """A device context (vr_ctx). `device` is a GPU index (vr_init) or a tuple of GPU indices: a
    multi-GPU context (vr_init_multi) that splits every frame's tiles over those GPUs and gathers
    them over RCCL (a GPU listed twice rehearses the split on one GPU, gathering with device copies).
    Scenes are uploaded lazily and re-uploaded when they change."""

    _cache = {}

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        if isinstance(device, (tuple, list)):
            devs = (ctypes.c_int32 * len(device))(*[int(d) for d in device])
            check(lib().vr_init_multi(len(device), devs, ctypes.byref(h)))
            device = tuple(int(d) for d in device)
        else:
            check(lib().vr_init(int(device), ctypes.byref(h)))
        self._h = h
        self.device = device
        self._scene_key = None

    @staticmethod
    def count():
        n = ctypes.c_int32()
        check(lib().vr_device_count(ctypes.byref(n)))
        return int(n.value)

    @property
    def num_devices(self):
        return int(lib().vr_ctx_num_devices(self._h))

    @property
    def uses_rccl(self):
        return bool(lib().vr_ctx_uses_rccl(self._h))

    def rank_stats(self, rank):
        """vr_get_rank_stats: one rank's statistics of the last frame (same keys as stats())."""
        s = L.vr_render_stats()
        check(lib().vr_get_rank_stats(self._h, int(rank), ctypes.byref(s)))
        return self._stats_dict(s)

    @classmethod
    def get(cls, device=0):
        if isinstance(device, list):
            device = tuple(device)
        d = cls._cache.get(device)
        if d is None:
            d = cls._cache[device] = cls(device)
        return d

    def upload(self, scene, force=False):
        key = (id(scene), scene.version)
        if force or key != self._scene_key:
            if isinstance(scene, DeviceScene):
                scene._upload_to(self)
            else:
                check(lib().vr_upload_scene(self._h, scene._h))
            self._scene_key = key
            self._scene_ref = scene

    def upload_gaussians(self, mean, cov6, density, albedo, lights=(), env_color=None):
        """vr_upload_gaussians_device: a Gaussian scene straight from device memory. mean (N, 3), cov6 (N, 6)
        [xx xy xz yy yz zz], density (N,), albedo (N,): float32 contiguous torch tensors on this context's GPU
        (ValueError otherwise, before the library is touched). Records, boxes and the tree are computed on the
        device; nothing is copied to the host (scenes under 256 Gaussians and trees deeper than the stacks take
        the host path, see include/vr_hip.h). Returns the DeviceScene, which is the context's current scene and
        stands wherever a scene argument stands."""
        ds = DeviceScene(mean, cov6, density, albedo, lights, env_color)
        self.upload(ds, force=True)
        return ds

    def stats(self):
        s = L.vr_render_stats()
        check(lib().vr_get_stats(self._h, ctypes.byref(s)))
        return self._stats_dict(s)

    def _stats_dict(self, s):
        return {"kernel_ms": s.kernel_ms, "pixels": s.pixels, "fallback_pixels": s.fallback_pixels,
                "error_pixels": s.error_pixels, "stage_ms": dict(zip(self.STAGES, list(s.stage_ms))),
                "scatter_records": s.scatter_records, "secondary_rays": s.secondary_rays,
                "record_overflow": bool(s.record_overflow), "deep_pixels": s.deep_pixels,
                "slow_rays": s.slow_rays, "band_rays": s.band_rays,
                "filtered_rays": s.filtered_rays}

    def fallback_pixels(self):
        """(n, 2) int array of the (x, y) pixels of the last ray-march frame that were re-run on the
        large-capacity fallback path (vr_get_fallback_pixels)."""
        n = ctypes.c_size_t()
        check(lib().vr_get_fallback_pixels(self._h, None, 0, ctypes.byref(n)))
        xy = np.zeros((max(n.value, 1), 2), np.uint32)
        check(lib().vr_get_fallback_pixels(self._h, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n.value,
                                           ctypes.byref(n)))
        return xy[:n.value].astype(np.int32)

    def debug_pixel_records(self, x, y):
        """vr_debug_pixel_records: the scatter records of pixel (x, y) of the last ray-march frame, (n, 9 + S)
        rows (S = lights + env_samples, the row width the context reports): step k, position xyz,
        T * sigma_s, Li + Le rgb, active-list length, then each secondary ray's Tr (lights, then
        environment samples)."""
        n, row = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().vr_debug_pixel_records(self._h, int(x), int(y), None, 0, 0, ctypes.byref(n), ctypes.byref(row)))
        out = np.zeros((max(n.value, 1), row.value), np.float32)
        check(lib().vr_debug_pixel_records(self._h, int(x), int(y), fptr(out), n.value, row.value, ctypes.byref(n), None))
        return out[:n.value]

    def debug_tree(self, arrays=None):
        """vr_debug_tree: the uploaded Gaussian scene's trees as they lie on the device, a dict of numpy arrays
        (L.TREE_ARRAYS: order, records, the structured nodes / hnodes / hnodes4 / hnodes4s, the per-axis word
        copies hnodes4w / hnodes4t, parent4, prim_node4; an array the scene does not have is empty) plus
        "info", a dict of the vr_tree_info fields. `arrays` limits the read-back to the names given."""
        info = L.vr_tree_info()
        out = {}
        for name in (L.TREE_ARRAYS if arrays is None else arrays):
            sel, dt = L.TREE_ARRAYS[name]
            n, elem = ctypes.c_size_t(), ctypes.c_size_t()
            check(lib().vr_debug_tree(self._h, sel, None, 0, ctypes.byref(n), ctypes.byref(elem), ctypes.byref(info)))
            a = np.zeros(n.value, np.dtype(dt))
            if np.dtype(dt).itemsize != elem.value:
                raise ValueError(f"{name}: elements of {elem.value} bytes, the table has {np.dtype(dt).itemsize}")
            if n.value:
                check(lib().vr_debug_tree(self._h, sel, a.ctypes.data, n.value, ctypes.byref(n), None, None))
            out[name] = a
        if not out:
            n = ctypes.c_size_t()
            check(lib().vr_debug_tree(self._h, 0, None, 0, ctypes.byref(n), None, ctypes.byref(info)))
        d = {k: getattr(info, k) for k, _ in L.vr_tree_info._fields_}
        for k in ("hn_center", "bounds_min", "bounds_max"):
            d[k] = np.array(list(d[k]), np.float32)
        d["hn_scale"] = np.float32(d["hn_scale"])
        for k in ("built_on_device", "wrec_pd"):
            d[k] = bool(d[k])
        out["info"] = d
        return out

    OPTIONS = {"half_nodes": L.VR_OPT_HALF_NODES, "secondary_budget": L.VR_OPT_SECONDARY_BUDGET,
               "ff_window0": L.VR_OPT_FF_WINDOW0, "record_capacity": L.VR_OPT_RECORD_CAPACITY,
               "device_bvh": L.VR_OPT_DEVICE_BVH, "ff_nee_queue": L.VR_OPT_FF_NEE_QUEUE,
               "march_binned": L.VR_OPT_MARCH_BINNED, "ff_solver": L.VR_OPT_FF_SOLVER,
               "start_subtree": L.VR_OPT_START_SUBTREE, "ff_kernel": L.VR_OPT_FF_KERNEL,
               "sec_tight": L.VR_OPT_SEC_TIGHT, "march_wide_min": L.VR_OPT_MARCH_WIDE_MIN,
               "sec_filter": L.VR_OPT_SEC_FILTER}

    def set_option(self, name, value):
        """vr_set_option (include/vr_hip.h): explicit per-context tuning (half_nodes applies at the
        next upload, so the scene is re-uploaded)."""
        check(lib().vr_set_option(self._h, self.OPTIONS[name], int(value)))
        if name in ("half_nodes", "device_bvh", "sec_tight"):
            self._scene_key = None

    def get_option(self, name):
        v = ctypes.c_int64()
        check(lib().vr_get_option(self._h, self.OPTIONS[name], ctypes.byref(v)))
        return int(v.value)

    # vr_render_stats.stage_ms (include/vr_hip.h)
    STAGES = ("march", "sizing", "secondary", "accumulate")

    def synchronize(self):
        """Waits for the device; raises VRError(VR_ERR_OVERFLOW) if the last frame is invalid."""
        check(lib().vr_synchronize(self._h))

    def render_tiles_device(self, camera, params, width, height, first_tile, tile_stride, num_tiles, packed,
                            out_ptr, stream_ptr=0):
        check(lib().vr_render_tiles_device(self._h, ctypes.byref(camera.struct), ctypes.byref(params), width,
                                           height, first_tile, tile_stride, num_tiles, int(packed),
                                           ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream_ptr)))

    # Work counters of the instrumented build (include/vr_hip.h vr_count_work), per stage.
    WORK_NAMES = {
        "march": ("node_tests", "gaussian_tests", "optical_depths", "densities", "unused", "active_steps",
                  "primary_queries", "pixels"),
        # secondary stage = the persistent kernel's own schedule (+ the exact slow path)
        "secondary": ("node_tests", "gaussian_tests", "optical_depths", "list_tests", "secondary_rays",
                      "cut_rays", "cut_ray_node_steps", "repeat_depths"),
        # free-flight integrators: the path kernel and the shadow-ray (deferred NEE) kernel
        "path": ("paths", "bounces", "node4_steps", "node2_steps", "gaussian_tests", "erf_evals", "nee_inline",
                 "nee_queued"),
        "nee": ("rays", "node4_steps", "gaussian_tests", "optical_depths", "unused4", "unused5", "unused6", "unused7"),
    }

    def count_work(self, camera, params, width, height, first_tile=0, tile_stride=1, num_tiles=None):
        """Instrumented (untimed) render of the given tiles; returns the raw counts per stage."""
        if num_tiles is None:
            num_tiles = len(range(first_tile, num_tiles_of(width, height), tile_stride))
        arr = (ctypes.c_uint64 * 16)()
        check(lib().vr_count_work(self._h, ctypes.byref(camera.struct), ctypes.byref(params), width, height,
                                  first_tile, tile_stride, num_tiles, arr))
        stages = ("path", "nee") if params.integrator in (L.VR_FREE_FLIGHT, L.VR_MULTI_SCATTER) else ("march", "secondary")
        out = {stage: {k: int(arr[8 * s + i]) for i, k in enumerate(self.WORK_NAMES[stage])}
               for s, stage in enumerate(stages)}
        sec = out.get("secondary")
        if sec is not None:  # node steps of the rays that ran to the end of the tree
            sec["full_ray_node_steps"] = sec["node_tests"] - sec["cut_ray_node_steps"]
        return out

    def unshuffle_tiles_device(self, slabs_ptr, nslabs, tiles_per_slab, width, height, image_ptr, stream_ptr=0):
        check(lib().vr_unshuffle_tiles_device(self._h, ctypes.c_void_p(slabs_ptr), nslabs, tiles_per_slab, width,
                                              height, ctypes.c_void_p(image_ptr), ctypes.c_void_p(stream_ptr)))

    # ---- mixture queries (vr_query_*, include/vr_hip.h): gmm.h:517-578, :457-515, :98-126 in batch form ----
    # Arguments are numpy arrays (host entry points) or torch tensors on this context's GPU (the `_device`
    # entry points on torch's current stream, no host copy); results are of the same kind. The scene is
    # uploaded lazily, as Integrator._device does. Shapes and dtypes are checked before the library is called.

    def _first_gpu(self):
        return self.device[0] if isinstance(self.device, tuple) else self.device

    def _check_torch(self, *tensors):
        for t in tensors:
            if t.device.type != "cuda" or t.device.index != self._first_gpu():
                raise ValueError(f"tensor on {t.device}: this context queries cuda:{self._first_gpu()}")

    def _pack_rays_torch(self, o, d, tmax):
        import torch
        n = o.shape[0]
        o, d = o.contiguous(), d.contiguous()
        if _is_torch(tmax):
            tm, stride = tmax.contiguous(), 0 if tmax.numel() == 1 else 1
        else:
            tm, stride = torch.full((1,), float(tmax), dtype=torch.float32, device=o.device), 0
        rays = torch.empty((n, 8), dtype=torch.float32, device=o.device)
        stream = torch.cuda.current_stream(o.device).cuda_stream
        check(lib().vr_query_pack_rays_device(self._h, o.data_ptr(), d.data_ptr(), tm.data_ptr(), stride, n,
                                              rays.data_ptr(), stream))
        return rays, stream

    @staticmethod
    def _pack_rays_numpy(o, d, tmax):
        rays = np.zeros((o.shape[0], 8), np.float32)
        rays[:, 0:3] = o
        rays[:, 3] = tmax
        rays[:, 4:7] = d
        return rays

    def _check_kind(self, kind, *arrays):
        """The torch tensors among a query's arguments live on this context's device (checked after the upload)."""
        if kind.torch:
            self._check_torch(*(x for x in arrays if _is_torch(x)))

    def _query_rays(self, kind, origins, directions, tmax, unit=False, also=()):
        """The vr_ray rows of a query's checked ray arguments; `also`: its further arrays, for _check_kind."""
        self._check_kind(kind, origins, directions, tmax, *also)
        if kind.torch:
            rays, _ = self._pack_rays_torch(origins, directions, tmax)
        else:
            rays = self._pack_rays_numpy(origins, directions, tmax)
        if unit:
            rays[:, 7] = 1.0
        return rays

    def query_transmittance(self, scene, origins, directions, tmax=float("inf"), return_tau=False):
        """GaussianMixtureModel::transmittance_up_to (gmm.h:517-578) for n rays: origins, directions (n, 3)
        float32, tmax a scalar or (n,) float32 (it broadcasts). Returns Tr (n,), or (Tr, tau) with the
        optical depth itself (Tr == expf(-tau) bit for bit). Rays with a non-finite origin or a zero /
        non-finite direction give NaN."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, tmax))
        self.upload(scene)
        n = origins.shape[0]
        rays = self._query_rays(kind, origins, directions, tmax)
        tr = kind.new(n)
        tau = kind.new(n) if return_tau else None
        kind.call("vr_query_transmittance", self._h, kind.ptr(rays), n, kind.ptr(tr), kind.ptr(tau))
        return (tr, tau) if return_tau else tr

    def query_transmittance_grad(self, scene, origins, directions, weights=None, tmax=float("inf"), moving_bounds=True):
        """The gradient of the optical depth with respect to the Gaussians (vr_query_transmittance_grad): for the
        rays of query_transmittance and one weight per ray (None: all 1; a loss over Tr passes -Tr * dL/dTr), the
        (N, 10) float32 array sum_i weights[i] * d tau_i / d (mean[3], cov6 [xx xy xz yy yz zz], density) of scene
        Gaussian g, tau_i being query_transmittance's tau. An off-diagonal cov6 entry is the derivative with
        respect to the stored number (it stands at (i, j) and (j, i)). moving_bounds=False holds each Gaussian's
        3-sigma entry / exit distances fixed (VR_GRAD_FROZEN_BOUNDS). Invalid rays and rays with tmax <= 0
        contribute nothing. Sums are double atomics: reproducible to the rounding of a double sum, not bit for bit."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, tmax))
        n = origins.shape[0]
        if weights is not None:
            if _query_f32(weights, "weights", ()) != kind.torch:
                raise ValueError("weights must be of the same kind as origins")
            if weights.shape[0] != n:
                raise ValueError(f"weights has {weights.shape[0]} entries for {n} rays")
        self.upload(scene)
        N = scene.get_num_primitives()
        if N == 0:
            return kind.new((0, 10), zero=True)
        rays = self._query_rays(kind, origins, directions, tmax, also=(weights,))
        grad = kind.new((N, 10))
        kind.call("vr_query_transmittance_grad", self._h, kind.ptr(rays), kind.ptr(kind.contiguous(weights)), n,
                  0 if moving_bounds else L.VR_GRAD_FROZEN_BOUNDS, kind.ptr(grad))
        return grad

    def query_transmittance_ray_grad(self, scene, origins, directions, tmax=float("inf"), unit=False, moving_bounds=True):
        """The gradient of the optical depth with respect to the rays (vr_query_transmittance_ray_grad), and the
        optical depth: for the rays of query_transmittance, (d_origin (n, 3), d_direction (n, 3), d_tmax (n,),
        tau (n,)) float32, row i being d tau_i / d (origin, direction, tmax) of ray i and tau_i query_transmittance's
        tau bit for bit. unit=False: the library normalises the directions and d_direction holds the chain through
        v / |v| (it is orthogonal to the direction); unit=True: the directions are unit vectors already, are used as
        they stand, and d_direction is the derivative with respect to the three components taken as free.
        d_tmax is the integrand at tmax where tmax cuts a Gaussian short, else 0 (always 0 for tmax = inf).
        moving_bounds=False holds each Gaussian's 3-sigma entry / exit distances fixed (VR_GRAD_FROZEN_BOUNDS).
        Invalid rays give NaN in every output, rays with tmax <= 0 or NaN zeros. Sums are per ray, in double, with
        no atomics. Inputs are numpy arrays or torch tensors on this context's device, never a mix."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, tmax))
        self.upload(scene)
        n = origins.shape[0]
        rays = self._query_rays(kind, origins, directions, tmax, unit)
        out = kind.new((n, 8))
        kind.call("vr_query_transmittance_ray_grad", self._h, kind.ptr(rays), n, 0 if moving_bounds else L.VR_GRAD_FROZEN_BOUNDS,
                  kind.ptr(out))
        return out[:, 0:3], out[:, 4:7], out[:, 3], out[:, 7]

    def query_transmittance_profile(self, scene, origins, directions, t, return_tau=False):
        """Transmittance at K distances along each of n rays from one tree walk per ray
        (vr_query_transmittance_profile): origins, directions (n, 3) float32; t float32 of shape (K,), one row of
        distances shared by all rays, or (n, K), of the same kind (numpy or torch) as the rays. Returns Tr (n, K), or
        (Tr, tau). Column k has the bits of query_transmittance(..., tmax=t[:, k], return_tau=True). Samples may come
        in any order; a sample <= 0 or NaN gives tau = 0, Tr = 1, an invalid ray NaN in its whole row."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, 0.0))
        n = origins.shape[0]
        K, stride = _query_profile_args(t, "t", n, kind.torch, shared_ok=True)
        self.upload(scene)
        rays = self._query_rays(kind, origins, directions, float("inf"), also=(t,))
        tr = kind.new((n, K))
        tau = kind.new((n, K)) if return_tau else None
        kind.call("vr_query_transmittance_profile", self._h, kind.ptr(rays), kind.ptr(kind.contiguous(t)), stride, n, K,
                  kind.ptr(tr), kind.ptr(tau))
        return (tr, tau) if return_tau else tr

    def query_transmittance_profile_grad(self, scene, origins, directions, t, weights=None, moving_bounds=True):
        """The gradient of a weighted sum of a profile's optical depths with respect to the Gaussians
        (vr_query_transmittance_profile_grad): for the rays and distances of query_transmittance_profile and weights
        (n, K) float32 (None: all 1), the (N, 10) float32 array sum_i sum_k weights[i, k] * d tau[i, k] / d (mean[3],
        cov6, density), in query_transmittance_grad's layout and with its moving_bounds. One walk per ray and ten
        atomic adds per (ray, Gaussian) hit whatever K is; equal to query_transmittance_grad on the n * K expanded rays
        up to the rounding of double sums."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, 0.0))
        n = origins.shape[0]
        K, stride = _query_profile_args(t, "t", n, kind.torch, shared_ok=True)
        if weights is not None and _query_profile_args(weights, "weights", n, kind.torch, shared_ok=False)[0] != K:
            raise ValueError(f"weights has {weights.shape[1]} columns for {K} samples")
        self.upload(scene)
        N = scene.get_num_primitives()
        if N == 0:
            return kind.new((0, 10), zero=True)
        rays = self._query_rays(kind, origins, directions, float("inf"), also=(t, weights))
        grad = kind.new((N, 10))
        kind.call("vr_query_transmittance_profile_grad", self._h, kind.ptr(rays), kind.ptr(kind.contiguous(t)), stride,
                  kind.ptr(kind.contiguous(weights)), n, K, 0 if moving_bounds else L.VR_GRAD_FROZEN_BOUNDS, kind.ptr(grad))
        return grad

    def query_sigma(self, scene, points, return_active=False):
        """GaussianMixtureModel::evaluate_sigma (gmm.h:98-126) at n points (n, 3) float32, over the Gaussians
        whose 3-sigma ellipsoid holds the point. Returns sigma (n, 2) = (sigma_a, sigma_s), or (sigma,
        n_active) with the size of that set per point."""
        kind = _ArrayKind(points, _query_point_args(points))
        self.upload(scene)
        n = points.shape[0]
        self._check_kind(kind, points)
        sig = kind.new((n, 2))
        act = kind.new(n, np.int32) if return_active else None  # (the library's uint32 counts)
        kind.call("vr_query_sigma", self._h, kind.ptr(kind.contiguous(points)), n, kind.ptr(sig), kind.ptr(act))
        return (sig, act) if return_active else sig

    def query_sigma_grad(self, scene, points, weights=None, gaussians=True, positions=False):
        """The gradient of query_sigma's sigma (vr_query_sigma_grad) at n points (n, 3) float32. weights (n, 2) float32
        = (dL/d sigma_a, dL/d sigma_s) per point; None: (1, 1) everywhere, the gradient of sigma_t, whose albedo
        column is exactly 0. gaussians=True: the (N, 11) float32 array sum_i w_i . d sigma(x_i) / d (mean[3], cov6 [xx xy
        xz yy yz zz], density, albedo) of scene Gaussian g (an off-diagonal cov6 entry is the derivative with respect
        to the stored number). positions=True: the (n, 3) array whose row i is w_i . d sigma(x_i) / d x_i. Returns the
        one asked for, or (gaussians, positions) for both; positions alone runs without a single atomic add. The active
        set is query_sigma's bit for bit; a point in no ellipsoid, or with a non-finite coordinate, contributes nothing
        and gets a zero row. The per-Gaussian sums are double atomics: reproducible to the rounding of a double sum."""
        kind = _ArrayKind(points, _query_point_args(points))
        n = points.shape[0]
        if not (gaussians or positions):
            raise ValueError("query_sigma_grad: ask for gaussians, positions or both")
        if weights is not None:
            if _query_f32(weights, "weights", (2,)) != kind.torch:
                raise ValueError("weights must be of the same kind as points")
            if weights.shape[0] != n:
                raise ValueError(f"weights has {weights.shape[0]} rows for {n} points")
        self.upload(scene)
        N = scene.get_num_primitives()
        self._check_kind(kind, points, weights)
        grad = kind.new((N, 11), zero=True) if gaussians else None
        gx = kind.new((n, 3), zero=True) if positions else None
        if n > 0 and (N > 0 or positions):
            kind.call("vr_query_sigma_grad", self._h, kind.ptr(kind.contiguous(points)), kind.ptr(kind.contiguous(weights)), n,
                      kind.ptr(grad) if N > 0 else None, kind.ptr(gx))
        return (grad, gx) if gaussians and positions else grad if gaussians else gx

    def evaluate_features(self, scene, points, features, return_mass=False, return_active=False):
        """The caller's per-Gaussian vectors at n points (vr_query_features): points (n, 3) float32, features (N, C)
        float32 of the same kind (numpy or torch), row g for scene Gaussian g, 1 <= C <= VR_FEATURES_MAX_CHANNELS.
        Returns F (n, C) with F[i, c] = sum_g m_g(x_i) features[g, c] over query_sigma's active set (m: its f32 mu_t; the
        sum in double, rounded once), or (F, mass), (F, n_active), (F, mass, n_active) with mass (n,) = sum_g m_g(x_i)
        and the size of the set. A channel of ones has the bits of mass; F / mass is the mass-weighted mean of the
        features at the point. A channel's bits do not depend on C or on its place among the channels."""
        kind = _ArrayKind(points, _query_point_args(points))
        C = _query_feature_args(features, "features", None, kind.torch, "Gaussians")
        n = points.shape[0]
        _query_feature_sizes(n, features.shape[0], C)
        N = scene.get_num_primitives()
        if features.shape[0] != N:
            raise ValueError(f"features has {features.shape[0]} rows for {N} Gaussians")
        self.upload(scene)
        self._check_kind(kind, points, features)
        run = n > 0 and N > 0  # (otherwise every result is zero and nothing is launched)
        out = kind.new((n, C), zero=not run)
        mass = kind.new(n, zero=not run) if return_mass else None
        act = kind.new(n, np.int32, zero=not run) if return_active else None  # (the library's uint32 counts)
        if run:
            kind.call("vr_query_features", self._h, kind.ptr(kind.contiguous(points)), n, kind.ptr(kind.contiguous(features)), C,
                      kind.ptr(out), kind.ptr(mass), kind.ptr(act))
        got = (out,) + ((mass,) if return_mass else ()) + ((act,) if return_active else ())
        return got if len(got) > 1 else out

    def features_gradient(self, scene, points, features, weights=None, weight_mass=None, gaussians=True, features_grad=True,
                            positions=False):
        """The gradient of L = sum_i (sum_c weights[i, c] F[i, c] + weight_mass[i] mass[i]) for evaluate_features' F and mass
        (vr_query_features_grad). weights (n, C) float32 or None (1 everywhere), weight_mass (n,) float32 or None (0).
        gaussians=True: the (N, 10) array d L / d (mean[3], cov6 [xx xy xz yy yz zz], density) of scene Gaussian g, in
        query_transmittance_grad's layout; features_grad=True: the (N, C) array d L / d features; positions=True: the
        (n, 3) array d L / d points. Returns the one asked for, or a tuple of those asked for in that order. Only what
        is asked for is computed: positions alone runs without a single atomic add. The active set is query_sigma's bit
        for bit and is not differentiated; a point in no ellipsoid, or with a non-finite coordinate, contributes nothing
        and gets a zero row. The per-Gaussian sums are double atomics: reproducible to the rounding of a double sum."""
        kind = _ArrayKind(points, _query_point_args(points))
        n = points.shape[0]
        C = _query_feature_args(features, "features", None, kind.torch, "Gaussians")
        if not (gaussians or features_grad or positions):
            raise ValueError("features_gradient: ask for gaussians, features_grad, positions or any of them together")
        if weights is not None and _query_feature_args(weights, "weights", n, kind.torch, "points") != C:
            raise ValueError(f"weights has {weights.shape[1]} columns for {C} channels")
        if weight_mass is not None:
            if _query_f32(weight_mass, "weight_mass", ()) != kind.torch:
                raise ValueError("weight_mass must be of the same kind as points")
            if weight_mass.shape[0] != n:
                raise ValueError(f"weight_mass has {weight_mass.shape[0]} entries for {n} points")
        _query_feature_sizes(n, features.shape[0], C)
        N = scene.get_num_primitives()
        if features.shape[0] != N:
            raise ValueError(f"features has {features.shape[0]} rows for {N} Gaussians")
        self.upload(scene)
        self._check_kind(kind, points, features, weights, weight_mass)
        run = n > 0 and N > 0  # (otherwise every result is zero and nothing is launched)
        grad = kind.new((N, 10), zero=not run) if gaussians else None
        gf = kind.new((N, C), zero=not run) if features_grad else None
        gx = kind.new((n, 3), zero=not run) if positions else None
        if run:
            kind.call("vr_query_features_grad", self._h, kind.ptr(kind.contiguous(points)), n, kind.ptr(kind.contiguous(features)),
                      C, kind.ptr(kind.contiguous(weights)), kind.ptr(kind.contiguous(weight_mass)), kind.ptr(grad), kind.ptr(gf),
                      kind.ptr(gx))
        got = tuple(a for a in (grad, gf, gx) if a is not None)
        return got if len(got) > 1 else got[0]

    def radiance(self, scene, origins, directions, t, features, weights=None, unit=False, return_opacity=False, return_tr=False,
                 return_pairs=False):
        """The emission-absorption sum along n rays in one call (vr_query_radiance): origins, directions (n, 3) float32; t
        float32 of shape (K,) (one row shared by all rays) or (n, K), the samples of query_transmittance_profile; features
        (N, C) float32, row g for scene Gaussian g, as for evaluate_features; weights the quadrature weights in t's two
        shapes, or None (all ones). All arrays are of one kind, numpy or torch. Returns L (n, C) with
            L[i, c] = sum_k weights[i, k] Tr[i, k] sum_g m_g(x_ik) features[g, c],   x_ik = origins[i] + t[i, k] * d_i
        (the f32 product and sum numpy computes; d_i the normalised direction, or directions[i] as it stands with
        unit=True), over query_sigma's active set at x_ik, with Tr the profile's; sums in double, rounded once. Further
        results follow in this order when asked for: opacity (n,), the same sum without the features; Tr (n, K), the bits of
        query_transmittance_profile; pairs (n,) int32, the active (sample, Gaussian) pairs of the ray. A sample that is
        negative, NaN or infinite contributes nothing. A channel of ones has the bits of opacity; a channel's bits do not
        depend on C or on its place. Unlike evaluate_features, a point whose summed m is <= 0 is not zeroed (this
        differs with non-positive densities only)."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, 0.0))
        n = origins.shape[0]
        K, stride = _query_profile_args(t, "t", n, kind.torch, shared_ok=True)
        C = _query_feature_args(features, "features", None, kind.torch, "Gaussians")
        q_stride = 0
        if weights is not None:
            Kq, q_stride = _query_profile_args(weights, "weights", n, kind.torch, shared_ok=True)
            if Kq != K:
                raise ValueError(f"weights has {Kq} columns for {K} samples")
        _query_feature_sizes(n, features.shape[0], C)
        N = scene.get_num_primitives()
        if features.shape[0] != N:
            raise ValueError(f"features has {features.shape[0]} rows for {N} Gaussians")
        self.upload(scene)
        rays = self._query_rays(kind, origins, directions, float("inf"), unit, also=(t, features, weights))
        out = kind.new((n, C))
        opacity = kind.new(n) if return_opacity else None
        tr = kind.new((n, K)) if return_tr else None
        pairs = kind.new(n, np.int32) if return_pairs else None  # (the library's uint32 counts)
        if n > 0:
            feats = kind.contiguous(features) if N > 0 else kind.new((1, C), zero=True)  # (no rows: never read, never NULL)
            kind.call("vr_query_radiance", self._h, kind.ptr(rays), kind.ptr(kind.contiguous(t)), stride,
                      kind.ptr(kind.contiguous(weights)), q_stride, n, K, kind.ptr(feats), C, kind.ptr(out), kind.ptr(opacity),
                      kind.ptr(tr), kind.ptr(pairs))
        got = (out,) + tuple(a for a in (opacity, tr, pairs) if a is not None)
        return got if len(got) > 1 else out

    def radiance_gradient(self, scene, origins, directions, t, features, weights=None, weight_opacity=None, q=None, tr=None,
                          unit=False, moving_bounds=True, gaussians=True, features_grad=True, grad_q=False, grad_tau=False):
        """The gradient of l = sum_i (sum_c weights[i, c] L[i, c] + weight_opacity[i] opacity[i]) for radiance's L and opacity,
        in one fused call (vr_query_radiance_grad). origins, directions, t, features and unit are radiance's; q holds the
        quadrature weights (radiance's `weights`) in t's two shapes, or None (ones); weights (n, C) float32 is dl/dL (None:
        ones), weight_opacity (n,) float32 dl/dopacity (None: zeros); tr (n, K) float32 is the Tr radiance returned (None:
        it is computed again, with the same bits in every result). All arrays are of one kind, numpy or torch.
        gaussians=True: the (N, 10) array d l / d (mean[3], cov6 [xx xy xz yy yz zz], density) of scene Gaussian g, in
        query_transmittance_grad's layout and with its moving_bounds, the emission part and the part through the
        transmittances together; features_grad=True: the (N, C) array d l / d features; grad_q=True: the (n, K) array
        d l / d q (meaningful for q=None too); grad_tau=True: the (n, K) array d l / d tau, tau the optical depth up to each
        sample. Returns the one asked for, or a tuple of those asked for in that order. Only what is asked for is computed:
        grad_q and grad_tau alone run without a single atomic add. The sample points, their validity and the active set
        are radiance's bit for bit and are not differentiated; an invalid ray contributes nothing and gets NaN rows in
        grad_q and grad_tau, an invalid sample +0. The per-Gaussian sums are double atomics: reproducible to the rounding
        of a double sum; grad_q and grad_tau are reproducible bit for bit."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, 0.0))
        n = origins.shape[0]
        K, stride = _query_profile_args(t, "t", n, kind.torch, shared_ok=True)
        C = _query_feature_args(features, "features", None, kind.torch, "Gaussians")
        if not (gaussians or features_grad or grad_q or grad_tau):
            raise ValueError("radiance_gradient: ask for gaussians, features_grad, grad_q, grad_tau or any of them together")
        q_stride = 0
        if q is not None:
            Kq, q_stride = _query_profile_args(q, "q", n, kind.torch, shared_ok=True)
            if Kq != K:
                raise ValueError(f"q has {Kq} columns for {K} samples")
        if tr is not None and _query_profile_args(tr, "tr", n, kind.torch, shared_ok=False)[0] != K:
            raise ValueError(f"tr has {tr.shape[1]} columns for {K} samples")
        if weights is not None and _query_feature_args(weights, "weights", n, kind.torch, "rays") != C:
            raise ValueError(f"weights has {weights.shape[1]} columns for {C} channels")
        if weight_opacity is not None:
            if _query_f32(weight_opacity, "weight_opacity", ()) != kind.torch:
                raise ValueError("weight_opacity must be of the same kind as origins")
            if weight_opacity.shape[0] != n:
                raise ValueError(f"weight_opacity has {weight_opacity.shape[0]} entries for {n} rays")
        _query_feature_sizes(n, features.shape[0], C)
        N = scene.get_num_primitives()
        if features.shape[0] != N:
            raise ValueError(f"features has {features.shape[0]} rows for {N} Gaussians")
        self.upload(scene)
        rays = self._query_rays(kind, origins, directions, float("inf"), unit, also=(t, features, weights, weight_opacity, q, tr))
        run = n > 0 and N > 0  # (otherwise the Gaussians' results are zero)
        grad = kind.new((N, 10), zero=not run) if gaussians else None
        gf = kind.new((N, C), zero=not run) if features_grad else None
        gq = kind.new((n, K)) if grad_q else None
        gt = kind.new((n, K)) if grad_tau else None
        if n > 0 and (N > 0 or grad_q or grad_tau):
            feats = kind.contiguous(features) if N > 0 else kind.new((1, C), zero=True)  # (no rows: never read, never NULL)
            kind.call("vr_query_radiance_grad", self._h, kind.ptr(rays), kind.ptr(kind.contiguous(t)), stride,
                      kind.ptr(kind.contiguous(q)), q_stride, n, K, kind.ptr(feats), C, kind.ptr(kind.contiguous(weights)),
                      kind.ptr(kind.contiguous(weight_opacity)), kind.ptr(kind.contiguous(tr)),
                      0 if moving_bounds else L.VR_GRAD_FROZEN_BOUNDS, kind.ptr(grad) if N > 0 else None,
                      kind.ptr(gf) if N > 0 else None, kind.ptr(gq), kind.ptr(gt))
        got = tuple(a for a in (grad, gf, gq, gt) if a is not None)
        return got if len(got) > 1 else got[0]

    def query_events(self, scene, origins, directions):
        """GaussianMixtureModel::intersect_events (gmm.h:457-515) for n rays. Returns (offsets, t, gaussian,
        entering): ray i's events are the slice offsets[i]:offsets[i + 1] (offsets: (n + 1,) int64) of t
        (float32, non-decreasing per ray), gaussian (int32 scene index) and entering (bool). Events of a ray with
        equal t come in scene order, entry before exit: deterministic, but not the tie order of the
        reference's std::sort."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, 0.0))
        self.upload(scene)
        n = origins.shape[0]
        total = ctypes.c_uint64()
        rays = self._query_rays(kind, origins, directions, 0.0)
        off = kind.new(n + 1, np.int32, zero=True)  # (the library's uint32 words)
        if kind.torch:  # the device form: a count call, which synchronises, then a fill call on torch's stream
            import torch
            check(lib().vr_query_events_count_device(self._h, kind.ptr(rays), n, kind.ptr(off), ctypes.byref(total)))
            t, ev = kind.new(total.value), kind.new(total.value, np.int32)
            kind.call("vr_query_events_fill", self._h, kind.ptr(rays), n, kind.ptr(off), kind.ptr(t), kind.ptr(ev), total.value)
            return off.to(torch.int64) & 0xffffffff, t, ev >> 1, (ev & 1).to(torch.bool)
        # the host form: one call without room for the events and, if there are any, the same call with room
        kind.call("vr_query_events", self._h, kind.ptr(rays), n, kind.ptr(off), None, None, 0, ctypes.byref(total))
        t, ev = kind.new(total.value), kind.new(total.value, np.uint32)
        if total.value:
            kind.call("vr_query_events", self._h, kind.ptr(rays), n, kind.ptr(off), kind.ptr(t), kind.ptr(ev), total.value,
                      ctypes.byref(total))
        return off.view(np.uint32).astype(np.int64), t, (ev >> 1).astype(np.int32), (ev & 1).astype(bool)

    def query_free_flight(self, scene, origins, directions, tau, unit=False, return_albedo=False, return_active=False):
        """One free-flight step per ray, MultiScatterGaussians::get_free_flight_distance (integrator.h:422-498):
        origins, directions (n, 3) float32, tau the target optical depth (-log(1 - xi), drawn by the caller), a
        scalar or (n,) float32 (it broadcasts). unit=True: the directions are of unit length already (a Ray
        object's) and are used as they stand. Returns t (n,): the collision distance, or -1 where the ray leaves
        the mixture first; then, if asked for, the albedo at the collision (gmm.h:128-143; 0 where t < 0) and the
        number of Gaussians active there (int32). Invalid rays and NaN targets give NaN. With query_transmittance
        (next-event estimation) and query_sigma this is a volumetric path tracer's kit."""
        kind = _ArrayKind(origins, _query_ray_args(origins, directions, tau))
        self.upload(scene)
        n = origins.shape[0]
        rays = self._query_rays(kind, origins, directions, 0.0, unit, also=(tau,))
        if not kind.torch:
            tg = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, np.float32).reshape(-1), (n,)))
        elif _is_torch(tau):
            tg = tau.reshape(-1).expand(n).contiguous()
        else:
            tg = kind.new(n).fill_(float(tau))
        t = kind.new(n)
        alb = kind.new(n) if return_albedo else None
        act = kind.new(n, np.int32) if return_active else None  # (the library's uint32 counts)
        kind.call("vr_query_free_flight", self._h, kind.ptr(rays), kind.ptr(tg), n, kind.ptr(t), kind.ptr(alb), kind.ptr(act))
        out = (t,) + ((alb,) if return_albedo else ()) + ((act,) if return_active else ())
        return out if len(out) > 1 else t

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and L is not None and L._lib is not None:  # (L is None during interpreter teardown)
            L._lib.vr_destroy(h)
            self._h = None


class DeviceScene:
    """A Gaussian scene whose parameters live in torch tensors on the GPU (Device.upload_gaussians). It stands
    wherever a `scene` argument stands: a context uploads it from the held tensors (vr_upload_gaussians_device)
    when another scene displaced it, and not at all while it is the context's current scene. The tensors are
    held detached, not copied: after changing them in place (an optimiser step), call refresh()."""

    GAUSSIANS = L.VR_VOLUME_GAUSSIANS
    volume_type = L.VR_VOLUME_GAUSSIANS
    _h = None  # no host vr_scene stands behind it

    def __init__(self, mean, cov6, density, albedo, lights=(), env_color=None):
        args = ((mean, "mean", (3,)), (cov6, "cov6", (6,)), (density, "density", ()), (albedo, "albedo", ()))
        for x, name, tail in args:
            if not _query_f32(x, name, tail):
                raise ValueError(f"{name} must be a torch tensor on the context's GPU, not a numpy array")
        for x, name, _ in args:
            if x.shape[0] != mean.shape[0]:
                raise ValueError(f"{name} has {x.shape[0]} rows for {mean.shape[0]} means")
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        for x, name, _ in args:
            if x.device.type != "cuda" or x.device != mean.device:
                raise ValueError(f"{name} is on {x.device}: upload_gaussians takes tensors on the context's GPU")
        self.mean, self.cov6, self.density, self.albedo = (x.detach() for x in (mean, cov6, density, albedo))
        self.lights = [Light(l.position, l.intensity) for l in lights]
        self.env_color = _v3([0.53, 0.81, 0.92] if env_color is None else env_color)  # (scene.h:29's default)
        self.version = 0

    def get_num_primitives(self):
        return int(self.mean.shape[0])

    def refresh(self):
        """The tensors changed in place: the next use uploads them again."""
        self.version += 1

    def _upload_to(self, dev):
        dev._check_torch(self.mean)
        n = len(self.lights)
        arr = (L.vr_light * max(n, 1))()
        for i, l in enumerate(self.lights):
            arr[i].position[:] = [float(v) for v in l.position]
            arr[i].intensity[:] = [float(v) for v in l.intensity]
        env = fptr(self.env_color)
        check(lib().vr_upload_gaussians_device(dev._h, self.mean.data_ptr(), self.cov6.data_ptr(), self.density.data_ptr(),
                                               self.albedo.data_ptr(), self.get_num_primitives(), arr, n, env))


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


class _ArrayKind:
    """The kind of a query's arrays, and what a query method needs of it: numpy arrays, which go to the host entry
    point, or torch tensors on the context's device, which go to its `_device` form on torch's current stream."""

    def __init__(self, like, torch_in):
        self.torch, self.device = torch_in, like.device if torch_in else None

    def new(self, shape, dtype=np.float32, zero=False):
        if not self.torch:
            return (np.zeros if zero else np.empty)(shape, dtype)
        import torch
        return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)

    def contiguous(self, x):
        return None if x is None else x.contiguous() if self.torch else np.ascontiguousarray(x)

    def ptr(self, x):
        if x is None:
            return None
        return x.data_ptr() if self.torch else x.ctypes.data_as(L.FP if x.dtype == np.float32 else L.U32P)

    def call(self, name, *args):
        if not self.torch:
            return check(getattr(lib(), name)(*args))
        import torch
        check(getattr(lib(), name + "_device")(*args, torch.cuda.current_stream(self.device).cuda_stream))


def _query_f32(x, name, shape_tail):
    """x is an (n,) + shape_tail float32 numpy array or torch tensor (ValueError otherwise); True for torch."""
    if _is_torch(x):
        import torch
        ok_dtype = x.dtype == torch.float32
    elif isinstance(x, np.ndarray):
        ok_dtype = x.dtype == np.float32
    else:
        raise ValueError(f"{name} must be a numpy array or a torch tensor, not {type(x).__name__}")
    if not ok_dtype:
        raise ValueError(f"{name} must be float32, not {x.dtype}")
    if len(x.shape) != 1 + len(shape_tail) or tuple(x.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name} must have shape (n{''.join(', %d' % k for k in shape_tail)}), not {tuple(x.shape)}")
    return _is_torch(x)


def _query_ray_args(origins, directions, tmax):
    """Checks the ray arguments of a query before anything reaches the library; True for torch input."""
    t_o = _query_f32(origins, "origins", (3,))
    t_d = _query_f32(directions, "directions", (3,))
    if t_o != t_d:
        raise ValueError("origins and directions must both be numpy arrays or both torch tensors")
    if origins.shape[0] != directions.shape[0]:
        raise ValueError(f"{origins.shape[0]} origins but {directions.shape[0]} directions")
    if _is_torch(tmax) or isinstance(tmax, np.ndarray):
        if len(tmax.shape) == 0:
            tmax = tmax.reshape(1)
        if _query_f32(tmax, "tmax", ()) != t_o:
            raise ValueError("tmax must be a scalar or of the same kind as origins")
        if tmax.shape[0] not in (1, origins.shape[0]):
            raise ValueError(f"tmax has {tmax.shape[0]} entries for {origins.shape[0]} rays")
    else:
        try:
            float(tmax)
        except (TypeError, ValueError):
            raise ValueError(f"tmax must be a number or a float32 array, not {type(tmax).__name__}") from None
    return t_o


def _query_profile_args(x, name, n, torch_in, shared_ok):
    """Checks a profile's samples or weights before anything reaches the library: float32, (n, K), or (K,) where one row
    may be shared, 1 <= K <= VR_PROFILE_MAX_SAMPLES, of the rays' kind. Returns (K, the row stride: K or 0)."""
    shape = tuple(getattr(x, "shape", ()))
    shared = shared_ok and len(shape) == 1
    if not shared and len(shape) != 2:
        raise ValueError(f"{name} must have shape {'(K,) or ' if shared_ok else ''}(n, K), not {shape}")
    K = shape[-1]
    if _query_f32(x, name, () if shared else (K,)) != torch_in:
        raise ValueError(f"{name} must be of the same kind as origins")
    if not shared and shape[0] != n:
        raise ValueError(f"{name} has {shape[0]} rows for {n} rays")
    if not 1 <= K <= L.VR_PROFILE_MAX_SAMPLES:
        raise ValueError(f"{name} has {K} samples per ray: 1 to {L.VR_PROFILE_MAX_SAMPLES} are allowed")
    if n * K >= 2 ** 31:
        raise ValueError(f"{n} rays of {K} samples: more than 2^31 - 1 samples in one call")
    return K, 0 if shared else K


def _query_point_args(points):
    return _query_f32(points, "points", (3,))


def _query_feature_args(x, name, rows, torch_in, of):
    """Checks a feature query's rows or weights before anything reaches the library: float32, (rows, C) with
    1 <= C <= VR_FEATURES_MAX_CHANNELS (rows None: any number), of the points' kind. Returns C."""
    shape = tuple(getattr(x, "shape", ()))
    if len(shape) != 2:
        raise ValueError(f"{name} must have shape ({'N' if rows is None else rows}, C), not {shape}")
    C = shape[1]
    if not 1 <= C <= L.VR_FEATURES_MAX_CHANNELS:
        raise ValueError(f"{name} has {C} channels: 1 to {L.VR_FEATURES_MAX_CHANNELS} are allowed")
    if _query_f32(x, name, (C,)) != torch_in:
        raise ValueError(f"{name} must be of the same kind as points")
    if rows is not None and shape[0] != rows:
        raise ValueError(f"{name} has {shape[0]} rows for {rows} {of}")
    return C


def _query_feature_sizes(n, N, C):
    if n * C >= 2 ** 31 or N * C >= 2 ** 31:
        raise ValueError(f"{n} points and {N} Gaussians of {C} channels: more than 2^31 - 1 entries in one call")


# ---- ray grids (vr_render_rays, include/vr_hip.h): Integrator.render_rays ----
RAY_BATCH_WIDTH = 256  # a flat (n, 3) batch is rendered as a grid of this width: ray i sits at (i % 256, i // 256)
_MAX_GRID_EDGE = 65535  # vr_render_rays: width and height lie in [1, 65535]


def _ray_grid_layout(origins, directions):
    """Checks the ray arguments of render_rays before anything reaches the library. Returns (torch input?,
    grid width, grid height, number of rays, leading shape of the results): an (H, W, 3) pair is a W x H grid; an
    (n, 3) pair a flat batch laid out RAY_BATCH_WIDTH wide and ceil(n / RAY_BATCH_WIDTH) high, whose last row
    is padded. ValueError otherwise."""
    kinds = []
    for x, name in ((origins, "origins"), (directions, "directions")):
        if _is_torch(x):
            import torch
            ok_dtype = x.dtype == torch.float32
        elif isinstance(x, np.ndarray):
            ok_dtype = x.dtype == np.float32
        else:
            raise ValueError(f"{name} must be a numpy array or a torch tensor, not {type(x).__name__}")
        if not ok_dtype:
            raise ValueError(f"{name} must be float32, not {x.dtype}")
        if len(x.shape) not in (2, 3) or x.shape[-1] != 3:
            raise ValueError(f"{name} must have shape (H, W, 3) or (n, 3), not {tuple(x.shape)}")
        kinds.append(_is_torch(x))
    if kinds[0] != kinds[1]:
        raise ValueError("origins and directions must both be numpy arrays or both torch tensors")
    if tuple(origins.shape) != tuple(directions.shape):
        raise ValueError(f"origins have shape {tuple(origins.shape)} but directions {tuple(directions.shape)}")
    lead = tuple(int(k) for k in origins.shape[:-1])
    if len(lead) == 2:
        H, W = lead
        n = W * H
    else:
        n = lead[0]
        if n > RAY_BATCH_WIDTH * _MAX_GRID_EDGE:
            raise ValueError(f"{n} rays in one flat batch: at most {RAY_BATCH_WIDTH * _MAX_GRID_EDGE} (split it)")
        W, H = RAY_BATCH_WIDTH, -(-n // RAY_BATCH_WIDTH)
    if not (1 <= W <= _MAX_GRID_EDGE and 1 <= H <= _MAX_GRID_EDGE):
        raise ValueError(f"a ray grid's width and height must be in [1, {_MAX_GRID_EDGE}], not {W} x {H}")
    return kinds[0], W, H, n, lead


def _pack_ray_grid_numpy(origins, directions, unit, W, H, n):
    """The W x H vr_ray rows of n rays (W * H >= n): origin, tmax (unread), direction, unit. Rows past the
    n-th, the pad of a flat batch's last grid row, have a zero direction (invalid: NaN results, dropped)."""
    rays = np.zeros((W * H, 8), np.float32)
    rays[:n, 0:3] = origins.reshape(n, 3)
    rays[:n, 4:7] = directions.reshape(n, 3)
    rays[:n, 7] = 1.0 if unit else 0.0
    return rays


def num_tiles(width, height):
    return int(lib().vr_num_tiles(width, height))


num_tiles_of = num_tiles


class Integrator:
    """integrator.h:49-57: Integrator(camera); render(scene, image) fills `image` in place."""

    integrator_id = None

    def __init__(self, camera, step_size=0.01, env_samples=20, t_eps=0.0, device=0):
        self.camera = camera
        self.params = L.vr_render_params()
        self.params.integrator = self.integrator_id
        self.params.step_size = float(step_size)
        self.params.env_samples = int(env_samples)
        self.params.t_eps = float(t_eps)
        self.params.flags = 0
        self.device = device
        self.last_stats = None

    solver = None  # free-flight integrators: a SOLVERS key (VR_OPT_FF_SOLVER), set on the device per render

    def _device(self, scene):
        dev = Device.get(self.device)
        dev.upload(scene)
        if self.solver is not None:
            dev.set_option("ff_solver", SOLVERS[self.solver])
        return dev

    def render(self, scene, image):
        dev = self._device(scene)
        W, H = image.get_width(), image.get_height()
        out = np.empty((H, W, 3), np.float32)
        check(lib().vr_render(dev._h, ctypes.byref(self.camera.struct), ctypes.byref(self.params), W, H, fptr(out)))
        image.pixels[...] = out
        self.last_stats = dev.stats()
        return image

    def render_rays(self, scene, origins, directions, unit=False, return_transmittance=False):
        """Radiance along the caller's own rays (vr_render_rays, include/vr_hip.h): the ray-march integrators
        render a grid of rays exactly as they render a frame, pixel (x, y) marching its own ray in place of the
        camera's (the integrator's camera is not read). origins, directions: float32, (H, W, 3) for a W x H grid
        or (n, 3) for a flat batch (laid out RAY_BATCH_WIDTH wide; the environment samples of ray i are keyed by
        its grid position (i % 256, i // 256)). unit: the directions are normalised already and are used as
        they stand (a Ray object's; otherwise they get the Ray constructor's one normalisation).
        numpy arrays go through the host entry point; torch tensors on this integrator's GPU through the device
        one on torch's current stream, with no host copy (the call waits for that stream). Returns rgb with
        the inputs' leading shape + (3,), of the inputs' kind; with return_transmittance, (rgb, tr), tr being the
        transmittance left at the end of each primary march (rgb - tr * env + tr * background composites over
        another background). A ray with a non-finite origin or a zero / non-finite direction gives NaN."""
        if self.integrator_id in (L.VR_FREE_FLIGHT, L.VR_MULTI_SCATTER):
            raise VRError(L.VR_ERR_UNSUPPORTED, f"{type(self).__name__}.render_rays: the free-flight integrators jitter "
                          "the sensor position of every sample, which a fixed ray does not have (ray-march integrators only)")
        torch_in, W, H, n, lead = _ray_grid_layout(origins, directions)
        dev = self._device(scene)
        if torch_in:
            import torch
            dev._check_torch(origins, directions)
            rays = torch.zeros((W * H, 8), dtype=torch.float32, device=origins.device)  # (pad rows: zero direction)
            zero = torch.zeros(1, dtype=torch.float32, device=origins.device)
            stream = torch.cuda.current_stream(origins.device).cuda_stream
            check(lib().vr_query_pack_rays_device(dev._h, origins.reshape(n, 3).contiguous().data_ptr(),
                                                  directions.reshape(n, 3).contiguous().data_ptr(), zero.data_ptr(), 0, n,
                                                  rays.data_ptr(), stream))
            if unit:
                rays[:n, 7] = 1.0
            rgb = torch.empty((W * H, 3), dtype=torch.float32, device=origins.device)
            tr = torch.empty(W * H, dtype=torch.float32, device=origins.device) if return_transmittance else None
            for attempt in range(3):  # a grid that outgrew the record buffers of earlier frames is rendered again
                check(lib().vr_render_rays_device(dev._h, rays.data_ptr(), W, H, ctypes.byref(self.params), rgb.data_ptr(),
                                                  tr.data_ptr() if return_transmittance else None, stream))
                try:
                    dev.synchronize()
                    break
                except VRError as e:
                    if attempt == 2 or e.status != L.VR_ERR_RETRY:
                        raise
        else:
            rays = _pack_ray_grid_numpy(origins, directions, unit, W, H, n)
            rgb = np.empty((W * H, 3), np.float32)
            tr = np.empty(W * H, np.float32) if return_transmittance else None
            check(lib().vr_render_rays(dev._h, rays.ctypes.data, W, H, ctypes.byref(self.params), fptr(rgb),
                                       fptr(tr) if return_transmittance else None))
        # (a multi-GPU context renders a grid on its first device: that rank's statistics)
        self.last_stats = dev.rank_stats(0) if isinstance(dev.device, tuple) else dev.stats()
        rgb = rgb[:n].reshape(lead + (3,))
        return (rgb, tr[:n].reshape(lead)) if return_transmittance else rgb


class RayMarchingGaussians(Integrator):
    """test_integrators.h:143-297: RayMarchingGaussians(camera, step_size=0.01, env_samples=20)."""

    integrator_id = L.VR_RAYMARCH_GAUSSIANS

    def __init__(self, camera, step_size=0.01, env_samples=20, t_eps=0.0, device=0):
        super().__init__(camera, step_size, env_samples, t_eps, device)


class PureRayMarching(Integrator):
    """integrator.h:100-267: PureRayMarching(camera, step_size=0.01, env_samples=20) — primary and
    shadow/environment transmittance marched at step_size (T *= exp(-sigma_t dt))."""

    integrator_id = L.VR_PURE_RAYMARCH

    def __init__(self, camera, step_size=0.01, env_samples=20, t_eps=0.0, device=0):
        super().__init__(camera, step_size, env_samples, t_eps, device)


# distance_solvers.h:143-147 (compile-time #defines in the reference) -> VR_OPT_FF_SOLVER values
SOLVERS = {"analytic_newton": 0, "bisection": 1, "newton": 2, "analytic_bisection": 3, "uniform": 4}


class FreeFlightGaussians(Integrator):
    """integrator.h:273-408: FreeFlightGaussians(camera, num_samples=256) — single scattering by
    free-flight sampling, one NEE sample (a light or the environment) per path. `solver`: the
    distance solver (SOLVERS; the reference's compiled-in ANALYTIC_PLUS_NEWTON by default)."""

    integrator_id = L.VR_FREE_FLIGHT

    def __init__(self, camera, num_samples=256, device=0, solver="analytic_newton"):
        super().__init__(camera, 0.01, 0, 0.0, device)
        self.params.num_samples = int(num_samples)
        self.solver = solver

    def set_num_samples(self, n):
        self.params.num_samples = int(n)


class MultiScatterGaussians(Integrator):
    """integrator.h:416-720: MultiScatterGaussians(camera, samples=16, min_bounces=5) — free-flight
    paths with NEE at every scattering event and Russian roulette after min_bounces."""

    integrator_id = L.VR_MULTI_SCATTER

    def __init__(self, camera, samples=16, min_bounces=5, device=0, solver="analytic_newton"):
        super().__init__(camera, 0.01, 0, 0.0, device)
        self.params.num_samples = int(samples)
        self.params.min_bounces = int(min_bounces)
        self.solver = solver

    def set_num_samples(self, n):  # integrator.h:719
        self.params.num_samples = int(n)

    def render(self, scene, image, per_pixel_gaussians=None, slot=0):
        """render(scene, image[, per_pixel_gaussians]) (integrator.h:525-536). With RECORD_PIXEL_GAUSSIANS
        semantics when `per_pixel_gaussians` is a list: it is filled with one sorted list of Gaussian
        indices per row-major pixel (integrator.h:616-644, 700-705). The device keeps the recording
        in `slot` (0/1) for vr_sfd_loss_diff; record() skips the host decode."""
        if per_pixel_gaussians is None:
            return super().render(scene, image)
        self.record(scene, image, slot)
        bits = self.pixel_gaussian_bits(slot)
        per_pixel_gaussians[:] = bits_to_lists(bits, scene.get_num_primitives())
        return image

    def record(self, scene, image, slot=0):
        dev = self._device(scene)
        W, H = image.get_width(), image.get_height()
        out = np.empty((H, W, 3), np.float32)
        check(lib().vr_render_record(dev._h, ctypes.byref(self.camera.struct), ctypes.byref(self.params), W, H,
                                     fptr(out), int(slot)))
        image.pixels[...] = out
        self._rec_shape = (scene.get_num_primitives(), W * H)
        self.last_stats = dev.stats()
        return image

    def pixel_gaussian_bits(self, slot=0):
        """(ceil(N/32), W*H) uint32: bit b of word w at pixel p <=> Gaussian 32w+b recorded at p."""
        n, npix = self._rec_shape
        bits = np.zeros(((n + 31) // 32, npix), np.uint32)
        check(lib().vr_get_pixel_gaussians(Device.get(self.device)._h, int(slot),
                                          bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), bits.size))
        return bits


def bits_to_lists(bits, n):
    """Decode a (words, npix) recording bitset into per-pixel sorted Gaussian index lists."""
    words, npix = bits.shape
    unpacked = np.unpackbits(bits.T.copy().view(np.uint8), axis=1, bitorder="little")[:, :n]
    return [np.nonzero(row)[0].astype(np.uint32).tolist() for row in unpacked]


class RayMarchingSpheres(Integrator):
    """test_integrators.h:11-136: RayMarchingSpheres(camera, step_size=0.01, env_samples=5)."""

    integrator_id = L.VR_RAYMARCH_SPHERES

    def __init__(self, camera, step_size=0.01, env_samples=5, t_eps=0.0, device=0):
        super().__init__(camera, step_size, env_samples, t_eps, device)


class TestIntegrator(Integrator):
    """integrator.h:65-94: magenta where the primary ray hits anything, env colour elsewhere."""

    __test__ = False  # not a pytest class
    integrator_id = L.VR_TEST_HITMASK

    def __init__(self, camera, device=0):
        super().__init__(camera, 0.01, 0, 0.0, device)
