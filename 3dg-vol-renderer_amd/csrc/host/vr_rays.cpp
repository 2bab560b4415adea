// Ray grids (vr_render_rays, vr_render_rays_device): a W x H image of the caller's own rays rendered by the
// ray-march integrators exactly as a frame is. Only the rays' source and the extent that sizes the step table
// are the grid's own; the kernel arguments, pipelines, report and retry logic are the frame's (vr_frame.cpp).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "vr_ctx.h"

using namespace vr;

namespace {

// A step table never holds more entries than this (64 MB): a ray that starts far from the scene is refused
// (VR_ERR_OVERFLOW) instead of sizing a table by the caller's coordinates.
constexpr uint32_t kMaxTableEntries = 1u << 24;

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The largest distance from the origin of a valid ray that hits the box [bmin, bmax] to the box's farthest corner
// (0: no such ray). Valid: a finite origin and a direction whose squared norm is positive and finite in f32 (the
// kernels' test, grid_ray). The slab test is the kernels' (vr_march.h slab: f32, NaN-dropping min / max, a hit iff
// tmax >= max(tmin, 0)); it does not depend on the direction's length. The distance is scene_tmax's: f32
// differences, squared and summed in double.
float grid_extent(const vr_ray* rays, size_t n, const float bmin[3], const float bmax[3]) {
    float best = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float* o = rays[i].origin;
        const float* d = rays[i].direction;
        const float s = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]);
        if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) && s > 0.0f && std::isfinite(s))) continue;
        float tmin = -INFINITY, tmax = INFINITY;
        for (int k = 0; k < 3; ++k) {
            const float inv = 1.0f / d[k];
            const float t1 = (bmin[k] - o[k]) * inv, t2 = (bmax[k] - o[k]) * inv;
            tmin = std::fmax(tmin, std::fmin(t1, t2));
            tmax = std::fmin(tmax, std::fmax(t1, t2));
        }
        if (!(tmax >= std::fmax(tmin, 0.0f))) continue;
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const float e = std::fmax(std::fabs(bmin[k] - o[k]), std::fabs(bmax[k] - o[k]));
            d2 += (double)e * e;
        }
        best = std::max(best, (float)std::sqrt(d2));
    }
    return best;
}

// What the two forms share before the rays are looked at: the frame's own checks, the grid's.
vr_status grid_begin(vr_ctx* c, const char* what, const void* rays, const vr_render_params* p, const float* rgb, uint32_t W,
                     uint32_t H, RenderArgs& A) {
    if (!c || !rays || !p || !rgb) return fail(VR_ERR_INVALID, std::string(what) + ": NULL argument");
    if (W == 0 || H == 0 || W > 65535 || H > 65535) return fail(VR_ERR_INVALID, "width/height must be in [1, 65535]");
    if (p->integrator == VR_FREE_FLIGHT || p->integrator == VR_MULTI_SCATTER)
        return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": the free-flight integrators jitter the sensor position of "
                                            "every sample, which a fixed ray does not have (ray-march integrators only)");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    return fill_scene_args(c, p, W, H, A);
}

// The whole W x H grid d_rays (device memory) as one frame into d_rgb / d_tr.
GridSrc grid_frame(RenderArgs& A, const vr_ray* d_rays, uint32_t W, uint32_t H, float* d_rgb, float* d_tr) {
    A.out = d_rgb;
    A.first_tile = 0;
    A.tile_stride = 1;
    A.num_tiles = vr_num_tiles(W, H);
    A.packed = 0;
    return GridSrc{reinterpret_cast<const float4*>(d_rays), d_tr};
}

}  // namespace

extern "C" {

vr_status vr_ray_grid_extent(const vr_ray* rays, size_t n, const float bounds_min[3], const float bounds_max[3], float* extent) {
    if (!extent || !bounds_min || !bounds_max || (n > 0 && !rays)) return fail(VR_ERR_INVALID, "vr_ray_grid_extent: NULL argument");
    *extent = grid_extent(rays, n, bounds_min, bounds_max);
    return VR_OK;
}

vr_status vr_render_rays_device(vr_ctx* c, const vr_ray* d_rays, uint32_t W, uint32_t H, const vr_render_params* p, float* d_rgb,
                                float* d_tr, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(grid_begin(c, "vr_render_rays_device", d_rays, p, d_rgb, W, H, A));
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_render_rays_device: the device ray array must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (needs_table(p)) {  // the extent of the caller's rays: a reduction and one 4-byte read-back (waits for `stream`)
        VR_TRY(c->ray_ext.grow(1, "hipMalloc(ray extent)"));
        HIP_TRY(ray_extent(d_rays, W * H, c->scene.bmin, c->scene.bmax, c->ray_ext.get(), s), "ray_extent_kernel");
        float extent = 0.0f;
        HIP_TRY(hipMemcpyAsync(&extent, c->ray_ext.get(), sizeof(float), hipMemcpyDeviceToHost, s), "hipMemcpy(ray extent)");
        HIP_TRY(hipStreamSynchronize(s), "ray_extent_kernel");
        VR_TRY(fill_table(c, p, table_tmax(c, extent), kMaxTableEntries, A));
    }
    const GridSrc grid = grid_frame(A, d_rays, W, H, d_rgb, d_tr);
    return launch(c, A, p, s, false, &grid);  // outcome: vr_synchronize / vr_get_stats
}

vr_status vr_render_rays(vr_ctx* c, const vr_ray* rays, uint32_t W, uint32_t H, const vr_render_params* p, float* rgb, float* tr) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(grid_begin(c, "vr_render_rays", rays, p, rgb, W, H, A));
    const size_t npix = (size_t)W * H;
    if (needs_table(p))
        VR_TRY(fill_table(c, p, table_tmax(c, grid_extent(rays, npix, c->scene.bmin, c->scene.bmax)), kMaxTableEntries, A));
    VR_TRY(c->ray_in.grow(npix, "hipMalloc(ray grid)"));
    HIP_TRY(hipMemcpy(c->ray_in.get(), rays, npix * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(ray grid)");
    if (npix * 3 > c->frame.count()) VR_TRY(c->frame.alloc(npix * 3, "hipMalloc(frame)"));
    if (tr) VR_TRY(c->ray_tr.grow(npix, "hipMalloc(ray transmittance)"));
    const GridSrc grid = grid_frame(A, c->ray_in.get(), W, H, c->frame.get(), tr ? c->ray_tr.get() : nullptr);
    VR_TRY(render_sync(c, A, p, &grid));
    HIP_TRY(hipMemcpy(rgb, c->frame.get(), npix * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(frame)");
    if (tr) HIP_TRY(hipMemcpy(tr, c->ray_tr.get(), npix * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(ray transmittance)");
    return VR_OK;
}

}  // extern "C"
