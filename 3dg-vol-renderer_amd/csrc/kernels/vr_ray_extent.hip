// Ray grids (vr_render_rays_device, include/vr_hip.h): how far the step table of a caller's rays must reach.
// The march itself is the frame's (the RAYS instantiations of vr_gauss_march.hip / vr_spheres.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vr_dev_common.h"

namespace vr {
namespace dev {

// The scene box as a kernel argument: min xyz, max xyz (slab's layout).
struct Box {
    float b[6];
};

// Over the valid rays (grid_ray's test) whose slab test hits the scene box: the largest distance from a ray's
// origin to the farthest corner of the box, as the bits of a non-negative float (they order as unsigned
// integers) in *out, which the host zeroes first. Restates grid_extent (host/vr_rays.cpp) in f32.
// One ray per lane and grid stride, a wave reduction, one atomic max per wave that found a hit.
__global__ __launch_bounds__(256) void ray_extent_kernel(const float4* __restrict__ rays, uint32_t n, Box box,
                                                         uint32_t* __restrict__ out) {
    float best = 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const float4 a = rays[2 * i], b = rays[2 * i + 1];
        const float s = dot3(b.x, b.y, b.z, b.x, b.y, b.z);
        if (!(isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && s > 0.0f && isfinite(s))) continue;
        // (the slab test does not depend on the direction's length: no normalisation)
        const Ray r{a.x, a.y, a.z, b.x, b.y, b.z};
        float tmin, tmax;
        slab(box.b, r, __frcp_rn(b.x), __frcp_rn(b.y), __frcp_rn(b.z), tmin, tmax);
        if (!(tmax >= fmaxf(tmin, 0.0f))) continue;
        const float o[3] = {a.x, a.y, a.z};
        float d2 = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float e = fmaxf(fabsf(box.b[k] - o[k]), fabsf(box.b[3 + k] - o[k]));
            d2 += e * e;
        }
        best = fmaxf(best, sqrtf(d2));
    }
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63u) == 0u && best > 0.0f) atomicMax(out, __float_as_uint(best));
}

}  // namespace dev

hipError_t ray_extent(const vr_ray* rays, uint32_t n, const float bmin[3], const float bmax[3], uint32_t* out, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    dev::Box box;
    for (int k = 0; k < 3; ++k) {
        box.b[k] = bmin[k];
        box.b[3 + k] = bmax[k];
    }
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)n + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(dev::ray_extent_kernel, dim3(std::max(grid, 1u)), dim3(256), 0, s, reinterpret_cast<const float4*>(rays), n,
                       box, out);
    return hipGetLastError();
}

}  // namespace vr
