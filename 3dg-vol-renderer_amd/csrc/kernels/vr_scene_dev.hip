// The front of the scene upload on the device (vr_upload_gaussians_device, include/vr_hip.h): what
// vr_scene.cpp's precompute_gaussian / gaussian_bounds and vr_upload.cpp's host loops compute per Gaussian,
// for parameters that already live in device memory.
//   1. scene_prepare_kernel, one thread per Gaussian: the 48-B record, the 6-float box, the box's largest
//      extent (half_tree_rule's `ext`) and, per block, a SceneStats partial (scene box, centroid box, the
//      overlap heuristic's double box and volume sum); scene_fold_kernel, one block, folds the partials.
//   2. scene_chord_sample_kernel: scene_median_chord_depth's sampled central-chord depths.
//   3. scene_sort_ext: hipcub key sort of `ext`, whose element of rank n / 2 is half_tree_rule's median.
// Floating point: this unit is compiled like every other with -ffp-contract=off and HIP's correctly rounded f32
// division and square root, and restates the host expressions operation by operation, so every record word
// but `norm` and every box word is the host's bit for bit. `norm` is (float)(K * (double)(float)(1 / sqrt(
// (double)det))) with K = (2 pi)^-1.5 passed in by the host: IEEE operations only (the host's powf is libm's).
// Minima and maxima are exact in any order; the volume sum is reduced in a fixed order (a butterfly per wave,
// the waves of a block in order, the blocks in order per thread of the one folding block), so a scene gives
// the same sum on every run.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "../vr_internal.h"

namespace vr {
namespace scene_dev {

constexpr uint32_t kBlock = 256;

// std::min / std::max as the host loops use them: a NaN operand never replaces the accumulator.
template <class T>
__device__ __forceinline__ T keep_min(T acc, T v) { return v < acc ? v : acc; }
template <class T>
__device__ __forceinline__ T keep_max(T acc, T v) { return acc < v ? v : acc; }

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, o, 64);
    hi = __shfl_xor(hi, o, 64);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void stats_identity(SceneStats& p) {
    for (int k = 0; k < 3; ++k) {
        p.bmin[k] = p.cmin[k] = INFINITY;
        p.bmax[k] = p.cmax[k] = -INFINITY;
        p.olo[k] = (double)INFINITY;
        p.ohi[k] = -(double)INFINITY;
    }
    p.vol = 0.0;
}

__device__ __forceinline__ void stats_merge(SceneStats& a, const SceneStats& b) {
    for (int k = 0; k < 3; ++k) {
        a.bmin[k] = keep_min(a.bmin[k], b.bmin[k]);
        a.bmax[k] = keep_max(a.bmax[k], b.bmax[k]);
        a.cmin[k] = keep_min(a.cmin[k], b.cmin[k]);
        a.cmax[k] = keep_max(a.cmax[k], b.cmax[k]);
        a.olo[k] = keep_min(a.olo[k], b.olo[k]);
        a.ohi[k] = keep_max(a.ohi[k], b.ohi[k]);
    }
    a.vol += b.vol;
}

// The block's threads' values folded into thread 0's p: a butterfly over each wave's 64 lanes, then the four
// waves in order. Every thread of the block calls it.
__device__ __forceinline__ void block_fold(SceneStats& p, SceneStats* lds /* kBlock / 64 */) {
    for (int o = 32; o > 0; o >>= 1) {
        SceneStats q;
        for (int k = 0; k < 3; ++k) {
            q.bmin[k] = __shfl_xor(p.bmin[k], o, 64);
            q.bmax[k] = __shfl_xor(p.bmax[k], o, 64);
            q.cmin[k] = __shfl_xor(p.cmin[k], o, 64);
            q.cmax[k] = __shfl_xor(p.cmax[k], o, 64);
            q.olo[k] = shfl_xor_f64(p.olo[k], o);
            q.ohi[k] = shfl_xor_f64(p.ohi[k], o);
        }
        q.vol = shfl_xor_f64(p.vol, o);
        stats_merge(p, q);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) lds[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < kBlock / 64; ++w) stats_merge(p, lds[w]);
}

// vr_scene.cpp, cof(): cofactor of a full row-major 3 x 3 matrix.
__device__ __forceinline__ float cof(const float m[3][3], int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}

__global__ __launch_bounds__(kBlock) void scene_prepare_kernel(const float* __restrict__ mean, const float* __restrict__ cov6,
                                                               const float* __restrict__ density,
                                                               const float* __restrict__ albedo, uint32_t n, double K,
                                                               float4* __restrict__ rec, float2* __restrict__ boxes,
                                                               float* __restrict__ ext, SceneStats* __restrict__ partials) {
    __shared__ SceneStats lds[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    SceneStats p;
    stats_identity(p);
    if (i < n) {
        const float mu[3] = {mean[3 * (size_t)i], mean[3 * (size_t)i + 1], mean[3 * (size_t)i + 2]};
        float c[6];
        for (int k = 0; k < 6; ++k) c[k] = cov6[6 * (size_t)i + k];
        // ---- precompute_gaussian (vr_scene.cpp), operation by operation ----
        const float m[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
        const float c00 = cof(m, 0, 0), c10 = cof(m, 1, 0), c20 = cof(m, 2, 0);
        const float det_inv = c00 * m[0][0] + (c10 * m[1][0] + c20 * m[2][0]);
        const float invdet = 1.0f / det_inv;
        const float i00 = c00 * invdet, i01 = c10 * invdet, i02 = c20 * invdet;
        const float i11 = cof(m, 1, 1) * invdet, i12 = cof(m, 2, 1) * invdet, i22 = cof(m, 2, 2) * invdet;
        const float d0 = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]);
        const float d1 = m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]);
        const float d2 = m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        const float det_cov = d0 - d1 + d2;
        const float rs = (float)(1.0 / sqrt((double)det_cov));
        const float norm = (float)(K * (double)rs);
        rec[3 * (size_t)i] = make_float4(mu[0], mu[1], mu[2], density[i]);
        rec[3 * (size_t)i + 1] = make_float4(i00, i01, i02, i11);
        rec[3 * (size_t)i + 2] = make_float4(i12, i22, norm, albedo[i]);
        // ---- gaussian_bounds, and upload_device_bvh's centroid and extent ----
        const float diag[3] = {c[0], c[3], c[5]};
        float lo[3], hi[3], e = 0.0f;
        for (int k = 0; k < 3; ++k) {
            float h = 3.0f * sqrtf(keep_max(diag[k], 0.0f));
            h = h * 1.05f + 1e-6f;
            lo[k] = mu[k] - h;
            hi[k] = mu[k] + h;
            p.bmin[k] = keep_min(p.bmin[k], lo[k]);
            p.bmax[k] = keep_max(p.bmax[k], hi[k]);
            const float ce = 0.5f * (lo[k] + hi[k]);
            p.cmin[k] = keep_min(p.cmin[k], ce);
            p.cmax[k] = keep_max(p.cmax[k], ce);
            e = keep_max(e, hi[k] - lo[k]);
        }
        boxes[3 * (size_t)i] = make_float2(lo[0], lo[1]);
        boxes[3 * (size_t)i + 1] = make_float2(lo[2], hi[0]);
        boxes[3 * (size_t)i + 2] = make_float2(hi[1], hi[2]);
        ext[i] = e;
        // ---- scene_overlap (vr_upload.cpp) ----
        const double a = c[0], b = c[1], cc = c[2], d = c[3], ee = c[4], f = c[5];
        const double det = a * (d * f - ee * ee) - b * (b * f - ee * cc) + cc * (b * ee - d * cc);
        if (det > 0.0) p.vol = 4.0 / 3.0 * M_PI * 27.0 * sqrt(det);
        const double ex[3] = {3.0 * sqrt(keep_max(a, 0.0)), 3.0 * sqrt(keep_max(d, 0.0)), 3.0 * sqrt(keep_max(f, 0.0))};
        for (int k = 0; k < 3; ++k) {
            p.olo[k] = keep_min(p.olo[k], (double)mu[k] - ex[k]);
            p.ohi[k] = keep_max(p.ohi[k], (double)mu[k] + ex[k]);
        }
    }
    block_fold(p, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

__global__ __launch_bounds__(kBlock) void scene_fold_kernel(const SceneStats* __restrict__ partials, uint32_t nblocks,
                                                            SceneStats* __restrict__ out) {
    __shared__ SceneStats lds[kBlock / 64];
    SceneStats p;
    stats_identity(p);
    for (uint32_t j = threadIdx.x; j < nblocks; j += kBlock) stats_merge(p, partials[j]);
    block_fold(p, lds);
    if (threadIdx.x == 0) *out = p;
}

// scene_median_chord_depth's samples (vr_upload.cpp): sample k is Gaussian k * step along direction k & 3; a
// Gaussian the host loop skips gives NaN.
__global__ __launch_bounds__(kBlock) void scene_chord_sample_kernel(const float4* __restrict__ rec, uint32_t n, uint32_t step,
                                                                    uint32_t count, double* __restrict__ out) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const size_t i = (size_t)k * step;
    double tau = __longlong_as_double(0x7ff8000000000000ll);
    if (i < n) {
        const float4 r0 = rec[3 * i], r1 = rec[3 * i + 1], r2 = rec[3 * i + 2];
        const float s = 0.57735027f;
        const uint32_t w = k & 3u;
        const float d[3] = {w == 0u ? 1.0f : (w == 3u ? s : 0.0f), w == 1u ? 1.0f : (w == 3u ? s : 0.0f),
                            w == 2u ? 1.0f : (w == 3u ? s : 0.0f)};
        const float m[6] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};  // 00 01 02 11 12 22
        const double a = (double)m[0] * d[0] * d[0] + (double)m[3] * d[1] * d[1] + (double)m[5] * d[2] * d[2] +
                         2.0 * ((double)m[1] * d[0] * d[1] + (double)m[2] * d[0] * d[2] + (double)m[4] * d[1] * d[2]);
        if (a > 0.0 && isfinite(a)) tau = (double)r0.w * (double)r2.z * sqrt(2.0 * M_PI / a);
    }
    out[k] = tau;
}

}  // namespace scene_dev

uint32_t scene_prepare_blocks(uint32_t n) { return (n + scene_dev::kBlock - 1) / scene_dev::kBlock; }

// partials: scene_prepare_blocks(n) + 1 entries, the last of which receives the scene's statistics.
hipError_t scene_prepare(const float* mean, const float* cov6, const float* density, const float* albedo, uint32_t n, double K,
                         GaussianRecord* rec, float* boxes, float* ext, SceneStats* partials, hipStream_t s) {
    using namespace scene_dev;
    const uint32_t nb = scene_prepare_blocks(n);
    hipLaunchKernelGGL(scene_prepare_kernel, dim3(nb), dim3(kBlock), 0, s, mean, cov6, density, albedo, n, K,
                       reinterpret_cast<float4*>(rec), reinterpret_cast<float2*>(boxes), ext, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scene_fold_kernel, dim3(1), dim3(kBlock), 0, s, partials, nb, partials + nb);
    return hipGetLastError();
}

hipError_t scene_chord_samples(const GaussianRecord* rec, uint32_t n, uint32_t step, uint32_t count, double* out, hipStream_t s) {
    using namespace scene_dev;
    hipLaunchKernelGGL(scene_chord_sample_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                       reinterpret_cast<const float4*>(rec), n, step, count, out);
    return hipGetLastError();
}

// tmp == nullptr: only tmp_bytes is set. The keys are non-negative floats or NaN; sorted ascending.
hipError_t scene_sort_ext(const float* ext, float* sorted, uint32_t n, void* tmp, size_t& tmp_bytes, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, ext, sorted, (int)n, 0, 32, s);
}

}  // namespace vr
