// The radiance query (include/vr_hip.h, vr_query_radiance): the emission-absorption sum along each ray,
//   out[i][c] = sum_k q_ik T_ik sum_{g active at x_ik} m_g(x_ik) f_gc,   x_ik = o_i + t_ik d_i,
// for the caller's samples t, quadrature weights q and per-Gaussian rows f, with T the transmittance profile's Tr. The
// profile launcher (vr_query_profile.hip) has written Tr before this unit's kernel starts; the kernel is one more
// operation on the persistent ray-queue walk (ray_queue_walk, vr_walk.h) through QueryOp / query_walk
// (vr_query_common.h), in a unit of its own so that no other kernel is compiled differently for it.
//
// Because sum_k q T sum_g m f = sum_g f (sum_k q T m), a (ray, Gaussian) pair costs one mu_t per active sample and one
// multiply-add per channel. A work item is (ray, chunk of kFeatChunk channels): its sums are kFeatChunk doubles, the
// opacity sum and the pair count in registers (every loop over them is unrolled), its walk is the ray's slab walk pruned
// at the row's largest valid sample, and per record it loops over the row's K samples, read from global memory as
// ProfileGradOp::add reads them. The leaves a ray reaches hold every leaf whose box holds one of its sample points (the
// boxes are the 3-sigma boxes grown by 5 %, the point fl(o + t d) lies within an ulp of the ray), and a record is in one
// leaf, so every active (sample, Gaussian) pair is met exactly once.
//
// Floating point: the point per component __fadd_rn(o, __fmul_rn(t, d)) (what numpy and torch compute from f32 arrays),
// the decision sigma_active and m = mu_t in f32 exactly as vr_query_sigma / vr_query_features have them, every product
// and sum after that in double, one rounding to f32 per output. A channel of ones adds W * 1.0 = W where the opacity
// adds W, in the same order: the same bits. A channel's sums do not depend on its chunk or on C.
#include "../host/vr_kernels.h"
#include "vr_query_common.h"
#include "vr_radiance_interval.h"

namespace vr {
namespace dev {

constexpr int kFeatChunk = 8;  // vr_query_features.hip's: double sums a lane holds at once, a chunk is two float4 of a row

struct RadianceOp : QueryOp<RadianceOp, true> {
    using Base = QueryOp<RadianceOp, true>;
    const float* __restrict__ t;
    const float* __restrict__ q;     // nullptr: ones
    const float* __restrict__ tr;    // the profile's Tr, n * K
    const float* __restrict__ feat;  // the caller's rows
    float* out;
    float* opacity;
    uint32_t* n_pairs;
    uint32_t t_stride, q_stride, K, C, chunks;
    bool vec4;
    const float* row;   // the ray's K samples,
    const float* qrow;  // their weights (nullptr: ones)
    const float* trow;  // and their Tr
    uint32_t c0, nc;    // the item's first channel and how many it has
    double f[kFeatChunk], op;
    uint32_t cnt;
    // item id = ray * chunks + chunk
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const uint32_t ray = id / chunks;
        c0 = (id - ray * chunks) * (uint32_t)kFeatChunk;
        nc = min(C - c0, (uint32_t)kFeatChunk);
        const int what = Base::load(A, ray, r, tmax);  // (the row's own tmax is not used)
        row = t + (size_t)t_stride * ray;
        qrow = q ? q + (size_t)q_stride * ray : nullptr;
        trow = tr + (size_t)K * ray;
        float hi = -1.0f;  // the largest valid sample: finite and >= 0
        for (uint32_t k = 0; k < K; ++k) {
            const float v = row[k];
            if (v >= 0.0f && v < INFINITY) hi = fmaxf(hi, v);
        }
        tmax = fmaxf(hi, 0.0f);
        if (what == kRayInvalid) return what;
        // (a row whose valid samples are all at 0 walks: its origin may lie inside Gaussians)
        return hi < 0.0f || A.num_prims <= 0 ? kRayFinish : kRayWalk;
    }
    __device__ __forceinline__ void reset() {
        op = 0.0;
        cnt = 0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k) f[k] = 0.0;
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        float lo, hi;
        if (!radiance_interval(g, r, tmax, lo, hi)) return true;
        double W = 0.0;
        uint32_t pairs = 0;
        for (uint32_t k = 0; k < K; ++k) {
            const float tk = row[k];
            if (!(tk >= lo && tk <= hi)) continue;  // outside the interval, or not valid (lo >= 0, hi <= tmax < inf)
            const float x = __fadd_rn(r.ox, __fmul_rn(tk, r.dx));
            const float y = __fadd_rn(r.oy, __fmul_rn(tk, r.dy));
            const float z = __fadd_rn(r.oz, __fmul_rn(tk, r.dz));
            if (!sigma_active(g, x, y, z)) continue;
            const double qk = qrow ? (double)qrow[k] : 1.0;
            W += qk * (double)trow[k] * (double)mu_t(g, x, y, z);
            ++pairs;
        }
        if (pairs == 0) return true;
        cnt += pairs;
        op += W;
        const float* frow = feat + (size_t)A.gauss_order[j] * C + c0;
        float v[kFeatChunk];
        if (vec4) {
            const float4 a = reinterpret_cast<const float4*>(frow)[0];
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (nc > 4) b = reinterpret_cast<const float4*>(frow)[1];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < kFeatChunk; ++k) v[k] = (uint32_t)k < nc ? frow[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k) f[k] += W * (double)v[k];
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        const uint32_t ray = id / chunks;
        float* o = out + (size_t)ray * C + c0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k)
            if ((uint32_t)k < nc) o[k] = (float)f[k];
        if (c0 == 0) {
            if (opacity) opacity[ray] = (float)op;
            if (n_pairs) n_pairs[ray] = cnt;
        }
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        const uint32_t ray = id / chunks;
        float* o = out + (size_t)ray * C + c0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k)
            if ((uint32_t)k < nc) o[k] = __builtin_nanf("");
        if (c0 == 0) {
            if (opacity) opacity[ray] = __builtin_nanf("");
            if (n_pairs) n_pairs[ray] = 0u;
        }
    }
};
static_assert(kFeatChunk == 8, "RadianceOp::prim reads a chunk as two float4");

__global__ void __launch_bounds__(kQBlock) query_radiance_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                 const float* __restrict__ t, uint32_t t_stride,
                                                                 const float* __restrict__ q, uint32_t q_stride, uint32_t items,
                                                                 uint32_t K, const float* __restrict__ feat, uint32_t C,
                                                                 uint32_t chunks, int vec4, const float* __restrict__ tr,
                                                                 float* __restrict__ out, float* __restrict__ opacity,
                                                                 uint32_t* __restrict__ n_pairs, uint32_t* __restrict__ next,
                                                                 int refill) {
    RadianceOp op;
    op.rays = rays;
    op.t = t;
    op.q = q;
    op.tr = tr;
    op.feat = feat;
    op.out = out;
    op.opacity = opacity;
    op.n_pairs = n_pairs;
    op.t_stride = t_stride;
    op.q_stride = q_stride;
    op.K = K;
    op.C = C;
    op.chunks = chunks;
    op.vec4 = vec4 != 0;
    op.row = op.qrow = op.trow = nullptr;
    op.c0 = op.nc = 0;
    op.reset();
    query_walk(A, items, next, refill, op);
}

}  // namespace dev

// ---- launcher (host/vr_query_host.cpp) ----
// tr: n * K floats, written by query_transmittance_profile earlier on the same stream; out: n * C floats; opacity,
// n_pairs: n each or nullptr; every entry written. n > 0, n * ceil(C / 8) <= n * C < 2^31.
hipError_t query_radiance(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, const float* q,
                          uint32_t q_stride, uint32_t n, uint32_t K, const float* feat, uint32_t C, const float* tr, float* out,
                          float* opacity, uint32_t* n_pairs, uint32_t* next, int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t chunks = (C + (uint32_t)dev::kFeatChunk - 1u) / (uint32_t)dev::kFeatChunk;
    const int vec4 = C % 4u == 0 && ((uintptr_t)feat & 15u) == 0;
    hipLaunchKernelGGL(dev::query_radiance_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, q, q_stride,
                       n * chunks, K, feat, C, chunks, vec4, tr, out, opacity, n_pairs, next, refill);
    return hipGetLastError();
}

}  // namespace vr
