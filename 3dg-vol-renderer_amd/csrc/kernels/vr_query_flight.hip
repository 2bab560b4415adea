// The free-flight query (include/vr_hip.h, vr_query_free_flight): for a caller's ray and target optical depth,
// the collision distance of MultiScatterGaussians::get_free_flight_distance (integrator.h:422-498, the double
// running sum), the albedo there (evaluate_albedo, gmm.h:128-143) and the size of the critical segment's active
// set. Nothing of the sweep lives here: free_flight_distance<true>, the solvers and evaluate_albedo are the path
// kernels' own (vr_ff_bounce.h), on the same FFScratch rows, so a query takes every discrete decision in the forms a
// path's bounce does. The one difference is free_flight_distance's KEEP: a query carries the active list across hit
// windows, so its answers do not depend on where the windows fall (VR_OPT_FF_WINDOW0); a path that needs several
// windows rebuilds the list at each and may round an f32 sum over it differently. What a path adds to the flight
// (camera, PCG stream, phase function, NEE, throughput) is absent, which is what a caller who brings those wants.
//
// One lane per ray on a persistent grid of the path kernel's size (the rows' stride): a wave claims 64 consecutive
// rays from a counter. A ray over the rows' capacity (more than ff_hit_cap Gaussians overlapping one point) is
// queued, one atomic per wave, and re-run by the second launch with kFFBigCap-entry rows, as ff_fallback_kernel
// re-runs paths; only beyond those does a ray fail (NaN, counted for the host form's VR_ERR_OVERFLOW).
#include "vr_ff_bounce.h"

namespace vr {
namespace dev {

// ctl words: [0] next unclaimed ray, [1] queued rays, [2] rays over kFFBigCap; the queue follows at ctl + 4.
enum { kQfNext = 0, kQfQueued = 1, kQfFailed = 2, kQfQueue = 4 };

struct FlightOut {
    float* t;
    float* albedo;
    uint32_t* n_active;
    __device__ __forceinline__ void put(uint32_t id, float ts, float al, uint32_t na) const {
        t[id] = ts;
        if (albedo) albedo[id] = al;
        if (n_active) n_active[id] = na;
    }
};

// Ray `id` of the batch on rows S. Returns false if it is over the rows' capacity (nothing written).
// The row is decoded as decode_ray does (vr_march.h), in a copy: calling it moves both kernels' VGPRs (166 -> 162, 165 -> 168).
__device__ __forceinline__ bool flight_ray(const RenderArgs& A, FFScratch<false>& S, const vr_ray* __restrict__ rays,
                                           const float* __restrict__ tau, uint32_t id, const FlightOut& out, int* stack) {
    const float4* p = reinterpret_cast<const float4*>(rays) + 2 * (size_t)id;
    const float4 a = p[0], b = p[1];
    const float target = tau[id];
    const float s = dot3(b.x, b.y, b.z, b.x, b.y, b.z);
    const bool ok = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && s > 0.0f && isfinite(s);
    if (!ok || isnan(target)) {
        out.put(id, __builtin_nanf(""), __builtin_nanf(""), 0u);
        return true;
    }
    const Ray r = b.w != 0.0f ? Ray{a.x, a.y, a.z, b.x, b.y, b.z} : make_ray(a.x, a.y, a.z, b.x, b.y, b.z);
    int m = 0;
    const float ts = A.num_prims > 0 ? free_flight_distance<true, true>(A, S, r, target, m, stack, kFFBlock, 0u, 0) : -1.0f;
    if (ts == -2.0f) return false;
    if (ts < 0.0f) {  // no event, or no scatter before the last event (integrator.h:496-497)
        out.put(id, -1.0f, 0.0f, 0u);
        return true;
    }
    float al = 0.0f;
    if (out.albedo) al = evaluate_albedo(A, S, m, r.ox + ts * r.dx, r.oy + ts * r.dy, r.oz + ts * r.dz);
    out.put(id, ts, al, (uint32_t)m);
    return true;
}

__global__ void __launch_bounds__(kFFBlock) query_flight_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                const float* __restrict__ tau, uint32_t n, FlightOut out,
                                                                uint32_t* __restrict__ ctl) {
    __shared__ int s_stack[(kStackSize + kCollectQueue) * kFFBlock];  // walk stack + the walk's leaf FIFO
    int* stack = s_stack + threadIdx.x;
    const uint32_t gt = blockIdx.x * kFFBlock + threadIdx.x;
    FFScratch<false> S = ff_thread_scratch<false>(A, gt);
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ctl + kQfNext, 64u);
        base = __shfl(base, 0, 64);
        if (base >= n) break;  // (n < 2^31 and every claim adds 64 while base < n: the counter cannot wrap)
        const uint32_t id = base + lane;
        const bool over = id < n && !flight_ray(A, S, rays, tau, id, out, stack);
        // over the rows' capacity: queued for the second launch (one atomic per wave)
        const uint64_t mask = __ballot(over);
        if (mask != 0ull) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            uint32_t q = 0;
            if (lane == 0) q = atomicAdd(ctl + kQfQueued, (uint32_t)__popcll(mask));
            q = __shfl(q, 0, 64);
            if (over) ctl[kQfQueue + q + rank] = id;  // (at most n entries: every ray is queued once)
        }
    }
}

// The queued rays on kFFBigCap-entry rows (the layout of ff_fallback_kernel's).
__global__ void __launch_bounds__(kFFBlock) query_flight_big_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                    const float* __restrict__ tau, uint32_t n, FlightOut out,
                                                                    uint32_t* __restrict__ ctl) {
    __shared__ int s_stack[(kStackSize + kCollectQueue) * kFFBlock];
    int* stack = s_stack + threadIdx.x;
    const uint32_t gt = blockIdx.x * kFFBlock + threadIdx.x, nt = gridDim.x * kFFBlock;
    const uint32_t nq = min(ctl[kQfQueued], n);
    RenderArgs B = A;
    B.ff_threads = nt;
    B.ff_hit_cap = B.ff_act_cap = kFFBigCap;
    B.ff_hit = A.ff_big;
    B.ff_act0 = A.ff_big + (size_t)kFFBigCap * nt;
    B.ff_act1 = A.ff_big + (size_t)2 * kFFBigCap * nt;
    FFScratch<false> S = ff_thread_scratch<false>(B, gt);
    for (uint32_t q = gt; q < nq; q += nt) {
        const uint32_t id = ctl[kQfQueue + q];
        if (id < n && !flight_ray(B, S, rays, tau, id, out, stack)) {
            out.put(id, __builtin_nanf(""), __builtin_nanf(""), 0u);
            atomicAdd(ctl + kQfFailed, 1u);
        }
    }
}

}  // namespace dev

// ctl: query_flight_ctl_words(n) words. A.ff_* describe the rows (ff_threads: the first launch's resident grid;
// ff_big: 3 * kFFBigCap * kFFBigThreads cells).
size_t query_flight_ctl_words(uint32_t n) { return (size_t)dev::kQfQueue + n; }

hipError_t query_free_flight(const RenderArgs& A, const vr_ray* rays, const float* tau, uint32_t n, float* t, float* albedo,
                             uint32_t* n_active, uint32_t* ctl, hipStream_t s) {
    hipError_t e = hipMemsetAsync(ctl, 0, dev::kQfQueue * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const dev::FlightOut out{t, albedo, n_active};
    // no more blocks than the batch has 256-ray groups (each wave's first claim decides whether it has work)
    const unsigned blocks = (unsigned)std::min<uint64_t>(A.ff_threads / dev::kFFBlock, ((uint64_t)n + dev::kFFBlock - 1) / dev::kFFBlock);
    hipLaunchKernelGGL(dev::query_flight_kernel, dim3(std::max(1u, blocks)), dim3(dev::kFFBlock), 0, s, A, rays, tau, n, out, ctl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dev::query_flight_big_kernel, dim3(kFFBigThreads / dev::kFFBlock), dim3(dev::kFFBlock), 0, s, A, rays, tau, n,
                       out, ctl);
    return hipGetLastError();
}

}  // namespace vr
