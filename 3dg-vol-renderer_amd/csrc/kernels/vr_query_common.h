// What the units of the batched ray queries share (vr_query.hip, vr_query_profile.hip): the block shape of a query
// walk, the base of a ray's operation on the persistent ray-queue walk (ray_queue_walk, vr_walk.h), one block of that
// walk with its LDS, and the launch grid.
#pragma once
#include <algorithm>

#include "vr_dev_common.h"
#include "vr_walk.h"

namespace vr {
namespace dev {

constexpr int kQBlock = 256;
#ifndef VR_QUERY_BLOCKS
#define VR_QUERY_BLOCKS 4  // resident 256-lane blocks per CU (40 KB of LDS each: 4 waves per SIMD)
#endif
constexpr int kQQueue = 8, kQSteps = 4;  // leaf FIFO entries; node steps / Gaussians per lane per wave iteration

// ---- per-ray operations of the walk (ray_queue_walk's Op) ----
// What the three share. vr_ray row i (16-B aligned), its normalisation and what makes it invalid: decode_ray
// (vr_march.h). PRUNE: rays with tmax <= 0 / NaN finish at once.
template <class Op, bool PRUNE>
struct QueryOp {
    static constexpr bool kPrune = PRUNE;
    const vr_ray* __restrict__ rays;
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        if (!decode_ray(reinterpret_cast<const float4*>(rays) + 2 * (size_t)id, r, tmax)) return kRayInvalid;
        return (PRUNE && !(tmax > 0.0f)) || A.num_prims <= 0 ? kRayFinish : kRayWalk;  // gmm.h:518-519 / :462: no walk
    }
    __device__ __forceinline__ void on_node() {}
    // The whole walk of the ray on the child-pair tree (half-precision nodes if the scene has them), and its result.
    __device__ __forceinline__ void redo(const RenderArgs& A, uint32_t id, const Ray& r, float tmax, float lim, int* stack) {
        Op& op = static_cast<Op&>(*this);
        op.reset();
        auto prune = [&](float tmin, float) { return !PRUNE || tmin <= lim; };
        auto leaf = [&](uint32_t first, uint32_t count) {
            for (uint32_t j = first; j < first + count; ++j)
                if (!op.prim(A, r, tmax, j)) return false;
            return true;
        };
        if (A.hnodes) traverse<true>(A, r, stack, kQBlock, prune, leaf);
        else traverse<false>(A, r, stack, kQBlock, prune, leaf);
        op.finish(A, id, tmax);
    }
};

// One block of the persistent grid: its LDS stack and leaf FIFO, then the walk.
template <class Op>
__device__ __forceinline__ void query_walk(const RenderArgs& A, uint32_t n, uint32_t* next, int refill, Op& op) {
    __shared__ int s_stack[(kStackSize + kQQueue) * kQBlock];
    int* stack = s_stack + threadIdx.x;
    ray_queue_walk<kQQueue, kQSteps>(A, n, next, refill, stack, stack + kStackSize * kQBlock, kQBlock, op);
}

}  // namespace dev

static inline dim3 query_grid(int cus) { return dim3((unsigned)std::max(1, cus) * VR_QUERY_BLOCKS); }

}  // namespace vr
