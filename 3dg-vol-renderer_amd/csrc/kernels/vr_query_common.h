// What the units of the batched queries share (vr_query.hip, vr_query_profile.hip, vr_query_features.hip): the block
// shape of a query walk, the base of a ray's operation on the persistent ray-queue walk (ray_queue_walk, vr_walk.h), one
// block of that walk with its LDS, and the launch grid; for the point queries (sigma, features) the active-set decision
// and the two containment walks.
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

// ---- sigma: containment walk, one point per lane ----
// Gaussian i is active at x iff p.(M p) - 9 <= 0, p = x - mean, in f32 in quad's order for Cq (the value
// whose sign decides intersect_direct's C for a ray starting at x). A child is entered iff the point lies
// in its box: the leaf boxes are the 3-sigma boxes grown by 5 % (gaussian_bounds), and the f16 boxes of the
// 4-wide tree are rounded outward from them (f16_directed, host and device builders), so every ellipsoid
// holding x is reached. Sums in double (see the head of vr_query.hip).
// The decision itself: the sigma query's, its gradient's and the feature queries', so their active sets are the same bit
// for bit.
__device__ __forceinline__ bool sigma_active(const GRec& g, float x, float y, float z) {
    const float px = x - g.mx, py = y - g.my, pz = z - g.mz;
    const float mpx = g.m00 * px + (g.m01 * py + g.m02 * pz);
    const float mpy = g.m01 * px + (g.m11 * py + g.m12 * pz);
    const float mpz = g.m02 * px + (g.m12 * py + g.m22 * pz);
    const float C = dot3(px, py, pz, mpx, mpy, mpz) - 9.0f;
    return C <= 0.0f;
}

// The containment walk of the 4-wide f16 tree, shared by the sigma and the feature kernels through the leaf
// accumulator: acc.leaf(A, ref, x, y, z) for every leaf whose box holds the point. True: the LDS stack could
// overflow and the walk broke off (some leaves were handed out already); the caller walks the child-pair tree.
template <class Acc>
__device__ __forceinline__ bool sigma_walk_wide(const RenderArgs& A, float x, float y, float z, int* stack, Acc& acc) {
    float ux = x, uy = y, uz = z;
    node_space<true>(A, ux, uy, uz);
    int sp = 0, node = 0;
    for (;;) {
        const uint4* np = reinterpret_cast<const uint4*>(A.hnodes4 + node);
        const uint4 q0 = np[0], q1 = np[1], q2 = np[2], rf = np[3];
        const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        const int32_t ref[4] = {(int32_t)rf.x, (int32_t)rf.y, (int32_t)rf.z, (int32_t)rf.w};
        if (sp + 4 > kStackSize) return true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // child c: halves 6c .. 6c + 5 = min xyz, max xyz
            float b[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int h = 6 * c + k;
                const uint32_t word = w[h >> 1];
                b[k] = (float)__builtin_bit_cast(_Float16, (uint16_t)((h & 1) ? (word >> 16) : (word & 0xffffu)));
            }
            const bool in = ref[c] != 0 && ux >= b[0] && ux <= b[3] && uy >= b[1] && uy <= b[4] && uz >= b[2] && uz <= b[5];
            if (in) {
                if (ref[c] < 0) acc.leaf(A, ref[c], x, y, z);
                else stack[(sp++) * kQBlock] = ref[c];
            }
        }
        if (sp == 0) return false;
        node = stack[(--sp) * kQBlock];
    }
}

// The same walk on the f32 child-pair tree: one push per level at most. True: the tree is deeper than the builder
// allows and the walk broke off.
template <class Acc>
__device__ __forceinline__ bool sigma_walk_pair(const RenderArgs& A, float x, float y, float z, int* stack, Acc& acc) {
    int sp = 0, node = 0;
    for (;;) {
        float f[12];
        int2 nc;
        load_pair<false>(A, node, f, nc);
        int32_t go[2] = {0, 0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float* b = f + 6 * s;
            const int32_t c = s == 0 ? nc.x : nc.y;
            const bool in = c != 0 && x >= b[0] && x <= b[3] && y >= b[1] && y <= b[4] && z >= b[2] && z <= b[5];
            if (in) {
                if (c < 0) acc.leaf(A, c, x, y, z);
                else go[s] = c;
            }
        }
        if (go[0] > 0 && go[1] > 0) {
            if (sp >= kStackSize) return true;  // (deeper than the builder allows)
            stack[(sp++) * kQBlock] = go[1];
            node = go[0];
        } else if (go[0] > 0 || go[1] > 0) {
            node = go[0] > 0 ? go[0] : go[1];
        } else {
            if (sp == 0) return false;
            node = stack[(--sp) * kQBlock];
        }
    }
}

}  // namespace dev

static inline dim3 query_grid(int cus) { return dim3((unsigned)std::max(1, cus) * VR_QUERY_BLOCKS); }

}  // namespace vr
