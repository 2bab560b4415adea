// The while-while walk of the 4-wide tree, defined once: a lane's walk state and its NODE and PRIM steps
// (WideWalk), the wave's NODE-or-PRIM choice, and the persistent "rays from a counter" kernel body
// (ray_queue_walk) that the shadow-ray kernel and the batched ray queries run as operations.
#pragma once
#include "vr_dev_common.h"

namespace vr {
namespace dev {

// ---- while-while walk of the 4-wide tree ----
// One lane's walk split into steps, so that a wave can spend each of its iterations on what most of its lanes
// need: a NODE iteration (4-wide node steps; leaf children go into a Q-entry LDS FIFO near-first, the nearest
// inner child is walked next, the others are pushed far-first) or a PRIM iteration (Gaussians of the queued
// leaves). The FIFO hands leaves out in the order the walk reaches them, which is traverse_wide's order.
// `stack` and `ring` are the lane's columns of LDS arrays with `stride` words per row.
template <int Q>
struct WideWalk {
    int sp, node, qh, qn;
    uint32_t j, end;  // Gaussians of the leaf being tested
    // wide = false (no 4-wide tree): nothing to walk, drained at once
    __device__ __forceinline__ void start(bool wide) {
        sp = 0;
        node = wide ? 0 : -1;
        qh = qn = 0;
        j = end = 0;
    }
    __device__ __forceinline__ bool has_prim() const { return j < end || qn > 0; }
    __device__ __forceinline__ bool can_node() const { return node >= 0 && qn <= Q - 4; }
    __device__ __forceinline__ bool drained() const { return node < 0 && j == end && qn == 0; }

    // One node step. False: the stack could overflow; the walk of the nodes ends there (node = -1) and the
    // caller redoes the whole walk on the child-pair tree.
    template <typename Prune>
    __device__ __forceinline__ bool node_step(const RenderArgs& A, const WideSlab& s, Prune prune, int* stack, int* ring,
                                              int stride) {
        float key[4];
        int32_t kr[4];
        wide_children(A, node, s.ix, s.iy, s.iz, s.oxi, s.oyi, s.ozi, prune, key, kr);
#pragma unroll
        for (int i = 0; i < 4; ++i)  // leaves, near first
            if (kr[i] < 0) {
                ring[((qh + qn) & (Q - 1)) * stride] = kr[i];
                ++qn;
            }
        int first = -1;
        int32_t next = 0;  // the nearest inner child (selects only: no dynamic register indexing)
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            first = kr[i] > 0 ? i : first;
            next = kr[i] > 0 ? kr[i] : next;
        }
        if (sp + 3 > kStackSize) {
            node = -1;
            return false;
        }
#pragma unroll
        for (int i = 3; i >= 0; --i)
            if (kr[i] > 0 && i != first) stack[(sp++) * stride] = kr[i];
        if (first >= 0) node = next;
        else if (sp > 0) node = stack[(--sp) * stride];
        else node = -1;
        return true;
    }

    // One Gaussian: prim(j) for the next record of the current leaf, or of the FIFO's next leaf (has_prim() holds).
    template <typename Prim>
    __device__ __forceinline__ void prim_step(const int* ring, int stride, Prim prim) {
        if (j == end) {
            const int32_t ref = ring[qh * stride];
            qh = (qh + 1) & (Q - 1);
            --qn;
            j = leaf_first(ref);
            end = j + leaf_count(ref);
        }
        prim(j);
        ++j;
    }
};

// The wave's next iteration, from the ballots of has_prim() and can_node(): PRIM (true) if no lane can take a
// node step, or at least as many lanes have a Gaussian to test.
__device__ __forceinline__ bool prim_iteration(uint64_t has_prim, uint64_t can_node) {
    const int np = __popcll(has_prim), nn = __popcll(can_node);
    return nn == 0 || (np > 0 && np >= nn);
}

// Prune bound of a walk that ends at tmax: tmax padded by a few ulp of the slab distances.
__device__ __forceinline__ float shadow_prune_lim(float tmax) { return tmax + kTPad * (1.0f + fminf(tmax, 1e30f)); }

// The persistent "rays from a counter" walk: rays 0 .. n - 1 are claimed from the counter word *next by a grid
// of resident waves, one ray per lane; a wave claims new rays by ballot once `refill` of its lanes are idle (or
// all are), so it never waits for its longest ray. Live lanes walk in NODE / PRIM iterations of STEPS steps.
// The ray's operation:
//   Op::kPrune          children beyond tmax are skipped
//   load(A, id, r, tmax) the ray and its tmax; kRayWalk, kRayFinish (no walk: reset() and finish()) or kRayInvalid
//   reset()             before the first prim() of a walk
//   prim(A, r, tmax, j) record j; false: the ray needs no further Gaussian
//   on_node()           per node step (work counters)
//   redo(A, id, r, tmax, lim, stack)  the whole walk again on the child-pair tree and the ray's result: a walk
//                       whose stack could overflow, and every walk of a scene without the 4-wide tree
//   finish(A, id, tmax) / invalid(id)  the ray's result
enum { kRayWalk = 0, kRayFinish = 1, kRayInvalid = 2 };
template <int Q, int STEPS, class Op>
__device__ __forceinline__ void ray_queue_walk(const RenderArgs& A, uint32_t n, uint32_t* next, int refill, int* stack,
                                               int* ring, int stride, Op& op) {
    const uint32_t lane = threadIdx.x & 63u;
    bool live = false, exhausted = false;
    uint32_t id = 0;
    Ray r{};
    float tmax = 0.0f, lim = 0.0f;
    WideSlab s{};
    WideWalk<Q> w;
    w.start(false);
    bool redo = false;  // no 4-wide tree, or its stack could overflow: the pair-tree walk at completion
    bool stop = false;  // the operation needs no further Gaussian
    auto prune = [&](float tmin, float) { return !Op::kPrune || tmin <= lim; };
    for (;;) {
        const uint64_t idle = __ballot(!live);
        if (!exhausted && (idle == ~0ull || __popcll(idle) >= refill)) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(next, (uint32_t)__popcll(idle));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            // (64-bit compare: the counter stays below n + 64 * waves, but base + 64 must not wrap)
            exhausted = (uint64_t)base + (uint64_t)__popcll(idle) >= (uint64_t)n;
            if (!live) {
                const uint64_t mine = (uint64_t)base +
                                      __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (mine < (uint64_t)n) {
                    id = (uint32_t)mine;
                    const int what = op.load(A, id, r, tmax);
                    if (what == kRayInvalid) {
                        op.invalid(id);
                    } else if (what == kRayFinish) {
                        op.reset();
                        op.finish(A, id, tmax);
                    } else {
                        s = wide_slab(A, r);
                        lim = Op::kPrune ? shadow_prune_lim(tmax) : INFINITY;
                        op.reset();
                        stop = false;
                        redo = A.hnodes4 == nullptr;
                        w.start(!redo);
                        live = true;
                    }
                }
            }
        }
        if (!__any(live)) {
            if (exhausted) break;
            continue;
        }
        const bool has_prim = live && w.has_prim();  // (a lane that stopped or must redo was finished below)
        const bool can_node = live && w.can_node();
        if (prim_iteration(__ballot(has_prim), __ballot(can_node))) {
            bool go = has_prim;
            for (int k = 0; k < STEPS; ++k) {
                if (go) w.prim_step(ring, stride, [&](uint32_t j) { stop = !op.prim(A, r, tmax, j); });
                go = go && w.has_prim() && !stop;
            }
        } else {
            bool go = can_node;
            for (int k = 0; k < STEPS; ++k) {
                if (go) {
                    op.on_node();
                    if (!w.node_step(A, s, prune, stack, ring, stride)) redo = true;
                }
                go = go && w.can_node();
            }
        }
        if (live && (redo || stop || w.drained())) {
            if (redo) op.redo(A, id, r, tmax, lim, stack);
            else op.finish(A, id, tmax);
            live = false;
        }
    }
}

}  // namespace dev
}  // namespace vr
