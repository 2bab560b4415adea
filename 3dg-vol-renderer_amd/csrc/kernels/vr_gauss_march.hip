// Stage 1 of the RayMarchingGaussians pipeline (vr_gauss_common.h): the primary march, its fallback passes and
// the binned variant, with their launchers gauss_march, gauss_bin and gauss_bin_scan.
#include <hipcub/hipcub.hpp>

#include "vr_gauss_common.h"

// Tuning knobs of this unit (A/B builds: tools/ab_build.sh NAME vr_gauss_march "-DVR_...=...").
#ifndef VR_MARCH_DEEP
// Private-memory (scratch) stack entries of the primary march's 4-wide walks past its LDS stack; a walk past both goes
// to the fallback pass. Round 6, C4 (same frame hash): LDS 24 + 0 -> 14 + 10 moved the quarter-tile workgroup from
// 10 to 7.5 KB of LDS, 4 -> 5 waves/SIMD, march 13.95 -> 12.92 ms (12 + 12: 13.02, 10 + 14: 13.2, 16 + 8: 13.7).
#define VR_MARCH_DEEP 10
#endif
#ifndef VR_BIN_PEND
#define VR_BIN_PEND 48  // pending entries per lane of the binned march (kPendCap)
#endif
#ifndef VR_MARCH_BLOCK
#define VR_MARCH_BLOCK 64  // lanes per march workgroup: 256 (a tile) or 64 (a quarter tile; -6 % march time)
#endif
#ifndef VR_MARCH_ACT
#define VR_MARCH_ACT 16  // active-list LDS slots per lane of the primary march (A/B)
#endif
#ifndef VR_MARCH_STACK4
#define VR_MARCH_STACK4 14  // LDS stack entries per lane of the primary march's 4-wide walks (A/B; then VR_MARCH_DEEP)
#endif
#ifndef VR_MARCH_ACT_BIG
#define VR_MARCH_ACT_BIG 32  // the primary march's slots once a scene's frames overflow 16 on >= 5 % of their pixels
#endif

namespace vr {

constexpr int kMarchBlock = VR_MARCH_BLOCK;                                // lanes per workgroup of the tile pass
constexpr int kActFast = VR_MARCH_ACT, kActBig = VR_MARCH_ACT_BIG;         // its active-list slots per lane (LDS)
constexpr int kMarchStack4 = VR_MARCH_STACK4, kMarchDeep = VR_MARCH_DEEP;  // its 4-wide walks' LDS + private stack entries
constexpr int kActFallback = 64, kWaveBlock = 64;  // the wave pass: active-list slots per pixel (LDS); one wave

namespace dev {

// ---------------------------------------------------------------------------------------------
// Stage 1: primary march
//
// Every pixel is marched by march<>: the same queries, steps and records whichever pass runs it, so a pixel's records
// do not depend on the pass. A pass differs in how pixels map to lanes, where the active list lives and how many
// Gaussians it holds; a pixel that outgrows a pass (kOverflow) is queued for the next one and marched again from its
// start.
//   Tile  march_kernel           one pixel per lane, a workgroup of kMarchBlock lanes per 8x8 quarter of a 16x16 tile;
//                                16 (or 32: march_big) active-list slots per lane in LDS. Overflow: the fallback queue.
//   Wave  march_fallback_kernel  a fallback queue shorter than A.wide_min: one pixel per wave (the step's evaluation
//                                split over the lanes), kActFallback slots in LDS. Overflow: the deep queue.
//   Lane  march_wide_kernel      a longer fallback queue: one pixel per lane, kActWide slots per lane in global
//                                memory. Overflow: the deep queue.
//   Deep  march_deep_kernel      the deep queue: one pixel per wave, kActDeep slots in global memory. Overflow: an error
//                                pixel (NaN, VR_ERR_OVERFLOW).
// The tree a pass's window queries walk is the scene's (march_pass). Its boxes only propose candidates; every decision
// is the exact quadratic.
// ---------------------------------------------------------------------------------------------
enum class MarchPass { Tile, Wave, Lane, Deep };
enum class MarchTree {
    Wide4,    // the 4-wide f16 tree (traverse_wide); a walk past its stack sends the pixel to the next pass
    PairF16,  // the f16 child-pair tree: the deep pass of a scene with a 4-wide tree, where no walk may overflow
    PairF32,  // the f32 child-pair tree, every pass (scenes whose leaf boxes are too small for f16 boxes)
};
constexpr MarchTree deep_tree(MarchTree TREE) { return TREE == MarchTree::Wide4 ? MarchTree::PairF16 : TREE; }

// What follows from the pass, the tree and the tile pass's two choices: BIG, kActBig slots instead of kActFast (a 4-wide
// scene whose frames overflow 16 on >= 5 % of their pixels), and TALL, a kStackSize-entry stack instead of
// kShallowStack (a pair tree deeper than kShallowStack + 1: a child-pair walk pushes at most depth - 1 entries).
struct MarchShape {
    int act;    // active-list capacity
    int stack;  // LDS stack entries per lane
    int deep;   // private-memory stack entries of a 4-wide walk past them
    bool coop;  // one pixel per wave (march)
};
constexpr MarchShape march_shape(MarchPass P, MarchTree TREE, bool BIG, bool TALL) {
    const bool wide = TREE == MarchTree::Wide4;
    if (P == MarchPass::Tile)
        return {BIG ? kActBig : kActFast, wide ? kMarchStack4 : TALL ? kStackSize : kShallowStack, wide ? kMarchDeep : 0, false};
    if (P == MarchPass::Wave) return {kActFallback, kStackSize, 0, true};
    if (P == MarchPass::Lane) return {kActWide, kStackSize, 0, false};
    return {kActDeep, kStackSize, 0, true};
}

// Early-out weight (t_eps > 0). Stopping after step k drops
//   sum_{j>k} T_j sigma_s,j dt (Li_j + Le_j) / (4 pi) + T_end env
// and T_j sigma_s,j dt is not bounded by T alone: the reference's point-sampled estimator can
// weigh a step by sigma_t dt >> 1 inside an opaque blob (C4's blobs carry tau ~ 400 per chord).
// With every Tr <= 1 a record adds at most T sigma_s dt W per channel, W = max_c (sum_l I_lc /
// (4 pi d_l^2) + env_c), and for exponentially falling T the tail sums to <= T_{k+1} W (1 +
// sigma_t,k+1 dt). The ray therefore stops once T (1 + sigma_t,k dt) W <= t_eps: this step's
// point density stands in for the next one's (one step of look-ahead), so a ray inside a dense
// blob takes the extra step that drives T to 0 instead of dropping it.
__device__ __forceinline__ float tail_weight(const RenderArgs& A, float x, float y, float z, float sigma_t) {
    float w0 = fabsf(A.env[0]), w1 = fabsf(A.env[1]), w2 = fabsf(A.env[2]);
    for (int l = 0; l < A.num_lights; ++l) {
        const LightRecord& lr = A.lights[l];
        const float dx = lr.px - x, dy = lr.py - y, dz = lr.pz - z;
        const float s = kInv4Pi / (dx * dx + dy * dy + dz * dz);
        w0 += fabsf(lr.ix) * s;
        w1 += fabsf(lr.iy) * s;
        w2 += fabsf(lr.iz) * s;
    }
    return fmaxf(fmaxf(w0, w1), w2) * (1.0f + sigma_t * A.step_size);
}

// One step k of a pixel's march once its entrants are in `act` (test_integrators.h:202-289): retire
// the Gaussians that exited (b <= t_k), sigma at the position (gmm.h:98-126), the step's optical depth
// (:146-157), a scatter record if sigma_s > 0, T. Returns false once the march ends (T == 0 or the
// early-out). COOP: one pixel per wave (see march).
template <bool S, bool COOP>
__device__ __forceinline__ bool march_step(const RenderArgs& A, const Ray& ray, uint32_t p, int px, int py, int k, float t_k,
                                           ActList& act, float& T, uint32_t& prev, Ctr& c, bool writer) {
    const GaussianRecord* __restrict__ G = A.gauss;
    const float step = A.step_size;
    // retire (b <= t_k); sigma at pos (gmm.h:98-126); the step's optical depth (:146-157)
    const float px_ = ray.ox + t_k * ray.dx;
    const float py_ = ray.oy + t_k * ray.dy;
    const float pz_ = ray.oz + t_k * ray.dz;
    const float t_k1 = t_k + step;  // `t + step_size` (test_integrators.h:286)
    float smu = 0.0f, smua = 0.0f, tau_seg = 0.0f;
    int w = 0;
    bool bnd = false;  // a member's 3-sigma surface passes within the band of the position (kRecBoundary)
    if constexpr (COOP) {
        const int lane = (int)__lane_id();
        for (int i0 = 0; i0 < act.n; i0 += 64) {  // (compaction writes stay below i0 + 64)
            const int i = i0 + lane;
            int j = 0;
            bool surv = false;
            float m = 0.0f, ma = 0.0f, od = 0.0f;
            if (i < act.n) {
                j = act.get(i);
                GRec g = load_rec(G, j);
                Quad q = quad(g, ray);
                float a, b;
                if (intersect(q, a, b) && b > t_k) {
                    surv = true;
                    float ex;
                    m = mu_t(g, px_, py_, pz_, &ex);
                    bnd = bnd || -2.0f * ex > 9.0f - 2.0f * kMemberAmb;
                    ma = m * g.albedo;
                    if (!A.pure) od = optical_depth(g, q, t_k, t_k1);
                }
            }
            bnd = __ballot(bnd) != 0ull;
            for (uint64_t sm = __ballot(surv); sm; sm &= sm - 1) {  // survivors in list order
                const int sl = __ffsll((unsigned long long)sm) - 1;
                act.set(w++, __shfl(j, sl, 64));
                smu += __shfl(m, sl, 64);
                smua += __shfl(ma, sl, 64);
                if (!A.pure) tau_seg += __shfl(od, sl, 64);
                if constexpr (S) {
                    c.v[kCtrMu]++;
                    c.v[kCtrOD]++;
                    c.v[kCtrPrims]++;
                }
            }
        }
    } else {
        for (int i = 0; i < act.n; ++i) {
            int j = act.get(i);
            GRec g = load_rec(G, j);
            Quad q = quad(g, ray);
            float a, b;
            if (!intersect(q, a, b) || b <= t_k) continue;
            act.set(w++, j);
            float ex;
            float m = mu_t(g, px_, py_, pz_, &ex);
            bnd = bnd || -2.0f * ex > 9.0f - 2.0f * kMemberAmb;
            smu += m;
            smua += m * g.albedo;
            if (!A.pure) tau_seg += optical_depth(g, q, t_k, t_k1);
            if constexpr (S) {
                c.v[kCtrMu]++;
                c.v[kCtrOD]++;
                c.v[kCtrPrims]++;
            }
        }
    }
    act.n = w;
    if (w == 0) return true;
    if constexpr (S) c.v[kCtrSteps]++;
    float sigma_s = 0.0f;
    if (smu > 0.0f) {
        float a_mix = smua / smu;
        sigma_s = a_mix * smu;
    }
    if (sigma_s > 0.0f) {  // scattering step -> one record
        uint32_t r, o = 0;
        if constexpr (COOP) {  // one pixel per wave: lane 0 allocates
            uint32_t base = 0;
            if (writer) {
                base = atomicAdd(&A.rec_alloc[0], 1u);
                if (w > kActInline) o = atomicAdd(&A.rec_alloc[1], (uint32_t)w);
            }
            r = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            o = (uint32_t)__builtin_amdgcn_readfirstlane((int)o);
        } else {
            // lanes emitting now share one atomic (this branch is divergent: ballot = them)
            const uint64_t m = __ballot(true);
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            uint32_t base = 0;
            if (__lane_id() == leader) base = atomicAdd(&A.rec_alloc[0], (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
            r = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (w > kActInline) o = atomicAdd(&A.rec_alloc[1], (uint32_t)w);  // rare: the overflow pool
        }
        uint32_t aoff = r * (uint32_t)kActInline;
        bool fits = r < A.rec_cap;
        if (w > kActInline) {  // long active lists go to the overflow pool
            aoff = A.rec_cap * (uint32_t)kActInline + o;
            fits = fits && o + (uint32_t)w <= A.act_ovf_cap;
        }
        if (fits) {
            uint64_t bl = 0;
            for (int i = 0; i < w; ++i) {
                const int j = act.get(i);
                if (COOP ? (i & 63) == (int)__lane_id() : true) A.rec_act[aoff + i] = j;
                bl |= 1ull << (j & 63);
            }
            if (writer) {
                A.rec_pos[r] = make_float4(px_, py_, pz_, T * sigma_s);
                A.rec_meta[r] = make_uint4((uint32_t)px | ((uint32_t)py << 16), (uint32_t)k, aoff,
                                           (uint32_t)w | (bnd && kMemberAmb > 0.0f ? kRecBoundary : 0u));
                A.rec_bloom[r] = bl;
                A.rec_next[r] = kNoRecord;
                if (prev == kNoRecord) A.px_first[p] = r;
                else A.rec_next[prev] = r;
            }
            prev = r;
        } else if (writer) {
            A.rec_alloc[2] = 1u;  // capacity exceeded: the frame is reported and rendered again
            if (r < A.rec_cap) {  // a slot inside [0, nrec) whose active list did not fit the pool:
                // the later stages still read it (the host does not wait for the march), so
                // it must be a valid record, not the previous frame's: an empty one
                A.rec_pos[r] = make_float4(px_, py_, pz_, 0.0f);
                A.rec_meta[r] = make_uint4((uint32_t)px | ((uint32_t)py << 16), (uint32_t)k, 0u, 0u);
                A.rec_bloom[r] = 0ull;
                A.rec_next[r] = kNoRecord;
            }
        }
    }
    if (A.pure) {  // integrator.h:196-198, 259: T *= exp(-sigma_t * step), sigma_t = sigma_a + sigma_s
        float sa = 0.0f, ss = 0.0f;
        if (smu > 0.0f) {
            const float a_mix = smua / smu;
            ss = a_mix * smu;
            sa = (1.0f - a_mix) * smu;
        }
        T *= expf(-(sa + ss) * step);
    } else {
        T *= expf(-tau_seg);
    }
    if (T <= 0.0f) return false;  // exact: nothing after this step can add to L or to T * env
    return !(A.t_eps > 0.0f && T * tail_weight(A, px_, py_, pz_, smu) <= A.t_eps);
}

// One pass: each scattering step allocates its record with a wave-aggregated atomic and links it
// to the pixel's previous record (px_first / rec_next), so a pixel's records are visited in step
// order by accumulate_kernel wherever they landed in memory. Records that do not fit the
// capacity raise rec_alloc[2]; the host then grows the buffers and re-runs the march.
// <P, TREE, S, RAYS, BIG, TALL>: the pass, the tree its window queries walk, the instrumented build (vr_count_work), a ray
// grid, and the tile pass's two choices; capacities and COOP follow (march_shape).
// COOP: the whole wave marches the same pixel (the wave and deep passes: a pixel whose active set
// outgrew the tile pass's slots marches serially for a long time). Every lane runs the same
// queries and keeps its own identical copy of the active list; only the per-step evaluation of the
// active list is split over the lanes (one Gaussian each), its sums and compaction then taken in
// list order through lane broadcasts — the serial loop's operations in its order, so the result is
// bit-identical — and lane 0 writes the records.
// (Measured and not kept, DESIGN.md §3: window queries starting in the subtree holding the window and climbing,
// a fast-form pre-test of the candidates, look-ahead windows over 2-4 steps, a closest-entry query merged with
// the following entrant query, a sorting network in the entrant walk; all bit-identical, all slower at C4.)
// RAYS: the pixel marches its row of the caller's ray grid (GridArgs) instead of the camera's ray; everything after the
// ray is the frame's. An invalid row (grid_ray) ends the pixel at once: NaN transmittance, no records, no error count.
template <MarchPass P, MarchTree TREE, bool S, bool RAYS, bool BIG = false, bool TALL = false>
__device__ int march(const FrameArgs<RAYS>& A, uint32_t p, int px, int py, int* act_base, int* stack, int stride, Ctr& c,
                     int act_stride = -1) {
    static_assert(P == MarchPass::Deep ? TREE != MarchTree::Wide4 : TREE != MarchTree::PairF16,
                  "the deep pass walks a pair tree, and it alone the f16 one (deep_tree)");
    static_assert(P == MarchPass::Tile ? !(BIG && TREE != MarchTree::Wide4) && !(TALL && TREE == MarchTree::Wide4) : !BIG && !TALL,
                  "BIG: the tile pass on the 4-wide tree; TALL: the tile pass on a pair tree");
    constexpr MarchShape kShape = march_shape(P, TREE, BIG, TALL);
    constexpr int ACT = kShape.act, CAP = kShape.stack, DEEP = kShape.deep;
    constexpr bool COOP = kShape.coop, W = TREE == MarchTree::Wide4;
    const bool writer = !COOP || __lane_id() == 0u;  // COOP: lane 0 writes the pixel's records
    bool ray_ok = true;
    const Ray ray = pixel_ray<RAYS>(A, px, py, ray_ok);
    if constexpr (RAYS) {
        if (!ray_ok) {
            if (writer) {
                A.px_first[p] = kNoRecord;
                A.px_T[p] = __builtin_nanf("");
            }
            return kOK;
        }
    }
    const GaussianRecord* __restrict__ G = A.gauss;
    const float* __restrict__ ts = A.tsteps;
    const int nts = A.num_tsteps;
    const float step = A.step_size;
    float T = 1.0f;
    uint32_t prev = kNoRecord;  // this pixel's last record
    if (writer) A.px_first[p] = kNoRecord;
    ActList act{act_base, act_stride < 0 ? stride : act_stride, 0, 0};
    auto walk = [&](auto prune, auto leaf) -> bool {
        if constexpr (W) {
            return traverse_wide<CAP, decltype(prune), decltype(leaf), NodeCount<S>, true, DEEP>(A, ray, stack, stride, prune, leaf,
                                                                                                NodeCount<S>{&c});
        } else {
            traverse<TREE == MarchTree::PairF16>(A, ray, stack, stride, prune, leaf, NodeCount<S>{&c});
            return true;
        }
    };
    // the entrants query collects every entry of (t_lo, t_k] whatever the visit order: no sorting network
    auto walk_any = [&](auto prune, auto leaf) -> bool {
        if constexpr (W) {
            return traverse_wide<CAP, decltype(prune), decltype(leaf), NodeCount<S>, false, DEEP>(A, ray, stack, stride, prune, leaf,
                                                                                                    NodeCount<S>{&c});
        } else {
            return walk(prune, leaf);
        }
    };
    int kq = 0;
    if (A.num_prims > 0) {
        for (;;) {
            float t_lo = (kq == 0) ? -1.0f : ts[kq - 1];
            int k;
            if (act.n == 0) {  // closest entry strictly after t_lo
                if constexpr (S) c.v[kCtrPrimQueries]++;
                float best = INFINITY;
                auto prune_c = [&](float tmin, float tmax) {
                    return tmax >= t_lo - kTPad * (1.0f + fabsf(t_lo)) && tmin <= best + kTPad * (1.0f + best);
                };
                auto leaf_c = [&](uint32_t first, uint32_t count) {
                    for (uint32_t j = first; j < first + count; ++j) {
                        if constexpr (S) c.v[kCtrPrims]++;
                        GRec g = load_rec(G, j);
                        Quad q = quad(g, ray);
                        float a, b;
                        if (!intersect(q, a, b) || !(a > t_lo)) continue;
                        if (a < best) best = a;
                    }
                    return true;
                };
                if (!walk(prune_c, leaf_c)) return kOverflow;
                if (best == INFINITY) break;
                k = kfirst(ts, nts, step, best);
                // No entry lies in (t_lo, best) and ts[k - 1] < best: the step's entrant window (t_lo, t_k] holds
                // exactly the entries of (ts[k - 1], t_k]. The short window keeps the query local to the step
                // (from t_lo = -1 the first query of every pixel walked every box along [0, t_k]). Same set.
                if (k > kq) t_lo = ts[k - 1];
            } else {
                k = kq;
            }
            if (k >= nts - 1) return kError;  // step table too short (host sizes it from scene bounds)
            const float t_k = ts[k];
            bool ovf = false;
            // entrants: t_lo < a <= t_k and still inside at t_k (b > t_k)
            if constexpr (S) c.v[kCtrPrimQueries]++;
            auto prune_w = [&](float tmin, float tmax) {
                return tmax >= t_lo - kTPad * (1.0f + fabsf(t_lo)) && tmin <= t_k + kTPad * (1.0f + t_k);
            };
            const bool ok = walk_any(
                prune_w,
                [&](uint32_t first, uint32_t count) {
                    for (uint32_t j = first; j < first + count; ++j) {
                        if constexpr (S) c.v[kCtrPrims]++;
                        GRec g = load_rec(G, j);
                        Quad q = quad(g, ray);
                        float a, b;
                        if (!intersect(q, a, b) || !(a > t_lo) || !(a <= t_k)) continue;
                        if (!(b > t_k)) continue;
                        if (act.n >= ACT) {
                            ovf = true;
                            continue;
                        }
                        // sorted insert by scene index (gmm.h:98-126 sums in that order): a step's sums do not
                        // depend on how the tree's builder ordered the records
                        const uint32_t key = A.gauss_order[j];
                        int i = act.n;
                        while (i > 0 && A.gauss_order[act.get(i - 1)] > key) {
                            act.set(i, act.get(i - 1));
                            --i;
                        }
                        act.set(i, (int)j);
                        act.n++;
                    }
                    return true;
                });
            if (ovf || !ok) return kOverflow;
            kq = k + 1;
            if (!march_step<S, COOP>(A, ray, p, px, py, k, t_k, act, T, prev, c, writer)) break;
        }
    }
    if (writer) A.px_T[p] = T;
    if constexpr (S) c.v[kCtrPixels]++;
    return kOK;
}

__device__ __forceinline__ void mark_error(const RenderArgs& A, uint32_t p) {
    atomicAdd(A.counters, 1u);
    A.px_T[p] = __builtin_nanf("");
}

// A pixel that overflowed a pass is marched again from its start by the next pass, which relinks it;
// the records this pass already wrote for it are unreachable. Their weight T sigma_s (rec_pos.w, >= 0 for
// every live record) is set to the sentinel -1 so the secondary stage starts none of their rays (sec_init).
constexpr float kOrphanWeight = -1.0f;  // rec_pos.w of an orphaned record (a live record's T sigma_s is >= 0)
__device__ __forceinline__ void orphan_records(const RenderArgs& A, uint32_t p) {
    for (uint32_t r = A.px_first[p]; r != kNoRecord && r < A.rec_cap; r = A.rec_next[r])
        reinterpret_cast<float*>(A.rec_pos + r)[3] = kOrphanWeight;
}

// The tile pass. LDS per lane: (active-list slots + stack entries) * 4 B.
template <MarchTree TREE, bool S, bool RAYS, bool BIG, bool TALL>
__global__ __launch_bounds__(kMarchBlock) void march_kernel(FrameArgs<RAYS> A) {
    constexpr int BLOCK = kMarchBlock;
    constexpr MarchShape kShape = march_shape(MarchPass::Tile, TREE, BIG, TALL);
    __shared__ int s_act[kShape.act * BLOCK];
    __shared__ int s_stack[kShape.stack * BLOCK];
    // A workgroup is one 16x16 tile (BLOCK 256) or one of its 8x8 quarters (BLOCK 64: four times as
    // many, shorter workgroups, so the frame's last ones leave a shorter tail). Lanes never share LDS.
    constexpr uint32_t kParts = 256u / BLOCK;
    const uint32_t q = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t tile_local = q / kParts;
    const int tid = (int)((q % kParts) * BLOCK + threadIdx.x);  // lane within the tile
    const uint32_t p = tile_local * 256u + (uint32_t)tid;
    int lx, ly, x, y;
    tile_pixel(A, tile_local, tid, lx, ly, x, y);
    Ctr c{};
    int st = kOK;
    if (x < (int)A.width && y < (int)A.height) {
        st = march<MarchPass::Tile, TREE, S, RAYS, BIG, TALL>(A, p, x, y, s_act + threadIdx.x, s_stack + threadIdx.x, BLOCK, c);
    } else {
        A.px_first[p] = kNoRecord;
        A.px_T[p] = 0.0f;
    }
    if constexpr (S) flush_counters(A.work, c);
    if (st == kOverflow) {
        orphan_records(A, p);
        uint32_t slot = atomicAdd(A.queue, 1u);
        if (slot < A.queue_cap) A.queue[1 + slot] = p;
        else mark_error(A, p);
    } else if (st == kError) {
        mark_error(A, p);
    }
}

// The wave pass marches one pixel per wave (march's COOP): a pixel lands here because its active
// set is large, and its serial march was the tail of the whole march stage (~1 ms at C4, also for a
// 1/8 multi-GPU share).
template <MarchTree TREE, bool S, bool RAYS>
__global__ __launch_bounds__(kWaveBlock) void march_fallback_kernel(FrameArgs<RAYS> A) {
    static_assert(kWaveBlock == 64, "one pixel per wave");
    constexpr int BLOCK = kWaveBlock;
    __shared__ int s_act[kActFallback * BLOCK];
    __shared__ int s_stack[kStackSize * BLOCK];
    const int tid = threadIdx.x;
    const uint32_t n = min(A.queue[0], A.queue_cap);
    if (n >= A.wide_min) return;  // a long queue: march_wide_kernel takes it (one pixel per lane)
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const uint32_t p = A.queue[1 + q];
        int lx, ly, x, y;
        tile_pixel(A, p >> 8, (int)(p & 255u), lx, ly, x, y);
        Ctr c{};
        // (Wide4: half the dependent node fetches of the pair tree on a single pixel's serial queries; a walk past
        // the kStackSize stack goes to the deep pass)
        int st = march<MarchPass::Wave, TREE, S, RAYS>(A, p, x, y, s_act + tid, s_stack + tid, BLOCK, c);  // re-links px_first
        if (tid != 0) continue;
        if constexpr (S)
            for (int i = 0; i < kNumCtr; ++i) atomicAdd(A.work + i, (unsigned long long)c.v[i]);
        if (st == kOverflow) {  // more than kActFallback Gaussians active at one step: the deep pass
            orphan_records(A, p);
            const uint32_t slot = atomicAdd(A.deepq, 1u);
            if (slot < A.deepq_cap) A.deepq[1 + slot] = p;
            else mark_error(A, p);
        } else if (st != kOK) {
            mark_error(A, p);
        }
    }
}

// A long fallback queue (translucent scenes with many overlapping Gaussians: C2 sends most pixels here)
// one pixel per lane: the main kernel's march with kActWide active-list slots per lane in global memory
// ([slot][thread] rows, coalesced over a wave's lanes) instead of 16 in LDS. One wave per pixel
// (march_fallback_kernel) shortens a single pixel's march but runs the queue 64x narrower; it keeps
// queues shorter than A.wide_min (C4: 833 pixels). Same march<> operations as every other pass, so
// a pixel's records do not depend on which pass marched it. Overflow (more than kActWide active, or a
// 4-wide walk past its stack): the deep pass.
template <MarchTree TREE, bool S, bool RAYS>
__global__ __launch_bounds__(kWideBlock) void march_wide_kernel(FrameArgs<RAYS> A) {
    __shared__ int s_stack[kStackSize * kWideBlock];
    const int tid = threadIdx.x;
    const uint32_t gt = blockIdx.x * kWideBlock + tid, nthreads = gridDim.x * kWideBlock;
    const uint32_t n = min(A.queue[0], A.queue_cap);
    if (n < A.wide_min) return;
    Ctr c{};
    for (uint32_t q = gt; q < n; q += nthreads) {
        const uint32_t p = A.queue[1 + q];
        int lx, ly, x, y;
        tile_pixel(A, p >> 8, (int)(p & 255u), lx, ly, x, y);
        const int st = march<MarchPass::Lane, TREE, S, RAYS>(A, p, x, y, A.wide_act + gt, s_stack + tid, kWideBlock, c, (int)nthreads);
        if (st == kOverflow) {
            orphan_records(A, p);
            const uint32_t slot = atomicAdd(A.deepq, 1u);
            if (slot < A.deepq_cap) A.deepq[1 + slot] = p;
            else mark_error(A, p);
        } else if (st != kOK) {
            mark_error(A, p);
        }
    }
    if constexpr (S) flush_counters(A.work, c);
}

// Pixels whose active set outgrew the fallback's 64 LDS slots: the same march with the active list in
// global memory (kActDeep slots per lane, [slot][thread] rows, one pixel per wave).
// Only an active set past kActDeep, Gaussians overlapping one point, fails (NaN, VR_ERR_OVERFLOW).
// TREE: a child-pair tree (deep_tree).
template <MarchTree TREE, bool S, bool RAYS>
__global__ __launch_bounds__(kDeepBlock) void march_deep_kernel(FrameArgs<RAYS> A) {
    static_assert(kDeepBlock == 64, "one pixel per wave");
    __shared__ int s_stack[kStackSize * kDeepBlock];
    const int tid = threadIdx.x;
    const uint32_t gt = blockIdx.x * kDeepBlock + tid, nthreads = gridDim.x * kDeepBlock;
    const uint32_t n = min(A.deepq[0], A.deepq_cap);
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const uint32_t p = A.deepq[1 + q];
        int lx, ly, x, y;
        tile_pixel(A, p >> 8, (int)(p & 255u), lx, ly, x, y);
        Ctr c{};
        const int st = march<MarchPass::Deep, TREE, S, RAYS>(A, p, x, y, A.deep_act + gt, s_stack + tid, kDeepBlock, c, (int)nthreads);
        if (tid != 0) continue;
        if constexpr (S)
            for (int i = 0; i < kNumCtr; ++i) atomicAdd(A.work + i, (unsigned long long)c.v[i]);
        if (st != kOK) mark_error(A, p);
    }
}

// ---------------------------------------------------------------------------------------------
// Stage 1, binned variant (VR_OPT_MARCH_BINNED; A/B against the BVH window queries):
// every record is binned to the 16x16 tiles its 3.15-sigma box can project onto, by a depth bucket of
// a lower bound of the entry distance of the tile's pixel rays; a quarter-tile wave then streams its
// tile's entries bucket by bucket (wave-uniform: scalar loads of index and record), tests each against
// every lane's ray with the exact intersect, keeps the hits that have not entered yet in a per-lane
// pending list sorted by entry distance, and marches every step that lies before the next bucket's
// lower bound (no later entry can enter at or before it). The active lists, steps and records are
// those of march(): the same intersect decides every entry, the same march_step evaluates.
// ---------------------------------------------------------------------------------------------
constexpr int kPendCap = VR_BIN_PEND;  // pending entries per lane (more: the pixel re-runs in march_fallback_kernel)
constexpr int kBinAct = 16;      // active Gaussians per lane (as march_kernel's)

// The pixel rectangle (inclusive, clamped to the frame) that the box [lo, hi] can project onto, and
// false if it projects onto nothing; all = true when the box reaches the pinhole's side of the image
// plane (then every tile).
__device__ __forceinline__ bool bin_rect(const RenderArgs& A, const float* lo, const float* hi, int& x0, int& x1, int& y0,
                                         int& y1) {
    const float* R = A.cam_right;
    const float* U = A.cam_up;
    const float n0 = R[1] * U[2] - R[2] * U[1], n1 = R[2] * U[0] - R[0] * U[2], n2 = R[0] * U[1] - R[1] * U[0];
    const float rr = R[0] * R[0] + R[1] * R[1] + R[2] * R[2], uu = U[0] * U[0] + U[1] * U[1] + U[2] * U[2];
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    bool all = false;
    for (int c = 0; c < 8; ++c) {
        const float X[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
        float o[3];
        if (A.cam_type == 0) {  // the ray from o passes through the pinhole P: o = P + s (X - P) on the plane
            const float* P = A.cam_pinhole;
            const float pn = (P[0] - A.cam_pos[0]) * n0 + (P[1] - A.cam_pos[1]) * n1 + (P[2] - A.cam_pos[2]) * n2;
            const float xn = (X[0] - P[0]) * n0 + (X[1] - P[1]) * n1 + (X[2] - P[2]) * n2;
            if (!(xn * pn > 1e-6f * fabsf(pn) * (fabsf(pn) + fabsf(xn)))) {  // not strictly beyond the pinhole
                all = true;
                break;
            }
            const float sc = -pn / xn;
            for (int k = 0; k < 3; ++k) o[k] = P[k] + sc * (X[k] - P[k]);
        } else {  // orthographic: along the view direction onto the plane
            const float* V = A.cam_view;
            const float vn = V[0] * n0 + V[1] * n1 + V[2] * n2;
            if (!(fabsf(vn) > 0.0f)) {
                all = true;
                break;
            }
            const float lam = ((X[0] - A.cam_pos[0]) * n0 + (X[1] - A.cam_pos[1]) * n1 + (X[2] - A.cam_pos[2]) * n2) / vn;
            for (int k = 0; k < 3; ++k) o[k] = X[k] - lam * V[k];
        }
        const float d0 = o[0] - A.cam_pos[0], d1 = o[1] - A.cam_pos[1], d2 = o[2] - A.cam_pos[2];
        const float u = (d0 * R[0] + d1 * R[1] + d2 * R[2]) / rr, v = (d0 * U[0] + d1 * U[1] + d2 * U[2]) / uu;
        umin = fminf(umin, u);
        umax = fmaxf(umax, u);
        vmin = fminf(vmin, v);
        vmax = fmaxf(vmax, v);
    }
    const float W = (float)A.width, H = (float)A.height;
    float fx0, fx1, fy0, fy1;
    if (all) {
        fx0 = fy0 = 0.0f;
        fx1 = W;
        fy1 = H;
    } else if (A.cam_type == 0) {  // u = 1 - 2 (x + .5) / W, v = 2 (y + .5) / H - 1
        fx0 = (1.0f - umax) * 0.5f * W - 0.5f;
        fx1 = (1.0f - umin) * 0.5f * W - 0.5f;
        fy0 = (vmin + 1.0f) * 0.5f * H - 0.5f;
        fy1 = (vmax + 1.0f) * 0.5f * H - 0.5f;
    } else {  // u = 2 (x + .5) / W - 1, v = 1 - 2 (y + .5) / H
        fx0 = (umin + 1.0f) * 0.5f * W - 0.5f;
        fx1 = (umax + 1.0f) * 0.5f * W - 0.5f;
        fy0 = (1.0f - vmax) * 0.5f * H - 0.5f;
        fy1 = (1.0f - vmin) * 0.5f * H - 0.5f;
    }
    // two pixels of slack for rounding (directions, the box's own projection)
    x0 = (int)fmaxf(floorf(fx0) - 2.0f, 0.0f);
    y0 = (int)fmaxf(floorf(fy0) - 2.0f, 0.0f);
    x1 = (int)fminf(ceilf(fx1) + 2.0f, W - 1.0f);
    y1 = (int)fminf(ceilf(fy1) + 2.0f, H - 1.0f);
    return fx1 + 2.0f >= 0.0f && fy1 + 2.0f >= 0.0f && fx0 - 2.0f <= W && fy0 - 2.0f <= H;
}

// 3.15-sigma box of record j (Sigma = M^-1 in double; the intersect's 3-sigma ellipsoid of the f32 M
// lies inside with a 5 % margin, as the BVH boxes).
__device__ __forceinline__ void bin_box(const GaussianRecord& g, float* lo, float* hi) {
    const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
    const double c00 = m11 * m22 - m12 * m12, c11 = m00 * m22 - m02 * m02, c22 = m00 * m11 - m01 * m01;
    const double det = m00 * c00 - m01 * (m01 * m22 - m12 * m02) + m02 * (m01 * m12 - m11 * m02);
    const double s[3] = {c00 / det, c11 / det, c22 / det};
    const float m[3] = {g.mx, g.my, g.mz};
    for (int k = 0; k < 3; ++k) {
        const float e = (float)(3.15 * sqrt(fmax(s[k], 0.0)));
        const bool ok = det > 0.0 && e == e;
        lo[k] = ok ? m[k] - e : -INFINITY;
        hi[k] = ok ? m[k] + e : INFINITY;
    }
}

// Tile tile_local (of this call's strided tile set) if global tile (tx, ty) belongs to it, else -1.
__device__ __forceinline__ int local_tile(const RenderArgs& A, uint32_t tx, uint32_t ty) {
    const uint32_t g = ty * A.tiles_x + tx;
    if (g < A.first_tile) return -1;
    const uint32_t d = g - A.first_tile;
    if (d % A.tile_stride) return -1;
    const uint32_t t = d / A.tile_stride;
    return t < A.num_tiles ? (int)t : -1;
}

// Lower bound of the entry distance into box [lo, hi] of every pixel ray of global tile (tx, ty): the
// distance from the tile's central ray origin less the half diagonal of its origins (|d| = 1, so a
// ray's t is the distance from its origin), less a relative margin for rounding.
__device__ __forceinline__ float bin_key(const RenderArgs& A, uint32_t tx, uint32_t ty, const float* lo, const float* hi,
                                         float hd) {
    const float cx = (float)(tx * kTile) + 0.5f * kTile, cy = (float)(ty * kTile) + 0.5f * kTile;
    const float uvx = cx / (float)A.width, uvy = cy / (float)A.height;
    const float u = A.cam_type == 0 ? 1.0f - 2.0f * uvx : 2.0f * uvx - 1.0f;
    const float v = A.cam_type == 0 ? 2.0f * uvy - 1.0f : 1.0f - 2.0f * uvy;
    float d2 = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float o = A.cam_pos[k] + u * A.cam_right[k] + v * A.cam_up[k];
        const float e = fmaxf(fmaxf(lo[k] - o, o - hi[k]), 0.0f);
        d2 += e * e;
    }
    return fmaxf((sqrtf(d2) - hd) * (1.0f - 1e-4f) - 1e-4f, 0.0f);
}

__device__ __forceinline__ float bin_half_diag(const RenderArgs& A) {
    const float* R = A.cam_right;
    const float* U = A.cam_up;
    const float du = 2.0f * kTile / (float)A.width * sqrtf(R[0] * R[0] + R[1] * R[1] + R[2] * R[2]);
    const float dv = 2.0f * kTile / (float)A.height * sqrtf(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
    return 0.5f * sqrtf(du * du + dv * dv);
}

// EMIT = false: count the entries of every bin; true: write them at bin_off + a cursor per bin.
template <bool EMIT>
__global__ __launch_bounds__(256) void bin_kernel(RenderArgs A) {
    const float hd = bin_half_diag(A);
    const uint32_t nb = A.bin_nb;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < (uint32_t)A.num_prims; j += gridDim.x * 256u) {
        const GaussianRecord g = A.gauss[j];
        float lo[3], hi[3];
        bin_box(g, lo, hi);
        int x0, x1, y0, y1;
        if (!bin_rect(A, lo, hi, x0, x1, y0, y1)) continue;
        for (uint32_t ty = (uint32_t)y0 / kTile; ty <= (uint32_t)y1 / kTile; ++ty)
            for (uint32_t tx = (uint32_t)x0 / kTile; tx <= (uint32_t)x1 / kTile; ++tx) {
                const int t = local_tile(A, tx, ty);
                if (t < 0) continue;
                const uint32_t b = min(nb - 1u, (uint32_t)(bin_key(A, tx, ty, lo, hi, hd) / A.bin_dz));
                const uint32_t bin = (uint32_t)t * nb + b;
                if constexpr (EMIT) {
                    const uint32_t pos = A.bin_off[bin] + atomicAdd(&A.bin_cnt[bin], 1u);
                    A.bin_out[pos] = j;
                } else {
                    atomicAdd(&A.bin_cnt[bin], 1u);
                }
            }
    }
}

// The binned march of one quarter tile (a wave, one lane per pixel). Returns the per-lane status.
template <bool S>
__global__ __launch_bounds__(64) void march_binned_kernel(RenderArgs A) {
    __shared__ float s_pa[kPendCap * 64];  // pending entries, sorted by entry distance, largest first
    __shared__ int s_pj[kPendCap * 64];
    __shared__ int s_act[kBinAct * 64];
    const uint32_t q = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t tile_local = q >> 2;
    const int lane = (int)threadIdx.x;
    const int tid = (int)((q & 3u) * 64u) + lane;
    const uint32_t p = tile_local * 256u + (uint32_t)tid;
    int lx, ly, x, y;
    tile_pixel(A, tile_local, tid, lx, ly, x, y);
    Ctr c{};
    const bool valid = x < (int)A.width && y < (int)A.height;
    const Ray ray = primary_ray(A, x, y);
    float* pa = s_pa + lane;
    int* pj = s_pj + lane;
    ActList act{s_act + lane, 64, 0, 0};
    float T = 1.0f;
    uint32_t prev = kNoRecord;
    int np = 0, kq = 0, st = kOK;
    float t_lo = -1.0f;
    bool done = !valid;
    if (valid) A.px_first[p] = kNoRecord;
    const float* __restrict__ ts = A.tsteps;
    const int nts = A.num_tsteps;
    // every step before `bound` (no entry of a later bucket can enter at or before it)
    auto march_to = [&](float bound) {
        for (;;) {
            int k;
            if (act.n == 0) {
                if (np == 0) return;
                k = kfirst(ts, nts, A.step_size, pa[(np - 1) * 64]);  // the closest entry after t_lo
            } else {
                k = kq;
            }
            if (k >= nts - 1) {
                st = kError;
                done = true;
                return;
            }
            const float t_k = ts[k];
            if (!(t_k < bound)) return;
            while (np > 0 && pa[(np - 1) * 64] <= t_k) {  // entrants: entered at or before t_k, still inside
                const int j = pj[--np * 64];
                if constexpr (S) c.v[kCtrPrims]++;
                float a, b;
                if (!intersect(quad(load_rec(A.gauss, j), ray), a, b) || !(b > t_k)) continue;
                if (act.n >= kBinAct) {
                    if constexpr (S) c.v[kCtrSecRays]++;  // (instrumented build: overflow causes)
                    st = kOverflow;
                    done = true;
                    return;
                }
                const uint32_t key = A.gauss_order[j];  // sorted insert (scene-index order, gmm.h:98-126)
                int i = act.n;
                while (i > 0 && A.gauss_order[act.get(i - 1)] > key) {
                    act.set(i, act.get(i - 1));
                    --i;
                }
                act.set(i, j);
                act.n++;
            }
            kq = k + 1;
            t_lo = t_k;
            if (!march_step<S, false>(A, ray, p, x, y, k, t_k, act, T, prev, c, true)) {
                done = true;
                return;
            }
        }
    };
    if (A.num_prims > 0) {
        const uint32_t nb = A.bin_nb;
        const uint32_t* __restrict__ off = A.bin_off + tile_local * nb;
        for (uint32_t b = 0;; ++b) {  // wave-uniform: bucket by bucket
            while (b < nb && off[b] == off[b + 1]) ++b;  // (empty buckets)
            // every entry of bucket b on enters at or after b * dz: march the steps before it first
            if (!done) march_to(b < nb ? (float)b * A.bin_dz : INFINITY);
            if (b >= nb || __ballot(!done) == 0ull) break;
            for (uint32_t pos = off[b]; pos < off[b + 1]; ++pos) {
                const int j = (int)A.bin_ent[pos];
                if (!done) {
                    if constexpr (S) c.v[kCtrPrims]++;
                    float ta, tb;
                    if (intersect(quad(load_rec(A.gauss, j), ray), ta, tb)) {
                        if (!(ta > t_lo)) {  // (a key below its bound: the exact BVH march re-runs the pixel)
                            if constexpr (S) c.v[kCtrPrimQueries]++;
                            st = kOverflow;
                            done = true;
                        } else if (np >= kPendCap) {
                            if constexpr (S) c.v[kCtrNodes]++;
                            st = kOverflow;
                            done = true;
                        } else {
                            int i = np++;  // sorted insert, largest entry distance first
                            while (i > 0 && pa[(i - 1) * 64] < ta) {
                                pa[i * 64] = pa[(i - 1) * 64];
                                pj[i * 64] = pj[(i - 1) * 64];
                                --i;
                            }
                            pa[i * 64] = ta;
                            pj[i * 64] = j;
                        }
                    }
                }
            }
        }
    }
    if (valid && st == kOK) A.px_T[p] = T;
    if constexpr (S) {
        c.v[kCtrPixels] += valid ? 1u : 0u;
        flush_counters(A.work, c);
    }
    if (!valid) {
        A.px_first[p] = kNoRecord;
        A.px_T[p] = 0.0f;
    } else if (st == kOverflow) {
        orphan_records(A, p);
        uint32_t slot = atomicAdd(A.queue, 1u);
        if (slot < A.queue_cap) A.queue[1 + slot] = p;
        else mark_error(A, p);
    } else if (st == kError) {
        mark_error(A, p);
    }
}

}  // namespace dev

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
hipError_t gauss_bin(const RenderArgs& A, bool emit, hipStream_t stream) {
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)A.num_prims + 255) / 256, 16384);
    if (emit) hipLaunchKernelGGL(dev::bin_kernel<true>, dim3(std::max(grid, 1u)), dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(dev::bin_kernel<false>, dim3(std::max(grid, 1u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t gauss_bin_scan(const uint32_t* cnt, uint32_t* off, uint32_t n, void* tmp, size_t& tmp_bytes, hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, off, (int)n, stream);
}

// RAYS: a ray grid (never binned: the bins are built from the camera's tile frusta).
template <dev::MarchTree TREE, bool S, bool RAYS, bool BIG, bool TALL>
static void tile_launch(const FrameArgs<RAYS>& A, hipStream_t stream) {
    hipLaunchKernelGGL((dev::march_kernel<TREE, S, RAYS, BIG, TALL>), dim3(A.num_tiles * (256 / kMarchBlock)), dim3(kMarchBlock), 0, stream, A);
}

// The four passes of a frame on the scene's tree TREE.
template <dev::MarchTree TREE, bool S, bool RAYS>
static hipError_t march_passes(const FrameArgs<RAYS>& A, hipStream_t stream) {
    if (!RAYS && A.bin_ent != nullptr) {  // binned march (its overflowing pixels re-run in the BVH fallback below)
        hipLaunchKernelGGL((dev::march_binned_kernel<S>), dim3(A.num_tiles * 4), dim3(64), 0, stream, static_cast<const RenderArgs&>(A));
    } else if constexpr (TREE == dev::MarchTree::Wide4) {  // a query that could overflow the stack goes to the fallback
        // march_big: translucent, densely overlapping scenes (C2): fewer pixels overflow, and their records come from
        // coherent quarter tiles instead of the fallback queue
        if (A.march_big) tile_launch<TREE, S, RAYS, true, false>(A, stream);
        else tile_launch<TREE, S, RAYS, false, false>(A, stream);
    } else {
        if (A.bvh_depth <= kShallowStack + 1) tile_launch<TREE, S, RAYS, false, false>(A, stream);
        else tile_launch<TREE, S, RAYS, false, true>(A, stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (exactly one of the wave and lane passes takes the fallback queue, by its length)
    hipLaunchKernelGGL((dev::march_fallback_kernel<TREE, S, RAYS>), dim3(1024), dim3(kWaveBlock), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((dev::march_wide_kernel<TREE, S, RAYS>), dim3(kWideThreads / kWideBlock), dim3(kWideBlock), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((dev::march_deep_kernel<dev::deep_tree(TREE), S, RAYS>), dim3(kDeepThreads / kDeepBlock), dim3(kDeepBlock), 0, stream, A);
    return hipGetLastError();
}

// The scene's tree: hnodes4 alone says whether it has its f16 trees (the invariant stated in fill_scene_args,
// vr_frame.cpp), as in secondary_launch.
template <bool S, bool RAYS = false>
static hipError_t march_pass(const FrameArgs<RAYS>& A, hipStream_t stream) {
    return A.hnodes4 != nullptr ? march_passes<dev::MarchTree::Wide4, S, RAYS>(A, stream)
                                : march_passes<dev::MarchTree::PairF32, S, RAYS>(A, stream);
}

hipError_t gauss_march(const RenderArgs& A, hipStream_t stream, bool stats, const GridSrc* grid) {
    if (grid != nullptr) {  // a ray grid (no instrumented build: vr_count_work takes a camera)
        if (stats) return hipErrorInvalidValue;
        return march_pass<false, true>(GridArgs{A, *grid}, stream);
    }
    return stats ? march_pass<true>(A, stream) : march_pass<false>(A, stream);
}

}  // namespace vr
