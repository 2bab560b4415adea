// Stage 2 of the RayMarchingGaussians pipeline (vr_gauss_common.h): every record's start subtree and environment
// ray order, the persistent kernel that traces the secondary rays, and the fix-up of its chord-band rays, with
// the launcher gauss_secondary. The rays it queues for the exact slow path: vr_gauss_exact.hip.
#include <cstdio>
#include <type_traits>

#include "vr_gauss_common.h"

// Tuning knobs of this unit (A/B builds: tools/ab_build.sh NAME vr_gauss_secondary "-DVR_...=...").
// Scheduling constants of the persistent kernel (tuned on C4): refill once this many
// lanes are idle (amortises sec_init), and up to this many NODE / PRIM steps per lane per iteration
// (amortises the per-iteration ballots and decisions).
#ifndef VR_WW_REFILL
#define VR_WW_REFILL 24
#endif
#ifndef VR_WW_NODE_STEPS
#define VR_WW_NODE_STEPS 6
#endif
#ifndef VR_WW_PRIM_STEPS
#define VR_WW_PRIM_STEPS 3  // A/B round 4 (tight tree, C4 secondary): 3: 77.1, 4: 77.1-77.3, 5: 77.6-78.0, 7: 85.7 ms;
                            // round 6 (with PRIM bias 85, tools/gpu_r6n.sh): 3 + 85 %: 78.0 vs 4 + 70 %: 78.4-78.5 ms
#endif
#ifndef VR_WW_PRIM_UNROLL
#define VR_WW_PRIM_UNROLL 5  // unroll of the PRIM iteration's step loop (A/B: code size vs. scheduling)
#endif
#ifndef VR_WW_NODE_UNROLL
#define VR_WW_NODE_UNROLL 1
#endif
#ifndef VR_WW_PRIM_BIAS
#define VR_WW_PRIM_BIAS 85  // a PRIM iteration needs this many % of the lanes a NODE iteration could use (A/B, round 6:
                            // 60 / 70 / 85 / 100 % -> 79.1 / 78.5 / 78.0-78.3 / 78.7 ms at 4 PRIM steps)
#endif
#ifndef VR_WW_SPLIT_CPW
#define VR_WW_SPLIT_CPW 32  // chunks per resident wave below which claim units get shorter (A/B)
#endif
#ifndef VR_WW_STACK
#define VR_WW_STACK 14  // LDS traversal-stack entries per lane (deeper ones spill to the global overflow)
#endif
#ifndef VR_WW_WAVES
#define VR_WW_WAVES 7  // waves per SIMD of the whitened form (launch bounds: 72 VGPRs at 7; A/B at C4: 7 + 14-entry stack
                       // 95.6 ms, 6 + 18 99.2 ms)
#endif
#ifndef VR_WW_QCAP
#define VR_WW_QCAP 9  // leaf queue of the persistent kernel: the head entry + an LDS ring of QCAP - 1 (1 + 2^k)
#endif

namespace vr {
namespace dev {

// ---------------------------------------------------------------------------------------------
// The persistent kernel (secondary_ww_kernel): "while-while" tracing of all secondary rays with postponed leaves.
//
// Secondary rays have very uneven lengths (the optical-depth cut-off ends a ray after a few dense hits, a ray through
// empty space walks many nodes), so one ray per lane per launch would leave most of a wave idle behind its slowest
// lane. One resident grid traces them all instead; each lane holds one ray at a time.
//   * Claim units. The rays are handed out by record chunk (neighbouring records, light rays first, then the
//     environment rays in env_order_kernel's direction order, so a wave's rays stay coherent). A wave claims the next
//     unit with one atomic on A.ray_next: a whole chunk, or 1/2, 1/4, 1/8 of one when the launch has few chunks per
//     resident wave (VR_WW_SPLIT_CPW). Its lanes take consecutive rays of the unit as they fall idle.
//   * Refill and batched completions. Once VR_WW_REFILL lanes are idle the wave refills them in one pass: the rays
//     completed since the last refill write their Tr (sec_finish), then every idle lane starts its next ray (sec_init,
//     list_begin). A completed lane idles until then.
//   * NODE and PRIM iterations. A wave never runs the node code and the primitive code in the same iteration. In a
//     NODE iteration the lanes with room in their leaf queue take up to VR_WW_NODE_STEPS tree steps (sec_node4v /
//     sec_node); leaf children are queued, not tested. In a PRIM iteration the lanes with a list member or a queued
//     leaf test up to VR_WW_PRIM_STEPS primitives. The kind is whichever more lanes can use (VR_WW_PRIM_BIAS), never one
//     that no lane can use. So a wave neither waits for its longest ray nor stalls its walking lanes on a leaf visit.
// Light rays whose result depends on the first event past the light (a Gaussian straddling the light, or a
// pre-activated Gaussian the ray misses through rounding) are rare; they go to a queue served by
// secondary_slow_kernel's exact three-pass light_transmittance.
//
// The kernel's variants, <S, F, T>: S is the instrumented build (vr_count_work): the same schedule, counting its own
// work. The form F of the primitive test and the tree T the walk reads are the scene's (secondary_launch).
// ---------------------------------------------------------------------------------------------
enum class SecForm {
    Whitened,  // RayMarchingGaussians on the whitened records (A.wrec): the credit scheme, no membership lookup
    MForm,     // RayMarchingGaussians on the records' M forms (a scene with a non-positive-definite M): act_find
    Pure,      // PureRayMarching: the M forms with the marched optical depth
};
enum class SecTree {
    Wide4,    // the 4-wide f16 tree (per-axis copy, scene-normalised coordinates), from the record's start subtree
    PairF32,  // the f32 child-pair tree from the root (scenes whose leaf boxes are too small for f16 boxes)
};
constexpr int kSecBlock = 256;           // lanes per workgroup
constexpr int kSecStack = VR_WW_STACK;   // LDS traversal-stack entries per lane
constexpr int kSecQcap = VR_WW_QCAP;     // leaf-queue entries per lane
static_assert(kSecQcap >= 5 && ((kSecQcap - 1) & (kSecQcap - 2)) == 0, "VR_WW_QCAP: 1 + 2^k with k >= 2 (ring queue)");
// Waves per SIMD of the launch bounds: PureRayMarching's marched depth does not fit 6 waves' registers without spills.
constexpr int sec_waves(SecForm F) { return F == SecForm::Pure ? 5 : F == SecForm::Whitened ? VR_WW_WAVES : 6; }

struct SecRay {
    Ray ray;
    float ix, iy, iz, oxi, oyi, ozi;  // 1/d and o/d for the slab test
    float tau, lim;                   // optical depth so far; light: dist, env: +inf
    // `lim`: a light ray's distance to the light; an environment ray's last event so far (the
    // reference's t_env_end, test_integrators.h:258-271), which bounds nothing during traversal
    float cut;         // optical depth at which the ray's transmittance counts as 0 (error budget)
    float plim;        // node boxes entered beyond this distance hold nothing for the ray (light: past the light)
    uint64_t hitmask;  // which of the record's active Gaussians the ray has met
    uint64_t bloom;    // membership mask of the record's active list (act_find; PureRayMarching)
    float cmax;        // largest p.M.p (p = origin - mean) over the record's active list
    float credit;      // RayMarchingGaussians: list members' optical depth not yet met again by the tree walk
    uint32_t act_off, act_n;  // the record's active list
    bool light, needs_stop;
    bool bnd;          // the record has a member at its 3-sigma surface (kRecBoundary): the list phase tests the band
    uint32_t nsteps;  // instrumented build only: node steps taken by this ray
    // 4-wide walk: the parent entry of the subtree the ray walks (hn4_parent's form: the subtree's child slot + 1 in
    // bits 28-30), -1 at the root: the node of the next climb, loaded one climb ahead (sec_node4v).
    int32_t up;
    uint32_t rec;     // record index
    uint32_t slot;    // result slot s * rec_cap + rec in tr
};

// The ray's optical depth is known to have reached its cut-off. RayMarchingGaussians: tau holds what
// the tree walk met (list members included), credit the list members' depth it has not met yet, so
// tau + credit is a lower bound of the final depth (see wtest in secondary_ww_kernel; a credit that a
// non-member candidate drove below 0 only makes the bound lower).
template <bool PURE>
__device__ __forceinline__ bool cut_reached(const SecRay& R) {
    if constexpr (PURE) return R.tau >= R.cut;
    else return R.tau + R.credit >= R.cut;
}

// Slot of Gaussian j in the record's active list, or -1. The list is scanned four entries per
// round trip (independent loads), since a scan sits on the dependent chain of a primitive test.
__device__ __forceinline__ int act_find(const RenderArgs& A, const SecRay& R, int j) {
    if (!((R.bloom >> (j & 63)) & 1ull)) return -1;
    const int* __restrict__ p = A.rec_act + R.act_off;
    const int n = (int)R.act_n;
    for (int i = 0; i < n; i += 4) {
        const int v0 = p[i];
        const int v1 = i + 1 < n ? p[i + 1] : -1;
        const int v2 = i + 2 < n ? p[i + 2] : -1;
        const int v3 = i + 3 < n ? p[i + 3] : -1;
        if (v0 == j) return i;
        if (v1 == j) return i + 1;
        if (v2 == j) return i + 2;
        if (v3 == j) return i + 3;
    }
    return -1;
}

// Direction cells of the environment rays: the 16 x 16 cells of the sample's (xi1, xi2) = (azimuth, cos polar)
// grid, Morton-numbered (equal-area direction cells without evaluating the direction; measured against the
// octahedral map of the evaluated direction, round 3: 3.3 ms slower at C4).
constexpr int kEnvBits = 4, kEnvSide = 1 << kEnvBits, kEnvCells = kEnvSide * kEnvSide;

// The environment rays' list filter (VR_OPT_SEC_FILTER; DESIGN.md §3, pipeline step 2): the list phase of one
// environment ray, as secondary_ww_kernel's wtest runs it for a list member (ls >= 0) of a ray that is no light ray —
// the member's chord [max(t0, 0), t1] goes to `credit`, a stretch [0, t0] ahead of the origin to `tau`. The band and
// boundary tests of wtest only raise needs_stop, which sec_finish reads after the cut-off, so a ray that reaches its
// cut-off here stores Tr = 0 there whatever they say. A second definition rather than a shared one: the persistent
// kernel sits at its register limit (72 VGPRs) and its test is left as it compiles; the operations
// are the same ones in the same order (explicit fmaf, no contraction), so the decision is the kernel's bit for bit
// (tests/test_gpu_sec_filter.py: frames and per-ray rows with the filter on and off).
__device__ __forceinline__ bool list_member_depth(const WRec& g, const Ray& ray, float& tau, float& credit) {
    const WQuad q = wquad(g, ray);
    float t0, t1, sd;
    if (!wintersect(q, t0, t1, sd)) return false;
    const bool inside = q.hr > -sd;  // t0 < 0: the origin lies in the 3-sigma sphere
    constexpr float kRs2 = 0.70710678118654752f;
    const float F1 = erf_chord(sd * kRs2), F0 = erf_chord(q.hr * kRs2);  // a member is summed from 0
    const float pf = (g.dn * q.r) * __expf(-0.5f * q.e2);
    const float od = pf * fmaxf(F1 - F0, 0.0f);
    const float chord = inside ? od : pf * (F1 + F1);
    credit += chord;
    tau += od - chord;
    return true;
}
#ifndef VR_SEC_FILTER_MAX
#define VR_SEC_FILTER_MAX 16  // longest active list the filter tests; the rays of longer ones are handed out
#endif
constexpr uint32_t kFilterMax = VR_SEC_FILTER_MAX;

// One sorting group per record chunk: counting sort of the chunk's environment rays by direction key
// (order inside a key is arbitrary: every ray's result is independent of when it is traced). A group
// is one wave: 4 chunks in flight per workgroup of 256, wave-local LDS and no workgroup barriers; the
// chunk's chain of dependent loads is the cost, not its arithmetic (C4: 1.56 ms; a workgroup per chunk 1.91).
// One more bucket follows the direction cells: the rays the persistent kernel need not trace — those of padding
// records, of records without a ray to trace (weight <= 0, sec_init) and, with A.sec_filter, those that reach
// their optical-depth cut-off on their record's active list (list_member_depth). The order still lists every
// ray of the chunk, so a ray's Tr slot is its position in it as before; the rays of that bucket get their
// Tr = 0 here, and A.env_count tells the persistent kernel how many rays come before them.
// S: the instrumented build (vr_count_work) counts the filter's list tests and the rays it keeps back where the
// persistent kernel counts its own.
template <bool S>
__global__ __launch_bounds__(256) void env_order_kernel(RenderArgs A) {
    constexpr int G = 64, kGroups = 256 / G;
    constexpr uint32_t kKeyCap = 8192 / kGroups;  // keys kept in LDS per group; larger chunks recompute them
    constexpr uint32_t kRecMax = 1u << VR_CHUNK_SHIFT;  // records per chunk (A.chunk_rec)
    constexpr uint32_t kTail = kEnvCells;         // the bucket behind every direction cell
    static_assert(kEnvCells <= 256, "direction keys are kept in 8 bits");
    constexpr int kPer = kEnvCells / 64;  // counts per lane of the scan
    __shared__ uint32_t hist_s[kGroups][kEnvCells + 1];
    __shared__ uint8_t keys_s[kGroups][kKeyCap];
    __shared__ uint64_t tail_s[kGroups][kKeyCap / 64];  // with the keys: the rays of the last bucket, a bit each
    __shared__ uint64_t base_s[kGroups][kRecMax];  // the chunk's generator states
    // the chunk's records: position and weight, active list (offset, count; count 0: not tested), cut-off
    __shared__ float4 pos_s[kGroups][kRecMax];
    __shared__ uint2 act_s[kGroups][kRecMax];
    __shared__ float cut_s[kGroups][kRecMax];
    __shared__ int32_t ids_s[kGroups][kRecMax * kFilterMax];  // the tested lists' members (shared by a record's rays)
    const uint32_t grp = threadIdx.x / G, tid = threadIdx.x % G;
    uint32_t* hist = hist_s[grp];
    uint8_t* keys = keys_s[grp];
    uint64_t* tailm = tail_s[grp];
    uint64_t* base = base_s[grp];
    float4* rpos = pos_s[grp];
    uint2* ract = act_s[grp];
    float* rcut = cut_s[grp];
    int32_t* ids = ids_s[grp];
    auto group_sync = [] {
        if constexpr (G == 64) {  // the wave's own LDS traffic: wait for it, keep the compiler from moving it
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
        } else {
            __syncthreads();
        }
    };
    const uint32_t nrec = dev_nrec(A);
    const uint32_t cr = A.chunk_rec, ne = (uint32_t)A.env_samples;
    const uint32_t n = cr * ne, nch = (nrec + cr - 1) / cr;
    const bool cached = n <= kKeyCap;
    const bool filter = A.sec_filter != 0 && A.wrec != nullptr;
    Ctr c{};
    uint32_t nfiltered = 0;  // this lane's rays cut on their list
    if (cr > kRecMax) return;  // (never: gauss_pipeline sets chunk_rec = 1 << VR_CHUNK_SHIFT with env_order)
    for (uint32_t chunk = blockIdx.x * kGroups + grp; chunk < nch; chunk += gridDim.x * kGroups) {  // group-uniform loop
        const uint32_t r0 = chunk * cr;
        for (uint32_t i = tid; i <= kEnvCells; i += G) hist[i] = 0;
        for (uint32_t rl = tid; rl < cr; rl += G) {  // seeded once per record, not per sample
            float4 pos = make_float4(0.0f, 0.0f, 0.0f, -1.0f);  // a padding record: no ray to trace
            uint2 act = make_uint2(0u, 0u);
            float cut = A.tau_cut;
            if (r0 + rl < nrec) {
                const uint4 meta = A.rec_meta[r0 + rl];
                base[rl] = env_base_state(meta);
                A.env_base[r0 + rl] = base[rl];  // for sec_init: one 8-B load instead of the seeding per ray
                pos = A.rec_pos[r0 + rl];
                const uint32_t an = meta.w & ~kRecBoundary;
                if (filter && an <= kFilterMax) act = make_uint2(meta.z, an);
                if (A.rec_cut != nullptr) cut = A.rec_cut[r0 + rl];
            }
            rpos[rl] = pos;
            ract[rl] = act;
            rcut[rl] = cut;
        }
        group_sync();
        if (filter)  // the members' ids, gathered side by side: no link of a ray's load chain
            for (uint32_t i = tid; i < cr * kFilterMax; i += G) {
                const uint2 act = ract[i / kFilterMax];
                if (i % kFilterMax < act.y) ids[i] = A.rec_act[act.x + i % kFilterMax];
            }
        group_sync();
        // the ray's bucket; count: the instrumented build's counts (once per ray: an uncached chunk asks twice)
        auto key = [&](uint32_t i, bool count) -> uint32_t {
            const uint32_t rl = i / ne;
            const float4 pos = rpos[rl];
            if (!(pos.w > 0.0f)) {  // padding, weightless and orphaned records (sec_init hands none of their rays on)
                if constexpr (S) c.v[kCtrSecRays] += count ? 1u : 0u;
                return kTail;
            }
            // the cell of the sample's (xi1, xi2) = (azimuth, cos polar) grid: equal-area direction
            // cells without evaluating the direction
            float xi1, xi2;
            env_xi_at(A, base[rl], i - rl * ne, xi1, xi2);
            const uint2 act = ract[rl];
            if (act.y > 0u) {  // the list phase, members in list order, up to the first that reaches the cut-off
                float wx, wy, wz;
                env_dir(xi1, xi2, wx, wy, wz);
                const Ray ray{pos.x, pos.y, pos.z, wx, wy, wz};
                const float cut = rcut[rl];
                float tau = 0.0f, credit = 0.0f;
                const int32_t* mem = ids + rl * kFilterMax;
                for (uint32_t m = 0; m < act.y; ++m) {
                    // (the next member's record loaded ahead of this test, A/B at C4: 86 VGPRs, 5 waves, 0.5 ms slower)
                    const bool hit = list_member_depth(load_wrec(A.wrec, mem[m]), ray, tau, credit);
                    if constexpr (S) {
                        c.v[kCtrMu] += count ? 1u : 0u;
                        c.v[kCtrOD] += (count && hit) ? 1u : 0u;
                    }
                    if (tau + credit >= cut) {  // cut_reached
                        if constexpr (S) {
                            c.v[kCtrSecRays] += count ? 1u : 0u;
                            c.v[kCtrSteps] += count ? 1u : 0u;  // a cut ray without node steps
                        }
                        nfiltered += count ? 1u : 0u;
                        return kTail;
                    }
                }
            }
            const uint32_t cu = min((uint32_t)(xi1 * kEnvSide), (uint32_t)kEnvSide - 1u);
            const uint32_t cv = min((uint32_t)(xi2 * kEnvSide), (uint32_t)kEnvSide - 1u);
            uint32_t k = 0;
#pragma unroll
            for (int b = 0; b < kEnvBits; ++b) k |= (((cu >> b) & 1u) << (2 * b)) | (((cv >> b) & 1u) << (2 * b + 1));
            return k;
        };
        for (uint32_t i = tid; i < n; i += G) {
            const uint32_t k = key(i, true);
            if (cached) {
                keys[i] = (uint8_t)k;  // (the last bucket: the bit below)
                const uint64_t tails = __ballot(k == kTail);  // rays i - tid .. of this round (lane 0 is in every round)
                if (tid == 0) tailm[i / 64u] = tails;
            }
            atomicAdd(&hist[k], 1u);
        }
        group_sync();
        if (tid < 64) {  // exclusive scan of the counts by one wave (kPer consecutive per lane)
            const uint32_t l = tid;
            uint32_t v[kPer], sum = 0;
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                v[j] = hist[kPer * l + j];
                sum += v[j];
            }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o, 64);
                if (l >= (uint32_t)o) incl += y;
            }
            uint32_t ex = incl - sum;
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                hist[kPer * l + j] = ex;
                ex += v[j];
            }
            if (l == 63u) hist[kTail] = incl;  // the last bucket starts behind every direction cell
        }
        group_sync();
        const uint32_t kept = hist[kTail];  // rays the persistent kernel hands out (read before the scatter moves it)
        group_sync();
        uint16_t* out = A.env_order + (size_t)chunk * n;
        for (uint32_t i = tid; i < n; i += G) {
            const uint32_t rl = i / ne;
            const uint32_t k = !cached ? key(i, false) : ((tailm[i / 64u] >> tid) & 1ull) ? kTail : (uint32_t)keys[i];
            out[atomicAdd(&hist[k], 1u)] = (uint16_t)((rl << 8) | (i - rl * ne));
        }
        // the last bucket's results: a contiguous run of the chunk's Tr slots (rays_per_chunk: lights first)
        float* tr = A.tr + (size_t)chunk * rays_per_chunk(A) + cr * (uint32_t)A.num_lights;
        for (uint32_t i = kept + tid; i < n; i += G) tr[i] = 0.0f;
        if (tid == 0) A.env_count[chunk] = kept;
        group_sync();  // hist / keys / base are reused by the group's next chunk (staging the order in LDS
                       // for coalesced stores measured slower: 1.64 vs 1.56 ms at C4)
    }
    for (int o = 32; o > 0; o >>= 1) nfiltered += __shfl_xor(nfiltered, o, 64);
    if (tid == 0 && nfiltered != 0u) atomicAdd(&A.rec_alloc[3], nfiltered);
    if constexpr (S) flush_counters(A.work + kNumCtr, c);
}

// Start ray `rem` of record chunk `chunk`. Returns false if the ray is already complete (Tr
// written) or a padding id. The 4-wide tree: slab-test terms in the half nodes' scene-normalised
// coordinates (HNode). start: the node the tree walk starts at (the 4-wide walk: in the record's start subtree;
// otherwise the root); the record's start entry (its node and that node's parent entry, for the first climb) is
// gathered here, next to the record's other words, so that it is no link of the ray's load chain.
template <SecTree T>
__device__ __forceinline__ bool sec_init(const RenderArgs& A, uint32_t nrec, uint32_t chunk, uint32_t rem, SecRay& R,
                                         int32_t& start) {
    constexpr bool norm = T == SecTree::Wide4, wide = T == SecTree::Wide4;
    uint32_t s, r;
    if (!ray_slot(A, chunk, rem, nrec, s, r)) return false;  // padding id
    R.slot = chunk * rays_per_chunk(A) + rem;
    const float4 pos = A.rec_pos[r];
    if (!(pos.w > 0.0f)) {  // no ray to trace
        // a live record whose weight T sigma_s is 0 (an f32 underflow, or an over-capacity frame's empty
        // record): its radiance is weighed by 0, but record_radiance reads every slot, so a finite Tr;
        // an orphaned record (orphan_records, weight -1): no pixel reads its rays
        if (!(pos.w < 0.0f)) A.tr[R.slot] = 0.0f;
        return false;
    }
    const uint4 meta = A.rec_meta[r];
    RecStart st{0, -1};  // (the root)
    if (wide && A.rec_start != nullptr) st = A.rec_start[r];
    start = st.node;
    R.rec = r;
    R.cut = A.tau_cut;  // (a select of the two addresses would make this one flat load)
    if (A.rec_cut != nullptr) R.cut = __builtin_nontemporal_load(A.rec_cut + r);
    R.act_off = meta.z;
    R.act_n = meta.w & ~kRecBoundary;
    R.bnd = (meta.w & kRecBoundary) != 0u;
    R.bloom = A.rec_bloom[r];
    R.cmax = -INFINITY;
    R.credit = 0.0f;
    R.hitmask = 0;
    R.nsteps = 0;
    R.up = st.up;
    R.tau = 0.0f;
    R.needs_stop = false;
    if (s < (uint32_t)A.num_lights) {
        const LightRecord& lr = A.lights[s];
        float dx = lr.px - pos.x, dy = lr.py - pos.y, dz = lr.pz - pos.z;
        // a secondary ray feeds only its Tr (continuous): one hardware-rsqrt normalisation instead of
        // the reference's two correctly rounded ones (direction within ~1 ulp)
        const float d2 = dot3(dx, dy, dz, dx, dy, dz);
        const float dist = sqrtf(d2);
        const float inv = __builtin_amdgcn_rsqf(d2);
        R.ray = Ray{pos.x, pos.y, pos.z, dx * inv, dy * inv, dz * inv};
        R.light = true;
        R.lim = dist;
        if (!(dist > 0.0f)) {  // `while (t_prev < dist)` never runs
            A.tr[R.slot] = 1.0f;
            return false;
        }
    } else {
        float wx, wy, wz;
        float xi1, xi2;  // (env_order_kernel left the record's generator state when it ran)
        env_xi_at(A, A.env_order != nullptr ? A.env_base[r] : env_base_state(meta), s - (uint32_t)A.num_lights, xi1, xi2);
        env_dir(xi1, xi2, wx, wy, wz);
        R.ray = Ray{pos.x, pos.y, pos.z, wx, wy, wz};  // env_dir's direction is unit up to rounding
        R.light = false;
        R.lim = 0.0f;  // last event so far
    }
    R.plim = R.light ? R.lim + kTPad * (1.0f + R.lim) : INFINITY;
    // |d| clamped away from 0: the fma slab form b/d - o/d must never see inf - inf
    const float sc = norm ? A.hn_scale : 1.0f;
    const float dx = R.ray.dx * sc, dy = R.ray.dy * sc, dz = R.ray.dz * sc;
    R.ix = __builtin_amdgcn_rcpf(fabsf(dx) > 1e-30f ? dx : copysignf(1e-30f, dx));
    R.iy = __builtin_amdgcn_rcpf(fabsf(dy) > 1e-30f ? dy : copysignf(1e-30f, dy));
    R.iz = __builtin_amdgcn_rcpf(fabsf(dz) > 1e-30f ? dz : copysignf(1e-30f, dz));
    if (norm) {
        R.oxi = (R.ray.ox - A.hn_center[0]) * sc * R.ix;
        R.oyi = (R.ray.oy - A.hn_center[1]) * sc * R.iy;
        R.ozi = (R.ray.oz - A.hn_center[2]) * sc * R.iz;
    } else {
        R.oxi = R.ray.ox * R.ix;
        R.oyi = R.ray.oy * R.iy;
        R.ozi = R.ray.oz * R.iz;
    }
    return true;
}

// PureRayMarching (integrator.h:105-135): the marched transmittance multiplies exp(-sigma_t dt)
// over the iterated steps t_k = 0, dt, 2dt, ... of the secondary ray; grouped per Gaussian that is
// dt * sum of its mu_t at the steps t_k in [lo, hi) where it is active.
__device__ __forceinline__ float marched_depth(const RenderArgs& A, const GRec& g, const Ray& r, float lo, float hi) {
    const float* __restrict__ ts = A.tsteps;
    float s = 0.0f;
    for (int k = kfirst(ts, A.num_tsteps, A.step_size, lo); k < A.num_tsteps; ++k) {
        const float t = ts[k];
        if (!(t < hi)) break;
        s += mu_t(g, r.ox + t * r.dx, r.oy + t * r.dy, r.oz + t * r.dz);
    }
    return s * A.step_size;
}

// Adds Gaussian g (active on the secondary ray over [lo, b)) to the ray's optical depth.
//   RayMarchingGaussians: analytic segment depth; a light ray's Gaussian straddling the light
//   needs the first event past the light (test_integrators.h:220-235) -> exact slow path.
//   PureRayMarching: marched to t < dist (light) / t < last event (environment, b <= tlast).
template <bool S, bool PURE>
__device__ __forceinline__ void sec_add(const RenderArgs& A, SecRay& R, const GRec& g, const Quad& q, float lo, float b,
                                        Ctr& c) {
    if constexpr (S) c.v[kCtrOD]++;
    if constexpr (PURE) {
        if (!R.light) {
            R.tau += marched_depth(A, g, R.ray, lo, b);
            R.lim = fmaxf(R.lim, b);
        } else if (lo < R.lim) {
            R.tau += marched_depth(A, g, R.ray, lo, fminf(b, R.lim));
        }
        return;
    }
    // one optical-depth evaluation for light and environment lanes alike
    const bool add = !R.light || b < R.lim;
    R.needs_stop = R.needs_stop || (!add && lo < R.lim);
    if (!R.light) R.lim = fmaxf(R.lim, b);
    if (add) R.tau += optical_depth_chord(g, q, lo, b);  // [lo, b] lies on the 3-sigma chord
}

// VR_DIAG_SKIP_TR_STORES: diagnostic builds only (tools_dbg, never the product library): the
// secondary rays' Tr stores are dropped so that rocprofv3 WRITE_SIZE attributes the kernel's write
// traffic (Tr stores vs traversal-stack spills). The traversal itself is unchanged.
#ifdef VR_DIAG_SKIP_TR_STORES
#define VR_TR_STORE(A, slot, v) ((void)(slot), (void)(v))
#else
#define VR_TR_STORE(A, slot, v) ((A).tr[slot] = (v))
#endif

// Hands a ray to the exact slow path (secondary_slow_kernel). A full queue raises the frame's capacity flag
// (rec_alloc[2], as a full record buffer does): the frame is reported and rendered again with the queue grown to
// what this one queued (the host's slow_hint), so no ray is ever lost to the queue's size.
__device__ __forceinline__ void to_slow(const RenderArgs& A, uint32_t slot) {
    const uint32_t q = atomicAdd(A.slowq, 1u);
    if (q < A.slowq_cap) {
        A.slowq[1 + q] = slot;
    } else {
        A.rec_alloc[2] = 1u;
        A.tr[slot] = __builtin_nanf("");
    }
}

// Hands an environment ray with one chord in the f32 error band to secondary_fix_kernel: its slot, the optical
// depth of everything else it crossed and the band Gaussian. A full queue: as to_slow.
__device__ __forceinline__ void to_fix(const RenderArgs& A, uint32_t slot, float tau, uint32_t j) {
    const uint32_t q = atomicAdd(A.fixq, 1u);
    if (q < A.fixq_cap) {
        A.fixq[1 + 3 * q] = slot;
        A.fixq[2 + 3 * q] = __float_as_uint(tau);
        A.fixq[3 + 3 * q] = j;
    } else {
        A.rec_alloc[2] = 1u;
        A.tr[slot] = __builtin_nanf("");
    }
}

// Ray complete: write its transmittance (or hand it to the exact slow path).
template <bool S, SecForm F>
__device__ __forceinline__ void sec_finish(const RenderArgs& A, SecRay& R, Ctr& c) {
    constexpr bool PURE = F == SecForm::Pure, WH = F == SecForm::Whitened;
#if !defined(VR_DIAG_WAVE_UTIL) && !defined(VR_DIAG_CYCLES)
    if constexpr (S) {  // secondary-stage diagnostics in otherwise unused counter slots
        if (cut_reached<PURE>(R)) {
            c.v[kCtrSteps]++;                 // rays ended by the optical-depth cut-off
            c.v[kCtrPrimQueries] += R.nsteps;  // ... and their node steps
        }
    }
#endif
    if (cut_reached<PURE>(R)) {
        VR_TR_STORE(A, R.slot, 0.0f);
        return;
    }
    if (!PURE && R.needs_stop) {  // the exact slow path: a light ray's stopping event, a member at the boundary,
        to_slow(A, R.slot);       // a chord in the f32 error band
        return;
    }
    const bool band = !PURE && !R.light && isnan(R.lim);
    if (band && (R.act_n >= 64 || (R.hitmask & ((1ull << R.act_n) - 1ull)) != ((1ull << R.act_n) - 1ull))) {
        to_slow(A, R.slot);  // a band ray with a missed member (active to the last event): the whole ray exactly
        return;
    }
    if (R.act_n > 64) {  // (march_deep_kernel records) missed members: re-intersect the whole list
        bool any = false;
        for (uint32_t s = 0; s < R.act_n; ++s) {
            const int j = A.rec_act[R.act_off + s];
            if constexpr (!PURE && WH) {  // the list phase's whitened test
                const WRec g = load_wrec(A.wrec, j);
                const WQuad q = wquad(g, R.ray);
                float t0, t1, sd;
                if (wintersect(q, t0, t1, sd)) continue;
                any = true;
                if (!R.light) R.tau += wod_range(g, q, 0.0f, R.lim);
                else break;
                continue;
            }
            const GRec g = load_rec(A.gauss, j);
            const Quad q = quad_fast(g, R.ray);
            float a, b;
            if (intersect_fast(q, a, b)) continue;
            any = true;
            if constexpr (PURE) R.tau += marched_depth(A, g, R.ray, 0.0f, R.lim);
            else if (!R.light) R.tau += optical_depth_fast(g, q, 0.0f, R.lim);
            else break;
        }
        if (!PURE && R.light && (R.needs_stop || any)) {
            to_slow(A, R.slot);
            return;
        }
        VR_TR_STORE(A, R.slot, expf(-R.tau));
        return;
    }
    const uint64_t all = R.act_n >= 64 ? ~0ull : ((1ull << R.act_n) - 1ull);
    uint64_t missed = all & ~R.hitmask;
    if constexpr (PURE) {  // pre-activated, missed through rounding: active to the end of the march
        while (missed) {
            int s = __ffsll((unsigned long long)missed) - 1;
            missed &= missed - 1;
            GRec g = load_rec(A.gauss, A.rec_act[R.act_off + s]);
            R.tau += marched_depth(A, g, R.ray, 0.0f, R.lim);  // dist (light) / last event (environment)
        }
    } else if (R.light) {
        if (R.needs_stop || missed) {
            to_slow(A, R.slot);
            return;
        }
    } else if (band) {  // (no missed member: see above)
    } else {
        while (missed) {  // pre-activated, missed through rounding: active up to the last event
            int s = __ffsll((unsigned long long)missed) - 1;
            missed &= missed - 1;
            if constexpr (S) c.v[kCtrOD]++;
            if constexpr (WH) {
                const WRec g = load_wrec(A.wrec, A.rec_act[R.act_off + s]);
                R.tau += wod_range(g, wquad(g, R.ray), 0.0f, R.lim);
            } else {
                const GRec g = load_rec(A.gauss, A.rec_act[R.act_off + s]);
                R.tau += optical_depth_fast(g, quad_fast(g, R.ray), 0.0f, R.lim);
            }
        }
    }
    if (band) {  // the band Gaussian's contribution: secondary_fix_kernel
        to_fix(A, R.slot, R.tau, band_id(R.lim));
        return;
    }
    VR_TR_STORE(A, R.slot, expf(-R.tau));
}

// An int in LDS (address space 3). The traversal stack and leaf queue are reached through this type
// so that a pop that may come from the LDS stack or the global overflow stays two typed loads (a
// ds_read and a global_load) instead of one flat load whose wait covers every outstanding access.
using LdsInt = __attribute__((address_space(3))) int;

// FIFO of up to kSecQcap leaf refs + the leaf being tested: the head entry in q0, the others in an LDS ring of
// kSecQcap - 1 words per lane above the traversal stack (`ext`), ring head in q1. A lane may take a NODE step while
// the queue has room for the leaves a step can add, so a lane holding queued leaves keeps walking the tree.
constexpr int kQueueLds = kSecQcap - 1;  // LDS words per lane of the queue

struct LeafQueue {
    int32_t q0, q1;
    int n;
    uint32_t j, end;  // current primitive range [j, end)
    // branch-free for the register entry: writes r at slot `idx` (no slot matches idx < 0)
    __device__ __forceinline__ void put(int idx, int32_t r, LdsInt* ext) {
        q0 = idx == 0 ? r : q0;
        if (idx >= 1) ext[((q1 + idx - 1) & (kSecQcap - 2)) * kSecBlock] = r;
    }
    __device__ __forceinline__ bool has_prim() const { return j < end || n > 0; }
    __device__ __forceinline__ uint32_t next(LdsInt* ext) {  // requires has_prim()
        if (j == end) {
            j = leaf_first(q0);
            end = j + leaf_count(q0);
            if (n > 1) {
                q0 = ext[(q1 & (kSecQcap - 2)) * kSecBlock];
                q1 = (q1 + 1) & (kSecQcap - 2);
            }
            --n;
        }
        return j++;
    }
};

// Traversal-stack entries past the kSecStack held in LDS spill to the global overflow buffer, laid
// out [depth - kSecStack][lane of the resident grid]: the lanes of a wave that are at the same depth
// share cache lines, and the shallow overflow levels every deep walk touches stay a small, dense,
// L2-resident region (a per-lane [lane][depth] layout gives every lane its own line per level).
__device__ __forceinline__ uint32_t ovf_slot(const RenderArgs& A, int sp) {
    return (uint32_t)(sp - kSecStack) * A.stack_ovf_lanes + blockIdx.x * kSecBlock + threadIdx.x;
}

// One step of the 4-wide traversal without a sorting network (measured against one with a near-to-far sorting
// network of the children, round 3: 102.4 -> 99.2 ms at C4): the nearest inner child is walked next
// (a min-reduction over the inner children's entry distances), the other inner children are pushed
// and the leaf children queued in the node's child order. Empty slots carry NaN boxes, so the slab
// test alone rejects them. The node is read from the per-axis copy of the tree (A.hnodes4t, soa_nodes_kernel's layout).
template <bool S>
__device__ __forceinline__ void sec_node4v(const RenderArgs& A, SecRay& R, LdsInt* stack, int& sp, int& node, LeafQueue& Q,
                                           Ctr& c) {
    if constexpr (S) {
        c.v[kCtrNodes]++;
        ++R.nsteps;
    }
    const int skip = node >> 28;  // a climb's node: the finished child's slot + 1 (0: none)
    const uint4* np = reinterpret_cast<const uint4*>(A.hnodes4t + (node & kNodeIndexMask));
    const uint4 q0 = np[0], q1 = np[1], q2 = np[2], rf = np[3];
    const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    const int32_t ref[4] = {(int32_t)rf.x, (int32_t)rf.y, (int32_t)rf.z, (int32_t)rf.w};
    // Per axis, the ray's near bound word pair and far bound word pair, picked once for the four children by the sign
    // of its direction: for 1/d > 0 the near slab is the min (fma is monotone in the bound), so the slab distances are
    // the min/max of the per-child (HNode4) test bit for bit, without the per-child min/max
    float smin[4], smax[4];  // the children's slab entry / exit (a child pair at a time, in the child loop)
    LdsInt* ext = stack + kSecStack * kSecBlock;
    float best = INFINITY;
    int32_t next = 0;  // the nearest inner child
    bool inner[4];
    // ring cursor: the next leaf goes to ring slot cur & (kSecQcap - 2); cur == head while the queue is
    // empty (the next leaf is the register head q0). Q.n follows from cur after the four children.
    const int head = Q.q1 - 1;
    int cur = head + Q.n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // children i, i + 1 from one word pair per axis, just before child i: computing all four children's slabs
        // up front kept 8 more values live across the step (12 spilled VGPRs at the 72-VGPR limit, twice the
        // write traffic, 77.5 vs 76.0 ms at C4)
        if (i == 0 || i == 2) {
            const int pr = i >> 1;
            const float inv[3] = {R.ix, R.iy, R.iz}, oi[3] = {R.oxi, R.oyi, R.ozi};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const bool neg = inv[ax] < 0.0f;
                const uint32_t nwd = neg ? w[4 * ax + 2 + pr] : w[4 * ax + pr], fwd = neg ? w[4 * ax + pr] : w[4 * ax + 2 + pr];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float nb = (float)__builtin_bit_cast(_Float16, (uint16_t)(h ? (nwd >> 16) : (nwd & 0xffffu)));
                    const float fb = (float)__builtin_bit_cast(_Float16, (uint16_t)(h ? (fwd >> 16) : (fwd & 0xffffu)));
                    const float tn = fmaf(nb, inv[ax], -oi[ax]), tf = fmaf(fb, inv[ax], -oi[ax]);
                    smin[i + h] = ax == 0 ? tn : fmaxf(smin[i + h], tn);
                    smax[i + h] = ax == 0 ? tf : fminf(smax[i + h], tf);
                }
            }
        }
        const float tmin = smin[i], tmax = smax[i];
        // [max(tmin, 0), min(tmax, plim)] not empty; a NaN box (empty slot) fails the first compare; the
        // subtree the ray has just finished (child slot skip - 1, right after a climb) is skipped
        const bool hit = (tmin <= fminf(tmax, R.plim)) & (tmax >= 0.0f) & (skip != i + 1);
        const bool leaf = hit & (ref[i] < 0);
        inner[i] = hit & !leaf;  // an empty slot (ref 0) never hits
        // leaf -> the queue's end: branch-free, a non-leaf store lands past the last entry (never
        // read). A NODE step starts with at most kSecQcap - 4 entries, so that slot is a free ring word.
        Q.q0 = (leaf & (cur == head)) ? ref[i] : Q.q0;
        ext[(cur & (kSecQcap - 2)) * kSecBlock] = ref[i];
        cur += (int)leaf;
        const bool nearer = inner[i] & (tmin < best);
        best = nearer ? tmin : best;
        next = nearer ? ref[i] : next;
    }
    Q.n = cur - head;
    // the other inner children -> stack, branch-free while every stepping lane has room for 4: the loop stores at
    // the running sp for every slot, so after three pushes the fourth slot's store, kept or not, lands at sp + 3,
    // and row kSecStack is the leaf queue's ring slot 0 (with room for 3 only, a queued leaf there was overwritten)
    if (__builtin_expect(__ballot(sp > kSecStack - 4) == 0ull, 1)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            stack[sp * kSecBlock] = ref[i];
            sp += (int)(inner[i] & (ref[i] != next));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (inner[i] & (ref[i] != next)) {
                if (sp < kSecStack) stack[sp * kSecBlock] = ref[i];
                else A.stack_ovf[ovf_slot(A, sp)] = ref[i];
                ++sp;
            }
        }
    }
    if (next != 0) {
        node = next;
    } else if (sp > 0) {
        --sp;
        node = sp < kSecStack ? stack[sp * kSecBlock] : A.stack_ovf[ovf_slot(A, sp)];
    } else {
        // the subtree is done: its parent next, without that child (every node is still visited at most once: the
        // walk from the record's start subtree up to the root covers the tree). The parent entry carries the
        // child's slot in bits 28-30 (slot + 1), which the next step skips.
        // R.up is that entry, loaded when the ray entered the subtree (-1: the root's subtree is done); the
        // parent's own entry is issued now and read at the next climb, many node steps later
        node = R.up;
        if (R.up >= 0) R.up = A.hn4_parent[R.up & kNodeIndexMask];
    }
}

// One step of the f32 child-pair traversal: leaf children go to the queue (nearer
// first); node < 0 afterwards means the traversal is finished. Written branch-free (bitwise
// predicates, selects) so a wave does not split inside the step.
template <bool S>
__device__ __forceinline__ void sec_node(const RenderArgs& A, SecRay& R, LdsInt* stack, int& sp, int& node, LeafQueue& Q,
                                         Ctr& c) {
    if constexpr (S) {
        c.v[kCtrNodes]++;
        ++R.nsteps;
    }
    float f[12];  // left min xyz, left max xyz, right min xyz, right max xyz
    int2 nc;
    load_pair<false>(A, node, f, nc);  // the f32 nodes
    const float tx1 = fmaf(f[0], R.ix, -R.oxi), tx2 = fmaf(f[3], R.ix, -R.oxi);
    const float ty1 = fmaf(f[1], R.iy, -R.oyi), ty2 = fmaf(f[4], R.iy, -R.oyi);
    const float tz1 = fmaf(f[2], R.iz, -R.ozi), tz2 = fmaf(f[5], R.iz, -R.ozi);
    const float lmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float lmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    const float ux1 = fmaf(f[6], R.ix, -R.oxi), ux2 = fmaf(f[9], R.ix, -R.oxi);
    const float uy1 = fmaf(f[7], R.iy, -R.oyi), uy2 = fmaf(f[10], R.iy, -R.oyi);
    const float uz1 = fmaf(f[8], R.iz, -R.ozi), uz2 = fmaf(f[11], R.iz, -R.ozi);
    const float rmin = fmaxf(fmaxf(fminf(ux1, ux2), fminf(uy1, uy2)), fminf(uz1, uz2));
    const float rmax = fminf(fminf(fmaxf(ux1, ux2), fmaxf(uy1, uy2)), fmaxf(uz1, uz2));
    const float lim = R.plim;
    const bool hl = (nc.x != 0) & (lmax >= fmaxf(lmin, 0.0f)) & (lmin <= lim);
    const bool hr = (nc.y != 0) & (rmax >= fmaxf(rmin, 0.0f)) & (rmin <= lim);
    const bool r_near = rmin < lmin;
    const bool ll = hl & (nc.x < 0), lr = hr & (nc.y < 0);  // leaf refs are negative
    const int32_t near_ref = r_near ? nc.y : nc.x, far_ref = r_near ? nc.x : nc.y;
    // leaves -> queue, nearer first
    const int32_t first_leaf = (ll & lr) ? near_ref : (ll ? nc.x : nc.y);
    Q.put((ll | lr) ? Q.n : -1, first_leaf, stack + kSecStack * kSecBlock);
    Q.put((ll & lr) ? Q.n + 1 : -1, far_ref, stack + kSecStack * kSecBlock);
    Q.n += (int)ll + (int)lr;
    // inner children -> continue / stack
    const bool il = hl & !ll, ir = hr & !lr;
    if (il & ir) {
        if (sp < kSecStack) stack[sp * kSecBlock] = far_ref;
        else A.stack_ovf[ovf_slot(A, sp)] = far_ref;
        ++sp;
    }
    if (il | ir) {
        node = (il & ir) ? near_ref : (il ? nc.x : nc.y);
    } else if (sp > 0) {
        --sp;
        node = sp < kSecStack ? stack[sp * kSecBlock] : A.stack_ovf[ovf_slot(A, sp)];
    } else {
        node = -1;
    }
}

// The list phase: every secondary ray of a record first tests the record's active list (the
// Gaussians active at the record's step: they contain the record position, so they carry the
// largest optical depths from it and most rays become opaque right there, without touching the
// tree); the tree walk that follows skips exactly these members (act_find). The phase lives in
// `node`: node <= kNodeList (-2) walks the active list [Q.j, Q.end) and carries the tree walk's start node X as
// kNodeList - X (no register of its own: SecRay::up holds X's parent entry), node >= 0 is the tree walk, -1 the end.
// (Until round 3 the phase walked a per-record neighbour list {j : q_j(pos) <= 9.5} built by a BVH
// point query per record; the active list is a subset the march already holds: no list stage
// (-6.1 ms at C4) and a 2.4 % faster secondary stage)
constexpr int kNodeList = -2;


// Start ray R's list phase (or go straight to the tree, at node `start`).
__device__ __forceinline__ void list_begin(SecRay& R, LeafQueue& Q, int& node, int32_t start) {
    Q.n = 0;
    Q.q1 = 0;  // ring head (ring queues): valid whenever the tree walk starts here
    Q.j = R.act_off;
    Q.end = R.act_off + R.act_n;
    node = R.act_n > 0u ? kNodeList - start : start;
}

// After a list slot was consumed: move to the tree (its start subtree) once the list is done.
__device__ __forceinline__ void list_advance(LeafQueue& Q, int& node) {
    if (node > kNodeList || Q.j < Q.end) return;
    Q.j = Q.end = 0;
    node = kNodeList - node;
}

constexpr int kRefillMin = VR_WW_REFILL, kNodeSteps = VR_WW_NODE_STEPS, kPrimSteps = VR_WW_PRIM_STEPS;
constexpr int kPrimBias = VR_WW_PRIM_BIAS;
constexpr int kPrimUnroll = VR_WW_PRIM_UNROLL, kNodeUnroll = VR_WW_NODE_UNROLL;

// The persistent kernel (the header at the top of this unit). Launch bounds, sec_waves(F) waves per SIMD: the whitened
// form at 7 = 72 VGPRs (the product kernel on the 4-wide tree sits at that limit with 2 spilled VGPRs),
// the M form at 6 = 80 VGPRs, PureRayMarching at 5 = 96 VGPRs (it needs 81 to 93).
template <bool S, SecForm F, SecTree T>
__global__ __launch_bounds__(kSecBlock, sec_waves(F)) void secondary_ww_kernel(RenderArgs A) {
    constexpr bool PURE = F == SecForm::Pure, WH = F == SecForm::Whitened, W = T == SecTree::Wide4;
    __shared__ int s_stack[(kSecStack + kQueueLds) * kSecBlock];
    LdsInt* stack = (LdsInt*)(s_stack + threadIdx.x);  // LDS-typed: stack/queue accesses are ds_* ops, never flat
    const uint32_t lane = threadIdx.x & 63u;
    Ctr c{};
    SecRay R;
    LeafQueue Q{0, 0, 0, 0u, 0u};
    uint32_t t = 0;
    int sp = 0, node = -1;
    bool live = false;
    // wave-uniform: the record chunk being handed out and its rays [pool, pool_end) not yet handed out
    uint32_t chunk = 0, pool = 0, pool_end = 0;
    bool counter_done = false;  // wave-uniform: the global chunk counter has passed nchunks
    bool fin = false;           // the lane's ray is complete and its Tr not yet written (batched completions)
    const uint32_t per = A.chunk_rec * (uint32_t)(A.num_lights + A.env_samples);
    const uint32_t nrec = dev_nrec(A), nchunks = (nrec + A.chunk_rec - 1u) >> A.chunk_shift;
    // Claim units: a chunk's rays in hand-out order, cut into 2^split equal parts when the launch has
    // few chunks per resident wave (a frame share of a multi-GPU split): shorter last units, a shorter
    // tail of the persistent launch (8-way C4 share: 22.7 -> 21.7 ms). Whole chunks otherwise (record
    // locality). (Measured and not kept, round 6: a guided tail — the launch's last 1/2/4 units per wave handed
    // out in 1/8 or 1/16 chunks — 8-way share prediction 7.12 -> 7.19/7.15/7.13, 1/16: 6.93; the tail after
    // the counter runs out is the in-flight rays' latency, not the unstarted rays left in a wave's pool. Nor is
    // that latency a few long walks: handing rays past 150/300/600/1200 node steps to the wave-per-ray slow path
    // re-routed 17 k/15/0/0 rays per C4 frame and cost 1.8 ms in spills. A ray waits on its wave's NODE/PRIM
    // schedule: ~100-250 us typical, up to ~2 ms, over ~30 node steps, measured with a diagnostic build since retired: DESIGN.md.)
    const uint32_t waves = gridDim.x * (kSecBlock / 64u), cpw = nchunks / max(waves, 1u);
    constexpr uint32_t kSplitCpw = VR_WW_SPLIT_CPW;
    const uint32_t split = cpw >= kSplitCpw ? 0u : cpw >= kSplitCpw / 2u ? 1u : cpw >= kSplitCpw / 4u ? 2u : 3u;
    const uint32_t nunits = nchunks << split;
    counter_done = nunits == 0u;
#ifdef VR_DIAG_CYCLES  // diagnostic builds only (S = true): wave cycles per phase, lane 0's counters
    // kCtrSteps: NODE iterations, kCtrPrimQueries: PRIM iterations, kCtrPixels: refill + completion
    uint64_t diag_t = __builtin_amdgcn_s_memtime();
    auto diag_lap = [&](int slot) {
        const uint64_t now = __builtin_amdgcn_s_memtime();
        if constexpr (S) c.v[slot] += lane == 0u ? (uint32_t)(now - diag_t) : 0u;
        diag_t = now;
    };
#else
    auto diag_lap = [](int) {};
#endif
    for (;;) {
        const uint64_t idle = __ballot(!live);
        if (__popcll(idle) >= kRefillMin) {  // refill once enough lanes are idle (amortises sec_init)
            if (fin) {  // the completions since the last refill, in one pass
                sec_finish<S, F>(A, R, c);
                fin = false;
            }
            if (pool == pool_end && !counter_done) {  // next unit of a record chunk
                uint32_t cnext = 0;
                if (lane == 0) cnext = (uint32_t)atomicAdd(A.ray_next, 1ull);
                cnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnext);  // wave-uniform: scalar register
                if (cnext < nunits) {
                    chunk = cnext >> split;
                    const uint32_t part = cnext & ((1u << split) - 1u);
                    // with an environment-ray order, the chunk's light rays and the head of its order: the rays behind
                    // it are complete (env_order_kernel); a chunk with neither is an empty unit, the next claim follows
                    uint32_t cper = per;
                    if (A.env_order != nullptr) cper = A.chunk_rec * (uint32_t)A.num_lights + A.env_count[chunk];
                    pool = (part * cper) >> split;
                    pool_end = ((part + 1u) * cper) >> split;
                }
                counter_done = cnext + 1u >= nunits;
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            if (!live && pool + rank < pool_end) {
                t = pool + rank;
                if constexpr (S) c.v[kCtrSecRays]++;
                int32_t start;
                live = sec_init<T>(A, nrec, chunk, t, R, start);  // false: padding id, or complete already (Tr written)
                sp = 0;
                node = -1;
                Q.n = 0;
                Q.j = Q.end = 0;
                if (live) list_begin(R, Q, node, start);
            }
            const uint32_t handed = (uint32_t)__popcll(idle);
            pool = pool_end - pool > handed ? pool + handed : pool_end;
        }
        if (!__any(live)) {
            if (fin) {  // (only if the refill threshold exceeded the wave: every lane idle refills above)
                sec_finish<S, F>(A, R, c);
                fin = false;
            }
            if (counter_done && pool == pool_end) break;
            continue;
        }
#ifdef VR_DIAG_WAVE_UTIL  // diagnostic builds only: wave iterations with a live lane, and live lanes in them
        if constexpr (S) c.v[kCtrPixels] += (lane == 0u ? 1u : 0u);
#endif
        diag_lap(kCtrPixels);
        const bool has_prim = live && Q.has_prim();
        constexpr int kRoom = W ? 4 : 2;  // leaves one NODE step can queue
        const bool can_node = live && node >= 0 && Q.n <= kSecQcap - kRoom;
        const int np = __popcll(__ballot(has_prim)), nn = __popcll(__ballot(can_node));
        // whichever kind more lanes can use; never a kind no lane can use (that would not progress)
        const bool prim_iter = nn == 0 || (np > 0 && np * 100 >= nn * kPrimBias);
        if (prim_iter) {  // PRIM iteration: up to kPrimSteps primitive tests per lane
            LdsInt* ext = stack + kSecStack * kSecBlock;
            // next primitive of the lane: a list member (ls = its slot) or a queued leaf's (ls = -1)
            auto fetch = [&](uint32_t& j, int& ls) {
                if (node <= kNodeList) {
                    ls = (int)(Q.j - R.act_off);
                    j = (uint32_t)A.rec_act[Q.j++];
                    list_advance(Q, node);
                } else {
                    ls = -1;
                    j = Q.next(ext);
                }
            };
            // one primitive test; ls >= 0: list member ls (pre-activated: optical depth from 0).
            // RayMarchingGaussians: the whitened record (WRecord); PureRayMarching: the record itself
            // (its marched depth evaluates mu_t)
            // The whitened primitive test (RayMarchingGaussians). The list phase sums the members' depths into
            // `credit` (the cut-off sees them at once); the tree walk then sums every Gaussian it meets into
            // tau, members included, so no membership lookup is needed. A member's p.M.p is <= cmax (the same
            // bits the list phase took), so it is a candidate when the walk meets it again; a candidate's
            // depth comes off the credit, which stays a lower bound of what the walk has still to meet. The
            // walk sums every Gaussian from its entry max(t0, 0): for a member that holds the origin (and for
            // any Gaussian that does) that is 0, the reference's pre-activation. A member whose chord starts
            // ahead of the origin (t0 > 0: the march's camera-ray test can activate a Gaussian a few percent
            // outside its ellipsoid) is pre-activated all the same: the list phase adds its stretch [0, t0]
            // to tau at once and only [t0, t1] to the credit. (Until round 5 every candidate was summed from
            // 0, so a non-member the origin lies just outside of, heading in, had [0, t0] too — with cmax > 9
            // such Gaussians pass the c test, and for a dense one that stretch is worth ~0.1 of optical depth:
            // C4 at t_eps 0, pixel (2224, 3653) 2.3e-3 dark.) Selects rather than fmaxf where an operand is
            // not known canonical: fmaxf would canonicalise it first, one more VALU op each.
            auto wtest = [&](const WRec& g, uint32_t j, int ls) {
                if constexpr (S) c.v[ls >= 0 ? kCtrMu : kCtrPrims]++;  // list members counted apart
                const WQuad q = wquad(g, R.ray);
                // A chord within the reference's f32 error band (kChordBand): on an environment ray, that one
                // Gaussian's contribution is left to the reference's M form (secondary_fix_kernel; the ray's tau
                // leaves it out, its id rides in R.lim); a member, a light ray or a second such chord sends the
                // whole ray to the exact slow path
                if constexpr (kChordBand > 0.0f) {
                    if (__builtin_expect(fmaf(-kChordBand, q.c, fabsf(9.0f - q.e2)) < 0.0f, false)) {
                        if (ls >= 0 || R.light || isnan(R.lim) || j >= 0x007fffffu) {
                            R.needs_stop = true;  // a member, a light ray or a second band chord: the whole ray exactly
                        } else {
                            R.lim = band_lim(j);
                            return;
                        }
                    }
                }
                R.cmax = (ls >= 0 && q.c > R.cmax) ? q.c : R.cmax;
                const bool cand = ls < 0 && q.c <= R.cmax;
                // A member whose 3-sigma surface passes within rounding of the record position (or that the ray
                // grazes): whether the reference's f32 test finds it crossed (active on [0, t1]) or missed
                // (active to the ray's last event — for a dense Gaussian ~1 of optical depth) is a rounding
                // decision the whitened form cannot reproduce: the exact slow path decides the ray (C4 at
                // t_eps 0, pixel (470, 3144): c = 9.00000, t1 = -0.00000 in the reference, 2.6e-2 bright).
                if (__builtin_expect(R.bnd, false))  // (~1 % of the records: rarely taken by a wave)
                    if (ls >= 0 && (fabsf(q.c - 9.0f) < kMemberAmb || fabsf(9.0f - q.e2) < kMemberAmb)) R.needs_stop = true;
                float t0, t1, sd;
                if (!wintersect(q, t0, t1, sd)) return;
                const bool inside = q.hr > -sd;  // t0 < 0: the origin lies in the 3-sigma sphere
                const bool pre = ls >= 0 || inside;
                const float lo = pre ? 0.0f : t0;
                const float u0 = pre ? q.hr : -sd;  // erf argument x sqrt 2 at lo
                if (ls >= 0) R.hitmask |= slot_bit(ls);
                if constexpr (S) {
                    c.v[kCtrOD]++;
#if !defined(VR_DIAG_WAVE_UTIL) && !defined(VR_DIAG_CYCLES)
                    c.v[kCtrPixels] += cand ? 1u : 0u;  // a list member's depth again (the credit scheme)
#endif
                }
                // sec_add's rule: one optical-depth evaluation for light and environment lanes
                const bool add = !R.light || t1 < R.lim;
                R.needs_stop = R.needs_stop | (!add & (lo < R.lim));
                R.lim = (!R.light && t1 > R.lim) ? t1 : R.lim;
                if (add) {  // wod_chord over [lo, t1] (the 3-sigma chord, but for a member's stretch [0, t0])
                    constexpr float kRs2 = 0.70710678118654752f;
                    const float F1 = erf_chord(sd * kRs2), F0 = erf_chord(u0 * kRs2);
                    const float pf = (g.dn * q.r) * __expf(-0.5f * q.e2);
                    const float od = pf * fmaxf(F1 - F0, 0.0f);  // (f32 noise can invert a tiny interval)
                    if (ls >= 0) {  // the credit takes the chord [max(t0, 0), t1] (erf_chord is odd), tau the rest
                        const float chord = inside ? od : pf * (F1 + F1);
                        R.credit += chord;
                        R.tau += od - chord;  // + 0 when the origin lies inside
                    } else {
                        R.tau += od;
                        if (cand) R.credit -= od;
                    }
                }
            };
            auto test = [&](const GRec& g, uint32_t j, int ls) {
                if constexpr (S) c.v[ls >= 0 ? kCtrMu : kCtrPrims]++;  // list members counted apart
                const Quad q = quad_fast(g, R.ray);
                int slot = ls;
                if (ls >= 0) {
                    R.cmax = fmaxf(R.cmax, q.Cq);
                } else if (q.Cq <= R.cmax) {
                    // a tree leaf skips the record's active Gaussians (already summed by the list phase).
                    // Only a Gaussian that holds the origin as far as the members' own p.M.p values go
                    // (the same cq_fast bits, taken by the list phase) can be one: no scan otherwise
                    slot = act_find(A, R, (int)j);
                    if (slot >= 0) return;
                }
                float a, b;
                if (intersect_fast(q, a, b)) {
                    float lo = a;
                    if (slot >= 0) {
                        lo = 0.0f;
                        R.hitmask |= slot_bit(slot);
                    }
                    sec_add<S, PURE>(A, R, g, q, lo, b, c);
                }
            };
            bool go = has_prim;
#pragma unroll kPrimUnroll
            for (int k = 0; k < kPrimSteps; ++k) {
#ifdef VR_DIAG_WAVE_UTIL  // diagnostic builds only: wave-level PRIM steps (lane utilisation)
                if constexpr (S) c.v[kCtrPrimQueries] += (__ballot(go) != 0ull && lane == 0u) ? 1u : 0u;
#endif
                if (go) {
                    uint32_t j;
                    int ls;
                    fetch(j, ls);
                    if constexpr (!WH) test(load_rec(A.gauss, (int)j), j, ls);
                    else wtest(load_wrec(A.wrec, (int)j), j, ls);
                }
                go = go && Q.has_prim() && !cut_reached<PURE>(R);
            }
            diag_lap(kCtrPrimQueries);
        } else {  // NODE iteration: up to kNodeSteps node steps per lane
            bool go = can_node;
#pragma unroll kNodeUnroll
            for (int k = 0; k < kNodeSteps; ++k) {
#ifdef VR_DIAG_WAVE_UTIL  // diagnostic builds only: wave-level NODE steps (lane utilisation)
                if constexpr (S) c.v[kCtrSteps] += (__ballot(go) != 0ull && lane == 0u) ? 1u : 0u;
#endif
                if (go) {
                    if constexpr (W) sec_node4v<S>(A, R, stack, sp, node, Q, c);
                    else sec_node<S>(A, R, stack, sp, node, Q, c);
                }
                go = go && node >= 0 && Q.n <= kSecQcap - kRoom;
            }
            diag_lap(kCtrSteps);
        }
        if (live && (cut_reached<PURE>(R) || (node == -1 && !Q.has_prim()))) {
            fin = true;  // written at the next refill (the lane idles until then anyway)
            live = false;
        }
    }
    if constexpr (S) flush_counters(A.work + kNumCtr, c);
}

// Environment rays with one chord in the reference f32 quadratic's error band (to_fix): the band Gaussian's
// contribution as the reference computes it — its M-form crossing on the exactly normalised ray (a collapsed chord
// contributes nothing, a phantom one its tiny depth), active from max(t0, 0) to t1 (test_integrators.h:242-271 with
// stable tie order) — added to the optical depth of everything else the ray crossed.
__global__ __launch_bounds__(64) void secondary_fix_kernel(RenderArgs A) {
    const uint32_t n = min(A.fixq[0], A.fixq_cap);
    for (uint32_t q = blockIdx.x * 64u + threadIdx.x; q < n; q += gridDim.x * 64u) {
        const uint32_t t = A.fixq[1 + 3 * q];
        const float tau = __uint_as_float(A.fixq[2 + 3 * q]);
        const GRec g = load_rec(A.gauss, (int)A.fixq[3 + 3 * q]);
        // (the environment-ray part of decode_queued_ray: the whole decode, with its light branch, active list and
        // 64-bit slot, makes this kernel 675 -> 815 instructions)
        const uint32_t per = rays_per_chunk(A), chunk = t / per, rem = t - chunk * per;
        uint32_t s, r;
        ray_slot(A, chunk, rem, dev_nrec(A), s, r);
        const float4 pos = A.rec_pos[r];
        float xi1, xi2, wx, wy, wz;
        env_xi_at(A, A.env_order != nullptr ? A.env_base[r] : env_base_state(A.rec_meta[r]), s - (uint32_t)A.num_lights, xi1, xi2);
        env_dir(xi1, xi2, wx, wy, wz);
        const Ray er = make_ray(pos.x, pos.y, pos.z, wx, wy, wz);
        const Quad qd = quad(g, er);
        float a, b;
        const float od = intersect(qd, a, b) ? optical_depth(g, qd, a, b) : 0.0f;
        A.tr[t] = expf(-(tau + od));
    }
}

// Start subtree of a record's secondary rays: the deepest 4-wide node whose box holds the record position,
// taking at every level the inner child with the most room. The rays walk that subtree first and then climb to its parents (sec_node4v), so every node is
// still visited at most once, and a ray whose optical-depth cut-off is reached near its origin — most of
// them: the record sits inside an opaque blob's neighbours — skips the descent from the root.
// Every record has an active Gaussian (a step scatters only with sigma_s > 0): the 4-wide node whose
// child is that Gaussian's leaf is a leaf-level node near the record (the Gaussian holds the position),
// found with two loads instead of a descent from the root (record_start_kernel 0.63 -> ~0.1 ms at C4); the
// descent remains for a record without one.
__global__ __launch_bounds__(256) void record_start_kernel(RenderArgs A) {
    const uint32_t nrec = dev_nrec(A);
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nrec; r += gridDim.x * 256u) {
        if (A.prim_node4 != nullptr) {
            const uint4 meta = A.rec_meta[r];
            if ((meta.w & ~kRecBoundary) > 0u) {
                const int32_t x = A.prim_node4[A.rec_act[meta.z]];
                A.rec_start[r] = RecStart{x, A.hn4_parent[x]};
                continue;
            }
        }
        const float4 pos = A.rec_pos[r];
        float p[3] = {pos.x, pos.y, pos.z};
        node_space<true>(A, p[0], p[1], p[2]);
        int32_t node = 0;
        for (int depth = 0; depth < kWideStackMax; ++depth) {
            const uint4* np = reinterpret_cast<const uint4*>(A.hnodes4s + node);
            const uint4 q0 = np[0], q1 = np[1], q2 = np[2], rf = np[3];
            const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            const int32_t ref[4] = {(int32_t)rf.x, (int32_t)rf.y, (int32_t)rf.z, (int32_t)rf.w};
            float best = 0.0f;
            int32_t next = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float room = INFINITY;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t wl = w[(6 * i + k) >> 1], wh = w[(6 * i + 3 + k) >> 1];
                    const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(((6 * i + k) & 1) ? (wl >> 16) : (wl & 0xffffu)));
                    const float hi =
                        (float)__builtin_bit_cast(_Float16, (uint16_t)(((6 * i + 3 + k) & 1) ? (wh >> 16) : (wh & 0xffffu)));
                    room = fminf(room, fminf(p[k] - lo, hi - p[k]));
                }
                const bool take = (ref[i] > 0) & (room >= best);  // (a NaN box never has room)
                best = take ? room : best;
                next = take ? ref[i] : next;
            }
            if (next < 0) break;
            node = next;
        }
        A.rec_start[r] = RecStart{node, A.hn4_parent[node]};  // (start entries exist with a parent table only: gauss_pipeline)
    }
}

}  // namespace dev

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
// One launch of the persistent kernel: one resident grid (every CU filled to the kernel's occupancy).
// LDS words per lane: 14 traversal-stack entries (deeper ones overflow to global memory) + the
// 8-entry LDS ring of the 9-entry leaf queue = 22 (7 blocks of 256 lanes per CU).
template <bool S, dev::SecForm F, dev::SecTree T>
static hipError_t ww_launch(const RenderArgs& A, hipStream_t stream) {
    constexpr int kBlock = dev::kSecBlock;
    const void* fn = (const void*)dev::secondary_ww_kernel<S, F, T>;
    int dv = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dv) != hipSuccess) return hipErrorUnknown;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dv) != hipSuccess) return hipErrorUnknown;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    uint64_t grid = (uint64_t)cus * (uint64_t)per_cu;
    if (grid * kBlock > A.stack_ovf_lanes) grid = A.stack_ovf_lanes / kBlock;  // overflow slots
    if (grid == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(A.ray_next, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    // The 4-wide walk reads the per-axis copy of its tree (A.hnodes4t): the tight tree's under the whitened test; the
    // M forms walk the shared tree's padded boxes, and so does a whitened scene without a tight tree
    RenderArgs B = A;
    if (F != dev::SecForm::Whitened) B.hnodes4s = A.hnodes4;
    if (T == dev::SecTree::Wide4 && B.hnodes4s == A.hnodes4) B.hnodes4t = A.hnodes4w;
    hipLaunchKernelGGL((dev::secondary_ww_kernel<S, F, T>), dim3((unsigned)grid), dim3(kBlock), 0, stream, B);
    return hipGetLastError();
}

template <bool S, dev::SecForm F>
static hipError_t secondary_launch(const RenderArgs& A, hipStream_t stream) {
    // the 4-wide f16 tree when the scene has one (its leaf boxes are large enough for f16 boxes), else the f32 pairs
    hipError_t e = A.hnodes4 != nullptr ? ww_launch<S, F, dev::SecTree::Wide4>(A, stream)
                                        : ww_launch<S, F, dev::SecTree::PairF32>(A, stream);
    if (e != hipSuccess) return e;
    if (F != dev::SecForm::Pure) {  // PureRayMarching has no first-event-past-the-light quirk, hence no slow path
        hipLaunchKernelGGL(dev::secondary_fix_kernel, dim3(1024), dim3(64), 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        e = secondary_slow_launch(A, stream, S);
    }
    return e;
}

// The form of a frame's secondary rays: PureRayMarching; else the whitened records, or the M forms for a scene with a
// record without a Cholesky factor (A.wrec == nullptr; rare scenes).
template <bool S>
static hipError_t secondary_form_launch(const RenderArgs& A, hipStream_t stream) {
    if (A.pure) return secondary_launch<S, dev::SecForm::Pure>(A, stream);
    if (A.wrec == nullptr) return secondary_launch<S, dev::SecForm::MForm>(A, stream);
    return secondary_launch<S, dev::SecForm::Whitened>(A, stream);
}

hipError_t gauss_secondary(const RenderArgs& A, hipStream_t stream, bool stats) {
    if (A.num_lights + A.env_samples == 0) return hipSuccess;
    if (A.rec_start != nullptr) {  // every record's start subtree (the 4-wide walk with parents only)
        hipLaunchKernelGGL(dev::record_start_kernel, dim3(record_grid(A, 256, 16384)), dim3(256), 0, stream, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (A.env_order != nullptr) {
        // (stats: the instrumented build counts the list filter's work with the persistent kernel's)
        if (stats) hipLaunchKernelGGL((dev::env_order_kernel<true>), dim3(record_grid(A, A.chunk_rec * 4, 4096)), dim3(256), 0, stream, A);
        else hipLaunchKernelGGL((dev::env_order_kernel<false>), dim3(record_grid(A, A.chunk_rec * 4, 4096)), dim3(256), 0, stream, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // stats: the instrumented build of the same persistent kernel (vr_count_work), which counts
    // the work this schedule really does (node steps, list and leaf primitive tests, optical depths)
    return stats ? secondary_form_launch<true>(A, stream) : secondary_form_launch<false>(A, stream);
}

}  // namespace vr
