// The exact slow path of stage 2 of the RayMarchingGaussians pipeline (vr_gauss_common.h): the reference's light
// and environment transmittances on the exactly normalised ray, serial and with the whole wave on one ray, and the
// two kernels that serve the frame's queue of such rays (to_slow, vr_gauss_secondary.hip) through
// secondary_slow_launch.
#include <cstdio>

#include "vr_gauss_common.h"

// Tuning knobs of this unit (A/B builds: tools/ab_build.sh NAME vr_gauss_exact "-DVR_...=...").
#ifndef VR_SLOW_RPW
#define VR_SLOW_RPW 8  // rays per wave of the exact slow path: each ray is a long dependent chain (~250 us), so a wave
                        // of 64 lasts as long as its slowest; 64 / 16 / 12 / 8 / 6 / 4 / 2 / 1 -> 377 / 309 / 273 / 254-270 /
                        // 262 / 276-290 / 306 / 342 us per C4 frame (round 5). (Measured and not kept, round 6: the
                        // persistent kernel's idle waves tracing queued rays in its drain — slow kernel 412 -> 130 us,
                        // but the persistent kernel 76.8 -> 78.9 ms with the slow path's registers in it.)
#endif
#ifndef VR_SLOW_GRID
#define VR_SLOW_GRID 4096  // workgroups of the exact slow path (grid-stride over its queue; 32 k rays a pass at 8 per wave)
#endif
#ifndef VR_SLOW_COOP
#define VR_SLOW_COOP 1  // 1: the wave-cooperative exact slow path on scenes with the 4-wide tree (A/B)
#endif
#ifndef VR_SLOW_COOP_GRID
#define VR_SLOW_COOP_GRID 8192  // one-wave workgroups of the cooperative slow path (one queued ray at a time each)
#endif

namespace vr {
namespace dev {

// ---------------------------------------------------------------------------------------------
// Exact light-ray transmittance (the slow path of Stage 2)
// ---------------------------------------------------------------------------------------------

// Towards a point light at distance `dist` (test_integrators.h:202-237).
template <bool S>
__device__ float light_transmittance(const RenderArgs& A, const Ray& sr, float dist, const ActList& act, int* stack,
                                     int stride, Ctr& c) {
    if (!(dist > 0.0f)) return 1.0f;  // `while (t_prev < dist)` never runs
    const GaussianRecord* __restrict__ G = A.gauss;
    float tau = 0.0f;
    bool needs_stop = false;
    uint64_t hitmask = 0;
    // the 4-wide half-precision tree when the scene has one (half the dependent node fetches of the
    // f32 pair tree; boxes only propose candidates, every decision is the exact quadratic), the pair
    // tree when it has not or when a 4-wide walk could overflow its stack (`reset` undoes the partial walk)
    auto walk = [&](auto prune, auto leaf, auto reset) {
        if (A.hnodes4 != nullptr) {
            if (traverse_wide<kStackSize>(A, sr, stack, stride, prune, leaf, NodeCount<S>{&c})) return;
            reset();
        }
        traverse<false>(A, sr, stack, stride, prune, leaf, NodeCount<S>{&c});
    };
    walk(
        [&](float tmin, float) { return tmin <= dist + kTPad * (1.0f + dist); },
        [&](uint32_t first, uint32_t count) {
            for (uint32_t j = first; j < first + count; ++j) {
                if constexpr (S) c.v[kCtrPrims]++;
                GRec g = load_rec(G, j);
                Quad q = quad(g, sr);
                float a, b;
                if (!intersect(q, a, b)) continue;
                int slot = act.find((int)j);
                float lo = a;
                if (slot >= 0) {
                    lo = 0.0f;
                    hitmask |= slot_bit(slot);
                }
                if (b < dist) {
                    if constexpr (S) c.v[kCtrOD]++;
                    tau += optical_depth(g, q, lo, b);
                } else if (lo < dist) {
                    needs_stop = true;  // straddles the light: needs the stopping event
                }
            }
            return tau < kTauCut;
        },
        [&]() {
            tau = 0.0f;
            needs_stop = false;
            hitmask = 0;
        });
    uint64_t all = act.n >= 64 ? ~0ull : ((1ull << act.n) - 1ull);
    uint64_t missed = all & ~hitmask;  // pre-activated but not intersected (rounding at the surface)
    if (tau >= kTauCut) return 0.0f;   // exp(-tau) == 0 exactly; later terms are >= 0
    // more than 64 active Gaussians: a member is missed iff the ray does not intersect it
    auto deep_missed = [&](int s, GRec& g, Quad& q) {
        float a, b;
        g = load_rec(G, act.get(s));
        q = quad(g, sr);
        return !intersect(q, a, b);
    };
    bool deep_any = false;
    if (act.n > 64) {
        missed = 0;
        for (int s = 0; s < act.n && !deep_any; ++s) {
            GRec g;
            Quad q;
            deep_any = deep_missed(s, g, q);
        }
    }
    if (needs_stop || missed || deep_any) {
        float tstop = INFINITY;  // first event at or beyond the light
        walk(
            [&](float tmin, float tmax) {
                return tmax >= dist - kTPad * (1.0f + dist) && tmin <= tstop + kTPad * (1.0f + tstop);
            },
            [&](uint32_t first, uint32_t count) {
                for (uint32_t j = first; j < first + count; ++j) {
                    if constexpr (S) c.v[kCtrPrims]++;
                    GRec g = load_rec(G, j);
                    Quad q = quad(g, sr);
                    float a, b;
                    if (!intersect(q, a, b)) continue;
                    if (b >= dist) tstop = fminf(tstop, (a >= dist) ? a : b);
                }
                return true;
            },
            [&]() { tstop = INFINITY; });
        if (tstop == INFINITY) tstop = dist;
        if (needs_stop) {
            const float tau0 = tau;
            walk(
                [&](float tmin, float tmax) {
                    return tmin <= dist + kTPad * (1.0f + dist) && tmax >= dist - kTPad * (1.0f + dist);
                },
                [&](uint32_t first, uint32_t count) {
                    for (uint32_t j = first; j < first + count; ++j) {
                        if constexpr (S) c.v[kCtrPrims]++;
                        GRec g = load_rec(G, j);
                        Quad q = quad(g, sr);
                        float a, b;
                        if (!intersect(q, a, b)) continue;
                        float lo = act.find((int)j) >= 0 ? 0.0f : a;
                        if (lo < dist && b >= dist) {
                            if constexpr (S) c.v[kCtrOD]++;
                            tau += optical_depth(g, q, lo, tstop);
                        }
                    }
                    return tau < kTauCut;
                },
                [&]() { tau = tau0; });
        }
        while (missed) {
            int s = __ffsll((unsigned long long)missed) - 1;
            missed &= missed - 1;
            GRec g = load_rec(G, act.get(s));
            Quad q = quad(g, sr);
            if constexpr (S) c.v[kCtrOD]++;
            tau += optical_depth(g, q, 0.0f, tstop);
        }
        if (deep_any)
            for (int s = 0; s < act.n; ++s) {
                GRec g;
                Quad q;
                if (deep_missed(s, g, q)) tau += optical_depth(g, q, 0.0f, tstop);
            }
    }
    return expf(-tau);
}

// Exact environment-ray transmittance (test_integrators.h:242-271): the record's active Gaussians are
// pre-activated at t = 0, every event comes from the exact intersect on the exactly normalised ray, so a
// member's decision matches the reference bit for bit: a member the ray crosses is active on [0, t1], a member
// it misses (t1 < 0 through rounding) stays active to the ray's last event, any other Gaussian on [t0, t1].
// For the rare environment rays whose whitened member test sits at the decision boundary (sec_finish).
template <bool S>
__device__ float env_transmittance(const RenderArgs& A, const Ray& er, const ActList& act, int* stack, int stride, Ctr& c) {
    const GaussianRecord* __restrict__ G = A.gauss;
    float tau = 0.0f, t_last = 0.0f;
    uint64_t hitmask = 0;
    auto walk = [&](auto prune, auto leaf, auto reset) {
        if (A.hnodes4 != nullptr) {
            if (traverse_wide<kStackSize>(A, er, stack, stride, prune, leaf, NodeCount<S>{&c})) return;
            reset();
        }
        traverse<false>(A, er, stack, stride, prune, leaf, NodeCount<S>{&c});
    };
    walk([&](float, float) { return true; },
         [&](uint32_t first, uint32_t count) {
             for (uint32_t j = first; j < first + count; ++j) {
                 if constexpr (S) c.v[kCtrPrims]++;
                 const GRec g = load_rec(G, j);
                 const Quad q = quad(g, er);
                 float a, b;
                 if (!intersect(q, a, b)) continue;
                 t_last = fmaxf(t_last, b);  // (entries come before their exits)
                 const int slot = act.find((int)j);
                 if (slot >= 0) hitmask |= slot_bit(slot);
                 if constexpr (S) c.v[kCtrOD]++;
                 tau += optical_depth(g, q, slot >= 0 ? 0.0f : a, b);
             }
             // the whole walk (a missed member needs the last event) unless Tr is already 0: expf(-tau) == 0
             // in f32 from tau >= 104, and later terms (the missed members' too) only add to tau
             return tau < 104.0f;
         },
         [&]() {
             tau = t_last = 0.0f;
             hitmask = 0;
         });
    for (int s = 0; s < act.n; ++s) {  // members the ray misses: active to the last event
        if (s < 64 && ((hitmask >> s) & 1ull)) continue;
        const GRec g = load_rec(G, act.get(s));
        const Quad q = quad(g, er);
        float a, b;
        if (s >= 64 && intersect(q, a, b)) continue;
        if constexpr (S) c.v[kCtrOD]++;
        tau += optical_depth(g, q, 0.0f, t_last);
    }
    return expf(-tau);
}

// ---------------------------------------------------------------------------------------------
// The same exact transmittances with the whole wave on one ray (the slow path, round 6). A serial walk of one
// long ray is a chain of ~100 dependent node and record loads (~250-400 us); here the wave expands the walk one
// tree level at a time — each lane one frontier node (its four child boxes), the hit inner children appended to
// the next level and the hit leaves to a list in lane order (ballots: a deterministic order), then each lane
// one listed leaf's primitives — so the chain is the tree's depth. Every Gaussian the serial walk tests is
// tested (no prune is tighter), with the same exact M forms; only the order of the optical-depth sum differs
// (per-lane partial sums, then a fixed butterfly). kCoopCap nodes or leaves per level at most: a wider level
// (never seen at C4) falls back to the serial walk on lane 0.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kCoopCap = 256;
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ float wave_min(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ uint64_t wave_or(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
        x |= ((uint64_t)hi << 32) | lo;
    }
    return x;
}
// Level-by-level walk of the 4-wide tree by the whole wave (every lane calls it with the same ray); leaf(j) runs
// for every primitive of every hit leaf, on the lane the leaf fell to. False: a level outgrew kCoopCap.
template <typename Prune, typename Leaf>
__device__ bool coop_walk(const RenderArgs& A, const Ray& r0, int* buf, Prune prune, Leaf leaf) {
    float ox = r0.ox, oy = r0.oy, oz = r0.oz;
    node_space<true>(A, ox, oy, oz);
    auto inv = [&](float d) {
        d *= A.hn_scale;
        return __frcp_rn(fabsf(d) > 1e-30f ? d : copysignf(1e-30f, d));
    };
    const float ix = inv(r0.dx), iy = inv(r0.dy), iz = inv(r0.dz);
    const float oxi = ox * ix, oyi = oy * iy, ozi = oz * iz;
    const uint32_t lane = __lane_id();
    int* cur = buf;
    int* nxt = buf + kCoopCap;
    int* lv = buf + 2 * kCoopCap;
    if (lane == 0) cur[0] = 0;
    __builtin_amdgcn_wave_barrier();
    uint32_t n = 1;
    while (n > 0) {
        uint32_t nn = 0, nl = 0;
        for (uint32_t base = 0; base < n; base += 64u) {
            const bool valid = base + lane < n;
            float key[4];
            int32_t kr[4] = {0, 0, 0, 0};
            if (valid) wide_children<Prune, false>(A, cur[base + lane], ix, iy, iz, oxi, oyi, ozi, prune, key, kr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t bi = __ballot(kr[k] > 0), bl = __ballot(kr[k] < 0);
                const uint32_t ci = (uint32_t)__popcll(bi), cl = (uint32_t)__popcll(bl);
                if (nn + ci > kCoopCap || nl + cl > kCoopCap) return false;
                const uint64_t below = (1ull << lane) - 1ull;
                if (kr[k] > 0) nxt[nn + (uint32_t)__popcll(bi & below)] = kr[k];
                if (kr[k] < 0) lv[nl + (uint32_t)__popcll(bl & below)] = kr[k];
                nn += ci;
                nl += cl;
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t base = 0; base < nl; base += 64u)
            if (base + lane < nl) {
                const int32_t ref = lv[base + lane];
                for (uint32_t j = leaf_first(ref); j < leaf_first(ref) + leaf_count(ref); ++j) leaf(j);
            }
        __builtin_amdgcn_wave_barrier();
        int* t = cur;
        cur = nxt;
        nxt = t;
        n = nn;
    }
    return true;
}

// light_transmittance with the wave on one ray (test_integrators.h:202-237): the three passes as there.
template <bool S>
__device__ float light_transmittance_coop(const RenderArgs& A, const Ray& sr, float dist, const ActList& act, int* buf,
                                          Ctr& c, bool& ok) {
    ok = true;
    if (!(dist > 0.0f)) return 1.0f;
    const GaussianRecord* __restrict__ G = A.gauss;
    const float pad = kTPad * (1.0f + dist);
    float tau = 0.0f;
    bool needs_stop = false;
    uint64_t hitmask = 0;
    ok = coop_walk(
        A, sr, buf, [&](float tmin, float) { return tmin <= dist + pad; },
        [&](uint32_t j) {
            if constexpr (S) c.v[kCtrPrims]++;
            const GRec g = load_rec(G, (int)j);
            const Quad q = quad(g, sr);
            float a, b;
            if (!intersect(q, a, b)) return;
            const int slot = act.find((int)j);
            float lo = a;
            if (slot >= 0) {
                lo = 0.0f;
                hitmask |= slot_bit(slot);
            }
            if (b < dist) {
                if constexpr (S) c.v[kCtrOD]++;
                tau += optical_depth(g, q, lo, b);
            } else if (lo < dist) {
                needs_stop = true;
            }
        });
    if (!ok) return 0.0f;
    tau = wave_sum(tau);
    hitmask = wave_or(hitmask);
    needs_stop = __any(needs_stop);
    if (tau >= kTauCut) return 0.0f;  // exp(-tau) == 0 exactly; later terms are >= 0
    const uint64_t all = act.n >= 64 ? ~0ull : ((1ull << act.n) - 1ull);
    uint64_t missed = all & ~hitmask;
    bool deep_any = false;
    if (act.n > 64) {  // a member is missed iff the ray does not intersect it
        missed = 0;
        for (int s = 0; s < act.n && !deep_any; ++s) {
            float a, b;
            deep_any = !intersect(quad(load_rec(G, act.get(s)), sr), a, b);
        }
    }
    if (needs_stop || missed || deep_any) {
        float tstop = INFINITY;  // first event at or beyond the light
        ok = coop_walk(
            A, sr, buf, [&](float, float tmax) { return tmax >= dist - pad; },
            [&](uint32_t j) {
                if constexpr (S) c.v[kCtrPrims]++;
                const GRec g = load_rec(G, (int)j);
                float a, b;
                if (!intersect(quad(g, sr), a, b)) return;
                if (b >= dist) tstop = fminf(tstop, (a >= dist) ? a : b);
            });
        if (!ok) return 0.0f;
        tstop = wave_min(tstop);
        if (tstop == INFINITY) tstop = dist;
        if (needs_stop) {
            float t3 = 0.0f;
            ok = coop_walk(
                A, sr, buf, [&](float tmin, float tmax) { return tmin <= dist + pad && tmax >= dist - pad; },
                [&](uint32_t j) {
                    if constexpr (S) c.v[kCtrPrims]++;
                    const GRec g = load_rec(G, (int)j);
                    const Quad q = quad(g, sr);
                    float a, b;
                    if (!intersect(q, a, b)) return;
                    const float lo = act.find((int)j) >= 0 ? 0.0f : a;
                    if (lo < dist && b >= dist) {
                        if constexpr (S) c.v[kCtrOD]++;
                        t3 += optical_depth(g, q, lo, tstop);
                    }
                });
            if (!ok) return 0.0f;
            tau += wave_sum(t3);
        }
        while (missed) {
            const int s = __ffsll((unsigned long long)missed) - 1;
            missed &= missed - 1;
            const GRec g = load_rec(G, act.get(s));
            tau += optical_depth(g, quad(g, sr), 0.0f, tstop);
        }
        if (deep_any)
            for (int s = 0; s < act.n; ++s) {
                const GRec g = load_rec(G, act.get(s));
                const Quad q = quad(g, sr);
                float a, b;
                if (!intersect(q, a, b)) tau += optical_depth(g, q, 0.0f, tstop);
            }
    }
    return expf(-tau);
}

// env_transmittance with the wave on one ray (test_integrators.h:242-271).
template <bool S>
__device__ float env_transmittance_coop(const RenderArgs& A, const Ray& er, const ActList& act, int* buf, Ctr& c, bool& ok) {
    const GaussianRecord* __restrict__ G = A.gauss;
    float tau = 0.0f, t_last = 0.0f;
    uint64_t hitmask = 0;
    ok = coop_walk(
        A, er, buf, [&](float, float) { return true; },
        [&](uint32_t j) {
            if constexpr (S) c.v[kCtrPrims]++;
            const GRec g = load_rec(G, (int)j);
            const Quad q = quad(g, er);
            float a, b;
            if (!intersect(q, a, b)) return;
            t_last = fmaxf(t_last, b);
            const int slot = act.find((int)j);
            if (slot >= 0) hitmask |= slot_bit(slot);
            if constexpr (S) c.v[kCtrOD]++;
            tau += optical_depth(g, q, slot >= 0 ? 0.0f : a, b);
        });
    if (!ok) return 0.0f;
    tau = wave_sum(tau);
    t_last = wave_max(t_last);
    hitmask = wave_or(hitmask);
    for (int s = 0; s < act.n; ++s) {  // members the ray misses: active to the last event
        if (s < 64 && ((hitmask >> s) & 1ull)) continue;
        const GRec g = load_rec(G, act.get(s));
        const Quad q = quad(g, er);
        float a, b;
        if (s >= 64 && intersect(q, a, b)) continue;
        tau += optical_depth(g, q, 0.0f, t_last);
    }
    return expf(-tau);
}

// ---------------------------------------------------------------------------------------------
// The kernels that serve the slow-path queue
// ---------------------------------------------------------------------------------------------
// One queued ray of the exact slow path on one lane (result slot t: decode_queued_ray). True: a light ray.
template <bool S>
__device__ bool slow_ray(const RenderArgs& A, uint64_t t, int* stack, int stride, Ctr& c) {
    const QueuedRay q = decode_queued_ray(A, t);
    if (q.light) A.tr[t] = light_transmittance<S>(A, q.ray, q.dist, q.act, stack, stride, c);
    else A.tr[t] = env_transmittance<S>(A, q.ray, q.act, stack, stride, c);
    return q.light;
}

// The instrumented slow kernels' counters into the secondary stage's totals: each lane adds its own non-zero ones.
__device__ __forceinline__ void flush_lane_counters(const RenderArgs& A, const Ctr& c) {
    for (int i = 0; i < kNumCtr; ++i)
        if (c.v[i]) atomicAdd(A.work + kNumCtr + i, (unsigned long long)c.v[i]);
}

#ifdef VR_DIAG_SLOW
__device__ uint32_t g_slow_hist[2][16], g_slow_max[2], g_slow_done;
#endif
// Exact three-pass light transmittance for the queued rays (see light_transmittance).
template <int BLOCK, bool S>
__global__ __launch_bounds__(BLOCK) void secondary_slow_kernel(RenderArgs A) {
    __shared__ int s_stack[kStackSize * BLOCK];
    int* stack = s_stack + threadIdx.x;
    const uint32_t n = min(A.slowq[0], A.slowq_cap);
    Ctr c{};
#ifdef VR_DIAG_SLOW  // diagnostic builds only: a histogram of the rays' latencies, printed by the last block
    uint32_t my_max = 0;
#endif
    // VR_SLOW_RPW rays per wave (the rest of its lanes idle): a wave lasts as long as its slowest ray. A queue
    // longer than one pass at that rate (many chord-band rays) takes as many lanes per wave as one pass needs
    // (a power of two up to 64): a second pass would cost a whole ray chain again.
    const uint32_t lane = threadIdx.x % 64u, wave = (blockIdx.x * BLOCK + threadIdx.x) / 64u;
    const uint32_t waves = gridDim.x * (BLOCK / 64u);
    uint32_t rpw = VR_SLOW_RPW;
    while (rpw < 64u && (uint64_t)waves * rpw < n) rpw *= 2u;
    const uint32_t q0 = lane < rpw ? wave * rpw + lane : n;
    for (uint32_t q = q0; q < n; q += waves * rpw) {
#ifdef VR_DIAG_SLOW
        const uint64_t t_beg = wall_clock64();
#endif
        [[maybe_unused]] const bool light = slow_ray<S>(A, A.slowq[1 + q], stack, BLOCK, c);
#ifdef VR_DIAG_SLOW
        const uint32_t us = (uint32_t)((wall_clock64() - t_beg) / 100);  // 100 MHz constant clock
        const int kind = light;
        atomicAdd(&g_slow_hist[kind][min(31 - __clz(us | 1), 15)], 1u);
        atomicMax(&g_slow_max[kind], us);
        my_max = max(my_max, us);
#endif
    }
#ifdef VR_DIAG_SLOW
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&g_slow_done, 1u) == gridDim.x - 1) {
            printf("slowq n=%u grid=%u max_us env %u light %u\n", n, gridDim.x, atomicAdd(&g_slow_max[0], 0u), atomicAdd(&g_slow_max[1], 0u));
            for (int k = 0; k < 2; ++k)
                for (int b = 0; b < 16; ++b) {
                    const uint32_t v = atomicExch(&g_slow_hist[k][b], 0u);
                    if (v) printf("  %s us<%u: %u\n", k ? "light" : "env", 2u << b, v);
                }
            atomicExch(&g_slow_max[0], 0u);
            atomicExch(&g_slow_max[1], 0u);
            atomicExch(&g_slow_done, 0u);
        }
    }
#endif
    if constexpr (S) flush_lane_counters(A, c);
}

// The exact slow path with the wave on one ray at a time (coop_walk; scenes with the 4-wide tree): the queue's
// rays one per wave, so a ray's latency is the tree's depth in node and record loads instead of its whole walk.
template <bool S>
__global__ __launch_bounds__(64) void secondary_slow_coop_kernel(RenderArgs A) {
    __shared__ int s_buf[3 * kCoopCap];
    const uint32_t n = min(A.slowq[0], A.slowq_cap);
    const uint32_t lane = __lane_id();
    Ctr c{};
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const uint64_t t = A.slowq[1 + q];
        const QueuedRay qr = decode_queued_ray(A, t);
        bool ok = true;
        float tr;
        if (qr.light) {
            tr = light_transmittance_coop<S>(A, qr.ray, qr.dist, qr.act, s_buf, c, ok);
            __builtin_amdgcn_wave_barrier();
            if (!ok && lane == 0) tr = light_transmittance<S>(A, qr.ray, qr.dist, qr.act, s_buf, 1, c);  // a level over kCoopCap
        } else {
            tr = env_transmittance_coop<S>(A, qr.ray, qr.act, s_buf, c, ok);
            __builtin_amdgcn_wave_barrier();
            if (!ok && lane == 0) tr = env_transmittance<S>(A, qr.ray, qr.act, s_buf, 1, c);
        }
        if (lane == 0) A.tr[t] = tr;
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (S) flush_lane_counters(A, c);
}

}  // namespace dev

// ---------------------------------------------------------------------------------------------
// Host launcher (secondary_launch calls it after the persistent kernel and the fix-up)
// ---------------------------------------------------------------------------------------------
template <bool S>
static hipError_t slow_launch(const RenderArgs& A, hipStream_t stream) {
    if (VR_SLOW_COOP && A.hnodes4 != nullptr)
        hipLaunchKernelGGL(dev::secondary_slow_coop_kernel<S>, dim3(VR_SLOW_COOP_GRID), dim3(64), 0, stream, A);
    else
        hipLaunchKernelGGL((dev::secondary_slow_kernel<64, S>), dim3(VR_SLOW_GRID), dim3(64), 0, stream, A);
    return hipGetLastError();
}

hipError_t secondary_slow_launch(const RenderArgs& A, hipStream_t stream, bool stats) {
    return stats ? slow_launch<true>(A, stream) : slow_launch<false>(A, stream);
}

}  // namespace vr
