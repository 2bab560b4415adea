// The free-flight integrators' kernels: the two persistent path kernels (a bounce per wave iteration, and
// phase-scheduled), the fallback for paths over the row capacity, the shadow-ray kernel, the accumulation, and
// their launcher. The per-path helpers and ff_bounce are vr_ff_bounce.h.
#include "vr_ff_bounce.h"

namespace vr {
namespace dev {

// Persistent: a grid of resident waves; every lane follows one path a bounce per wave iteration and,
// once its path is complete, starts the next unclaimed path of the launch (claimed per wave when
// kFFRefill lanes are idle), so a wave never waits for its longest path. Launch bounds: 4 waves/SIMD
// (128 VGPRs, some spills) measured faster than 2, 3 and 5.
#ifndef VR_FF_WAVES
#define VR_FF_WAVES 4  // waves per SIMD of the path kernel (launch bounds; the grid fills them)
#endif
// CNT: the instrumented build (vr_count_work) counts its work into A.work[0..7].
#ifndef VR_FF_REFILL
#define VR_FF_REFILL 16  // idle lanes of a wave that trigger its path refill
#endif
template <bool MULTI, bool CNT = false>
__global__ void __launch_bounds__(kFFBlock, VR_FF_WAVES) ff_path_kernel(RenderArgs A) {
    __shared__ int s_stack[(kStackSize + kCollectQueue) * kFFBlock];  // walk stack + the walks' leaf FIFO
    int* stack = s_stack + threadIdx.x;
    const uint32_t gt = blockIdx.x * kFFBlock + threadIdx.x;
    FFScratch<CNT> S = ff_thread_scratch<CNT>(A, gt);
    const uint32_t lane = threadIdx.x & 63u;
    FFPath P{PCG32(0, 1)};
    bool live = false, exhausted = false;
    for (;;) {
        const uint64_t idle = __ballot(!live);
        if (!exhausted && (idle == ~0ull || __popcll(idle) >= VR_FF_REFILL)) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(A.ff_next, (unsigned long long)__popcll(idle));
            base = __shfl(base, 0, 64);
            exhausted = base + (unsigned long long)__popcll(idle) >= A.ff_total;
            if (!live) {
                const unsigned long long pid =
                    base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (pid < A.ff_total) {
                    S.C.add(kFFPaths);
                    live = ff_start(A, (uint32_t)pid, P);
                }
            }
        }
        if (!__any(live)) {
            if (exhausted) break;
            continue;
        }
        if (live) live = ff_bounce<MULTI>(A, S, stack, P);
    }
    if constexpr (CNT) {
        Ctr c{};
        for (int i = 0; i < kFFNumCtr; ++i) c.v[i] = S.C.v[i];
        flush_counters(A.work, c);
    }
}

// Phase-scheduled persistent path kernel. ff_path_kernel runs a whole bounce per wave iteration, so a
// wave waits at every phase for its slowest lane (the hit collection of one lane's second window, the
// event sweep of the lane with the most events, the shading of the lanes that scattered). Here every
// lane carries its path's bounce as a state (COLLECT: the resumable while-while walk of the window's hit
// collection; SWEEP: the window's events, one (or a budget of) per iteration; SHADE: the distance solver,
// the albedo and the rest of the bounce), and each wave iteration runs the ONE phase most of the wave's
// lanes are in, with those lanes only. Every path runs ff_bounce's operations in ff_bounce's order (the
// same RNG draws, sums and decisions), so frames are the persistent kernel's, bit for bit.
#ifndef VR_FFSM_EVENT_BUDGET
#define VR_FFSM_EVENT_BUDGET 24  // active-entry evaluations a lane may spend on events per SWEEP iteration (0: one event)
#endif
// The sweep reads an entry's row once and the next active entry's rows one ahead, and recomputes F at each segment
// start instead of keeping it in the rows. (Measured and not kept: the PRIM iterations reading the next Gaussian one
// step ahead, 134.8 vs 134.3 ms at C2.)
#ifndef VR_FFSM_SHADE_MIN
#define VR_FFSM_SHADE_MIN 20  // SHADE runs when it has the most lanes and at least this many (or nothing else is left)
#endif
#ifndef VR_FFSM_WAVES
#define VR_FFSM_WAVES 4  // waves per SIMD of the phase-scheduled path kernel (launch bounds)
#endif
enum : int { kSmIdle = 0, kSmCollect = 1, kSmSweep = 2, kSmShade = 3 };
template <bool MULTI, bool CNT = false>
__global__ void __launch_bounds__(kFFBlock, VR_FFSM_WAVES) ff_path_sm_kernel(RenderArgs A) {
    using Acc = typename std::conditional<MULTI, double, float>::type;
    __shared__ int s_stack[(kStackSize + kCollectQueue) * kFFBlock];  // walk stack + the walks' leaf FIFO
    int* stack = s_stack + threadIdx.x;
    int* ring = stack + kStackSize * kFFBlock;
    const uint32_t gt = blockIdx.x * kFFBlock + threadIdx.x;
    FFScratch<CNT> S = ff_thread_scratch<CNT>(A, gt);
    const uint32_t lane = threadIdx.x & 63u;
    FFPath P{PCG32(0, 1)};
    int phase = kSmIdle;
    bool exhausted = false;
    // the bounce (free_flight_distance's state across windows)
    float target = 0.0f, t_prev = 0.0f, W0 = 0.0f;
    Acc acc = 0;
    int cap = 0;
    // the window's hit collection (its walk: WideWalk, vr_walk.h); in SHADE, t_cut holds ts (m < 0) or
    // the scatter segment's end t_evt, and kfull the target left on that segment
    int n = 0;
    float t_cut = INFINITY, kfull = INFINITY, klast = 0.0f;
    WideWalk<kCollectQueue> w;
    w.start(false);
    bool redo = false;  // no 4-wide tree, or its stack could overflow: the pair-tree walk at completion
    // the window's event sweep
    int i = 0, m = 0, exit_pos = -1;
    float next_exit = INFINITY;
    auto begin_window = [&]() {
        n = 0;
        t_cut = kfull = INFINITY;
        redo = A.hnodes4 == nullptr;  // no 4-wide tree: the pair-tree walk at once
        w.start(!redo);
        phase = kSmCollect;
    };
    auto begin_bounce = [&]() {  // ff_bounce's start: the target draw, window 0 from t = 0
        target = -logf(1.0f - P.rng.uniform());
        S.C.add(kFFBounces);
        acc = 0;
        t_prev = W0 = 0.0f;
        cap = A.ff_hit_cap0;
        begin_window();
    };
    auto to_shade = [&](float ts) {
        m = -1;
        t_cut = ts;
        phase = kSmShade;
    };
    auto prune = [&](float tmin, float tmax) {
        if (tmax < W0 - kTPad * (1.0f + W0)) return false;
        const float lim = fminf(t_cut, kfull);
        return !(tmin > lim + kTPad * (1.0f + fminf(lim, 1e30f)));
    };
    auto prim_g = [&](uint32_t jj, const GRec& g) {  // free_flight_distance's insertion, term for term
        S.C.add(kFFPrims);
        float t0, t1;
        if (!intersect(quad(g, P.ray), t0, t1)) return;
        if (!(t0 <= t1)) return;
        if (W0 > 0.0f && !(t1 > W0)) return;
        const float key = fmaxf(t0, W0);
        if (key >= t_cut) return;
        if (n == cap) {
            if (key >= kfull) {
                t_cut = fminf(t_cut, key);
                return;
            }
            t_cut = fminf(t_cut, kfull);
            --n;
            if (n > 0) klast = S.K(n - 1);  // (the evicted entry was the largest)
        }
        // klast = the largest kept key (the last row): an entry in walk order past it is appended without
        // reading the rows back (the rows live in global memory: a read there is a dependent round trip)
        int p = n;
        if (n > 0 && klast > key) {
            while (p > 0) {
                const float4 prev = S.H(p - 1);
                if (!(prev.x > key)) break;
                S.H(p) = prev;
                --p;
            }
        } else {
            klast = key;
        }
        S.H(p) = make_float4(key, t1, __int_as_float((int)jj), 0.0f);
        ++n;
        if (n == cap) kfull = klast;
    };
    auto prim = [&](uint32_t jj) { prim_g(jj, load_rec(A.gauss, (int)jj)); };
    for (;;) {
        const uint64_t idle = __ballot(phase == kSmIdle);
        if (!exhausted && (idle == ~0ull || __popcll(idle) >= VR_FF_REFILL)) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(A.ff_next, (unsigned long long)__popcll(idle));
            base = __shfl(base, 0, 64);
            exhausted = base + (unsigned long long)__popcll(idle) >= A.ff_total;
            if (phase == kSmIdle) {
                const unsigned long long pid =
                    base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (pid < A.ff_total) {
                    S.C.add(kFFPaths);
                    if (ff_start(A, (uint32_t)pid, P)) begin_bounce();
                }
            }
        }
        const int nc = __popcll(__ballot(phase == kSmCollect)), ns = __popcll(__ballot(phase == kSmSweep)),
                  nh = __popcll(__ballot(phase == kSmShade));
        if (nc + ns + nh == 0) {
            if (exhausted) break;
            continue;
        }
        const bool shade_now = nh >= VR_FFSM_SHADE_MIN ? (nh >= ns && nh >= nc) : (ns + nc == 0);
#ifdef VR_DIAG_FFSM  // (CNT builds) lane 0 of each wave: cycles/16 of each phase [0..2], its iterations [3..5], and the
        // lanes it ran with, COLLECT [6] and SWEEP [7] (SHADE's are the bounces)
        // (VR_DIAG_FFSM=2: cycles/16 of NODE, PRIM, SWEEP, SHADE iterations [0..3] and their counts [4..7])
        const int dphase = shade_now ? 2 : (ns >= nc ? 1 : 0);
        const uint64_t dt0 = __builtin_amdgcn_s_memtime();
        bool dnode = false;
#endif
        if (shade_now) {
            // ---- SHADE: ff_bounce after free_flight_distance, term for term ----
            if (phase == kSmShade) {
                float ts = t_cut;
                const int ma = m;
                if (ma >= 0) {  // the scatter lies in [t_prev, t_cut] with kfull of the target left
                    S.ph = 0;  // the solver reads F at the segment start from .x
                    for (int a = 0; a < ma; ++a) {
                        const float4 c = S.A0(a);
                        reinterpret_cast<float*>(&S.A1(a))[0] = erff(__fdiv_rn(c.y + c.z * t_prev, c.w));
                    }
                    const uint64_t useed = A.ff_solver == kSolverUniform ? ff_path_seed(A, P.out) : 0ull;
                    ts = solve_distance(A, S, ma, P.ray, t_prev, t_cut, kfull, useed, P.bounce);
                }
                bool done = false, requeued = false;
                if (MULTI && A.rec_bits && ts != -2.0f)
                    record_hits(A, P.ray, ts >= 0.0f ? ts + 1e-6f : INFINITY, P.px, stack, kFFBlock);
                if (ts == -2.0f && A.ff_fbq != nullptr) {  // over the hit-buffer capacity: the whole path re-runs
                    const uint32_t q = atomicAdd(A.ff_fbq, 1u);  // in ff_fallback_kernel with larger rows
                    atomicAdd(A.counters + 2, 1u);
                    if (q < A.ff_fbq_cap) {
                        A.ff_fbq[1 + q] = P.out;
                        A.ff_tail[P.out] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kFFNone));
                        requeued = true;
                    }
                }
                if (requeued) {
                    done = true;
                } else if (ts == -2.0f || P.bounce >= A.ff_max_bounces) {
                    P.L0 = P.L1 = P.L2 = __builtin_nanf("");
                    P.after = true;
                    atomicAdd(A.counters, 1u);
                    done = true;
                } else if (ts < 0.0f) {  // no event, or no scatter before the last event: environment
                    P.L0 += P.tp0 * A.env[0];
                    P.L1 += P.tp1 * A.env[1];
                    P.L2 += P.tp2 * A.env[2];
                    P.after |= P.first != kFFNone;
                    done = true;
                } else {
                    const float px = P.ray.ox + ts * P.ray.dx, py = P.ray.oy + ts * P.ray.dy, pz = P.ray.oz + ts * P.ray.dz;
                    const float albedo = evaluate_albedo(A, S, ma, px, py, pz);
                    const int nl = A.num_lights;
                    const bool is_env = P.rng.uniform() < __fdiv_rn(1.0f, (float)(nl + 1));
                    int li = -1;
                    float dist = INFINITY;
                    Ray sr;
                    if (!is_env) {
                        li = (int)(P.rng.uniform() * (float)nl);
                        const LightRecord& Lt = A.lights[li];
                        float wx = Lt.px - px, wy = Lt.py - py, wz = Lt.pz - pz;
                        dist = sqrtf(dot3(wx, wy, wz, wx, wy, wz));
                        normalize3(wx, wy, wz);
                        sr = make_ray(px, py, pz, wx, wy, wz);
                    } else {
                        float wx, wy, wz;
                        sample_uniform_direction(P.rng, wx, wy, wz);
                        sr = make_ray(px, py, pz, wx, wy, wz);
                    }
                    const float w = (albedo * kInv4Pi) * (float)(nl + 1);
                    const float m0 = MULTI ? P.tp0 * w : w, m1 = MULTI ? P.tp1 * w : w, m2 = MULTI ? P.tp2 * w : w;
                    const bool queued = nee_queue(A, sr, dist, li, m0, m1, m2, P.first, P.last, P.defer);
                    S.C.add(queued ? kFFNeeQueued : kFFNeeInline);
                    if (!queued) {
                        float Li0, Li1, Li2;
                        nee_radiance(A, transmittance_up_to(A, sr, dist, stack, kFFBlock), li, dist, Li0, Li1, Li2);
                        P.after |= P.first != kFFNone;
                        if constexpr (!MULTI) {
                            P.L0 = m0 * Li0;
                            P.L1 = m1 * Li1;
                            P.L2 = m2 * Li2;
                        } else {
                            P.L0 += m0 * Li0;
                            P.L1 += m1 * Li1;
                            P.L2 += m2 * Li2;
                        }
                    }
                    if constexpr (!MULTI) {
                        done = true;
                    } else {
                        P.tp0 *= albedo;
                        P.tp1 *= albedo;
                        P.tp2 *= albedo;
                        if (P.bounce >= A.ff_min_bounces) {  // integrator.h:691-695
                            const float rr = fminf(fmaxf(P.tp0, fmaxf(P.tp1, P.tp2)), 0.9f);
                            if (P.rng.uniform() > rr) {
                                done = true;
                            } else {
                                P.tp0 = __fdiv_rn(P.tp0, rr);
                                P.tp1 = __fdiv_rn(P.tp1, rr);
                                P.tp2 = __fdiv_rn(P.tp2, rr);
                            }
                        }
                        if (!done) {
                            float nx, ny, nz;
                            sample_uniform_direction(P.rng, nx, ny, nz);
                            P.ray = make_ray(px, py, pz, nx, ny, nz);
                            ++P.bounce;
                        }
                    }
                }
                if (done) {
                    if (!requeued)
                        A.ff_tail[P.out] = make_float4(P.L0, P.L1, P.L2, __uint_as_float(P.first | (P.after ? kFFTailAfter : 0u)));
                    phase = kSmIdle;
                } else {
                    begin_bounce();
                }
            }
        } else if (ns >= nc) {
            // ---- SWEEP: free_flight_distance's event sweep, term for term ----
            int budget = VR_FFSM_EVENT_BUDGET;
            bool go = phase == kSmSweep;
            while (go) {
                budget -= max(m, 1);
                const float4 hn = i < n ? S.H(i) : make_float4(INFINITY, 0.0f, 0.0f, 0.0f);  // (the entry's row, once)
                const float next_entry = hn.x;
                float t_evt = fminf(next_entry, next_exit);
                const bool window_end = t_cut <= t_evt;
                if (window_end) t_evt = t_cut;
                if (t_evt == INFINITY) {  // past the last event: no scatter (integrator.h:362-366)
                    to_shade(-1.0f);
                    break;
                }
                const bool is_entry = next_entry <= next_exit;
                float nx = INFINITY;
                int npos = -1;
                Acc seg = 0;
                // F at the segment start recomputed (the cached value's own float operations: bit-identical),
                // so the sweep reads 20 B per active entry and writes nothing; the next entry's read in flight
                float4 cn = m > 0 ? S.A0(0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                float tn = m > 0 ? S.T1(0) : 0.0f;
#pragma unroll 1
                for (int a = 0; a < m; ++a) {
                    const float4 c = cn;
                    const float t1a = tn;
                    if (a + 1 < m) {
                        cn = S.A0(a + 1);
                        tn = S.T1(a + 1);
                    }
                    S.C.add(kFFErf);
                    const float f1 = erff(__fdiv_rn(c.y + c.z * t_evt, c.w));
                    const float f0 = erff(__fdiv_rn(c.y + c.z * t_prev, c.w));
                    seg += (Acc)(c.x * (f1 - f0));
                    int pp = a;
                    if (!is_entry && a == m - 1) pp = exit_pos;
                    const bool gone = !is_entry && a == exit_pos;
                    if (!gone && (t1a < nx || (t1a == nx && pp < npos))) {
                        nx = t1a;
                        npos = pp;
                    }
                }
                if (acc + seg > (Acc)target) {  // the scatter lies in [t_prev, t_evt]: SHADE solves for it
                    kfull = (float)((Acc)target - acc);
                    t_cut = t_evt;
                    phase = kSmShade;
                    break;
                }
                acc += seg;
                t_prev = t_evt;
                if (window_end) {  // the next window starts at t_cut
                    W0 = t_cut;
                    cap = min(2 * cap, A.ff_hit_cap);
                    begin_window();
                    break;
                }
                if (is_entry) {
                    if (m >= A.ff_act_cap) {
                        to_shade(-2.0f);
                        break;
                    }
                    const float t1n = S.template enter_row<false>(A, m, hn, P.ray, t_evt);
                    ++i;
                    if (t1n < nx) {
                        nx = t1n;
                        npos = m;
                    }
                    ++m;
                } else {
                    S.move(exit_pos, m - 1);
                    --m;
                }
                next_exit = nx;
                exit_pos = npos;
                go = budget > 0;
            }
        } else {
            // ---- COLLECT: one NODE or PRIM iteration of the window's while-while walk ----
            const bool col = phase == kSmCollect;
            const bool has_prim = col && w.has_prim();
            const bool can_node = col && w.can_node();
            if (prim_iteration(__ballot(has_prim), __ballot(can_node))) {
                bool go = has_prim;
                for (int k = 0; k < kSmCollectSteps; ++k) {
                    if (go) w.prim_step(ring, kFFBlock, prim);
                    go = go && w.has_prim();
                }
            } else {  // (the ray's node-space slab constants are recomputed per iteration, not carried across phases)
#ifdef VR_DIAG_FFSM
                dnode = true;
#endif
                const WideSlab s = wide_slab(A, P.ray);
                bool go = can_node;
                for (int k = 0; k < kSmCollectSteps; ++k) {
                    if (go) {
                        S.C.add(kFFNode4);
                        if (!w.node_step(A, s, prune, stack, ring, kFFBlock)) redo = true;  // (no further node step)
                    }
                    go = go && w.can_node();
                }
            }
            if (col && (redo || w.drained())) {  // the window's collection is complete
                if (redo) {  // the pair tree (at most one push per level) redoes the whole collection
                    n = 0;
                    t_cut = kfull = INFINITY;
                    auto leaf = [&](uint32_t first, uint32_t count) {
                        for (uint32_t jj = first; jj < first + count; ++jj) prim(jj);
                        return true;
                    };
                    auto on2 = [&]() { S.C.add(kFFNode2); };
                    if (A.hnodes) traverse<true>(A, P.ray, stack, kFFBlock, prune, leaf, on2);
                    else traverse<false>(A, P.ray, stack, kFFBlock, prune, leaf, on2);
                }
                // a buffer that filled ends the window at its largest kept key (subtrees skipped while full hold
                // only larger keys; whether one was skipped depends on the wave's NODE/PRIM schedule, so the cut must not)
                if (n == cap) t_cut = fminf(t_cut, S.K(n - 1));
                while (n > 0 && S.K(n - 1) >= t_cut) --n;
                if (t_cut <= W0) {  // more than cap Gaussians overlap at W0: no progress at this cap
                    if (cap >= A.ff_hit_cap) {
                        to_shade(-2.0f);
                    } else {
                        cap = min(2 * cap, A.ff_hit_cap);
                        begin_window();
                    }
                } else if (n == 0 && t_cut == INFINITY) {
                    to_shade(-1.0f);
                } else {
                    i = m = 0;
                    next_exit = INFINITY;
                    exit_pos = -1;
                    S.ph = 0;  // (entries write both F slots: the phase at a window's start is free)
                    phase = kSmSweep;
                }
            }
        }
#ifdef VR_DIAG_FFSM
        if constexpr (CNT) {
            if (lane == 0u) {
                const uint32_t dc = (uint32_t)((__builtin_amdgcn_s_memtime() - dt0) >> 4);
#if VR_DIAG_FFSM == 2
                const int k = dphase == 0 ? (dnode ? 0 : 1) : dphase + 1;
                S.C.v[k] += dc;
                S.C.v[4 + k] += 1u;
#else
                S.C.v[dphase] += dc;
                S.C.v[3 + dphase] += 1u;
                if (dphase == 0) S.C.v[6] += (uint32_t)nc;
                if (dphase == 1) S.C.v[7] += (uint32_t)ns;
#endif
            }
        }
#endif
    }
    if constexpr (CNT) {
        Ctr c{};
        for (int k = 0; k < kFFNumCtr; ++k) c.v[k] = S.C.v[k];
        flush_counters(A.work, c);
    }
}

// Paths the path kernel queued because more Gaussians overlapped one point than its rows hold: each
// re-runs from its first bounce (same seed, so the same path) with kFFBigCap-entry rows and inline
// shadow rays, and writes its radiance as one inline sum (its earlier queued shadow rays are dropped).
// Only a path over kFFBigCap fails (NaN, VR_ERR_OVERFLOW).
template <bool MULTI>
__global__ void __launch_bounds__(kFFBlock) ff_fallback_kernel(RenderArgs A) {
    __shared__ int s_stack[(kStackSize + kCollectQueue) * kFFBlock];
    int* stack = s_stack + threadIdx.x;
    const uint32_t gt = blockIdx.x * kFFBlock + threadIdx.x, nt = gridDim.x * kFFBlock;
    const uint32_t n = min(A.ff_fbq[0], A.ff_fbq_cap);
    RenderArgs B = A;
    B.ff_threads = nt;
    B.ff_hit_cap = B.ff_act_cap = kFFBigCap;
    B.ff_hit = A.ff_big;
    B.ff_act0 = A.ff_big + (size_t)kFFBigCap * nt;
    B.ff_act1 = A.ff_big + (size_t)2 * kFFBigCap * nt;
    B.ff_nee_cap = 0;  // shadow rays inline
    B.ff_fbq = nullptr;
    FFScratch<false> S{B.ff_hit + gt, B.ff_act0 + gt, B.ff_act1 + gt, nt, 0, {}};
    for (uint32_t q = gt; q < n; q += nt) {
        FFPath P{PCG32(0, 1)};
        if (!ff_start(B, A.ff_fbq[1 + q], P)) continue;
        while (ff_bounce<MULTI>(B, S, stack, P)) {
        }
    }
}

// Traces the launch's queued shadow rays (the walk of transmittance_up_to on the 4-wide tree, the
// same double sum and early stop) as an operation on the persistent ray-queue walk (ray_queue_walk,
// vr_walk.h): a lane whose ray is done takes the next queued ray, claimed per wave once ff_nee_refill
// lanes are idle, so a wave never waits for its longest ray. Each ray's contribution m * Li replaces
// its weight m in place.
__device__ __forceinline__ void nee_finish(const RenderArgs& A, uint32_t id, float tmax, float Tr) {
    float4& c = A.ff_nee[3 * (size_t)id + 2];
    const float4 m = c;
    float Li0, Li1, Li2;
    nee_radiance(A, Tr, __float_as_int(m.w), tmax, Li0, Li1, Li2);
    c = make_float4(m.x * Li0, m.y * Li1, m.z * Li2, m.w);
}

#ifndef VR_NEE_BLOCKS
#define VR_NEE_BLOCKS 4  // resident 256-lane blocks per CU
#endif
#ifndef VR_NEE_STEPS
#define VR_NEE_STEPS 4  // node steps / primitives per lane per wave iteration of the shadow-ray kernel
#endif
constexpr int kNeeQueue = 8, kNeeSteps = VR_NEE_STEPS;
// The leaf FIFO hands leaves out in the order the walk reaches them, so the double sum adds the same terms in
// the same order as transmittance_up_to (bit-identical Tr; a sum stopped mid-leaf is >= 104 either way).
template <bool CNT>
struct NeeOp {
    static constexpr bool kPrune = true;
    FFCount<CNT> C;
    double sum;
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const float4 a = A.ff_nee[3 * (size_t)id], b = A.ff_nee[3 * (size_t)id + 1];
        r = Ray{a.x, a.y, a.z, b.x, b.y, b.z};
        tmax = a.w;
        if (!(tmax > 0.0f)) return kRayFinish;  // Tr = 1
        C.add(kNeeRays);
        return kRayWalk;
    }
    __device__ __forceinline__ void reset() { sum = 0.0; }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        shadow_leaf(A, r, tmax, j, 1u, sum, &C);
        return sum < 104.0;  // expf(-x) == 0 in f32 for x >= 104: later terms cannot change Tr
    }
    __device__ __forceinline__ void on_node() { C.add(kNeeNode4); }
    // transmittance_up_to itself: traverse_wide if the scene has the 4-wide tree, then the pair tree
    __device__ __forceinline__ void redo(const RenderArgs& A, uint32_t id, const Ray& r, float tmax, float, int* stack) {
        nee_finish(A, id, tmax, transmittance_up_to(A, r, tmax, stack, kFFBlock));
    }
    __device__ __forceinline__ void finish(const RenderArgs& A, uint32_t id, float tmax) {
        nee_finish(A, id, tmax, expf(-(float)sum));
    }
    __device__ __forceinline__ void invalid(uint32_t) {}
};

template <bool CNT = false>
__global__ void __launch_bounds__(kFFBlock) ff_nee_kernel(RenderArgs A) {
    __shared__ int s_stack[(kStackSize + kNeeQueue) * kFFBlock];
    int* stack = s_stack + threadIdx.x;
    NeeOp<CNT> op{};
    ray_queue_walk<kNeeQueue, kNeeSteps>(A, min(A.ff_nee_n[0], A.ff_nee_cap), A.ff_nee_n + 1, A.ff_nee_refill, stack,
                                         stack + kStackSize * kFFBlock, kFFBlock, op);
    if constexpr (CNT) {
        Ctr c{};
        for (int i = 0; i < kFFNumCtr; ++i) c.v[i] = op.C.v[i];
        flush_counters(A.work + 8, c);
    }
}

// Each path's radiance from its queued contributions (bounce order) and its inline part, one thread
// per path of the launch (the chains are walked in parallel, not by the pixel's thread sample after
// sample); written back into the path's ff_tail entry with no chain left.
__global__ void __launch_bounds__(kFFBlock) ff_path_radiance_kernel(RenderArgs A) {
    const size_t q = (size_t)blockIdx.x * kFFBlock + threadIdx.x;
    if (q == 0) atomicMax(A.counters + 3, A.ff_nee_n[0]);  // the frame's largest launch queue need (host sizing)
    if (q >= A.ff_total) return;
    const float4 t = A.ff_tail[q];
    const uint32_t f = __float_as_uint(t.w);
    if ((f & ~kFFTailAfter) == kFFNone) return;
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
    for (uint32_t e = f & ~kFFTailAfter; e != kFFNone; e = __float_as_uint(A.ff_nee[3 * (size_t)e + 1].w)) {
        const float4 c = A.ff_nee[3 * (size_t)e + 2];
        p0 += c.x;
        p1 += c.y;
        p2 += c.z;
    }
    if (f & kFFTailAfter) {
        p0 += t.x;
        p1 += t.y;
        p2 += t.z;
    }
    A.ff_tail[q] = make_float4(p0, p1, p2, __uint_as_float(kFFNone));
}

// pixel_L += L_accum in sample order (integrator.h:706), then pixel_L / num_samples on the last batch.
__global__ void __launch_bounds__(kFFBlock) ff_accumulate_kernel(RenderArgs A, uint32_t chunk_tiles) {
    const uint32_t tl = blockIdx.x;  // tile within the chunk
    if (tl >= chunk_tiles) return;
    const uint32_t tile_local = A.ff_tile_base + tl;
    const size_t p = (size_t)tile_local * kFFBlock + threadIdx.x;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (A.ff_si0 != 0) {
        s0 = A.ff_sum[p * 3 + 0];
        s1 = A.ff_sum[p * 3 + 1];
        s2 = A.ff_sum[p * 3 + 2];
    }
    for (uint32_t s = 0; s < A.ff_nsb; ++s) {
        const size_t q = (size_t)(tl * A.ff_nsb + s) * kFFBlock + threadIdx.x;
        // the path's radiance: no tail of the launch has a chain here (without a queue no path starts one; with
        // one, ff_path_radiance_kernel has summed every chain of the ff_total paths this grid reads into t.xyz)
        const float4 t = A.ff_tail[q];
        s0 += t.x;
        s1 += t.y;
        s2 += t.z;
    }
    if (A.ff_si0 + A.ff_nsb < (uint32_t)A.ff_samples) {
        A.ff_sum[p * 3 + 0] = s0;
        A.ff_sum[p * 3 + 1] = s1;
        A.ff_sum[p * 3 + 2] = s2;
        return;
    }
    int lx, ly, x, y;
    tile_pixel(A, tile_local, threadIdx.x, lx, ly, x, y);
    const float fs = (float)A.ff_samples;
    store_px(A, tile_local, lx, ly, x, y, __fdiv_rn(s0, fs), __fdiv_rn(s1, fs), __fdiv_rn(s2, fs));
}

}  // namespace dev

// Threads of the resident path-kernel grid on a device with `cus` CUs (the scratch row stride).
uint32_t free_flight_threads(int cus) {
    int per_cu = 0;
    int per_sm = 0;  // (both path kernels run a resident grid over the same rows: the smaller occupancy)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)dev::ff_path_kernel<true, false>, dev::kFFBlock, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_sm, (const void*)dev::ff_path_sm_kernel<true, false>, dev::kFFBlock, 0) !=
            hipSuccess)
        per_cu = per_sm = 1;
    per_cu = std::max(1, std::min(per_cu, per_sm));
    return (uint32_t)std::max(1, cus) * (uint32_t)per_cu * (uint32_t)dev::kFFBlock;
}

// Host launcher: one (tile chunk, sample batch) step. A.ff_* describe the step.
hipError_t launch_free_flight(const RenderArgs& A, uint32_t chunk_tiles, hipStream_t stream, hipEvent_t* ev) {
    hipError_t e0 = hipMemsetAsync(A.ff_next, 0, sizeof(unsigned long long), stream);
    if (e0 != hipSuccess) return e0;
    if (A.ff_nee_cap > 0 && (e0 = hipMemsetAsync(A.ff_nee_n, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e0;
    if (A.ff_fbq != nullptr && (e0 = hipMemsetAsync(A.ff_fbq, 0, sizeof(uint32_t), stream)) != hipSuccess) return e0;
    dim3 grid(A.ff_threads / dev::kFFBlock);
    const bool cnt = A.work != nullptr;  // vr_count_work: the instrumented kernels
    if ((e0 = hipEventRecord(ev[0], stream)) != hipSuccess) return e0;
    if (A.ff_sm) {  // the phase-scheduled path kernel (VR_OPT_FF_KERNEL)
        if (A.ff_multi) {
            if (cnt) hipLaunchKernelGGL((dev::ff_path_sm_kernel<true, true>), grid, dim3(dev::kFFBlock), 0, stream, A);
            else hipLaunchKernelGGL((dev::ff_path_sm_kernel<true>), grid, dim3(dev::kFFBlock), 0, stream, A);
        } else {
            if (cnt) hipLaunchKernelGGL((dev::ff_path_sm_kernel<false, true>), grid, dim3(dev::kFFBlock), 0, stream, A);
            else hipLaunchKernelGGL((dev::ff_path_sm_kernel<false>), grid, dim3(dev::kFFBlock), 0, stream, A);
        }
    } else if (A.ff_multi) {
        if (cnt) hipLaunchKernelGGL((dev::ff_path_kernel<true, true>), grid, dim3(dev::kFFBlock), 0, stream, A);
        else hipLaunchKernelGGL((dev::ff_path_kernel<true>), grid, dim3(dev::kFFBlock), 0, stream, A);
    } else {
        if (cnt) hipLaunchKernelGGL((dev::ff_path_kernel<false, true>), grid, dim3(dev::kFFBlock), 0, stream, A);
        else hipLaunchKernelGGL((dev::ff_path_kernel<false>), grid, dim3(dev::kFFBlock), 0, stream, A);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (A.ff_fbq != nullptr) {  // paths over the hit-buffer capacity (usually none: the kernel exits at once)
        if (A.ff_multi) hipLaunchKernelGGL((dev::ff_fallback_kernel<true>), dim3(kFFBigThreads / dev::kFFBlock), dim3(dev::kFFBlock), 0, stream, A);
        else hipLaunchKernelGGL((dev::ff_fallback_kernel<false>), dim3(kFFBigThreads / dev::kFFBlock), dim3(dev::kFFBlock), 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    if (A.ff_nee_cap > 0) {
        int dv = 0, cus = 1;
        if (hipGetDevice(&dv) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dv);
        const dim3 ng((unsigned)std::max(1, cus) * VR_NEE_BLOCKS);
        if (cnt) hipLaunchKernelGGL(dev::ff_nee_kernel<true>, ng, dim3(dev::kFFBlock), 0, stream, A);
        else hipLaunchKernelGGL(dev::ff_nee_kernel<false>, ng, dim3(dev::kFFBlock), 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    if (A.ff_nee_cap > 0) {
        hipLaunchKernelGGL(dev::ff_path_radiance_kernel, dim3((unsigned)((A.ff_total + dev::kFFBlock - 1) / dev::kFFBlock)),
                           dim3(dev::kFFBlock), 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dev::ff_accumulate_kernel, dim3(chunk_tiles), dim3(dev::kFFBlock), 0, stream, A, chunk_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipEventRecord(ev[3], stream);
}

}  // namespace vr
