// RayMarchingGaussians (test_integrators.h:160-296) as a three-stage wavefront pipeline for gfx950.
//
// The reference marches every pixel on one CPU thread and, at each step that scatters, traces
// nlights + env_samples secondary rays one after another. The transmittance T of the primary ray
// never depends on those secondary rays (they only add to L), so the device path splits the loop:
//
//   1. march_kernel (one lane per pixel, a 64-lane workgroup per 8x8 quarter of a 16x16 tile): walks the primary
//      ray's steps and emits one *scatter record* per step with sigma_s > 0 (position, T*sigma_s,
//      step index k, the active Gaussian set). Run twice: MODE 0 counts records per pixel, an
//      exclusive scan places them, MODE 1 writes them — so the record order is a pure function of
//      the frame, and the final image is bitwise reproducible.
//   2. secondary_persistent_kernel (every light / environment ray of every record; ray ids in
//      sample-major order so that neighbouring lanes trace rays from neighbouring pixels towards the
//      same light): transmittance of each secondary ray, see Stage 2 below.
//   3. accumulate_kernel (one thread per pixel): L += T*sigma_s*(Li + Le)*dt/(4 pi) over the
//      pixel's records in step order, then L += T*env — the reference's operation order.
//
// No per-ray event list is ever built or sorted:
//   * the step sequence t_k is the reference's own iterated float sum (host table), so empty
//     stretches are skipped by index;
//   * the active set at step k is {i : a_i <= t_k < b_i}; it is kept as a short list of
//     Gaussian ids in LDS, sorted by scene index (the order the reference sums a step's densities in), extended by BVH queries restricted to the window (t_{k-1}, t_k] or by a
//     closest-entry query when it runs empty;
//   * a secondary ray's transmittance telescopes the reference's segment loop into one sum of
//     per-Gaussian optical depths over each Gaussian's active interval on that ray, reproducing the
//     quirks: primary-active Gaussians are pre-activated at t = 0 (test_integrators.h:209-211), a
//     light ray's last segment runs to the first event at or past the light (:220-235), an
//     environment ray runs to its last event (:258-271);
//   * a ray stops marching when T <= t_eps (exactly 0 by default: bit-neutral).
// Pixels whose active set outgrows the fast path's LDS list (32) are queued and re-run by the
// fallback kernels (64), so results never depend on capacity.
//
// The pipeline's translation units (this header holds only what more than one of them uses):
//   vr_gauss_march.hip      stage 1: the primary march and its binned variant
//   vr_gauss_secondary.hip  stage 2: the persistent secondary-ray kernel, its ray order and start subtrees
//   vr_gauss_exact.hip      stage 2's exact slow path (serial and wave-cooperative)
//   vr_gauss_shade.hip      stage 3: cut-offs, per-record radiance, accumulation
//   vr_gauss_tree.hip       at upload: parents, the secondary rays' tight tree and its copies, whitening
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vr_dev_common.h"

namespace vr {
namespace dev {

// Optical-depth cut-off of a secondary ray: expf(-104) rounds to 0 in f32 and every optical depth
// is >= 0, so once the running sum reaches kTauCut the ray's transmittance is exactly 0 whatever
// else it crosses — the traversal stops there. (The reference's product of per-segment
// exponentials reaches 0 or a denormal <= 1.4e-45 at the same point.)
constexpr float kTauCut = 104.0f;

// Band around a list member's 3-sigma surface (in p.M.p and in the chord's 9 - e2) inside which a secondary
// ray's decision for that member is left to the exact slow path: ~10x the f32 difference between the
// whitened and the reference's M forms for an origin near the Gaussian (~1e-7 relative, times the
// covariance's condition number). The march marks a record whose members include one with p.M.p above
// 9 - 2 kMemberAmb (kRecBoundary in the active count), so only the rays of such records (~1 %) test it.
#ifndef VR_MEMBER_AMB
#define VR_MEMBER_AMB 5e-5f  // (A/B: 0 removes the test)
#endif
constexpr float kMemberAmb = VR_MEMBER_AMB;

// Band around a secondary ray's grazing chords inside which the reference's f32 quadratic (gaussian.h:137-151:
// B*B - 4*A*C with A = d.M.d, B = 2 p.M.d, C = p.M.p - 9) may decide otherwise than the whitened chord test: its
// discriminant, in units of D = 9 - e2 (the chord's half length squared in whitened units), carries an absolute
// error of up to ~5 eps c (eps = 2^-23, c = p.M.p; measured maximum 5.1 eps c over 2.3e5 grazing rays of the
// make_random distribution, tools/chord_band.py). Inside it the reference can collapse a chord to a point or miss it
// (C4 at t_eps 0, pixel (598, 3212): D = 3.3e-4 at c = 2735, [0.32260, 0.32282] became [0.3227114, 0.3227114] and its
// 0.078 of optical depth was lost) or keep a tiny phantom chord the whitened test misses. A ray with a test inside
// |D| < kChordBand c goes to the exact slow path, which runs the reference's M forms on the exactly normalised ray.
// Both bands were sized at condition numbers <= 12. Measured beyond (tests/test_gpu_aniso_records.py: discs of axis
// ratio 10 and 30, needles of ratio 10, condition numbers 1e2 .. 9e2, every secondary ray of six pixels each):
// where the reference's own f32 Tr is within 0.5e-4 of a float64 ray model the device is within 4.9e-5 of the
// reference, and elsewhere (the reference up to 3.0e-3 from float64) the device is never further from float64
// than the reference is, so the bands stand unscaled up to 9e2. Nothing is measured above that.
#ifndef VR_CHORD_BAND
#define VR_CHORD_BAND 8.0f  // in eps c (A/B: 0 removes the test)
#endif
constexpr float kChordBand = VR_CHORD_BAND * 1.1920928955078125e-7f;
constexpr uint32_t kRecBoundary = 0x80000000u;  // rec_meta.w: active count | this flag
// An environment ray with one non-member chord in the f32 error band (kChordBand) keeps that Gaussian's id in its
// `lim` (the last event so far, only needed for a missed member: such a ray goes to the exact slow path anyway) as
// a NaN payload, which `t1 > lim` never overwrites: no register and no store on the traversal's path.
__device__ __forceinline__ float band_lim(uint32_t j) { return __uint_as_float(0x7f800000u | (j + 1u)); }
__device__ __forceinline__ uint32_t band_id(float lim) { return (__float_as_uint(lim) & 0x007fffffu) - 1u; }

// Bit of active-list slot `slot` in a ray's 64-bit hit mask. Records with more than 64 active
// Gaussians (march_deep_kernel) find their missed members by re-intersecting the whole list instead.
__device__ __forceinline__ uint64_t slot_bit(int slot) { return slot < 64 ? 1ull << slot : 0ull; }

// Scatter records of the frame, read on the device: the host never waits for the march (the
// buffers are sized from the previous frame; a frame that outgrew them is reported and re-run).
// Clamped to the capacity, so an overflowing frame stays in bounds.
__device__ __forceinline__ uint32_t dev_nrec(const RenderArgs& A) { return min(A.rec_alloc[0], A.rec_cap); }

// A 4-wide node index (< 2^27 nodes) in the walk's `node`; bits 28-30 may carry a child slot to skip.
constexpr int32_t kNodeIndexMask = 0x0fffffff;

// Direction of environment sample e of a record: PCG32 keyed by (pixel, step) as the oracle does;
// the 2e draws of the earlier samples are skipped by LCG jump-ahead s -> M s + C (host table).
// A record's environment samples all jump from one state: its path's seeded stream-1 generator.
__device__ __forceinline__ uint64_t env_base_state(const uint4& meta) {
    const int px = (int)(meta.x & 0xffffu), py = (int)(meta.x >> 16);
    return PCG32(derive_path_seed(px, py, (int)meta.y), 1).state;
}
__device__ __forceinline__ void env_xi_at(const RenderArgs& A, uint64_t base, uint32_t e, float& xi1, float& xi2) {
    PCG32 rng(PCG32::FromState{}, A.pcg_jump[4 * e] * base + A.pcg_jump[4 * e + 1], 1);
    xi1 = rng.uniform_env();
    xi2 = rng.uniform_env();
}
__device__ __forceinline__ void env_sample_xi(const RenderArgs& A, const uint4& meta, uint32_t e, float& xi1, float& xi2) {
    env_xi_at(A, env_base_state(meta), e, xi1, xi2);
}
__device__ __forceinline__ void env_sample_dir(const RenderArgs& A, const uint4& meta, uint32_t e, float& wx, float& wy,
                                               float& wz) {
    float xi1, xi2;
    env_sample_xi(A, meta, e, xi1, xi2);
    env_dir(xi1, xi2, wx, wy, wz);
}

// Ray ids are scheduled record-chunk-major: a chunk is A.chunk_rec consecutive records x all
// their samples (light rays first, then environment rays), so a wave that takes consecutive ids
// reads each record's data (position, active list, neighbour list) from its cache instead of
// once per sample. Light rays of a chunk go sample-major (neighbouring records towards the same
// light: coherent). Environment rays are random directions; with A.env_order they are handed
// out in the direction order env_order_kernel computed for the chunk, so a wave traces similar
// directions from nearby records. The result slot stays sample-major: tr[s * rec_cap + r].
__device__ __forceinline__ bool ray_slot(const RenderArgs& A, uint32_t chunk, uint32_t rem, uint32_t nrec, uint32_t& s,
                                         uint32_t& r) {
    const uint32_t cr = A.chunk_rec, lights = cr * (uint32_t)A.num_lights;
    if (A.env_order == nullptr || rem < lights) {
        s = rem >> A.chunk_shift;
        r = chunk * cr + (rem & (cr - 1u));
    } else {  // entry = record-in-chunk << 8 | environment sample
        const uint32_t v = A.env_order[(size_t)chunk * (cr * (uint32_t)A.env_samples) + (rem - lights)];
        s = (uint32_t)A.num_lights + (v & 0xffu);
        r = chunk * cr + (v >> 8);
    }
    return r < nrec;
}

// Result slot of a secondary ray: its position in the hand-out order (chunk-major, then the order
// ray_slot hands the chunk's rays out). A wave takes a chunk's rays in that order and writes each Tr
// when its ray completes, so one chunk's results fill a contiguous run of lines within a short time
// (a [sample][record] layout scattered every chunk's 4-B stores over S rows: lines left L2 partially
// written and were re-read — 7x write amplification). record_radiance_kernel reads a chunk back
// whole.
__device__ __forceinline__ uint32_t rays_per_chunk(const RenderArgs& A) {
    return A.chunk_rec * (uint32_t)(A.num_lights + A.env_samples);
}

// A queued secondary ray (to_slow, to_fix) decoded again from its result slot t: sample s (lights first) of
// record r, the record's position, meta word and active list, and the exactly normalised ray the reference
// traces — towards light s at distance `dist` (test_integrators.h:202-237), or environment sample
// s - num_lights (:242-271, Ray env_ray(pos, wi) normalises the sampled direction).
struct QueuedRay {
    uint32_t s, r;
    float4 pos;
    uint4 meta;
    ActList act;
    bool light;
    Ray ray;
    float dist;  // an environment ray: +inf
};
__device__ __forceinline__ QueuedRay decode_queued_ray(const RenderArgs& A, uint64_t t) {
    QueuedRay q;
    const uint32_t per = rays_per_chunk(A), chunk = (uint32_t)(t / per), rem = (uint32_t)(t - (uint64_t)chunk * per);
    ray_slot(A, chunk, rem, dev_nrec(A), q.s, q.r);
    q.pos = A.rec_pos[q.r];
    q.meta = A.rec_meta[q.r];
    q.act = ActList{A.rec_act + q.meta.z, 1, (int)(q.meta.w & ~kRecBoundary), A.rec_bloom[q.r]};
    q.light = q.s < (uint32_t)A.num_lights;
    if (q.light) {
        const LightRecord& lr = A.lights[q.s];
        float dx = lr.px - q.pos.x, dy = lr.py - q.pos.y, dz = lr.pz - q.pos.z;
        q.dist = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
        normalize3(dx, dy, dz);
        q.ray = make_ray(q.pos.x, q.pos.y, q.pos.z, dx, dy, dz);
    } else {
        float xi1, xi2, wx, wy, wz;
        env_xi_at(A, A.env_order != nullptr ? A.env_base[q.r] : env_base_state(q.meta), q.s - (uint32_t)A.num_lights, xi1, xi2);
        env_dir(xi1, xi2, wx, wy, wz);
        q.dist = INFINITY;
        q.ray = make_ray(q.pos.x, q.pos.y, q.pos.z, wx, wy, wz);
    }
    return q;
}

}  // namespace dev

// Grid for a per-record kernel over at most rec_cap records (the live count is read on the device).
static unsigned record_grid(const RenderArgs& A, uint32_t per_block, unsigned max_blocks) {
    const uint64_t b = ((uint64_t)A.rec_cap + per_block - 1) / per_block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, max_blocks));
}

// vr_gauss_exact.hip, called by vr_gauss_secondary.hip: the exact slow path over the frame's queue of rays
// (stats: the instrumented kernels). Internal to the library, not part of what it exports.
__attribute__((visibility("hidden"))) hipError_t secondary_slow_launch(const RenderArgs& A, hipStream_t stream, bool stats);

}  // namespace vr
