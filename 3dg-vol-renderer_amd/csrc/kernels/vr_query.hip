// Batched mixture queries over the uploaded scene (include/vr_hip.h, vr_query_*): the three questions
// the reference's GaussianMixtureModel answers about the mixture itself, for a caller's rays / points:
//   transmittance_up_to(ray, tmax)          gmm.h:517-578   query_transmittance_kernel
//   intersect_events(ray, events)           gmm.h:457-515   query_events_count_kernel / _fill_kernel + sort
//   evaluate_sigma(active, pos, sa, ss)     gmm.h:98-126    query_sigma_kernel (active = the 3-sigma ellipsoids
//                                                            holding pos, the set the integrators pass)
// and, for the first of them, the gradient of its optical depth with respect to the Gaussians
// (query_grad_kernel / query_grad_finish_kernel: f32 decisions, double arithmetic per hit, double atomic adds)
// and with respect to the ray (query_ray_grad_kernel: the same per-hit arithmetic, summed per ray in registers);
// for the last, the gradient of sigma with respect to the Gaussians (albedo included) and to the points
// (query_sigma_grad_kernel / query_sigma_grad_points_kernel / query_grad_finish_kernel: the forward's walk and
// f32 decision, double per active Gaussian, double atomic adds per Gaussian, register sums per point).
//
// Floating point: a query is an API for fidelity, so every Gaussian is tested with the exact forms of
// vr_march.h (quad / intersect / optical_depth / mu_t: the reference's evaluation order, correctly rounded
// division and square root, no contraction): hit decisions and t_enter / t_exit are bit-identical to
// intersect_direct (gaussian.h:126-164). erf / exp come from the device library (a few ulp from glibc's).
// Sums over Gaussians (optical depth, mu_t, mu_t * albedo) are kept in double, where adding a few dozen f32
// terms is exact, so a result does not depend on the order in which a tree hands the Gaussians out:
// VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH change the walk, not the answer.
//
// Ray walks (transmittance, events) are operations on the persistent ray-queue walk the shadow-ray kernel
// uses too (ray_queue_walk, vr_walk.h): a walk whose LDS stack could overflow, and every walk of a scene without
// the 4-wide tree (VR_OPT_HALF_NODES = 0, or boxes too small for f16), is redone on the child-pair tree at the
// ray's completion. The walk's block shape and the operations' base (QueryOp, query_walk) are in vr_query_common.h,
// which vr_query_profile.hip shares.
#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "vr_query_common.h"

namespace vr {
namespace dev {

// gmm.h:539-551: a = max(0, t_enter), b = min(tmax, t_exit), optical_depth(a, b) added if b > a.
// TAU: the caller wants the optical depth itself, so the sum runs to the end; otherwise it stops at 104,
// where expf(-x) is 0 in f32 whatever follows (the shadow kernel's early-out: the same Tr bit for bit).
template <bool TAU>
struct TransOp : QueryOp<TransOp<TAU>, true> {
    float* tr;
    float* tau;
    double sum;
    __device__ __forceinline__ void reset() { sum = 0.0; }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        const Quad q = quad(g, r);
        float t0, t1;
        if (intersect(q, t0, t1)) {
            const float a = fmaxf(0.0f, t0);
            const float b = fminf(tmax, t1);
            if (b > a) sum += (double)optical_depth(g, q, a, b);
        }
        return TAU ? true : sum < 104.0;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        tr[id] = expf(-(float)sum);
        if constexpr (TAU) tau[id] = (float)sum;
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        tr[id] = __builtin_nanf("");
        if constexpr (TAU) tau[id] = __builtin_nanf("");
    }
};

// gmm.h:482-485: an entry event if t_enter >= 0, an exit event if t_exit >= 0.
struct EventCountOp : QueryOp<EventCountOp, false> {
    uint32_t* counts;
    uint32_t cnt;
    __device__ __forceinline__ void reset() { cnt = 0; }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        float t0, t1;
        if (intersect(quad(g, r), t0, t1)) cnt += (t0 >= 0.0f ? 1u : 0u) + (t1 >= 0.0f ? 1u : 0u);
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) { counts[id] = cnt; }
    __device__ __forceinline__ void invalid(uint32_t id) { counts[id] = 0; }
};

// The same walk again, writing each event as a 64-bit sort key at the ray's offset: high word the bits of
// t + 0.0f (-0 becomes +0; every t is >= 0, so the bits order as unsigned integers), low word
// scene_index << 1 | exiting. Sorted per ray, events with equal t therefore come in scene order, a
// Gaussian's entry before its exit, whatever order the tree produced them in.
struct EventFillOp : QueryOp<EventFillOp, false> {
    const uint32_t* offsets;
    unsigned long long* keys;
    unsigned long long cap;
    uint32_t base, room, w;
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        base = offsets[id];
        room = offsets[id + 1] - base;
        return QueryOp::load(A, id, r, tmax);
    }
    __device__ __forceinline__ void reset() { w = 0; }
    __device__ __forceinline__ void put(float t, uint32_t low) {
        // (room: the count pass's number for this ray; cap: the caller's buffers. Neither is ever passed.)
        if (w < room && (unsigned long long)base + w < cap)
            keys[(size_t)base + w] = ((unsigned long long)__float_as_uint(t + 0.0f) << 32) | low;
        ++w;
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        float t0, t1;
        if (intersect(quad(g, r), t0, t1)) {
            const uint32_t si = A.gauss_order[j] << 1;
            if (t0 >= 0.0f) put(t0, si);
            if (t1 >= 0.0f) put(t1, si | 1u);
        }
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t, float) {}
    __device__ __forceinline__ void invalid(uint32_t) {}
};

// The head of a decided hit's double arithmetic (include/vr_hip.h, vr_query_transmittance_grad, has the notation): the
// record's f32 numbers and the ray read as doubles, p = o - mean, M d, M p, A, B, the closest approach m, c = p + m d,
// u = t - m at the f32 clip bounds [a, b], k and the moments. RayGradOp's; GradOp::add keeps its own copy of the same
// lines, because calling this from it changes query_grad_kernel's register allocation (SGPR spills 99 -> 95).
struct HitMoments {
    double dx, dy, dz, px, py, pz;
    double m00, m01, m02, m11, m12, m22;
    double mdx, mdy, mdz, mpx, mpy, mpz;
    double A, B, m, cx, cy, cz, k, eb, J0, J1, J2;
};
__device__ __forceinline__ HitMoments hit_moments(const GRec& g, const Ray& r, float a, float b) {
    const double dx = r.dx, dy = r.dy, dz = r.dz;
    const double px = (double)r.ox - (double)g.mx, py = (double)r.oy - (double)g.my, pz = (double)r.oz - (double)g.mz;
    const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
    const double mdx = m00 * dx + m01 * dy + m02 * dz, mdy = m01 * dx + m11 * dy + m12 * dz, mdz = m02 * dx + m12 * dy + m22 * dz;
    const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz, mpz = m02 * px + m12 * py + m22 * pz;
    const double A = dx * mdx + dy * mdy + dz * mdz;
    const double B = 2.0 * (px * mdx + py * mdy + pz * mdz);
    const double C = px * mpx + py * mpy + pz * mpz;
    const double m = -B / (2.0 * A);  // the line's closest approach: c = p + m d, u = t - m
    const double cx = px + m * dx, cy = py + m * dy, cz = pz + m * dz;
    const double ua = (double)a - m, ub = (double)b - m;
    const double k = exp(-0.5 * (C - B * B / (4.0 * A)));
    const double sA = sqrt(0.5 * A);
    const double J0 = sqrt(3.14159265358979323846 / (2.0 * A)) * (erf(ub * sA) - erf(ua * sA));
    const double ea = exp(-0.5 * A * ua * ua), eb = exp(-0.5 * A * ub * ub);
    const double J1 = (ea - eb) / A;
    const double J2 = (ua * ea - ub * eb) / A + J0 / A;
    return HitMoments{dx, dy, dz, px, py, pz, m00, m01, m02, m11, m12, m22, mdx, mdy, mdz, mpx, mpy, mpz,
                      A, B, m, cx, cy, cz, k, eb, J0, J1, J2};
}

// The gradient of the ray's optical depth (TransOp<true>'s sum, without its rounding to f32) with respect to the
// Gaussians it crosses, times the ray's weight, added to the staging rows acc[10 j .. 10 j + 9] of record j (tree
// order): g_mean[3], G_M {00, 01, 02, 11, 12, 22} and U, each per unit density (include/vr_hip.h,
// vr_query_transmittance_grad, has the formulas; query_grad_finish_kernel turns a row into the caller's).
// The hit decision and the clip bounds [a, b] are TransOp's f32 ones; everything on a decided hit is double.
// No early-out: every hit counts. The adds are global_atomic_add_f64 (no compare-and-swap loop), in arrival order.
// A walk that is redone after Gaussians were added (the LDS stack could overflow) first takes those back: the
// FIFO handed them out in traverse_wide's order, so the first `cnt` Gaussians of that walk are added with the
// opposite sign before the pair-tree walk adds the ray's whole hit set.
struct GradOp : QueryOp<GradOp, true> {
    const float* weight;
    double* acc;
    uint32_t moving;  // the ellipsoid's own bounds move with the parameters (not VR_GRAD_FROZEN_BOUNDS)
    float w;          // the ray's weight (negated while a walk is taken back)
    uint32_t cnt;     // Gaussians this walk has tested
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        w = weight ? weight[id] : 1.0f;
        const int what = QueryOp::load(A, id, r, tmax);
        return what == kRayWalk && w == 0.0f ? kRayFinish : what;
    }
    __device__ __forceinline__ void reset() { cnt = 0; }
    __device__ void add(const GRec& g, const Ray& r, float a, float b, bool mv_in, bool mv_out, uint32_t j) {
        const double dx = r.dx, dy = r.dy, dz = r.dz;
        const double px = (double)r.ox - (double)g.mx, py = (double)r.oy - (double)g.my, pz = (double)r.oz - (double)g.mz;
        const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
        const double mdx = m00 * dx + m01 * dy + m02 * dz, mdy = m01 * dx + m11 * dy + m12 * dz, mdz = m02 * dx + m12 * dy + m22 * dz;
        const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz, mpz = m02 * px + m12 * py + m22 * pz;
        const double A = dx * mdx + dy * mdy + dz * mdz;
        const double B = 2.0 * (px * mdx + py * mdy + pz * mdz);
        const double C = px * mpx + py * mpy + pz * mpz;
        const double m = -B / (2.0 * A);  // the line's closest approach: c = p + m d, u = t - m
        const double cx = px + m * dx, cy = py + m * dy, cz = pz + m * dz;
        const double ua = (double)a - m, ub = (double)b - m;
        const double k = exp(-0.5 * (C - B * B / (4.0 * A)));
        const double sA = sqrt(0.5 * A);
        const double J0 = sqrt(3.14159265358979323846 / (2.0 * A)) * (erf(ub * sA) - erf(ua * sA));
        const double ea = exp(-0.5 * A * ua * ua), eb = exp(-0.5 * A * ub * ub);
        const double J1 = (ea - eb) / A;
        const double J2 = (ua * ea - ub * eb) / A + J0 / A;
        const double wn = (double)w * (double)g.norm;
        const double s = wn * k;
        // g_mean = s M (c J0 + d J1)
        const double vx = cx * J0 + dx * J1, vy = cy * J0 + dy * J1, vz = cz * J0 + dz * J1;
        double o0 = s * (m00 * vx + m01 * vy + m02 * vz);
        double o1 = s * (m01 * vx + m11 * vy + m12 * vz);
        double o2 = s * (m02 * vx + m12 * vy + m22 * vz);
        // G_M = -s/2 (J0 c c^T + J1 (c d^T + d c^T) + J2 d d^T)
        const double h = -0.5 * s;
        double g00 = h * (J0 * cx * cx + J1 * (2.0 * cx * dx) + J2 * dx * dx);
        double g01 = h * (J0 * cx * cy + J1 * (cx * dy + cy * dx) + J2 * dx * dy);
        double g02 = h * (J0 * cx * cz + J1 * (cx * dz + cz * dx) + J2 * dx * dz);
        double g11 = h * (J0 * cy * cy + J1 * (2.0 * cy * dy) + J2 * dy * dy);
        double g12 = h * (J0 * cy * cz + J1 * (cy * dz + cz * dy) + J2 * dy * dz);
        double g22 = h * (J0 * cz * cz + J1 * (2.0 * cz * dz) + J2 * dz * dz);
        // a bound on the ellipsoid itself (q = 9 there) moves with the parameters: x = p + t d,
        // wb = +- w norm e^-4.5 / (2 A t + B), G_M -= wb x x^T, g_mean += 2 wb M x
        auto bound = [&](double t, double sg) {
            const double x = px + t * dx, y = py + t * dy, z = pz + t * dz;
            const double wb = sg * wn * 0.011108996538242306 / (2.0 * A * t + B);
            g00 -= wb * x * x, g01 -= wb * x * y, g02 -= wb * x * z;
            g11 -= wb * y * y, g12 -= wb * y * z, g22 -= wb * z * z;
            o0 += 2.0 * wb * (mpx + t * mdx);
            o1 += 2.0 * wb * (mpy + t * mdy);
            o2 += 2.0 * wb * (mpz + t * mdz);
        };
        if (mv_out) bound((double)b, 1.0);
        if (mv_in) bound((double)a, -1.0);
        double* row = acc + 10 * (size_t)j;
#ifdef VR_DIAG_GRAD_NO_ADD  // A/B: the per-hit arithmetic without its adds (kept alive by a comparison that never holds)
        if (o0 + o1 + o2 + g00 + g01 + g02 + g11 + g12 + g22 + s * J0 != 0x1.23456789abcdep+300) return;
#endif
        atomicAdd(row + 0, o0);
        atomicAdd(row + 1, o1);
        atomicAdd(row + 2, o2);
        atomicAdd(row + 3, g00);
        atomicAdd(row + 4, g01);
        atomicAdd(row + 5, g02);
        atomicAdd(row + 6, g11);
        atomicAdd(row + 7, g12);
        atomicAdd(row + 8, g22);
        atomicAdd(row + 9, s * J0);
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        ++cnt;
        const GRec g = load_rec(A.gauss, (int)j);
        const Quad q = quad(g, r);
        float t0, t1;
        if (intersect(q, t0, t1)) {  // (t0 is clamped to 0 already)
            const float b = fminf(tmax, t1);
            if (b > t0) add(g, r, t0, b, moving != 0u && t0 > 0.0f, moving != 0u && t1 <= tmax, j);
        }
        return true;
    }
    // (ProfileGradOp::redo has a copy of the take-back: through a shared helper the resource listing stayed but the
    // three stack pushes below gained a move each, and this query ran 0.4 % slower on 1000_random, 315.8 against 314.5 ms)
    __device__ __forceinline__ void redo(const RenderArgs& A, uint32_t id, const Ray& r, float tmax, float lim, int* stack) {
        if (cnt > 0) {
            uint32_t left = cnt;
            w = -w;
            auto prune = [&](float tmin, float) { return tmin <= lim; };
            auto leaf = [&](uint32_t first, uint32_t count) {
                for (uint32_t j = first; j < first + count && left > 0; ++j, --left) prim(A, r, tmax, j);
                return left > 0;
            };
            traverse_wide<kStackSize>(A, r, stack, kQBlock, prune, leaf);
            w = -w;
        }
        QueryOp::redo(A, id, r, tmax, lim, stack);
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t, float) {}
    __device__ __forceinline__ void invalid(uint32_t) {}
};

// The gradient of the ray's optical depth with respect to the ray itself, and the optical depth: row `id` of out
// (vr_ray_grad: d tau / d origin[3], d tau / d tmax, d tau / d direction[3], tau; include/vr_hip.h,
// vr_query_transmittance_ray_grad, has the formulas). Hit decisions, clip bounds and tau are TransOp<true>'s, f32 and
// bit for bit; everything else on a decided hit is double. The seven sums and TransOp's stay in registers and are
// rounded once in finish(), so nothing is written before it: the base redo() (reset, the whole walk again) is right
// as it stands, and there are no atomics.
struct RayGradOp : QueryOp<RayGradOp, true> {
    vr_ray_grad* out;
    uint32_t moving;   // the ellipsoid's own bounds move with the ray (not VR_GRAD_FROZEN_BOUNDS)
    float dx, dy, dz;  // the direction the walk uses
    float len2;        // the loader's f32 squared norm of the stored direction; 0: `unit` was set, no chain through v / |v|
    double o0, o1, o2, d0, d1, d2, gt, sum;
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const int what = QueryOp::load(A, id, r, tmax);
        const float4 b = reinterpret_cast<const float4*>(rays)[2 * (size_t)id + 1];
        len2 = b.w != 0.0f ? 0.0f : dot3(b.x, b.y, b.z, b.x, b.y, b.z);
        dx = r.dx, dy = r.dy, dz = r.dz;
        return what;
    }
    __device__ __forceinline__ void reset() { o0 = o1 = o2 = d0 = d1 = d2 = gt = sum = 0.0; }
    __device__ void add(const GRec& g, const Ray& r, float a, float b, bool mv_in, bool mv_out, bool clipped) {
        const HitMoments h = hit_moments(g, r, a, b);
        const double rn = (double)g.density * (double)g.norm;
        const double s = rn * h.k;
        // g_o = -s M (c J0 + d J1), g_d = -s M (m c J0 + (c + m d) J1 + d J2) = -s M (m v + c J1 + d J2)
        const double vx = h.cx * h.J0 + h.dx * h.J1, vy = h.cy * h.J0 + h.dy * h.J1, vz = h.cz * h.J0 + h.dz * h.J1;
        const double ux = h.m * vx + h.cx * h.J1 + h.dx * h.J2, uy = h.m * vy + h.cy * h.J1 + h.dy * h.J2,
                     uz = h.m * vz + h.cz * h.J1 + h.dz * h.J2;
        double go0 = -s * (h.m00 * vx + h.m01 * vy + h.m02 * vz);
        double go1 = -s * (h.m01 * vx + h.m11 * vy + h.m12 * vz);
        double go2 = -s * (h.m02 * vx + h.m12 * vy + h.m22 * vz);
        double gd0 = -s * (h.m00 * ux + h.m01 * uy + h.m02 * uz);
        double gd1 = -s * (h.m01 * ux + h.m11 * uy + h.m12 * uz);
        double gd2 = -s * (h.m02 * ux + h.m12 * uy + h.m22 * uz);
        // a bound on the ellipsoid itself (q = 9 there) moves with the ray: x = p + t d,
        // wb = +- rho norm e^-4.5 / (2 A t + B), g_o -= 2 wb M x, g_d -= 2 wb t M x
        auto bound = [&](double t, double sg) {
            const double wb = 2.0 * sg * rn * 0.011108996538242306 / (2.0 * h.A * t + h.B);
            const double x = wb * (h.mpx + t * h.mdx), y = wb * (h.mpy + t * h.mdy), z = wb * (h.mpz + t * h.mdz);
            go0 -= x, go1 -= y, go2 -= z;
            gd0 -= t * x, gd1 -= t * y, gd2 -= t * z;
        };
        if (mv_out) bound((double)b, 1.0);
        if (mv_in) bound((double)a, -1.0);
        o0 += go0, o1 += go1, o2 += go2;
        d0 += gd0, d1 += gd1, d2 += gd2;
        if (clipped) gt += s * h.eb;  // the upper bound is tmax itself: the integrand there
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        const Quad q = quad(g, r);
        float t0, t1;
        if (intersect(q, t0, t1)) {
            const float a = fmaxf(0.0f, t0);
            const float b = fminf(tmax, t1);
            if (b > a) {
                sum += (double)optical_depth(g, q, a, b);
                add(g, r, a, b, moving != 0u && t0 > 0.0f, moving != 0u && t1 <= tmax, t1 > tmax);
            }
        }
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        double e0 = d0, e1 = d1, e2 = d2;
        if (len2 != 0.0f) {  // the library normalised v: (g_d - d (d . g_d)) / |v|
            const double x = dx, y = dy, z = dz;
            const double dot = x * d0 + y * d1 + z * d2, len = sqrt((double)len2);
            e0 = (d0 - x * dot) / len, e1 = (d1 - y * dot) / len, e2 = (d2 - z * dot) / len;
        }
        float4* p = reinterpret_cast<float4*>(out) + 2 * (size_t)id;
        p[0] = make_float4((float)o0, (float)o1, (float)o2, (float)gt);
        p[1] = make_float4((float)e0, (float)e1, (float)e2, (float)sum);
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        const float q = __builtin_nanf("");
        float4* p = reinterpret_cast<float4*>(out) + 2 * (size_t)id;
        p[0] = p[1] = make_float4(q, q, q, q);
    }
};

template <bool TAU>
__global__ void __launch_bounds__(kQBlock) query_transmittance_kernel(RenderArgs A, const vr_ray* __restrict__ rays, uint32_t n,
                                                                      float* __restrict__ tr, float* __restrict__ tau,
                                                                      uint32_t* __restrict__ next, int refill) {
    TransOp<TAU> op;
    op.rays = rays;
    op.tr = tr;
    op.tau = tau;
    op.sum = 0.0;
    query_walk(A, n, next, refill, op);
}

__global__ void __launch_bounds__(kQBlock) query_events_count_kernel(RenderArgs A, const vr_ray* __restrict__ rays, uint32_t n,
                                                                     uint32_t* __restrict__ counts, uint32_t* __restrict__ next,
                                                                     int refill) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[n] = 0;  // the scan's last input: offsets[n] = total
    EventCountOp op;
    op.rays = rays;
    op.counts = counts;
    op.cnt = 0;
    query_walk(A, n, next, refill, op);
}

__global__ void __launch_bounds__(kQBlock) query_events_fill_kernel(RenderArgs A, const vr_ray* __restrict__ rays, uint32_t n,
                                                                    const uint32_t* __restrict__ offsets,
                                                                    unsigned long long* __restrict__ keys, unsigned long long cap,
                                                                    uint32_t* __restrict__ next, int refill) {
    EventFillOp op;
    op.rays = rays;
    op.offsets = offsets;
    op.keys = keys;
    op.cap = cap;
    op.base = op.room = op.w = 0;
    query_walk(A, n, next, refill, op);
}

__global__ void __launch_bounds__(kQBlock) query_grad_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                             const float* __restrict__ weight, uint32_t n, uint32_t moving,
                                                             double* __restrict__ acc, uint32_t* __restrict__ next, int refill) {
    GradOp op;
    op.rays = rays;
    op.weight = weight;
    op.acc = acc;
    op.moving = moving;
    op.w = 0.0f;
    op.cnt = 0;
    query_walk(A, n, next, refill, op);
}

__global__ void __launch_bounds__(kQBlock) query_ray_grad_kernel(RenderArgs A, const vr_ray* __restrict__ rays, uint32_t n,
                                                                 uint32_t moving, vr_ray_grad* __restrict__ out,
                                                                 uint32_t* __restrict__ next, int refill) {
    RayGradOp op;
    op.rays = rays;
    op.out = out;
    op.moving = moving;
    op.dx = op.dy = op.dz = op.len2 = 0.0f;
    op.reset();
    query_walk(A, n, next, refill, op);
}

// Staging row j (tree order, in M's space, W doubles) -> the caller's row gauss_order[j] (W floats): d/d mean[3],
// d/d cov {xx, xy, xz, yy, yz, zz}, d/d density and, for W = 11, d/d albedo. T = rho U, G_Sigma = -M G_M M - T M / 2,
// all in double and rounded to f32 once; an off-diagonal stored number stands at (i, j) and (j, i), hence twice
// G_Sigma[i][j]. The two widths are the two stagings, each with its own expressions (they decide signed zeros):
//   W = 10 (the transmittance and profile gradients): g_mean, G_M and U are staged per unit density, rho multiplies here;
//   W = 11 (the sigma gradient): they carry the density already, and every output gets + 0.0.
template <int W>
__global__ void __launch_bounds__(256) query_grad_finish_kernel(const GaussianRecord* __restrict__ gauss,
                                                                const uint32_t* __restrict__ order,
                                                                const double* __restrict__ acc, uint32_t n,
                                                                float* __restrict__ grad) {
    static_assert(W == 10 || W == 11, "a staging row is 10 or 11 doubles");
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const GRec g = load_rec(gauss, (int)j);
    const double* a = acc + W * (size_t)j;
    const double rho = g.density, U = a[9], T = rho * U;
    auto staged = [&](int k) {
        if constexpr (W == 10) return rho * a[k];
        else return a[k];
    };
    const double M[3][3] = {{g.m00, g.m01, g.m02}, {g.m01, g.m11, g.m12}, {g.m02, g.m12, g.m22}};
    const double G[3][3] = {{staged(3), staged(4), staged(5)}, {staged(4), staged(6), staged(7)}, {staged(5), staged(7), staged(8)}};
    double MG[3][3], S[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) MG[r][c] = M[r][0] * G[0][c] + M[r][1] * G[1][c] + M[r][2] * G[2][c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[r][c] = -(MG[r][0] * M[0][c] + MG[r][1] * M[1][c] + MG[r][2] * M[2][c]) - 0.5 * T * M[r][c];
    float* out = grad + W * (size_t)order[j];
    // (+ 0.0: a Gaussian that nothing hit gets +0, not the -0 of -(0) - 0)
    if constexpr (W == 10) {
        out[0] = (float)(rho * a[0]);
        out[1] = (float)(rho * a[1]);
        out[2] = (float)(rho * a[2]);
    } else {
        out[0] = (float)(a[0] + 0.0);
        out[1] = (float)(a[1] + 0.0);
        out[2] = (float)(a[2] + 0.0);
    }
    out[3] = (float)(S[0][0] + 0.0);
    out[4] = (float)(2.0 * S[0][1] + 0.0);
    out[5] = (float)(2.0 * S[0][2] + 0.0);
    out[6] = (float)(S[1][1] + 0.0);
    out[7] = (float)(2.0 * S[1][2] + 0.0);
    out[8] = (float)(S[2][2] + 0.0);
    if constexpr (W == 10) {
        out[9] = (float)U;
    } else {
        out[9] = (float)(U + 0.0);
        out[10] = (float)(a[10] + 0.0);
    }
}

// Sorted keys -> the caller's arrays: t, and ev = scene_index << 1 | entering.
__global__ void __launch_bounds__(256) query_events_unpack_kernel(const unsigned long long* __restrict__ keys,
                                                                  unsigned long long total, float* __restrict__ t,
                                                                  uint32_t* __restrict__ ev) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = keys[i];
    t[i] = __uint_as_float((uint32_t)(k >> 32));
    ev[i] = (uint32_t)k ^ 1u;
}

// ---- sigma: containment walk, one point per lane (sigma_active and the two walks: vr_query_common.h) ----
struct SigmaAcc {
    double sum, sum_alb;
    uint32_t cnt;
    __device__ __forceinline__ void reset() {
        sum = sum_alb = 0.0;
        cnt = 0;
    }
    __device__ __forceinline__ void leaf(const RenderArgs& A, int32_t ref, float x, float y, float z) {
        const uint32_t first = leaf_first(ref), end = first + leaf_count(ref);
        for (uint32_t j = first; j < end; ++j) {
            const GRec g = load_rec(A.gauss, (int)j);
            if (sigma_active(g, x, y, z)) {
                const float m = mu_t(g, x, y, z);
                sum += (double)m;
                sum_alb += (double)(m * g.albedo);
                ++cnt;
            }
        }
    }
};

// The gradient of sigma at the point (include/vr_hip.h, vr_query_sigma_grad, has the formulas): on every active
// Gaussian (sigma_active, f32) the record and the point are read as doubles, p = x - mean, q = p.Mp,
// e = norm exp(-q / 2), m = rho e, c = w_a (1 - alpha) + w_s alpha.
//   GAUSS:  eleven atomic adds into the staging row acc[11 j .. 11 j + 10] of record j (tree order): g_mean = c m M p,
//           G_M {00, 01, 02, 11, 12, 22} = -c m p p^T / 2, U = c e and g_albedo = (w_s - w_a) m, each times `sg`
//           (global_atomic_add_f64, arrival order, as GradOp::add). sg = -1 takes a walk's adds back: the walk
//           hands the same Gaussians out again, see query_sigma_grad_kernel.
//   POINTS: g_x = -c m M p summed in registers.
// `mass` is the double sum of m (the point contributes iff it is > 0), cnt the Gaussians added.
// The points-only instantiation has no staging pointer to carry and no atomics.
template <bool GAUSS>
struct SigmaGradStage {};
template <>
struct SigmaGradStage<true> {
    double* acc;
    double sg;
};
template <bool POINTS>
struct SigmaGradSum {};
template <>
struct SigmaGradSum<true> {
    double gx, gy, gz;
};
template <bool GAUSS, bool POINTS>
struct SigmaGradAcc : SigmaGradStage<GAUSS>, SigmaGradSum<POINTS> {
    double wa, ws, mass;
    uint32_t cnt;
    __device__ __forceinline__ void reset() {
        this->mass = 0.0;
        this->cnt = 0;
        if constexpr (POINTS) this->gx = this->gy = this->gz = 0.0;
    }
    __device__ __forceinline__ void leaf(const RenderArgs& A, int32_t ref, float x, float y, float z) {
        const uint32_t first = leaf_first(ref), end = first + leaf_count(ref);
        for (uint32_t j = first; j < end; ++j) {
            const GRec g = load_rec(A.gauss, (int)j);
            if (!sigma_active(g, x, y, z)) continue;
            const double px = (double)x - (double)g.mx, py = (double)y - (double)g.my, pz = (double)z - (double)g.mz;
            const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
            const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz,
                         mpz = m02 * px + m12 * py + m22 * pz;
            const double q = px * mpx + py * mpy + pz * mpz;
            const double e = (double)g.norm * exp(-0.5 * q), m = (double)g.density * e;
            const double alpha = g.albedo;
            const double c = this->wa * (1.0 - alpha) + this->ws * alpha, cm = c * m;
            this->mass += m;
            ++this->cnt;
            if constexpr (POINTS) {
                this->gx -= cm * mpx;
                this->gy -= cm * mpy;
                this->gz -= cm * mpz;
            }
            if constexpr (GAUSS) {
                const double s = this->sg * cm, h = -0.5 * s;
                double* row = this->acc + 11 * (size_t)j;
                atomicAdd(row + 0, s * mpx);
                atomicAdd(row + 1, s * mpy);
                atomicAdd(row + 2, s * mpz);
                atomicAdd(row + 3, h * px * px);
                atomicAdd(row + 4, h * px * py);
                atomicAdd(row + 5, h * px * pz);
                atomicAdd(row + 6, h * py * py);
                atomicAdd(row + 7, h * py * pz);
                atomicAdd(row + 8, h * pz * pz);
                atomicAdd(row + 9, this->sg * (c * e));
                atomicAdd(row + 10, this->sg * ((this->ws - this->wa) * m));
            }
        }
    }
};

__global__ void __launch_bounds__(kQBlock) query_sigma_kernel(RenderArgs A, const float* __restrict__ xyz, uint32_t n,
                                                              float* __restrict__ out, uint32_t* __restrict__ n_active) {
    __shared__ int s_stack[kStackSize * kQBlock];
    int* stack = s_stack + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    SigmaAcc acc;
    acc.reset();
    bool redo = A.hnodes4 == nullptr;
    if (A.num_prims > 0 && !redo) redo = sigma_walk_wide(A, x, y, z, stack, acc);
    if (A.num_prims > 0 && redo) {
        acc.reset();
        if (sigma_walk_pair(A, x, y, z, stack, acc)) {
            out[2 * i] = out[2 * i + 1] = __builtin_nanf("");
            if (n_active) n_active[i] = 0;
            return;
        }
    }
    // gmm.h:115-125
    const float sum = (float)acc.sum, sum_alb = (float)acc.sum_alb;
    float sa = 0.0f, ss = 0.0f;
    if (!(sum <= 0.0f)) {
        const float a_mix = __fdiv_rn(sum_alb, sum);
        ss = a_mix * sum;
        sa = (1.0f - a_mix) * sum;
    }
    out[2 * i] = sa;
    out[2 * i + 1] = ss;
    if (n_active) n_active[i] = acc.cnt;
}

// One point of the sigma gradient: query_sigma_kernel's walks with the gradient's leaf accumulator. The adds to the
// staging rows happen while a walk runs, so a walk whose adds must not stand is taken back by walking it again with
// sg = -1: the walk is a function of the point and the tree alone, so it hands out the same Gaussians and breaks off
// at the same node. That happens to a 4-wide walk that broke off for its stack (the child-pair walk then adds the
// whole active set), to a child-pair walk deeper than the builder allows (the forward's NaN case) and to a point whose
// summed m is <= 0 (the forward's (0, 0): non-positive densities only). None of it is on the path of an ordinary
// point, and the loop keeps one inlined copy of each walk. The points-only form has nothing to take back.
template <bool GAUSS, bool POINTS>
__device__ __forceinline__ void sigma_grad_point(const RenderArgs& A, const float* __restrict__ xyz,
                                                 const float* __restrict__ weight_as, uint32_t n,
                                                 SigmaGradAcc<GAUSS, POINTS>& acc, float* __restrict__ grad_xyz) {
    __shared__ int s_stack[kStackSize * kQBlock];
    int* stack = s_stack + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    acc.wa = weight_as ? (double)weight_as[2 * i] : 1.0;
    acc.ws = weight_as ? (double)weight_as[2 * i + 1] : 1.0;
    acc.reset();
    if constexpr (GAUSS) acc.sg = 1.0;
    bool wide = A.hnodes4 != nullptr, bad = false, dead = true;
    int undo = 0;  // 1: taking a broken-off 4-wide walk back, the child-pair walk follows; 2: taking the point back
    while (A.num_prims > 0) {
        const bool broke = wide ? sigma_walk_wide(A, x, y, z, stack, acc) : sigma_walk_pair(A, x, y, z, stack, acc);
        if constexpr (GAUSS) {
            if (undo == 2) break;
            if (undo == 1) {
                undo = 0;
                acc.sg = 1.0;
                wide = false;
                acc.reset();
                continue;
            }
        }
        if (wide && broke) {
            if (GAUSS && acc.cnt > 0) {
                undo = 1;
                if constexpr (GAUSS) acc.sg = -1.0;
                continue;
            }
            wide = false;
            acc.reset();
            continue;
        }
        bad = broke;
        dead = bad || acc.mass <= 0.0;
        if (GAUSS && dead && acc.cnt > 0) {
            undo = 2;
            if constexpr (GAUSS) acc.sg = -1.0;
            continue;
        }
        break;
    }
    if constexpr (POINTS) {
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        if (bad) ox = oy = oz = __builtin_nanf("");
        else if (!dead) ox = (float)acc.gx, oy = (float)acc.gy, oz = (float)acc.gz;
        grad_xyz[3 * i] = ox;
        grad_xyz[3 * i + 1] = oy;
        grad_xyz[3 * i + 2] = oz;
    }
}

template <bool POINTS>
__global__ void __launch_bounds__(kQBlock) query_sigma_grad_kernel(RenderArgs A, const float* __restrict__ xyz,
                                                                   const float* __restrict__ weight_as, uint32_t n,
                                                                   double* __restrict__ stage, float* __restrict__ grad_xyz) {
    SigmaGradAcc<true, POINTS> acc;
    acc.acc = stage;
    sigma_grad_point<true, POINTS>(A, xyz, weight_as, n, acc, grad_xyz);
}

// grad sigma at the points alone: no staging, no atomics.
__global__ void __launch_bounds__(kQBlock) query_sigma_grad_points_kernel(RenderArgs A, const float* __restrict__ xyz,
                                                                          const float* __restrict__ weight_as, uint32_t n,
                                                                          float* __restrict__ grad_xyz) {
    SigmaGradAcc<false, true> acc;
    sigma_grad_point<false, true>(A, xyz, weight_as, n, acc, grad_xyz);
}

// Device-side packing of the Python mirror's torch inputs into vr_ray rows (tmax: one value per ray, or one
// for all with tmax_stride = 0).
__global__ void __launch_bounds__(256) query_pack_rays_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                              const float* __restrict__ tmax, uint32_t tmax_stride, uint32_t n,
                                                              vr_ray* __restrict__ rays) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4* p = reinterpret_cast<float4*>(rays) + 2 * i;
    p[0] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], tmax[(size_t)tmax_stride * i]);
    p[1] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.0f);
}

struct ToU64 {
    __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t v) const { return v; }
};

}  // namespace dev

// ---- launchers (host/vr_device.cpp) ----
hipError_t query_transmittance(const RenderArgs& A, const vr_ray* rays, uint32_t n, float* tr, float* tau, uint32_t* next,
                               int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (tau) hipLaunchKernelGGL(dev::query_transmittance_kernel<true>, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, n, tr, tau, next, refill);
    else hipLaunchKernelGGL(dev::query_transmittance_kernel<false>, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, n, tr, tau, next, refill);
    return hipGetLastError();
}

// The staging rows of the scene's Gaussians (width 10 or 11 doubles each, query_grad_finish_kernel) -> grad, as many
// floats per Gaussian. The profile gradient's unit calls it too.
hipError_t query_grad_finish(const RenderArgs& A, const double* acc, int width, float* grad, hipStream_t s) {
    const dim3 grid(((uint32_t)A.num_prims + 255u) / 256u), block(256);
    if (width == 10) hipLaunchKernelGGL(dev::query_grad_finish_kernel<10>, grid, block, 0, s, A.gauss, A.gauss_order, acc, (uint32_t)A.num_prims, grad);
    else hipLaunchKernelGGL(dev::query_grad_finish_kernel<11>, grid, block, 0, s, A.gauss, A.gauss_order, acc, (uint32_t)A.num_prims, grad);
    return hipGetLastError();
}

// acc: 10 doubles per Gaussian of staging, zeroed here; grad: 10 floats per Gaussian, every one written.
hipError_t query_transmittance_grad(const RenderArgs& A, const vr_ray* rays, const float* weight, uint32_t n, bool moving,
                                    double* acc, float* grad, uint32_t* next, int refill, int cus, hipStream_t s) {
    if (A.num_prims <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(acc, 0, (size_t)A.num_prims * 10 * sizeof(double), s)) != hipSuccess) return e;
    if (n > 0) {
        hipLaunchKernelGGL(dev::query_grad_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, weight, n, moving ? 1u : 0u,
                           acc, next, refill);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return query_grad_finish(A, acc, 10, grad, s);
}

// out: one vr_ray_grad row per ray, every one written.
hipError_t query_transmittance_ray_grad(const RenderArgs& A, const vr_ray* rays, uint32_t n, bool moving, vr_ray_grad* out,
                                        uint32_t* next, int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::query_ray_grad_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, n, moving ? 1u : 0u, out,
                       next, refill);
    return hipGetLastError();
}

hipError_t query_sigma(const RenderArgs& A, const float* xyz, uint32_t n, float* out, uint32_t* n_active, hipStream_t s) {
    hipLaunchKernelGGL(dev::query_sigma_kernel, dim3((n + dev::kQBlock - 1) / dev::kQBlock), dim3(dev::kQBlock), 0, s, A, xyz, n,
                       out, n_active);
    return hipGetLastError();
}

// stage: 11 doubles per Gaussian of staging, zeroed here; grad: 11 floats per Gaussian, every one written; grad_xyz: 3
// floats per point, every one written. Either output may be nullptr: without grad there is no staging and no atomic.
hipError_t query_sigma_grad(const RenderArgs& A, const float* xyz, const float* weight_as, uint32_t n, double* stage, float* grad,
                            float* grad_xyz, hipStream_t s) {
    const dim3 grid((n + dev::kQBlock - 1) / dev::kQBlock), block(dev::kQBlock);
    hipError_t e;
    if (!grad || A.num_prims <= 0) {  // (an empty scene: grad has no entries)
        if (grad_xyz && n > 0) hipLaunchKernelGGL(dev::query_sigma_grad_points_kernel, grid, block, 0, s, A, xyz, weight_as, n, grad_xyz);
        return hipGetLastError();
    }
    if ((e = hipMemsetAsync(stage, 0, (size_t)A.num_prims * 11 * sizeof(double), s)) != hipSuccess) return e;
    if (n > 0) {
        if (grad_xyz) hipLaunchKernelGGL(dev::query_sigma_grad_kernel<true>, grid, block, 0, s, A, xyz, weight_as, n, stage, grad_xyz);
        else hipLaunchKernelGGL(dev::query_sigma_grad_kernel<false>, grid, block, 0, s, A, xyz, weight_as, n, stage, grad_xyz);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return query_grad_finish(A, stage, 11, grad, s);
}

// counts: n + 1 words of scratch; offsets: n + 1 words (exclusive scan of the counts, offsets[n] = the
// total modulo 2^32); total: the 64-bit sum. tmp == nullptr: only tmp_bytes is set.
hipError_t query_events_count(const RenderArgs& A, const vr_ray* rays, uint32_t n, uint32_t* counts, uint32_t* offsets,
                              unsigned long long* total, uint32_t* next, int refill, int cus, void* tmp, size_t& tmp_bytes,
                              hipStream_t s) {
    hipcub::TransformInputIterator<unsigned long long, dev::ToU64, const uint32_t*> it(counts, dev::ToU64());
    if (!tmp) {
        size_t a = 0, b = 0;
        hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, a, counts, offsets, (int)(n + 1), s);
        if (e != hipSuccess) return e;
        e = hipcub::DeviceReduce::Sum(nullptr, b, it, total, (int)(n + 1), s);
        tmp_bytes = std::max(a, b);
        return e;
    }
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::query_events_count_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, n, counts, next, refill);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = tmp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, offsets, (int)(n + 1), s)) != hipSuccess) return e;
    bytes = tmp_bytes;
    return hipcub::DeviceReduce::Sum(tmp, bytes, it, total, (int)(n + 1), s);
}

// keys / keys2: `total` 64-bit words each. tmp == nullptr: only tmp_bytes is set.
hipError_t query_events_fill(const RenderArgs& A, const vr_ray* rays, uint32_t n, const uint32_t* offsets, uint32_t total,
                             unsigned long long* keys, unsigned long long* keys2, float* t, uint32_t* ev, uint32_t* next,
                             int refill, int cus, void* tmp, size_t& tmp_bytes, hipStream_t s) {
    if (!tmp) return rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, keys, keys2, total, n, offsets, offsets + 1, 0, 63, s);
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::query_events_fill_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, n, offsets, keys,
                       (unsigned long long)total, next, refill);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = tmp_bytes;
    if ((e = rocprim::segmented_radix_sort_keys(tmp, bytes, keys, keys2, total, n, offsets, offsets + 1, 0, 63, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::query_events_unpack_kernel, dim3((unsigned)(((unsigned long long)total + 255u) / 256u)), dim3(256), 0, s,
                       keys2, (unsigned long long)total, t, ev);
    return hipGetLastError();
}

hipError_t query_pack_rays(const float* o, const float* d, const float* tmax, uint32_t tmax_stride, uint32_t n, vr_ray* rays,
                           hipStream_t s) {
    hipLaunchKernelGGL(dev::query_pack_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, o, d, tmax, tmax_stride, n, rays);
    return hipGetLastError();
}

}  // namespace vr
