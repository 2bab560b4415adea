// The transmittance profile query (include/vr_hip.h, vr_query_transmittance_profile): tau and Tr at K distances along
// each ray from one tree walk, and the gradient of a weighted sum of those K optical depths with respect to the
// Gaussians from one walk and one row of ten atomic adds per (ray, Gaussian) hit.
//
// Both are operations on the persistent ray-queue walk (ray_queue_walk, vr_walk.h) through the base and the block shape
// of the other ray queries (QueryOp, query_walk: vr_query_common.h), in a unit of their own so that no kernel of
// vr_query.hip is compiled differently for them.
//
// Forward. In optical_depth(g, q, a, b) (vr_march.h) only F1 = erff((B + 2A b) / den) depends on the upper bound: pref,
// den, F0 and e are one hit's, whatever the sample. A work item is (ray, chunk of kProfileChunk samples): its sums are
// kProfileChunk doubles in registers (every loop over them is unrolled: a dynamically indexed array would live in
// scratch), its walk is pruned at the chunk's largest sample, and per hit it evaluates the shared head once and one
// erff per sample whose bound b = min(t_k, t_exit) lies past a = max(0, t_enter). That is optical_depth's operation
// sequence for the ray (origin, direction, tmax = t_k), term by term, and the terms are added in double, where the
// order does not matter: tau[i][k] and tr[i][k] have the bits vr_query_transmittance returns for that ray. A sample that
// is not > 0 (NaN included) is walked as 0: no term passes b > a, so tau = 0 and tr = 1.
//
// Gradient. Per decided hit the gradient of vr_query_transmittance_grad is linear in the moments J0, J1, J2 over
// [u_a, u_b] and in the two boundary terms, and of those only u_b depends on the sample. So for one (ray, Gaussian) hit,
// with a = max(0, t_enter) and t1 = t_exit (f32, the forward's), the K weighted samples fold:
//   t_k <= a, or not > 0     nothing
//   t_k >= t1                the whole chord: W_full += w_k
//   a < t_k < t1             u_b = t_k - m: (S0, S1, S2) += w_k (J0, J1, J2)(u_b), W_in += w_k
//   then once                (S0, S1, S2) += W_full (J0, J1, J2)(t1 - m)
// and the ten outputs are GradOp::add's with (J0, J1, J2) = (S0, S1, S2) and w = 1, the exit's boundary term (t1 <= t_k:
// the whole-chord class alone) weighted W_full and the entry's (t_enter > 0: every sample that contributes) W_full + W_in.
// The head (p, M d, M p, A, B, C, m, c, k, u_a, erf(u_a sqrt(A / 2)), e^{-A u_a^2 / 2}) is computed once per hit, the
// samples and weights are read from global memory per hit (a shared row is one address for the wave), and nothing is
// kept per ray but the pointers. One walk per ray, pruned at the ray's largest sample.
#include "../host/vr_kernels.h"  // query_grad_finish (vr_query.hip)
#include "vr_query_common.h"

namespace vr {
namespace dev {

#ifndef VR_PROFILE_KC
#define VR_PROFILE_KC 16  // samples per work item of the forward walk (DESIGN.md 3e has the 4 / 8 / 16 comparison)
#endif
constexpr int kProfileChunk = VR_PROFILE_KC;

template <int KC>
struct ProfileOp : QueryOp<ProfileOp<KC>, true> {
    using Base = QueryOp<ProfileOp<KC>, true>;
    const float* __restrict__ t;
    float* tr;
    float* tau;
    uint32_t t_stride, K, chunks;
    float ts[KC];    // the chunk's samples (0: not > 0, or past the row's end)
    double sum[KC];
    // item id = ray * chunks + chunk
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const uint32_t ray = id / chunks, first = (id - ray * chunks) * (uint32_t)KC;
        const int what = Base::load(A, ray, r, tmax);  // (the row's own tmax is not used)
        const float* row = t + (size_t)t_stride * ray + first;
        float hi = 0.0f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float v = first + (uint32_t)k < K ? row[k] : 0.0f;
            ts[k] = v > 0.0f ? v : 0.0f;
            hi = fmaxf(hi, ts[k]);
        }
        tmax = hi;
        if (what == kRayInvalid) return what;
        return !(hi > 0.0f) || A.num_prims <= 0 ? kRayFinish : kRayWalk;
    }
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int k = 0; k < KC; ++k) sum[k] = 0.0;
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        const Quad q = quad(g, r);
        float t0, t1;
        if (intersect(q, t0, t1)) {
            const float a = fmaxf(0.0f, t0);
            if (fminf(tmax, t1) > a) {  // (the largest sample's test: no other sample passes where it fails)
                // optical_depth(g, q, a, b), vr_march.h, with everything but F1 taken out of the loop over b
                const float twoA = 2.0f * q.A;
                const float pref = (g.density * g.norm) * sqrtf(__fdiv_rn(3.14159265358979323846f, twoA));
                const float den = 2.0f * sqrtf(twoA);
                const float F0 = erff(__fdiv_rn(q.B + twoA * a, den));
                const float e = expf(-0.5f * (q.Cq - __fdiv_rn(q.B * q.B, 4.0f * q.A)));
                const float pe = pref * e;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const float b = fminf(ts[k], t1);
                    if (b > a) sum[k] += (double)(pe * (erff(__fdiv_rn(q.B + twoA * b, den)) - F0));
                }
            }
        }
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        const uint32_t ray = id / chunks, first = (id - ray * chunks) * (uint32_t)KC;
        const size_t o = (size_t)ray * K + first;
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (first + (uint32_t)k < K) {
                if (tr) tr[o + k] = expf(-(float)sum[k]);
                if (tau) tau[o + k] = (float)sum[k];
            }
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        const uint32_t ray = id / chunks, first = (id - ray * chunks) * (uint32_t)KC;
        const size_t o = (size_t)ray * K + first;
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (first + (uint32_t)k < K) {
                if (tr) tr[o + k] = __builtin_nanf("");
                if (tau) tau[o + k] = __builtin_nanf("");
            }
    }
};

// The staging rows, the order of the adds and the take-back of a walk that is redone are GradOp's (vr_query.hip): the
// first `cnt` Gaussians of the 4-wide walk are added again with the opposite sign before the pair-tree walk adds the
// ray's whole hit set.
struct ProfileGradOp : QueryOp<ProfileGradOp, true> {
    const float* __restrict__ t;
    const float* __restrict__ weight;
    double* acc;
    uint32_t t_stride, K;
    uint32_t moving;    // the ellipsoid's own bounds move with the parameters (not VR_GRAD_FROZEN_BOUNDS)
    double sg;          // +1, or -1 while a walk is taken back
    uint32_t cnt;       // Gaussians this walk has tested
    const float* row;   // the ray's K samples
    const float* wrow;  // and their weights (nullptr: ones)
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const int what = QueryOp::load(A, id, r, tmax);  // (the row's own tmax is not used)
        row = t + (size_t)t_stride * id;
        wrow = weight ? weight + (size_t)K * id : nullptr;
        float hi = 0.0f;
        for (uint32_t k = 0; k < K; ++k) hi = fmaxf(hi, row[k]);
        tmax = hi;
        if (what == kRayInvalid) return what;
        return !(hi > 0.0f) || A.num_prims <= 0 ? kRayFinish : kRayWalk;
    }
    __device__ __forceinline__ void reset() { cnt = 0; }
    // a = max(0, t_enter), t1 = t_exit, t1 > a and the ray's largest sample > a
    __device__ void add(const GRec& g, const Ray& r, float a, float t1, uint32_t j) {
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
        const double ua = (double)a - m;
        const double k = exp(-0.5 * (C - B * B / (4.0 * A)));
        const double sA = sqrt(0.5 * A), c0 = sqrt(3.14159265358979323846 / (2.0 * A));
        const double erfa = erf(ua * sA), ea = exp(-0.5 * A * ua * ua);
        double S0 = 0.0, S1 = 0.0, S2 = 0.0, Wf = 0.0, Wi = 0.0;
        auto moments = [&](float tb, double w) {
            const double ub = (double)tb - m;
            const double J0 = c0 * (erf(ub * sA) - erfa);
            const double eb = exp(-0.5 * A * ub * ub);
            S0 += w * J0;
            S1 += w * ((ea - eb) / A);
            S2 += w * ((ua * ea - ub * eb) / A + J0 / A);
        };
        for (uint32_t s = 0; s < K; ++s) {
            const float tk = row[s];
            if (!(tk > a)) continue;  // before the entry, or not > 0 (a >= 0), or NaN
            const double w = wrow ? (double)wrow[s] : 1.0;
            if (tk >= t1) {
                Wf += w;
            } else {
                moments(tk, w);
                Wi += w;
            }
        }
        if (Wf != 0.0) moments(t1, Wf);
        const double wn = sg * (double)g.norm;
        const double sk = wn * k;
        // g_mean = s M (c J0 + d J1)
        const double vx = cx * S0 + dx * S1, vy = cy * S0 + dy * S1, vz = cz * S0 + dz * S1;
        double o0 = sk * (m00 * vx + m01 * vy + m02 * vz);
        double o1 = sk * (m01 * vx + m11 * vy + m12 * vz);
        double o2 = sk * (m02 * vx + m12 * vy + m22 * vz);
        // G_M = -s/2 (J0 c c^T + J1 (c d^T + d c^T) + J2 d d^T)
        const double h = -0.5 * sk;
        double g00 = h * (S0 * cx * cx + S1 * (2.0 * cx * dx) + S2 * dx * dx);
        double g01 = h * (S0 * cx * cy + S1 * (cx * dy + cy * dx) + S2 * dx * dy);
        double g02 = h * (S0 * cx * cz + S1 * (cx * dz + cz * dx) + S2 * dx * dz);
        double g11 = h * (S0 * cy * cy + S1 * (2.0 * cy * dy) + S2 * dy * dy);
        double g12 = h * (S0 * cy * cz + S1 * (cy * dz + cz * dy) + S2 * dy * dz);
        double g22 = h * (S0 * cz * cz + S1 * (2.0 * cz * dz) + S2 * dz * dz);
        // a bound on the ellipsoid itself (q = 9 there) moves with the parameters: x = p + t d,
        // wb = +- W norm e^-4.5 / (2 A t + B), G_M -= wb x x^T, g_mean += 2 wb M x
        auto bound = [&](double tb, double W) {
            const double x = px + tb * dx, y = py + tb * dy, z = pz + tb * dz;
            const double wb = W * wn * 0.011108996538242306 / (2.0 * A * tb + B);
            g00 -= wb * x * x, g01 -= wb * x * y, g02 -= wb * x * z;
            g11 -= wb * y * y, g12 -= wb * y * z, g22 -= wb * z * z;
            o0 += 2.0 * wb * (mpx + tb * mdx);
            o1 += 2.0 * wb * (mpy + tb * mdy);
            o2 += 2.0 * wb * (mpz + tb * mdz);
        };
        if (moving != 0u && Wf != 0.0) bound((double)t1, Wf);
        if (moving != 0u && a > 0.0f) bound((double)a, -(Wf + Wi));
        double* out = acc + 10 * (size_t)j;
        atomicAdd(out + 0, o0);
        atomicAdd(out + 1, o1);
        atomicAdd(out + 2, o2);
        atomicAdd(out + 3, g00);
        atomicAdd(out + 4, g01);
        atomicAdd(out + 5, g02);
        atomicAdd(out + 6, g11);
        atomicAdd(out + 7, g12);
        atomicAdd(out + 8, g22);
        atomicAdd(out + 9, sk * S0);
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        ++cnt;
        const GRec g = load_rec(A.gauss, (int)j);
        const Quad q = quad(g, r);
        float t0, t1;
        if (intersect(q, t0, t1)) {  // (t0 is clamped to 0 already)
            if (fminf(tmax, t1) > t0) add(g, r, t0, t1, j);
        }
        return true;
    }
    __device__ __forceinline__ void redo(const RenderArgs& A, uint32_t id, const Ray& r, float tmax, float lim, int* stack) {
        if (cnt > 0) {
            uint32_t left = cnt;
            sg = -sg;
            auto prune = [&](float tmin, float) { return tmin <= lim; };
            auto leaf = [&](uint32_t first, uint32_t count) {
                for (uint32_t j = first; j < first + count && left > 0; ++j, --left) prim(A, r, tmax, j);
                return left > 0;
            };
            traverse_wide<kStackSize>(A, r, stack, kQBlock, prune, leaf);
            sg = -sg;
        }
        QueryOp::redo(A, id, r, tmax, lim, stack);
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t, float) {}
    __device__ __forceinline__ void invalid(uint32_t) {}
};

__global__ void __launch_bounds__(kQBlock) query_profile_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                const float* __restrict__ t, uint32_t t_stride, uint32_t items,
                                                                uint32_t K, uint32_t chunks, float* __restrict__ tr,
                                                                float* __restrict__ tau, uint32_t* __restrict__ next, int refill) {
    ProfileOp<kProfileChunk> op;
    op.rays = rays;
    op.t = t;
    op.tr = tr;
    op.tau = tau;
    op.t_stride = t_stride;
    op.K = K;
    op.chunks = chunks;
#pragma unroll
    for (int k = 0; k < kProfileChunk; ++k) op.ts[k] = 0.0f;
    op.reset();
    query_walk(A, items, next, refill, op);
}

__global__ void __launch_bounds__(kQBlock) query_profile_grad_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                     const float* __restrict__ t, uint32_t t_stride,
                                                                     const float* __restrict__ weight, uint32_t n, uint32_t K,
                                                                     uint32_t moving, double* __restrict__ acc,
                                                                     uint32_t* __restrict__ next, int refill) {
    ProfileGradOp op;
    op.rays = rays;
    op.t = t;
    op.weight = weight;
    op.acc = acc;
    op.t_stride = t_stride;
    op.K = K;
    op.moving = moving;
    op.sg = 1.0;
    op.cnt = 0;
    op.row = op.wrow = nullptr;
    query_walk(A, n, next, refill, op);
}

}  // namespace dev

// ---- launchers (host/vr_query_host.cpp) ----
// t: n * K floats (t_stride = K) or K (t_stride = 0); tr / tau: n * K floats each, either may be nullptr. n * K < 2^31.
hipError_t query_transmittance_profile(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, uint32_t n,
                                       uint32_t K, float* tr, float* tau, uint32_t* next, int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t chunks = (K + (uint32_t)dev::kProfileChunk - 1u) / (uint32_t)dev::kProfileChunk;
    hipLaunchKernelGGL(dev::query_profile_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, n * chunks, K,
                       chunks, tr, tau, next, refill);
    return hipGetLastError();
}

// acc: 10 doubles per Gaussian of staging, zeroed here; grad: 10 floats per Gaussian, every one written.
hipError_t query_transmittance_profile_grad(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride,
                                            const float* weight, uint32_t n, uint32_t K, bool moving, double* acc, float* grad,
                                            uint32_t* next, int refill, int cus, hipStream_t s) {
    if (A.num_prims <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(acc, 0, (size_t)A.num_prims * 10 * sizeof(double), s)) != hipSuccess) return e;
    if (n > 0) {
        hipLaunchKernelGGL(dev::query_profile_grad_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, weight, n,
                           K, moving ? 1u : 0u, acc, next, refill);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return query_grad_finish(A, acc, 10, grad, s);  // (vr_query.hip: GradOp's staging, so its finish)
}

// The same kernel adding into staging rows that the caller has zeroed (and may have added to) and finishes itself: the
// radiance gradient's second pass (vr_query_radiance_grad.hip). n > 0, A.num_prims > 0.
hipError_t query_transmittance_profile_grad_add(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride,
                                                const float* weight, uint32_t n, uint32_t K, bool moving, double* acc,
                                                uint32_t* next, int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::query_profile_grad_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, weight, n, K,
                       moving ? 1u : 0u, acc, next, refill);
    return hipGetLastError();
}

}  // namespace vr
