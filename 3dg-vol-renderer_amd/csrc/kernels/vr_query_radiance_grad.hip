// The radiance gradient query (include/vr_hip.h, vr_query_radiance_grad): the gradient of
//   l = sum_i ( sum_c w_ic L_ic + u_i opacity_i ),   L, opacity = vr_query_radiance's,
// with respect to the Gaussians, the feature rows, the quadrature weights q and the optical depths tau, from one walk per
// ray. Rays, samples, points, sample validity and the active set are the forward's (vr_query_radiance.hip) bit for bit:
// the same load, the same prefilter (radiance_interval), the point __fadd_rn(o, __fmul_rn(t, d)) and sigma_active.
//
// Because sum_k q T sum_g m f = sum_g f (sum_k q T m), a (ray, Gaussian) pair sums its samples in registers and issues
// its 10 + C atomic adds once, not once per sample. A work item is a ray (phi_ig = u_i + sum_c w_ic f_gc needs all C
// channels). Per candidate Gaussian, with a_ik = q_ik T_ik, p = x_ik - mean, e = norm exp(-p.Mp / 2), m = rho e, all in
// double from the f32 record, point, row and weights (vr_query_features_grad's arithmetic, not the forward's f32 mu_t):
//   the loop over the row's samples   E0 += a e, V += a e p (3), P += a e p p^T (6) in registers, and s[i][k] += phi m in
//                                     the ray's own row of an n * K double workspace (one lane owns the row: plain
//                                     loads and stores, no atomics)
//   once, if a sample was active      ten adds into the Gaussian's staging row, per unit density so that
//                                     query_grad_finish_kernel<10> converts it (phi M V, -phi P / 2, phi E0), and C adds
//                                     w_ic rho E0 into the feature staging
// phi is formed on the pair's first active sample (C multiply-adds and two row reads), so a candidate that the interval
// lets through but no sample activates costs neither; a query that asks for grad_features alone never forms it.
// finish writes grad_q[i][k] = f32(T s) and grad_tau[i][k] = f32(-(q T) s) from the row. The launcher then runs the
// profile gradient's kernel (vr_query_profile.hip, untouched) with grad_tau as its weights into the same staging, and
// one finish per staging: each output is rounded once.
//
// A walk that is redone for its stack (QueryOp::redo) first takes back what the broken-off 4-wide walk added, as
// ProfileGradOp::redo does: its first `cnt` Gaussians again with sg = -1; reset() re-zeroes the lane's s row.
// ATOMICS = false is the query for grad_q / grad_tau alone: no staging, no register sums, not a single atomic add.
#include "../host/vr_kernels.h"  // query_grad_finish (vr_query.hip), the two launchers of the other units
#include "vr_query_common.h"
#include "vr_radiance_interval.h"

namespace vr {
namespace dev {

template <bool ATOMICS>
struct RadianceGradOp : QueryOp<RadianceGradOp<ATOMICS>, true> {
    using Base = QueryOp<RadianceGradOp<ATOMICS>, true>;
    const float* __restrict__ t;
    const float* __restrict__ q;        // nullptr: ones
    const float* __restrict__ tr;       // the profile's Tr, n * K
    const float* __restrict__ feat;     // the caller's rows
    const float* __restrict__ weights;  // n * C, nullptr: ones
    const float* __restrict__ weight_opacity;  // n, nullptr: zeros
    double* s;        // n * K, nullptr: neither grad_q nor grad_tau nor grad is wanted (phi is not formed)
    double* stage;    // 10 per Gaussian (tree order) or nullptr
    double* fstage;   // C per Gaussian (tree order) or nullptr
    float* grad_q;    // n * K or nullptr
    float* grad_tau;  // n * K or nullptr
    uint32_t t_stride, q_stride, K, C;
    bool vec4;        // C is a multiple of 4 and the rows of feat and weights are 16-byte aligned
    const float* row;   // the ray's K samples,
    const float* qrow;  // their weights (nullptr: ones),
    const float* trow;  // their Tr,
    const float* wrow;  // the ray's C weights (nullptr: ones)
    double* srow;       // and its row of s
    double u;           // the ray's opacity weight
    double sg;          // +1, or -1 while a walk is taken back
    uint32_t cnt;       // Gaussians this walk has tested
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const int what = Base::load(A, id, r, tmax);  // (the row's own tmax is not used)
        row = t + (size_t)t_stride * id;
        qrow = q ? q + (size_t)q_stride * id : nullptr;
        trow = tr + (size_t)K * id;
        wrow = weights ? weights + (size_t)C * id : nullptr;
        srow = s ? s + (size_t)K * id : nullptr;
        u = weight_opacity ? (double)weight_opacity[id] : 0.0;
        float hi = -1.0f;  // the largest valid sample: finite and >= 0
        for (uint32_t k = 0; k < K; ++k) {
            const float v = row[k];
            if (v >= 0.0f && v < INFINITY) hi = fmaxf(hi, v);
        }
        tmax = fmaxf(hi, 0.0f);
        if (what == kRayInvalid) return what;
        // (a row whose valid samples are all at 0 walks: its origin may lie inside Gaussians)
        return hi < 0.0f || A.num_prims <= 0 ? kRayFinish : kRayWalk;
    }
    __device__ __forceinline__ void reset() {
        cnt = 0;
        if (srow)
            for (uint32_t k = 0; k < K; ++k) srow[k] = 0.0;
    }
    // phi = u + sum_c w_c f_c for tree record j
    __device__ __forceinline__ double phi_of(const RenderArgs& A, uint32_t j) const {
        const float* frow = feat + (size_t)A.gauss_order[j] * C;
        double c = u;
        if (vec4) {
            for (uint32_t k = 0; k < C; k += 4) {
                const float4 f = *reinterpret_cast<const float4*>(frow + k);
                float4 w = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
                if (wrow) w = *reinterpret_cast<const float4*>(wrow + k);
                c += (double)w.x * (double)f.x;
                c += (double)w.y * (double)f.y;
                c += (double)w.z * (double)f.z;
                c += (double)w.w * (double)f.w;
            }
        } else {
            for (uint32_t k = 0; k < C; ++k) c += (wrow ? (double)wrow[k] : 1.0) * (double)frow[k];
        }
        return c;
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        ++cnt;
        const GRec g = load_rec(A.gauss, (int)j);
        float lo, hi;
        if (!radiance_interval(g, r, tmax, lo, hi)) return true;
        const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
        double E0 = 0.0, V0 = 0.0, V1 = 0.0, V2 = 0.0, P00 = 0.0, P01 = 0.0, P02 = 0.0, P11 = 0.0, P12 = 0.0, P22 = 0.0;
        double phi = 0.0;
        bool have = false;
        for (uint32_t k = 0; k < K; ++k) {
            const float tk = row[k];
            if (!(tk >= lo && tk <= hi)) continue;  // outside the interval, or not valid (lo >= 0, hi <= tmax < inf)
            const float x = __fadd_rn(r.ox, __fmul_rn(tk, r.dx));
            const float y = __fadd_rn(r.oy, __fmul_rn(tk, r.dy));
            const float z = __fadd_rn(r.oz, __fmul_rn(tk, r.dz));
            if (!sigma_active(g, x, y, z)) continue;
            if (!have) {
                have = true;
                if (srow) phi = phi_of(A, j);
            }
            const double px = (double)x - (double)g.mx, py = (double)y - (double)g.my, pz = (double)z - (double)g.mz;
            const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz,
                         mpz = m02 * px + m12 * py + m22 * pz;
            const double e = (double)g.norm * exp(-0.5 * (px * mpx + py * mpy + pz * mpz));
            if (srow && sg > 0.0) srow[k] += phi * ((double)g.density * e);
            if constexpr (ATOMICS) {
                const double ae = ((qrow ? (double)qrow[k] : 1.0) * (double)trow[k]) * e;
                E0 += ae;
                V0 += ae * px, V1 += ae * py, V2 += ae * pz;
                P00 += ae * px * px, P01 += ae * px * py, P02 += ae * px * pz;
                P11 += ae * py * py, P12 += ae * py * pz, P22 += ae * pz * pz;
            }
        }
        if constexpr (ATOMICS) {
            if (!have) return true;
            if (stage) {
                const double c = sg * phi, h = -0.5 * c;
                double* out = stage + 10 * (size_t)j;
                atomicAdd(out + 0, c * (m00 * V0 + m01 * V1 + m02 * V2));
                atomicAdd(out + 1, c * (m01 * V0 + m11 * V1 + m12 * V2));
                atomicAdd(out + 2, c * (m02 * V0 + m12 * V1 + m22 * V2));
                atomicAdd(out + 3, h * P00);
                atomicAdd(out + 4, h * P01);
                atomicAdd(out + 5, h * P02);
                atomicAdd(out + 6, h * P11);
                atomicAdd(out + 7, h * P12);
                atomicAdd(out + 8, h * P22);
                atomicAdd(out + 9, c * E0);
            }
            if (fstage) {
                const double b = sg * ((double)g.density * E0);
                double* fst = fstage + (size_t)j * C;
                for (uint32_t k = 0; k < C; ++k) atomicAdd(fst + k, wrow ? (double)wrow[k] * b : b);
            }
        }
        return true;
    }
    __device__ __forceinline__ void redo(const RenderArgs& A, uint32_t id, const Ray& r, float tmax, float lim, int* stack) {
        if constexpr (ATOMICS) {
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
        }
        Base::redo(A, id, r, tmax, lim, stack);
    }
    // An invalid sample, and a sample that no pair reached (whatever its q), gets +0.
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        if (!srow) return;
        float* gq = grad_q ? grad_q + (size_t)K * id : nullptr;
        float* gt = grad_tau ? grad_tau + (size_t)K * id : nullptr;
        for (uint32_t k = 0; k < K; ++k) {
            const float tk = row[k];
            const double sk = tk >= 0.0f && tk < INFINITY ? srow[k] : 0.0;
            const double T = (double)trow[k];
            float vq = 0.0f, vt = 0.0f;
            if (sk != 0.0) {
                vq = (float)(T * sk);
                vt = (float)(-(((qrow ? (double)qrow[k] : 1.0) * T) * sk));
            }
            if (gq) gq[k] = vq;
            if (gt) gt[k] = vt;
        }
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        for (uint32_t k = 0; k < K; ++k) {
            if (grad_q) grad_q[(size_t)K * id + k] = __builtin_nanf("");
            if (grad_tau) grad_tau[(size_t)K * id + k] = __builtin_nanf("");
        }
    }
};

template <bool ATOMICS>
__global__ void __launch_bounds__(kQBlock) query_radiance_grad_kernel(
    RenderArgs A, const vr_ray* __restrict__ rays, const float* __restrict__ t, uint32_t t_stride, const float* __restrict__ q,
    uint32_t q_stride, uint32_t n, uint32_t K, const float* __restrict__ feat, uint32_t C, int vec4,
    const float* __restrict__ weights, const float* __restrict__ weight_opacity, const float* __restrict__ tr, double* s,
    double* stage, double* fstage, float* grad_q, float* grad_tau, uint32_t* __restrict__ next, int refill) {
    RadianceGradOp<ATOMICS> op;
    op.rays = rays;
    op.t = t;
    op.q = q;
    op.tr = tr;
    op.feat = feat;
    op.weights = weights;
    op.weight_opacity = weight_opacity;
    op.s = s;
    op.stage = stage;
    op.fstage = fstage;
    op.grad_q = grad_q;
    op.grad_tau = grad_tau;
    op.t_stride = t_stride;
    op.q_stride = q_stride;
    op.K = K;
    op.C = C;
    op.vec4 = vec4 != 0;
    op.row = op.qrow = op.trow = op.wrow = nullptr;
    op.srow = nullptr;
    op.u = 0.0;
    op.sg = 1.0;
    op.cnt = 0;
    query_walk(A, n, next, refill, op);
}

}  // namespace dev

// ---- launcher (host/vr_query_host.cpp) ----
// tr: n * K floats, the forward's (the caller's, or written by query_transmittance_profile earlier on s). s_rows: n * K
// doubles, needed unless grad_features is the only output. stage: 10 doubles per Gaussian, needed with grad; fstage: C per
// Gaussian, needed with grad_features; both zeroed here. tau_ws: n * K floats, needed when grad is asked for without
// grad_tau. next: three counter words. Every entry of a given output is written. n > 0; at least one output.
hipError_t query_radiance_grad(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, const float* q,
                               uint32_t q_stride, uint32_t n, uint32_t K, const float* feat, uint32_t C, const float* weights,
                               const float* weight_opacity, const float* tr, bool moving, double* s_rows, double* stage,
                               double* fstage, float* tau_ws, float* grad, float* grad_features, float* grad_q, float* grad_tau,
                               uint32_t* next, int refill, int cus, hipStream_t s) {
    const size_t N = (size_t)std::max(A.num_prims, 0);
    if (N == 0) grad = grad_features = nullptr;  // (no rows to write)
    if (!grad) stage = nullptr;
    if (!grad_features) fstage = nullptr;
    if (grad && !grad_tau) grad_tau = tau_ws;
    if (!grad && !grad_q && !grad_tau) s_rows = nullptr;
    if (!stage && !fstage && !s_rows) return hipSuccess;
    hipError_t e = hipMemsetAsync(next, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (stage && (e = hipMemsetAsync(stage, 0, N * 10 * sizeof(double), s)) != hipSuccess) return e;
    if (fstage && (e = hipMemsetAsync(fstage, 0, N * C * sizeof(double), s)) != hipSuccess) return e;
    const int vec4 = C % 4u == 0 && ((uintptr_t)feat & 15u) == 0 && ((uintptr_t)weights & 15u) == 0;
    if (stage || fstage)
        hipLaunchKernelGGL(dev::query_radiance_grad_kernel<true>, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, q,
                           q_stride, n, K, feat, C, vec4, weights, weight_opacity, tr, s_rows, stage, fstage, grad_q, grad_tau, next,
                           refill);
    else
        hipLaunchKernelGGL(dev::query_radiance_grad_kernel<false>, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, q,
                           q_stride, n, K, feat, C, vec4, weights, weight_opacity, tr, s_rows, stage, fstage, grad_q, grad_tau, next,
                           refill);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (stage) {
        // d tau / d theta for the weights grad_tau as rounded to f32, into the same staging rows; then one conversion
        if ((e = query_transmittance_profile_grad_add(A, rays, t, t_stride, grad_tau, n, K, moving, stage, next + 1, refill, cus,
                                                      s)) != hipSuccess)
            return e;
        if ((e = query_grad_finish(A, stage, 10, grad, s)) != hipSuccess) return e;
    }
    if (fstage) return query_features_finish(A, fstage, C, grad_features, s);
    return hipSuccess;
}

}  // namespace vr
