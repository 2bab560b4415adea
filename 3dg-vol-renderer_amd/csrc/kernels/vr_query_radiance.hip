// The radiance query (include/vr_hip.h, vr_query_radiance): the emission-absorption sum along each ray,
//   out[i][c] = sum_k q_ik T_ik sum_{g active at x_ik} m_g(x_ik) f_gc,   x_ik = o_i + t_ik d_i,
// for the caller's samples t, quadrature weights q and per-Gaussian rows f, with T the transmittance profile's Tr. The
// profile launcher (vr_query_profile.hip) has written Tr before this unit's kernel starts; the kernel is one more
// operation on the persistent ray-queue walk (ray_queue_walk, vr_walk.h) through QueryOp / query_walk
// (vr_query_common.h), in a unit of its own so that no other kernel is compiled differently for it.
//
// Because sum_k q T sum_g m f = sum_g f (sum_k q T m), a (ray, Gaussian) pair costs one mu_t per active sample and one
// multiply-add per channel. A work item is (ray, chunk of kFeatChunk channels): its sums are kFeatChunk doubles, the
// opacity sum and the pair count in registers (every loop over them is unrolled), its walk is the ray's slab walk pruned
// at the row's largest valid sample, and per record it loops over the row's K samples, read from global memory as
// ProfileGradOp::add reads them. The leaves a ray reaches hold every leaf whose box holds one of its sample points (the
// boxes are the 3-sigma boxes grown by 5 %, the point fl(o + t d) lies within an ulp of the ray), and a record is in one
// leaf, so every active (sample, Gaussian) pair is met exactly once.
//
// Floating point: the point per component __fadd_rn(o, __fmul_rn(t, d)) (what numpy and torch compute from f32 arrays),
// the decision sigma_active and m = mu_t in f32 exactly as vr_query_sigma / vr_query_features have them, every product
// and sum after that in double, one rounding to f32 per output. A channel of ones adds W * 1.0 = W where the opacity
// adds W, in the same order: the same bits. A channel's sums do not depend on its chunk or on C.
#include "../host/vr_kernels.h"
#include "vr_query_common.h"

namespace vr {
namespace dev {

constexpr int kFeatChunk = 8;  // vr_query_features.hip's: double sums a lane holds at once, a chunk is two float4 of a row

// The only prefilter: an interval [lo, hi] of t outside which no sample point of the ray can pass sigma_active for
// this Gaussian. False: no sample can (the Gaussian is skipped). It is conservative by the following bound, and where
// the bound's premises fail the interval is the whole row [0, tmax].
//
// In exact arithmetic on the f32 inputs let l(t) = o + t d - mean and Q(t) = l.M l = A t^2 + B t + C. The interval is
// the chord of Q <= 13.5 (not 9), padded by 2^-22 (|lo| + |hi|) >= 2^-22 |B| / A for the roots' own rounding (double,
// then f32). For a sample outside it Q(t) > 13.5, and the kernel's f32 decision differs from Q in two ways:
//   the point: x = fl(o + fl(t d)) is off the line by at most dl = 2^-23 (tmax |d|_inf + |o|_inf) per component
//     (two roundings, u = 2^-24 each, of magnitudes at most |t d| and |t d| + |o|); in the M-norm that is at most
//     s = sqrt(3 tr M) dl, so with p = x - mean: sqrt(p.M p) >= sqrt(13.5) - s;
//   the evaluation: sigma_active rounds p once per component and each term M_ij p_i p_j six more times at most, so its
//     value is p.M p + e with |e| <= 2^-20 m1 |p|^2 <= rho p.M p, m1 = sum_ij |M_ij| >= lambda_max,
//     rho = 2^-20 m1 / lambda_lb, and lambda_lb = 4 det M / (tr M)^2 <= lambda_min (lambda_max lambda_mid <= (tr / 2)^2).
// The premises are s <= 0.1 and rho <= 0.1 (and A > 0, everything finite); then the f32 value is above
// (sqrt(13.5) - 0.1)^2 * 0.9 = 11.4 > 9, and fl(v - 9) <= 0 only if v <= 9: the sample is inactive. rho <= 0.1 also
// bounds the condition number, so the double det and chord carry relative errors far below the slack used here. An
// elongated Gaussian that fails a premise is tested on every valid sample.
__device__ __forceinline__ bool radiance_interval(const GRec& g, const Ray& r, float tmax, float& lo, float& hi) {
    lo = 0.0f;
    hi = tmax;
    const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
    const double tr = m00 + m11 + m22;
    const double m1 = fabs(m00) + fabs(m11) + fabs(m22) + 2.0 * (fabs(m01) + fabs(m02) + fabs(m12));
    const double det = m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02) + m02 * (m01 * m12 - m11 * m02);
    const double dinf = fmax(fabs((double)r.dx), fmax(fabs((double)r.dy), fabs((double)r.dz)));
    const double oinf = fmax(fabs((double)r.ox), fmax(fabs((double)r.oy), fabs((double)r.oz)));
    const double dl = 0x1p-23 * ((double)tmax * dinf + oinf);
    // rho <= 0.1 and s <= 0.1, written so that a NaN fails
    if (!(tr > 0.0 && det > 0.0 && 0x1p-20 * m1 * tr * tr <= 0.4 * det && 3.0 * tr * dl * dl <= 0.01)) return true;
    const double dx = r.dx, dy = r.dy, dz = r.dz;
    const double px = (double)r.ox - (double)g.mx, py = (double)r.oy - (double)g.my, pz = (double)r.oz - (double)g.mz;
    const double mdx = m00 * dx + m01 * dy + m02 * dz, mdy = m01 * dx + m11 * dy + m12 * dz, mdz = m02 * dx + m12 * dy + m22 * dz;
    const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz, mpz = m02 * px + m12 * py + m22 * pz;
    const double A = dx * mdx + dy * mdy + dz * mdz;
    const double B = 2.0 * (px * mdx + py * mdy + pz * mdz);
    const double C = px * mpx + py * mpy + pz * mpz - 13.5;
    const double disc = B * B - 4.0 * A * C;
    if (!(A > 0.0) || !(fabs(disc) < INFINITY)) return true;
    if (disc < 0.0) return false;  // the line stays outside Q <= 13.5
    const double sq = sqrt(disc), t0 = (-B - sq) / (2.0 * A), t1 = (-B + sq) / (2.0 * A);
    const double pad = 0x1p-22 * (fabs(t0) + fabs(t1));
    if (!(pad < INFINITY)) return true;
    if (t1 + pad < 0.0 || t0 - pad > (double)tmax) return false;
    lo = fmaxf(lo, (float)(t0 - 2.0 * pad));  // (the conversion's rounding is within the second pad)
    hi = fminf(hi, (float)(t1 + 2.0 * pad));
    return true;
}

struct RadianceOp : QueryOp<RadianceOp, true> {
    using Base = QueryOp<RadianceOp, true>;
    const float* __restrict__ t;
    const float* __restrict__ q;     // nullptr: ones
    const float* __restrict__ tr;    // the profile's Tr, n * K
    const float* __restrict__ feat;  // the caller's rows
    float* out;
    float* opacity;
    uint32_t* n_pairs;
    uint32_t t_stride, q_stride, K, C, chunks;
    bool vec4;
    const float* row;   // the ray's K samples,
    const float* qrow;  // their weights (nullptr: ones)
    const float* trow;  // and their Tr
    uint32_t c0, nc;    // the item's first channel and how many it has
    double f[kFeatChunk], op;
    uint32_t cnt;
    // item id = ray * chunks + chunk
    __device__ __forceinline__ int load(const RenderArgs& A, uint32_t id, Ray& r, float& tmax) {
        const uint32_t ray = id / chunks;
        c0 = (id - ray * chunks) * (uint32_t)kFeatChunk;
        nc = min(C - c0, (uint32_t)kFeatChunk);
        const int what = Base::load(A, ray, r, tmax);  // (the row's own tmax is not used)
        row = t + (size_t)t_stride * ray;
        qrow = q ? q + (size_t)q_stride * ray : nullptr;
        trow = tr + (size_t)K * ray;
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
        op = 0.0;
        cnt = 0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k) f[k] = 0.0;
    }
    __device__ __forceinline__ bool prim(const RenderArgs& A, const Ray& r, float tmax, uint32_t j) {
        const GRec g = load_rec(A.gauss, (int)j);
        float lo, hi;
        if (!radiance_interval(g, r, tmax, lo, hi)) return true;
        double W = 0.0;
        uint32_t pairs = 0;
        for (uint32_t k = 0; k < K; ++k) {
            const float tk = row[k];
            if (!(tk >= lo && tk <= hi)) continue;  // outside the interval, or not valid (lo >= 0, hi <= tmax < inf)
            const float x = __fadd_rn(r.ox, __fmul_rn(tk, r.dx));
            const float y = __fadd_rn(r.oy, __fmul_rn(tk, r.dy));
            const float z = __fadd_rn(r.oz, __fmul_rn(tk, r.dz));
            if (!sigma_active(g, x, y, z)) continue;
            const double qk = qrow ? (double)qrow[k] : 1.0;
            W += qk * (double)trow[k] * (double)mu_t(g, x, y, z);
            ++pairs;
        }
        if (pairs == 0) return true;
        cnt += pairs;
        op += W;
        const float* frow = feat + (size_t)A.gauss_order[j] * C + c0;
        float v[kFeatChunk];
        if (vec4) {
            const float4 a = reinterpret_cast<const float4*>(frow)[0];
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (nc > 4) b = reinterpret_cast<const float4*>(frow)[1];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < kFeatChunk; ++k) v[k] = (uint32_t)k < nc ? frow[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k) f[k] += W * (double)v[k];
        return true;
    }
    __device__ __forceinline__ void finish(const RenderArgs&, uint32_t id, float) {
        const uint32_t ray = id / chunks;
        float* o = out + (size_t)ray * C + c0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k)
            if ((uint32_t)k < nc) o[k] = (float)f[k];
        if (c0 == 0) {
            if (opacity) opacity[ray] = (float)op;
            if (n_pairs) n_pairs[ray] = cnt;
        }
    }
    __device__ __forceinline__ void invalid(uint32_t id) {
        const uint32_t ray = id / chunks;
        float* o = out + (size_t)ray * C + c0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k)
            if ((uint32_t)k < nc) o[k] = __builtin_nanf("");
        if (c0 == 0) {
            if (opacity) opacity[ray] = __builtin_nanf("");
            if (n_pairs) n_pairs[ray] = 0u;
        }
    }
};
static_assert(kFeatChunk == 8, "RadianceOp::prim reads a chunk as two float4");

__global__ void __launch_bounds__(kQBlock) query_radiance_kernel(RenderArgs A, const vr_ray* __restrict__ rays,
                                                                 const float* __restrict__ t, uint32_t t_stride,
                                                                 const float* __restrict__ q, uint32_t q_stride, uint32_t items,
                                                                 uint32_t K, const float* __restrict__ feat, uint32_t C,
                                                                 uint32_t chunks, int vec4, const float* __restrict__ tr,
                                                                 float* __restrict__ out, float* __restrict__ opacity,
                                                                 uint32_t* __restrict__ n_pairs, uint32_t* __restrict__ next,
                                                                 int refill) {
    RadianceOp op;
    op.rays = rays;
    op.t = t;
    op.q = q;
    op.tr = tr;
    op.feat = feat;
    op.out = out;
    op.opacity = opacity;
    op.n_pairs = n_pairs;
    op.t_stride = t_stride;
    op.q_stride = q_stride;
    op.K = K;
    op.C = C;
    op.chunks = chunks;
    op.vec4 = vec4 != 0;
    op.row = op.qrow = op.trow = nullptr;
    op.c0 = op.nc = 0;
    op.reset();
    query_walk(A, items, next, refill, op);
}

}  // namespace dev

// ---- launcher (host/vr_query_host.cpp) ----
// tr: n * K floats, written by query_transmittance_profile earlier on the same stream; out: n * C floats; opacity,
// n_pairs: n each or nullptr; every entry written. n > 0, n * ceil(C / 8) <= n * C < 2^31.
hipError_t query_radiance(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, const float* q,
                          uint32_t q_stride, uint32_t n, uint32_t K, const float* feat, uint32_t C, const float* tr, float* out,
                          float* opacity, uint32_t* n_pairs, uint32_t* next, int refill, int cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(next, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t chunks = (C + (uint32_t)dev::kFeatChunk - 1u) / (uint32_t)dev::kFeatChunk;
    const int vec4 = C % 4u == 0 && ((uintptr_t)feat & 15u) == 0;
    hipLaunchKernelGGL(dev::query_radiance_kernel, query_grid(cus), dim3(dev::kQBlock), 0, s, A, rays, t, t_stride, q, q_stride,
                       n * chunks, K, feat, C, chunks, vec4, tr, out, opacity, n_pairs, next, refill);
    return hipGetLastError();
}

}  // namespace vr
