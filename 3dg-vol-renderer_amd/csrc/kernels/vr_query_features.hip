// The feature query (include/vr_hip.h, vr_query_features / vr_query_features_grad): F_c(x) = sum_g m_g(x) f_gc over the
// Gaussians active at x, for the caller's own per-Gaussian rows f (N x C floats in scene order, passed per call), the
// mass sum_g m_g(x) itself, and the gradient of a weighted sum of both with respect to the Gaussians, the rows and the
// points. The sigma query (vr_query.hip) is the one-channel case with the albedo for f; everything that decides is
// shared with it (vr_query_common.h): sigma_active's f32 decision and the two containment walks, so the active set is
// the forward sigma's bit for bit.
//   query_features_kernel        one point per lane; per chunk of kFeatChunk channels one walk with as many double sums
//   query_features_grad_kernel   one walk per point; per active (point, Gaussian) one pass over the C channels (c, the
//                                adds to the feature staging), then ten adds to the Gaussian's staging row
//   query_features_finish_kernel feature staging (tree order, double) -> grad_features (scene order, f32)
// Floating point as in vr_query.hip: f32 decisions and f32 m (mu_t) in the forward, sums in double in walk order; in the
// gradient everything on a decided (point, Gaussian) is double from the f32 record, point, row and weights.
#include "../host/vr_kernels.h"  // query_grad_finish (vr_query.hip)
#include "vr_query_common.h"

namespace vr {
namespace dev {

constexpr int kFeatChunk = 8;  // double sums a lane holds at once (16 VGPRs); gridDim.y = ceil(C / kFeatChunk)

// The forward's leaf accumulator: SigmaAcc with `nc` caller channels in place of the albedo. sum and cnt are
// SigmaAcc's; f[k] += (double)(m * row[k]) is its sum_alb, one f32 multiply per channel. A channel is summed in walk
// order whatever chunk it stands in, so its bits depend neither on C nor on its place among the C.
// vec4: C is a multiple of 4 and the rows are 16-byte aligned, so the chunk (it starts at a multiple of 8 channels and
// holds 4 or 8) is read as one or two float4; otherwise nc guarded scalar loads.
struct FeatAcc {
    const float* __restrict__ feat;  // the caller's rows, advanced to the chunk's first channel
    uint32_t C, nc;
    bool vec4;
    double sum, f[kFeatChunk];
    uint32_t cnt;
    __device__ __forceinline__ void reset() {
        sum = 0.0;
        cnt = 0;
#pragma unroll
        for (int k = 0; k < kFeatChunk; ++k) f[k] = 0.0;
    }
    __device__ __forceinline__ void leaf(const RenderArgs& A, int32_t ref, float x, float y, float z) {
        const uint32_t first = leaf_first(ref), end = first + leaf_count(ref);
        for (uint32_t j = first; j < end; ++j) {
            const GRec g = load_rec(A.gauss, (int)j);
            if (!sigma_active(g, x, y, z)) continue;
            const float m = mu_t(g, x, y, z);
            sum += (double)m;
            ++cnt;
            const float* row = feat + (size_t)A.gauss_order[j] * C;
            float v[kFeatChunk];
            if (vec4) {
                const float4 a = reinterpret_cast<const float4*>(row)[0];
                float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (nc > 4) b = reinterpret_cast<const float4*>(row)[1];
                v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < kFeatChunk; ++k) v[k] = (uint32_t)k < nc ? row[k] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kFeatChunk; ++k) f[k] += (double)(m * v[k]);
        }
    }
};
static_assert(kFeatChunk == 8, "FeatAcc::leaf reads a chunk as two float4");

// query_sigma_kernel's walks with FeatAcc, once per chunk of channels (blockIdx.y). A point is live as the forward
// sigma's is: the f32 rounding of the summed m is not <= 0. A dead point gets +0 everywhere, a point whose child-pair
// walk broke off NaN and no active Gaussian. Chunk 0 alone writes mass and n_active.
__global__ void __launch_bounds__(kQBlock) query_features_kernel(RenderArgs A, const float* __restrict__ xyz, uint32_t n,
                                                                 const float* __restrict__ feat, uint32_t C, int vec4,
                                                                 float* __restrict__ out, float* __restrict__ mass,
                                                                 uint32_t* __restrict__ n_active) {
    __shared__ int s_stack[kStackSize * kQBlock];
    int* stack = s_stack + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c0 = blockIdx.y * (uint32_t)kFeatChunk;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    FeatAcc acc;
    acc.feat = feat + c0;
    acc.C = C;
    acc.nc = min(C - c0, (uint32_t)kFeatChunk);
    acc.vec4 = vec4 != 0;
    acc.reset();
    bool redo = A.hnodes4 == nullptr, bad = false;
    if (A.num_prims > 0 && !redo) redo = sigma_walk_wide(A, x, y, z, stack, acc);
    if (A.num_prims > 0 && redo) {
        acc.reset();
        bad = sigma_walk_pair(A, x, y, z, stack, acc);
    }
    const float sum = (float)acc.sum;
    const bool live = !bad && !(sum <= 0.0f);
    const float nan = __builtin_nanf("");
    float* row = out + (size_t)i * C + c0;
#pragma unroll
    for (int k = 0; k < kFeatChunk; ++k)
        if ((uint32_t)k < acc.nc) row[k] = bad ? nan : live ? (float)acc.f[k] : 0.0f;
    if (c0 == 0) {
        if (mass) mass[i] = bad ? nan : live ? sum : 0.0f;
        if (n_active) n_active[i] = bad ? 0u : acc.cnt;
    }
}

// The gradient's leaf accumulator (include/vr_hip.h, vr_query_features_grad, has the formulas): on every active Gaussian
// the record and the point are read as doubles, p = x - mean, q = p.Mp, e = norm exp(-q / 2), m = rho e; one pass over
// the channels forms c = u + sum_k w_k f_k from the lane's own weight row and the Gaussian's row and, with a feature
// staging, adds sg w_k m to facc[C j + k]; then
//   GAUSS:  with a Gaussian staging, ten adds into acc[10 j .. 10 j + 9] of record j (tree order), per unit density so
//           that query_grad_finish_kernel<10> converts the row: c e M p, -c e p p^T / 2 {00, 01, 02, 11, 12, 22}, c e,
//           each times sg. The two staging pointers are tested at run time (the same for every lane); sg = -1 takes a
//           walk's adds back, see features_grad_point.
//   POINTS: g_x = -c m M p summed in registers.
// The points-only instantiation carries no staging pointer and has no atomics.
template <bool GAUSS>
struct FeatGradStage {};
template <>
struct FeatGradStage<true> {
    double* acc;
    double* facc;
    double sg;
};
template <bool POINTS>
struct FeatGradSum {};
template <>
struct FeatGradSum<true> {
    double gx, gy, gz;
};
template <bool GAUSS, bool POINTS>
struct FeatGradAcc : FeatGradStage<GAUSS>, FeatGradSum<POINTS> {
    const float* __restrict__ feat;
    const float* __restrict__ wrow;  // the point's C weights, or nullptr: every one is 1
    uint32_t C;
    double u, mass;
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
            this->mass += m;
            ++this->cnt;
            const float* frow = feat + (size_t)A.gauss_order[j] * C;
            double c = this->u;
            if constexpr (GAUSS) {
                double* fst = this->facc ? this->facc + (size_t)j * C : nullptr;
                const double sm = this->sg * m;
                for (uint32_t k = 0; k < C; ++k) {
                    const double wk = wrow ? (double)wrow[k] : 1.0;
                    c += wk * (double)frow[k];
                    if (fst) atomicAdd(fst + k, wk * sm);
                }
            } else {
                for (uint32_t k = 0; k < C; ++k) c += (wrow ? (double)wrow[k] : 1.0) * (double)frow[k];
            }
            if constexpr (POINTS) {
                const double cm = c * m;
                this->gx -= cm * mpx;
                this->gy -= cm * mpy;
                this->gz -= cm * mpz;
            }
            if constexpr (GAUSS) {
                if (this->acc) {
                    const double s = this->sg * (c * e), h = -0.5 * s;
                    double* row = this->acc + 10 * (size_t)j;
                    atomicAdd(row + 0, s * mpx);
                    atomicAdd(row + 1, s * mpy);
                    atomicAdd(row + 2, s * mpz);
                    atomicAdd(row + 3, h * px * px);
                    atomicAdd(row + 4, h * px * py);
                    atomicAdd(row + 5, h * px * pz);
                    atomicAdd(row + 6, h * py * py);
                    atomicAdd(row + 7, h * py * pz);
                    atomicAdd(row + 8, h * pz * pz);
                    atomicAdd(row + 9, s);
                }
            }
        }
    }
};

// One point of the gradient: the control flow of sigma_grad_point (vr_query.hip) with this query's accumulator. The adds
// to the staging rows happen while a walk runs, so a walk whose adds must not stand is walked again with sg = -1: a
// 4-wide walk that broke off for its stack (the child-pair walk then adds the whole active set), a child-pair walk deeper
// than the builder allows (the forward's NaN case) and a point whose summed m is <= 0 (the forward's zeros). The
// points-only form has nothing to take back.
template <bool GAUSS, bool POINTS>
__device__ __forceinline__ void features_grad_point(const RenderArgs& A, const float* __restrict__ xyz,
                                                    const float* __restrict__ weights, const float* __restrict__ weight_mass,
                                                    uint32_t n, FeatGradAcc<GAUSS, POINTS>& acc, float* __restrict__ grad_xyz) {
    __shared__ int s_stack[kStackSize * kQBlock];
    int* stack = s_stack + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    acc.wrow = weights ? weights + (size_t)i * acc.C : nullptr;
    acc.u = weight_mass ? (double)weight_mass[i] : 0.0;
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
__global__ void __launch_bounds__(kQBlock) query_features_grad_kernel(RenderArgs A, const float* __restrict__ xyz, uint32_t n,
                                                                      const float* __restrict__ feat, uint32_t C,
                                                                      const float* __restrict__ weights,
                                                                      const float* __restrict__ weight_mass,
                                                                      double* __restrict__ stage, double* __restrict__ fstage,
                                                                      float* __restrict__ grad_xyz) {
    FeatGradAcc<true, POINTS> acc;
    acc.feat = feat;
    acc.C = C;
    acc.acc = stage;
    acc.facc = fstage;
    features_grad_point<true, POINTS>(A, xyz, weights, weight_mass, n, acc, grad_xyz);
}

// The gradient at the points alone: no staging, no atomics.
__global__ void __launch_bounds__(kQBlock) query_features_grad_points_kernel(RenderArgs A, const float* __restrict__ xyz,
                                                                             uint32_t n, const float* __restrict__ feat,
                                                                             uint32_t C, const float* __restrict__ weights,
                                                                             const float* __restrict__ weight_mass,
                                                                             float* __restrict__ grad_xyz) {
    FeatGradAcc<false, true> acc;
    acc.feat = feat;
    acc.C = C;
    features_grad_point<false, true>(A, xyz, weights, weight_mass, n, acc, grad_xyz);
}

// Feature staging word (j, k) (tree order) -> grad_features[C gauss_order[j] + k], rounded to f32 once (+ 0.0: a row
// whose adds were all taken back to -0 gets +0).
__global__ void __launch_bounds__(256) query_features_finish_kernel(const uint32_t* __restrict__ order,
                                                                    const double* __restrict__ fstage, uint32_t words, uint32_t C,
                                                                    float* __restrict__ grad_features) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= words) return;
    const uint32_t j = w / C, k = w - j * C;
    grad_features[(size_t)order[j] * C + k] = (float)(fstage[w] + 0.0);
}

}  // namespace dev

// ---- launchers (host/vr_query_host.cpp) ----
// out: n * C floats; mass, n_active: n each or nullptr; every entry written. n > 0, 1 <= C.
hipError_t query_features(const RenderArgs& A, const float* xyz, uint32_t n, const float* feat, uint32_t C, float* out, float* mass,
                          uint32_t* n_active, hipStream_t s) {
    const dim3 grid((n + dev::kQBlock - 1) / dev::kQBlock, (C + dev::kFeatChunk - 1) / dev::kFeatChunk);
    const int vec4 = C % 4u == 0 && ((uintptr_t)feat & 15u) == 0;
    hipLaunchKernelGGL(dev::query_features_kernel, grid, dim3(dev::kQBlock), 0, s, A, xyz, n, feat, C, vec4, out, mass, n_active);
    return hipGetLastError();
}

// The finish of a feature staging (C doubles per Gaussian, tree order) -> grad_features; the radiance gradient's unit calls
// it too. A.num_prims > 0.
hipError_t query_features_finish(const RenderArgs& A, const double* fstage, uint32_t C, float* grad_features, hipStream_t s) {
    const uint32_t words = (uint32_t)((size_t)A.num_prims * C);
    hipLaunchKernelGGL(dev::query_features_finish_kernel, dim3((words + 255u) / 256u), dim3(256), 0, s, A.gauss_order, fstage, words,
                       C, grad_features);
    return hipGetLastError();
}

// stage: 10 doubles per Gaussian, fstage: C doubles per Gaussian, both zeroed here, each needed only with its output;
// grad: 10 floats per Gaussian, grad_features: C floats per Gaussian, grad_xyz: 3 floats per point, every entry of a
// given output written. Any output may be nullptr; a scene without Gaussians has no rows to write.
hipError_t query_features_grad(const RenderArgs& A, const float* xyz, uint32_t n, const float* feat, uint32_t C,
                               const float* weights, const float* weight_mass, double* stage, double* fstage, float* grad,
                               float* grad_features, float* grad_xyz, hipStream_t s) {
    const dim3 grid((n + dev::kQBlock - 1) / dev::kQBlock), block(dev::kQBlock);
    hipError_t e;
    if ((!grad && !grad_features) || A.num_prims <= 0) {
        if (grad_xyz && n > 0)
            hipLaunchKernelGGL(dev::query_features_grad_points_kernel, grid, block, 0, s, A, xyz, n, feat, C, weights, weight_mass,
                               grad_xyz);
        return hipGetLastError();
    }
    const size_t N = (size_t)A.num_prims;
    if (!grad) stage = nullptr;
    if (!grad_features) fstage = nullptr;
    if (stage && (e = hipMemsetAsync(stage, 0, N * 10 * sizeof(double), s)) != hipSuccess) return e;
    if (fstage && (e = hipMemsetAsync(fstage, 0, N * C * sizeof(double), s)) != hipSuccess) return e;
    if (n > 0) {
        if (grad_xyz)
            hipLaunchKernelGGL(dev::query_features_grad_kernel<true>, grid, block, 0, s, A, xyz, n, feat, C, weights, weight_mass,
                               stage, fstage, grad_xyz);
        else
            hipLaunchKernelGGL(dev::query_features_grad_kernel<false>, grid, block, 0, s, A, xyz, n, feat, C, weights, weight_mass,
                               stage, fstage, grad_xyz);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (stage && (e = query_grad_finish(A, stage, 10, grad, s)) != hipSuccess) return e;
    if (fstage && (e = query_features_finish(A, fstage, C, grad_features, s)) != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace vr
