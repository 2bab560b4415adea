// Mixture queries (vr_query_*, kernels/vr_query.hip, kernels/vr_query_profile.hip, kernels/vr_query_flight.hip): batched
// transmittance and its gradients with respect to the Gaussians and to the rays, transmittance profiles and their
// gradient, ray events, sigma and its gradient, and free-flight distances.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "vr_ctx.h"

using namespace vr;

namespace {

// The scene part of the kernel arguments, after the checks every query shares. `n` entries of a batch.
vr_status query_begin(vr_ctx* c, const char* what, size_t n, RenderArgs& A) {
    if (!c) return fail(VR_ERR_INVALID, std::string(what) + ": NULL ctx");
    if (!c->has_scene) return fail(VR_ERR_NOSCENE, "no scene uploaded (call vr_upload_scene first)");
    if (c->type != VR_VOLUME_GAUSSIANS) return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": mixture queries need a Gaussian scene");
    if (n >= (1ull << 31)) return fail(VR_ERR_INVALID, std::string(what) + ": more than 2^31 - 1 entries in one call");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    std::memset(&A, 0, sizeof(A));
    const SceneDev& sd = c->scene;
    A.gauss = sd.gauss.get();
    A.nodes = sd.nodes.get();
    A.hnodes = sd.hnodes.get();
    // the 4-wide walks read the per-axis copy, which exists whenever the 4-wide tree does (upload_parents)
    A.hnodes4 = sd.hnodes4w ? sd.hnodes4.get() : nullptr;
    A.hnodes4w = sd.hnodes4w.get();
    A.num_nodes4 = (uint32_t)sd.num_nodes4;
    for (int k = 0; k < 3; ++k) A.hn_center[k] = sd.hn_center[k];
    A.hn_scale = sd.hn_scale;
    A.num_prims = c->num_prims;
    A.bvh_depth = sd.bvh_depth;
    A.gauss_order = sd.order.get();
    return c->q_ctl.grow(48, "hipMalloc(query counters)");
}
int query_refill(const vr_ctx* c) { return std::clamp<int>(c->auto_nee_refill, 1, 64); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

vr_status vr_query_transmittance_device(vr_ctx* c, const vr_ray* d_rays, size_t n, float* d_tr, float* d_tau, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_tr) return fail(VR_ERR_INVALID, "vr_query_transmittance: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance: the device ray array must be 16-byte aligned");
    HIP_TRY(query_transmittance(A, d_rays, (uint32_t)n, d_tr, d_tau, (uint32_t*)c->q_ctl.get(), query_refill(c), c->cus,
                                (hipStream_t)stream),
            "query_transmittance_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance(vr_ctx* c, const vr_ray* rays, size_t n, float* tr, float* tau) {
    c = first_device(c);
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_transmittance", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!rays || !tr) return fail(VR_ERR_INVALID, "vr_query_transmittance: NULL argument");
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_out.grow(n, "hipMalloc(query results)"));
    if (tau) VR_TRY(c->q_out2.grow(n * sizeof(float), "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    VR_TRY(vr_query_transmittance_device(c, (const vr_ray*)c->q_in.get(), n, c->q_out.get(), tau ? (float*)c->q_out2.get() : nullptr,
                                       c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_transmittance_kernel");
    HIP_TRY(hipMemcpy(tr, c->q_out.get(), n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (tau) HIP_TRY(hipMemcpy(tau, c->q_out2.get(), n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

vr_status vr_query_transmittance_grad_device(vr_ctx* c, const vr_ray* d_rays, const float* d_weight, size_t n, uint32_t flags,
                                             float* d_grad, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_grad", n, A));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: unknown flag bits");
    if (!d_grad || (n > 0 && !d_rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: the device ray array must be 16-byte aligned");
    // the staging rows are the query's own: a frame queued on another stream never sees them
    VR_TRY(c->q_grad.grow((size_t)std::max(A.num_prims, 1) * 10, "hipMalloc(gradient staging)"));
    HIP_TRY(query_transmittance_grad(A, d_rays, d_weight, (uint32_t)n, !(flags & VR_GRAD_FROZEN_BOUNDS), c->q_grad.get(), d_grad,
                                     (uint32_t*)c->q_ctl.get() + 3, query_refill(c), c->cus, (hipStream_t)stream),
            "query_grad_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_grad(vr_ctx* c, const vr_ray* rays, const float* weight, size_t n, uint32_t flags, float* grad) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_grad", n, A));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: unknown flag bits");
    if (!grad || (n > 0 && !rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: NULL argument");
    const size_t words = (size_t)std::max(A.num_prims, 0) * 10;
    if (n == 0 || words == 0) {
        std::memset(grad, 0, words * sizeof(float));
        return VR_OK;
    }
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    if (weight) VR_TRY(c->q_tau.grow(n, "hipMalloc(query weights)"));
    VR_TRY(c->q_out.grow(words, "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    if (weight) HIP_TRY(hipMemcpy(c->q_tau.get(), weight, n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(query weights)");
    VR_TRY(vr_query_transmittance_grad_device(c, (const vr_ray*)c->q_in.get(), weight ? c->q_tau.get() : nullptr, n, flags,
                                              c->q_out.get(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_grad_kernel");
    HIP_TRY(hipMemcpy(grad, c->q_out.get(), words * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

vr_status vr_query_transmittance_ray_grad_device(vr_ctx* c, const vr_ray* d_rays, size_t n, uint32_t flags, vr_ray_grad* d_out,
                                                 void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_ray_grad", n, A));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: unknown flag bits");
    if (n == 0) return VR_OK;
    if (!d_rays || !d_out) return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: NULL argument");
    if (!aligned16(d_rays) || !aligned16(d_out))
        return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: the device arrays must be 16-byte aligned");
    HIP_TRY(query_transmittance_ray_grad(A, d_rays, (uint32_t)n, !(flags & VR_GRAD_FROZEN_BOUNDS), d_out,
                                         (uint32_t*)c->q_ctl.get() + 6, query_refill(c), c->cus, (hipStream_t)stream),
            "query_ray_grad_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_ray_grad(vr_ctx* c, const vr_ray* rays, size_t n, uint32_t flags, vr_ray_grad* out) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_ray_grad", n, A));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: unknown flag bits");
    if (n == 0) return VR_OK;
    if (!rays || !out) return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: NULL argument");
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_out.grow(n * (sizeof(vr_ray_grad) / sizeof(float)), "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    VR_TRY(vr_query_transmittance_ray_grad_device(c, (const vr_ray*)c->q_in.get(), n, flags, (vr_ray_grad*)c->q_out.get(),
                                                  c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_ray_grad_kernel");
    HIP_TRY(hipMemcpy(out, c->q_out.get(), n * sizeof(vr_ray_grad), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

// ---- transmittance profile: K samples per ray from one walk ----
namespace {

// The checks of the four profile entry points that precede every launch. `what` names the entry point.
vr_status profile_check(const char* what, size_t t_stride, size_t n, uint32_t K) {
    if (K == 0 || K > VR_PROFILE_MAX_SAMPLES)
        return fail(VR_ERR_INVALID, std::string(what) + ": K must lie in [1, " + std::to_string(VR_PROFILE_MAX_SAMPLES) + "]");
    if (t_stride != 0 && t_stride != K) return fail(VR_ERR_INVALID, std::string(what) + ": t_stride must be 0 (one shared row) or K");
    if (n >= (1ull << 31) || n * (size_t)K >= (1ull << 31))
        return fail(VR_ERR_INVALID, std::string(what) + ": more than 2^31 - 1 samples in one call");
    return VR_OK;
}

}  // namespace

vr_status vr_query_transmittance_profile_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride, size_t n,
                                                uint32_t K, float* d_tr, float* d_tau, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile", t_stride, n, K));
    if (!d_tr && !d_tau) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: both outputs are NULL");
    if (n == 0) return VR_OK;
    if (!d_rays || !d_t) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: the device ray array must be 16-byte aligned");
    HIP_TRY(query_transmittance_profile(A, d_rays, d_t, (uint32_t)t_stride, (uint32_t)n, K, d_tr, d_tau,
                                        (uint32_t*)c->q_ctl.get() + 8, query_refill(c), c->cus, (hipStream_t)stream),
            "query_profile_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_profile(vr_ctx* c, const vr_ray* rays, const float* t, size_t t_stride, size_t n, uint32_t K,
                                         float* tr, float* tau) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile", t_stride, n, K));
    if (!tr && !tau) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: both outputs are NULL");
    if (n == 0) return VR_OK;
    if (!rays || !t) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: NULL argument");
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K;
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_prof_t.grow(nt, "hipMalloc(profile samples)"));
    VR_TRY(c->q_prof_out.grow(2 * nk, "hipMalloc(profile results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    HIP_TRY(hipMemcpy(c->q_prof_t.get(), t, nt * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(profile samples)");
    float* d_tr = c->q_prof_out.get();
    float* d_tau = d_tr + nk;
    VR_TRY(vr_query_transmittance_profile_device(c, (const vr_ray*)c->q_in.get(), c->q_prof_t.get(), t_stride, n, K,
                                                 tr ? d_tr : nullptr, tau ? d_tau : nullptr, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_profile_kernel");
    if (tr) HIP_TRY(hipMemcpy(tr, d_tr, nk * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(profile results)");
    if (tau) HIP_TRY(hipMemcpy(tau, d_tau, nk * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(profile results)");
    return VR_OK;
}

vr_status vr_query_transmittance_profile_grad_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride,
                                                     const float* d_weight, size_t n, uint32_t K, uint32_t flags, float* d_grad,
                                                     void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile_grad", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile_grad", t_stride, n, K));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: unknown flag bits");
    if (!d_grad || (n > 0 && (!d_rays || !d_t))) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: NULL argument");
    if (!aligned16(d_rays))
        return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: the device ray array must be 16-byte aligned");
    // the staging rows are this query's own: a frame or another gradient query queued on another stream never sees them
    VR_TRY(c->q_prof_grad.grow((size_t)std::max(A.num_prims, 1) * 10, "hipMalloc(gradient staging)"));
    HIP_TRY(query_transmittance_profile_grad(A, d_rays, d_t, (uint32_t)t_stride, d_weight, (uint32_t)n, K,
                                             !(flags & VR_GRAD_FROZEN_BOUNDS), c->q_prof_grad.get(), d_grad,
                                             (uint32_t*)c->q_ctl.get() + 9, query_refill(c), c->cus, (hipStream_t)stream),
            "query_profile_grad_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_profile_grad(vr_ctx* c, const vr_ray* rays, const float* t, size_t t_stride, const float* weight,
                                              size_t n, uint32_t K, uint32_t flags, float* grad) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile_grad", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile_grad", t_stride, n, K));
    if (flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: unknown flag bits");
    if (!grad || (n > 0 && (!rays || !t))) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: NULL argument");
    const size_t words = (size_t)std::max(A.num_prims, 0) * 10;
    if (n == 0 || words == 0) {
        std::memset(grad, 0, words * sizeof(float));
        return VR_OK;
    }
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K;
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_prof_t.grow(nt, "hipMalloc(profile samples)"));
    if (weight) VR_TRY(c->q_prof_w.grow(nk, "hipMalloc(profile weights)"));
    VR_TRY(c->q_prof_out.grow(words, "hipMalloc(profile results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    HIP_TRY(hipMemcpy(c->q_prof_t.get(), t, nt * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(profile samples)");
    if (weight) HIP_TRY(hipMemcpy(c->q_prof_w.get(), weight, nk * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(profile weights)");
    VR_TRY(vr_query_transmittance_profile_grad_device(c, (const vr_ray*)c->q_in.get(), c->q_prof_t.get(), t_stride,
                                                      weight ? c->q_prof_w.get() : nullptr, n, K, flags, c->q_prof_out.get(),
                                                      c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_profile_grad_kernel");
    HIP_TRY(hipMemcpy(grad, c->q_prof_out.get(), words * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(profile results)");
    return VR_OK;
}

vr_status vr_query_sigma_device(vr_ctx* c, const float* d_xyz, size_t n, float* d_sigma_as, uint32_t* d_n_active, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_sigma", n, A));
    if (n == 0) return VR_OK;
    if (!d_xyz || !d_sigma_as) return fail(VR_ERR_INVALID, "vr_query_sigma: NULL argument");
    HIP_TRY(query_sigma(A, d_xyz, (uint32_t)n, d_sigma_as, d_n_active, (hipStream_t)stream), "query_sigma_kernel");
    return VR_OK;
}

vr_status vr_query_sigma(vr_ctx* c, const float* xyz, size_t n, float* sigma_as, uint32_t* n_active) {
    c = first_device(c);
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_sigma", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!xyz || !sigma_as) return fail(VR_ERR_INVALID, "vr_query_sigma: NULL argument");
    VR_TRY(c->q_in.grow(n * 3 * sizeof(float), "hipMalloc(query points)"));
    VR_TRY(c->q_out.grow(n * 2, "hipMalloc(query results)"));
    if (n_active) VR_TRY(c->q_out2.grow(n * sizeof(uint32_t), "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(query points)");
    VR_TRY(vr_query_sigma_device(c, (const float*)c->q_in.get(), n, c->q_out.get(), n_active ? (uint32_t*)c->q_out2.get() : nullptr,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_sigma_kernel");
    HIP_TRY(hipMemcpy(sigma_as, c->q_out.get(), n * 2 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (n_active) HIP_TRY(hipMemcpy(n_active, c->q_out2.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

vr_status vr_query_sigma_grad_device(vr_ctx* c, const float* d_xyz, const float* d_weight_as, size_t n, float* d_grad,
                                     float* d_grad_xyz, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_sigma_grad", n, A));
    const size_t words = (size_t)std::max(A.num_prims, 0) * 11;
    if (n == 0) {
        if (d_grad && words) HIP_TRY(hipMemsetAsync(d_grad, 0, words * sizeof(float), (hipStream_t)stream), "hipMemset(sigma gradient)");
        return VR_OK;
    }
    if (!d_xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: NULL argument");
    if (!d_grad && !d_grad_xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: both outputs are NULL");
    // the staging rows are the query's own: a frame or another gradient query queued on another stream never sees them
    if (d_grad) VR_TRY(c->q_sgrad.grow(std::max<size_t>(words, 11), "hipMalloc(gradient staging)"));
    HIP_TRY(query_sigma_grad(A, d_xyz, d_weight_as, (uint32_t)n, d_grad ? c->q_sgrad.get() : nullptr, d_grad, d_grad_xyz,
                             (hipStream_t)stream),
            "query_sigma_grad_kernel");
    return VR_OK;
}

vr_status vr_query_sigma_grad(vr_ctx* c, const float* xyz, const float* weight_as, size_t n, float* grad, float* grad_xyz) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_sigma_grad", n, A));
    const size_t words = (size_t)std::max(A.num_prims, 0) * 11;
    if (n == 0) {
        if (grad) std::memset(grad, 0, words * sizeof(float));
        return VR_OK;
    }
    if (!xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: NULL argument");
    if (!grad && !grad_xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: both outputs are NULL");
    const bool gauss = grad && words > 0;
    VR_TRY(c->q_in.grow(n * 3 * sizeof(float), "hipMalloc(query points)"));
    if (weight_as) VR_TRY(c->q_tau.grow(n * 2, "hipMalloc(query weights)"));
    if (gauss) VR_TRY(c->q_out.grow(words, "hipMalloc(query results)"));
    if (grad_xyz) VR_TRY(c->q_out2.grow(n * 3 * sizeof(float), "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(query points)");
    if (weight_as) HIP_TRY(hipMemcpy(c->q_tau.get(), weight_as, n * 2 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(query weights)");
    if (gauss || grad_xyz) {
        VR_TRY(vr_query_sigma_grad_device(c, (const float*)c->q_in.get(), weight_as ? c->q_tau.get() : nullptr, n,
                                          gauss ? c->q_out.get() : nullptr, grad_xyz ? (float*)c->q_out2.get() : nullptr, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream), "query_sigma_grad_kernel");
    }
    if (gauss) HIP_TRY(hipMemcpy(grad, c->q_out.get(), words * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (grad_xyz) HIP_TRY(hipMemcpy(grad_xyz, c->q_out2.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

vr_status vr_query_events_count_device(vr_ctx* c, const vr_ray* d_rays, size_t n, uint32_t* d_offsets, uint64_t* total) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_events", n, A));
    if (!total) return fail(VR_ERR_INVALID, "vr_query_events: NULL total");
    *total = 0;
    if (n == 0) return VR_OK;
    if (!d_rays || !d_offsets) return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_events: the device ray array must be 16-byte aligned");
    c->q_count_valid = false;
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");  // d_rays may come from any stream
    VR_TRY(c->q_cnt.grow(n + 1, "hipMalloc(event counts)"));
    uint32_t* ctl = (uint32_t*)c->q_ctl.get();
    unsigned long long* d_total = (unsigned long long*)(ctl + 4);
    size_t tmp_bytes = 0;
    auto count = [&](void* tmp) {  // tmp == nullptr: only the scratch size
        return query_events_count(A, d_rays, (uint32_t)n, c->q_cnt.get(), d_offsets, d_total, ctl + 1, query_refill(c), c->cus, tmp,
                                  tmp_bytes, c->stream);
    };
    HIP_TRY(count(nullptr), "event count scratch");
    VR_TRY(c->q_tmp.grow(tmp_bytes + 16, "hipMalloc(event scan scratch)"));
    HIP_TRY(count(c->q_tmp.get()), "query_events_count_kernel");
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof(tot), hipMemcpyDeviceToHost, c->stream), "hipMemcpy(event total)");
    HIP_TRY(hipStreamSynchronize(c->stream), "query_events_count_kernel");
    *total = tot;
    if (tot > 0xffffffffull) return fail(VR_ERR_INVALID, "vr_query_events: more than 2^32 - 1 events in one call (split the batch)");
    c->q_count_valid = true;
    c->q_count_n = n;
    c->q_count_total = tot;
    return VR_OK;
}

vr_status vr_query_events_fill_device(vr_ctx* c, const vr_ray* d_rays, size_t n, const uint32_t* d_offsets, float* d_t,
                                      uint32_t* d_ev, uint64_t cap, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_events", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_offsets) return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_events: the device ray array must be 16-byte aligned");
    if (!c->q_count_valid || c->q_count_n != n)
        return fail(VR_ERR_INVALID, "vr_query_events_fill_device: no vr_query_events_count_device call for this many rays preceded it");
    const uint64_t tot = c->q_count_total;
    if (cap < tot)
        return fail(VR_ERR_OVERFLOW, "vr_query_events: " + std::to_string(tot) + " events, room for " + std::to_string(cap));
    if (tot == 0) return VR_OK;
    if (!d_t || !d_ev) return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    VR_TRY(c->q_keys.grow(tot, "hipMalloc(event keys)"));
    VR_TRY(c->q_keys2.grow(tot, "hipMalloc(event keys)"));
    uint32_t* ctl = (uint32_t*)c->q_ctl.get();
    size_t tmp_bytes = 0;
    auto fill = [&](void* tmp) {  // tmp == nullptr: only the scratch size
        return query_events_fill(A, d_rays, (uint32_t)n, d_offsets, (uint32_t)tot, c->q_keys.get(), c->q_keys2.get(), d_t, d_ev,
                                 ctl + 2, query_refill(c), c->cus, tmp, tmp_bytes, (hipStream_t)stream);
    };
    HIP_TRY(fill(nullptr), "event sort scratch");
    VR_TRY(c->q_tmp.grow(tmp_bytes + 16, "hipMalloc(event sort scratch)"));
    HIP_TRY(fill(c->q_tmp.get()), "query_events_fill_kernel");
    return VR_OK;
}

vr_status vr_query_events(vr_ctx* c, const vr_ray* rays, size_t n, uint32_t* offsets, float* t, uint32_t* ev, uint64_t cap,
                          uint64_t* total) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_events", n, A));
    if (!total) return fail(VR_ERR_INVALID, "vr_query_events: NULL total");
    *total = 0;
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return VR_OK;
    }
    if (!rays || (cap > 0 && (!t || !ev)) || (cap == 0 && ((t == nullptr) != (ev == nullptr))))
        return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_off.grow(n + 1, "hipMalloc(event offsets)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    VR_TRY(vr_query_events_count_device(c, (const vr_ray*)c->q_in.get(), n, c->q_off.get(), total));
    if (offsets) HIP_TRY(hipMemcpy(offsets, c->q_off.get(), (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(event offsets)");
    if (cap == 0 && !t && !ev) return VR_OK;
    const uint64_t tot = *total;
    if (cap < tot) return fail(VR_ERR_OVERFLOW, "vr_query_events: " + std::to_string(tot) + " events, room for " + std::to_string(cap));
    if (tot == 0) return VR_OK;
    VR_TRY(c->q_out.grow(tot, "hipMalloc(query results)"));
    VR_TRY(c->q_out2.grow(tot * sizeof(uint32_t), "hipMalloc(query results)"));
    VR_TRY(vr_query_events_fill_device(c, (const vr_ray*)c->q_in.get(), n, c->q_off.get(), c->q_out.get(),
                                     (uint32_t*)c->q_out2.get(), tot, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_events_fill_kernel");
    HIP_TRY(hipMemcpy(t, c->q_out.get(), tot * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    HIP_TRY(hipMemcpy(ev, c->q_out2.get(), tot * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    return VR_OK;
}

vr_status vr_query_free_flight_device(vr_ctx* c, const vr_ray* d_rays, const float* d_tau_target, size_t n, float* d_t,
                                      float* d_albedo, uint32_t* d_n_active, void* stream) {
    c = first_device(c);
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_free_flight", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_tau_target || !d_t) return fail(VR_ERR_INVALID, "vr_query_free_flight: NULL argument");
    if (!aligned16(d_rays)) return fail(VR_ERR_INVALID, "vr_query_free_flight: the device ray array must be 16-byte aligned");
    if (c->opt_ff_solver == 4)
        return fail(VR_ERR_UNSUPPORTED, "vr_query_free_flight: the UNIFORM solver (VR_OPT_FF_SOLVER = 4) draws from a path's seed");
    // the rows of free_flight_pipeline (vr_frame.cpp), in this query's own buffers
    const uint32_t threads = free_flight_threads(c->cus);
    VR_TRY(c->q_ff_rows.grow((size_t)threads * (kFFHitCap + 2 * kFFActCap) * 16, "hipMalloc(free-flight query rows)"));
    VR_TRY(c->q_ff_big.grow((size_t)kFFBigThreads * 3 * (size_t)kFFBigCap * 16, "hipMalloc(free-flight query rows)"));
    VR_TRY(c->q_ff_ctl.grow(query_flight_ctl_words((uint32_t)n), "hipMalloc(free-flight query queue)"));
    float4* base = (float4*)c->q_ff_rows.get();
    A.ff_threads = threads;
    A.ff_hit_cap = kFFHitCap;
    A.ff_act_cap = kFFActCap;
    const int64_t w0 = c->opt_ff_window0 > 0 ? c->opt_ff_window0 : (int64_t)c->auto_window0;
    A.ff_hit_cap0 = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kFFHitCap, w0));
    A.ff_hit = base;
    A.ff_act0 = base + (size_t)kFFHitCap * threads;
    A.ff_act1 = base + (size_t)(kFFHitCap + kFFActCap) * threads;
    A.ff_big = (float4*)c->q_ff_big.get();
    A.ff_solver = (int32_t)c->opt_ff_solver;
    HIP_TRY(query_free_flight(A, d_rays, d_tau_target, (uint32_t)n, d_t, d_albedo, d_n_active, c->q_ff_ctl.get(), (hipStream_t)stream),
            "query_flight_kernel");
    return VR_OK;
}

vr_status vr_query_free_flight(vr_ctx* c, const vr_ray* rays, const float* tau_target, size_t n, float* t, float* albedo,
                               uint32_t* n_active) {
    c = first_device(c);
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_free_flight", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!rays || !tau_target || !t) return fail(VR_ERR_INVALID, "vr_query_free_flight: NULL argument");
    VR_TRY(c->q_in.grow(n * sizeof(vr_ray), "hipMalloc(query rays)"));
    VR_TRY(c->q_tau.grow(n, "hipMalloc(query targets)"));
    VR_TRY(c->q_out.grow(n * 2, "hipMalloc(query results)"));
    if (n_active) VR_TRY(c->q_out2.grow(n * sizeof(uint32_t), "hipMalloc(query results)"));
    HIP_TRY(hipMemcpy(c->q_in.get(), rays, n * sizeof(vr_ray), hipMemcpyHostToDevice), "hipMemcpy(query rays)");
    HIP_TRY(hipMemcpy(c->q_tau.get(), tau_target, n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(query targets)");
    VR_TRY(vr_query_free_flight_device(c, (const vr_ray*)c->q_in.get(), c->q_tau.get(), n, c->q_out.get(),
                                       albedo ? c->q_out.get() + n : nullptr, n_active ? (uint32_t*)c->q_out2.get() : nullptr, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream), "query_flight_kernel");
    HIP_TRY(hipMemcpy(t, c->q_out.get(), n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (albedo) HIP_TRY(hipMemcpy(albedo, c->q_out.get() + n, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (n_active) HIP_TRY(hipMemcpy(n_active, c->q_out2.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    uint32_t failed = 0;  // rays over kFFBigCap Gaussians at one point (ctl word 2): every output is written, those NaN
    HIP_TRY(hipMemcpy(&failed, c->q_ff_ctl.get() + 2, sizeof(failed), hipMemcpyDeviceToHost), "hipMemcpy(query results)");
    if (failed)
        return fail(VR_ERR_OVERFLOW, "vr_query_free_flight: " + std::to_string(failed) + " rays cross more than " +
                                         std::to_string(kFFBigCap) + " Gaussians overlapping one point (their results are NaN)");
    return VR_OK;
}

vr_status vr_query_pack_rays_device(vr_ctx* c, const float* d_origins, const float* d_directions, const float* d_tmax,
                                    uint32_t tmax_stride, size_t n, vr_ray* d_rays, void* stream) {
    c = first_device(c);
    if (!c) return fail(VR_ERR_INVALID, "vr_query_pack_rays_device: NULL ctx");
    if (n == 0) return VR_OK;
    if (!d_origins || !d_directions || !d_tmax || !d_rays || tmax_stride > 1 || n >= (1ull << 31) || !aligned16(d_rays))
        return fail(VR_ERR_INVALID, "vr_query_pack_rays_device: bad argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(query_pack_rays(d_origins, d_directions, d_tmax, tmax_stride, (uint32_t)n, d_rays, (hipStream_t)stream),
            "query_pack_rays_kernel");
    return VR_OK;
}

}  // extern "C"
