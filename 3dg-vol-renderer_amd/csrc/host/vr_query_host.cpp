// Mixture queries (vr_query_*, kernels/vr_query.hip, kernels/vr_query_profile.hip, kernels/vr_query_features.hip,
// kernels/vr_query_radiance.hip, kernels/vr_query_radiance_grad.hip, kernels/vr_query_flight.hip): batched transmittance and
// its gradients with respect to the Gaussians and to the rays, transmittance profiles and their gradient, ray events, sigma
// and its gradient, per-Gaussian features at points and their gradient, the emission-absorption sum along rays and its
// gradient, and free-flight distances.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>

#include "vr_ctx.h"

using namespace vr;

namespace {

// What every entry point does first: the checks they share, then the scene part of the kernel arguments. `n` entries
// of a batch; c becomes the context's first device.
vr_status query_begin(vr_ctx*& c, const char* what, size_t n, RenderArgs& A) {
    c = first_device(c);
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
    return c->q_ctl.grow(64, "hipMalloc(query counters)");  // (16 words: vr_ctx.h)
}
int query_refill(const vr_ctx* c) { return std::clamp<int>(c->auto_nee_refill, 1, 64); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Checks of more than one entry point, each with its message. `what` names the entry point.
vr_status rays_aligned(const char* what, const vr_ray* d_rays) {
    return aligned16(d_rays) ? VR_OK : fail(VR_ERR_INVALID, std::string(what) + ": the device ray array must be 16-byte aligned");
}
vr_status grad_flags(const char* what, uint32_t flags) {
    return flags & ~(uint32_t)VR_GRAD_FROZEN_BOUNDS ? fail(VR_ERR_INVALID, std::string(what) + ": unknown flag bits") : VR_OK;
}
// The four profile entry points' own, before every launch.
vr_status profile_check(const char* what, size_t t_stride, size_t n, uint32_t K) {
    if (K == 0 || K > VR_PROFILE_MAX_SAMPLES)
        return fail(VR_ERR_INVALID, std::string(what) + ": K must lie in [1, " + std::to_string(VR_PROFILE_MAX_SAMPLES) + "]");
    if (t_stride != 0 && t_stride != K) return fail(VR_ERR_INVALID, std::string(what) + ": t_stride must be 0 (one shared row) or K");
    if (n >= (1ull << 31) || n * (size_t)K >= (1ull << 31))
        return fail(VR_ERR_INVALID, std::string(what) + ": more than 2^31 - 1 samples in one call");
    return VR_OK;
}
// The two feature entry points' own, before every launch. N: the scene's Gaussians.
vr_status features_check(const char* what, size_t n, size_t N, uint32_t C) {
    if (C == 0 || C > VR_FEATURES_MAX_CHANNELS)
        return fail(VR_ERR_INVALID, std::string(what) + ": C must lie in [1, " + std::to_string(VR_FEATURES_MAX_CHANNELS) + "]");
    if (n * (size_t)C >= (1ull << 31) || N * (size_t)C >= (1ull << 31))
        return fail(VR_ERR_INVALID, std::string(what) + ": more than 2^31 - 1 feature entries in one call");
    return VR_OK;
}
// The gradient over no entries, or of a scene without Gaussians, is `words` zeros: true, and no launch follows.
bool grad_is_zero(size_t n, size_t words, float* grad) {
    if (n != 0 && words != 0) return false;
    if (grad) std::memset(grad, 0, words * sizeof(float));
    return true;
}

// ---- the host forms ----
// Each is five steps: its checks; its inputs staged in the context's workspaces (q_in, q_w, q_out, q_out2: vr_ctx.h);
// its `_device` form on c->stream; a synchronise; its results fetched. host_form is the last four. An array is
// {workspace, host pointer, 4-byte words, its name in a HIP failure's message, first word in the workspace}. One whose
// host pointer is NULL (an optional input or output) is skipped, and dev() hands the `_device` form NULL for it.
struct In { DevBuf<float>& buf; const void* host; size_t words; const char* what; };
struct Out { DevBuf<float>& buf; void* host; size_t words; const char* what; size_t at = 0; };
constexpr size_t kRayWords = sizeof(vr_ray) / 4;

vr_status room(DevBuf<float>& buf, size_t words, const char* what) {
    return buf.grow(words, (std::string("hipMalloc(") + what + ")").c_str());
}
vr_status copy(void* dst, const void* src, size_t words, hipMemcpyKind kind, const char* what) {
    return hip_status(hipMemcpy(dst, src, words * 4, kind), (std::string("hipMemcpy(") + what + ")").c_str());
}
template <class T>
T* dev(const DevBuf<float>& buf, const void* host, size_t at = 0) {
    return host ? reinterpret_cast<T*>(buf.get() + at) : nullptr;
}
template <class Call>
vr_status host_form(vr_ctx* c, std::initializer_list<In> ins, std::initializer_list<Out> outs, const char* kernel, Call call) {
    for (const In& a : ins)
        if (a.host) {
            VR_TRY(room(a.buf, a.words, a.what));
            VR_TRY(copy(a.buf.get(), a.host, a.words, hipMemcpyHostToDevice, a.what));
        }
    for (const Out& a : outs)
        if (a.host) VR_TRY(room(a.buf, a.at + a.words, a.what));
    VR_TRY(call());
    HIP_TRY(hipStreamSynchronize(c->stream), kernel);
    for (const Out& a : outs)
        if (a.host) VR_TRY(copy(a.host, a.buf.get() + a.at, a.words, hipMemcpyDeviceToHost, a.what));
    return VR_OK;
}

}  // namespace

extern "C" {

vr_status vr_query_transmittance_device(vr_ctx* c, const vr_ray* d_rays, size_t n, float* d_tr, float* d_tau, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_tr) return fail(VR_ERR_INVALID, "vr_query_transmittance: NULL argument");
    VR_TRY(rays_aligned("vr_query_transmittance", d_rays));
    HIP_TRY(query_transmittance(A, d_rays, (uint32_t)n, d_tr, d_tau, (uint32_t*)c->q_ctl.get(), query_refill(c), c->cus,
                                (hipStream_t)stream),
            "query_transmittance_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance(vr_ctx* c, const vr_ray* rays, size_t n, float* tr, float* tau) {
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_transmittance", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!rays || !tr) return fail(VR_ERR_INVALID, "vr_query_transmittance: NULL argument");
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}},
                     {{c->q_out, tr, n, "query results"}, {c->q_out2, tau, n, "query results"}}, "query_transmittance_kernel", [&] {
                         return vr_query_transmittance_device(c, dev<vr_ray>(c->q_in, rays), n, dev<float>(c->q_out, tr),
                                                              dev<float>(c->q_out2, tau), c->stream);
                     });
}

vr_status vr_query_transmittance_grad_device(vr_ctx* c, const vr_ray* d_rays, const float* d_weight, size_t n, uint32_t flags,
                                             float* d_grad, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_grad", n, A));
    VR_TRY(grad_flags("vr_query_transmittance_grad", flags));
    if (!d_grad || (n > 0 && !d_rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: NULL argument");
    VR_TRY(rays_aligned("vr_query_transmittance_grad", d_rays));
    // the staging rows are the query's own: a frame queued on another stream never sees them
    VR_TRY(c->q_grad.grow((size_t)std::max(A.num_prims, 1) * 10, "hipMalloc(gradient staging)"));
    HIP_TRY(query_transmittance_grad(A, d_rays, d_weight, (uint32_t)n, !(flags & VR_GRAD_FROZEN_BOUNDS), c->q_grad.get(), d_grad,
                                     (uint32_t*)c->q_ctl.get() + 3, query_refill(c), c->cus, (hipStream_t)stream),
            "query_grad_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_grad(vr_ctx* c, const vr_ray* rays, const float* weight, size_t n, uint32_t flags, float* grad) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_grad", n, A));
    VR_TRY(grad_flags("vr_query_transmittance_grad", flags));
    if (!grad || (n > 0 && !rays)) return fail(VR_ERR_INVALID, "vr_query_transmittance_grad: NULL argument");
    const size_t words = (size_t)std::max(A.num_prims, 0) * 10;
    if (grad_is_zero(n, words, grad)) return VR_OK;
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, weight, n, "query weights"}},
                     {{c->q_out, grad, words, "query results"}}, "query_grad_kernel", [&] {
                         return vr_query_transmittance_grad_device(c, dev<vr_ray>(c->q_in, rays), dev<float>(c->q_w, weight), n, flags,
                                                                   c->q_out.get(), c->stream);
                     });
}

vr_status vr_query_transmittance_ray_grad_device(vr_ctx* c, const vr_ray* d_rays, size_t n, uint32_t flags, vr_ray_grad* d_out,
                                                 void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_ray_grad", n, A));
    VR_TRY(grad_flags("vr_query_transmittance_ray_grad", flags));
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
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_ray_grad", n, A));
    VR_TRY(grad_flags("vr_query_transmittance_ray_grad", flags));
    if (n == 0) return VR_OK;
    if (!rays || !out) return fail(VR_ERR_INVALID, "vr_query_transmittance_ray_grad: NULL argument");
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}},
                     {{c->q_out, out, n * (sizeof(vr_ray_grad) / 4), "query results"}}, "query_ray_grad_kernel", [&] {
                         return vr_query_transmittance_ray_grad_device(c, dev<vr_ray>(c->q_in, rays), n, flags,
                                                                       dev<vr_ray_grad>(c->q_out, out), c->stream);
                     });
}

// ---- transmittance profile: K samples per ray from one walk ----
vr_status vr_query_transmittance_profile_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride, size_t n,
                                                uint32_t K, float* d_tr, float* d_tau, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile", t_stride, n, K));
    if (!d_tr && !d_tau) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: both outputs are NULL");
    if (n == 0) return VR_OK;
    if (!d_rays || !d_t) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: NULL argument");
    VR_TRY(rays_aligned("vr_query_transmittance_profile", d_rays));
    HIP_TRY(query_transmittance_profile(A, d_rays, d_t, (uint32_t)t_stride, (uint32_t)n, K, d_tr, d_tau,
                                        (uint32_t*)c->q_ctl.get() + 8, query_refill(c), c->cus, (hipStream_t)stream),
            "query_profile_kernel");
    return VR_OK;
}

vr_status vr_query_transmittance_profile(vr_ctx* c, const vr_ray* rays, const float* t, size_t t_stride, size_t n, uint32_t K,
                                         float* tr, float* tau) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile", t_stride, n, K));
    if (!tr && !tau) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: both outputs are NULL");
    if (n == 0) return VR_OK;
    if (!rays || !t) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile: NULL argument");
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K;
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, t, nt, "profile samples"}},
                     {{c->q_out, tr, nk, "profile results"}, {c->q_out2, tau, nk, "profile results"}}, "query_profile_kernel", [&] {
                         return vr_query_transmittance_profile_device(c, dev<vr_ray>(c->q_in, rays), c->q_w.get(), t_stride, n, K,
                                                                      dev<float>(c->q_out, tr), dev<float>(c->q_out2, tau), c->stream);
                     });
}

vr_status vr_query_transmittance_profile_grad_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride,
                                                     const float* d_weight, size_t n, uint32_t K, uint32_t flags, float* d_grad,
                                                     void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile_grad", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile_grad", t_stride, n, K));
    VR_TRY(grad_flags("vr_query_transmittance_profile_grad", flags));
    if (!d_grad || (n > 0 && (!d_rays || !d_t))) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: NULL argument");
    VR_TRY(rays_aligned("vr_query_transmittance_profile_grad", d_rays));
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
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_transmittance_profile_grad", n, A));
    VR_TRY(profile_check("vr_query_transmittance_profile_grad", t_stride, n, K));
    VR_TRY(grad_flags("vr_query_transmittance_profile_grad", flags));
    if (!grad || (n > 0 && (!rays || !t))) return fail(VR_ERR_INVALID, "vr_query_transmittance_profile_grad: NULL argument");
    const size_t words = (size_t)std::max(A.num_prims, 0) * 10;
    if (grad_is_zero(n, words, grad)) return VR_OK;
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K;
    // (three inputs and one result: the weights stand in the second result's workspace)
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, t, nt, "profile samples"},
                         {c->q_out2, weight, nk, "profile weights"}},
                     {{c->q_out, grad, words, "profile results"}}, "query_profile_grad_kernel", [&] {
                         return vr_query_transmittance_profile_grad_device(c, dev<vr_ray>(c->q_in, rays), c->q_w.get(), t_stride,
                                                                           dev<float>(c->q_out2, weight), n, K, flags, c->q_out.get(),
                                                                           c->stream);
                     });
}

vr_status vr_query_sigma_device(vr_ctx* c, const float* d_xyz, size_t n, float* d_sigma_as, uint32_t* d_n_active, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_sigma", n, A));
    if (n == 0) return VR_OK;
    if (!d_xyz || !d_sigma_as) return fail(VR_ERR_INVALID, "vr_query_sigma: NULL argument");
    HIP_TRY(query_sigma(A, d_xyz, (uint32_t)n, d_sigma_as, d_n_active, (hipStream_t)stream), "query_sigma_kernel");
    return VR_OK;
}

vr_status vr_query_sigma(vr_ctx* c, const float* xyz, size_t n, float* sigma_as, uint32_t* n_active) {
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_sigma", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!xyz || !sigma_as) return fail(VR_ERR_INVALID, "vr_query_sigma: NULL argument");
    return host_form(c, {{c->q_in, xyz, n * 3, "query points"}},
                     {{c->q_out, sigma_as, n * 2, "query results"}, {c->q_out2, n_active, n, "query results"}}, "query_sigma_kernel", [&] {
                         return vr_query_sigma_device(c, c->q_in.get(), n, c->q_out.get(), dev<uint32_t>(c->q_out2, n_active), c->stream);
                     });
}

vr_status vr_query_sigma_grad_device(vr_ctx* c, const float* d_xyz, const float* d_weight_as, size_t n, float* d_grad,
                                     float* d_grad_xyz, void* stream) {
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
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_sigma_grad", n, A));
    const size_t words = (size_t)std::max(A.num_prims, 0) * 11;
    if (n == 0 && grad_is_zero(n, words, grad)) return VR_OK;
    if (!xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: NULL argument");
    if (!grad && !grad_xyz) return fail(VR_ERR_INVALID, "vr_query_sigma_grad: both outputs are NULL");
    if (words == 0) grad = nullptr;  // an empty scene: grad has no entries,
    if (!grad && !grad_xyz) return VR_OK;  // and nothing else was asked for
    return host_form(c, {{c->q_in, xyz, n * 3, "query points"}, {c->q_w, weight_as, n * 2, "query weights"}},
                     {{c->q_out, grad, words, "query results"}, {c->q_out2, grad_xyz, n * 3, "query results"}},
                     "query_sigma_grad_kernel", [&] {
                         return vr_query_sigma_grad_device(c, c->q_in.get(), dev<float>(c->q_w, weight_as), n, dev<float>(c->q_out, grad),
                                                           dev<float>(c->q_out2, grad_xyz), c->stream);
                     });
}

// ---- features: sum_g m_g(x) f_gc over the active set, for the caller's rows f ----
vr_status vr_query_features_device(vr_ctx* c, const float* d_xyz, size_t n, const float* d_features, uint32_t C, float* d_out,
                                   float* d_mass, uint32_t* d_n_active, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_features", n, A));
    VR_TRY(features_check("vr_query_features", n, (size_t)std::max(A.num_prims, 0), C));
    if (n == 0) return VR_OK;
    if (!d_xyz || !d_features || !d_out) return fail(VR_ERR_INVALID, "vr_query_features: NULL argument");
    HIP_TRY(query_features(A, d_xyz, (uint32_t)n, d_features, C, d_out, d_mass, d_n_active, (hipStream_t)stream),
            "query_features_kernel");
    return VR_OK;
}

vr_status vr_query_features(vr_ctx* c, const float* xyz, size_t n, const float* features, uint32_t C, float* out, float* mass,
                            uint32_t* n_active) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_features", n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(features_check("vr_query_features", n, N, C));
    if (n == 0) return VR_OK;
    if (!xyz || !features || !out) return fail(VR_ERR_INVALID, "vr_query_features: NULL argument");
    if (N == 0) {  // an empty scene: there are no rows to send, and every result is +0
        std::memset(out, 0, n * (size_t)C * sizeof(float));
        if (mass) std::memset(mass, 0, n * sizeof(float));
        if (n_active) std::memset(n_active, 0, n * sizeof(uint32_t));
        return VR_OK;
    }
    // (the mass and the counts share the second result's workspace)
    return host_form(c, {{c->q_in, xyz, n * 3, "query points"}, {c->q_feat, features, N * C, "query features"}},
                     {{c->q_out, out, n * (size_t)C, "query results"}, {c->q_out2, mass, n, "query results"},
                      {c->q_out2, n_active, n, "query results", n}},
                     "query_features_kernel", [&] {
                         return vr_query_features_device(c, c->q_in.get(), n, c->q_feat.get(), C, c->q_out.get(),
                                                         dev<float>(c->q_out2, mass), dev<uint32_t>(c->q_out2, n_active, n), c->stream);
                     });
}

vr_status vr_query_features_grad_device(vr_ctx* c, const float* d_xyz, size_t n, const float* d_features, uint32_t C,
                                        const float* d_weights, const float* d_weight_mass, float* d_grad, float* d_grad_features,
                                        float* d_grad_xyz, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_features_grad", n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(features_check("vr_query_features_grad", n, N, C));
    if (n == 0) {
        if (d_grad && N) HIP_TRY(hipMemsetAsync(d_grad, 0, N * 10 * sizeof(float), (hipStream_t)stream), "hipMemset(feature gradient)");
        if (d_grad_features && N)
            HIP_TRY(hipMemsetAsync(d_grad_features, 0, N * C * sizeof(float), (hipStream_t)stream), "hipMemset(feature gradient)");
        return VR_OK;
    }
    if (!d_xyz || !d_features) return fail(VR_ERR_INVALID, "vr_query_features_grad: NULL argument");
    if (!d_grad && !d_grad_features && !d_grad_xyz) return fail(VR_ERR_INVALID, "vr_query_features_grad: all three outputs are NULL");
    // the staging rows are the query's own: a frame or another gradient query queued on another stream never sees them
    if (d_grad) VR_TRY(c->q_feat_grad.grow(std::max<size_t>(N, 1) * 10, "hipMalloc(gradient staging)"));
    if (d_grad_features) VR_TRY(c->q_feat_fgrad.grow(std::max<size_t>(N, 1) * C, "hipMalloc(feature gradient staging)"));
    HIP_TRY(query_features_grad(A, d_xyz, (uint32_t)n, d_features, C, d_weights, d_weight_mass,
                                d_grad ? c->q_feat_grad.get() : nullptr, d_grad_features ? c->q_feat_fgrad.get() : nullptr, d_grad,
                                d_grad_features, d_grad_xyz, (hipStream_t)stream),
            "query_features_grad_kernel");
    return VR_OK;
}

vr_status vr_query_features_grad(vr_ctx* c, const float* xyz, size_t n, const float* features, uint32_t C, const float* weights,
                                 const float* weight_mass, float* grad, float* grad_features, float* grad_xyz) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_features_grad", n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(features_check("vr_query_features_grad", n, N, C));
    if (n == 0) {
        grad_is_zero(0, N * 10, grad);
        grad_is_zero(0, N * C, grad_features);
        return VR_OK;
    }
    if (!xyz || !features) return fail(VR_ERR_INVALID, "vr_query_features_grad: NULL argument");
    if (!grad && !grad_features && !grad_xyz) return fail(VR_ERR_INVALID, "vr_query_features_grad: all three outputs are NULL");
    if (N == 0) {  // an empty scene: grad and grad_features have no entries, and no point has an active Gaussian
        if (grad_xyz) std::memset(grad_xyz, 0, n * 3 * sizeof(float));
        return VR_OK;
    }
    // (the points' rows follow the features' in the second result's workspace)
    const size_t at_xyz = grad_features ? N * C : 0;
    return host_form(c, {{c->q_in, xyz, n * 3, "query points"}, {c->q_feat, features, N * C, "query features"},
                         {c->q_w, weights, n * (size_t)C, "query weights"}, {c->q_w2, weight_mass, n, "query weights"}},
                     {{c->q_out, grad, N * 10, "query results"}, {c->q_out2, grad_features, N * C, "query results"},
                      {c->q_out2, grad_xyz, n * 3, "query results", at_xyz}},
                     "query_features_grad_kernel", [&] {
                         return vr_query_features_grad_device(c, c->q_in.get(), n, c->q_feat.get(), C, dev<float>(c->q_w, weights),
                                                              dev<float>(c->q_w2, weight_mass), dev<float>(c->q_out, grad),
                                                              dev<float>(c->q_out2, grad_features),
                                                              dev<float>(c->q_out2, grad_xyz, at_xyz), c->stream);
                     });
}

// ---- radiance: sum_k q T sum_g m f along each ray; the profile's walk for T, then one walk for the sum ----
namespace {
vr_status radiance_check(size_t t_stride, size_t q_stride, bool has_q, size_t n, size_t N, uint32_t K, uint32_t C,
                         const char* what = "vr_query_radiance") {
    VR_TRY(profile_check(what, t_stride, n, K));
    VR_TRY(features_check(what, n, N, C));
    if (has_q && q_stride != 0 && q_stride != K) return fail(VR_ERR_INVALID, std::string(what) + ": q_stride must be 0 (one shared row) or K");
    return VR_OK;
}
}  // namespace

vr_status vr_query_radiance_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride, const float* d_q,
                                   size_t q_stride, size_t n, uint32_t K, const float* d_features, uint32_t C, float* d_out,
                                   float* d_opacity, float* d_tr, uint32_t* d_n_pairs, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_radiance", n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(radiance_check(t_stride, q_stride, d_q != nullptr, n, N, K, C));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_t || !d_features || !d_out) return fail(VR_ERR_INVALID, "vr_query_radiance: NULL argument");
    VR_TRY(rays_aligned("vr_query_radiance", d_rays));
    // Tr without a place of the caller's: the query's own workspace, so a profile query on another stream never shares it
    if (!d_tr) {
        VR_TRY(c->q_rad_tr.grow(n * (size_t)K, "hipMalloc(radiance transmittances)"));
        d_tr = c->q_rad_tr.get();
    }
    uint32_t* ctl = (uint32_t*)c->q_ctl.get();
    HIP_TRY(query_transmittance_profile(A, d_rays, d_t, (uint32_t)t_stride, (uint32_t)n, K, d_tr, nullptr, ctl + 10, query_refill(c),
                                        c->cus, (hipStream_t)stream),
            "query_profile_kernel");
    HIP_TRY(query_radiance(A, d_rays, d_t, (uint32_t)t_stride, d_q, (uint32_t)q_stride, (uint32_t)n, K, d_features, C, d_tr, d_out,
                           d_opacity, d_n_pairs, ctl + 11, query_refill(c), c->cus, (hipStream_t)stream),
            "query_radiance_kernel");
    return VR_OK;
}

vr_status vr_query_radiance(vr_ctx* c, const vr_ray* rays, const float* t, size_t t_stride, const float* q, size_t q_stride, size_t n,
                            uint32_t K, const float* features, uint32_t C, float* out, float* opacity, float* tr, uint32_t* n_pairs) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_radiance", n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(radiance_check(t_stride, q_stride, q != nullptr, n, N, K, C));
    if (n == 0) return VR_OK;
    if (!rays || !t || !features || !out) return fail(VR_ERR_INVALID, "vr_query_radiance: NULL argument");
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K, nq = q_stride ? nk : (size_t)K;
    VR_TRY(room(c->q_feat, std::max<size_t>(N * C, 1), "query features"));  // (an empty scene has no rows; the pointer is not read)
    // (the opacity and the counts share the third result's workspace)
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, t, nt, "profile samples"},
                         {c->q_w3, q, nq, "quadrature weights"}, {c->q_feat, N ? features : nullptr, N * C, "query features"}},
                     {{c->q_out, out, n * (size_t)C, "query results"}, {c->q_out2, tr, nk, "profile results"},
                      {c->q_out3, opacity, n, "query results"}, {c->q_out3, n_pairs, n, "query results", n}},
                     "query_radiance_kernel", [&] {
                         return vr_query_radiance_device(c, dev<vr_ray>(c->q_in, rays), c->q_w.get(), t_stride, dev<float>(c->q_w3, q),
                                                         q_stride, n, K, c->q_feat.get(), C, c->q_out.get(), dev<float>(c->q_out3, opacity),
                                                         dev<float>(c->q_out2, tr), dev<uint32_t>(c->q_out3, n_pairs, n), c->stream);
                     });
}

// ---- radiance gradient: the profile's walk for T if the caller has none, one walk per ray, the profile gradient's walk ----
vr_status vr_query_radiance_grad_device(vr_ctx* c, const vr_ray* d_rays, const float* d_t, size_t t_stride, const float* d_q,
                                        size_t q_stride, size_t n, uint32_t K, const float* d_features, uint32_t C,
                                        const float* d_weights, const float* d_weight_opacity, const float* d_tr, uint32_t flags,
                                        float* d_grad, float* d_grad_features, float* d_grad_q, float* d_grad_tau, void* stream) {
    const char* what = "vr_query_radiance_grad";
    RenderArgs A;
    VR_TRY(query_begin(c, what, n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(radiance_check(t_stride, q_stride, d_q != nullptr, n, N, K, C, what));
    VR_TRY(grad_flags(what, flags));
    if (n == 0) {
        if (d_grad && N) HIP_TRY(hipMemsetAsync(d_grad, 0, N * 10 * sizeof(float), (hipStream_t)stream), "hipMemset(radiance gradient)");
        if (d_grad_features && N)
            HIP_TRY(hipMemsetAsync(d_grad_features, 0, N * C * sizeof(float), (hipStream_t)stream), "hipMemset(radiance gradient)");
        return VR_OK;
    }
    if (!d_rays || !d_t || !d_features) return fail(VR_ERR_INVALID, "vr_query_radiance_grad: NULL argument");
    if (!d_grad && !d_grad_features && !d_grad_q && !d_grad_tau) return fail(VR_ERR_INVALID, "vr_query_radiance_grad: all four outputs are NULL");
    VR_TRY(rays_aligned(what, d_rays));
    if (N == 0) d_grad = d_grad_features = nullptr;  // an empty scene: they have no entries
    if (!d_grad && !d_grad_features && !d_grad_q && !d_grad_tau) return VR_OK;
    // the workspaces are the query's own: a frame or another query queued on another stream never sees them
    const size_t nk = n * (size_t)K;
    const bool rows = d_grad || d_grad_q || d_grad_tau;
    if (rows) VR_TRY(c->q_radg_s.grow(nk, "hipMalloc(radiance gradient rows)"));
    if (d_grad) VR_TRY(c->q_radg_stage.grow(N * 10, "hipMalloc(gradient staging)"));
    if (d_grad_features) VR_TRY(c->q_radg_fstage.grow(N * C, "hipMalloc(feature gradient staging)"));
    if (d_grad && !d_grad_tau) VR_TRY(c->q_radg_tau.grow(nk, "hipMalloc(radiance gradient weights)"));
    uint32_t* ctl = (uint32_t*)c->q_ctl.get();
    if (!d_tr) {
        VR_TRY(c->q_radg_tr.grow(nk, "hipMalloc(radiance transmittances)"));
        HIP_TRY(query_transmittance_profile(A, d_rays, d_t, (uint32_t)t_stride, (uint32_t)n, K, c->q_radg_tr.get(), nullptr, ctl + 12,
                                            query_refill(c), c->cus, (hipStream_t)stream),
                "query_profile_kernel");
        d_tr = c->q_radg_tr.get();
    }
    HIP_TRY(query_radiance_grad(A, d_rays, d_t, (uint32_t)t_stride, d_q, (uint32_t)q_stride, (uint32_t)n, K, d_features, C, d_weights,
                                d_weight_opacity, d_tr, !(flags & VR_GRAD_FROZEN_BOUNDS), rows ? c->q_radg_s.get() : nullptr,
                                d_grad ? c->q_radg_stage.get() : nullptr, d_grad_features ? c->q_radg_fstage.get() : nullptr,
                                d_grad && !d_grad_tau ? c->q_radg_tau.get() : nullptr, d_grad, d_grad_features, d_grad_q, d_grad_tau,
                                ctl + 13, query_refill(c), c->cus, (hipStream_t)stream),
            "query_radiance_grad_kernel");
    return VR_OK;
}

vr_status vr_query_radiance_grad(vr_ctx* c, const vr_ray* rays, const float* t, size_t t_stride, const float* q, size_t q_stride,
                                 size_t n, uint32_t K, const float* features, uint32_t C, const float* weights,
                                 const float* weight_opacity, const float* tr, uint32_t flags, float* grad, float* grad_features,
                                 float* grad_q, float* grad_tau) {
    const char* what = "vr_query_radiance_grad";
    RenderArgs A;
    VR_TRY(query_begin(c, what, n, A));
    const size_t N = (size_t)std::max(A.num_prims, 0);
    VR_TRY(radiance_check(t_stride, q_stride, q != nullptr, n, N, K, C, what));
    VR_TRY(grad_flags(what, flags));
    if (n == 0) {
        grad_is_zero(0, N * 10, grad);
        grad_is_zero(0, N * C, grad_features);
        return VR_OK;
    }
    if (!rays || !t || !features) return fail(VR_ERR_INVALID, "vr_query_radiance_grad: NULL argument");
    if (!grad && !grad_features && !grad_q && !grad_tau) return fail(VR_ERR_INVALID, "vr_query_radiance_grad: all four outputs are NULL");
    if (N == 0) grad = grad_features = nullptr;  // an empty scene: they have no entries,
    if (!grad && !grad_features && !grad_q && !grad_tau) return VR_OK;  // and nothing else was asked for
    const size_t nk = n * (size_t)K, nt = t_stride ? nk : (size_t)K, nq = q_stride ? nk : (size_t)K;
    VR_TRY(room(c->q_feat, std::max<size_t>(N * C, 1), "query features"));  // (an empty scene has no rows; the pointer is not read)
    // (the rows' gradient follows the Gaussians' in the first result's workspace)
    return host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, t, nt, "profile samples"},
                         {c->q_w3, q, nq, "quadrature weights"}, {c->q_feat, N ? features : nullptr, N * C, "query features"},
                         {c->q_w2, weights, n * (size_t)C, "query weights"}, {c->q_w4, weight_opacity, n, "query weights"},
                         {c->q_w5, tr, nk, "profile results"}},
                     {{c->q_out, grad, N * 10, "query results"}, {c->q_out, grad_features, N * C, "query results", N * 10},
                      {c->q_out2, grad_q, nk, "query results"}, {c->q_out3, grad_tau, nk, "query results"}},
                     "query_radiance_grad_kernel", [&] {
                         return vr_query_radiance_grad_device(c, dev<vr_ray>(c->q_in, rays), c->q_w.get(), t_stride, dev<float>(c->q_w3, q),
                                                              q_stride, n, K, c->q_feat.get(), C, dev<float>(c->q_w2, weights),
                                                              dev<float>(c->q_w4, weight_opacity), dev<float>(c->q_w5, tr), flags,
                                                              dev<float>(c->q_out, grad), dev<float>(c->q_out, grad_features, N * 10),
                                                              dev<float>(c->q_out2, grad_q), dev<float>(c->q_out3, grad_tau), c->stream);
                     });
}

vr_status vr_query_events_count_device(vr_ctx* c, const vr_ray* d_rays, size_t n, uint32_t* d_offsets, uint64_t* total) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_events", n, A));
    if (!total) return fail(VR_ERR_INVALID, "vr_query_events: NULL total");
    *total = 0;
    if (n == 0) return VR_OK;
    if (!d_rays || !d_offsets) return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    VR_TRY(rays_aligned("vr_query_events", d_rays));
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
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_events", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_offsets) return fail(VR_ERR_INVALID, "vr_query_events: NULL argument");
    VR_TRY(rays_aligned("vr_query_events", d_rays));
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

// The pair's host form: the count (it synchronises itself) and the offsets, which stay in q_w for the fill; then, if
// the caller gave room, the fill as a host form of its own.
vr_status vr_query_events(vr_ctx* c, const vr_ray* rays, size_t n, uint32_t* offsets, float* t, uint32_t* ev, uint64_t cap,
                          uint64_t* total) {
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
    VR_TRY(room(c->q_in, n * kRayWords, "query rays"));
    VR_TRY(room(c->q_w, n + 1, "event offsets"));
    const vr_ray* d_rays = (const vr_ray*)c->q_in.get();
    uint32_t* d_off = (uint32_t*)c->q_w.get();
    VR_TRY(copy(c->q_in.get(), rays, n * kRayWords, hipMemcpyHostToDevice, "query rays"));
    VR_TRY(vr_query_events_count_device(c, d_rays, n, d_off, total));
    if (offsets) VR_TRY(copy(offsets, d_off, n + 1, hipMemcpyDeviceToHost, "event offsets"));
    if (cap == 0 && !t && !ev) return VR_OK;
    const uint64_t tot = *total;
    if (cap < tot) return fail(VR_ERR_OVERFLOW, "vr_query_events: " + std::to_string(tot) + " events, room for " + std::to_string(cap));
    if (tot == 0) return VR_OK;
    return host_form(c, {}, {{c->q_out, t, tot, "query results"}, {c->q_out2, ev, tot, "query results"}}, "query_events_fill_kernel", [&] {
        return vr_query_events_fill_device(c, d_rays, n, d_off, c->q_out.get(), dev<uint32_t>(c->q_out2, ev), tot, c->stream);
    });
}

vr_status vr_query_free_flight_device(vr_ctx* c, const vr_ray* d_rays, const float* d_tau_target, size_t n, float* d_t,
                                      float* d_albedo, uint32_t* d_n_active, void* stream) {
    RenderArgs A;
    VR_TRY(query_begin(c, "vr_query_free_flight", n, A));
    if (n == 0) return VR_OK;
    if (!d_rays || !d_tau_target || !d_t) return fail(VR_ERR_INVALID, "vr_query_free_flight: NULL argument");
    VR_TRY(rays_aligned("vr_query_free_flight", d_rays));
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
    RenderArgs A;
    vr_status st = query_begin(c, "vr_query_free_flight", n, A);
    if (st != VR_OK || n == 0) return st;
    if (!rays || !tau_target || !t) return fail(VR_ERR_INVALID, "vr_query_free_flight: NULL argument");
    // (t and the albedo share the first result's workspace)
    VR_TRY(host_form(c, {{c->q_in, rays, n * kRayWords, "query rays"}, {c->q_w, tau_target, n, "query targets"}},
                     {{c->q_out, t, n, "query results"}, {c->q_out, albedo, n, "query results", n},
                      {c->q_out2, n_active, n, "query results"}},
                     "query_flight_kernel", [&] {
                         return vr_query_free_flight_device(c, dev<vr_ray>(c->q_in, rays), c->q_w.get(), n, c->q_out.get(),
                                                            dev<float>(c->q_out, albedo, n), dev<uint32_t>(c->q_out2, n_active), c->stream);
                     }));
    uint32_t failed = 0;  // rays over kFFBigCap Gaussians at one point (ctl word 2): every output is written, those NaN
    VR_TRY(copy(&failed, c->q_ff_ctl.get() + 2, 1, hipMemcpyDeviceToHost, "query results"));
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
