// query.h — the reference's GaussianMixtureModel queries (include/gmm.h) in batch form over the C ABI
// (include/vr_hip.h, vr_query_*): the mixture is the uploaded scene, the batch runs on the GPU.
#pragma once
#include <limits>

#include "integrator.h"
#include "ray.h"

// smm.h:7-15
struct PrimitiveHitEvent {
    float t;        // distance along ray
    bool entering;  // entering/exiting primitive
    size_t index;   // index in mixture model array
    bool operator<(const PrimitiveHitEvent& other) const { return t < other.t; }
};

// The three questions the reference's integrators ask scene.gmm, for many rays / points at once. The
// context is obtained as HipIntegrator obtains its own (one per GPU, created on first use) and the scene is
// uploaded when it changed, so a MixtureQuery and the integrators of one program share the uploaded scene.
class MixtureQuery {
    const Scene& scene_;
    int device_;

    vr_ctx* ready() const {
        vr_ctx* ctx = context();
        HipIntegrator::upload(ctx, scene_);
        return ctx;
    }
    // A Ray's direction was normalised by its constructor (ray.h:11-12): it goes to the device as it stands.
    static std::vector<vr_ray> pack(const std::vector<Ray>& rays, const std::vector<float>* tmax, float tmax_all) {
        std::vector<vr_ray> r(rays.size());
        for (size_t i = 0; i < rays.size(); ++i) {
            for (int k = 0; k < 3; ++k) {
                r[i].origin[k] = rays[i].origin[k];
                r[i].direction[k] = rays[i].direction[k];
            }
            r[i].tmax = tmax ? (*tmax)[i] : tmax_all;
            r[i].unit = 1.0f;
        }
        return r;
    }

public:
    explicit MixtureQuery(const Scene& scene, int dev = 0) : scene_(scene), device_(dev) {}
    vr_ctx* context() const { return vr_cpp::device(device_); }

    // gmm.h:517-578 transmittance_up_to(ray, tmax) per ray; *tau (if given) receives the optical depths.
    std::vector<float> transmittance_up_to(const std::vector<Ray>& rays, const std::vector<float>& tmax,
                                           std::vector<float>* tau = nullptr) const {
        if (tmax.size() != rays.size()) throw std::runtime_error("transmittance_up_to: one tmax per ray");
        return transmittance(pack(rays, &tmax, 0.0f), tau);
    }
    std::vector<float> transmittance_up_to(const std::vector<Ray>& rays, float tmax = std::numeric_limits<float>::infinity(),
                                           std::vector<float>* tau = nullptr) const {
        return transmittance(pack(rays, nullptr, tmax), tau);
    }

    // The gradient of those optical depths with respect to the Gaussians (vr_query_transmittance_grad): row g of the
    // result (10 floats per scene Gaussian) is sum_i weights[i] * d tau_i / d (mean[3], cov[6] = {xx, xy, xz, yy, yz,
    // zz}, density); an empty `weights` means 1 for every ray. moving_bounds = false holds each Gaussian's entry and
    // exit distances fixed (VR_GRAD_FROZEN_BOUNDS).
    std::vector<float> transmittance_gradient(const std::vector<Ray>& rays, const std::vector<float>& tmax,
                                              const std::vector<float>& weights = {}, bool moving_bounds = true) const {
        if (tmax.size() != rays.size()) throw std::runtime_error("transmittance_gradient: one tmax per ray");
        if (!weights.empty() && weights.size() != rays.size()) throw std::runtime_error("transmittance_gradient: one weight per ray");
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, &tmax, 0.0f);
        std::vector<float> grad(10 * scene_.get_num_primitives() + 1, 0.0f);  // (+ 1: never a NULL pointer)
        vr_cpp::check(vr_query_transmittance_grad(ctx, r.data(), weights.empty() ? nullptr : weights.data(), r.size(),
                                                  moving_bounds ? 0u : (uint32_t)VR_GRAD_FROZEN_BOUNDS, grad.data()));
        grad.pop_back();
        return grad;
    }

    // The gradient of those optical depths with respect to the rays (vr_query_transmittance_ray_grad): row i is
    // d tau_i / d (origin, tmax, direction) and tau_i itself (the forward query's, bit for bit). A Ray's direction is
    // its constructor's (unit = 1), so `direction` is the derivative with respect to the three stored components
    // taken as free. moving_bounds = false holds each Gaussian's entry and exit distances fixed (VR_GRAD_FROZEN_BOUNDS).
    std::vector<vr_ray_grad> transmittance_ray_gradient(const std::vector<Ray>& rays, const std::vector<float>& tmax,
                                                        bool moving_bounds = true) const {
        if (tmax.size() != rays.size()) throw std::runtime_error("transmittance_ray_gradient: one tmax per ray");
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, &tmax, 0.0f);
        std::vector<vr_ray_grad> out(r.size());
        vr_cpp::check(vr_query_transmittance_ray_grad(ctx, r.data(), r.size(),
                                                      moving_bounds ? 0u : (uint32_t)VR_GRAD_FROZEN_BOUNDS, out.data()));
        return out;
    }

    // transmittance_up_to at K distances along every ray from one tree walk per ray (vr_query_transmittance_profile):
    // the result holds Tr row-major, rays.size() * K floats, *tau (if given) the optical depths. `t` holds K distances
    // shared by all rays, or rays.size() * K, row i for ray i, in any order; entry (i, k) has the bits of
    // transmittance_up_to(ray i, t[i][k]).
    std::vector<float> transmittance_profile(const std::vector<Ray>& rays, const std::vector<float>& t, uint32_t K,
                                             std::vector<float>* tau = nullptr) const {
        const size_t stride = profile_stride("transmittance_profile", rays.size(), t.size(), K);
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, std::numeric_limits<float>::infinity());
        std::vector<float> tr(r.size() * K);
        if (tau) tau->assign(r.size() * K, 0.0f);
        vr_cpp::check(vr_query_transmittance_profile(ctx, r.data(), t.data(), stride, r.size(), K, tr.data(),
                                                     tau ? tau->data() : nullptr));
        return tr;
    }

    // The gradient of a weighted sum of that profile's optical depths with respect to the Gaussians
    // (vr_query_transmittance_profile_grad): row g of the result (10 floats per scene Gaussian, transmittance_gradient's
    // layout) is sum_i sum_k weights[i * K + k] * d tau[i][k] / d theta_g; an empty `weights` means 1 for every sample.
    // One walk per ray and ten atomic adds per (ray, Gaussian) hit, whatever K is.
    std::vector<float> transmittance_profile_gradient(const std::vector<Ray>& rays, const std::vector<float>& t, uint32_t K,
                                                      const std::vector<float>& weights = {}, bool moving_bounds = true) const {
        const size_t stride = profile_stride("transmittance_profile_gradient", rays.size(), t.size(), K);
        if (!weights.empty() && weights.size() != rays.size() * K)
            throw std::runtime_error("transmittance_profile_gradient: one weight per ray and sample");
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, std::numeric_limits<float>::infinity());
        std::vector<float> grad(10 * scene_.get_num_primitives() + 1, 0.0f);  // (+ 1: never a NULL pointer)
        vr_cpp::check(vr_query_transmittance_profile_grad(ctx, r.data(), t.data(), stride, weights.empty() ? nullptr : weights.data(),
                                                          r.size(), K, moving_bounds ? 0u : (uint32_t)VR_GRAD_FROZEN_BOUNDS,
                                                          grad.data()));
        grad.pop_back();
        return grad;
    }

    // gmm.h:457-515 intersect_events(ray, events) per ray: sorted by t; events with equal t in scene order,
    // entry before exit (not the order the reference's std::sort happens to leave).
    std::vector<std::vector<PrimitiveHitEvent>> intersect_events(const std::vector<Ray>& rays) const {
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, 0.0f);
        std::vector<uint32_t> off(rays.size() + 1, 0u);
        uint64_t total = 0;
        vr_cpp::check(vr_query_events(ctx, r.data(), r.size(), off.data(), nullptr, nullptr, 0, &total));
        std::vector<float> t(total);
        std::vector<uint32_t> ev(total);
        if (total) vr_cpp::check(vr_query_events(ctx, r.data(), r.size(), off.data(), t.data(), ev.data(), total, &total));
        std::vector<std::vector<PrimitiveHitEvent>> out(rays.size());
        for (size_t i = 0; i < rays.size(); ++i) {
            out[i].reserve(off[i + 1] - off[i]);
            for (uint32_t k = off[i]; k < off[i + 1]; ++k) out[i].push_back(PrimitiveHitEvent{t[k], (ev[k] & 1u) != 0, ev[k] >> 1});
        }
        return out;
    }

    // gmm.h:98-126 evaluate_sigma(active, pos, sigma_a, sigma_s) per point, `active` being the Gaussians
    // whose 3-sigma ellipsoid holds the point; *n_active (if given) receives how many those are.
    void evaluate_sigma(const std::vector<Eigen::Vector3f>& pos, std::vector<float>& sigma_a, std::vector<float>& sigma_s,
                        std::vector<uint32_t>* n_active = nullptr) const {
        vr_ctx* ctx = ready();
        std::vector<float> xyz(3 * pos.size()), as(2 * pos.size());
        for (size_t i = 0; i < pos.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = pos[i][k];
        if (n_active) n_active->assign(pos.size(), 0u);
        vr_cpp::check(vr_query_sigma(ctx, xyz.data(), pos.size(), as.data(), n_active ? n_active->data() : nullptr));
        sigma_a.resize(pos.size());
        sigma_s.resize(pos.size());
        for (size_t i = 0; i < pos.size(); ++i) {
            sigma_a[i] = as[2 * i];
            sigma_s[i] = as[2 * i + 1];
        }
    }

    // The gradient of those sigmas with respect to the Gaussians (vr_query_sigma_grad): row g of the result (11 floats
    // per scene Gaussian) is sum_i (w_a d sigma_a + w_s d sigma_s)(pos_i) / d (mean[3], cov[6] = {xx, xy, xz, yy, yz, zz},
    // density, albedo), weights_as = (w_a, w_s) per point; an empty `weights_as` means (1, 1) for every point, the
    // gradient of sigma_t. *grad_pos (if given) receives 3 floats per point, the same weighted gradient with respect to
    // the point itself.
    std::vector<float> sigma_gradient(const std::vector<Eigen::Vector3f>& pos, const std::vector<float>& weights_as = {},
                                      std::vector<float>* grad_pos = nullptr) const {
        if (!weights_as.empty() && weights_as.size() != 2 * pos.size()) throw std::runtime_error("sigma_gradient: two weights per point");
        vr_ctx* ctx = ready();
        std::vector<float> xyz(3 * pos.size() + 1, 0.0f);  // (+ 1: never a NULL pointer)
        for (size_t i = 0; i < pos.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = pos[i][k];
        std::vector<float> grad(11 * scene_.get_num_primitives() + 1, 0.0f);
        if (grad_pos) grad_pos->assign(3 * pos.size(), 0.0f);
        vr_cpp::check(vr_query_sigma_grad(ctx, xyz.data(), weights_as.empty() ? nullptr : weights_as.data(), pos.size(), grad.data(),
                                          grad_pos && !pos.empty() ? grad_pos->data() : nullptr));
        grad.pop_back();
        return grad;
    }

    // The caller's own per-Gaussian vectors at points (vr_query_features): `features` holds C floats per scene Gaussian,
    // row g for Gaussian g. The result holds F row-major, pos.size() * C floats, F[i][c] = sum_g m_g(pos_i) features[g][c]
    // over evaluate_sigma's active set; *mass (if given) receives sum_g m_g(pos_i), *n_active the size of the set.
    std::vector<float> evaluate_features(const std::vector<Eigen::Vector3f>& pos, const std::vector<float>& features, uint32_t C,
                                         std::vector<float>* mass = nullptr, std::vector<uint32_t>* n_active = nullptr) const {
        feature_rows("evaluate_features", features.size(), C);
        vr_ctx* ctx = ready();
        std::vector<float> xyz(3 * pos.size()), out(pos.size() * C);
        for (size_t i = 0; i < pos.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = pos[i][k];
        if (mass) mass->assign(pos.size(), 0.0f);
        if (n_active) n_active->assign(pos.size(), 0u);
        vr_cpp::check(vr_query_features(ctx, xyz.data(), pos.size(), features.data(), C, out.data(), mass ? mass->data() : nullptr,
                                        n_active ? n_active->data() : nullptr));
        return out;
    }

    // The gradient of L = sum_i (sum_c weights[i][c] F[i][c] + weight_mass[i] mass[i]) for evaluate_features' F and mass
    // (vr_query_features_grad): row g of the result (10 floats per scene Gaussian, transmittance_gradient's layout) is
    // d L / d (mean[3], cov[6], density). An empty `weights` means 1 everywhere, an empty `weight_mass` 0. *grad_features
    // (if given) receives C floats per Gaussian, d L / d features; *grad_pos (if given) 3 floats per point, d L / d pos.
    std::vector<float> features_gradient(const std::vector<Eigen::Vector3f>& pos, const std::vector<float>& features, uint32_t C,
                                         const std::vector<float>& weights = {}, const std::vector<float>& weight_mass = {},
                                         std::vector<float>* grad_features = nullptr, std::vector<float>* grad_pos = nullptr) const {
        feature_rows("features_gradient", features.size(), C);
        if (!weights.empty() && weights.size() != pos.size() * C) throw std::runtime_error("features_gradient: C weights per point");
        if (!weight_mass.empty() && weight_mass.size() != pos.size()) throw std::runtime_error("features_gradient: one mass weight per point");
        vr_ctx* ctx = ready();
        std::vector<float> xyz(3 * pos.size() + 1, 0.0f);  // (+ 1: never a NULL pointer)
        for (size_t i = 0; i < pos.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = pos[i][k];
        std::vector<float> grad(10 * scene_.get_num_primitives() + 1, 0.0f);
        if (grad_features) grad_features->assign(features.size(), 0.0f);
        if (grad_pos) grad_pos->assign(3 * pos.size(), 0.0f);
        vr_cpp::check(vr_query_features_grad(ctx, xyz.data(), pos.size(), features.data(), C, weights.empty() ? nullptr : weights.data(),
                                             weight_mass.empty() ? nullptr : weight_mass.data(), grad.data(),
                                             grad_features && !features.empty() ? grad_features->data() : nullptr,
                                             grad_pos && !pos.empty() ? grad_pos->data() : nullptr));
        grad.pop_back();
        return grad;
    }

    // The emission-absorption sum along rays in one call (vr_query_radiance): `t` holds K distances shared by all rays, or
    // rays.size() * K, as for transmittance_profile; `features` C floats per scene Gaussian, as for evaluate_features; `q`
    // the quadrature weights in t's two layouts, or empty (all ones). The result holds L row-major, rays.size() * C floats,
    //   L[i][c] = sum_k q[i][k] Tr[i][k] sum_g m_g(x_ik) features[g][c],   x_ik = origin_i + t[i][k] * direction_i in f32,
    // over evaluate_sigma's active set at x_ik with Tr the profile's. *opacity (if given) receives the same sum without
    // the features, *tr the profile's Tr (rays.size() * K floats), *n_pairs the active (sample, Gaussian) pairs per ray.
    std::vector<float> radiance(const std::vector<Ray>& rays, const std::vector<float>& t, uint32_t K,
                                const std::vector<float>& features, uint32_t C, const std::vector<float>& q = {},
                                std::vector<float>* opacity = nullptr, std::vector<float>* tr = nullptr,
                                std::vector<uint32_t>* n_pairs = nullptr) const {
        const size_t stride = profile_stride("radiance", rays.size(), t.size(), K);
        const size_t q_stride = q.empty() ? 0 : profile_stride("radiance", rays.size(), q.size(), K);
        feature_rows("radiance", features.size(), C);
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, std::numeric_limits<float>::infinity());
        std::vector<float> out(r.size() * C), none(1, 0.0f);  // (none: a scene without Gaussians has no rows, never a NULL pointer)
        if (opacity) opacity->assign(r.size(), 0.0f);
        if (tr) tr->assign(r.size() * K, 0.0f);
        if (n_pairs) n_pairs->assign(r.size(), 0u);
        vr_cpp::check(vr_query_radiance(ctx, r.data(), t.data(), stride, q.empty() ? nullptr : q.data(), q_stride, r.size(), K,
                                        features.empty() ? none.data() : features.data(), C, out.data(),
                                        opacity ? opacity->data() : nullptr, tr ? tr->data() : nullptr,
                                        n_pairs ? n_pairs->data() : nullptr));
        return out;
    }

    // The gradient of l = sum_i (sum_c weights[i][c] L[i][c] + weight_opacity[i] opacity[i]) for radiance's L and opacity, in
    // one fused call (vr_query_radiance_grad): rays, t, K, features, C and q are radiance's; an empty `weights` means 1
    // everywhere, an empty `weight_opacity` 0. The transmittances are computed again (the bits radiance returns). Row g of
    // the result (10 floats per scene Gaussian, transmittance_gradient's layout and its moving_bounds) is d l / d (mean[3],
    // cov[6], density), the emission part and the part through the transmittances together. *grad_features (if given)
    // receives C floats per Gaussian, d l / d features; *grad_q and *grad_tau rays.size() * K floats each, d l / d q and
    // d l / d tau (the optical depth up to the sample).
    std::vector<float> radiance_gradient(const std::vector<Ray>& rays, const std::vector<float>& t, uint32_t K,
                                         const std::vector<float>& features, uint32_t C, const std::vector<float>& weights = {},
                                         const std::vector<float>& weight_opacity = {}, const std::vector<float>& q = {},
                                         bool moving_bounds = true, std::vector<float>* grad_features = nullptr,
                                         std::vector<float>* grad_q = nullptr, std::vector<float>* grad_tau = nullptr) const {
        const size_t stride = profile_stride("radiance_gradient", rays.size(), t.size(), K);
        const size_t q_stride = q.empty() ? 0 : profile_stride("radiance_gradient", rays.size(), q.size(), K);
        feature_rows("radiance_gradient", features.size(), C);
        if (!weights.empty() && weights.size() != rays.size() * C) throw std::runtime_error("radiance_gradient: C weights per ray");
        if (!weight_opacity.empty() && weight_opacity.size() != rays.size())
            throw std::runtime_error("radiance_gradient: one opacity weight per ray");
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, std::numeric_limits<float>::infinity());
        std::vector<float> grad(10 * scene_.get_num_primitives() + 1, 0.0f), none(1, 0.0f);  // (+ 1, none: never a NULL pointer)
        if (grad_features) grad_features->assign(features.size(), 0.0f);
        if (grad_q) grad_q->assign(r.size() * K, 0.0f);
        if (grad_tau) grad_tau->assign(r.size() * K, 0.0f);
        vr_cpp::check(vr_query_radiance_grad(ctx, r.data(), t.data(), stride, q.empty() ? nullptr : q.data(), q_stride, r.size(), K,
                                             features.empty() ? none.data() : features.data(), C,
                                             weights.empty() ? nullptr : weights.data(),
                                             weight_opacity.empty() ? nullptr : weight_opacity.data(), nullptr,
                                             moving_bounds ? 0u : (uint32_t)VR_GRAD_FROZEN_BOUNDS, grad.data(),
                                             grad_features && !features.empty() ? grad_features->data() : nullptr,
                                             grad_q && !r.empty() ? grad_q->data() : nullptr,
                                             grad_tau && !r.empty() ? grad_tau->data() : nullptr));
        grad.pop_back();
        return grad;
    }

    // integrator.h:422-498 MultiScatterGaussians::get_free_flight_distance(ray, events, target_tau) per ray, the
    // events being the ray's own: the collision distance, or -1 where the ray leaves the mixture before the
    // target is reached. *albedo (if given) receives evaluate_albedo (gmm.h:128-143) over the critical segment's
    // active Gaussians at the collision, *n_active how many those are (both 0 where t < 0).
    std::vector<float> query_free_flight(const std::vector<Ray>& rays, const std::vector<float>& target_tau,
                                         std::vector<float>* albedo = nullptr, std::vector<uint32_t>* n_active = nullptr) const {
        if (target_tau.size() != rays.size()) throw std::runtime_error("query_free_flight: one target_tau per ray");
        vr_ctx* ctx = ready();
        const std::vector<vr_ray> r = pack(rays, nullptr, 0.0f);
        std::vector<float> t(r.size());
        if (albedo) albedo->assign(r.size(), 0.0f);
        if (n_active) n_active->assign(r.size(), 0u);
        vr_cpp::check(vr_query_free_flight(ctx, r.data(), target_tau.data(), r.size(), t.data(), albedo ? albedo->data() : nullptr,
                                           n_active ? n_active->data() : nullptr));
        return t;
    }

private:
    // `features` holds C floats for each of the scene's Gaussians.
    void feature_rows(const char* what, size_t words, uint32_t C) const {
        if (C == 0 || C > VR_FEATURES_MAX_CHANNELS) throw std::runtime_error(std::string(what) + ": C must lie in [1, 64]");
        if (words != (size_t)scene_.get_num_primitives() * C) throw std::runtime_error(std::string(what) + ": C features per Gaussian");
    }
    // t of size K is one row shared by all rays (stride 0), of size n * K a row per ray (stride K).
    static size_t profile_stride(const char* what, size_t n, size_t nt, uint32_t K) {
        if (K == 0) throw std::runtime_error(std::string(what) + ": K must be positive");
        if (nt == n * K) return K;
        if (nt == K) return 0;
        throw std::runtime_error(std::string(what) + ": t holds K distances, or K per ray");
    }
    std::vector<float> transmittance(const std::vector<vr_ray>& r, std::vector<float>* tau) const {
        vr_ctx* ctx = ready();
        std::vector<float> tr(r.size());
        if (tau) tau->assign(r.size(), 0.0f);
        vr_cpp::check(vr_query_transmittance(ctx, r.data(), r.size(), tr.data(), tau ? tau->data() : nullptr));
        return tr;
    }
};
