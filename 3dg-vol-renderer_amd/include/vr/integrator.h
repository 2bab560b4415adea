// integrator.h — C++ mirror of the reference's include/integrator.h over the C ABI (include/vr_hip.h).
#pragma once
#include "camera.h"
#include "image.h"
#include "scene.h"
// ---------------------------------------------------------------------------------------------
// integrator.h:49-57 and the device integrators
// ---------------------------------------------------------------------------------------------
class Integrator {
protected:
    const std::shared_ptr<Camera> camera;

public:
    Integrator(const std::shared_ptr<Camera>& camera) : camera(camera) {}
    virtual ~Integrator() = default;
    virtual void render(const Scene& scene, Image& image) = 0;
};

// The device integrators render on every visible GPU by default, as the reference's render uses
// every CPU core (OpenMP): one GPU renders on its own; several split the frame's tiles and gather
// over RCCL (vr_init_multi). set_devices() picks the GPUs explicitly (a device
// listed more than once rehearses the split on one GPU); the `dev` constructor argument pins one GPU.
class HipIntegrator : public Integrator {
protected:
    vr_render_params params_{};
    int device_ = -1;            // >= 0: this one GPU
    std::vector<int> devices_;   // explicit device list (multi-GPU context, even for one device)
    int solver_ = -1;            // free-flight integrators: VR_OPT_FF_SOLVER set before each render

public:
    HipIntegrator(const std::shared_ptr<Camera>& camera, int integrator, float step_size, int env_samples, int dev)
        : Integrator(camera), device_(dev) {
        params_.integrator = integrator;
        params_.step_size = step_size;
        params_.env_samples = env_samples;
        params_.t_eps = 0.0f;
        params_.flags = 0;
    }
    void set_t_eps(float t) { params_.t_eps = t; }
    void set_devices(const std::vector<int>& devs) { devices_ = devs; }
    const vr_render_params& params() const { return params_; }
    vr_ctx* context() const {
        if (!devices_.empty()) return vr_cpp::device_group(devices_);
        if (device_ >= 0) return vr_cpp::device(device_);
        const int n = vr_cpp::device_count();
        if (n <= 1) return vr_cpp::device(0);
        std::vector<int> all(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        return vr_cpp::device_group(all);
    }
    void render(const Scene& scene, Image& image) override {
        vr_ctx* ctx = context();
        upload(ctx, scene);
        apply_solver(ctx);
        vr_cpp::check(vr_render(ctx, &camera->state(), &params_, image.get_width(), image.get_height(), image.data()));
    }
    // Radiance along the caller's own rays (vr_render_rays, include/vr_hip.h): `rays` is a W x H grid in row-major
    // order, rendered by the ray-march integrators exactly as a frame is, pixel (x, y) marching rays[y * W + x]
    // in place of the camera's ray (the integrator's camera is not read). A Ray's direction was normalised by its
    // constructor (ray.h:11-12): it goes to the device as it stands (unit = 1), as MixtureQuery passes its rays.
    // *transmittance (if given) receives the W * H transmittances left at the end of the primary marches. The
    // free-flight integrators throw (VR_ERR_UNSUPPORTED). Runs on the context's first device.
    void render_rays(const Scene& scene, const std::vector<Ray>& rays, uint32_t W, uint32_t H, Image& out,
                     std::vector<float>* transmittance = nullptr) {
        if (rays.size() != (size_t)W * H) throw std::runtime_error("render_rays: W * H rays expected");
        if (out.get_width() != W || out.get_height() != H) throw std::runtime_error("render_rays: the image is not W x H");
        std::vector<vr_ray> r(rays.size());
        for (size_t i = 0; i < rays.size(); ++i) {
            for (int k = 0; k < 3; ++k) {
                r[i].origin[k] = rays[i].origin[k];
                r[i].direction[k] = rays[i].direction[k];
            }
            r[i].tmax = 0.0f;
            r[i].unit = 1.0f;
        }
        vr_ctx* ctx = context();
        upload(ctx, scene);
        if (transmittance) transmittance->assign(rays.size(), 0.0f);
        vr_cpp::check(vr_render_rays(ctx, r.data(), W, H, &params_, out.data(), transmittance ? transmittance->data() : nullptr));
    }
    // re-upload when the scene (or the scene object) changed since the last upload to this context
    static void upload(vr_ctx* ctx, const Scene& scene) {
        vr_scene* ns = scene.native();
        std::lock_guard<std::mutex> lock(upload_mutex());
        auto& uploaded = upload_cache();
        auto it = uploaded.find(ctx);
        if (it == uploaded.end() || it->second.first != (const void*)ns || it->second.second != scene.native_version()) {
            vr_cpp::check(vr_upload_scene(ctx, ns));
            uploaded[ctx] = {ns, scene.native_version()};
        }
    }
    // A Gaussian scene straight from device memory (vr_upload_gaussians_device, include/vr_hip.h): d_mean (3 n),
    // d_cov6 (6 n), d_density (n), d_albedo (n) on the context's GPU, lights and env_color (nullptr: the default) on
    // the host. The upload cache forgets the context, so it cannot mistake its scene for a host one: the next
    // render(scene, ...) uploads `scene` again, and render_uploaded() renders what this call put there.
    static void upload_device(vr_ctx* ctx, const float* d_mean, const float* d_cov6, const float* d_density, const float* d_albedo,
                              size_t n, const vr_light* lights = nullptr, size_t n_lights = 0, const float* env_color = nullptr) {
        vr_status st = vr_upload_gaussians_device(ctx, d_mean, d_cov6, d_density, d_albedo, n, lights, n_lights, env_color);
        forget(ctx);
        vr_cpp::check(st);
    }
    // render() of the scene the context holds (upload_device's), without an upload
    void render_uploaded(Image& image) {
        vr_ctx* ctx = context();
        apply_solver(ctx);
        vr_cpp::check(vr_render(ctx, &camera->state(), &params_, image.get_width(), image.get_height(), image.data()));
    }
    void apply_solver(vr_ctx* ctx) const {
        if (solver_ >= 0) vr_cpp::check(vr_set_option(ctx, VR_OPT_FF_SOLVER, solver_));
    }
    // a context's scene was replaced behind upload()'s back (vr_sfd_optimize re-uploads): forget it
    static void forget(vr_ctx* ctx) {
        std::lock_guard<std::mutex> lock(upload_mutex());
        upload_cache().erase(ctx);
    }

private:
    static std::mutex& upload_mutex() {
        static std::mutex mu;
        return mu;
    }
    static std::map<vr_ctx*, std::pair<const void*, uint64_t>>& upload_cache() {  // per device context
        static std::map<vr_ctx*, std::pair<const void*, uint64_t>> uploaded;
        return uploaded;
    }

public:
    vr_render_stats stats() const {
        vr_render_stats s{};
        vr_cpp::check(vr_get_stats(context(), &s));
        return s;
    }
};

// integrator.h:100-142 — PureRayMarching(camera, step_size = 0.01, env_samples = 20)
class PureRayMarching : public HipIntegrator {
public:
    PureRayMarching(const std::shared_ptr<Camera>& camera, float step_size = 0.01f, int env_samples = 20, int dev = -1)
        : HipIntegrator(camera, VR_PURE_RAYMARCH, step_size, env_samples, dev) {}
};

// distance_solvers.h:143-147: the reference picks one of these with a #define (ANALYTIC_PLUS_NEWTON
// compiled in); here a run-time choice per free-flight integrator (VR_OPT_FF_SOLVER). UNIFORM draws
// from a seeded PCG32 stream instead of rand01()'s random_device (include/vr_hip.h).
enum DistanceSolver { ANALYTIC_PLUS_NEWTON = 0, BISECTION = 1, NEWTON = 2, ANALYTIC_PLUS_BISECTION = 3, UNIFORM = 4 };

// integrator.h:273-408 — FreeFlightGaussians(camera, num_samples = 256)
class FreeFlightGaussians : public HipIntegrator {
public:
    FreeFlightGaussians(const std::shared_ptr<Camera>& camera, int num_samples = 256, int dev = -1)
        : HipIntegrator(camera, VR_FREE_FLIGHT, 0.01f, 0, dev) {
        params_.num_samples = num_samples;
        solver_ = ANALYTIC_PLUS_NEWTON;
    }
    void set_distance_solver(DistanceSolver s) { solver_ = (int)s; }
};

// integrator.h:416-720 — MultiScatterGaussians(camera, samples = 16, min_bounces = 5)
class MultiScatterGaussians : public HipIntegrator {
public:
    MultiScatterGaussians(const std::shared_ptr<Camera>& camera, int samples = 16, int min_bounces = 5, int dev = -1)
        : HipIntegrator(camera, VR_MULTI_SCATTER, 0.01f, 0, dev) {
        params_.num_samples = samples;
        params_.min_bounces = min_bounces;
        solver_ = ANALYTIC_PLUS_NEWTON;
    }
    void set_num_samples(int n) { params_.num_samples = n; }  // integrator.h:719
    void set_distance_solver(DistanceSolver s) { solver_ = (int)s; }
    using HipIntegrator::render;
    // integrator.h:532-536 with RECORD_PIXEL_GAUSSIANS: per_pixel_gaussians[y * W + x] receives the
    // sorted indices of the Gaussians recorded at that pixel (integrator.h:616-644, 700-705).
    void render(const Scene& scene, Image& image, std::vector<std::vector<uint32_t>>* per_pixel_gaussians) {
        if (!per_pixel_gaussians) return render(scene, image);
        vr_ctx* ctx = context();
        upload(ctx, scene);
        apply_solver(ctx);
        vr_cpp::check(vr_render_record(ctx, &camera->state(), &params_, image.get_width(), image.get_height(), image.data(), 0));
        const size_t npix = (size_t)image.get_width() * image.get_height(), n = scene.get_num_primitives();
        const size_t words = (n + 31) / 32;
        std::vector<uint32_t> bits(words * npix);
        vr_cpp::check(vr_get_pixel_gaussians(ctx, 0, bits.data(), bits.size()));
        per_pixel_gaussians->assign(npix, {});
        for (size_t w = 0; w < words; ++w)
            for (size_t p = 0; p < npix; ++p)
                for (uint32_t b = bits[w * npix + p]; b; b &= b - 1)
                    (*per_pixel_gaussians)[p].push_back((uint32_t)(32 * w + __builtin_ctz(b)));
    }
    int num_samples() const { return params_.num_samples; }
};

// integrator.h:65-94 — TestIntegrator(camera)
class TestIntegrator : public HipIntegrator {
public:
    TestIntegrator(const std::shared_ptr<Camera>& camera, int dev = -1)
        : HipIntegrator(camera, VR_TEST_HITMASK, 0.01f, 0, dev) {}
};

