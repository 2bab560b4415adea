// vol_render: command-line renderer over the C++ host API (the role of the reference's
// tests/main.cpp, which hard-codes scene, camera and integrator; here they are arguments).
//
//   vol_render --scene scenes/many_gaussians.txt [--spheres] [--xml] [--size 512x512]
//              [--integrator gaussians|pure|spheres|test|freeflight|multiscatter] [--step 0.01] [--env 20]
//              [--spp N] (free-flight paths per pixel; main.cpp:42 renders MultiScatterGaussians at 256)
//              [--camera pinhole|ortho] [--pos 0,1,6] [--lookat 0,1,0] [--fov 0.785398]
//              [--out output.ppm] [--dump-rays N] [--devices 0,1,...]
//
// --record (multiscatter): the 3-argument render with per-pixel Gaussian lists (RECORD_PIXEL_GAUSSIANS);
// prints the number of recorded (pixel, Gaussian) pairs.
// --inverse N --ref I_ref.ppm [--seed S] [--stoch K] [--lr X] [--final-spp F] [--sfd-out DIR]: N iterations
// of StochasticFiniteDiffInverseIntegrator from --scene towards I_ref (MultiScatterGaussians at --spp);
// prints every iteration's mean loss (the reference's tests/main.cpp inverse mode, main.cpp:48-75).
// --gif out.gif [--frames 120] [--fps 30]: the reference driver's turntable (main.cpp:81-114): an
// Orthographic_Camera orbiting the look-at point at radius 6 and height +1, RayMarchingGaussians
// (step 0.01, --env samples), one GIF frame each.
// --devices renders on a multi-GPU context over exactly these GPUs (tiles split, RCCL gather); by
// default every visible GPU is used (one GPU: a plain single-device context).
// --dump-rays N prints the first N primary rays (host only, no GPU) — used by the CPU tests.
// --query RAYS.bin runs the mixture queries of vr/query.h (MixtureQuery: transmittance_up_to,
// intersect_events, evaluate_sigma, then query_free_flight aimed at half of each ray's optical depth) on the scene
// and prints every result with the bits of its floats. The
// file: uint32 n_rays, uint32 n_points, then n_rays rows of 7 floats (origin, direction, tmax; the direction
// is normalised by Ray's constructor), then n_points rows of 3 floats.
// --query-grad RAYS.bin (the same file) prints MixtureQuery::transmittance_gradient of the file's rays, all weights 1:
// one line `tg <scene index> <10 hex words>` per Gaussian (d/d mean[3], cov[6], density).
// --query-ray-grad RAYS.bin (the same file) prints MixtureQuery::transmittance_ray_gradient of the file's rays: one line
// `rg <ray index> <8 hex words>` per ray (d/d origin[3], d/d tmax, d/d direction[3], tau).
// --query-sigma-grad RAYS.bin (the same file) prints MixtureQuery::sigma_gradient at the file's points, all weights (1, 1):
// one line `sg <scene index> <11 hex words>` per Gaussian (d/d mean[3], cov[6], density, albedo), then one line
// `sx <point index> <3 hex words>` per point (the gradient with respect to the point).
// --query-features RAYS.bin FEATURES.bin (FEATURES.bin: uint32 N, uint32 C, then N rows of C floats, row g for scene Gaussian
// g) prints MixtureQuery::evaluate_features at the first file's points: one line `fq <point index> <n_active> <mass and C
// channels as hex words>` per point; then MixtureQuery::features_gradient there, all weights 1 and mass weights 0: one line
// `fg <scene index> <10 hex words>` per Gaussian, one line `fr <scene index> <C hex words>` per Gaussian (the gradient with
// respect to its row), one line `fx <point index> <3 hex words>` per point.
// --query-profile RAYS.bin K (the same file) prints MixtureQuery::transmittance_profile of the file's rays at K distances
// per ray, t[i][k] = tmax_i * (k + 1) / K in f32: one line `tp <ray index> <k> <t, Tr, tau as hex words>` per sample, then
// MixtureQuery::transmittance_profile_gradient of the same samples, all weights 1: one line `pg <scene index> <10 hex
// words>` per Gaussian.
// --query-radiance RAYS.bin K FEATURES.bin (the two files above) prints MixtureQuery::radiance of the file's rays at
// --query-profile's K distances per ray with the quadrature weights q[i][k] = tmax_i / K in f32: one line `rq <ray index>
// <n_pairs> <opacity and C channels as hex words>` per ray, then one line `rt <ray index> <K hex words of Tr>` per ray.
// --query-radiance-grad RAYS.bin K FEATURES.bin (the same files, samples and q) prints MixtureQuery::radiance_gradient with all
// weights 1 and opacity weights 0: one line `Rg <scene index> <10 hex words>` per Gaussian, one line `Rf <scene index> <C hex
// words>` per Gaussian (the gradient with respect to its row), then per ray one line `Rq <ray index> <K hex words>` (d/d q)
// and one line `Rt <ray index> <K hex words>` (d/d tau).
// --upload-device (Gaussian scenes, one GPU): copies the loaded scene's rows to device memory and uploads them with
// HipIntegrator::upload_device (vr_upload_gaussians_device: records, boxes and tree computed on the device), then
// renders the scene the context holds.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <cmath>
#include <numbers>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "vr/integrator.h"
#include "vr/query.h"
#include "vr/gif.h"
#include "vr/inverse_integrator.h"
#include "vr/test_integrators.h"

static uint32_t fbits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static void read_query_file(const std::string& path, std::vector<Ray>& rays, std::vector<float>& tmax,
                            std::vector<Eigen::Vector3f>& pos) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    uint32_t hdr[2] = {0, 0};
    bool ok = std::fread(hdr, 4, 2, f) == 2;
    std::vector<float> rows(ok ? 7 * (size_t)hdr[0] : 0), pts(ok ? 3 * (size_t)hdr[1] : 0);
    ok = ok && std::fread(rows.data(), 4, rows.size(), f) == rows.size() && std::fread(pts.data(), 4, pts.size(), f) == pts.size();
    std::fclose(f);
    if (!ok) throw std::runtime_error("short query file " + path);
    for (uint32_t i = 0; i < hdr[0]; ++i) {
        const float* r = &rows[7 * (size_t)i];
        rays.emplace_back(Eigen::Vector3f(r[0], r[1], r[2]), Eigen::Vector3f(r[3], r[4], r[5]));
        tmax.push_back(r[6]);
    }
    for (uint32_t i = 0; i < hdr[1]; ++i) pos.emplace_back(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
}

static int run_queries(const Scene& scene, const std::string& path) {
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    MixtureQuery q(scene);
    std::vector<float> tau;
    const std::vector<float> tr = q.transmittance_up_to(rays, tmax, &tau);
    for (size_t i = 0; i < tr.size(); ++i) std::printf("tr %zu %08x %08x\n", i, fbits(tr[i]), fbits(tau[i]));
    const auto events = q.intersect_events(rays);
    for (size_t i = 0; i < events.size(); ++i)
        for (const PrimitiveHitEvent& e : events[i]) std::printf("ev %zu %08x %zu %d\n", i, fbits(e.t), e.index, e.entering ? 1 : 0);
    std::vector<float> sa, ss;
    std::vector<uint32_t> na;
    q.evaluate_sigma(pos, sa, ss, &na);
    for (size_t i = 0; i < sa.size(); ++i) std::printf("sigma %zu %08x %08x %u\n", i, fbits(sa[i]), fbits(ss[i]), na[i]);
    // one free-flight step per ray, aimed at half the optical depth the ray has up to its tmax
    std::vector<float> target(tau.size()), albedo;
    for (size_t i = 0; i < tau.size(); ++i) target[i] = 0.5f * tau[i];
    std::vector<uint32_t> nf;
    const std::vector<float> tf = q.query_free_flight(rays, target, &albedo, &nf);
    for (size_t i = 0; i < tf.size(); ++i) std::printf("ff %zu %08x %08x %08x %u\n", i, fbits(target[i]), fbits(tf[i]), fbits(albedo[i]), nf[i]);
    return 0;
}

// --query-grad: the optical-depth gradient of the file's rays (their tmax; all weights 1), one line per Gaussian.
static int run_query_grad(const Scene& scene, const std::string& path) {
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    const std::vector<float> g = MixtureQuery(scene).transmittance_gradient(rays, tmax);
    for (size_t i = 0; i < g.size() / 10; ++i) {
        std::printf("tg %zu", i);
        for (int k = 0; k < 10; ++k) std::printf(" %08x", fbits(g[10 * i + k]));
        std::printf("\n");
    }
    return 0;
}

// --query-ray-grad: the optical depth of the file's rays (their tmax) and its gradient with respect to each ray.
static int run_query_ray_grad(const Scene& scene, const std::string& path) {
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    const std::vector<vr_ray_grad> g = MixtureQuery(scene).transmittance_ray_gradient(rays, tmax);
    for (size_t i = 0; i < g.size(); ++i) {
        const float row[8] = {g[i].origin[0], g[i].origin[1], g[i].origin[2], g[i].tmax,
                              g[i].direction[0], g[i].direction[1], g[i].direction[2], g[i].tau};
        std::printf("rg %zu", i);
        for (int k = 0; k < 8; ++k) std::printf(" %08x", fbits(row[k]));
        std::printf("\n");
    }
    return 0;
}

// --query-sigma-grad: the gradient of sigma_t at the file's points, per Gaussian and per point.
static int run_query_sigma_grad(const Scene& scene, const std::string& path) {
    std::vector<Ray> rays;
    std::vector<float> tmax, gx;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    const std::vector<float> g = MixtureQuery(scene).sigma_gradient(pos, {}, &gx);
    for (size_t i = 0; i < g.size() / 11; ++i) {
        std::printf("sg %zu", i);
        for (int k = 0; k < 11; ++k) std::printf(" %08x", fbits(g[11 * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < gx.size() / 3; ++i)
        std::printf("sx %zu %08x %08x %08x\n", i, fbits(gx[3 * i]), fbits(gx[3 * i + 1]), fbits(gx[3 * i + 2]));
    return 0;
}

// FEATURES.bin: the rows, and C.
static std::vector<float> read_feature_file(const std::string& feat_path, uint32_t& C) {
    std::FILE* f = std::fopen(feat_path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + feat_path);
    uint32_t hdr[2] = {0, 0};
    bool ok = std::fread(hdr, 4, 2, f) == 2 && hdr[1] >= 1 && hdr[1] <= VR_FEATURES_MAX_CHANNELS;
    std::vector<float> feat(ok ? (size_t)hdr[0] * hdr[1] : 0);
    ok = ok && std::fread(feat.data(), 4, feat.size(), f) == feat.size();
    std::fclose(f);
    if (!ok) throw std::runtime_error("short or malformed feature file " + feat_path);
    C = hdr[1];
    return feat;
}

// --query-features: the caller's rows at the file's points, and the gradient of the sum of the result's entries.
static int run_query_features(const Scene& scene, const std::string& path, const std::string& feat_path) {
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    uint32_t C = 0;
    const std::vector<float> feat = read_feature_file(feat_path, C);
    MixtureQuery q(scene);
    std::vector<float> mass, gf, gx;
    std::vector<uint32_t> na;
    const std::vector<float> F = q.evaluate_features(pos, feat, C, &mass, &na);
    for (size_t i = 0; i < pos.size(); ++i) {
        std::printf("fq %zu %u %08x", i, na[i], fbits(mass[i]));
        for (uint32_t k = 0; k < C; ++k) std::printf(" %08x", fbits(F[C * i + k]));
        std::printf("\n");
    }
    const std::vector<float> g = q.features_gradient(pos, feat, C, {}, {}, &gf, &gx);
    for (size_t i = 0; i < g.size() / 10; ++i) {
        std::printf("fg %zu", i);
        for (int k = 0; k < 10; ++k) std::printf(" %08x", fbits(g[10 * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < gf.size() / C; ++i) {
        std::printf("fr %zu", i);
        for (uint32_t k = 0; k < C; ++k) std::printf(" %08x", fbits(gf[C * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < gx.size() / 3; ++i)
        std::printf("fx %zu %08x %08x %08x\n", i, fbits(gx[3 * i]), fbits(gx[3 * i + 1]), fbits(gx[3 * i + 2]));
    return 0;
}

// --query-profile: tau and Tr at K distances up to each ray's tmax, and the gradient of the sum of those optical depths.
static int run_query_profile(const Scene& scene, const std::string& path, int K) {
    if (K <= 0) throw std::runtime_error("--query-profile: K must be positive");
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    std::vector<float> t(rays.size() * (size_t)K), tau;
    for (size_t i = 0; i < rays.size(); ++i)
        for (int k = 0; k < K; ++k) t[i * (size_t)K + k] = tmax[i] * (float)(k + 1) / (float)K;
    const MixtureQuery q(scene);
    const std::vector<float> tr = q.transmittance_profile(rays, t, (uint32_t)K, &tau);
    for (size_t i = 0; i < tr.size(); ++i)
        std::printf("tp %zu %zu %08x %08x %08x\n", i / (size_t)K, i % (size_t)K, fbits(t[i]), fbits(tr[i]), fbits(tau[i]));
    const std::vector<float> g = q.transmittance_profile_gradient(rays, t, (uint32_t)K);
    for (size_t i = 0; i < g.size() / 10; ++i) {
        std::printf("pg %zu", i);
        for (int k = 0; k < 10; ++k) std::printf(" %08x", fbits(g[10 * i + k]));
        std::printf("\n");
    }
    return 0;
}

// --query-radiance: the emission-absorption sum of the file's rays over --query-profile's samples, in one call.
static int run_query_radiance(const Scene& scene, const std::string& path, int K, const std::string& feat_path) {
    if (K <= 0) throw std::runtime_error("--query-radiance: K must be positive");
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    uint32_t C = 0;
    const std::vector<float> feat = read_feature_file(feat_path, C);
    std::vector<float> t(rays.size() * (size_t)K), q(t.size()), opacity, tr;
    for (size_t i = 0; i < rays.size(); ++i)
        for (int k = 0; k < K; ++k) {
            t[i * (size_t)K + k] = tmax[i] * (float)(k + 1) / (float)K;
            q[i * (size_t)K + k] = tmax[i] / (float)K;
        }
    std::vector<uint32_t> np;
    const std::vector<float> L = MixtureQuery(scene).radiance(rays, t, (uint32_t)K, feat, C, q, &opacity, &tr, &np);
    for (size_t i = 0; i < rays.size(); ++i) {
        std::printf("rq %zu %u %08x", i, np[i], fbits(opacity[i]));
        for (uint32_t k = 0; k < C; ++k) std::printf(" %08x", fbits(L[C * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < rays.size(); ++i) {
        std::printf("rt %zu", i);
        for (int k = 0; k < K; ++k) std::printf(" %08x", fbits(tr[i * (size_t)K + k]));
        std::printf("\n");
    }
    return 0;
}

// --query-radiance-grad: the fused gradient of the sum of --query-radiance's channels, over the same samples and weights.
static int run_query_radiance_grad(const Scene& scene, const std::string& path, int K, const std::string& feat_path) {
    if (K <= 0) throw std::runtime_error("--query-radiance-grad: K must be positive");
    std::vector<Ray> rays;
    std::vector<float> tmax;
    std::vector<Eigen::Vector3f> pos;
    read_query_file(path, rays, tmax, pos);
    uint32_t C = 0;
    const std::vector<float> feat = read_feature_file(feat_path, C);
    std::vector<float> t(rays.size() * (size_t)K), q(t.size()), gf, gq, gt;
    for (size_t i = 0; i < rays.size(); ++i)
        for (int k = 0; k < K; ++k) {
            t[i * (size_t)K + k] = tmax[i] * (float)(k + 1) / (float)K;
            q[i * (size_t)K + k] = tmax[i] / (float)K;
        }
    const std::vector<float> g = MixtureQuery(scene).radiance_gradient(rays, t, (uint32_t)K, feat, C, {}, {}, q, true, &gf, &gq, &gt);
    for (size_t i = 0; i < g.size() / 10; ++i) {
        std::printf("Rg %zu", i);
        for (int k = 0; k < 10; ++k) std::printf(" %08x", fbits(g[10 * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < gf.size() / C; ++i) {
        std::printf("Rf %zu", i);
        for (uint32_t k = 0; k < C; ++k) std::printf(" %08x", fbits(gf[C * i + k]));
        std::printf("\n");
    }
    for (size_t i = 0; i < rays.size(); ++i) {
        std::printf("Rq %zu", i);
        for (int k = 0; k < K; ++k) std::printf(" %08x", fbits(gq[i * (size_t)K + k]));
        std::printf("\nRt %zu", i);
        for (int k = 0; k < K; ++k) std::printf(" %08x", fbits(gt[i * (size_t)K + k]));
        std::printf("\n");
    }
    return 0;
}

// --upload-device: the scene's rows as four device arrays, uploaded from there.
static void upload_from_device_memory(vr_ctx* ctx, const Scene& scene) {
    if (scene.volume_type != Scene::VolumeType::GAUSSIANS) throw std::runtime_error("--upload-device needs a Gaussian scene");
    std::vector<float> host[4];  // mean, cov6, density, albedo
    if (scene.gmm && !scene.gmm->empty())
        for (const Gaussian& x : (*scene.gmm)[0].gaussians) {
            const vr_gaussian g = x.to_record();
            host[0].insert(host[0].end(), g.mean, g.mean + 3);
            host[1].insert(host[1].end(), g.cov, g.cov + 6);
            host[2].push_back(g.density);
            host[3].push_back(g.albedo);
        }
    const size_t n = host[2].size();
    float* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto release = [&] {
        for (float* p : dev)
            if (p) (void)hipFree(p);
    };
    for (int k = 0; k < 4 && n > 0; ++k)
        if (hipMalloc((void**)&dev[k], host[k].size() * sizeof(float)) != hipSuccess ||
            hipMemcpy(dev[k], host[k].data(), host[k].size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            release();
            throw std::runtime_error("--upload-device: could not copy the scene to the device");
        }
    std::vector<vr_light> ls;
    for (const Light& l : scene.lights)
        ls.push_back(vr_light{{l.position[0], l.position[1], l.position[2]}, {l.intensity[0], l.intensity[1], l.intensity[2]}});
    const float env[3] = {scene.env_color[0], scene.env_color[1], scene.env_color[2]};
    try {
        HipIntegrator::upload_device(ctx, dev[0], dev[1], dev[2], dev[3], n, ls.data(), ls.size(), env);
    } catch (...) {
        release();
        throw;
    }
    release();
}

static Eigen::Vector3f parse3(const char* s) {
    float a = 0, b = 0, c = 0;
    if (std::sscanf(s, "%f,%f,%f", &a, &b, &c) != 3) throw std::runtime_error(std::string("bad vector: ") + s);
    return Eigen::Vector3f(a, b, c);
}

int main(int argc, char** argv) try {
    std::string scene_path, out = "output.ppm", integ = "gaussians", cam_type = "pinhole";
    bool spheres = false, xml = false;
    unsigned W = 512, H = 512;
    float step = 0.01f, fov = 0.25f * std::numbers::pi_v<float>;
    int env = -1, dump = 0, spp = -1;
    std::vector<int> devices;
    bool record = false, upload_device = false;
    int inverse = 0, stoch = 4, final_spp = 0;
    uint64_t seed = 0;
    float lr = 1e-2f;
    std::string ref_path, sfd_out, gif_path, query_path, query_grad_path, query_ray_grad_path, query_sigma_grad_path, query_profile_path,
        query_features_path, features_path, query_radiance_path, query_radiance_grad_path;
    int radiance_k = 0;
    int profile_k = 0;
    int frames = 120;
    float fps = 30.0f;
    Eigen::Vector3f pos(0, 1, 6), lookat(0, 1, 0);
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + a);
            return argv[++i];
        };
        if (a == "--scene") scene_path = next();
        else if (a == "--spheres") spheres = true;
        else if (a == "--xml") xml = true;
        else if (a == "--size") { if (std::sscanf(next(), "%ux%u", &W, &H) != 2) throw std::runtime_error("bad --size"); }
        else if (a == "--integrator") integ = next();
        else if (a == "--spp") spp = std::stoi(next());
        else if (a == "--step") step = std::strtof(next(), nullptr);
        else if (a == "--env") env = std::atoi(next());
        else if (a == "--camera") cam_type = next();
        else if (a == "--pos") pos = parse3(next());
        else if (a == "--lookat") lookat = parse3(next());
        else if (a == "--fov") fov = std::strtof(next(), nullptr);
        else if (a == "--out") out = next();
        else if (a == "--dump-rays") dump = std::atoi(next());
        else if (a == "--record") record = true;
        else if (a == "--upload-device") upload_device = true;
        else if (a == "--query") query_path = next();
        else if (a == "--query-grad") query_grad_path = next();
        else if (a == "--query-ray-grad") query_ray_grad_path = next();
        else if (a == "--query-sigma-grad") query_sigma_grad_path = next();
        else if (a == "--query-features") { query_features_path = next(); features_path = next(); }
        else if (a == "--query-radiance") { query_radiance_path = next(); radiance_k = std::atoi(next()); features_path = next(); }
        else if (a == "--query-radiance-grad") { query_radiance_grad_path = next(); radiance_k = std::atoi(next()); features_path = next(); }
        else if (a == "--query-profile") { query_profile_path = next(); profile_k = std::atoi(next()); }
        else if (a == "--gif") gif_path = next();
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--fps") fps = std::strtof(next(), nullptr);
        else if (a == "--inverse") inverse = std::atoi(next());
        else if (a == "--ref") ref_path = next();
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--stoch") stoch = std::atoi(next());
        else if (a == "--lr") lr = std::strtof(next(), nullptr);
        else if (a == "--final-spp") final_spp = std::atoi(next());
        else if (a == "--sfd-out") sfd_out = next();
        else if (a == "--devices") {
            std::string v = next();
            for (size_t p = 0; p <= v.size();) {
                size_t q = v.find(',', p);
                if (q == std::string::npos) q = v.size();
                devices.push_back(std::stoi(v.substr(p, q - p)));
                p = q + 1;
            }
        }
        else throw std::runtime_error("unknown argument " + a);
    }
    if (scene_path.empty()) throw std::runtime_error("--scene is required");

    std::shared_ptr<Camera> camera;
    Scene scene;
    vr_render_params xml_params{};
    if (xml) {
        vr_camera st{};
        uint32_t w = 0, h = 0;
        scene = Scene::load_XML(scene_path, &st, &w, &h, &xml_params);
        camera = std::make_shared<State_Camera>(st);
        W = w;
        H = h;
        integ = xml_params.integrator == VR_RAYMARCH_SPHERES ? "spheres" : "gaussians";
        if (env < 0) env = xml_params.env_samples;
        step = xml_params.step_size;
    } else {
        scene = spheres ? Scene::load_SMM(scene_path) : Scene::load_GMM(scene_path);
        Eigen::Vector3f view_dir = (lookat - pos).normalized();
        if (cam_type == "ortho") camera = std::make_shared<Orthographic_Camera>(pos, view_dir);
        else camera = std::make_shared<Pinhole_Camera>(pos, view_dir, fov);
    }
    std::printf("scene: %zu primitives, %zu lights\n", scene.get_num_primitives(), scene.lights.size());

    if (dump > 0) {  // host-only: primary rays through pixel centres, row-major
        for (int k = 0; k < dump; ++k) {
            unsigned x = k % W, y = k / W;
            Eigen::Vector2d uv((x + 0.5) / W, (y + 0.5) / H);
            Ray r = camera->sample_ray(uv);
            std::printf("ray %u %u %.9g %.9g %.9g %.9g %.9g %.9g\n", x, y, r.origin.x(), r.origin.y(), r.origin.z(),
                        r.direction.x(), r.direction.y(), r.direction.z());
        }
        return 0;
    }

    if (!query_path.empty()) return run_queries(scene, query_path);
    if (!query_grad_path.empty()) return run_query_grad(scene, query_grad_path);
    if (!query_ray_grad_path.empty()) return run_query_ray_grad(scene, query_ray_grad_path);
    if (!query_sigma_grad_path.empty()) return run_query_sigma_grad(scene, query_sigma_grad_path);
    if (!query_features_path.empty()) return run_query_features(scene, query_features_path, features_path);
    if (!query_radiance_path.empty()) return run_query_radiance(scene, query_radiance_path, radiance_k, features_path);
    if (!query_radiance_grad_path.empty()) return run_query_radiance_grad(scene, query_radiance_grad_path, radiance_k, features_path);
    if (!query_profile_path.empty()) return run_query_profile(scene, query_profile_path, profile_k);

    if (!gif_path.empty()) {  // main.cpp:81-114
        const float radius = 6.0f, height_pos = 1.0f;
        GifWriter gif;
        if (!GifBegin(&gif, gif_path.c_str(), W, H, (uint32_t)(100.0f / fps))) throw std::runtime_error(vr_last_error());
        for (int frame = 0; frame < frames; ++frame) {
            const float angle = 2.0f * std::numbers::pi_v<float> * ((float)frame / (float)frames);
            Eigen::Vector3f cpos = lookat + Eigen::Vector3f(radius * std::sin(angle), height_pos, radius * std::cos(angle));
            Eigen::Vector3f vd = (lookat - cpos).normalized();
            auto cam = std::make_shared<Orthographic_Camera>(cpos, vd);
            RayMarchingGaussians rm(cam, step, env < 0 ? 20 : env);
            if (!devices.empty()) rm.set_devices(devices);
            Image image(W, H);
            rm.render(scene, image);
            auto rgba = image.get_rgba_buffer();
            if (!GifWriteFrame(&gif, rgba.data(), W, H, (uint32_t)(100.0f / fps))) throw std::runtime_error(vr_last_error());
            std::printf("Frame %d / %d complete.\n", frame + 1, frames);
        }
        if (!GifEnd(&gif)) throw std::runtime_error(vr_last_error());
        std::printf("GIF saved.\n");
        return 0;
    }

    std::unique_ptr<HipIntegrator> integrator;
    if (integ == "gaussians") integrator = std::make_unique<RayMarchingGaussians>(camera, step, env < 0 ? 20 : env);
    else if (integ == "spheres") integrator = std::make_unique<RayMarchingSpheres>(camera, step, env < 0 ? 5 : env);
    else if (integ == "pure") integrator = std::make_unique<PureRayMarching>(camera, step, env < 0 ? 20 : env);
    else if (integ == "test") integrator = std::make_unique<TestIntegrator>(camera);
    else if (integ == "freeflight") integrator = std::make_unique<FreeFlightGaussians>(camera, spp < 0 ? 256 : spp);
    else if (integ == "multiscatter") integrator = std::make_unique<MultiScatterGaussians>(camera, spp < 0 ? 16 : spp);
    else throw std::runtime_error("unknown integrator " + integ);

    if (!devices.empty()) integrator->set_devices(devices);
    if (inverse > 0) {  // main.cpp:48-75: optimise the scene towards a reference image
        if (integ != "multiscatter") throw std::runtime_error("--inverse needs --integrator multiscatter");
        Image I_ref(ref_path);
        auto fwd = std::make_shared<MultiScatterGaussians>(camera, spp < 0 ? 16 : spp);
        if (!devices.empty()) fwd->set_devices(devices);
        SFDDConfig cfg;
        cfg.max_iters = inverse;
        cfg.num_stoch_samples = stoch;
        cfg.lr = lr;
        cfg.seed = seed;
        cfg.final_samples = final_spp;
        cfg.out_dir = sfd_out;
        StochasticFiniteDiffInverseIntegrator sfd(camera, fwd, cfg);
        if (!sfd.optimize(scene, I_ref)) throw std::runtime_error("SFD optimisation failed");
        for (size_t i = 0; i < sfd.loss_history().size(); ++i) std::printf("sfd iter %zu loss %.17g\n", i, sfd.loss_history()[i]);
        if (final_spp > 0) std::printf("sfd final loss %.17g\n", sfd.final_loss());
        return 0;
    }
    Image image(W, H);
    auto t0 = std::chrono::high_resolution_clock::now();
    if (record) {
        auto* ms = dynamic_cast<MultiScatterGaussians*>(integrator.get());
        if (!ms) throw std::runtime_error("--record needs --integrator multiscatter");
        std::vector<std::vector<uint32_t>> per_pixel;
        ms->render(scene, image, &per_pixel);
        size_t pairs = 0;
        for (const auto& l : per_pixel) pairs += l.size();
        std::printf("recorded pairs %zu\n", pairs);
    } else if (upload_device) {
        upload_from_device_memory(integrator->context(), scene);
        integrator->render_uploaded(image);
    } else {
        integrator->render(scene, image);
    }
    auto t1 = std::chrono::high_resolution_clock::now();
    vr_render_stats st = integrator->stats();
    std::printf("Render time: %.6f seconds (device %.3f ms, %lld pixels, %lld fallback, %d device(s)%s)\n",
                std::chrono::duration<double>(t1 - t0).count(), st.kernel_ms, (long long)st.pixels,
                (long long)st.fallback_pixels, vr_ctx_num_devices(integrator->context()),
                !vr_ctx_uses_rccl(integrator->context()) ? ""
                : vr_ctx_num_devices(integrator->context()) > 1 ? ", RCCL gather"
                                                                : ", RCCL communicator (one rank: nothing to gather)");
    image.make_PPM(out);
    return 0;
} catch (const std::exception& e) {
    std::fprintf(stderr, "vol_render: %s\n", e.what());
    return 1;
}
