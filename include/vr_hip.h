/*
 * vr_hip.h — C ABI of the MI355X-native forward volume renderer (libvr_hip.so).
 *
 * This is the drop-in boundary for the reference's forward render call
 *     Integrator::render(const Scene&, Image&)            (include/integrator.h:49-57)
 * of wantonsushi/3DG-vol-renderer. Plain C: opaque handles, plain structs, pointers and sizes,
 * integer status codes, no exceptions and no C++/torch types across the boundary. The header-only
 * C++ mirror of the reference API (3dg-vol-renderer_amd/include/vr/: Scene, Camera, Image,
 * Integrator, HipRayMarchingGaussians ...) and the Python ctypes mirror (vr_amd) both sit on top
 * of exactly these entry points. INTEGRATION.md shows the bindings.
 *
 * Every entry point returns VR_OK (0) on success; on failure it returns a non-zero vr_status and
 * vr_last_error() (thread-local) describes why. The C++ wrappers turn a non-zero status into
 * std::runtime_error, which is the reference's error convention (scene.h:47,79; image.h:26,30).
 */
#ifndef VR_HIP_H_
#define VR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 11
/* (still 11 with vr_query_features / vr_query_features_grad, vr_query_radiance and vr_query_radiance_grad: entry points
 * were added, none changed) */

typedef enum vr_status {
    VR_OK = 0,
    VR_ERR_INVALID = 1,     /* bad argument / inconsistent request */
    VR_ERR_IO = 2,          /* cannot open / read / write a file */
    VR_ERR_PARSE = 3,       /* malformed scene / XML / PPM */
    VR_ERR_HIP = 4,         /* HIP runtime error (includes "no GPU") */
    VR_ERR_NOSCENE = 5,     /* render before vr_upload_scene */
    VR_ERR_OVERFLOW = 6,    /* a per-ray capacity (active set, stack, step table) was exceeded */
    VR_ERR_UNSUPPORTED = 7, /* valid request the device path does not implement */
    VR_ERR_RETRY = 8        /* vr_synchronize only: the last frame outgrew the scatter-record buffers
                               sized from earlier frames; they have been grown, render it again */
} vr_status;

/* scene.h:18-22 Scene::VolumeType */
typedef enum vr_volume_type { VR_VOLUME_GAUSSIANS = 0, VR_VOLUME_SPHERES = 1 } vr_volume_type;

/* camera.h:31 Pinhole_Camera, camera.h:58 Orthographic_Camera */
typedef enum vr_camera_type { VR_CAMERA_PINHOLE = 0, VR_CAMERA_ORTHOGRAPHIC = 1 } vr_camera_type;

/* Integrators with a device implementation. */
typedef enum vr_integrator {
    VR_RAYMARCH_GAUSSIANS = 0, /* RayMarchingGaussians  test_integrators.h:143-297 */
    VR_RAYMARCH_SPHERES = 1,   /* RayMarchingSpheres    test_integrators.h:11-136  */
    VR_TEST_HITMASK = 2,       /* TestIntegrator        integrator.h:65-94         */
    VR_PURE_RAYMARCH = 3,      /* PureRayMarching       integrator.h:100-267       */
    VR_FREE_FLIGHT = 4,        /* FreeFlightGaussians   integrator.h:273-408 (single scattering) */
    VR_MULTI_SCATTER = 5       /* MultiScatterGaussians integrator.h:416-720 (ANALYTIC_PLUS_NEWTON) */
} vr_integrator;

/* Light (scene.h:12-15). */
typedef struct vr_light {
    float position[3];
    float intensity[3];
} vr_light;

/* One 'g' record of a scene file / arguments of Gaussian(mean, cov, density, albedo, emission)
 * (scene.h:91-113, gaussian.h:75-92). cov = {xx, xy, xz, yy, yz, zz}. Emission is carried for API
 * parity but is never read by any reference integrator. */
typedef struct vr_gaussian {
    float mean[3];
    float cov[6];
    float density;
    float albedo;
    float emission[3];
} vr_gaussian;

/* Sphere(center, radius, sigma_a, sigma_s) (smm.h:17-27). */
typedef struct vr_sphere {
    float center[3];
    float radius;
    float sigma_a;
    float sigma_s;
} vr_sphere;

/* Camera state after the reference constructors ran (camera.h:15-22, 38-43, 60-62). */
typedef struct vr_camera {
    int32_t type;        /* vr_camera_type */
    float position[3];
    float view_dir[3];   /* normalised member Camera::view_dir */
    float right[3];
    float up[3];
    float pinhole[3];    /* pinhole cameras only */
    float fov;
    float focal_length;  /* 1 / tan(fov / 2) */
} vr_camera;

/* Render parameters = the integrator constructor arguments (test_integrators.h:17,149-153;
 * integrator.h:278-281, 501-505). */
typedef struct vr_render_params {
    int32_t integrator;   /* vr_integrator */
    float step_size;      /* ray-march step (reference default 0.01) */
    int32_t env_samples;  /* environment directions per scattering step (20 Gaussians, 5 spheres) */
    float t_eps;          /* stop a ray once T <= t_eps; 0 = exact (stop only when T == 0) */
    uint32_t flags;       /* reserved, must be 0 */
    int32_t num_samples;  /* free-flight integrators: paths per pixel (FreeFlightGaussians 256,
                             MultiScatterGaussians 16; set_num_samples, integrator.h:719) */
    int32_t min_bounces;  /* MultiScatterGaussians min_scatter (default 5): Russian roulette after it */
} vr_render_params;

typedef struct vr_scene_info {
    int32_t volume_type;  /* vr_volume_type */
    int64_t num_primitives;
    int64_t num_lights;
    float env_color[3];
    float bounds_min[3];  /* union of the primitives' 3-sigma / sphere boxes */
    float bounds_max[3];
} vr_scene_info;

/* Statistics of the last vr_render / vr_render_tiles_device call on a context (waits for it).
 * A frame's pixels do not depend on what the context did before. The counts of a ray-march frame (pixels,
 * fallback_pixels, error_pixels, scatter_records, deep_pixels) depend on it in one way: a frame that re-ran 5 % of its
 * pixels on the large-capacity path makes the context's later frames of that scene march with twice the slots (until
 * the next upload), and a frame that outgrew the buffers left by earlier frames and was rendered again counts as such a
 * later frame. A frame therefore reports the counts of a new context's first frame of the scene, or those of its
 * second: fewer fallback_pixels, and another scatter_records, which counts the records of abandoned marches too.
 * filtered_rays is 0 on the frames that leave the list filter out. */
typedef struct vr_render_stats {
    double kernel_ms;         /* device time of the render kernels (HIP events) */
    int64_t pixels;           /* pixels rendered */
    int64_t fallback_pixels;  /* pixels re-run on the large-capacity path (active-set overflow);
                                 free-flight integrators: paths re-run with kFFBigCap-entry rows
                                 (more than 128 Gaussians overlapping one point) */
    int64_t error_pixels;     /* pixels that exceeded every capacity (output NaN) */
    /* Stages (HIP events on the render stream). RayMarchingGaussians: [0] primary march (scatter
     * records), [1] record-buffer sizing (one host sync; a re-run of the march if the capacity
     * carried over from the last frame was too small) and secondary-ray cut-offs, [2] secondary-ray
     * transmittance, [3] accumulate. FreeFlight / MultiScatterGaussians: [0] path kernel, [2]
     * deferred shadow rays, [3] accumulate. 0 for the other integrators. */
    double stage_ms[4];
    int64_t scatter_records;  /* march steps with sigma_s > 0 (each spawns lights + env_samples rays) */
    int64_t secondary_rays;   /* records * (lights + env_samples) */
    int64_t record_overflow;  /* 1: the frame outgrew the scatter-record buffers sized from earlier
                                 frames (its output is invalid; the buffers have been grown, render
                                 again). vr_render does that itself. */
    int64_t deep_pixels;      /* pixels re-run on the global-memory active-list pass (> 64 active) */
    int64_t slow_rays;        /* RayMarchingGaussians: secondary rays traced again on the exact slow path (a light
                                 ray's stopping event, a missed member, a member at its 3-sigma boundary, two
                                 chords or a member's within the reference f32 quadratic's error band) */
    int64_t band_rays;        /* RayMarchingGaussians: secondary rays with one non-member chord within that band,
                                 whose contribution the reference's M form recomputes (secondary_fix_kernel) */
    int64_t filtered_rays;    /* RayMarchingGaussians: environment rays whose record's active list alone reaches the
                                 optical-depth cut-off: their Tr = 0 is written by the pass that orders the
                                 environment rays and the persistent kernel never traces them (VR_OPT_SEC_FILTER;
                                 0 with the option off). Part of secondary_rays. (ABI 10) */
} vr_render_stats;

typedef struct vr_scene vr_scene; /* host-side scene: primitives, lights, env colour */
typedef struct vr_ctx vr_ctx;     /* device context: one GPU, uploaded scene, workspaces */

/* ---------------- library ---------------- */
const char* vr_version(void);
/* Thread-local description of the last failure of any vr_* call on this thread. */
const char* vr_last_error(void);

/* ---------------- host scene (scene.h) ---------------- */
vr_status vr_scene_create(int32_t volume_type, vr_scene** out);
/* Scene::load_GMM (scene.h:72-120), incl. its skip-unknown-token and emission-peek behaviour. */
vr_status vr_scene_load_gmm(const char* path, vr_scene** out);
/* Scene::load_SMM (scene.h:38-68). */
vr_status vr_scene_load_smm(const char* path, vr_scene** out);
/* Mitsuba-3 subset used by tests/env_one_sphere_test_ortho.xml (no reference equivalent; the
 * reference rendered that XML in Mitsuba). Fills the scene, camera, film size and parameters.
 * Any output pointer may be NULL. */
vr_status vr_scene_load_xml(const char* path, vr_scene** out, vr_camera* camera, uint32_t* width,
                            uint32_t* height, vr_render_params* params);
vr_status vr_scene_add_gaussians(vr_scene* s, const vr_gaussian* g, size_t n);
/* Synthetic scenes of the reference generators' distribution (tests/make_random.py:21-45 for
 * variant 0, tests/make_nonuniform_random.py:19-30 (y biased towards 0) for variant 1): mean
 * x,z ~ U(-1,1), y ~ U(0,2); per-axis diameter ~ U(0.01, 0.035); covariance
 * Q diag((d/2)^2) Q^T with Q from the QR of a 3x3 standard-normal matrix (det fixed to +1);
 * density ~ U(0.2, 0.5); albedo ~ U(0.25, 0.95); emission ~ U(0,1)^3. Values are rounded exactly as
 * the generators print them (%.4f / %.6f) and then read back as floats, so a generated scene is
 * the scene load_GMM would produce from the generator's text file. Seeded PCG32 (rng.h). */
vr_status vr_scene_add_random_gaussians(vr_scene* s, uint64_t n, uint64_t seed, int32_t variant);
vr_status vr_scene_add_spheres(vr_scene* s, const vr_sphere* sp, size_t n);
vr_status vr_scene_add_lights(vr_scene* s, const vr_light* l, size_t n);
vr_status vr_scene_set_env_color(vr_scene* s, const float rgb[3]);
vr_status vr_scene_get_info(const vr_scene* s, vr_scene_info* out);
/* Gaussian precompute (gaussian.h:52-55): 12 floats per Gaussian, in scene order:
 * mean[3], density, inv_cov{00,01,02,11,12,22}, norm, albedo. */
vr_status vr_scene_get_records(const vr_scene* s, float* out, size_t n);
vr_status vr_scene_get_lights(const vr_scene* s, vr_light* out, size_t n);
vr_status vr_scene_get_gaussians(const vr_scene* s, vr_gaussian* out, size_t n);
vr_status vr_scene_get_spheres(const vr_scene* s, vr_sphere* out, size_t n);
void vr_scene_destroy(vr_scene* s);

/* ---------------- camera (camera.h) ---------------- */
vr_status vr_camera_pinhole(const float position[3], const float view_dir[3], float fov, vr_camera* out);
vr_status vr_camera_orthographic(const float position[3], const float forward[3], vr_camera* out);
/* Camera::sample_ray (camera.h:45-53, 64-73) followed by Ray's normalisation (ray.h:11-12). */
vr_status vr_camera_sample_ray(const vr_camera* c, double u, double v, float origin[3], float direction[3]);

/* ---------------- image (image.h) ---------------- */
/* Image::make_PPM (image.h:62-84): 8-bit P6 with clamp(v*255) truncation. rgb is 3*W*H floats. */
vr_status vr_image_write_ppm(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* Image(const std::string&) (image.h:24-45): P6 reader; rgb must hold 3*W*H floats. Pass rgb=NULL
 * to query width/height only. */
vr_status vr_image_read_ppm(const char* path, float* rgb, uint32_t* width, uint32_t* height);

/* ---------------- animated GIF (tests/main.cpp:81-114 turntable; gif-h's role) ---------------- */
typedef struct vr_gif vr_gif;
/* GifBegin: a looping GIF89a of width x height frames (delay_cs: the default frame delay, 1/100 s). */
vr_status vr_gif_begin(const char* path, uint32_t width, uint32_t height, uint32_t delay_cs, vr_gif** out);
/* GifWriteFrame: one RGBA8 frame (Image::get_rgba_buffer, image.h:89-104) shown for delay_cs
 * hundredths of a second; its own 256-colour palette (median cut), LZW-compressed. */
vr_status vr_gif_write_frame(vr_gif* gif, const uint8_t* rgba, uint32_t delay_cs);
/* GifEnd: trailer, close, free. */
vr_status vr_gif_end(vr_gif* gif);

/* ---------------- device ---------------- */
vr_status vr_init(int device, vr_ctx** out);
/* Number of visible GPUs. */
vr_status vr_device_count(int32_t* n);
/* Multi-GPU context: one host thread drives `ndev` GPUs (devices[0..ndev-1], or
 * 0..ndev-1 if devices is NULL). vr_upload_scene replicates the scene on every device; vr_render cuts
 * the frame into 16x16 tiles, rank r renders tiles r, r+ndev, r+2ndev, ... into a packed slab on its
 * device, the slabs are gathered to devices[0] with RCCL (one ncclGroupStart/End of every rank's
 * ncclSend and the root's ncclRecv over xGMI; librccl is loaded at this call) and unshuffled there
 * into the row-major frame. A device listed more than once shares its GPU between ranks (rehearsal
 * of the split on one GPU; the slabs then move with device copies, RCCL holds one rank per device).
 * vr_synchronize / vr_set_option apply to every device; vr_get_stats sums counts over the ranks and
 * reports the slowest rank's times (vr_get_rank_stats: one rank). The other entry points act on the
 * first device. vr_destroy releases the whole group. */
vr_status vr_init_multi(int32_t ndev, const int32_t* devices, vr_ctx** out);
/* Devices a context drives (1 for vr_init contexts); whether its gather runs over RCCL. */
int32_t vr_ctx_num_devices(const vr_ctx* ctx);
int32_t vr_ctx_uses_rccl(const vr_ctx* ctx);
vr_status vr_get_rank_stats(vr_ctx* ctx, int32_t rank, vr_render_stats* out);
void vr_destroy(vr_ctx* ctx);
/* Prepare (BVH build) and upload the scene; replaces any previous one. Host copies are not kept. */
vr_status vr_upload_scene(vr_ctx* ctx, const vr_scene* s);
/* A Gaussian scene straight from device memory: d_mean (3 n), d_cov6 (6 n: xx xy xz yy yz zz), d_density (n) and
 * d_albedo (n) are float arrays on the context's GPU (an optimiser's parameters, say); lights (n_lights of them)
 * and env_color (NULL: scene.h:29's default) are host memory. Records, boxes and scene statistics are computed on
 * the device and handed to the device BVH builder: nothing goes through the host. The context ends up in the state
 * vr_upload_scene leaves it in under VR_OPT_DEVICE_BVH = 1 for a vr_scene built by vr_scene_add_gaussians from the
 * same floats, lights and environment (emission is not taken: nothing reads it): every record word, every box and
 * so the scene bounds, the half-tree decision and every tree array are that upload's bit for bit, with one
 * deviation, the records' `norm`. The host computes (float)(K * (double)powf(det, -0.5f)), K = (2 pi)^-1.5 in
 * double, and libm's powf is not reproducible on the device; this call computes
 *     (float)(K * (double)(float)(1.0 / sqrt((double)det)))
 * with the same f32 determinant det and the host's K: IEEE operations only, so it can be restated exactly
 * anywhere. Both inverse square roots are faithful (within one ulp of each other) and the product is rounded once
 * more: the two norms differ by at most 2 f32 ulp (against glibc's powf on 0.06-0.07 % of seeded covariances).
 * Synchronous: it begins with the device synchronise vr_upload_scene begins with, so arrays written on any
 * stream are complete, and on return the scene is current and the caller may overwrite its arrays (nothing of
 * them is kept). It replaces the previous scene, collects its last report and resets what vr_upload_scene resets;
 * on a failure after the arguments were accepted the context holds no scene. VR_OPT_HALF_NODES and VR_OPT_SEC_TIGHT apply as at any upload;
 * VR_OPT_DEVICE_BVH is not consulted. Two cases copy the arrays to the host and take vr_upload_scene's host path
 * (such a scene is the host upload's in every bit, norm included; vr_tree_info.built_on_device tells): fewer than
 * 256 Gaussians (n = 0 included), and a radix tree deeper than the traversal stacks, as vr_upload_scene falls
 * back. The scene heuristics (first window, shadow-ray refill, free-flight kernel choice) are the host's; the
 * overlap estimate is a double sum reduced in a fixed order, so it is the same on every run but may differ from
 * the host loop's in its last bits (it feeds a threshold only; results do not depend on it).
 * VR_ERR_INVALID: NULL ctx, a NULL array with n > 0, NULL lights with n_lights > 0. VR_ERR_UNSUPPORTED: more than
 * 16 lights, n >= 2^27, or a vr_init_multi context (the arrays live on one device). */
vr_status vr_upload_gaussians_device(vr_ctx* ctx, const float* d_mean, const float* d_cov6, const float* d_density,
                                     const float* d_albedo, size_t n, const vr_light* lights, size_t n_lights,
                                     const float env_color[3]);
/* Integrator::render(scene, image): full W x H frame into rgb_host (3*W*H floats, row-major,
 * idx = 3*(y*W + x) as image.h:13-17). Synchronous. */
vr_status vr_render(vr_ctx* ctx, const vr_camera* cam, const vr_render_params* p, uint32_t width,
                    uint32_t height, float* rgb_host);
/* Multi-GPU building block (asynchronous on `stream`, a hipStream_t or NULL for the default; the
 * host never waits for the device inside a frame once the context has rendered one frame of this
 * kind — the first sizes the scatter-record buffers). The frame's outcome is reported by
 * vr_synchronize (VR_ERR_RETRY if the frame outgrew the record buffers, which are then grown:
 * render it again; VR_ERR_OVERFLOW if pixels exceeded a per-ray capacity) and by vr_get_stats.
 * The frame is cut into 16x16 tiles numbered row-major; this call renders tiles
 * first_tile, first_tile + tile_stride, ... (num_tiles of them). If `packed` is non-zero the
 * output is a slab of num_tiles * 256 pixels (tile-major, row-major inside a tile, 3 floats per
 * pixel; pixels outside the frame are written as 0); otherwise `d_out` is the full W x H frame and
 * only those tiles' pixels are written. d_out is device memory. */
vr_status vr_render_tiles_device(vr_ctx* ctx, const vr_camera* cam, const vr_render_params* p,
                                 uint32_t width, uint32_t height, uint32_t first_tile,
                                 uint32_t tile_stride, uint32_t num_tiles, int32_t packed,
                                 float* d_out, void* stream);
/* Scatter `nslabs` packed slabs (slab r = tiles r, r+nslabs, ...; each tiles_per_slab * 256 px)
 * into the row-major W x H frame d_image. Asynchronous on `stream`. */
vr_status vr_unshuffle_tiles_device(vr_ctx* ctx, const float* d_slabs, uint32_t nslabs,
                                    uint32_t tiles_per_slab, uint32_t width, uint32_t height,
                                    float* d_image, void* stream);
/* Scatter the packed slabs of ranks first .. first + nslabs - 1 of a stride-way split (slab k = tiles
 * first + k, first + k + stride, ...; each tiles_per_slab * 256 px) into the row-major W x H frame
 * d_image: the gather of a split whose root rendered its own tiles straight into the frame.
 * Asynchronous on `stream`. */
vr_status vr_unshuffle_tiles_part_device(vr_ctx* ctx, const float* d_slabs, uint32_t first, uint32_t nslabs,
                                         uint32_t stride, uint32_t tiles_per_slab, uint32_t width, uint32_t height,
                                         float* d_image, void* stream);
/* Diagnostics (untimed): render the given tiles once with the instrumented build of the same
 * kernels and return the work they executed. counts[0..7], the march kernels (both passes):
 * [0] BVH node tests (4-wide nodes, or child pairs on the fallback path), [1] ray-Gaussian
 * quadratic + intersect evaluations, [2] optical-depth evaluations, [3] density (mu_t)
 * evaluations, [4] unused, [5] active march steps, [6] primary-ray BVH queries, [7] pixels completed.
 * counts[8..15], the secondary-ray stage (the persistent kernel's own schedule + the exact slow path):
 * [8] BVH node steps, [9] tree-leaf primitive tests, [10] optical-depth evaluations, [11] active-
 * list primitive tests, [12] secondary rays started, [13] rays ended by the optical-depth cut-off,
 * [14] node steps of those rays, [15] node steps of the rays that ran to the end of the tree.
 * Free-flight integrators: counts[0..7], the path kernel: [0] paths, [1] free-flight distance
 * searches (bounces), [2] 4-wide node steps and [3] child-pair node steps of the hit-collection
 * walks, [4] ray-Gaussian quadratic + intersect evaluations, [5] erf evaluations of the event sweep,
 * the entries' cached factors and the distance solver, [6] shadow rays traced inline, [7] shadow
 * rays queued; counts[8..11], the shadow-ray kernel: [8] rays, [9] 4-wide node steps, [10] primitive
 * tests, [11] optical depths. Synchronous; Gaussian scenes only. Used for the roofline reports. */
vr_status vr_count_work(vr_ctx* ctx, const vr_camera* cam, const vr_render_params* p, uint32_t width,
                        uint32_t height, uint32_t first_tile, uint32_t tile_stride, uint32_t num_tiles,
                        uint64_t counts[16]);
/* MultiScatterGaussians::render(scene, image, &per_pixel_gaussians) under RECORD_PIXEL_GAUSSIANS
 * (integrator.h:532-536, 616-644): renders like vr_render (params->integrator must be
 * VR_MULTI_SCATTER) and records, per pixel, the Gaussians (scene order) with an event at or before
 * a path's scattering point (t <= t_scatter + 1e-6), or every Gaussian hit by a path segment that did
 * not scatter, as a bitset in the context's recording `slot` (0 or 1). Synchronous. */
vr_status vr_render_record(vr_ctx* ctx, const vr_camera* cam, const vr_render_params* p, uint32_t width,
                           uint32_t height, float* rgb_host, int32_t slot);
/* Copy a recording to the host: bits[w * W*H + p] bit b set <=> Gaussian 32w + b was recorded at
 * row-major pixel p. n_words must be ceil(N/32) * W * H. */
vr_status vr_get_pixel_gaussians(vr_ctx* ctx, int32_t slot, uint32_t* bits, size_t n_words);
/* Stochastic finite-difference statistic of StochasticFiniteDiffInverseIntegrator::optimize
 * (inverse_integrator.h:166-182): out[g] = sum over the union of the pixels recorded for Gaussian g
 * in slot 0 (base render) and slot 1 (perturbed render) of loss_plus[p] - loss_base[p] (double).
 * loss_* are host arrays of W*H per-pixel L1 losses (compute_pixel_losses, :21-30); n = N. */
vr_status vr_sfd_loss_diff(vr_ctx* ctx, const float* loss_base, const float* loss_plus, uint32_t width,
                           uint32_t height, double* out, size_t n);
/* ---------------- inverse rendering (gmm.h:583-706, optimizer.h, inverse_integrator.h) ---------------- */
/* GaussianMixtureModel::pack_parameters (gmm.h:583-628): 11 floats per Gaussian, scene order: mean(3),
 * Rodrigues rotation of the covariance eigenbasis (3), log scale (3), log density, logit albedo.
 * n_params must be 11 * N. (Eigenbasis from a Jacobi solver, made right-handed: DESIGN.md §3c.) */
vr_status vr_gmm_pack_parameters(const vr_scene* s, float* params, size_t n_params);
/* apply_params_to_gmm_local (gmm.h:634-674): a new scene with base's lights / environment and every
 * Gaussian rebuilt from params (covariance R S S^T R^T, density exp, albedo sigmoid). */
vr_status vr_gmm_apply_parameters(const vr_scene* base, const float* params, size_t n_params, vr_scene** out);
/* make_default_eps_for_params (gmm.h:678-706). */
vr_status vr_gmm_default_eps(float* eps, size_t n_params);
/* AdamOptimizer::step (optimizer.h:31-44) for step number t >= 1 (m, v: the moment vectors). */
vr_status vr_adam_step(float* params, const float* grads, float* m, float* v, size_t n, int32_t t, float lr, float beta1,
                       float beta2, float eps);
/* Sign vector k of vr_sfd_optimize's run with `seed` (+1 / -1 per parameter): the deterministic
 * stand-in for the reference's coin(mt19937(random_device)) (inverse_integrator.h:101-103, 139-141).
 * The stream is the textbook PCG32 (XSH-RR 64/32) after pcg32_srandom(initstate = splitmix64(seed),
 * initseq = splitmix64(k)), splitmix64 being the usual finaliser of x + 0x9e3779b97f4a7c15; entry i is +1
 * where the i-th output's 24-bit uniform (output >> 8) / 2^24 is below 0.5, else -1. vr_sfd_optimize draws
 * vector it * num_stoch_samples + j for sample j of iteration it. */
vr_status vr_sfd_sign_vector(uint64_t seed, uint64_t k, float* signs, size_t n);

/* SFDDConfig (inverse_integrator.h:52-57) + run options. */
typedef struct vr_sfd_config {
    int32_t max_iters;          /* reference default 1000 */
    int32_t save_every;         /* 25: render + write out_dir/iter_NNNN.ppm every save_every iterations */
    int32_t num_stoch_samples;  /* 4: sign vectors per iteration */
    float lr;                   /* 1e-2 (Adam) */
    uint64_t seed;              /* sign-vector stream (vr_sfd_sign_vector) */
    int32_t final_samples;      /* 16384: paths per pixel of the final render (:229-238); 0 skips it */
    const char* out_dir;        /* NULL / "": write no images (the reference writes ./sfd_output) */
} vr_sfd_config;
typedef struct vr_sfd_result {
    float* params;         /* out, 11 * N: the optimised parameters (caller-allocated) */
    double* loss_history;  /* out, max_iters: mean L1 loss of every base render */
    double* last_grads;    /* out (may be NULL), 11 * N: the last iteration's SFD gradient estimate */
    float* final_image;    /* out (may be NULL), 3 * W * H: the final render */
    double final_loss;     /* out: its mean L1 loss (-1 if final_samples == 0) */
} vr_sfd_result;
/* StochasticFiniteDiffInverseIntegrator::optimize(scene_initial, I_ref) (inverse_integrator.h:61-238)
 * on the context's device: per iteration a recorded base render (RECORD_PIXEL_GAUSSIANS bitsets in
 * HBM), num_stoch_samples perturbed recorded renders, the per-Gaussian union-of-pixels loss
 * statistic and per-pixel L1 losses on the device, Adam on the host; every parameter update is
 * re-uploaded with the device BVH build. fwd: MultiScatterGaussians parameters; I_ref: 3 * W * H. */
vr_status vr_sfd_optimize(vr_ctx* ctx, const vr_camera* cam, const vr_render_params* fwd, const vr_scene* scene_initial,
                          const float* I_ref, uint32_t width, uint32_t height, const vr_sfd_config* cfg,
                          vr_sfd_result* result);
/* Number of 16x16 tiles of a W x H frame. */
uint32_t vr_num_tiles(uint32_t width, uint32_t height);
/* Per-context tuning options (defaults are the benchmark/product settings). Explicit and
 * re-entrant: the library reads no environment variables. */
typedef enum vr_option {
    VR_OPT_HALF_NODES = 1,       /* 1 (default): upload f16 copies of the BVH (pair + 4-wide) when the
                                    scene's leaf boxes suit them; 0: f32 nodes only. Applies at the next
                                    vr_upload_scene. Results are identical either way (boxes only
                                    propose candidates; every decision is the exact quadratic). */
    VR_OPT_SECONDARY_BUDGET = 2, /* 1 (default): with t_eps > 0, stop secondary rays at a per-record
                                    optical depth that keeps each pixel within t_eps (DESIGN.md error
                                    budget); 0: the frame-wide cut-off ln(1/t_eps) + ln(1000) only. */
    VR_OPT_FF_WINDOW0 = 3,       /* free-flight integrators: first hit-window capacity, 1..128, doubling per
                                    window; 0 (default): derived from the uploaded scene's typical optical
                                    depth per Gaussian (4..32). Results do not depend on it. */
    VR_OPT_RECORD_CAPACITY = 4,  /* scatter-record buffer capacity (records; the active-list pool gets the
                                    same) carried into the next frame: 0 (size it at the next frame, with one
                                    host sync) or >= 4096. The context normally sizes it from earlier frames;
                                    setting it lets a test drive a frame over capacity (reported, then
                                    rendered again with grown buffers). Results do not depend on it. */
    VR_OPT_DEVICE_BVH = 5,       /* 0 (default): vr_upload_scene builds the BVH on the host (binned SAH);
                                    1: on the device (linear BVH: Morton sort + radix tree, kernels/
                                    vr_lbvh.hip) for scenes of >= 256 Gaussians — the fast path for the
                                    inverse loop's re-upload after every parameter update. Results are
                                    identical up to summation order (the event set is tree-independent). */
    VR_OPT_FF_NEE_QUEUE = 6,     /* free-flight integrators: shadow-ray queue capacity, in rays per path of a
                                    launch, 0..16 (default 6). The path kernel queues each bounce's next-event
                                    shadow ray for a separate tracing kernel; 0 traces them inline. Results
                                    are identical (the same walk and sums). A frame whose launch found the
                                    queue full is reported (VR_ERR_RETRY from the asynchronous entry points;
                                    vr_render re-renders by itself) and rendered again with a grown queue, or,
                                    once the queue is at this bound, with every shadow ray inline (so for the
                                    context's later frames, until the next upload or a change of this option).
                                    Memory: the queue holds value x (paths of a launch, at most 2^23) rays
                                    of 48 B, 2.4 GB at the default 6 per path; it is grown, never shrunk,
                                    per context (lower it for many contexts on one device). */
    VR_OPT_MARCH_BINNED = 7,     /* RayMarchingGaussians / PureRayMarching primary march: 0 (default): BVH
                                    window queries per pixel; 1: Gaussians binned to 16x16 tiles by depth
                                    bucket, each tile's list streamed by its waves.
                                    Results are identical (the same exact intersect decides every entry). */
    VR_OPT_FF_SOLVER = 8,        /* free-flight integrators: the distance solver (distance_solvers.h:143-187, a
                                    compile-time #define in the reference): 0 (default) ANALYTIC_PLUS_NEWTON, the
                                    mode the reference compiles (:146); 1 BISECTION; 2 NEWTON; 3
                                    ANALYTIC_PLUS_BISECTION; 4 UNIFORM, whose rand01() (mt19937 seeded by
                                    random_device, not reproducible) is replaced by the textbook-PCG32 uniform of
                                    stream 2 + bounce of the path's derive_path_seed (documented deviation). */
    VR_OPT_START_SUBTREE = 9,    /* RayMarchingGaussians / PureRayMarching secondary rays (4-wide tree): 1 (default):
                                    a ray walks the deepest subtree holding its record's position first, then
                                    climbs to the root (no descent from the root for rays cut near their origin);
                                    0: every walk starts at the root. Same Gaussians, same decisions; only the
                                    order of the optical-depth sum differs (float association). */
    /* 10: retired (round 6): the staged free-flight pipeline, measured 2.3x slower than the persistent path kernel */
    VR_OPT_SEC_TIGHT = 11,       /* RayMarchingGaussians secondary rays, applied at the next upload: 1 (default):
                                    their own copy of the 4-wide tree with the exact boxes of the ellipsoids the
                                    whitened test accepts (the shared tree's boxes are padded by 5 % for the
                                    camera rays' M-form test); 0: the shared tree. Same Gaussians, same
                                    decisions; only the order of the optical-depth sum differs. */
    VR_OPT_MARCH_WIDE_MIN = 12,  /* RayMarchingGaussians / PureRayMarching: pixels whose active set outgrew the
                                    primary march's 16 LDS slots are marched again; a queue of at least this
                                    many pixels (default 2048) goes one pixel per lane with 64 slots in
                                    global memory, a shorter one one pixel per wave (64 LDS slots). Same
                                    operations either way: frames are identical. */
    VR_OPT_SEC_FILTER = 14,      /* RayMarchingGaussians secondary rays (scenes with whitened records): 1 (default):
                                    the pass that orders a record chunk's environment rays by direction also runs
                                    each ray's list phase (the record's active Gaussians, at most 16 of them) and
                                    keeps the rays that reach their optical-depth cut-off there out of the
                                    persistent kernel (vr_render_stats.filtered_rays); 0: every ray is handed
                                    out. The same arithmetic decides either way: frames are identical. */
    VR_OPT_FF_KERNEL = 13        /* free-flight integrators, persistent path kernel: 0 (default) chosen from the
                                    uploaded scene: the phase-scheduled kernel for translucent scenes of many
                                    Gaussians (at least 256, median central-chord optical depth below 16: long
                                    hit collections and event sweeps per bounce), else the bounce kernel;
                                    1: the bounce kernel (a whole bounce per lane and wave iteration);
                                    2: the phase-scheduled kernel (each wave iteration runs the collection, sweep
                                    or shading phase most of its lanes are in). Frames are identical. */
} vr_option;
vr_status vr_set_option(vr_ctx* ctx, int32_t option, int64_t value);
vr_status vr_get_option(vr_ctx* ctx, int32_t option, int64_t* value);
/* Waits for the context's device work; returns VR_ERR_RETRY / VR_ERR_OVERFLOW if the last frame is
 * invalid (see vr_render_tiles_device). The outcome is reported once per frame, also when vr_get_stats
 * (or any other call) collected the frame's report first; a later frame's call replaces it. */
vr_status vr_synchronize(vr_ctx* ctx);
vr_status vr_get_stats(vr_ctx* ctx, vr_render_stats* out);
/* Diagnostics: the pixels of the last RayMarchingGaussians / PureRayMarching frame that were re-run
 * on the large-capacity fallback path (vr_render_stats.fallback_pixels of them). Writes up to `cap`
 * (x, y) pairs into xy[2*cap] (global frame coordinates, queue order) and the total count into *n. */
vr_status vr_get_fallback_pixels(vr_ctx* ctx, uint32_t* xy, size_t cap, size_t* n);
/* Diagnostics (slow: one copy per value): the scatter records of pixel (x, y) of the last
 * RayMarchingGaussians frame in step order, one row of 9 + S floats each (S = lights + env_samples):
 * step index k, record position xyz, T * sigma_s, Li + Le (rgb), active-list length, then the
 * transmittance of each secondary ray (lights first, then environment samples, in sample order).
 * Writes up to `cap` rows of `row` floats into out, the record count into *n and the frame's row
 * width 9 + S into *row_out (if not NULL). With cap > 0, `row` must equal that width (VR_ERR_INVALID
 * otherwise: a narrower buffer would be written past its end); call with cap = 0 to learn both. */
vr_status vr_debug_pixel_records(vr_ctx* ctx, uint32_t x, uint32_t y, float* out, size_t cap, size_t row, size_t* n,
                                 size_t* row_out);

/* Diagnostics: the trees of the uploaded Gaussian scene as they lie on the device (read-only: no state of the
 * context changes and nothing is allocated past the call; the context's stream is synchronised first).
 * `array` selects one of the scene's arrays; elements are copied as stored (csrc/vr_internal.h):
 *   ORDER       uint32          record (tree order) -> scene index
 *   RECORDS     12 x float      mean xyz, density, M 00 01 02 11 12 22, norm, albedo, in tree order
 *   NODES       64 B BVHNode    child-pair tree: float f[12] (left box min xyz max xyz, right box), int32 c[4]
 *   HNODES      32 B HNode      its half-precision copy: uint16 h[12], int32 c[2]
 *   HNODES4     64 B HNode4     the 4-wide collapse: uint16 h[4][6], int32 c[4]
 *   HNODES4S    64 B HNode4     the secondary rays' tight refit of it
 *   HNODES4W    16 x uint32     HNODES4 laid out per axis (words 4a .. 4a+3: axis a's bounds as f16 pairs {min of
 *   HNODES4T    16 x uint32     children 0, 1}, {min 2, 3}, {max 0, 1}, {max 2, 3}; words 12-15 the refs); of HNODES4S
 *   PARENT4     int32           parent of every 4-wide node | (its slot + 1) << 28, root -1
 *   PRIM_NODE4  int32           the 4-wide node holding each record's leaf
 * Two calls, as vr_debug_pixel_records: with cap = 0 the element count goes into *n and the element size into
 * *elem_bytes (if not NULL); with cap > 0, up to cap elements are written to out. An array the scene does not have
 * (no half-precision trees, no tight refit) has count 0. `info`, if not NULL, is filled by every successful call.
 * VR_ERR_INVALID: no scene, a sphere scene, a vr_init_multi context, or an unknown array. */
typedef enum vr_tree_array {
    VR_TREE_ORDER = 0,
    VR_TREE_RECORDS = 1,
    VR_TREE_NODES = 2,
    VR_TREE_HNODES = 3,
    VR_TREE_HNODES4 = 4,
    VR_TREE_HNODES4S = 5,
    VR_TREE_HNODES4W = 6,
    VR_TREE_HNODES4T = 7,
    VR_TREE_PARENT4 = 8,
    VR_TREE_PRIM_NODE4 = 9
} vr_tree_array;
typedef struct vr_tree_info {
    int64_t num_prims, num_nodes, num_nodes4;
    int32_t bvh_depth;       /* levels of the child-pair tree, leaves included (root = 1): picks the traversal stack */
    int32_t built_on_device; /* 1: the device builder made this tree, 0: the host builder (also as its fallback) */
    int32_t wrec_pd;         /* 1: every record's M is positive definite (whitened secondary rays) */
    int32_t leaf_max;        /* build constants: primitives per leaf, */
    int32_t max_depth;       /*   the builders' depth bound (bvh_depth <= max_depth + 1), */
    int32_t wide_stack_max;  /*   per-lane stack entries of a 4-wide walk */
    float hn_center[3];      /* half-precision normalisation: u = (x - hn_center) * hn_scale */
    float hn_scale;
    float bounds_min[3], bounds_max[3]; /* the scene box */
} vr_tree_info;
vr_status vr_debug_tree(vr_ctx* ctx, int32_t array, void* out, size_t cap, size_t* n, size_t* elem_bytes,
                        vr_tree_info* info);
/* The build constants of vr_tree_info alone (no context needed); any pointer may be NULL. */
vr_status vr_tree_limits(int32_t* leaf_max, int32_t* max_depth, int32_t* wide_stack_max);

/* ---------------- mixture queries (gmm.h) ---------------- */
/* The questions GaussianMixtureModel and the free-flight integrators ask about the mixture itself, for a batch of the caller's
 * rays or points against the uploaded Gaussian scene (sphere scenes: VR_ERR_UNSUPPORTED). Every Gaussian is
 * tested with the exact forms (intersect_direct gaussian.h:126-164, optical_depth :208-231, mu_t :111-117 in
 * the reference's evaluation order), so hit decisions and entry / exit distances are the reference's bit for
 * bit; erf / exp come from the device library. Results do not depend on VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH.
 * Queries leave the last frame's report and statistics (vr_synchronize, vr_get_stats) untouched; on a
 * vr_init_multi context they act on the first device. A context runs one query at a time (they share its
 * workspaces): calls on one context are ordered by the caller, as renders are.
 * Common errors: VR_ERR_NOSCENE before an upload; VR_ERR_INVALID for a NULL pointer with n > 0, a device ray
 * array that is not 16-byte aligned, or n >= 2^31; n == 0 is VR_OK and touches nothing.
 * The `_device` forms take device pointers and are asynchronous on `stream` (a hipStream_t, NULL: the default
 * stream), like vr_render_tiles_device; the host forms copy and synchronise. */

/* One query ray, Ray(origin, direction) (ray.h:5-13) plus the distance bound of transmittance_up_to. 32 bytes. */
typedef struct vr_ray {
    float origin[3];
    float tmax;      /* transmittance only; +inf is valid */
    float direction[3];
    float unit;      /* 0: the direction is normalised as the Ray constructor does (ray.h:11-12); non-zero: it is a
                        Ray object's, normalised already, and is used as it stands (normalising twice would
                        move it by an ulp, and with it every entry / exit distance) */
} vr_ray;

/* GaussianMixtureModel::transmittance_up_to (gmm.h:517-578): tr[i] = expf(-(float)sum) with sum the double
 * sum over the Gaussians ray i hits of optical_depth(max(0, t_enter), min(tmax, t_exit)) where that interval
 * is not empty; tau[i] = (float)sum if tau is not NULL (then tr[i] == expf(-tau[i]) bit for bit). tmax <= 0 or
 * NaN: tr = 1, tau = 0 (gmm.h:518). A ray with a non-finite origin, or a direction whose squared norm is 0,
 * NaN or infinite in f32, gets NaN in both. */
vr_status vr_query_transmittance(vr_ctx* ctx, const vr_ray* rays, size_t n, float* tr, float* tau);
vr_status vr_query_transmittance_device(vr_ctx* ctx, const vr_ray* d_rays, size_t n, float* d_tr, float* d_tau,
                                        void* stream);

/* The gradient of the optical depth with respect to the Gaussians (differentiable transmittance):
 *   grad[10 g + k] = sum_i weight[i] * d tau_i / d theta_{g,k}
 * tau_i being what vr_query_transmittance returns as tau for ray i (tmax, unit and the validity rule as there), g the
 * SCENE index and theta the vr_gaussian row in its own order: mean[3], cov[6] = {xx, xy, xz, yy, yz, zz}, density. An
 * off-diagonal cov component is the derivative with respect to the stored number, which stands at (i, j) and (j, i):
 * 2 G_Sigma[i][j]. Albedo and emission do not enter tau; the gradient with respect to the rays is
 * vr_query_transmittance_ray_grad's, below.
 * weight == NULL: every weight is 1. A weight is used as it stands: for a loss over Tr the caller passes dL/dtau =
 * -Tr dL/dTr. Invalid rays contribute nothing, nor do rays with tmax <= 0 or NaN; a Gaussian no ray hits gets ten
 * zeros. Every entry of grad (10 * num_primitives floats) is written; n == 0 zeroes it (VR_OK). Unknown flag bits:
 * VR_ERR_INVALID; grad == NULL: VR_ERR_INVALID; the common errors above apply.
 * Definition. From the record's f32 mean, M (inverse covariance), norm and density rho, read as doubles, and the ray,
 * with p = o - mean: A = d.Md, B = 2 p.Md, C = p.Mp, q(t) = A t^2 + B t + C. [a, b] are the f32 clip bounds of the
 * transmittance query, a = max(0, t_enter), b = min(tmax, t_exit) from the exact f32 intersect_direct, so the hit set is
 * that query's bit for bit; a hit contributes iff b > a (no early-out at large optical depths). Centred at m = -B / 2A:
 * c = p + m d, k = exp(-(C - B^2 / 4A) / 2), u = t - m, and over [u_a, u_b]
 *   J0 = sqrt(pi / 2A) (erf(u_b sqrt(A / 2)) - erf(u_a sqrt(A / 2)))
 *   J1 = (e^{-A u_a^2 / 2} - e^{-A u_b^2 / 2}) / A
 *   J2 = (u_a e^{-A u_a^2 / 2} - u_b e^{-A u_b^2 / 2}) / A + J0 / A
 *   U = norm k J0 (tau per unit density), G_M = -rho norm k (J0 c c^T + J1 (c d^T + d c^T) + J2 d d^T) / 2,
 *   g_mean = rho norm k M (c J0 + d J1).
 * Without VR_GRAD_FROZEN_BOUNDS the ellipsoid's own bounds move with the parameters: the exit iff t_exit <= tmax, the
 * entry iff t_enter > 0. For each moving bound t, x = p + t d and w = +- rho norm e^{-4.5} / (2 A t + B) (+ exit,
 * - entry; 2 A t + B in double at the f32 t): G_M -= w x x^T, g_mean += 2 w M x. (A ray that grazes the ellipsoid has
 * 2 A t + B near 0: its bound terms are as large as the true derivative is.) With the flag the bounds are held, the
 * gradient of the integral over a fixed interval. Per Gaussian, summed over the rays with their weights: T = rho sum U,
 * G_Sigma = -M G_M M - T M / 2, and the density component is sum U.
 * Arithmetic: the decisions are f32 (the forward query's), everything on a decided hit is double, the sums over rays
 * are double atomic adds in arrival order and the result is rounded to f32 once. A result is therefore reproducible
 * to the rounding of a double sum, not bit for bit, and does not depend on VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH
 * beyond that. The staging (80 bytes per Gaussian) is the query's own and is zeroed on `stream` by each call. */
enum { VR_GRAD_FROZEN_BOUNDS = 1 };
vr_status vr_query_transmittance_grad(vr_ctx* ctx, const vr_ray* rays, const float* weight, size_t n, uint32_t flags,
                                      float* grad);
vr_status vr_query_transmittance_grad_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_weight, size_t n,
                                             uint32_t flags, float* d_grad, void* stream);

/* The gradient of the optical depth with respect to the ray (the other half of differentiable transmittance): row i
 * of out is d tau_i / d (origin, tmax, direction) of ray i and tau_i itself, tau_i being what vr_query_transmittance
 * returns as tau (tmax, unit and the validity rule as there). flags: 0 or VR_GRAD_FROZEN_BOUNDS, as above; unknown bits:
 * VR_ERR_INVALID. out == NULL with n > 0: VR_ERR_INVALID; the device form wants both arrays 16-byte aligned; the common
 * errors above apply (n == 0 is VR_OK and touches nothing).
 * Per hit, in double, in the notation of vr_query_transmittance_grad (the record's f32 numbers read as doubles, p, d the
 * direction the walk uses, A, B, C, m, c, k, u, J0, J1, J2, and [a, b] the forward query's f32 clip bounds; a hit
 * contributes iff b > a, no early-out):
 *   g_o = -rho norm k M (c J0 + d J1)                      (minus that hit's g_mean: tau sees o and mean through p only)
 *   g_d = -rho norm k M (m c J0 + (c + m d) J1 + d J2)
 * Without VR_GRAD_FROZEN_BOUNDS, for each moving bound t (the exit iff t_exit <= tmax, the entry iff t_enter > 0), with
 * x = p + t d and w = +- rho norm e^{-4.5} / (2 A t + B) (+ exit, - entry): g_o -= 2 w M x, g_d -= 2 w t M x.
 *   g_tmax = rho norm k e^{-A u_b^2 / 2} iff the upper bound is tmax itself (t_exit > tmax), else 0, with or without the
 * flag: tmax is the caller's bound, not the ellipsoid's. At t_exit == tmax the ellipsoid's exit is the bound (one-sided:
 * no tmax term). tmax = +inf gives 0.
 * The row: the seven sums over the ray's hits are kept in double and rounded to f32 once. `direction` with unit != 0 is
 * the sum of g_d, the derivative with respect to the three stored components taken as free; with unit == 0 the library
 * normalised the stored v itself and the row holds the chain through v / |v|, (g_d - d (d.g_d)) / |v|, |v| the square
 * root (in double) of the f32 squared norm the query computes. `tau` is computed as the transmittance query computes it
 * (f32 optical_depth per hit, added in double, rounded once) and equals its tau bit for bit: one call gives the value
 * and its ray Jacobian. An invalid ray (the queries' rule) gets NaN in all eight floats; tmax <= 0 or NaN gives eight
 * zeros. The hit set and every bound are the forward query's f32 ones and nothing is added atomically, so a result is
 * reproducible to the rounding of a double sum and does not depend on VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH beyond that. */
/* d tau / d ray, one row per ray, laid out as the vr_ray row it differentiates. 32 bytes. */
typedef struct vr_ray_grad {
    float origin[3];     /* d tau / d origin */
    float tmax;          /* d tau / d tmax */
    float direction[3];  /* d tau / d direction (see `unit`) */
    float tau;           /* the optical depth itself: vr_query_transmittance's tau for this ray, bit for bit */
} vr_ray_grad;
vr_status vr_query_transmittance_ray_grad(vr_ctx* ctx, const vr_ray* rays, size_t n, uint32_t flags, vr_ray_grad* out);
vr_status vr_query_transmittance_ray_grad_device(vr_ctx* ctx, const vr_ray* d_rays, size_t n, uint32_t flags,
                                                 vr_ray_grad* d_out, void* stream);

/* The transmittance profile: tau and Tr at K distances along each ray, from one tree walk per ray instead of K.
 * t holds the distances: n * K floats, row i for ray i, with t_stride = K, or one row of K shared by all rays with
 * t_stride = 0 (any other t_stride: VR_ERR_INVALID). tr and tau are n * K floats, row-major; either may be NULL, not
 * both (VR_ERR_INVALID).
 *   tau[i][k] and tr[i][k] are, bit for bit, what vr_query_transmittance returns for ray i with tmax = t[i][k].
 * So a sample <= 0 or NaN gives tau = 0, tr = 1; +inf is valid; an invalid ray (that query's rule) gets NaN in its whole
 * row; `unit` means what it means there; the row's own tmax field is not read. Samples may come in any order and may
 * repeat. Results do not depend on VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH (the sums are that query's double sums).
 * How: of optical_depth(a, b) only erf at the upper bound depends on b, so a hit's other factors are computed once for
 * all samples. The walk's work item is (ray, chunk of samples) and is pruned at the chunk's largest sample (NaN
 * ignored; no sample > 0: no walk), so with ascending samples the early chunks walk a shorter ray.
 * K == 0, K > VR_PROFILE_MAX_SAMPLES or n * K >= 2^31: VR_ERR_INVALID before anything is launched; a sphere scene:
 * VR_ERR_UNSUPPORTED; the common errors above apply. */
#define VR_PROFILE_MAX_SAMPLES 1024
vr_status vr_query_transmittance_profile(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride, size_t n,
                                         uint32_t K, float* tr, float* tau);
vr_status vr_query_transmittance_profile_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride,
                                                size_t n, uint32_t K, float* d_tr, float* d_tau, void* stream);

/* The gradient of a weighted sum of a profile's optical depths with respect to the Gaussians:
 *   grad[10 g + c] = sum_i sum_k weight[i][k] * d tau[i][k] / d theta_{g,c}
 * in the layout, with the flags (VR_GRAD_FROZEN_BOUNDS), the per-hit double arithmetic and the f32 decisions of
 * vr_query_transmittance_grad: it equals the gradient that query returns for the n * K rays (ray i, tmax = t[i][k],
 * weight[i][k]) up to the rounding of double sums. weight is n * K floats, row-major, or NULL (all ones). Samples <= 0 or
 * NaN and invalid rays contribute nothing. Every entry of grad is written; n == 0 zeroes it. grad == NULL, unknown flag
 * bits and the profile's argument errors: VR_ERR_INVALID.
 * Folding rule. One walk per ray; per (ray, Gaussian) hit, with a = max(0, t_enter), t1 = t_exit (f32) and the head of
 * vr_query_transmittance_grad (p, A, B, C, m, c, k, u_a) computed once, the K samples fall into three classes:
 *   t_k <= a, or not > 0:  nothing;
 *   t_k >= t1:             the whole chord, W_full += w_k;
 *   a < t_k < t1:          (S0, S1, S2) += w_k (J0, J1, J2) over [u_a, t_k - m], W_in += w_k;
 * then once (S0, S1, S2) += W_full (J0, J1, J2) over [u_a, t1 - m]. The hit's ten numbers are that query's with
 * (S0, S1, S2) for (J0, J1, J2) and weight 1; the exit's moving-bound term (t_exit <= t_k, the second class) carries
 * W_full, the entry's (t_enter > 0) carries W_full + W_in. So a hit costs ten atomic adds whatever K is.
 * The staging (80 bytes per Gaussian) is this query's own and is zeroed on `stream` by each call. */
vr_status vr_query_transmittance_profile_grad(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride,
                                              const float* weight, size_t n, uint32_t K, uint32_t flags, float* grad);
vr_status vr_query_transmittance_profile_grad_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride,
                                                     const float* d_weight, size_t n, uint32_t K, uint32_t flags,
                                                     float* d_grad, void* stream);

/* GaussianMixtureModel::evaluate_sigma (gmm.h:98-126) at n points xyz[3n], with `active` = the Gaussians
 * whose 3-sigma ellipsoid holds the point (p.(M p) - 9 <= 0 in f32, p = x - mean: the sign of
 * intersect_direct's C, gaussian.h:136, for a ray starting there), the set the integrators pass.
 * sigma_as[2i] = sigma_a, sigma_as[2i + 1] = sigma_s (both 0 when the summed mu_t is <= 0, gmm.h:115-118; no
 * clamp); n_active[i] (may be NULL) = the size of that set. The two sums are kept in double and rounded to
 * f32 once (the reference adds in f32 in scene order), so they do not depend on a visit order. */
vr_status vr_query_sigma(vr_ctx* ctx, const float* xyz, size_t n, float* sigma_as, uint32_t* n_active);
vr_status vr_query_sigma_device(vr_ctx* ctx, const float* d_xyz, size_t n, float* d_sigma_as, uint32_t* d_n_active,
                                void* stream);

/* The gradient of sigma at the points of vr_query_sigma, with respect to the Gaussians (albedo included) and to the
 * points themselves. weight_as[2n] = (w_a, w_s)_i is dL/d sigma_a and dL/d sigma_s at point i; NULL: every weight is
 * (1, 1), the gradient of sigma_t = sigma_a + sigma_s, whose albedo column is exactly 0.
 *   grad[11 g + k] = sum_i (w_a d sigma_a(x_i) + w_s d sigma_s(x_i)) / d theta_{g,k}
 * g the SCENE index and theta the vr_gaussian row in its own order: mean[3], cov[6] = {xx, xy, xz, yy, yz, zz}, density,
 * albedo (the order of vr_query_transmittance_grad, plus albedo). An off-diagonal cov component is the derivative with
 * respect to the stored number, 2 G_Sigma[i][j], as there. Every entry of grad (11 * num_primitives floats) is written;
 * a Gaussian holding no point gets eleven +0.
 *   grad_xyz[3 i + k] = (w_a d sigma_a + w_s d sigma_s)(x_i) / d x_{i,k}     (with NULL weights: grad sigma_t)
 * Either output may be NULL: grad == NULL is the gradient at the points alone (no staging, no atomic add); both NULL with
 * n > 0 is VR_ERR_INVALID. n == 0 is VR_OK: it zeroes grad if given and touches nothing else. The common errors above
 * apply (xyz == NULL with n > 0: VR_ERR_INVALID).
 * Definition. The function differentiated is sigma_s = sum alpha_g m_g, sigma_a = sum (1 - alpha_g) m_g over the active
 * set (what the forward's a_mix * sum and (1 - a_mix) * sum are, up to rounding). The active set is the forward query's
 * bit for bit: p.(M p) - 9 <= 0 in f32, in its arithmetic. The 3-sigma cut-off itself is not differentiated (a point on
 * it has measure zero). Per active (i, g), from the record's f32 mean, M, norm, rho, alpha and the point read as doubles:
 * p = x - mean, q = p.Mp, e = norm exp(-q / 2), m = rho e, c = w_a (1 - alpha) + w_s alpha, and
 *   g_mean += c m M p      G_M += -c m p p^T / 2      U += c e (the density component)
 *   g_albedo += (w_s - w_a) m      g_x(i) += -c m M p.
 * Per Gaussian, as for the optical depth: T = rho U, G_Sigma = -M G_M M - T M / 2 (the second term is the derivative of
 * norm through |Sigma|^(-1/2)).
 * A point whose double sum of m over its active set is <= 0 (non-positive densities only; the forward gives (0, 0)) and
 * a point with a non-finite coordinate (it lies in no box) contribute nothing and get a zero grad_xyz row. A point whose
 * child-pair walk is deeper than the builder allows (the forward's NaN) contributes nothing and gets a NaN row. (The
 * adds to grad happen while a point's walk runs; those of a point that turns out not to contribute are added again
 * with the opposite sign, so "nothing" holds to the rounding of a double sum.)
 * Arithmetic: the decisions are f32, everything on a decided (i, g) is double, the sums per Gaussian are double atomic
 * adds in arrival order, the sums per point stay in registers, and each result is rounded to f32 once. A result is
 * reproducible to the rounding of a double sum (grad_xyz bit for bit) and does not depend on VR_OPT_HALF_NODES /
 * VR_OPT_DEVICE_BVH beyond that. The staging (88 bytes per Gaussian) is the query's own and is zeroed on `stream` by
 * each call that asks for grad. */
vr_status vr_query_sigma_grad(vr_ctx* ctx, const float* xyz, const float* weight_as, size_t n, float* grad,
                              float* grad_xyz);
vr_status vr_query_sigma_grad_device(vr_ctx* ctx, const float* d_xyz, const float* d_weight_as, size_t n, float* d_grad,
                                     float* d_grad_xyz, void* stream);

/* The caller's own per-Gaussian vectors at n points xyz[3n]: features[N * C], row g (C floats) for SCENE Gaussian g
 * (emission, RGB, SH coefficients, semantic features, a temperature ...), passed per call, not part of the scene. Over
 * the active set A(x) of vr_query_sigma (the same f32 decision, the same walks: bit for bit the same set), with m_g the
 * f32 mu_t of vr_query_sigma:
 *   mass[i]        = f32( sum_{g in A} (double) m_g )                    (may be NULL)
 *   out[C i + c]   = f32( sum_{g in A} (double)(m_g * features[C g + c]) )   (one f32 multiply per term)
 *   n_active[i]    = |A|                                                  (may be NULL)
 * both sums in double, rounded to f32 once. A point whose summed m is <= 0 (non-positive densities only; vr_query_sigma's
 * (0, 0)) gets a +0 row and mass +0; a point whose child-pair walk is deeper than the builder allows (vr_query_sigma's
 * NaN) gets NaN in out and mass and n_active 0. Hence two exact ties: a channel whose features are all 1.0f has the bits
 * of mass; and with C = 1 and features = the albedos, a = out / mass (correctly rounded), sigma_s = a * mass,
 * sigma_a = (1 - a) * mass, (0, 0) where mass is not > 0, are vr_query_sigma's (sigma_a, sigma_s) bit for bit. A channel's
 * bits depend neither on C nor on the channel's place among the C. vr_query_sigma is the one-channel case.
 * C == 0, C > VR_FEATURES_MAX_CHANNELS, n * C >= 2^31 or num_primitives * C >= 2^31: VR_ERR_INVALID before anything is
 * launched; xyz, features or out NULL with n > 0: VR_ERR_INVALID; the common errors above apply. A scene without
 * Gaussians gives zeros. */
#define VR_FEATURES_MAX_CHANNELS 64   /* SH degree 3 x RGB = 48, with room; bounds the w/f row pass per hit */
vr_status vr_query_features(vr_ctx* ctx, const float* xyz, size_t n, const float* features, uint32_t C, float* out,
                            float* mass, uint32_t* n_active);
vr_status vr_query_features_device(vr_ctx* ctx, const float* d_xyz, size_t n, const float* d_features, uint32_t C,
                                   float* d_out, float* d_mass, uint32_t* d_n_active, void* stream);

/* The gradient of L = sum_i ( sum_c w_ic F_ic + u_i mass_i ), F = vr_query_features' out, with respect to the Gaussians,
 * the feature rows and the points. weights[n * C] = w (NULL: 1 everywhere), weight_mass[n] = u (NULL: 0).
 * Notation of vr_query_sigma_grad: per active (i, g), from the record's f32 numbers, the point, the row and the weights
 * read as doubles, p = x - mean, q = p.Mp, e = norm exp(-q / 2), m = rho e, and c = u_i + sum_c w_ic f_gc:
 *   grad[10 g + k]           d L / d (mean[3], cov[6] = {xx, xy, xz, yy, yz, zz}, density) of SCENE Gaussian g, the layout
 *                            of vr_query_transmittance_grad: mean: c m M p; cov: c m ((Mp)(Mp)^T - M) / 2, an
 *                            off-diagonal entry the derivative with respect to the stored number (twice that); density: c e
 *   grad_features[C g + c]   w_ic m
 *   grad_xyz[3 i + k]        -c m M p
 * summed over the active pairs of the points that contribute. Any output may be NULL (all three with n > 0:
 * VR_ERR_INVALID); every entry of a given output is written. grad_features == NULL runs without the feature staging and
 * its adds, grad == NULL without the other ten adds per pair, and grad_xyz alone without a single atomic add.
 * A point whose summed m is <= 0 and a point with a non-finite coordinate contribute nothing and get a +0 grad_xyz row; a
 * point whose child-pair walk is deeper than the builder allows contributes nothing and gets a NaN row (adds of a point
 * that turns out not to contribute are added again with the opposite sign, as in vr_query_sigma_grad). n == 0 is VR_OK:
 * it zeroes grad and grad_features if given and launches nothing. The other errors are vr_query_features'.
 * Arithmetic: the active set is the forward's f32 decision and is not differentiated; everything on a decided pair is
 * double; per Gaussian the sums are double atomic adds into staging rows (10 + C doubles per Gaussian, the query's own,
 * zeroed on `stream` by each call), staged per unit density (c e M p, -c e p p^T / 2, c e) and converted as
 * vr_query_transmittance_grad's are; the sums per point stay in registers; each result is rounded to f32 once.
 * Reproducible to the rounding of a double sum (grad_xyz bit for bit). Not differentiable a second time. */
vr_status vr_query_features_grad(vr_ctx* ctx, const float* xyz, size_t n, const float* features, uint32_t C,
                                 const float* weights, const float* weight_mass, float* grad, float* grad_features,
                                 float* grad_xyz);
vr_status vr_query_features_grad_device(vr_ctx* ctx, const float* d_xyz, size_t n, const float* d_features, uint32_t C,
                                        const float* d_weights, const float* d_weight_mass, float* d_grad,
                                        float* d_grad_features, float* d_grad_xyz, void* stream);

/* The emission-absorption sum along n rays, in one call: the caller's per-Gaussian rows (features[N * C], as for
 * vr_query_features) weighted by the mixture's m at the caller's K samples per ray, by the transmittance up to each sample
 * and by the caller's quadrature weights. t is the sample array of vr_query_transmittance_profile (n * K floats with
 * t_stride = K, or one shared row with t_stride = 0); q holds the quadrature weights in the same two layouts (q_stride 0
 * or K; NULL: all ones). The quadrature rule (midpoint, trapezoid, stratified ...) lives in t and q, not in the library.
 * Sample k of ray i is valid iff t_ik is finite and >= 0. Its point is x_ik = o_i + t_ik d_i, per component one f32
 * multiply and then one f32 add, never fused (the point numpy or torch compute from the f32 arrays); d is the direction
 * the walk uses (normalised once if unit == 0). With A(x) the active set of vr_query_sigma (the same f32 decision), m_g its
 * f32 mu_t and T_ik the f32 tr of vr_query_transmittance_profile for that ray and sample, all bit for bit:
 *   out[C i + c]  = f32( sum_{k valid} sum_{g in A(x_ik)} (double)q_ik (double)T_ik (double)m_g(x_ik) (double)f_gc )
 *   opacity[i]    = f32( the same sum without the f factor )            (may be NULL)
 *   tr[K i + k]   = the profile's tr for (ray i, t_ik), bit for bit      (may be NULL)
 *   n_pairs[i]    = sum_{k valid} |A(x_ik)|                              (may be NULL)
 * The sums are double (a Gaussian's samples are added first, then its term W f_gc, W = sum_k q T m, to each channel) and
 * each result is rounded to f32 once. tr is written for every sample, valid or not, by the profile's own rules (a sample
 * that is not > 0 has tr = 1). Terms exist only for active pairs: a sample in no ellipsoid contributes exactly nothing
 * whatever q is, and a row without pairs is +0. An invalid ray (the queries' rule) gets NaN in out, opacity and its tr
 * row, and 0 pairs. With q_k = the spacing of the samples, opacity is the Riemann sum of int T sigma_t dt = 1 - T(end).
 * Hence: a channel whose features are all 1.0f has the bits of opacity; a channel's bits depend neither on C nor on its
 * place among the C; n_pairs[i] is the sum of vr_query_features' n_active over ray i's valid sample points; tr is the
 * profile query's output.
 * One deliberate difference from composing vr_query_transmittance_profile and vr_query_features: the feature query zeroes
 * a point whose summed m is <= 0, which happens with non-positive densities only; this query does not apply that rule,
 * every active pair counts. With positive densities the two definitions coincide.
 * 1 <= K <= VR_PROFILE_MAX_SAMPLES, 1 <= C <= VR_FEATURES_MAX_CHANNELS, and n * K, n * C and num_primitives * C each
 * below 2^31; a t_stride or q_stride other than 0 and K; rays, t, features or out NULL with n > 0; a device ray array
 * that is not 16-byte aligned: VR_ERR_INVALID before anything is launched. The common errors above apply (a sphere
 * scene: VR_ERR_UNSUPPORTED; no scene: VR_ERR_NOSCENE). n == 0 is VR_OK and touches nothing. A scene without Gaussians
 * gives zeros and tr = 1.
 * Two passes on `stream`: the profile's walk writes tr (into a workspace of the query's own, n * K floats, when tr is
 * NULL: the only intermediate), then one walk per (ray, 8 channels) forms the sums. */
vr_status vr_query_radiance(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride, const float* q,
                            size_t q_stride, size_t n, uint32_t K, const float* features, uint32_t C, float* out,
                            float* opacity, float* tr, uint32_t* n_pairs);
vr_status vr_query_radiance_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride, const float* d_q,
                                   size_t q_stride, size_t n, uint32_t K, const float* d_features, uint32_t C,
                                   float* d_out, float* d_opacity, float* d_tr, uint32_t* d_n_pairs, void* stream);

/* The gradient of l = sum_i ( sum_c w_ic L_ic + u_i opacity_i ), L and opacity vr_query_radiance's out and opacity, with
 * respect to the Gaussians, the feature rows, the quadrature weights and the optical depths, in one fused call: a
 * (ray, Gaussian) pair sums its samples on chip and adds to the Gaussian's 10 + C sums once, and nothing of size n * K * C
 * or n * K * 3 exists. weights[n * C] = w (NULL: ones), weight_opacity[n] = u (NULL: zeros). rays, t, t_stride, q,
 * q_stride, n, K, features and C are vr_query_radiance's, and so are, bit for bit, the sample points x_ik, the validity of a
 * sample and the active set A(x_ik) (every active pair counts; there is no "summed m <= 0" rule).
 * T_ik is tr[K i + k], the tr the forward returned; tr == NULL: the profile's walk writes it into a workspace first, as the
 * forward does, and every output has the same bits either way.
 * Per active pair everything is double from the f32 record, point, row and weights: p = x_ik - mean, e = norm exp(-p.Mp / 2),
 * m = rho e (vr_query_features_grad's m, not the forward's f32 mu_t). With phi_ig = u_i + sum_c w_ic f_gc and a_ik = q_ik T_ik
 * (q == NULL: T_ik; an invalid sample: 0), and s_ik = sum_{g in A(x_ik)} m_g(x_ik) phi_ig:
 *   grad_q[K i + k]          f32( T_ik s_ik ) = d l / d q_ik (meaningful with q == NULL too)
 *   grad_tau[K i + k]        f32( -q_ik T_ik s_ik ) = d l / d tau_ik, tau the optical depth up to the sample
 *   grad_features[C g + c]   sum_i w_ic sum_k a_ik m_g(x_ik)
 *   grad[10 g + .]           d l / d (mean[3], cov[6], density) of SCENE Gaussian g, vr_query_transmittance_grad's layout:
 *                            sum_i phi_ig sum_k a_ik d m_g(x_ik) / d theta_g (vr_query_features_grad's three formulas with
 *                            c = a_ik phi_ig), plus exactly what vr_query_transmittance_profile_grad adds for the weights
 *                            grad_tau as rounded to f32, honouring flags (VR_GRAD_FROZEN_BOUNDS or 0). Both parts are
 *                            summed in one staging row per Gaussian and converted once: one rounding per output.
 * Any output may be NULL (all four with n > 0: VR_ERR_INVALID); every entry of a given output is written. What is not
 * asked for costs nothing: grad_q and / or grad_tau alone run one walk without a single atomic add and without the
 * profile gradient's pass; grad_features alone runs without the ten adds per pair and without that pass.
 * An invalid ray contributes nothing and gets NaN rows in grad_q and grad_tau; an invalid sample (t negative, NaN or
 * infinite) contributes nothing and gets +0, and so does a sample in no ellipsoid, whatever its q. n == 0 is VR_OK: it
 * zeroes grad and grad_features if given and launches nothing. A scene without Gaussians gives zeros. Argument errors are
 * vr_query_radiance's (features NULL with n > 0 among them), plus unknown flag bits: VR_ERR_INVALID before anything is
 * launched, the outputs untouched.
 * Passes on `stream`: the profile's walk (tr == NULL only); one walk per ray (a lane owns its ray's row of s, plain loads
 * and stores; per pair with an active sample 10 double atomic adds if grad is asked for and C if grad_features is); with
 * grad, the profile gradient's walk with grad_tau as weights into the same staging; one conversion per staging.
 * Workspaces, the query's own: s n * K doubles, tr and grad_tau n * K floats each when the caller gives none, staging
 * (10 + C) doubles per Gaussian. grad_q and grad_tau are reproducible bit for bit, grad and grad_features to the rounding
 * of a double sum. Not differentiable a second time; gradients with respect to origins, directions and t are not computed. */
vr_status vr_query_radiance_grad(vr_ctx* ctx, const vr_ray* rays, const float* t, size_t t_stride, const float* q,
                                 size_t q_stride, size_t n, uint32_t K, const float* features, uint32_t C,
                                 const float* weights, const float* weight_opacity, const float* tr, uint32_t flags,
                                 float* grad, float* grad_features, float* grad_q, float* grad_tau);
vr_status vr_query_radiance_grad_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_t, size_t t_stride,
                                        const float* d_q, size_t q_stride, size_t n, uint32_t K, const float* d_features,
                                        uint32_t C, const float* d_weights, const float* d_weight_opacity,
                                        const float* d_tr, uint32_t flags, float* d_grad, float* d_grad_features,
                                        float* d_grad_q, float* d_grad_tau, void* stream);

/* GaussianMixtureModel::intersect_events (gmm.h:457-515; tmax is not read): per ray the events of every
 * Gaussian it hits, an entry at t_enter (clamped to 0 for an origin inside) and an exit at t_exit, sorted by
 * t. Ray i's events are t[offsets[i] .. offsets[i + 1]) and ev[..] = scene_index << 1 | entering
 * (PrimitiveHitEvent{t, entering, index}); t is canonical (-0 is stored as +0). Events of one ray with equal
 * t come in scene order, a Gaussian's entry before its exit: deterministic and independent of the tree, but
 * NOT the order the reference's std::sort leaves them in (which depends on its BVH's traversal order); it
 * may change when the reference's tie order is settled. A ray with a non-finite origin or an unusable
 * direction has no events.
 * Two passes. Count: writes the n + 1 offsets and the total (= offsets[n]); it is synchronous (it waits for
 * the device's earlier work, whatever stream produced d_rays, and for its own, to return the total).
 * VR_ERR_INVALID if the total exceeds 2^32 - 1. Fill (asynchronous on `stream`): writes
 * the sorted events of the same rays; d_offsets must be the array that count call wrote and cap (the length
 * of d_t and d_ev) at least its total, VR_ERR_OVERFLOW otherwise (nothing is written); VR_ERR_INVALID if no
 * count call for n rays preceded it on this context. */
vr_status vr_query_events_count_device(vr_ctx* ctx, const vr_ray* d_rays, size_t n, uint32_t* d_offsets, uint64_t* total);
vr_status vr_query_events_fill_device(vr_ctx* ctx, const vr_ray* d_rays, size_t n, const uint32_t* d_offsets, float* d_t,
                                      uint32_t* d_ev, uint64_t cap, void* stream);
/* Host form, a two-call protocol as vr_get_fallback_pixels: *total is always set and offsets (n + 1 words, may
 * be NULL) filled whenever it is given. cap = 0 with t and ev NULL asks for those only (VR_OK). Otherwise t and
 * ev hold cap events each: with cap >= *total the events are written, with a smaller cap nothing is written to
 * t or ev and the call returns VR_ERR_OVERFLOW. */
vr_status vr_query_events(vr_ctx* ctx, const vr_ray* rays, size_t n, uint32_t* offsets, float* t, uint32_t* ev, uint64_t cap,
                          uint64_t* total);
/* One free-flight step (ABI 11): MultiScatterGaussians::get_free_flight_distance (integrator.h:422-498, the double
 * running sum over the ray's events) with solve_distance (distance_solvers.h:143-187) for ray i and the caller's
 * target optical depth tau_target[i]; the caller draws -log(1 - xi) itself, nothing here consumes random numbers.
 * With vr_query_transmittance (next-event estimation) and vr_query_sigma this is what a volumetric path tracer
 * over the uploaded scene needs. The sweep, the solvers and the albedo are the path kernels' own code, so every
 * discrete decision (segment, active list and its swap-remove order, solver branch) is taken in the exact forms a
 * VR_MULTI_SCATTER path's bounce takes it.
 *   t[i]        the collision distance, >= 0; -1 when the ray leaves the mixture before the running sum exceeds
 *               the target (:496-497) or has no events at all.
 *   albedo[i]   (may be NULL) evaluate_albedo (gmm.h:128-143) over the critical segment's active Gaussians at
 *               origin + t * direction, clamped to [0, 1] as :142 does; 0 when t < 0.
 *   n_active[i] (may be NULL) the size of that active set; 0 when t < 0.
 * Asking for albedo or n_active changes no bit of t. `unit` means what it means for the other queries; tmax is not
 * read. A ray with a non-finite origin, or a direction whose squared norm is 0, NaN or infinite in f32, gets NaN in
 * t and albedo and 0 in n_active, and so does a NaN target; every other target, <= 0 and +inf included (+inf: -1),
 * goes through the reference's own comparisons.
 * VR_OPT_FF_SOLVER 0-3 selects the solver as for frames; 4 (UNIFORM) is VR_ERR_UNSUPPORTED: it draws from a path's
 * seed, which a query does not have. VR_OPT_FF_WINDOW0 sizes the first hit window as for frames and changes no
 * result. VR_OPT_HALF_NODES / VR_OPT_DEVICE_BVH change the order in which Gaussians that enter at the same distance
 * join the active list, hence the order of f32 sums over it: t may move by rounding, nothing else.
 * Capacity: a ray on which more than 128 Gaussians overlap one point is run again with 1024-entry rows, as the
 * frames' fallback runs such paths; beyond 1024 the ray gets NaN in t and albedo (0 in n_active). The host form
 * then returns VR_ERR_OVERFLOW after writing every output of the batch; the device form reports the NaN only.
 * The query owns its scratch rows (sized as a free-flight frame's), so a frame queued on another stream is never
 * disturbed; the one-query-at-a-time rule above holds. */
vr_status vr_query_free_flight(vr_ctx* ctx, const vr_ray* rays, const float* tau_target, size_t n, float* t, float* albedo,
                               uint32_t* n_active);
vr_status vr_query_free_flight_device(vr_ctx* ctx, const vr_ray* d_rays, const float* d_tau_target, size_t n, float* d_t,
                                      float* d_albedo, uint32_t* d_n_active, void* stream);

/* Packs n rays from separate device arrays (origins[3n], directions[3n], tmax[n], or one tmax for all rays
 * with tmax_stride = 0, else 1) into vr_ray rows on the device. Asynchronous on `stream`. */
vr_status vr_query_pack_rays_device(vr_ctx* ctx, const float* d_origins, const float* d_directions, const float* d_tmax,
                                    uint32_t tmax_stride, size_t n, vr_ray* d_rays, void* stream);

/* ---------------- ray grids: radiance along the caller's own rays ---------------- */
/* A ray grid is a W x H image of rays, row-major: pixel (x, y) marches rays[y * W + x] (a vr_ray row; tmax is not
 * read) in place of the camera's ray. Everything else is the frame's, bit for bit: the step sequence t_k,
 * activation, scatter records, light and environment rays, the environment-sample key derive_path_seed(x, y, k)
 * of the pixel coordinates, the fallback / wide / deep passes, the exact slow path and band fix-ups, t_eps,
 * accumulation L + T env, the statistics and the retry of a frame that outgrew its record buffers. A grid filled
 * with a camera's own rays (vr_camera_sample_ray at ((x + 0.5f) / W, (y + 0.5f) / H) in f32, unit = 1) is that
 * camera's frame. The caller builds the rays: light probes inside the cloud, fisheye / equirectangular /
 * aspect-correct / distorted cameras, stereo pairs, a ray bundle a torch pipeline already holds on the device.
 * Integrators: VR_RAYMARCH_GAUSSIANS, VR_PURE_RAYMARCH, VR_RAYMARCH_SPHERES, VR_TEST_HITMASK. VR_FREE_FLIGHT and
 * VR_MULTI_SCATTER return VR_ERR_UNSUPPORTED: their samples jitter the sensor position inside the pixel, which a
 * fixed ray does not have, and no reference defines what a sample of a fixed ray would be.
 * rgb: 3 * W * H floats laid out as the full-frame render writes them. tr (may be NULL): W * H floats, the
 * transmittance left at the end of the primary march, the factor that multiplies the environment colour, so that
 * rgb - tr * env + tr * background composites over another background; asking for it changes no bit of rgb.
 * For VR_RAYMARCH_SPHERES it is the march's final T; for VR_TEST_HITMASK it is 0 where the ray hits a primitive
 * and 1 where it hits none. A ray that misses every primitive gets the environment colour exactly and tr = 1.
 * `unit` is honoured as the queries honour it: 0, the direction gets the Ray constructor's one normalisation;
 * non-zero, it is used as it stands and must be of unit length (the step table is sized in distances: a shorter
 * direction runs off its end, and those pixels are reported as error pixels). A ray with a non-finite origin, or a direction whose squared norm is 0, NaN or
 * infinite in f32, gets NaN in rgb and tr, spawns nothing and is counted nowhere (not in error_pixels: it is the
 * caller's input, not a capacity failure); the call still returns VR_OK.
 * The step table is sized from the rays, not from a camera: over the valid rays whose slab test hits the scene
 * bounds, the largest distance from a ray's origin to the farthest corner of the bounds, then the larger of that
 * and the bounds' diagonal, times 1.01 plus 1. VR_ERR_OVERFLOW, before anything is allocated, if that reach over
 * step_size exceeds 2^24 table entries (64 MB): a ray that starts 10^7 scene units away and hits the bounds.
 * VR_ERR_INVALID: a NULL pointer (tr excepted), width or height outside [1, 65535], a device ray array that is not
 * 16-byte aligned; otherwise the errors of a frame. VR_OPT_MARCH_BINNED is ignored (the bins are built from a
 * camera's tile frusta: grids always take the BVH march). On a vr_init_multi context the call runs on the first
 * device, as the queries do.
 * Host form: synchronous, copies in and out. Device form: d_rays, d_rgb, d_tr are device memory; the kernels
 * are queued on `stream` (a hipStream_t, NULL: the default stream) and the frame's outcome is reported by
 * vr_synchronize / vr_get_stats as for the tile entry point, but the call itself waits for `stream` once,
 * before the march is queued: the extent of the rays is reduced on the device and read back (4 bytes) to size
 * the step table, as the event count of the queries is. VR_TEST_HITMASK marches no table and does not wait. */
vr_status vr_render_rays(vr_ctx* ctx, const vr_ray* rays, uint32_t width, uint32_t height, const vr_render_params* p,
                         float* rgb_host, float* tr_host);
vr_status vr_render_rays_device(vr_ctx* ctx, const vr_ray* d_rays, uint32_t width, uint32_t height,
                                const vr_render_params* p, float* d_rgb, float* d_tr, void* stream);
/* Diagnostics (host only, no context): the extent the step table of a ray grid is sized from, for n rays and the
 * scene bounds [bounds_min, bounds_max] (vr_scene_info): the largest origin-to-farthest-corner distance over the
 * valid rays whose slab test hits the bounds; 0 if none does. */
vr_status vr_ray_grid_extent(const vr_ray* rays, size_t n, const float bounds_min[3], const float bounds_max[3],
                             float* extent);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* VR_HIP_H_ */
