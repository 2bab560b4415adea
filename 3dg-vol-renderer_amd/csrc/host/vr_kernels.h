// Kernel launchers the host files call (defined in kernels/*.hip; kernels/vr_lbvh.hip's is in ../vr_lbvh.h).
#pragma once
#include "vr_common.h"

namespace vr {

// kernels/vr_gauss_*.hip, a unit per pipeline stage (kernels/vr_gauss_common.h): march (gauss_march, gauss_bin,
// gauss_bin_scan), secondary (gauss_secondary), shade (gauss_accumulate, gauss_record_cut), tree (the others)
// (grid: a ray grid's rays and transmittance output, vr_render_rays; nullptr: a camera frame)
hipError_t gauss_march(const RenderArgs& A, hipStream_t stream, bool stats, const GridSrc* grid = nullptr);
hipError_t gauss_secondary(const RenderArgs& A, hipStream_t stream, bool stats);
hipError_t gauss_accumulate(const RenderArgs& A, hipStream_t stream, float* out_tr = nullptr);
hipError_t gauss_record_cut(const RenderArgs& A, float budget, hipStream_t stream);
hipError_t gauss_whiten(const GaussianRecord* rec, WRecord* out, uint32_t n, uint32_t* bad, hipStream_t stream);
hipError_t gauss_bin(const RenderArgs& A, bool emit, hipStream_t stream);
hipError_t gauss_parents(const HNode4* nodes, uint32_t n, int32_t* parent, int32_t* prim_node, hipStream_t stream);
hipError_t gauss_soa_nodes(const HNode4* src, HNode4* dst, uint32_t n, hipStream_t stream);
hipError_t gauss_refit_secondary(const HNode4* src, HNode4* dst, HNode4* dst_t, uint32_t n, const GaussianRecord* rec, const int32_t* parent,
                                 uint8_t* depth, float* nbox, uint32_t* maxd, const float hc[3], float hs, float diag,
                                 hipStream_t stream);
hipError_t gauss_bin_scan(const uint32_t* cnt, uint32_t* off, uint32_t n, void* tmp, size_t& tmp_bytes, hipStream_t stream);

// kernels/vr_freeflight.hip (per-path helpers and ff_bounce: kernels/vr_ff_bounce.h)
hipError_t launch_free_flight(const RenderArgs& A, uint32_t chunk_tiles, hipStream_t stream, hipEvent_t* ev);
uint32_t free_flight_threads(int cus);

// kernels/vr_loss.hip
// (partial: sfd_partial_count(npix, n) doubles of scratch, the per-chunk sums)
size_t sfd_partial_count(uint32_t npix, uint32_t n);
hipError_t launch_sfd_loss_diff(const uint32_t* bits0, const uint32_t* bits1, const float* lb, const float* lp, uint32_t npix,
                                uint32_t n, double* partial, double* out, hipStream_t stream);
hipError_t launch_pixel_losses(const float* img, const float* ref, uint32_t npix, float* out, hipStream_t stream);

// kernels/vr_query.hip
hipError_t query_transmittance(const RenderArgs& A, const vr_ray* rays, uint32_t n, float* tr, float* tau, uint32_t* next,
                               int refill, int cus, hipStream_t s);
hipError_t query_sigma(const RenderArgs& A, const float* xyz, uint32_t n, float* out, uint32_t* n_active, hipStream_t s);
hipError_t query_events_count(const RenderArgs& A, const vr_ray* rays, uint32_t n, uint32_t* counts, uint32_t* offsets,
                              unsigned long long* total, uint32_t* next, int refill, int cus, void* tmp, size_t& tmp_bytes,
                              hipStream_t s);
hipError_t query_events_fill(const RenderArgs& A, const vr_ray* rays, uint32_t n, const uint32_t* offsets, uint32_t total,
                             unsigned long long* keys, unsigned long long* keys2, float* t, uint32_t* ev, uint32_t* next,
                             int refill, int cus, void* tmp, size_t& tmp_bytes, hipStream_t s);
// (acc: 10 doubles per Gaussian of staging, zeroed by the call; grad: 10 floats per Gaussian)
hipError_t query_transmittance_grad(const RenderArgs& A, const vr_ray* rays, const float* weight, uint32_t n, bool moving,
                                    double* acc, float* grad, uint32_t* next, int refill, int cus, hipStream_t s);
// (the finish of the three gradients' staging rows, width 10 or 11 doubles per Gaussian -> as many floats; the profile
// gradient's unit calls it too)
hipError_t query_grad_finish(const RenderArgs& A, const double* acc, int width, float* grad, hipStream_t s);
// (out: one vr_ray_grad row per ray)
hipError_t query_transmittance_ray_grad(const RenderArgs& A, const vr_ray* rays, uint32_t n, bool moving, vr_ray_grad* out,
                                        uint32_t* next, int refill, int cus, hipStream_t s);
// (stage: 11 doubles per Gaussian of staging, zeroed by the call; grad: 11 floats per Gaussian; grad_xyz: 3 floats per
// point; either output may be nullptr, and without grad the staging is not touched)
hipError_t query_sigma_grad(const RenderArgs& A, const float* xyz, const float* weight_as, uint32_t n, double* stage, float* grad,
                            float* grad_xyz, hipStream_t s);
hipError_t query_pack_rays(const float* o, const float* d, const float* tmax, uint32_t tmax_stride, uint32_t n, vr_ray* rays,
                           hipStream_t s);

// kernels/vr_query_profile.hip
// (t: n * K samples with t_stride = K, or K with t_stride = 0; tr / tau: n * K floats, either may be nullptr; n * K < 2^31)
hipError_t query_transmittance_profile(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, uint32_t n,
                                       uint32_t K, float* tr, float* tau, uint32_t* next, int refill, int cus, hipStream_t s);
// (weight: n * K floats or nullptr; acc: 10 doubles per Gaussian of staging, zeroed by the call; grad: 10 floats per Gaussian)
hipError_t query_transmittance_profile_grad(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride,
                                            const float* weight, uint32_t n, uint32_t K, bool moving, double* acc, float* grad,
                                            uint32_t* next, int refill, int cus, hipStream_t s);
// (the same walk adding into staging rows the caller zeroed and finishes: the radiance gradient's second pass. n > 0)
hipError_t query_transmittance_profile_grad_add(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride,
                                                const float* weight, uint32_t n, uint32_t K, bool moving, double* acc,
                                                uint32_t* next, int refill, int cus, hipStream_t s);

// kernels/vr_query_features.hip
// (feat: C floats per scene Gaussian; out: n * C floats; mass, n_active: n each or nullptr. n > 0, 1 <= C, n * C < 2^31)
hipError_t query_features(const RenderArgs& A, const float* xyz, uint32_t n, const float* feat, uint32_t C, float* out, float* mass,
                          uint32_t* n_active, hipStream_t s);
// (weights: n * C floats or nullptr; weight_mass: n or nullptr; stage / fstage: 10 / C doubles per Gaussian of staging,
// zeroed by the call, each read only with its output; grad: 10 floats per Gaussian; grad_features: C per Gaussian; grad_xyz:
// 3 per point; any of the three may be nullptr)
hipError_t query_features_grad(const RenderArgs& A, const float* xyz, uint32_t n, const float* feat, uint32_t C,
                               const float* weights, const float* weight_mass, double* stage, double* fstage, float* grad,
                               float* grad_features, float* grad_xyz, hipStream_t s);
// (the finish of a feature staging, C doubles per Gaussian in tree order -> grad_features; the radiance gradient's too)
hipError_t query_features_finish(const RenderArgs& A, const double* fstage, uint32_t C, float* grad_features, hipStream_t s);

// kernels/vr_query_radiance.hip
// (t, q: n * K with stride K, or K with stride 0, q may be nullptr (ones); tr: n * K floats that query_transmittance_profile
// wrote earlier on s; feat: C floats per scene Gaussian; out: n * C floats; opacity, n_pairs: n each or nullptr. n > 0)
hipError_t query_radiance(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, const float* q,
                          uint32_t q_stride, uint32_t n, uint32_t K, const float* feat, uint32_t C, const float* tr, float* out,
                          float* opacity, uint32_t* n_pairs, uint32_t* next, int refill, int cus, hipStream_t s);

// kernels/vr_query_radiance_grad.hip
// (the inputs of query_radiance; weights: n * C or nullptr (ones); weight_opacity: n or nullptr (zeros); tr: n * K, the
// forward's. Workspaces: s_rows n * K doubles (not needed for grad_features alone), stage 10 and fstage C doubles per
// Gaussian (with grad / grad_features; zeroed by the call), tau_ws n * K floats (with grad and without grad_tau); next: three
// counter words. grad: 10 floats per Gaussian, grad_features: C per Gaussian, grad_q, grad_tau: n * K; any may be nullptr)
hipError_t query_radiance_grad(const RenderArgs& A, const vr_ray* rays, const float* t, uint32_t t_stride, const float* q,
                               uint32_t q_stride, uint32_t n, uint32_t K, const float* feat, uint32_t C, const float* weights,
                               const float* weight_opacity, const float* tr, bool moving, double* s_rows, double* stage,
                               double* fstage, float* tau_ws, float* grad, float* grad_features, float* grad_q, float* grad_tau,
                               uint32_t* next, int refill, int cus, hipStream_t s);

// kernels/vr_query_flight.hip (the sweep, the solvers and the albedo are the path kernels': kernels/vr_ff_bounce.h)
// (ctl: query_flight_ctl_words(n) words; A.ff_*: the scratch rows, sized as the free-flight frames size theirs)
size_t query_flight_ctl_words(uint32_t n);
hipError_t query_free_flight(const RenderArgs& A, const vr_ray* rays, const float* tau, uint32_t n, float* t, float* albedo,
                             uint32_t* n_active, uint32_t* ctl, hipStream_t s);

// kernels/vr_ray_extent.hip: *out = the bits of the largest distance from a ray's origin to the farthest corner of
// the box, over the valid rays that hit the box (0: none does)
hipError_t ray_extent(const vr_ray* rays, uint32_t n, const float bmin[3], const float bmax[3], uint32_t* out, hipStream_t s);

// kernels/vr_scene_dev.hip: the front of an upload from device arrays (vr_upload_gaussians_device)
// (rec, boxes (6 n), ext: in scene order; partials: scene_prepare_blocks(n) + 1 entries, the last one the scene's)
uint32_t scene_prepare_blocks(uint32_t n);
hipError_t scene_prepare(const float* mean, const float* cov6, const float* density, const float* albedo, uint32_t n, double K,
                         GaussianRecord* rec, float* boxes, float* ext, SceneStats* partials, hipStream_t s);
// (out[k]: the central-chord depth of Gaussian k * step along direction k & 3, NaN where the host loop skips it)
hipError_t scene_chord_samples(const GaussianRecord* rec, uint32_t n, uint32_t step, uint32_t count, double* out, hipStream_t s);
// (tmp == nullptr: sets tmp_bytes only)
hipError_t scene_sort_ext(const float* ext, float* sorted, uint32_t n, void* tmp, size_t& tmp_bytes, hipStream_t s);

// kernels/vr_spheres.hip
hipError_t launch_render(const RenderArgs& A, hipStream_t stream, int volume_type, int integrator, const GridSrc* grid = nullptr);
hipError_t launch_unshuffle(const float* slabs, uint32_t nslabs, uint32_t tiles_per_slab, uint32_t tiles_x, uint32_t W,
                            uint32_t H, float* img, hipStream_t stream);
hipError_t launch_unshuffle_part(const float* slabs, uint32_t first, uint32_t nslabs, uint32_t stride, uint32_t tiles_per_slab,
                                 uint32_t tiles_x, uint32_t W, uint32_t H, float* img, hipStream_t stream);

}  // namespace vr
