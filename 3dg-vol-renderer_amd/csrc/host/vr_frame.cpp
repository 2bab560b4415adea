// Frames: kernel arguments, the two pipelines (RayMarchingGaussians wavefront, free-flight), the frame report
// and its retry logic, the render entry points, statistics and debug read-back.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vr_ctx.h"

using namespace vr;

namespace {

// Farthest distance any ray can travel before leaving the scene box: the rays of both camera
// models start on the 2x2 sensor square position +- right +- up (camera.h:50,69).
float scene_tmax(const vr_ctx* c, const vr_camera* cam) {
    const float *bmin = c->scene.bmin, *bmax = c->scene.bmax;
    float best = 0.0f;
    for (int su = -1; su <= 1; su += 2)
        for (int sv = -1; sv <= 1; sv += 2) {
            float o[3];
            for (int k = 0; k < 3; ++k) o[k] = cam->position[k] + su * cam->right[k] + sv * cam->up[k];
            for (int cx = 0; cx < 2; ++cx)
                for (int cy = 0; cy < 2; ++cy)
                    for (int cz = 0; cz < 2; ++cz) {
                        float p[3] = {cx ? bmax[0] : bmin[0], cy ? bmax[1] : bmin[1], cz ? bmax[2] : bmin[2]};
                        double d = 0;
                        for (int k = 0; k < 3; ++k) d += (double)(p[k] - o[k]) * (p[k] - o[k]);
                        best = std::max(best, (float)std::sqrt(d));
                    }
        }
    return table_tmax(c, best);
}

// max_entries > 0 (ray grids, whose extent is the caller's): a table of more entries is refused before anything is
// allocated, and the doubling of a cached table stops there.
vr_status get_table(vr_ctx* c, float step, float tmax, const float** d, int* n, uint32_t max_entries = 0) {
    if (!(step > 0.0f) || !std::isfinite(step)) return fail(VR_ERR_INVALID, "step_size must be a positive finite float");
    if (max_entries > 0 && !((double)tmax / (double)step < (double)max_entries))
        return fail(VR_ERR_OVERFLOW, "the rays' extent over step_size needs a step table of more than " + std::to_string(max_entries) +
                                         " entries (move the ray origins closer to the scene, or enlarge step_size)");
    uint32_t key;
    std::memcpy(&key, &step, 4);
    auto it = c->tables.find(key);
    if (it == c->tables.end() || it->second.tmax < tmax) {
        float want = it == c->tables.end() ? tmax : std::max(tmax, 2.0f * it->second.tmax);
        if (max_entries > 0 && !((double)want / (double)step < (double)max_entries)) want = tmax;
        std::vector<float> t = step_table(step, want);
        if (t.back() <= tmax) return fail(VR_ERR_OVERFLOW, "step_size too small for the scene extent (float step sequence stalls)");
        vr_ctx::Table tb;
        tb.n = (int)t.size();
        tb.tmax = want;
        VR_TRY(tb.d.alloc(t.size(), "hipMalloc(step table)"));
        HIP_TRY(hipMemcpy(tb.d.get(), t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(step table)");
        it = c->tables.insert_or_assign(key, std::move(tb)).first;  // (a smaller table of this step is freed)
    }
    *d = it->second.d.get();
    *n = it->second.n;
    return VR_OK;
}

vr_status ensure_queue(vr_ctx* c, uint64_t pixels) {
    if (pixels + 1 > (uint64_t)c->queue_cap + 1 || !c->queue) {
        c->queue.reset();
        uint64_t cap = std::max<uint64_t>(pixels, 4096);
        if (cap > 0xffffffffull) return fail(VR_ERR_INVALID, "frame too large");
        VR_TRY(c->queue.alloc(cap + 1, "hipMalloc(queue)"));
        c->queue_cap = (uint32_t)cap;
    }
    return VR_OK;
}

}  // namespace

// Kernel arguments, in the three parts a frame is made of. fill_scene_args: the checks of the request and everything
// that does not depend on where the rays come from; the rays are a camera's (fill_args below) or a caller's grid
// (vr_rays.cpp), and either sizes the step table by its own extent (fill_table).
vr_status vr::fill_scene_args(vr_ctx* c, const vr_render_params* p, uint32_t W, uint32_t H, RenderArgs& A) {
    if (!c->has_scene) return fail(VR_ERR_NOSCENE, "no scene uploaded (call vr_upload_scene first)");
    if (!p) return fail(VR_ERR_INVALID, "NULL camera or params");
    if (W == 0 || H == 0 || W > 65535 || H > 65535) return fail(VR_ERR_INVALID, "width/height must be in [1, 65535]");
    if (p->flags != 0) return fail(VR_ERR_INVALID, "vr_render_params.flags must be 0");
    if ((p->integrator == VR_RAYMARCH_GAUSSIANS || p->integrator == VR_PURE_RAYMARCH) && c->type != VR_VOLUME_GAUSSIANS)
        return fail(VR_ERR_INVALID, "RayMarchingGaussians needs a Gaussian scene");
    if (p->integrator == VR_RAYMARCH_SPHERES && c->type != VR_VOLUME_SPHERES)
        return fail(VR_ERR_INVALID, "RayMarchingSpheres needs a sphere scene");
    const bool ff = p->integrator == VR_FREE_FLIGHT || p->integrator == VR_MULTI_SCATTER;
    if (p->integrator != VR_RAYMARCH_GAUSSIANS && p->integrator != VR_RAYMARCH_SPHERES && p->integrator != VR_TEST_HITMASK &&
        p->integrator != VR_PURE_RAYMARCH && !ff)
        return fail(VR_ERR_UNSUPPORTED, "integrator has no device implementation");
    if (ff && c->type != VR_VOLUME_GAUSSIANS)
        return fail(VR_ERR_INVALID, "free-flight integrators need a Gaussian scene (integrator.h:327 reads scene.gmm)");
    if (ff && p->num_samples <= 0) return fail(VR_ERR_INVALID, "num_samples must be > 0");
    if (ff && p->min_bounces < 0) return fail(VR_ERR_INVALID, "min_bounces must be >= 0");
    if (!ff && p->integrator != VR_TEST_HITMASK && p->env_samples < 0) return fail(VR_ERR_INVALID, "env_samples must be >= 0");
    if (!(p->t_eps >= 0.0f) || p->t_eps >= 1.0f) return fail(VR_ERR_INVALID, "t_eps must be in [0, 1)");
    std::memset(&A, 0, sizeof(A));
    A.width = W;
    A.height = H;
    A.tiles_x = (W + kTile - 1) / kTile;
    const SceneDev& sd = c->scene;
    A.gauss = sd.gauss.get();
    A.wrec = sd.wrec_pd ? sd.wrec.get() : nullptr;
    A.nodes = sd.nodes.get();
    // Invariant of both tree builders (upload_half_nodes, lbvh_build under `half`): hnodes and hnodes4 exist together
    // or not at all, so hnodes4 != nullptr alone says that the scene has its f16 trees (secondary_launch).
    A.hnodes = sd.hnodes.get();
    A.hnodes4 = sd.hnodes4.get();
    A.hnodes4s = sd.hnodes4s ? sd.hnodes4s.get() : sd.hnodes4.get();
    A.hnodes4t = sd.hnodes4s ? sd.hnodes4s.get() + sd.num_nodes4 : nullptr;  // (upload_secondary_tree: 2 n nodes)
    A.hnodes4w = sd.hnodes4w.get();
    A.hn4_parent = sd.parent4.get();
    A.prim_node4 = sd.prim_node4.get();
    A.num_nodes4 = (uint32_t)sd.num_nodes4;
    for (int k = 0; k < 3; ++k) A.hn_center[k] = sd.hn_center[k];
    A.hn_scale = sd.hn_scale;
    A.spheres = sd.spheres.get();
    A.num_prims = c->num_prims;
    A.bvh_depth = sd.bvh_depth;
    A.num_lights = (int32_t)c->lights.size();
    for (size_t l = 0; l < c->lights.size(); ++l) A.lights[l] = c->lights[l];
    for (int k = 0; k < 3; ++k) A.env[k] = c->env[k];
    A.step_size = p->step_size;
    A.env_samples = p->env_samples;
    A.t_eps = p->t_eps;
    A.pure = p->integrator == VR_PURE_RAYMARCH ? 1 : 0;
    A.chunk_rec = 64u;  // (env_order, env_base, rec_cut: set per frame by gauss_pipeline)
    A.chunk_shift = 6u;
    // Secondary-ray optical-depth cut-off. Exact mode (t_eps = 0): 104, where expf(-tau) is already
    // 0 in f32, so stopping is bit-neutral. With an early-out budget t_eps > 0 the cut-off is
    // ln(1/t_eps) + ln(1000): a dropped transmittance is <= 1e-3 * t_eps, a thousandth of the error
    // the primary early-out itself is allowed (DESIGN.md §Error budget).
    A.tau_cut = p->t_eps > 0.0f ? std::min(104.0f, (float)(std::log(1.0 / p->t_eps) + std::log(1000.0))) : 104.0f;
    if (ff) {
        A.ff_multi = p->integrator == VR_MULTI_SCATTER ? 1 : 0;
        A.ff_samples = p->num_samples;
        A.ff_n = (int32_t)std::sqrt((double)p->num_samples);  // int(std::sqrt(num_samples)), integrator.h:564
        A.ff_min_bounces = p->min_bounces;
        A.ff_max_bounces = 1 << 16;
        A.ff_solver = (int32_t)c->opt_ff_solver;
        A.ff_sm = c->opt_ff_kernel == 2 || (c->opt_ff_kernel == 0 && c->auto_ff_sm) ? 1 : 0;
    }
    A.counters = c->counters.get();
    A.gauss_order = sd.order.get();
    return VR_OK;
}

bool vr::needs_table(const vr_render_params* p) {
    return p->integrator == VR_RAYMARCH_GAUSSIANS || p->integrator == VR_PURE_RAYMARCH || p->integrator == VR_RAYMARCH_SPHERES;
}

// The step table of a ray-march frame whose rays travel at most tmax.
vr_status vr::fill_table(vr_ctx* c, const vr_render_params* p, float tmax, uint32_t max_entries, RenderArgs& A) {
    const float* d;
    int n;
    VR_TRY(get_table(c, p->step_size, tmax, &d, &n, max_entries));
    A.tsteps = d;
    A.num_tsteps = n;
    return VR_OK;
}

// Farthest a ray starting within `extent` of every corner of the scene box, or a secondary ray, travels in it.
float vr::table_tmax(const vr_ctx* c, float extent) {
    const float *bmin = c->scene.bmin, *bmax = c->scene.bmax;
    // secondary rays start inside the scene box: a Gaussian interval on them ends within one
    // box diagonal (PureRayMarching marches them over the same step table)
    double diag = 0.0;
    for (int k = 0; k < 3; ++k) diag += (double)(bmax[k] - bmin[k]) * (bmax[k] - bmin[k]);
    return std::max(extent, (float)std::sqrt(diag)) * 1.01f + 1.0f;
}

namespace {

vr_status fill_args(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, RenderArgs& A) {
    if (!c->has_scene) return fail(VR_ERR_NOSCENE, "no scene uploaded (call vr_upload_scene first)");
    if (!cam || !p) return fail(VR_ERR_INVALID, "NULL camera or params");
    if (W == 0 || H == 0 || W > 65535 || H > 65535) return fail(VR_ERR_INVALID, "width/height must be in [1, 65535]");
    if (cam->type != VR_CAMERA_PINHOLE && cam->type != VR_CAMERA_ORTHOGRAPHIC) return fail(VR_ERR_INVALID, "unknown camera type");
    VR_TRY(fill_scene_args(c, p, W, H, A));
    A.cam_type = cam->type;
    for (int k = 0; k < 3; ++k) {
        A.cam_pos[k] = cam->position[k];
        A.cam_view[k] = cam->view_dir[k];
        A.cam_right[k] = cam->right[k];
        A.cam_up[k] = cam->up[k];
        A.cam_pinhole[k] = cam->pinhole[k];
    }
    if (needs_table(p)) VR_TRY(fill_table(c, p, scene_tmax(c, cam), 0, A));
    return VR_OK;
}


// The environment rays' list filter (env_order_kernel, VR_OPT_SEC_FILTER) costs a pass over every environment ray's
// list and saves the persistent kernel the rays it filters. Measured on an MI355X against the parent commit
// (profiles/r08_c4_sec_filter_ab.json, kernel times of rocprofv3 --kernel-trace): per environment ray the pass costs
// 9 ps at C4, 18 ps at C2 (longer lists) and 6 ps at C3; per filtered ray the persistent kernel saves 32, 100 and
// 27 ps. The break-even share of filtered rays is their ratio: 0.29, 0.18, 0.23. C4 (share 0.53) and C3 (0.49) gain
// 4.5 and 0.6 ms a frame, C2 (0.065) lost 5.8 ms. Below a third, above the largest break-even, the filter is left out.
constexpr double kFilterMinShare = 1.0 / 3.0;
constexpr uint32_t kFilterProbe = 64;  // a context that leaves it out runs it again every so many frames (C2: + 0.1 ms a frame)

// RayMarchingGaussians: march (records) -> sizing / cut-offs -> secondary rays -> accumulate.
vr_status gauss_pipeline(vr_ctx* c, RenderArgs& A, hipStream_t s, bool stats, const GridSrc* grid) {
    const uint32_t npix = A.num_tiles * 256u;
    VR_TRY(c->px_first.grow(npix, "hipMalloc(px_first)", A.px_first));
    VR_TRY(c->px_T.grow(npix, "hipMalloc(px_T)", A.px_T));
    VR_TRY(c->rec_alloc.grow(4, "hipMalloc(rec_alloc)", A.rec_alloc));
    // PCG32 (rng.h:20-50, seq 1 -> inc 3) jump-ahead table for the environment samples
    if (c->pcg_jump_n < 2 * A.env_samples + 2) {
        const int n = 2 * A.env_samples + 2;
        std::vector<unsigned long long> tab(2 * (size_t)n);
        unsigned long long m = 1ull, a = 0ull;
        for (int k = 0; k < n; ++k) {
            tab[2 * k] = m;
            tab[2 * k + 1] = a;
            m *= 6364136223846793005ull;
            a = a * 6364136223846793005ull + 3ull;
        }
        VR_TRY(c->pcg_jump.grow(tab.size(), "hipMalloc(pcg)"));
        HIP_TRY(hipMemcpy(c->pcg_jump.get(), tab.data(), tab.size() * 8, hipMemcpyHostToDevice), "hipMemcpy(pcg)");
        c->pcg_jump_n = n;
    }
    A.pcg_jump = c->pcg_jump.get();
    VR_TRY(c->deep.grow((kDeepQueue + 1) * 4ull + (uint64_t)kActDeep * kDeepThreads * 4ull + (uint64_t)kActWide * kWideThreads * 4ull,
                           "hipMalloc(deep march)"));
    A.deepq = (uint32_t*)c->deep.get();
    A.deepq_cap = kDeepQueue;
    A.deep_act = (int32_t*)(A.deepq + kDeepQueue + 1);
    A.wide_act = A.deep_act + (size_t)kActDeep * kDeepThreads;
    A.wide_min = (uint32_t)c->opt_march_wide_min;
    A.march_big = c->march_big ? 1 : 0;

    // Tile bins of the binned march: count, scan, then (with one host sync for the entry count) emit.
    A.bin_off = A.bin_ent = nullptr;
    A.bin_cnt = A.bin_out = nullptr;
    if (c->opt_march_binned && A.num_prims > 0 && grid == nullptr) {  // (a ray grid has no tile frusta to bin by)
#ifndef VR_BIN_BUCKETS
#define VR_BIN_BUCKETS 256  // depth buckets per tile (a bucket's hits wait in a 16-entry per-lane list)
#endif
        const uint32_t nb = VR_BIN_BUCKETS, nbins = A.num_tiles * nb;
        VR_TRY(c->bin_cnt.grow((size_t)nbins + 1, "hipMalloc(bins)", A.bin_cnt));
        VR_TRY(c->bin_off.grow((size_t)nbins + 1, "hipMalloc(bins)"));
        A.bin_nb = nb;
        {  // depth buckets over [0, the farthest scene-box corner from any ray origin]
            float r = 0.0f, far = 0.0f;
            for (int k = 0; k < 3; ++k) r += std::fabs(A.cam_right[k]) + std::fabs(A.cam_up[k]);
            for (int cn = 0; cn < 8; ++cn) {
                float d2 = 0.0f;
                for (int k = 0; k < 3; ++k) {
                    const float v = ((cn >> k) & 1) ? c->scene.bmax[k] : c->scene.bmin[k];
                    d2 += (v - A.cam_pos[k]) * (v - A.cam_pos[k]);
                }
                far = std::max(far, std::sqrt(d2));
            }
            A.bin_dz = std::max((far + r) / (float)nb, 1e-6f);
        }
        HIP_TRY(hipMemsetAsync(A.bin_cnt, 0, (nbins + 1) * 4ull, s), "hipMemsetAsync(bins)");
        HIP_TRY(gauss_bin(A, false, s), "bin count");
        size_t tmp = 0;
        HIP_TRY(gauss_bin_scan(A.bin_cnt, c->bin_off.get(), nbins + 1, nullptr, tmp, s), "bin scan");
        // (the entries' buffer first serves as the scan's scratch)
        VR_TRY(c->bin_ent.grow_bytes(std::max<size_t>(tmp, 64), "hipMalloc(bin scan)"));
        HIP_TRY(gauss_bin_scan(A.bin_cnt, c->bin_off.get(), nbins + 1, c->bin_ent.get(), tmp, s), "bin scan");
        uint32_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, c->bin_off.get() + nbins, 4, hipMemcpyDeviceToHost, s), "bin total D2H");
        HIP_TRY(hipStreamSynchronize(s), "bin count");
        VR_TRY(c->bin_ent.grow(std::max<uint32_t>(total, 1), "hipMalloc(bin entries)"));
        A.bin_off = c->bin_off.get();
        A.bin_out = c->bin_ent.get();
        HIP_TRY(hipMemsetAsync(A.bin_cnt, 0, (nbins + 1) * 4ull, s), "hipMemsetAsync(bins)");
        HIP_TRY(gauss_bin(A, true, s), "bin emit");
        A.bin_ent = A.bin_out;
    }

    // Record capacity: from earlier frames of this context (hints), so the host never waits for
    // the march. A context's first frame sizes it: one host sync after the march, re-run with the
    // exact need if it did not fit. A later frame that outgrows the buffers is reported
    // (kRepExceeded) and the synchronous entry points render it again with grown buffers.
    const bool sized = c->rec_hint != 0;
    const uint32_t S = (uint32_t)(A.num_lights + A.env_samples);
    uint64_t cap = std::max<uint64_t>({c->rec_hint, 2ull * npix, 4096ull});
    // secondary-ray slots are 32-bit: a hint carried over from an earlier, larger frame (or one with
    // fewer samples per record) is clamped to what this frame's samples allow
    cap = std::min<uint64_t>(cap, std::max<uint64_t>(4096ull, (0xfffffffeull / std::max(S, 1u)) / 64 * 64 - 64));
    uint64_t ovf = std::max<uint64_t>({c->ovf_hint, cap, 4096ull});
    for (int attempt = 0;; ++attempt) {
        if (cap > 0xffffffffull / kActInline || ovf > 0xffffffffull - cap * kActInline || (cap + 63) / 64 * 64 * std::max(S, 1u) >= 0xffffffffull)
            return fail(VR_ERR_UNSUPPORTED, "too many scatter records in one call (split the frame)");
        VR_TRY(c->rec_pos.grow(cap, "hipMalloc(records)", A.rec_pos));
        VR_TRY(c->rec_meta.grow(cap, "hipMalloc(records)", A.rec_meta));
        VR_TRY(c->rec_next.grow(cap, "hipMalloc(records)", A.rec_next));
        VR_TRY(c->rec_bloom.grow(cap, "hipMalloc(record blooms)", A.rec_bloom));
        VR_TRY(c->rec_act.grow(cap * kActInline + ovf, "hipMalloc(active lists)", A.rec_act));
        A.rec_cap = (uint32_t)cap;
        A.act_ovf_cap = (uint32_t)ovf;
        HIP_TRY(hipMemsetAsync(A.rec_alloc, 0, 16, s), "hipMemsetAsync(rec_alloc)");
        HIP_TRY(hipMemsetAsync(c->queue.get(), 0, sizeof(uint32_t), s), "hipMemsetAsync(queue)");
        HIP_TRY(hipMemsetAsync(A.deepq, 0, sizeof(uint32_t), s), "hipMemsetAsync(deep queue)");
        HIP_TRY(gauss_march(A, s, stats, grid), "march");
        if (attempt == 0) HIP_TRY(hipEventRecord(c->ev_stage[0], s), "hipEventRecord");
        if (sized) break;
        HIP_TRY(hipMemcpyAsync(c->h_sizing.get(), A.rec_alloc, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "rec_alloc D2H");
        HIP_TRY(hipStreamSynchronize(s), "march");
        if (c->h_sizing[2] == 0) {
            c->rec_hint = std::max<uint64_t>(4096, (uint64_t)c->h_sizing[0] + c->h_sizing[0] / 8);
            c->ovf_hint = std::max<uint64_t>(c->ovf_hint, (uint64_t)c->h_sizing[1] + c->h_sizing[1] / 8);
            break;
        }
        if (attempt >= 3) return fail(VR_ERR_OVERFLOW, "scatter-record capacity could not be sized");
        cap = std::max<uint64_t>(2 * cap, (uint64_t)c->h_sizing[0] + c->h_sizing[0] / 4 + 1024);
        ovf = std::max<uint64_t>(2 * ovf, (uint64_t)c->h_sizing[1] + c->h_sizing[1] / 4 + 1024);
    }

    // Everything below is sized by the capacity; the kernels read the live record count on the device.
    // Tr slots: whole record chunks (<= 64 records; hand-out order, vr_gauss_common.h rays_per_chunk)
    VR_TRY(c->tr.grow(std::max<uint64_t>((cap + 63) / 64 * 64 * S, 1), "hipMalloc(secondary)", A.tr));
    VR_TRY(c->rec_rad.grow(std::max<uint64_t>(cap, 1), "hipMalloc(record radiance)", A.rec_rad));
    // exact slow path: light rays (stopping event / missed member), the rare rays with a member at its 3-sigma
    // boundary and those with a chord in the f32 error band (light or environment). Sized for every light ray plus
    // one more ray per record, or what earlier frames queued (+ 1/8); a frame that queues more (a boundary record's
    // environment rays can all go there) raises rec_alloc[2] and is rendered again with the grown queue
    const uint64_t nslow = std::min<uint64_t>(std::max<uint64_t>(cap * (uint64_t)A.num_lights + cap, c->slow_hint), 0xfffffffeull);
    VR_TRY(c->slowq.grow(nslow + 1, "hipMalloc(slow queue)", A.slowq));
    A.slowq_cap = (uint32_t)nslow;
    HIP_TRY(hipMemsetAsync(A.slowq, 0, sizeof(uint32_t), s), "hipMemsetAsync(slow queue)");
    {  // rays with one chord in the f32 error band (secondary_fix_kernel): one per record, or what earlier frames queued
        const uint64_t nfix = std::min<uint64_t>(std::max<uint64_t>(cap, c->fix_hint), 0x7ffffffeull / 3);
        VR_TRY(c->fixq.grow(3 * nfix + 1, "hipMalloc(band queue)", A.fixq));
        A.fixq_cap = (uint32_t)nfix;
        HIP_TRY(hipMemsetAsync(A.fixq, 0, sizeof(uint32_t), s), "hipMemsetAsync(band queue)");
    }
    VR_TRY(c->ray_next.grow(1, "hipMalloc(ray counter)", A.ray_next));
    {  // traversal-stack overflow of the persistent kernel: kWideStackMax entries for every lane it can keep resident
        const uint64_t lanes = (uint64_t)std::max(c->cus, 1) * 2048ull;  // 32 waves of 64 lanes per CU at most
        VR_TRY(c->stack_ovf.grow(lanes * kWideStackMax, "hipMalloc(stack overflow)", A.stack_ovf));
        A.stack_ovf_lanes = (uint32_t)lanes;
    }
    {  // per-pixel error budget of the secondary cut-off (record_cut_kernel): budget = t_eps, so the
       // secondary rays' truncation moves a pixel by at most t_eps, the same bound as the primary
       // early-out (error budget). t_eps = 0 (exact mode) keeps the bit-neutral 104.
        A.rec_cut = nullptr;
        if (c->opt_secondary_budget && A.t_eps > 0.0f) {
            VR_TRY(c->rec_cut.grow(cap, "hipMalloc(record cut-offs)", A.rec_cut));
            HIP_TRY(gauss_record_cut(A, A.t_eps, s), "record cut-offs");
        }
    }
    HIP_TRY(hipEventRecord(c->ev_stage[1], s), "hipEventRecord");
    A.rec_start = nullptr;  // per record: the 4-wide subtree its secondary rays walk first and its parent entry (record_start_kernel)
    if (A.hnodes4 != nullptr && A.hn4_parent != nullptr && c->opt_start_subtree) {
        VR_TRY(c->rec_start.grow(cap, "hipMalloc(record start nodes)", A.rec_start));
    }
    {  // environment rays traced in direction order within chunks of 32 records (see ray_slot; larger
       // chunks measured 2-20 % slower: record locality is lost)
        constexpr uint32_t shift = VR_CHUNK_SHIFT, cr = 1u << shift;  // entries hold record-in-chunk in 8 bits
        static_assert(VR_CHUNK_SHIFT <= 8, "environment-order entries and env_order_kernel hold record-in-chunk in 8 bits");
        A.env_order = nullptr;
        A.chunk_rec = cr;
        A.chunk_shift = shift;
        if (A.env_samples > 0 && A.env_samples <= kEnvOrderMax) {
            const uint64_t nch = (cap + cr - 1) / cr;
            VR_TRY(c->env_order.grow(nch * cr * (uint64_t)A.env_samples, "hipMalloc(environment-ray order)", A.env_order));
            VR_TRY(c->env_base.grow(nch * cr, "hipMalloc(environment generator states)", A.env_base));
            VR_TRY(c->env_count.grow(nch, "hipMalloc(environment-ray counts)", A.env_count));
            // the list filter runs the whitened list phase: RayMarchingGaussians on a scene with whitened records;
            // not on a context whose last filtered frame was below the break-even share, but for a probe now and then
            bool run = c->opt_sec_filter && A.wrec != nullptr && !A.pure;
            if (run && c->filter_low) {
                run = ++c->filter_skipped >= kFilterProbe;
                if (run) c->filter_skipped = 0;
            }
            A.sec_filter = run ? 1 : 0;
        }
        c->filter_ran = A.sec_filter != 0;
        c->last_env_samples = (uint32_t)A.env_samples;
    }
    HIP_TRY(gauss_secondary(A, s, stats), "secondary rays");
    HIP_TRY(hipEventRecord(c->ev_stage[2], s), "hipEventRecord");
    HIP_TRY(gauss_accumulate(A, s, grid ? grid->out_tr : nullptr), "accumulate");
    c->staged = true;
    c->report_gauss = true;
    c->report_pixels = (uint64_t)A.num_tiles * 256u;
    c->last_secondary_per_record = S;
    return VR_OK;
}

// Free-flight integrators: one persistent launch per chunk of tiles x batch of samples (at most
// kFFMaxPaths paths) on a grid of resident waves that claim 64-path groups from a counter, the
// launch's queued shadow rays (deferred NEE), then the paths' radiance is added to the pixels in
// sample order (vr_freeflight.hip; the bounce itself is vr_ff_bounce.h).
constexpr uint64_t kFFMaxPaths = 1ull << 23;
vr_status free_flight_pipeline(vr_ctx* c, RenderArgs& A, hipStream_t s) {
    const uint32_t spp = (uint32_t)A.ff_samples;
    const uint32_t nsb = (uint32_t)std::min<uint64_t>(spp, kFFMaxPaths / 256u);  // samples per launch
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(A.num_tiles, kFFMaxPaths / ((uint64_t)nsb * 256u));
    const uint64_t paths = (uint64_t)chunk * nsb * 256u;  // most paths of one launch
    // the persistent path kernel's resident grid (scratch rows per thread)
    const uint32_t threads = free_flight_threads(c->cus);
    VR_TRY(c->ff_scratch.grow((size_t)threads * (kFFHitCap + 2 * kFFActCap) * 16 + 64, "free-flight scratch"));
    VR_TRY(c->ff_tail.grow(paths, "free-flight paths", A.ff_tail));
    VR_TRY(c->ff_sum.grow((size_t)A.num_tiles * 256 * 3, "free-flight sums", A.ff_sum));
    {  // Deferred-NEE queue: VR_OPT_FF_NEE_QUEUE rays per path of a launch bound it; within that bound it is
       // sized from the need of this context's earlier frames (the most rays any launch queued, + 1/8;
       // never shrunk, like the record buffers, so a frame that fitted before fits again),
       // a first frame from the integrator (one shadow ray per bounce, min_bounces + 1 bounces before
       // Russian roulette). A launch that outgrows it is reported and the frame rendered again with a
       // grown queue (as the ray-march's record buffers), so frames never depend on the capacity.
        const uint64_t bound = std::min<uint64_t>(paths * (uint64_t)c->opt_ff_nee_queue, kFFNone);
        const uint64_t first = paths * (A.ff_multi ? (uint64_t)A.ff_min_bounces + 1ull : 1ull) + 4096ull;
        const uint64_t cap = c->nee_inline ? 0ull : std::min<uint64_t>(bound, c->nee_hint ? std::max<uint64_t>(c->nee_hint, 4096ull) : first);
        A.ff_nee_cap = (uint32_t)cap;
        c->last_nee_cap = (uint32_t)cap;
        c->last_nee_bound = (uint32_t)bound;
        if (cap > 0) {
            VR_TRY(c->ff_nee.grow((size_t)cap * 3, "free-flight shadow-ray queue", A.ff_nee));
        }
    }
    A.ff_nee_refill = c->auto_nee_refill;
    {  // paths over the hit-buffer capacity re-run in ff_fallback_kernel (queue + its own rows)
        const uint64_t qcap = paths;
        const uint64_t rows = (uint64_t)kFFBigThreads * 3ull * (uint64_t)kFFBigCap * 16ull;
        VR_TRY(c->ff_fb.grow(rows + (qcap + 1) * 4ull + 64, "free-flight fallback"));
        A.ff_big = (float4*)c->ff_fb.get();
        A.ff_fbq = (uint32_t*)(c->ff_fb.get() + rows);
        A.ff_fbq_cap = (uint32_t)qcap;
    }
    float4* base = (float4*)c->ff_scratch.get();
    A.ff_threads = threads;
    A.ff_hit_cap = kFFHitCap;
    A.ff_act_cap = kFFActCap;
    const int64_t w0 = c->opt_ff_window0 > 0 ? c->opt_ff_window0 : (int64_t)c->auto_window0;
    A.ff_hit_cap0 = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kFFHitCap, w0));
    A.ff_hit = base;
    A.ff_act0 = base + (size_t)kFFHitCap * threads;
    A.ff_act1 = base + (size_t)(kFFHitCap + kFFActCap) * threads;
    A.ff_next = (unsigned long long*)(base + (size_t)(kFFHitCap + 2 * kFFActCap) * threads);
    A.ff_nee_n = (uint32_t*)(A.ff_next + 1);
    c->ff_launches = 0;
    for (uint32_t t0 = 0; t0 < A.num_tiles; t0 += chunk) {
        const uint32_t nt = std::min(chunk, A.num_tiles - t0);
        for (uint32_t si = 0; si < spp; si += nsb) {
            A.ff_tile_base = t0;
            A.ff_si0 = si;
            A.ff_nsb = std::min(nsb, spp - si);
            A.ff_total = (unsigned long long)nt * A.ff_nsb * 256ull;
            const size_t e0 = 4 * (size_t)c->ff_launches;
            while (c->ff_ev.size() < e0 + 4) {
                Event e;
                HIP_TRY(hipEventCreate(e.put()), "hipEventCreate");
                c->ff_ev.push_back(std::move(e));
            }
            hipEvent_t ev[4] = {c->ff_ev[e0], c->ff_ev[e0 + 1], c->ff_ev[e0 + 2], c->ff_ev[e0 + 3]};
            HIP_TRY(launch_free_flight(A, nt, s, ev), "free-flight launch");
            ++c->ff_launches;
        }
    }
    return VR_OK;
}
}  // namespace

namespace vr {

// Collect the report of the last frame (waits for it). Grows the record capacity hints from its
// counts, so a frame that outgrew them renders correctly the next time.
vr_status collect(vr_ctx* c) {
    if (!c->stats_pending) return VR_OK;
    HIP_TRY(hipEventSynchronize(c->ev_report), "hipEventSynchronize");
    c->stats_pending = false;
    c->sync_pending = true;
    if (c->report_gauss) {
        const uint64_t nrec = c->h_report[kRepRecords], nact = c->h_report[kRepOverflowWords], nslow = c->h_report[kRepSlow];
        c->rec_hint = std::max<uint64_t>(c->rec_hint, nrec + nrec / 8);
        c->ovf_hint = std::max<uint64_t>(c->ovf_hint, nact + nact / 8);
        c->slow_hint = std::max<uint64_t>(c->slow_hint, nslow + nslow / 8);
        const uint64_t nfix = c->h_report[kRepFix];
        c->fix_hint = std::max<uint64_t>(c->fix_hint, nfix + nfix / 8);
        // >= 5 % of the pixels re-marched: the scene's active sets outgrow 16 slots; later frames march with
        // kActBig (same operations, so the frames are identical; kept until the next upload)
        if ((uint64_t)c->h_report[kRepFallback] * 20ull >= c->report_pixels && c->report_pixels > 0) c->march_big = true;
        if (c->filter_ran && c->h_report[kRepExceeded] == 0) {  // the list filter's share of the frame's environment rays
            const uint64_t env = nrec * c->last_env_samples;
            c->filter_low = (double)c->h_report[kRepFiltered] < kFilterMinShare * (double)env;
        }
    }
    if (c->report_ff && c->last_nee_bound > 0) {
        // a launch that found the queue full counted its paths' first refused claim only (they then
        // trace inline): grow at least twice over
        const uint64_t need = c->h_report[kRepNeeNeed];
        const bool over = need > c->last_nee_cap;
        c->nee_hint = std::max<uint64_t>({c->nee_hint, need + need / 8, over ? 2ull * c->last_nee_cap : 0ull});
        // full at the bound: a path that met it traced the rest inline and added them as one partial sum (float
        // association); the frame is rendered again with every shadow ray inline, which is the queued frame
        if (over && c->last_nee_cap >= c->last_nee_bound) c->nee_inline = true;
    }
    return VR_OK;
}

bool frame_exceeded(const vr_ctx* c) {
    if (c->report_gauss && c->h_report[kRepExceeded] != 0) return true;
    // the shadow-ray queue overflowed below its VR_OPT_FF_NEE_QUEUE bound: render again with a larger one
    // (or at it: the next frame traces inline, see nee_inline). A frame traced inline queues nothing.
    return c->report_ff && c->h_report[kRepNeeNeed] > c->last_nee_cap;
}

}  // namespace vr

vr_status vr::launch(vr_ctx* c, RenderArgs& A, const vr_render_params* p, hipStream_t s, bool stats, const GridSrc* grid) {
    VR_TRY(ensure_queue(c, (uint64_t)A.num_tiles * 256u));
    A.queue = c->queue.get();
    A.queue_cap = c->queue_cap;
    VR_TRY(collect(c));  // the previous report must land before the pinned buffer is reused
    c->sync_pending = false;  // vr_synchronize reports the last frame's outcome: this one's from here on
    HIP_TRY(hipMemsetAsync(c->queue.get(), 0, sizeof(uint32_t), s), "hipMemsetAsync(queue)");
    HIP_TRY(hipMemsetAsync(c->counters.get(), 0, 4 * sizeof(uint32_t), s), "hipMemsetAsync(counters)");
    HIP_TRY(hipEventRecord(c->ev_start, s), "hipEventRecord");
    c->staged = false;
    c->report_gauss = false;
    c->report_ff = false;
    c->ff_launches = 0;
    if (c->type == VR_VOLUME_GAUSSIANS && (p->integrator == VR_RAYMARCH_GAUSSIANS || p->integrator == VR_PURE_RAYMARCH)) {
        VR_TRY(gauss_pipeline(c, A, s, stats, grid));
    } else if (p->integrator == VR_FREE_FLIGHT || p->integrator == VR_MULTI_SCATTER) {
        VR_TRY(free_flight_pipeline(c, A, s));
        c->report_ff = true;
    } else {
        HIP_TRY(launch_render(A, s, c->type, p->integrator, grid), "kernel launch");
    }
    HIP_TRY(hipEventRecord(c->ev_stop, s), "hipEventRecord");
    auto report = [&](Report first, const uint32_t* src, size_t words) {
        return hipMemcpyAsync(&c->h_report[first], src, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    };
    HIP_TRY(report(kRepFallback, c->queue.get(), 1), "hipMemcpyAsync(report)");
    HIP_TRY(report(kRepErrors, c->counters.get(), 1), "hipMemcpyAsync(report)");
    if (c->report_gauss) {
        HIP_TRY(report(kRepRecords, A.rec_alloc, 3), "hipMemcpyAsync(report)");  // .. kRepExceeded
        HIP_TRY(report(kRepDeep, A.deepq, 1), "hipMemcpyAsync(report)");
        HIP_TRY(report(kRepSlow, A.slowq, 1), "hipMemcpyAsync(report)");
        HIP_TRY(report(kRepFix, A.fixq, 1), "hipMemcpyAsync(report)");
        HIP_TRY(report(kRepFiltered, A.rec_alloc + 3, 1), "hipMemcpyAsync(report)");
    }
    HIP_TRY(report(kRepFFFallback, c->counters.get() + 2, 2), "hipMemcpyAsync(report)");  // and kRepNeeNeed
    HIP_TRY(hipEventRecord(c->ev_report, s), "hipEventRecord");
    c->stats_pending = true;
    c->last_pixels = (int64_t)A.num_tiles * 256;
    c->last_first_tile = A.first_tile;
    c->last_tile_stride = A.tile_stride;
    c->last_tiles_x = A.tiles_x;
    c->last_w = A.width;
    c->last_h = A.height;
    return VR_OK;
}

// Synchronous frame into the context's device frame buffer (render_frame_device): a frame that outgrew
// the record buffers sized from earlier frames is rendered again with grown ones; pixels / paths over
// every per-ray capacity fail the call.
vr_status vr::render_sync(vr_ctx* c, RenderArgs& A, const vr_render_params* p, const GridSrc* grid) {
    struct Reported {  // every exit reports this frame's outcome itself: vr_synchronize must not report it again
        vr_ctx* c;
        ~Reported() { c->sync_pending = false; }
    } reported{c};
    for (int attempt = 1;; ++attempt) {
        VR_TRY(launch(c, A, p, c->stream, false, grid));
        VR_TRY(collect(c));
        if (!frame_exceeded(c)) break;
        if (attempt >= kFrameAttempts)
            return fail(VR_ERR_OVERFLOW, "scatter-record / shadow-ray queue capacity could not be sized");
    }
    if (c->h_report[kRepErrors] != 0)
        return fail(VR_ERR_OVERFLOW, std::to_string(c->h_report[kRepErrors]) + " pixels / paths exceeded a per-ray capacity (NaN)");
    return VR_OK;
}

namespace {

// The tiles first_tile, first_tile + tile_stride, ... (num_tiles >= 1 of them) lie in the W x H frame.
bool tiles_in_frame(uint32_t W, uint32_t H, uint32_t first_tile, uint32_t tile_stride, uint32_t num_tiles) {
    return tile_stride != 0 && num_tiles != 0 &&
           (uint64_t)first_tile + (uint64_t)(num_tiles - 1) * tile_stride < vr_num_tiles(W, H);
}

}  // namespace

// A full frame into the context's device frame buffer; slot 0/1 records RECORD_PIXEL_GAUSSIANS
// bitsets (MultiScatterGaussians only), slot -1 renders without recording.
vr_status vr::render_frame_device(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, int32_t slot) {
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    RenderArgs A;
    VR_TRY(fill_args(c, cam, p, W, H, A));
    const uint64_t npix = (uint64_t)W * H;
    if (slot >= 0) {
        const uint64_t words = std::max<uint64_t>(((uint64_t)c->num_prims + 31) / 32 * npix, 1);
        VR_TRY(c->rec_bits[slot].grow(words, "hipMalloc(pixel Gaussian bits)"));
        HIP_TRY(hipMemsetAsync(c->rec_bits[slot].get(), 0, words * 4, c->stream), "hipMemsetAsync(bits)");
        c->rec_npix[slot] = (uint32_t)npix;
        c->rec_n[slot] = (uint32_t)c->num_prims;
        A.rec_bits = c->rec_bits[slot].get();
        A.rec_npix = (uint32_t)npix;
    }
    if (npix * 3 > c->frame.count()) VR_TRY(c->frame.alloc(npix * 3, "hipMalloc(frame)"));  // exactly the largest frame so far
    A.first_tile = 0;
    A.tile_stride = 1;
    A.num_tiles = vr_num_tiles(W, H);
    A.packed = 0;
    A.out = c->frame.get();
    return render_sync(c, A, p);
}

extern "C" {

uint32_t vr_num_tiles(uint32_t W, uint32_t H) { return ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile); }

vr_status vr_render(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, float* rgb) {
    if (!c || !rgb) return fail(VR_ERR_INVALID, "vr_render: NULL argument");
    if (c->group) return vr::group_render(c->group, cam, p, W, H, rgb);
    VR_TRY(render_frame_device(c, cam, p, W, H, -1));
    HIP_TRY(hipMemcpy(rgb, c->frame.get(), (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(frame)");
    return VR_OK;
}

vr_status vr_render_tiles_device(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H,
                                 uint32_t first_tile, uint32_t tile_stride, uint32_t num_tiles, int32_t packed,
                                 float* d_out, void* stream) {
    c = first_device(c);
    if (!c || !d_out) return fail(VR_ERR_INVALID, "vr_render_tiles_device: NULL argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    RenderArgs A;
    VR_TRY(fill_args(c, cam, p, W, H, A));
    if (tile_stride == 0) return fail(VR_ERR_INVALID, "tile_stride must be >= 1");
    if (num_tiles == 0) return VR_OK;
    if (!tiles_in_frame(W, H, first_tile, tile_stride, num_tiles)) return fail(VR_ERR_INVALID, "tile range exceeds the frame");
    if (num_tiles >= (1u << 24)) return fail(VR_ERR_INVALID, "too many tiles in one call");
    A.first_tile = first_tile;
    A.tile_stride = tile_stride;
    A.num_tiles = num_tiles;
    A.packed = packed ? 1 : 0;
    A.out = d_out;
    return launch(c, A, p, (hipStream_t)stream);  // outcome: vr_synchronize / vr_get_stats
}

vr_status vr_count_work(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H,
                        uint32_t first_tile, uint32_t tile_stride, uint32_t num_tiles, uint64_t counts[16]) {
    c = first_device(c);
    if (!c || !counts) return fail(VR_ERR_INVALID, "vr_count_work: NULL argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    RenderArgs A;
    VR_TRY(fill_args(c, cam, p, W, H, A));
    if (p->integrator != VR_RAYMARCH_GAUSSIANS && p->integrator != VR_PURE_RAYMARCH && p->integrator != VR_FREE_FLIGHT &&
        p->integrator != VR_MULTI_SCATTER)
        return fail(VR_ERR_UNSUPPORTED, "vr_count_work: Gaussian ray-march and free-flight integrators only");
    if (!tiles_in_frame(W, H, first_tile, tile_stride, num_tiles)) return fail(VR_ERR_INVALID, "vr_count_work: bad tile range");
    DevBuf<float> d_out;
    DevBuf<unsigned long long> d_work;
    VR_TRY(d_out.alloc((size_t)num_tiles * 256 * 3, "hipMalloc(count_work out)"));
    VR_TRY(d_work.alloc(16, "hipMalloc(count_work)"));
    HIP_TRY(hipMemsetAsync(d_work.get(), 0, d_work.bytes(), c->stream), "hipMemsetAsync");
    A.first_tile = first_tile;
    A.tile_stride = tile_stride;
    A.num_tiles = num_tiles;
    A.packed = 1;
    A.out = d_out.get();
    A.work = d_work.get();
    vr_status st = VR_OK;
    unsigned long long h[16] = {0};
    for (int attempt = 0;; ++attempt) {  // a frame over the record capacity is counted again (grown)
        if (hipMemsetAsync(d_work.get(), 0, d_work.bytes(), c->stream) != hipSuccess) break;
        st = launch(c, A, p, c->stream, true);
        if (st == VR_OK) st = collect(c);
        if (st != VR_OK || !frame_exceeded(c) || attempt + 1 >= kFrameAttempts) break;
    }
    if (st == VR_OK) {
        hipError_t e = hipMemcpy(h, d_work.get(), sizeof(h), hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = hip_fail(e, "vr_count_work");
    }
    for (int i = 0; i < 16; ++i) counts[i] = h[i];
    return st;
}

vr_status vr_unshuffle_tiles_device(vr_ctx* c, const float* d_slabs, uint32_t nslabs, uint32_t tiles_per_slab, uint32_t W,
                                    uint32_t H, float* d_image, void* stream) {
    c = first_device(c);
    if (!c || !d_slabs || !d_image || nslabs == 0) return fail(VR_ERR_INVALID, "vr_unshuffle_tiles_device: bad argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(launch_unshuffle(d_slabs, nslabs, tiles_per_slab, (W + kTile - 1) / kTile, W, H, d_image, (hipStream_t)stream),
            "unshuffle launch");
    return VR_OK;
}

vr_status vr_unshuffle_tiles_part_device(vr_ctx* c, const float* d_slabs, uint32_t first, uint32_t nslabs, uint32_t stride,
                                         uint32_t tiles_per_slab, uint32_t W, uint32_t H, float* d_image, void* stream) {
    c = first_device(c);
    if (!c || !d_slabs || !d_image || nslabs == 0 || stride == 0 || (uint64_t)first + nslabs > stride)
        return fail(VR_ERR_INVALID, "vr_unshuffle_tiles_part_device: bad argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(launch_unshuffle_part(d_slabs, first, nslabs, stride, tiles_per_slab, (W + kTile - 1) / kTile, W, H, d_image,
                                  (hipStream_t)stream),
            "unshuffle launch");
    return VR_OK;
}

vr_status vr_render_record(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, float* rgb,
                           int32_t slot) {
    c = first_device(c);
    if (!c || !rgb || !p) return fail(VR_ERR_INVALID, "vr_render_record: NULL argument");
    if (slot != 0 && slot != 1) return fail(VR_ERR_INVALID, "vr_render_record: slot must be 0 or 1");
    if (p->integrator != VR_MULTI_SCATTER)
        return fail(VR_ERR_INVALID, "vr_render_record: MultiScatterGaussians only (integrator.h:532-536)");
    VR_TRY(render_frame_device(c, cam, p, W, H, slot));
    HIP_TRY(hipMemcpy(rgb, c->frame.get(), (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(frame)");
    return VR_OK;
}

vr_status vr_get_pixel_gaussians(vr_ctx* c, int32_t slot, uint32_t* bits, size_t n_words) {
    c = first_device(c);
    if (!c || !bits || (slot != 0 && slot != 1)) return fail(VR_ERR_INVALID, "vr_get_pixel_gaussians: bad argument");
    const size_t need = (size_t)((c->rec_n[slot] + 31) / 32) * c->rec_npix[slot];
    if (!c->rec_bits[slot] || c->rec_npix[slot] == 0) return fail(VR_ERR_INVALID, "slot holds no recording");
    if (n_words != need) return fail(VR_ERR_INVALID, "n_words must be ceil(N/32) * W * H = " + std::to_string(need));
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(bits, c->rec_bits[slot].get(), need * 4, hipMemcpyDeviceToHost), "hipMemcpy(bits)");
    return VR_OK;
}

vr_status vr_get_fallback_pixels(vr_ctx* c, uint32_t* xy, size_t cap, size_t* n) {
    c = first_device(c);
    if (!c || !n || (cap > 0 && !xy)) return fail(VR_ERR_INVALID, "vr_get_fallback_pixels: bad argument");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    VR_TRY(collect(c));
    const size_t count = std::min<size_t>(c->h_report[kRepFallback], c->queue_cap);
    *n = count;
    if (count == 0 || cap == 0) return VR_OK;
    std::vector<uint32_t> q(std::min(count, cap));
    HIP_TRY(hipMemcpy(q.data(), c->queue.get() + 1, q.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(queue)");
    for (size_t i = 0; i < q.size(); ++i) {  // tile_pixel (kernels/vr_dev_common.h): tile-local id << 8 | lane
        const uint32_t lane = q[i] & 255u, wv = lane >> 6, ln = lane & 63u;
        const uint32_t tile = c->last_first_tile + (q[i] >> 8) * c->last_tile_stride;
        xy[2 * i] = (tile % c->last_tiles_x) * kTile + (wv & 1u) * 8u + (ln & 7u);
        xy[2 * i + 1] = (tile / c->last_tiles_x) * kTile + (wv >> 1) * 8u + (ln >> 3);
    }
    return VR_OK;
}

vr_status vr_debug_pixel_records(vr_ctx* c, uint32_t x, uint32_t y, float* out, size_t cap, size_t row_in, size_t* n,
                                 size_t* row_out) {
    c = first_device(c);
    if (!c || !n || (cap > 0 && !out)) return fail(VR_ERR_INVALID, "vr_debug_pixel_records: bad argument");
    if (!c->report_gauss) return fail(VR_ERR_INVALID, "vr_debug_pixel_records: the last frame was not a ray-march frame");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    VR_TRY(collect(c));
    // the pixel's tile-local index (vr_dev_common.h tile_pixel: wave = 8x8 quadrant, lane row-major)
    const uint32_t tx = x / kTile, ty = y / kTile, g = ty * c->last_tiles_x + tx;
    if (x >= c->last_w || y >= c->last_h || g < c->last_first_tile || (g - c->last_first_tile) % c->last_tile_stride)
        return fail(VR_ERR_INVALID, "vr_debug_pixel_records: pixel not rendered by the last frame");
    const uint32_t lx = x % kTile, ly = y % kTile;
    const uint32_t lane = ((lx >> 3) + 2u * (ly >> 3)) * 64u + (ly & 7u) * 8u + (lx & 7u);
    const uint32_t p = ((g - c->last_first_tile) / c->last_tile_stride) * 256u + lane;
    const uint32_t nl = (uint32_t)c->lights.size(), S = c->last_secondary_per_record, ne = S - nl, cr = 1u << VR_CHUNK_SHIFT;
    const size_t row = 9 + S;
    if (row_out) *row_out = row;
    if (cap > 0 && row_in != row)
        return fail(VR_ERR_INVALID, "vr_debug_pixel_records: rows of " + std::to_string(row_in) + " floats, the frame's are " +
                                        std::to_string(row) + " (9 + lights + env_samples)");
    uint32_t r = 0;
    HIP_TRY(hipMemcpy(&r, c->px_first.get() + p, 4, hipMemcpyDeviceToHost), "hipMemcpy");
    size_t k = 0;
    std::vector<uint16_t> ord(cr * ne);
    for (; r != kNoRecord; ++k) {
        float4 pos, rad;
        uint4 meta;
        uint32_t next = kNoRecord;
        HIP_TRY(hipMemcpy(&pos, c->rec_pos.get() + r, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        HIP_TRY(hipMemcpy(&meta, c->rec_meta.get() + r, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        HIP_TRY(hipMemcpy(&rad, c->rec_rad.get() + r, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        HIP_TRY(hipMemcpy(&next, c->rec_next.get() + r, 4, hipMemcpyDeviceToHost), "hipMemcpy");
        if (k < cap) {
            float* o = out + k * row;
            const float v[9] = {(float)meta.y, pos.x, pos.y, pos.z, pos.w, rad.x, rad.y, rad.z, (float)(meta.w & 0x7fffffffu)};
            std::copy(v, v + 9, o);
            // Tr slots: hand-out order within the record's chunk (vr_gauss_common.h ray_slot / rays_per_chunk)
            const uint32_t chunk = r / cr, rl = r % cr;
            const size_t base = (size_t)chunk * cr * S;
            if (ne > 0 && c->env_order)
                HIP_TRY(hipMemcpy(ord.data(), c->env_order.get() + (size_t)chunk * cr * ne, ord.size() * 2,
                                  hipMemcpyDeviceToHost), "hipMemcpy");
            for (uint32_t s = 0; s < S; ++s) {
                size_t rem = 0;
                if (s < nl) rem = (size_t)s * cr + rl;
                else if (c->env_order) {
                    const uint16_t want = (uint16_t)((rl << 8) | (s - nl));
                    rem = (size_t)nl * cr + (size_t)(std::find(ord.begin(), ord.end(), want) - ord.begin());
                } else rem = (size_t)s * cr + rl;
                HIP_TRY(hipMemcpy(o + 9 + s, c->tr.get() + base + rem, 4, hipMemcpyDeviceToHost), "hipMemcpy");
            }
        }
        r = next;
    }
    *n = k;
    return VR_OK;
}

vr_status vr_get_stats(vr_ctx* c, vr_render_stats* o) {
    if (!c || !o) return fail(VR_ERR_INVALID, "vr_get_stats: NULL argument");
    if (c->group) return vr::group_stats(c->group, o);
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    VR_TRY(collect(c));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_start, c->ev_stop), "hipEventElapsedTime");
    o->kernel_ms = ms;
    o->pixels = c->last_pixels;
    o->fallback_pixels = !c->report_gauss && c->ff_launches > 0 ? c->h_report[kRepFFFallback] : c->h_report[kRepFallback];
    o->error_pixels = c->h_report[kRepErrors];
    for (double& v : o->stage_ms) v = 0.0;
    if (c->staged) {
        hipEvent_t b[5] = {c->ev_start, c->ev_stage[0], c->ev_stage[1], c->ev_stage[2], c->ev_stop};
        for (int i = 0; i < 4; ++i) {
            float m = 0.0f;
            HIP_TRY(hipEventElapsedTime(&m, b[i], b[i + 1]), "hipEventElapsedTime");
            o->stage_ms[i] = m;
        }
    }
    if (!c->report_gauss && c->ff_launches > 0) {  // free-flight: [0] path kernel, [2] shadow rays, [3] accumulation
        for (uint32_t l = 0; l < c->ff_launches; ++l) {
            const Event* e = &c->ff_ev[4 * (size_t)l];
            float m[3] = {0.0f, 0.0f, 0.0f};
            for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&m[i], e[i], e[i + 1]), "hipEventElapsedTime");
            o->stage_ms[0] += m[0];
            o->stage_ms[2] += m[1];
            o->stage_ms[3] += m[2];
        }
    }
    o->scatter_records = c->report_gauss ? (int64_t)c->h_report[kRepRecords] : 0;
    o->secondary_rays = o->scatter_records * (int64_t)c->last_secondary_per_record;
    o->record_overflow = frame_exceeded(c) ? 1 : 0;
    o->deep_pixels = c->report_gauss ? (int64_t)std::min(c->h_report[kRepDeep], kDeepQueue) : 0;
    o->slow_rays = c->report_gauss ? (int64_t)c->h_report[kRepSlow] : 0;
    o->band_rays = c->report_gauss ? (int64_t)c->h_report[kRepFix] : 0;
    o->filtered_rays = c->report_gauss ? (int64_t)c->h_report[kRepFiltered] : 0;
    return VR_OK;
}

}  // extern "C"
