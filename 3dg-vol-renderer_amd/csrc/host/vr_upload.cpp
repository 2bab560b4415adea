// Scene upload: BVH build (host binned SAH, or the device builder's hand-over) and the scene's HBM layout —
// records, whitened records, the child-pair / half-precision / 4-wide trees, parents and the secondary rays'
// refit tree — plus the per-scene heuristics of the free-flight kernels.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <bit>
#include <cmath>
#include <cstring>
#include <numbers>
#include <vector>

#include "vr_ctx.h"
#include "../vr_lbvh.h"

using namespace vr;

namespace {

GaussianRecord pack_record(const GaussianPre& p) {
    return GaussianRecord{p.mean[0], p.mean[1], p.mean[2], p.density, p.inv_cov[0], p.inv_cov[1], p.inv_cov[2],
                          p.inv_cov[3], p.inv_cov[4], p.inv_cov[5], p.norm, p.albedo};
}

// ---- half-precision node copy for the secondary rays ----
uint16_t f16_bits(_Float16 h) { return std::bit_cast<uint16_t>(h); }
double f16_to_double(uint16_t b) { return (double)std::bit_cast<_Float16>(b); }
uint16_t f16_step(uint16_t h, bool up) {  // next representable half toward +inf (up) or -inf
    const bool neg = h & 0x8000u;
    if ((h & 0x7fffu) == 0) return up ? 0x0001u : 0x8001u;
    return (uint16_t)((neg != up) ? h + 1 : h - 1);
}
uint16_t f16_directed(double v, bool up) {  // smallest half >= v (up) / largest half <= v
    if (std::isinf(v)) return v > 0 ? 0x7c00u : 0xfc00u;
    uint16_t h = f16_bits((_Float16)v);  // nearest, then stepped outward
    if (up) {
        while (f16_to_double(h) < v) h = f16_step(h, true);
    } else {
        while (f16_to_double(h) > v) h = f16_step(h, false);
    }
    return h;
}

// The half-precision trees' normalisation (hn_center, hn_scale: the scene box onto [-1, 1]) and whether the
// scene suits them: f16 keeps ~11 bits, so boxes widen by up to ~1e-3 of the scene's half extent; scenes
// whose boxes are small against that (median of `ext`, the largest extent of every leaf box, under 3 % of
// the half extent) keep the f32 nodes only. Reorders `ext`.
// (half_tree_norm: the normalisation and the half extent it rests on; false: no half trees whatever `ext` holds)
bool half_tree_norm(vr_ctx* c, double& half) {
    SceneDev& s = c->scene;
    half = 0.0;
    for (int k = 0; k < 3; ++k) {
        s.hn_center[k] = 0.5f * (s.bmin[k] + s.bmax[k]);
        half = std::max(half, 0.5 * ((double)s.bmax[k] - (double)s.bmin[k]));
    }
    if (!c->opt_half_nodes || !(half > 0.0) || !std::isfinite(half)) return false;
    s.hn_scale = (float)(1.0 / half);
    return true;
}
bool half_tree_rule(vr_ctx* c, std::vector<float>& ext) {
    double half;
    if (!half_tree_norm(c, half)) return false;
    if (ext.empty()) return true;
    std::nth_element(ext.begin(), ext.begin() + ext.size() / 2, ext.end());
    return ext[ext.size() / 2] >= 0.03 * half;
}

// Builds the 32-B half-precision node copy (HNode) and its 4-wide collapse when the scene suits them
// (half_tree_rule on the leaf boxes).
vr_status upload_half_nodes(vr_ctx* c, const std::vector<BVHNode>& nodes) {
    SceneDev& s = c->scene;
    s.hnodes.reset();
    s.hnodes4.reset();
    s.hnodes4s.reset();
    s.hnodes4w.reset();
    if (!c->opt_half_nodes) return VR_OK;
    std::vector<float> leaf_ext;
    for (const BVHNode& n : nodes)
        for (int side = 0; side < 2; ++side)
            if (n.c[side] < 0) {
                float e = 0.0f;
                for (int k = 0; k < 3; ++k) e = std::max(e, n.f[6 * side + 3 + k] - n.f[6 * side + k]);
                leaf_ext.push_back(e);
            }
    if (!half_tree_rule(c, leaf_ext)) return VR_OK;
    std::vector<HNode> hn(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        for (int side = 0; side < 2; ++side) {
            for (int k = 0; k < 3; ++k) {
                const float lo = nodes[i].f[6 * side + k], hi = nodes[i].f[6 * side + 3 + k];
                const double ulo = std::isinf(lo) ? (double)lo : ((double)lo - s.hn_center[k]) * (double)s.hn_scale;
                const double uhi = std::isinf(hi) ? (double)hi : ((double)hi - s.hn_center[k]) * (double)s.hn_scale;
                hn[i].h[6 * side + k] = f16_directed(ulo, false);
                hn[i].h[6 * side + 3 + k] = f16_directed(uhi, true);
            }
            hn[i].c[side] = nodes[i].c[side];
        }
    }
    VR_TRY(s.hnodes.alloc(hn.size(), "hipMalloc(half nodes)"));
    HIP_TRY(hipMemcpy(s.hnodes.get(), hn.data(), hn.size() * sizeof(HNode), hipMemcpyHostToDevice), "hipMemcpy(half nodes)");

    // 4-wide collapse for the secondary rays: a pair node's two children, then repeatedly the
    // inner child with the largest box surface replaced by its own two children, up to 4.
    struct Kid {
        int side;      // box source: nodes[pair].f[6 side ..]
        int32_t pair;  // pair node holding this child's box
        int32_t ref;   // the child's ref in the pair tree
    };
    auto area = [&](const Kid& k) {
        const float* f = &nodes[k.pair].f[6 * k.side];
        const float d0 = f[3] - f[0], d1 = f[4] - f[1], d2 = f[5] - f[2];
        return d0 * d1 + d0 * d2 + d1 * d2;
    };
    std::vector<HNode4> w4;
    std::vector<std::pair<int32_t, int32_t>> todo{{0, 0}};  // (pair node, HNode4 slot)
    w4.emplace_back();
    while (!todo.empty()) {
        const auto [pn, slot] = todo.back();
        todo.pop_back();
        Kid kids[4];
        int nk = 0;
        for (int side = 0; side < 2; ++side)
            if (nodes[pn].c[side] != 0) kids[nk++] = Kid{side, pn, nodes[pn].c[side]};
        for (;;) {
            int best = -1;
            float best_a = -1.0f;
            for (int i = 0; i < nk; ++i)
                if (kids[i].ref > 0) {
                    const int extra = (nodes[kids[i].ref].c[0] != 0) + (nodes[kids[i].ref].c[1] != 0) - 1;
                    if (nk + extra <= 4 && area(kids[i]) > best_a) {
                        best_a = area(kids[i]);
                        best = i;
                    }
                }
            if (best < 0) break;
            const int32_t inner = kids[best].ref;
            Kid repl[2];
            int nr = 0;
            for (int side = 0; side < 2; ++side)
                if (nodes[inner].c[side] != 0) repl[nr++] = Kid{side, inner, nodes[inner].c[side]};
            kids[best] = repl[0];
            if (nr == 2) kids[nk++] = repl[1];
        }
        HNode4 h{};
        for (int i = 0; i < 4; ++i) {
            if (i >= nk) {
                for (int k = 0; k < 6; ++k) h.h[i][k] = 0x7e00u;  // NaN box: no slab test reports a hit
                h.c[i] = 0;
                continue;
            }
            for (int k = 0; k < 6; ++k) h.h[i][k] = hn[kids[i].pair].h[6 * kids[i].side + k];
            if (kids[i].ref < 0) {
                h.c[i] = kids[i].ref;
            } else {
                h.c[i] = (int32_t)w4.size();
                w4.emplace_back();
                todo.push_back({kids[i].ref, h.c[i]});
            }
        }
        w4[slot] = h;
    }
    VR_TRY(s.hnodes4.alloc(w4.size(), "hipMalloc(wide nodes)"));
    HIP_TRY(hipMemcpy(s.hnodes4.get(), w4.data(), w4.size() * sizeof(HNode4), hipMemcpyHostToDevice), "hipMemcpy(wide nodes)");
    s.num_nodes4 = w4.size();
    return VR_OK;
}

// Scenes at least this large may use the device builder (VR_OPT_DEVICE_BVH); smaller ones build on
// the host in well under a millisecond.
constexpr size_t kDeviceBvhMin = 256;

// Whitened record copy for the secondary rays (WRecord), converted on the device from the records.
// A record whose f32 inverse covariance is not positive definite (a nearly singular covariance) has no
// Cholesky factor: such a scene's secondary rays use the records' M forms instead (wrec_pd = false,
// secondary_ww_kernel's M-form variant), as the reference's intersect_direct / optical_depth take any M.
vr_status upload_whitened(vr_ctx* c, size_t N) {
    SceneDev& s = c->scene;
    s.wrec_pd = true;
    VR_TRY(s.wrec.alloc(std::max<size_t>(N, 1), "hipMalloc(whitened records)"));
    if (N == 0) return VR_OK;
    uint32_t* d_bad = c->counters.get();
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), c->stream), "hipMemsetAsync(whitened records)");
    HIP_TRY(gauss_whiten(s.gauss.get(), s.wrec.get(), (uint32_t)N, d_bad, c->stream), "whitened records");
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream), "whitened records D2H");
    HIP_TRY(hipStreamSynchronize(c->stream), "hipStreamSynchronize(whitened records)");
    s.wrec_pd = bad == 0;
    return VR_OK;
}

// The part both device-builder uploads share, from the point where the records and boxes lie on the device in
// scene order (either copied up, upload_device_bvh, or computed there, vr_upload_gaussians_device): the build,
// the hand-over of its buffers to the scene and the whitened records. Frees d_rec and d_boxes.
vr_status finish_device_bvh(vr_ctx* c, DevBuf<GaussianRecord>& d_rec, DevBuf<float>& d_boxes, size_t N, const float cmin[3],
                            const float cmax[3], bool use_half) {
    SceneDev& s = c->scene;
    LbvhResult R;
    hipError_t e = lbvh_build(d_rec.get(), d_boxes.get(), (uint32_t)N, cmin, cmax, use_half, s.hn_center, s.hn_scale, c->stream, R);
    d_rec.reset();
    d_boxes.reset();
    if (e == hipErrorNotSupported) return fail(VR_ERR_UNSUPPORTED, "device BVH deeper than the traversal stacks");
    if (e != hipSuccess) return hip_fail(e, "device BVH build");
    // every buffer of the build belongs to the scene first (a fresh scene frees them on error)
    s.gauss.adopt(R.gauss, N);
    s.order.adopt(R.order, N);
    s.nodes.adopt(R.nodes, R.num_nodes);
    s.hnodes.adopt(R.hnodes, R.num_nodes);
    s.hnodes4.adopt(R.hnodes4, R.num_nodes4);
    s.num_nodes4 = R.hnodes4 ? R.num_nodes4 : 0;
    s.num_nodes = R.num_nodes;
    s.bvh_depth = R.max_depth;
    c->num_prims = (int32_t)N;
    s.last_upload_device_bvh = true;
    return upload_whitened(c, N);
}

// Device BVH build (kernels/vr_lbvh.hip): records and boxes go up in scene order, the device sorts
// them by Morton code and emits the child-pair, half-precision and 4-wide trees. VR_ERR_UNSUPPORTED:
// the tree is deeper than the traversal stacks allow (the caller builds on the host instead).
vr_status upload_device_bvh(vr_ctx* c, const HostScene& hs, const std::vector<float>& boxes) {
    const size_t N = hs.pre.size();
    std::vector<GaussianRecord> rec(N);
    float cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<float> ext(N);
    for (size_t i = 0; i < N; ++i) {
        rec[i] = pack_record(hs.pre[i]);
        float e = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float ce = 0.5f * (boxes[6 * i + k] + boxes[6 * i + 3 + k]);
            cmin[k] = std::min(cmin[k], ce);
            cmax[k] = std::max(cmax[k], ce);
            e = std::max(e, boxes[6 * i + 3 + k] - boxes[6 * i + k]);
        }
        ext[i] = e;
    }
    // half-precision trees: the host rule with the primitive boxes (leaves hold up to kLeafMax of them)
    // standing in for the leaf boxes
    const bool use_half = half_tree_rule(c, ext);
    DevBuf<GaussianRecord> d_rec;
    DevBuf<float> d_boxes;
    VR_TRY(d_rec.alloc(N, "hipMalloc(records)"));
    VR_TRY(d_boxes.alloc(N * 6, "hipMalloc(boxes)"));
    HIP_TRY(hipMemcpyAsync(d_rec.get(), rec.data(), N * sizeof(GaussianRecord), hipMemcpyHostToDevice, c->stream), "hipMemcpy(records)");
    HIP_TRY(hipMemcpyAsync(d_boxes.get(), boxes.data(), N * 24, hipMemcpyHostToDevice, c->stream), "hipMemcpy(boxes)");
    return finish_device_bvh(c, d_rec, d_boxes, N, cmin, cmax, use_half);
}

// The secondary rays' 4-wide tree: the shared tree's nodes refit with the records' tight boxes on the
// device (vr_gauss_tree.hip, refit_kernel; whitened scenes only: the M forms keep the padded boxes).
vr_status upload_secondary_tree(vr_ctx* c) {
    SceneDev& s = c->scene;
    s.hnodes4s.reset();
    if (!c->opt_sec_tight || !s.wrec_pd || !s.wrec || !s.hnodes4 || !s.parent4 || !s.gauss || s.num_nodes4 == 0) return VR_OK;
    const size_t n = s.num_nodes4;
    double d2 = 0.0;  // the scene box's diagonal: no ray origin is farther than that from a record
    for (int k = 0; k < 3; ++k) d2 += ((double)s.bmax[k] - s.bmin[k]) * ((double)s.bmax[k] - s.bmin[k]);
    DevBuf<uint8_t> depth;
    DevBuf<float> nbox;
    DevBuf<uint32_t> maxd;
    // n nodes as refit (HNode4), then the same n nodes with their boxes laid out per axis for the secondary kernel's
    // node step (soa_nodes_kernel)
    hipError_t e = s.hnodes4s.try_alloc(2 * n);
    if (e == hipSuccess) e = depth.try_alloc(n);
    if (e == hipSuccess) e = nbox.try_alloc(n * 6);
    if (e == hipSuccess) e = maxd.try_alloc(1);
    if (e == hipSuccess)
        e = gauss_refit_secondary(s.hnodes4.get(), s.hnodes4s.get(), s.hnodes4s.get() + n, (uint32_t)n,
                                  s.gauss.get(), s.parent4.get(), depth.get(), nbox.get(), maxd.get(), s.hn_center, s.hn_scale,
                                  (float)std::sqrt(d2), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipErrorNotSupported) {  // a tree deeper than 255 levels: the shared boxes
        s.hnodes4s.reset();
        return VR_OK;
    }
    if (e != hipSuccess) return hip_fail(e, "secondary-ray tree");
    return VR_OK;
}

// Parent of every 4-wide node (built on the device from the children refs): a secondary ray starts its
// tree walk in the subtree holding its origin and climbs to the parents once that subtree is done
// (vr_gauss_secondary.hip, record_start_kernel / sec_node4v).
vr_status upload_parents(vr_ctx* c) {
    SceneDev& s = c->scene;
    s.parent4.reset();
    s.prim_node4.reset();
    s.hnodes4w.reset();
    if (!s.hnodes4 || s.num_nodes4 == 0) return VR_OK;
    // every 4-wide walk's node test reads the per-axis copy (wide_children): it exists whenever hnodes4 does
    VR_TRY(s.hnodes4w.alloc(s.num_nodes4, "hipMalloc(per-axis wide nodes)"));
    HIP_TRY(gauss_soa_nodes(s.hnodes4.get(), s.hnodes4w.get(), (uint32_t)s.num_nodes4, c->stream), "per-axis wide nodes");
    VR_TRY(s.parent4.alloc(s.num_nodes4, "hipMalloc(wide-node parents)"));
    if (c->num_prims > 0) VR_TRY(s.prim_node4.alloc((size_t)c->num_prims, "hipMalloc(record leaf nodes)"));
    HIP_TRY(gauss_parents(s.hnodes4.get(), (uint32_t)s.num_nodes4, s.parent4.get(), s.prim_node4.get(), c->stream),
            "wide-node parents");
    HIP_TRY(hipStreamSynchronize(c->stream), "wide-node parents");
    return upload_secondary_tree(c);
}

}  // namespace

extern "C" {

// (The scene heuristics below have C linkage as vr_upload_scene does: they have always been exported symbols.)
// Median central-chord optical depth of the scene's Gaussians and what it sets. First hit-window
// capacity of the free-flight sweep: a path scatters once the optical
// depth of the hits it crossed passes an Exp(1) target, so the hits a bounce needs scale like
// 1 / (optical depth per hit). Median over (up to 4096 sampled) Gaussians of the central-chord depth
// density * norm * sqrt(2 pi / d^T M d) along a fixed direction per Gaussian; window0 = the power of
// two >= 64 / median, in [4, 32] (measured optima: 1000_random, median 4.5 -> 16; make_random and
// 10k_random, median ~450 -> 4). Results do not depend on it (every window yields the same events).
double scene_median_chord_depth(const HostScene& s) {
    const size_t N = s.pre.size();
    if (N == 0) return 0.0;
    const size_t step = std::max<size_t>(1, N / 4096);
    static const float dirs[4][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.57735027f, 0.57735027f, 0.57735027f}};
    std::vector<double> tau;
    for (size_t i = 0, k = 0; i < N; i += step, ++k) {
        const GaussianPre& p = s.pre[i];
        const float* d = dirs[k & 3];
        const float* m = p.inv_cov;  // 00 01 02 11 12 22
        const double a = (double)m[0] * d[0] * d[0] + (double)m[3] * d[1] * d[1] + (double)m[5] * d[2] * d[2] +
                         2.0 * ((double)m[1] * d[0] * d[1] + (double)m[2] * d[0] * d[2] + (double)m[4] * d[1] * d[2]);
        if (a > 0.0 && std::isfinite(a)) tau.push_back((double)p.density * (double)p.norm * std::sqrt(2.0 * M_PI / a));
    }
    if (tau.empty()) return 0.0;
    std::nth_element(tau.begin(), tau.begin() + tau.size() / 2, tau.end());
    return tau[tau.size() / 2];
}
// Mean number of 3-sigma ellipsoids covering a point of the scene's bounding box.
double scene_overlap(const HostScene& s) {
    double vol = 0.0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const GaussianPre& p : s.pre) {
        const double a = p.cov[0], b = p.cov[1], cc = p.cov[2], d = p.cov[3], e = p.cov[4], f = p.cov[5];
        const double det = a * (d * f - e * e) - b * (b * f - e * cc) + cc * (b * e - d * cc);
        if (det > 0.0) vol += 4.0 / 3.0 * M_PI * 27.0 * std::sqrt(det);
        const double ext[3] = {3.0 * std::sqrt(std::max(a, 0.0)), 3.0 * std::sqrt(std::max(d, 0.0)), 3.0 * std::sqrt(std::max(f, 0.0))};
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], (double)p.mean[k] - ext[k]);
            hi[k] = std::max(hi[k], (double)p.mean[k] + ext[k]);
        }
    }
    const double box = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
    return box > 0.0 && std::isfinite(box) ? vol / box : 0.0;
}
// ... and a path starting inside a dense region first meets every Gaussian covering its start point
// (all with entry key 0): scenes whose ellipsoids overlap >= 8-fold on average start at 8
// (1M make_random, overlap 17: 190 vs 205 ms at 4; 100k, overlap 1.8, and 10k_random, 0.2: 4 best).
int32_t scene_window0(double med, double overlap) {
    if (!(med > 0.0)) return 8;
    int32_t w = overlap >= 8.0 ? 8 : 4;
    while (w < 32 && (double)w * med < 64.0) w *= 2;
    return w;
}
// Refill threshold of the shadow-ray kernel: a refill (queue claim + ray setup) costs about a node
// step; opaque scenes end most shadow rays after a few steps (optical depth 104 reached), so waves
// refill in larger batches there (while-while kernel, measured: 56 for make_random and 10k_random,
// 16-32 alike for 1000_random).
#ifndef VR_NEE_REFILL_OPAQUE
#define VR_NEE_REFILL_OPAQUE 56
#endif
#ifndef VR_NEE_REFILL_TRANSLUCENT
#define VR_NEE_REFILL_TRANSLUCENT 24
#endif
int32_t scene_nee_refill(double med) { return med >= 50.0 ? VR_NEE_REFILL_OPAQUE : VR_NEE_REFILL_TRANSLUCENT; }

}  // extern "C"

namespace {

// What every upload begins with: the device is idle, the previous scene's last report is collected, the scene
// and what hangs on it are reset, and the lights and the environment are the new scene's.
vr_status begin_upload(vr_ctx* c, int32_t type, const vr_light* lights, size_t n_lights, const float env[3]) {
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    VR_TRY(collect(c));  // the previous scene's last report, before the reset
    c->scene = SceneDev{};  // frees the previous scene
    c->has_scene = false;
    c->q_count_valid = false;
    c->march_big = false;
    c->filter_low = false;
    c->filter_skipped = 0;
    c->nee_inline = false;  // (nee_hint is kept: the inverse loop re-uploads every iteration and renders alike)
    c->type = type;
    c->lights.clear();
    for (size_t i = 0; i < n_lights; ++i) {
        const vr_light& l = lights[i];
        c->lights.push_back(LightRecord{l.position[0], l.position[1], l.position[2], l.intensity[0], l.intensity[1], l.intensity[2]});
    }
    std::memcpy(c->env, env, sizeof(c->env));
    for (int k = 0; k < 3; ++k) {
        c->scene.bmin[k] = INFINITY;
        c->scene.bmax[k] = -INFINITY;
    }
    return VR_OK;
}

// vr_upload_scene on one device. try_device: Gaussian scenes of kDeviceBvhMin primitives or more try the device
// builder first (VR_OPT_DEVICE_BVH).
vr_status upload_host_scene(vr_ctx* c, const HostScene& s, bool try_device) {
    if (s.lights.size() > (size_t)kMaxLights) return fail(VR_ERR_UNSUPPORTED, "more than 16 lights");
    VR_TRY(begin_upload(c, s.type, s.lights.data(), s.lights.size(), s.env));
    float *bmin = c->scene.bmin, *bmax = c->scene.bmax;
    if (s.type == VR_VOLUME_GAUSSIANS) {
        const size_t N = s.pre.size();
        if (N >= (1u << 27)) return fail(VR_ERR_UNSUPPORTED, "more than 2^27 Gaussians");
        const double med = scene_median_chord_depth(s);
        c->auto_window0 = scene_window0(med, scene_overlap(s));
        c->auto_nee_refill = scene_nee_refill(med);
        // long per-bounce collections and sweeps (many translucent Gaussians per bounce: C2's 1000_random, median
        // 4.5) favour the phase-scheduled kernel; short ones its per-iteration scheduling cost (C3/C4/C5, main)
        c->auto_ff_sm = N >= 256 && med > 0.0 && med < 16.0;
        std::vector<float> boxes(6 * N);
        for (size_t i = 0; i < N; ++i) {
            gaussian_bounds(s.pre[i], &boxes[6 * i], &boxes[6 * i + 3]);
            for (int k = 0; k < 3; ++k) {
                bmin[k] = std::min(bmin[k], boxes[6 * i + k]);
                bmax[k] = std::max(bmax[k], boxes[6 * i + 3 + k]);
            }
        }
        if (try_device && N >= kDeviceBvhMin) {
            vr_status ds = upload_device_bvh(c, s, boxes);
            if (ds == VR_OK) {
                if ((ds = upload_parents(c)) != VR_OK) return ds;
                c->has_scene = true;
                return VR_OK;
            }
            // UNSUPPORTED: too deep for the stacks -> host build (the scene holds nothing of the failed build yet)
            if (ds != VR_ERR_UNSUPPORTED) return ds;
        }
        BVHBuild b = build_bvh(boxes);
        if (b.max_depth > kMaxDepth + 1) return fail(VR_ERR_OVERFLOW, "BVH deeper than the traversal stack");
        SceneDev& d = c->scene;
        std::vector<GaussianRecord> rec(std::max<size_t>(N, 1));
        for (size_t j = 0; j < N; ++j) rec[j] = pack_record(s.pre[b.order[j]]);
        VR_TRY(d.gauss.alloc(rec.size(), "hipMalloc(records)"));
        HIP_TRY(hipMemcpy(d.gauss.get(), rec.data(), rec.size() * sizeof(GaussianRecord), hipMemcpyHostToDevice), "hipMemcpy(records)");
        VR_TRY(upload_whitened(c, N));
        {
            std::vector<uint32_t> order(std::max<size_t>(N, 1), 0u);
            for (size_t j = 0; j < N; ++j) order[j] = (uint32_t)b.order[j];
            VR_TRY(d.order.alloc(order.size(), "hipMalloc(order)"));
            HIP_TRY(hipMemcpy(d.order.get(), order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(order)");
        }
        VR_TRY(d.nodes.alloc(b.nodes.size(), "hipMalloc(nodes)"));
        HIP_TRY(hipMemcpy(d.nodes.get(), b.nodes.data(), b.nodes.size() * sizeof(BVHNode), hipMemcpyHostToDevice), "hipMemcpy(nodes)");
        c->num_prims = (int32_t)N;
        d.bvh_depth = b.max_depth;
        VR_TRY(upload_half_nodes(c, b.nodes));
        d.num_nodes = b.nodes.size();
    } else {
        const size_t N = s.spheres.size();
        if (N > 16) return fail(VR_ERR_UNSUPPORTED, "the device sphere path supports at most 16 spheres");
        std::vector<SphereRecord> rec(std::max<size_t>(N, 1));
        for (size_t i = 0; i < N; ++i) {
            const vr_sphere& sp = s.spheres[i];
            rec[i] = SphereRecord{sp.center[0], sp.center[1], sp.center[2], sp.radius, sp.sigma_a, sp.sigma_s, 0, 0};
            float lo[3], hi[3];
            sphere_bounds(sp, lo, hi);
            for (int k = 0; k < 3; ++k) {
                bmin[k] = std::min(bmin[k], lo[k]);
                bmax[k] = std::max(bmax[k], hi[k]);
            }
        }
        VR_TRY(c->scene.spheres.alloc(rec.size(), "hipMalloc(spheres)"));
        HIP_TRY(hipMemcpy(c->scene.spheres.get(), rec.data(), rec.size() * sizeof(SphereRecord), hipMemcpyHostToDevice), "hipMemcpy(spheres)");
        c->num_prims = (int32_t)N;
    }
    if (c->num_prims == 0)
        for (int k = 0; k < 3; ++k) bmin[k] = bmax[k] = 0.0f;
    VR_TRY(upload_parents(c));
    c->has_scene = true;
    return VR_OK;
}

// The caller's device arrays as a host scene (vr_scene_add_gaussians of the same floats), through the host path:
// scenes under kDeviceBvhMin Gaussians, and those whose radix tree is deeper than the stacks.
vr_status upload_device_arrays_on_host(vr_ctx* c, const float* d_mean, const float* d_cov6, const float* d_density,
                                       const float* d_albedo, size_t n, const vr_light* lights, size_t n_lights,
                                       const float env[3]) {
    HostScene hs;
    std::vector<float> mean(3 * n), cov(6 * n), density(n), albedo(n);
    if (n > 0) {
        HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
        HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
        HIP_TRY(hipMemcpy(mean.data(), d_mean, 12 * n, hipMemcpyDeviceToHost), "hipMemcpy(means D2H)");
        HIP_TRY(hipMemcpy(cov.data(), d_cov6, 24 * n, hipMemcpyDeviceToHost), "hipMemcpy(covariances D2H)");
        HIP_TRY(hipMemcpy(density.data(), d_density, 4 * n, hipMemcpyDeviceToHost), "hipMemcpy(densities D2H)");
        HIP_TRY(hipMemcpy(albedo.data(), d_albedo, 4 * n, hipMemcpyDeviceToHost), "hipMemcpy(albedos D2H)");
    }
    hs.gaussians.resize(n);
    hs.pre.resize(n);
    for (size_t i = 0; i < n; ++i) {
        vr_gaussian g{};
        std::memcpy(g.mean, &mean[3 * i], sizeof(g.mean));
        std::memcpy(g.cov, &cov[6 * i], sizeof(g.cov));
        g.density = density[i];
        g.albedo = albedo[i];
        hs.gaussians[i] = g;
        hs.pre[i] = precompute_gaussian(g);
    }
    hs.lights.assign(lights, lights + n_lights);
    if (env) std::memcpy(hs.env, env, sizeof(hs.env));
    return upload_host_scene(c, hs, false);
}

// The device front of vr_upload_gaussians_device (kernels/vr_scene_dev.hip) and the shared tail. VR_ERR_UNSUPPORTED
// with nothing of the build in the scene: the radix tree is deeper than the stacks (the caller takes the host path).
vr_status upload_gaussians_device(vr_ctx* c, const float* d_mean, const float* d_cov6, const float* d_density,
                                  const float* d_albedo, size_t N, const vr_light* lights, size_t n_lights, const float env[3]) {
    VR_TRY(begin_upload(c, VR_VOLUME_GAUSSIANS, lights, n_lights, env));
    SceneDev& s = c->scene;
    const uint32_t n = (uint32_t)N, nb = scene_prepare_blocks(n);
    DevBuf<GaussianRecord> d_rec;
    DevBuf<float> d_boxes;
    SceneStats st;
    bool use_half = false;
    {
        DevBuf<float> d_ext, d_sorted;
        DevBuf<SceneStats> d_part;
        DevBuf<double> d_chord;
        DevBuf<std::byte> d_tmp;
        const size_t step = std::max<size_t>(1, N / 4096), count = (N + step - 1) / step;  // scene_median_chord_depth's samples
        VR_TRY(d_rec.alloc(N, "hipMalloc(records)"));
        VR_TRY(d_boxes.alloc(N * 6, "hipMalloc(boxes)"));
        VR_TRY(d_ext.alloc(N, "hipMalloc(box extents)"));
        VR_TRY(d_part.alloc((size_t)nb + 1, "hipMalloc(scene statistics)"));
        VR_TRY(d_chord.alloc(count, "hipMalloc(chord depths)"));
        // gaussian.h:55's first factor, as precompute_gaussian evaluates it (double)
        const double K = std::pow(2.0f * std::numbers::pi, -1.5f);
        HIP_TRY(scene_prepare(d_mean, d_cov6, d_density, d_albedo, n, K, d_rec.get(), d_boxes.get(), d_ext.get(), d_part.get(), c->stream),
                "scene records and boxes");
        HIP_TRY(scene_chord_samples(d_rec.get(), n, (uint32_t)step, (uint32_t)count, d_chord.get(), c->stream), "chord depths");
        std::vector<double> tau(count);
        HIP_TRY(hipMemcpyAsync(&st, d_part.get() + nb, sizeof(st), hipMemcpyDeviceToHost, c->stream), "scene statistics D2H");
        HIP_TRY(hipMemcpyAsync(tau.data(), d_chord.get(), count * sizeof(double), hipMemcpyDeviceToHost, c->stream), "chord depths D2H");
        HIP_TRY(hipStreamSynchronize(c->stream), "hipStreamSynchronize(scene statistics)");
        // the scene heuristics, as vr_upload_scene sets them
        tau.erase(std::remove_if(tau.begin(), tau.end(), [](double t) { return std::isnan(t); }), tau.end());
        double med = 0.0;
        if (!tau.empty()) {
            std::nth_element(tau.begin(), tau.begin() + tau.size() / 2, tau.end());
            med = tau[tau.size() / 2];
        }
        const double box = (st.ohi[0] - st.olo[0]) * (st.ohi[1] - st.olo[1]) * (st.ohi[2] - st.olo[2]);
        const double overlap = box > 0.0 && std::isfinite(box) ? st.vol / box : 0.0;
        c->auto_window0 = scene_window0(med, overlap);
        c->auto_nee_refill = scene_nee_refill(med);
        c->auto_ff_sm = N >= 256 && med > 0.0 && med < 16.0;
        for (int k = 0; k < 3; ++k) {
            s.bmin[k] = st.bmin[k];
            s.bmax[k] = st.bmax[k];
        }
        // half_tree_rule: the element of rank N / 2 of `ext`, by a full sort of the keys
        double half;
        if ((use_half = half_tree_norm(c, half))) {
            size_t tmp_bytes = 0;
            float median = 0.0f;
            HIP_TRY(scene_sort_ext(d_ext.get(), nullptr, n, nullptr, tmp_bytes, c->stream), "box extent sort");
            VR_TRY(d_sorted.alloc(N, "hipMalloc(sorted box extents)"));
            VR_TRY(d_tmp.alloc(std::max<size_t>(tmp_bytes, 1), "hipMalloc(sort scratch)"));
            HIP_TRY(scene_sort_ext(d_ext.get(), d_sorted.get(), n, d_tmp.get(), tmp_bytes, c->stream), "box extent sort");
            HIP_TRY(hipMemcpyAsync(&median, d_sorted.get() + N / 2, sizeof(float), hipMemcpyDeviceToHost, c->stream), "box extent D2H");
            HIP_TRY(hipStreamSynchronize(c->stream), "hipStreamSynchronize(box extents)");
            use_half = median >= 0.03 * half;
        }
    }
    VR_TRY(finish_device_bvh(c, d_rec, d_boxes, N, st.cmin, st.cmax, use_half));
    VR_TRY(upload_parents(c));
    c->has_scene = true;
    return VR_OK;
}

}  // namespace

extern "C" {

vr_status vr_upload_scene(vr_ctx* c, const vr_scene* sc) {
    if (!c || !sc) return fail(VR_ERR_INVALID, "vr_upload_scene: NULL argument");
    if (c->group) return vr::group_upload(c->group, sc);
    return upload_host_scene(c, sc->s, c->opt_device_bvh != 0);
}

vr_status vr_upload_gaussians_device(vr_ctx* c, const float* d_mean, const float* d_cov6, const float* d_density,
                                     const float* d_albedo, size_t n, const vr_light* lights, size_t n_lights,
                                     const float env_color[3]) {
    if (!c) return fail(VR_ERR_INVALID, "vr_upload_gaussians_device: NULL ctx");
    if (n > 0 && (!d_mean || !d_cov6 || !d_density || !d_albedo)) return fail(VR_ERR_INVALID, "vr_upload_gaussians_device: NULL array");
    if (n_lights > 0 && !lights) return fail(VR_ERR_INVALID, "vr_upload_gaussians_device: NULL lights");
    if (c->group) return fail(VR_ERR_UNSUPPORTED, "vr_upload_gaussians_device: a multi-device context (the arrays live on one device)");
    if (n_lights > (size_t)kMaxLights) return fail(VR_ERR_UNSUPPORTED, "more than 16 lights");
    if (n >= (1u << 27)) return fail(VR_ERR_UNSUPPORTED, "more than 2^27 Gaussians");
    const HostScene defaults;
    const float* env = env_color ? env_color : defaults.env;
    if (n >= kDeviceBvhMin) {
        vr_status st = upload_gaussians_device(c, d_mean, d_cov6, d_density, d_albedo, n, lights, n_lights, env);
        // UNSUPPORTED: too deep for the stacks -> host build, as vr_upload_scene falls back
        if (st != VR_ERR_UNSUPPORTED) return st;
    }
    return upload_device_arrays_on_host(c, d_mean, d_cov6, d_density, d_albedo, n, lights, n_lights, env);
}

vr_status vr_tree_limits(int32_t* leaf_max, int32_t* max_depth, int32_t* wide_stack_max) {
    if (leaf_max) *leaf_max = kLeafMax;
    if (max_depth) *max_depth = kMaxDepth;
    if (wide_stack_max) *wide_stack_max = kWideStackMax;
    return VR_OK;
}

vr_status vr_debug_tree(vr_ctx* c, int32_t array, void* out, size_t cap, size_t* n, size_t* elem_bytes, vr_tree_info* info) {
    if (!c || !n || (cap > 0 && !out)) return fail(VR_ERR_INVALID, "vr_debug_tree: bad argument");
    if (c->group) return fail(VR_ERR_INVALID, "vr_debug_tree: a multi-device context holds one scene per device");
    if (!c->has_scene) return fail(VR_ERR_INVALID, "vr_debug_tree: no scene uploaded");
    if (c->type != VR_VOLUME_GAUSSIANS) return fail(VR_ERR_INVALID, "vr_debug_tree: a sphere scene has no tree");
    const SceneDev& s = c->scene;
    const size_t np = (size_t)c->num_prims, n4 = s.hnodes4 ? s.num_nodes4 : 0;
    const void* src = nullptr;
    size_t count = 0, elem = 0;
    switch (array) {
        case VR_TREE_ORDER: src = s.order.get(), count = np, elem = sizeof(uint32_t); break;
        case VR_TREE_RECORDS: src = s.gauss.get(), count = np, elem = sizeof(GaussianRecord); break;
        case VR_TREE_NODES: src = s.nodes.get(), count = s.num_nodes, elem = sizeof(BVHNode); break;
        case VR_TREE_HNODES: src = s.hnodes.get(), count = s.num_nodes, elem = sizeof(HNode); break;
        case VR_TREE_HNODES4: src = s.hnodes4.get(), count = n4, elem = sizeof(HNode4); break;
        case VR_TREE_HNODES4S: src = s.hnodes4s.get(), count = n4, elem = sizeof(HNode4); break;
        case VR_TREE_HNODES4W: src = s.hnodes4w.get(), count = n4, elem = sizeof(HNode4); break;
        case VR_TREE_HNODES4T:  // the second half of the tight tree's allocation (upload_secondary_tree)
            src = s.hnodes4s ? s.hnodes4s.get() + n4 : nullptr, count = n4, elem = sizeof(HNode4);
            break;
        case VR_TREE_PARENT4: src = s.parent4.get(), count = n4, elem = sizeof(int32_t); break;
        case VR_TREE_PRIM_NODE4: src = s.prim_node4.get(), count = np, elem = sizeof(int32_t); break;
        default: return fail(VR_ERR_INVALID, "vr_debug_tree: unknown array");
    }
    if (!src) count = 0;
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    *n = count;
    if (elem_bytes) *elem_bytes = elem;
    if (info) {
        *info = vr_tree_info{};
        info->num_prims = c->num_prims;
        info->num_nodes = (int64_t)s.num_nodes;
        info->num_nodes4 = (int64_t)n4;
        info->bvh_depth = s.bvh_depth;
        info->built_on_device = s.last_upload_device_bvh ? 1 : 0;
        info->wrec_pd = s.wrec_pd ? 1 : 0;
        vr_tree_limits(&info->leaf_max, &info->max_depth, &info->wide_stack_max);
        for (int k = 0; k < 3; ++k) {
            info->hn_center[k] = s.hn_center[k];
            info->bounds_min[k] = s.bmin[k];
            info->bounds_max[k] = s.bmax[k];
        }
        info->hn_scale = s.hn_scale;
    }
    const size_t m = std::min(count, cap);
    if (m > 0) HIP_TRY(hipMemcpy(out, src, m * elem, hipMemcpyDeviceToHost), "hipMemcpy(tree)");
    return VR_OK;
}

}  // extern "C"
