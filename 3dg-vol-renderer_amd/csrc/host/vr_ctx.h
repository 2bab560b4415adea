// The device context (vr_ctx) and what its host files share: vr_device.cpp (init / destroy, options,
// vr_synchronize, the SFD helpers), vr_upload.cpp (vr_upload_scene), vr_frame.cpp (the frame pipelines,
// their report and the render entry points), vr_rays.cpp (vr_render_rays) and vr_query_host.cpp (vr_query_*).
#pragma once
#include <map>

#include "vr_devmem.h"
#include "vr_kernels.h"

#pragma GCC visibility push(hidden)  // internal to libvr_hip.so

// Pinned report of a frame's counts, copied on the render stream after its last kernel (launch) and read
// once ev_report has passed (collect).
enum Report {
    kRepFallback = 0,  // fallback-queue length (pixels re-marched)
    kRepErrors,        // error pixels / paths (over every per-ray capacity: NaN)
    kRepRecords,       // rec_alloc: scatter records,
    kRepOverflowWords, //   overflow-pool words,
    kRepExceeded,      //   record capacity exceeded (the frame is invalid and must be rendered again)
    kRepDeep,          // deep-pass queue length
    kRepFFFallback,    // counter 2: free-flight paths re-run in ff_fallback_kernel
    kRepNeeNeed,       // counter 3: free-flight, the most shadow rays one launch tried to queue
    kRepSlow,          // exact slow-path queue length
    kRepFix,           // band fix-up queue length
    kRepFiltered,      // rec_alloc[3]: environment rays cut on their record's active list before the walk
    kReportWords
};

// The active list indexes the hit buffer, so it never holds more than kFFHitCap entries: the only
// capacity a path can exceed is kFFHitCap Gaussians overlapping one point; such a path re-runs in
// ff_fallback_kernel with kFFBigCap-entry rows (only beyond that: error path, NaN).
constexpr int32_t kFFHitCap = 128, kFFActCap = kFFHitCap;

// The uploaded scene on the device. A fresh value frees all of it (free_scene).
struct SceneDev {
    vr::DevBuf<vr::GaussianRecord> gauss;
    vr::DevBuf<vr::WRecord> wrec;  // whitened copy (secondary rays)
    bool wrec_pd = true;           // every record's M is positive definite (else the secondary rays use the M forms)
    vr::DevBuf<vr::BVHNode> nodes;
    vr::DevBuf<vr::HNode> hnodes;
    vr::DevBuf<vr::HNode4> hnodes4;
    vr::DevBuf<vr::HNode4> hnodes4s;   // the secondary rays' copy with tight boxes (VR_OPT_SEC_TIGHT)
    vr::DevBuf<vr::HNode4> hnodes4w;   // hnodes4 laid out per axis (the 4-wide walks' node tests, wide_children)
    vr::DevBuf<int32_t> parent4;       // parent of every HNode4 (the secondary rays' climb out of their start subtree)
    vr::DevBuf<int32_t> prim_node4;    // the HNode4 whose child is each record's leaf (record starts)
    vr::DevBuf<uint32_t> order;        // record (leaf order) -> scene index
    vr::DevBuf<vr::SphereRecord> spheres;
    size_t num_nodes = 0, num_nodes4 = 0;
    int bvh_depth = 0;
    float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
    float hn_center[3] = {0, 0, 0}, hn_scale = 1.0f;
    bool last_upload_device_bvh = false;  // the tree came from the device builder
};

struct vr_ctx {
    int device = 0;
    int cus = 1;  // compute units of the device (vr_init)
    // The stream and the events come before every buffer: they are destroyed after them.
    vr::Stream stream;  // used by the synchronous vr_render
    vr::Event ev_start, ev_stop;
    vr::Event ev_report;    // after the frame report's copies (collect() waits for it)
    vr::Event ev_stage[3];  // stage boundaries of gauss_pipeline
    // free-flight frames: per launch, events before the path kernel, after it, after the shadow-ray
    // kernel and after the accumulation (stage_ms of vr_get_stats sums them over the frame's launches)
    std::vector<vr::Event> ff_ev;
    vr::PinnedBuf<uint32_t> h_report;  // kReportWords words (Report)
    vr::PinnedBuf<uint32_t> h_sizing;  // copy of rec_alloc for the sizing march of a context's first frame
    // scene
    bool has_scene = false;
    int32_t type = VR_VOLUME_GAUSSIANS;
    int32_t num_prims = 0;
    SceneDev scene;
    std::vector<vr::LightRecord> lights;
    float env[3] = {0, 0, 0};
    // step tables keyed by step size
    struct Table {
        vr::DevBuf<float> d;
        int n = 0;
        float tmax = 0;
    };
    std::map<uint32_t, Table> tables;
    // workspaces
    vr::DevBuf<uint32_t> queue;  // [0] length, then queue_cap entries
    uint32_t queue_cap = 0;
    vr::DevBuf<uint32_t> counters;  // [0] error pixels / paths of the frame, [2..3] see Report
    bool report_gauss = false;  // the last frame ran the RayMarchingGaussians pipeline (kRepRecords .. kRepExceeded)
    uint64_t report_pixels = 0; // pixels of that frame (its march)
    bool march_big = false;     // this scene's frames overflow the primary march's 16 slots often: kActBig (reset at upload)
    vr::DevBuf<float> frame;    // exactly the largest frame so far
    bool staged = false;        // last launch recorded ev_stage
    uint32_t ff_launches = 0;
    bool stats_pending = false;  // h_report of the last frame has not been collected yet
    bool sync_pending = false;   // the last frame's outcome (retry / overflow) is collected but not yet reported by
                                 // vr_synchronize: sticky, whoever collected it (vr_get_stats, an upload, ...)
    int64_t last_pixels = 0;
    uint32_t last_first_tile = 0, last_tile_stride = 1, last_tiles_x = 1, last_w = 0, last_h = 0;  // tile map of the last frame
    uint32_t last_secondary_per_record = 0;
    // The environment rays' list filter pays from about a third of the rays filtered (kFilterMinShare, vr_frame.cpp). A
    // frame that ran it and filtered less switches it off for this context's later frames (a hint, as rec_hint: frames
    // are identical either way); every kFilterProbe-th such frame runs it again, an upload or VR_OPT_SEC_FILTER resets it.
    bool filter_ran = false;      // the last ray-march frame ran the filter (with last_env_samples per record)
    bool filter_low = false;      // ... and the last one that did filtered less than the break-even share
    uint32_t filter_skipped = 0;  // frames rendered without it since
    uint32_t last_env_samples = 0;
    // wavefront pipeline buffers (grown on demand, never shrunk)
    vr::DevBuf<uint32_t> px_first, rec_next, rec_alloc, slowq, fixq;
    vr::DevBuf<float> px_T, tr, rec_cut;
    vr::DevBuf<float4> rec_pos, rec_rad;
    vr::DevBuf<uint4> rec_meta;
    vr::DevBuf<int32_t> rec_act, stack_ovf;
    vr::DevBuf<vr::RecStart> rec_start;
    vr::DevBuf<unsigned long long> rec_bloom, pcg_jump, ray_next;
    vr::DevBuf<uint16_t> env_order;
    vr::DevBuf<uint64_t> env_base;
    vr::DevBuf<uint32_t> env_count;
    vr::DevBuf<std::byte> deep;  // march_deep_kernel: pixel queue + global active lists (vr_gauss_march.hip)
    vr::DevBuf<uint32_t> bin_cnt, bin_off, bin_ent;  // tile bins of the binned march (VR_OPT_MARCH_BINNED)
    vr::DevBuf<std::byte> ff_scratch;                // free-flight integrators (vr_freeflight.hip, vr_ff_bounce.h)
    vr::DevBuf<float4> ff_tail, ff_nee;
    vr::DevBuf<float> ff_sum;
    vr::DevBuf<std::byte> ff_fb;      // ff_fallback_kernel: path queue + kFFBigCap rows
    vr::DevBuf<uint32_t> rec_bits[2];  // RECORD_PIXEL_GAUSSIANS bitsets (vr_render_record slots)
    uint32_t rec_npix[2] = {0, 0}, rec_n[2] = {0, 0};
    vr::DevBuf<std::byte> sfd_tmp;     // vr_sfd_loss_diff: losses + output
    vr::DevBuf<float> sfd_ref, sfd_loss[2];  // device inverse loop (vr_sfd_optimize): I_ref, base / perturbed losses
    vr::DevBuf<double> sfd_out, sfd_part;  // the union statistic and its per-chunk partial sums
    // mixture queries (vr_query_*, kernels/vr_query.hip): their own workspaces, grown on demand; nothing of a
    // frame (report, statistics, hints) is touched by a query
    // host forms (synchronous, one at a time): the batch on the device by role, each sized in 4-byte words: the inputs
    // (rays / points), the weights / targets / samples / event offsets, the first result and the second
    vr::DevBuf<float> q_in, q_w, q_out, q_out2;
    vr::DevBuf<float> q_feat, q_w2;             // the feature queries' further inputs: the rows, the mass weights
    vr::DevBuf<uint32_t> q_cnt;                 // events: counts,
    vr::DevBuf<unsigned long long> q_keys, q_keys2;  // sort keys (in / out),
    vr::DevBuf<std::byte> q_tmp;                // scan + sort scratch
    vr::DevBuf<std::byte> q_ctl;      // words [0..3], [6] ray counters of the five persistent walks, [4..5] the 64-bit event total,
                                      // [8], [9] the counters of the profile query's two walks, [10], [11] those of the
                                      // radiance query's (its profile pass and its own), [12] .. [14] those of the
                                      // radiance gradient query's three passes
    vr::DevBuf<double> q_grad;        // gradient query: 10 doubles of staging per Gaussian (tree order), zeroed per call
    vr::DevBuf<double> q_sgrad;       // sigma gradient query: 11 doubles of staging per Gaussian, its own (the two
                                      // gradient queries may be queued on different streams)
    vr::DevBuf<double> q_prof_grad;   // profile gradient query (kernels/vr_query_profile.hip): 10 doubles of staging per
                                      // Gaussian, its own for q_sgrad's reason
    vr::DevBuf<double> q_feat_grad;   // feature gradient query (kernels/vr_query_features.hip): 10 doubles of staging per
    vr::DevBuf<double> q_feat_fgrad;  // Gaussian and C per Gaussian for the rows' gradient (tree order), zeroed per call,
                                      // grown on demand; its own for q_sgrad's reason
    vr::DevBuf<float> q_rad_tr;       // radiance query (kernels/vr_query_radiance.hip): the profile's Tr, n * K floats, when the
                                      // caller does not ask for it; the query's only intermediate
    vr::DevBuf<float> q_w3, q_out3;   // its host form's further arrays: the quadrature weights; the opacity and the counts
    // radiance gradient query (kernels/vr_query_radiance_grad.hip), its own for q_sgrad's reason, grown on demand:
    vr::DevBuf<float> q_radg_tr;      //   the profile's Tr when the caller has none, n * K floats
    vr::DevBuf<float> q_radg_tau;     //   grad_tau when grad is asked for without it, n * K floats
    vr::DevBuf<double> q_radg_s;      //   s = sum_g m phi per sample, n * K doubles, each row zeroed by its own ray
    vr::DevBuf<double> q_radg_stage;  //   10 doubles of staging per Gaussian (both parts of grad), zeroed per call
    vr::DevBuf<double> q_radg_fstage; //   C doubles of feature staging per Gaussian, zeroed per call
    vr::DevBuf<float> q_w4, q_w5;     //   its host form's further inputs: the opacity weights, the forward's Tr
    // free-flight query (kernels/vr_query_flight.hip): its own scratch rows (the layouts of ff_scratch and of
    // ff_fb's rows), so a frame queued on another stream never shares them; counters + queue of rays over the rows
    vr::DevBuf<std::byte> q_ff_rows, q_ff_big;
    vr::DevBuf<uint32_t> q_ff_ctl;
    // ray grids (vr_render_rays, vr_rays.cpp)
    vr::DevBuf<vr_ray> ray_in;        // host form: the grid on the device,
    vr::DevBuf<float> ray_tr;         //   and its transmittance output
    vr::DevBuf<uint32_t> ray_ext;     // device form: the extent reduction's result (ray_extent_kernel)
    bool q_count_valid = false;       // the last vr_query_events_count_device of this scene: its n and total
    uint64_t q_count_n = 0, q_count_total = 0;
    int pcg_jump_n = -1;
    uint64_t rec_hint = 0, ovf_hint = 0;  // record / overflow-pool capacities (0: not known yet)
    uint64_t slow_hint = 0;               // exact slow-path queue: the most rays an earlier frame queued (+ 1/8)
    uint64_t fix_hint = 0;                // band fix-up queue (secondary_fix_kernel): the same
    uint64_t nee_hint = 0;                // deferred-NEE queue capacity from earlier free-flight frames (0: not known)
    uint32_t last_nee_cap = 0, last_nee_bound = 0;  // the last free-flight frame's queue capacity and its bound
    // A launch found the shadow-ray queue full at its VR_OPT_FF_NEE_QUEUE bound: the frame is reported
    // (VR_ERR_RETRY) and this context's later frames trace every shadow ray inline — the queue's own walk and
    // sums, so the same frame bit for bit as a queue with room — until the next upload or option change.
    bool nee_inline = false;
    bool report_ff = false;               // the last frame ran the free-flight pipeline (kRepNeeNeed)
    // vr_set_option values (explicit per-context tuning; no environment variables are read)
    int64_t opt_half_nodes = 1;        // VR_OPT_HALF_NODES
    int64_t opt_secondary_budget = 1;  // VR_OPT_SECONDARY_BUDGET
    int64_t opt_ff_window0 = 0;        // VR_OPT_FF_WINDOW0 (0: auto_window0)
    int32_t auto_window0 = 8;          // first hit-window capacity derived from the uploaded scene
    int32_t auto_nee_refill = 40;      // shadow-ray kernel refill threshold derived from the uploaded scene
    int64_t opt_ff_kernel = 0;         // VR_OPT_FF_KERNEL (0: auto_ff_sm)
    bool auto_ff_sm = false;           // the uploaded scene's free-flight paths take the phase-scheduled kernel
    int64_t opt_ff_nee_queue = 6;      // VR_OPT_FF_NEE_QUEUE
    int64_t opt_device_bvh = 0;        // VR_OPT_DEVICE_BVH
    int64_t opt_march_binned = 0;      // VR_OPT_MARCH_BINNED
    int64_t opt_ff_solver = 0;         // VR_OPT_FF_SOLVER
    int64_t opt_start_subtree = 1;     // VR_OPT_START_SUBTREE
    int64_t opt_sec_tight = 1;         // VR_OPT_SEC_TIGHT (next upload)
    int64_t opt_march_wide_min = 2048;  // VR_OPT_MARCH_WIDE_MIN
    int64_t opt_sec_filter = 1;        // VR_OPT_SEC_FILTER
    vr_group* group = nullptr;         // vr_init_multi: the devices this context drives (host/vr_multi.cpp)
};

namespace vr {

// Single-device entry points called on a multi-GPU context act on its first device.
inline vr_ctx* first_device(vr_ctx* c) { return (c && c->group) ? group_rank(c->group, 0) : c; }

// vr_frame.cpp
vr_status collect(vr_ctx* c);           // waits for the last frame's report and grows the capacity hints from it
bool frame_exceeded(const vr_ctx* c);   // that frame outgrew its buffers: render it again
// A full frame into the context's frame buffer; slot 0/1 records RECORD_PIXEL_GAUSSIANS bitsets, -1 none.
vr_status render_frame_device(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, int32_t slot);
// Kernel arguments of a frame apart from its rays' source (a camera: vr_frame.cpp, a ray grid: vr_rays.cpp)
vr_status fill_scene_args(vr_ctx* c, const vr_render_params* p, uint32_t W, uint32_t H, vr::RenderArgs& A);
bool needs_table(const vr_render_params* p);      // the integrator marches the step table
float table_tmax(const vr_ctx* c, float extent);  // the table's reach for primary rays that travel `extent` at most
// (max_entries > 0: VR_ERR_OVERFLOW, before anything is allocated, for a table of more entries)
vr_status fill_table(vr_ctx* c, const vr_render_params* p, float tmax, uint32_t max_entries, vr::RenderArgs& A);
// One frame's kernels and report on stream s (asynchronous), and the synchronous form on the context's stream,
// which renders a frame that outgrew its record buffers again
// (grid: a ray grid's rays and transmittance output; nullptr: a camera frame)
vr_status launch(vr_ctx* c, vr::RenderArgs& A, const vr_render_params* p, hipStream_t s, bool stats = false,
                 const vr::GridSrc* grid = nullptr);
vr_status render_sync(vr_ctx* c, vr::RenderArgs& A, const vr_render_params* p, const vr::GridSrc* grid = nullptr);

}  // namespace vr
#pragma GCC visibility pop
