// Device context: init and destroy, multi-context forwarding, the option table, vr_synchronize and the
// device side of the inverse loop. Scene upload is in vr_upload.cpp, frames in vr_frame.cpp, the mixture
// queries in vr_query_host.cpp; the context itself in vr_ctx.h.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "vr_ctx.h"

using namespace vr;

namespace vr {
int ctx_ranks(vr_ctx* c) { return (c && c->group) ? group_size(c->group) : 1; }
vr_ctx* ctx_rank(vr_ctx* c, int r) { return (c && c->group) ? group_rank(c->group, r) : (r == 0 ? c : nullptr); }
}  // namespace vr

extern "C" {

vr_status vr_init(int device, vr_ctx** out) {
    if (!out) return fail(VR_ERR_INVALID, "vr_init: out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(VR_ERR_HIP, "vr_init: no HIP device available");
    if (device < 0 || device >= n) return fail(VR_ERR_INVALID, "vr_init: device index out of range");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    vr_ctx* c = new vr_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(c->stream.put(), hipStreamNonBlocking) != hipSuccess || c->counters.try_alloc(4) != hipSuccess ||
        c->h_report.alloc(kReportWords) != hipSuccess || c->h_sizing.alloc(4) != hipSuccess ||
        hipEventCreate(c->ev_start.put()) != hipSuccess || hipEventCreate(c->ev_stop.put()) != hipSuccess ||
        hipEventCreate(c->ev_report.put()) != hipSuccess || hipEventCreate(c->ev_stage[0].put()) != hipSuccess ||
        hipEventCreate(c->ev_stage[1].put()) != hipSuccess || hipEventCreate(c->ev_stage[2].put()) != hipSuccess ||
        hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        vr_destroy(c);
        return fail(VR_ERR_HIP, "vr_init: failed to create stream/workspace");
    }
    std::memset(c->h_report.get(), 0, kReportWords * sizeof(uint32_t));
    *out = c;
    return VR_OK;
}

vr_status vr_device_count(int32_t* n) {
    if (!n) return fail(VR_ERR_INVALID, "vr_device_count: NULL argument");
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
    *n = k;
    return VR_OK;
}

vr_status vr_init_multi(int32_t ndev, const int32_t* devices, vr_ctx** out) {
    if (!out) return fail(VR_ERR_INVALID, "vr_init_multi: out is NULL");
    vr_group* g = nullptr;
    VR_TRY(vr::group_create(ndev, devices, &g));
    vr_ctx* c = nullptr;
    if (vr_status st = vr_init(devices ? devices[0] : 0, &c); st != VR_OK) {
        std::string m = vr_last_error();
        vr::group_destroy(g);
        return fail(st, m);
    }
    c->group = g;
    *out = c;
    return VR_OK;
}

int32_t vr_ctx_num_devices(const vr_ctx* c) { return !c ? 0 : c->group ? vr::group_size(c->group) : 1; }

int32_t vr_ctx_uses_rccl(const vr_ctx* c) { return c && c->group && vr::group_uses_rccl(c->group) ? 1 : 0; }

vr_status vr_get_rank_stats(vr_ctx* c, int32_t rank, vr_render_stats* out) {
    if (!c || !out) return fail(VR_ERR_INVALID, "vr_get_rank_stats: NULL argument");
    vr_ctx* r = vr::ctx_rank(c, rank);
    if (!r) return fail(VR_ERR_INVALID, "vr_get_rank_stats: rank out of range");
    return vr_get_stats(r, out);
}

void vr_destroy(vr_ctx* c) {
    if (!c) return;
    if (c->group) {
        vr::group_destroy(c->group);
        c->group = nullptr;
    }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;  // its members free the buffers, then the events, then the stream
}

// out[g] (host) = d_out[g] = sum over the union of the pixels recorded for g in slots 0 and 1 of lp - lb (device losses).
static vr_status loss_diff(vr_ctx* c, const float* lb, const float* lp, uint32_t npix, size_t n, double* d_out, double* out) {
    VR_TRY(c->sfd_part.grow(std::max<size_t>(sfd_partial_count(npix, (uint32_t)n), 1), "hipMalloc(sfd partial sums)"));
    HIP_TRY(hipMemsetAsync(d_out, 0, n * 8, c->stream), "hipMemsetAsync");
    if (n > 0)
        HIP_TRY(launch_sfd_loss_diff(c->rec_bits[0].get(), c->rec_bits[1].get(), lb, lp, npix, (uint32_t)n, c->sfd_part.get(), d_out,
                                     c->stream),
                "sfd launch");
    HIP_TRY(hipMemcpyAsync(out, d_out, n * 8, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    HIP_TRY(hipStreamSynchronize(c->stream), "sfd");
    return VR_OK;
}

vr_status vr_sfd_loss_diff(vr_ctx* c, const float* loss_base, const float* loss_plus, uint32_t W, uint32_t H, double* out,
                           size_t n) {
    c = first_device(c);
    if (!c || !loss_base || !loss_plus || !out) return fail(VR_ERR_INVALID, "vr_sfd_loss_diff: NULL argument");
    const uint32_t npix = W * H;
    if (c->rec_npix[0] != npix || c->rec_npix[1] != npix || c->rec_n[0] != c->rec_n[1] || n != c->rec_n[0])
        return fail(VR_ERR_INVALID, "vr_sfd_loss_diff: slots 0 and 1 must hold recordings of this frame size and n Gaussians");
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    VR_TRY(c->sfd_tmp.grow((size_t)npix * 8 + n * 8 + 16, "hipMalloc(sfd)"));
    float* lb = (float*)c->sfd_tmp.get();
    float* lp = lb + npix;
    double* d_out = (double*)(c->sfd_tmp.get() + (((size_t)npix * 8 + 15) & ~(size_t)15));
    HIP_TRY(hipMemcpyAsync(lb, loss_base, (size_t)npix * 4, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    HIP_TRY(hipMemcpyAsync(lp, loss_plus, (size_t)npix * 4, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    return loss_diff(c, lb, lp, npix, n, d_out, out);
}

}  // extern "C"

namespace vr {

// ---- device side of the inverse loop (host/vr_inverse.cpp) ----
vr_status sfd_set_reference(vr_ctx* c, const float* I_ref, uint32_t W, uint32_t H) {
    c = first_device(c);
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    const size_t npix = (size_t)W * H;
    VR_TRY(c->sfd_ref.grow(npix * 3, "hipMalloc(I_ref)"));
    for (auto& b : c->sfd_loss)
        VR_TRY(b.grow(npix, "hipMalloc(pixel losses)"));
    HIP_TRY(hipMemcpy(c->sfd_ref.get(), I_ref, npix * 12, hipMemcpyHostToDevice), "hipMemcpy(I_ref)");
    return VR_OK;
}

// One forward render of the loop (slot 0/1: recorded, -1: plain) and its per-pixel L1 losses against
// the reference image into device loss buffer `which`; loss_host (W*H floats) receives a copy, and
// rgb (3*W*H floats, may be NULL) the frame.
vr_status sfd_render(vr_ctx* c, const vr_camera* cam, const vr_render_params* p, uint32_t W, uint32_t H, int32_t slot,
                     int which, float* loss_host, float* rgb) {
    c = first_device(c);
    VR_TRY(render_frame_device(c, cam, p, W, H, slot));
    const uint32_t npix = W * H;
    HIP_TRY(launch_pixel_losses(c->frame.get(), c->sfd_ref.get(), npix, c->sfd_loss[which].get(), c->stream), "pixel losses");
    HIP_TRY(hipMemcpyAsync(loss_host, c->sfd_loss[which].get(), (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream),
            "hipMemcpyAsync(losses)");
    if (rgb)
        HIP_TRY(hipMemcpyAsync(rgb, c->frame.get(), (size_t)npix * 12, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(frame)");
    HIP_TRY(hipStreamSynchronize(c->stream), "sfd render");
    return VR_OK;
}

// out[g] = sum over the union of the pixels recorded for g in slots 0 and 1 of loss[1] - loss[0].
vr_status sfd_loss_diff_device(vr_ctx* c, uint32_t npix, double* out, size_t n) {
    c = first_device(c);
    VR_TRY(c->sfd_out.grow(std::max<size_t>(n, 1), "hipMalloc(sfd)"));
    return loss_diff(c, c->sfd_loss[0].get(), c->sfd_loss[1].get(), npix, n, c->sfd_out.get(), out);
}

}  // namespace vr

namespace {

// vr_set_option / vr_get_option: every option's range and the context member that holds it.
struct Option {
    int32_t id;
    const char* name;
    int64_t lo, hi;
    const char* range;  // as the error message states it
    int64_t vr_ctx::*value;  // nullptr: VR_OPT_RECORD_CAPACITY, held as the record / overflow-pool capacity hints
};
#define VR_OPTION(id, lo, hi, range, member) {id, #id, lo, hi, range, member}
const Option kOptions[] = {
    VR_OPTION(VR_OPT_HALF_NODES, 0, 1, "0 or 1", &vr_ctx::opt_half_nodes),
    VR_OPTION(VR_OPT_SECONDARY_BUDGET, 0, 1, "0 or 1", &vr_ctx::opt_secondary_budget),
    VR_OPTION(VR_OPT_FF_WINDOW0, 0, kFFHitCap, "in [0, 128]", &vr_ctx::opt_ff_window0),
    VR_OPTION(VR_OPT_FF_NEE_QUEUE, 0, (int64_t)kFFNeeMaxPerPath, "in [0, 16]", &vr_ctx::opt_ff_nee_queue),
    VR_OPTION(VR_OPT_DEVICE_BVH, 0, 1, "0 or 1", &vr_ctx::opt_device_bvh),
    VR_OPTION(VR_OPT_MARCH_BINNED, 0, 1, "0 or 1", &vr_ctx::opt_march_binned),
    VR_OPTION(VR_OPT_FF_SOLVER, 0, 4, "in [0, 4]", &vr_ctx::opt_ff_solver),
    VR_OPTION(VR_OPT_START_SUBTREE, 0, 1, "0 or 1", &vr_ctx::opt_start_subtree),
    VR_OPTION(VR_OPT_FF_KERNEL, 0, 2, "in [0, 2]", &vr_ctx::opt_ff_kernel),
    VR_OPTION(VR_OPT_SEC_TIGHT, 0, 1, "0 or 1", &vr_ctx::opt_sec_tight),
    VR_OPTION(VR_OPT_MARCH_WIDE_MIN, 0, 0xffffffffll, "in [0, 2^32)", &vr_ctx::opt_march_wide_min),
    VR_OPTION(VR_OPT_SEC_FILTER, 0, 1, "0 or 1", &vr_ctx::opt_sec_filter),
    VR_OPTION(VR_OPT_RECORD_CAPACITY, 0, 0x3fffffff, "0 or in [4096, 2^30)", nullptr),
};
#undef VR_OPTION
const Option* find_option(int32_t id) {
    for (const Option& o : kOptions)
        if (o.id == id) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

vr_status vr_set_option(vr_ctx* c, int32_t option, int64_t value) {
    if (!c) return fail(VR_ERR_INVALID, "vr_set_option: NULL ctx");
    if (c->group) return vr::group_set_option(c->group, option, value);
    const Option* o = find_option(option);
    if (!o) return fail(VR_ERR_INVALID, "vr_set_option: unknown option " + std::to_string(option));
    if (value < o->lo || value > o->hi || (!o->value && value != 0 && value < 4096))
        return fail(VR_ERR_INVALID, std::string(o->name) + " must be " + o->range);
    if (o->value) c->*o->value = value;
    else c->rec_hint = c->ovf_hint = (uint64_t)value;
    if (option == VR_OPT_FF_NEE_QUEUE) c->nee_inline = false;
    if (option == VR_OPT_SEC_FILTER) {  // (setting it also forgets what earlier frames said about the filter's share)
        c->filter_low = false;
        c->filter_skipped = 0;
    }
    return VR_OK;
}

vr_status vr_get_option(vr_ctx* c, int32_t option, int64_t* value) {
    c = first_device(c);
    if (!c || !value) return fail(VR_ERR_INVALID, "vr_get_option: NULL argument");
    const Option* o = find_option(option);
    if (!o) return fail(VR_ERR_INVALID, "vr_get_option: unknown option " + std::to_string(option));
    *value = o->value ? c->*o->value : (int64_t)c->rec_hint;
    return VR_OK;
}

vr_status vr_synchronize(vr_ctx* c) {
    if (!c) return fail(VR_ERR_INVALID, "vr_synchronize: NULL ctx");
    if (c->group) return vr::group_synchronize(c->group);
    HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    vr_status st = collect(c);
    if (st != VR_OK || !c->sync_pending) return st;
    c->sync_pending = false;  // (a frame that vr_get_stats or an upload collected first is still reported here)
    if (frame_exceeded(c))
        return fail(VR_ERR_RETRY, "the last frame outgrew the scatter-record buffers / shadow-ray queue sized from earlier frames; "
                                  "they have been grown: render it again");
    if (c->h_report[kRepErrors] != 0)
        return fail(VR_ERR_OVERFLOW, std::to_string(c->h_report[kRepErrors]) + " pixels / paths of the last frame exceeded a "
                                     "per-ray capacity (NaN)");
    return VR_OK;
}


}  // extern "C"
