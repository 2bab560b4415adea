// Stage 3 of the RayMarchingGaussians pipeline (vr_gauss_common.h): the records' optical-depth cut-offs (before
// stage 2), their incident radiance from the secondary rays' transmittances and the per-pixel sum, with the
// launchers gauss_record_cut and gauss_accumulate.
#include "vr_gauss_common.h"

namespace vr {
namespace dev {

// ---------------------------------------------------------------------------------------------
// Stage 3: per-pixel accumulation in step order (test_integrators.h:237, 272-277, 292).
// ---------------------------------------------------------------------------------------------
// Per-pixel error budget of the secondary optical-depth cut-off. accumulate_kernel weighs a light
// ray's Tr by C = Ts dt I_l / (4 pi d_l^2) and an environment ray's by Ts dt env / NE (per
// channel), so a ray stopped at optical depth >= cut (its true Tr <= e^-cut, output 0) moves the
// pixel by at most C e^-cut. Every ray of the pixel gets an equal share budget / N_p of the
// budget (N_p: the pixel's secondary rays): a record's rays stop at
//   cut_r = ln(Cmax_r * N_p / budget),   Cmax_r = the largest C of the record's rays,
// so the pixel moves by at most sum C e^-cut <= N_p * budget / N_p = budget in every channel.
// (Equal shares minimise the work: dim records deep in a pixel get small cut-offs.)
__device__ __forceinline__ float record_weight(const RenderArgs& A, const float4& pos) {
    float w = fmaxf(fmaxf(fabsf(A.env[0]), fabsf(A.env[1])), fabsf(A.env[2])) / (float)max(A.env_samples, 1);
    for (int l = 0; l < A.num_lights; ++l) {
        const LightRecord& lr = A.lights[l];
        const float dx = lr.px - pos.x, dy = lr.py - pos.y, dz = lr.pz - pos.z;
        const float s = kInv4Pi / (dx * dx + dy * dy + dz * dz);
        w = fmaxf(w, fmaxf(fmaxf(fabsf(lr.ix), fabsf(lr.iy)), fabsf(lr.iz)) * s);
    }
    return pos.w * A.step_size * w;
}

__global__ __launch_bounds__(256) void record_cut_kernel(RenderArgs A, float budget) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.num_tiles * 256u) return;
    uint32_t n = 0;
    for (uint32_t r = A.px_first[p]; r != kNoRecord; r = A.rec_next[r]) ++n;
    const float rays = (float)n * (float)(A.num_lights + A.env_samples);
    // 1.001: headroom for the f32 rounding of the weights and of the optical depths themselves
    for (uint32_t r = A.px_first[p]; r != kNoRecord; r = A.rec_next[r])
        A.rec_cut[r] = fminf(kTauCut, fmaxf(0.0f, logf(1.001f * record_weight(A, A.rec_pos[r]) * rays / budget)));
}

// Per-record incident radiance Li + Le (test_integrators.h:212-275), one wave per record chunk: the
// chunk's Tr values are one contiguous run in hand-out order; they are read once, coalesced, into
// LDS as [record][sample] (env_order tells where each environment ray went), then each lane sums its
// record's lights and environment samples in the reference's order. Without env_order a chunk's
// rays are sample-major ([sample][record-in-chunk]) and are read in place (coalesced).
constexpr int kRadBlock = 64;
template <bool ORDERED>
__global__ __launch_bounds__(kRadBlock) void record_radiance_kernel(RenderArgs A) {
    extern __shared__ float s_tr[];  // ORDERED: [record-in-chunk][sample]
    const uint32_t nrec = dev_nrec(A), cr = A.chunk_rec, nl = (uint32_t)A.num_lights, ne = (uint32_t)A.env_samples;
    const uint32_t S = nl + ne, per = rays_per_chunk(A), nch = (nrec + cr - 1u) >> A.chunk_shift;
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        const float* tr = A.tr + (size_t)chunk * per;
        if constexpr (ORDERED) {
          // the chunk gather in 16-B Tr / 8-B order loads (C4: 0.96 ms; 4-B loads 1.59, unrolled 4-B loads 1.85-2.48)
          if ((cr & 3u) == 0u) {  // four rays per load: the light rows and the env entries stay 4-aligned
            const uint32_t nlc = nl * cr;
            const uint16_t* ord = A.env_order + (size_t)chunk * (cr * ne);
            for (uint32_t q = threadIdx.x; q < per / 4u; q += kRadBlock) {
                const uint32_t i = 4u * q;
                const float4 v = *reinterpret_cast<const float4*>(tr + i);
                const float vv[4] = {v.x, v.y, v.z, v.w};
                if (i < nlc) {
                    const uint32_t s = i >> A.chunk_shift, rl = i & (cr - 1u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_tr[(rl + j) * S + s] = vv[j];
                } else {
                    const uint2 o = *reinterpret_cast<const uint2*>(ord + (i - nlc));
                    const uint32_t e4[4] = {o.x & 0xffffu, o.x >> 16, o.y & 0xffffu, o.y >> 16};
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_tr[(e4[j] >> 8) * S + nl + (e4[j] & 0xffu)] = vv[j];
                }
            }
          } else
            for (uint32_t i = threadIdx.x; i < per; i += kRadBlock) {
                uint32_t s, rl;
                if (i < nl * cr) {
                    s = i >> A.chunk_shift;
                    rl = i & (cr - 1u);
                } else {
                    const uint32_t v = A.env_order[(size_t)chunk * (cr * ne) + (i - nl * cr)];
                    s = nl + (v & 0xffu);
                    rl = v >> 8;
                }
                s_tr[rl * S + s] = tr[i];
            }
            __syncthreads();
        }
        const uint32_t r = chunk * cr + threadIdx.x;
        if (threadIdx.x < cr && r < nrec) {
            auto t = [&](uint32_t s) { return ORDERED ? s_tr[threadIdx.x * S + s] : tr[s * cr + threadIdx.x]; };
            const float4 pos = A.rec_pos[r];
            float Li0 = 0.0f, Li1 = 0.0f, Li2 = 0.0f;
            for (int l = 0; l < A.num_lights; ++l) {
                const LightRecord& lr = A.lights[l];
                float dx = lr.px - pos.x, dy = lr.py - pos.y, dz = lr.pz - pos.z;
                float dist = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
                float Tr = t((uint32_t)l);
                float d2 = dist * dist;
                Li0 += __fdiv_rn(Tr * lr.ix, d2);
                Li1 += __fdiv_rn(Tr * lr.iy, d2);
                Li2 += __fdiv_rn(Tr * lr.iz, d2);
            }
            float Le0 = 0.0f, Le1 = 0.0f, Le2 = 0.0f;
            for (uint32_t e = 0; e < ne; ++e) {
                float Tr = t(nl + e);
                Le0 += Tr * A.env[0];
                Le1 += Tr * A.env[1];
                Le2 += Tr * A.env[2];
            }
            const float fs = (float)A.env_samples;
            Le0 = __fdiv_rn(Le0, fs) * k4Pi;
            Le1 = __fdiv_rn(Le1, fs) * k4Pi;
            Le2 = __fdiv_rn(Le2, fs) * k4Pi;
            A.rec_rad[r] = make_float4(Li0 + Le0, Li1 + Le1, Li2 + Le2, 0.0f);
        }
        if constexpr (ORDERED) __syncthreads();  // s_tr is reused by the next chunk
    }
}

// TR: a ray grid that asked for the transmittance left at the end of its primary march (out_tr, W x H row-major).
template <bool TR>
__device__ __forceinline__ void accumulate(const RenderArgs& A, [[maybe_unused]] float* __restrict__ out_tr) {
    const uint32_t tile_local = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t p = tile_local * 256u + (uint32_t)tid;
    int lx, ly, x, y;
    tile_pixel(A, tile_local, tid, lx, ly, x, y);
    if (!(x < (int)A.width && y < (int)A.height)) {
        store_px(A, tile_local, lx, ly, x, y, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float step = A.step_size;
    float L0 = 0.0f, L1 = 0.0f, L2 = 0.0f;
    for (uint32_t r = A.px_first[p]; r != kNoRecord; r = A.rec_next[r]) {  // step order
        const float Ts = A.rec_pos[r].w;
        const float4 rad = A.rec_rad[r];  // Li + Le
        L0 += ((Ts * rad.x) * step) * kInv4Pi;
        L1 += ((Ts * rad.y) * step) * kInv4Pi;
        L2 += ((Ts * rad.z) * step) * kInv4Pi;
    }
    const float T = A.px_T[p];
    store_px(A, tile_local, lx, ly, x, y, L0 + T * A.env[0], L1 + T * A.env[1], L2 + T * A.env[2]);
    if constexpr (TR) out_tr[(size_t)y * A.width + (size_t)x] = T;
}

__global__ __launch_bounds__(256) void accumulate_kernel(RenderArgs A) { accumulate<false>(A, nullptr); }
__global__ __launch_bounds__(256) void accumulate_tr_kernel(RenderArgs A, float* __restrict__ out_tr) { accumulate<true>(A, out_tr); }

}  // namespace dev

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
hipError_t gauss_record_cut(const RenderArgs& A, float budget, hipStream_t stream) {
    if (A.rec_cut == nullptr) return hipSuccess;
    hipLaunchKernelGGL(dev::record_cut_kernel, dim3(A.num_tiles), dim3(256), 0, stream, A, budget);
    return hipGetLastError();
}

hipError_t gauss_accumulate(const RenderArgs& A, hipStream_t stream, float* out_tr) {
    {  // (also with no secondary rays: Le = 0 / 0 reproduces the reference's NaN for env_samples = 0)
        const dim3 grid(record_grid(A, A.chunk_rec, 65536));
        if (A.env_order != nullptr)  // <= 64 KB of LDS: env_samples <= kEnvOrderMax, lights <= kMaxLights
            hipLaunchKernelGGL(dev::record_radiance_kernel<true>, grid, dim3(dev::kRadBlock),
                               (size_t)A.chunk_rec * (size_t)(A.num_lights + A.env_samples) * sizeof(float), stream, A);
        else
            hipLaunchKernelGGL(dev::record_radiance_kernel<false>, grid, dim3(dev::kRadBlock), 0, stream, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (out_tr != nullptr) hipLaunchKernelGGL(dev::accumulate_tr_kernel, dim3(A.num_tiles), dim3(256), 0, stream, A, out_tr);
    else hipLaunchKernelGGL(dev::accumulate_kernel, dim3(A.num_tiles), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace vr
