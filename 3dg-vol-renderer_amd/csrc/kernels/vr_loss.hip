// The two loss kernels of the stochastic finite-difference inverse loop (inverse_integrator.h:21-30, 166-182):
// per-pixel L1 losses, and each Gaussian's loss difference summed over the pixels that recorded it.
#include "vr_dev_common.h"

namespace vr {
namespace dev {

constexpr uint32_t kSfdChunk = 4096;  // pixels per block of sfd_loss_diff_kernel

// inverse_integrator.h:166-182: the sum over pixels p whose bit g is set in bits0 or bits1 of
// (loss_plus[p] - loss_base[p]) (double), in two passes whose order of additions is fixed, so the result
// is the same in every run. Grid: (words, pixel chunks); each thread keeps the 32 Gaussians of its word
// in registers, a wave reduces them, the block adds its four waves in wave order and stores the chunk's
// partial sums: partial[chunk][32 * words] (every entry is written). sfd_sum_chunks_kernel adds the chunks
// in chunk order.
__global__ void __launch_bounds__(256) sfd_loss_diff_kernel(const uint32_t* __restrict__ bits0, const uint32_t* __restrict__ bits1,
                                                            const float* __restrict__ loss_base, const float* __restrict__ loss_plus,
                                                            uint32_t npix, uint32_t chunk, double* __restrict__ partial) {
    __shared__ double wave_sum[4][32];
    const uint32_t w = blockIdx.x;
    const uint32_t p0 = blockIdx.y * chunk, p1 = min(npix, p0 + chunk);
    double acc[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) acc[b] = 0.0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const uint32_t word = bits0[(size_t)w * npix + p] | bits1[(size_t)w * npix + p];
        if (!word) continue;
        const double d = (double)loss_plus[p] - (double)loss_base[p];
#pragma unroll
        for (int b = 0; b < 32; ++b)
            if ((word >> b) & 1u) acc[b] += d;
    }
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        double v = acc[b];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][b] = v;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const uint32_t b = threadIdx.x;
        partial[((size_t)blockIdx.y * gridDim.x + w) * 32u + b] = ((wave_sum[0][b] + wave_sum[1][b]) + wave_sum[2][b]) + wave_sum[3][b];
    }
}

// out[g] = partial[0][g] + partial[1][g] + ... (chunk order), g < n <= stride.
__global__ void __launch_bounds__(256) sfd_sum_chunks_kernel(const double* __restrict__ partial, uint32_t nchunks, uint32_t stride,
                                                             uint32_t n, double* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    double acc = 0.0;
    for (uint32_t y = 0; y < nchunks; ++y) acc += partial[(size_t)y * stride + g];
    out[g] = acc;
}

// compute_pixel_losses (inverse_integrator.h:21-30): per-pixel L1 over RGB, d.cwiseAbs().sum()
// (Eigen's 3-term reduction: |d0| + (|d1| + |d2|)).
__global__ void __launch_bounds__(256) pixel_loss_kernel(const float* __restrict__ img, const float* __restrict__ ref,
                                                         uint32_t npix, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float d0 = img[3 * (size_t)p] - ref[3 * (size_t)p];
    const float d1 = img[3 * (size_t)p + 1] - ref[3 * (size_t)p + 1];
    const float d2 = img[3 * (size_t)p + 2] - ref[3 * (size_t)p + 2];
    out[p] = fabsf(d0) + (fabsf(d1) + fabsf(d2));
}

}  // namespace dev

hipError_t launch_pixel_losses(const float* img, const float* ref, uint32_t npix, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(dev::pixel_loss_kernel, dim3((npix + 255) / 256), dim3(256), 0, stream, img, ref, npix, out);
    return hipGetLastError();
}

size_t sfd_partial_count(uint32_t npix, uint32_t n) {
    return (size_t)((npix + dev::kSfdChunk - 1) / dev::kSfdChunk) * ((n + 31) / 32) * 32;
}

hipError_t launch_sfd_loss_diff(const uint32_t* bits0, const uint32_t* bits1, const float* lb, const float* lp, uint32_t npix,
                                uint32_t n, double* partial, double* out, hipStream_t stream) {
    const uint32_t words = (n + 31) / 32, nchunks = (npix + dev::kSfdChunk - 1) / dev::kSfdChunk;
    if (words == 0 || nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::sfd_loss_diff_kernel, dim3(words, nchunks), dim3(256), 0, stream, bits0, bits1, lb, lp, npix,
                       dev::kSfdChunk, partial);
    hipLaunchKernelGGL(dev::sfd_sum_chunks_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, partial, nchunks, words * 32u, n, out);
    return hipGetLastError();
}

}  // namespace vr
