// The two loss kernels of the stochastic finite-difference inverse loop (inverse_integrator.h:21-30, 166-182):
// per-pixel L1 losses, and each Gaussian's loss difference summed over the pixels that recorded it.
#include "vr_dev_common.h"

namespace vr {
namespace dev {

// inverse_integrator.h:166-182: out[g] += sum over pixels p whose bit g is set in bits0 or bits1 of
// (loss_plus[p] - loss_base[p]) (double). Grid: (words, pixel chunks); each thread keeps the 32
// Gaussians of its word in registers, a wave reduces them, lane 0 adds them atomically.
__global__ void __launch_bounds__(256) sfd_loss_diff_kernel(const uint32_t* __restrict__ bits0, const uint32_t* __restrict__ bits1,
                                                            const float* __restrict__ loss_base, const float* __restrict__ loss_plus,
                                                            uint32_t npix, uint32_t chunk, uint32_t n, double* out) {
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
        const uint32_t g = w * 32u + (uint32_t)b;
        if ((threadIdx.x & 63) == 0 && v != 0.0 && g < n) atomicAdd(out + g, v);
    }
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

hipError_t launch_sfd_loss_diff(const uint32_t* bits0, const uint32_t* bits1, const float* lb, const float* lp, uint32_t npix,
                                uint32_t n, double* out, hipStream_t stream) {
    const uint32_t words = (n + 31) / 32, chunk = 4096;
    dim3 grid(words, (npix + chunk - 1) / chunk);
    hipLaunchKernelGGL(dev::sfd_loss_diff_kernel, grid, dim3(256), 0, stream, bits0, bits1, lb, lp, npix, chunk, n, out);
    return hipGetLastError();
}

}  // namespace vr
