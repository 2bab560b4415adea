// What the RayMarchingGaussians pipeline (vr_gauss_common.h) prepares once per scene upload: the 4-wide tree's
// parents and primitive-to-node map, the secondary rays' tight tree with its per-axis copy, and the whitened
// records, with the launchers gauss_parents, gauss_refit_secondary, gauss_soa_nodes and gauss_whiten.
#include "vr_gauss_common.h"

namespace vr {
namespace dev {

// Parent of every 4-wide node with the node's slot in it: parent | (slot + 1) << 28 (root: -1).
__global__ __launch_bounds__(256) void parents_kernel(const HNode4* __restrict__ nodes, uint32_t n, int32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (i == 0) parent[0] = -1;
    const int4 c = reinterpret_cast<const int4*>(nodes + i)[3];
    if (c.x > 0) parent[c.x] = (int32_t)(i | (1u << 28));
    if (c.y > 0) parent[c.y] = (int32_t)(i | (2u << 28));
    if (c.z > 0) parent[c.z] = (int32_t)(i | (3u << 28));
    if (c.w > 0) parent[c.w] = (int32_t)(i | (4u << 28));
}

// ---- the secondary rays' own 4-wide tree: the same nodes with tight boxes (round 4) -------------------
// The shared tree's boxes are the primitives' 3-sigma boxes padded by 5 % (gaussian_bounds): the exact
// M-form quadratic of the primary and free-flight rays, evaluated from a camera several units away,
// accepts points a few percent outside the ellipsoid, and their boxes must hold those. The secondary
// rays' whitened test takes the distance from the chord to the centre directly (wquad: |Lp - (h/a) Ld|^2,
// error linear in the origin's whitened distance instead of quadratic), so what it accepts lies within
// ~1e-5 of the ellipsoid, and their tree gets the exact box of {x : x^T M x <= 9}: half extent
// 3 sqrt((M^-1)_kk) from the record's M in double, outward rounding, and a relative pad of
// 2e-4 + 3.2e-7 rw, rw = diag sqrt(trace M) >= the whitened distance of any origin in the scene box
// (diagonal diag): the chord distance's f32 error is ~1.4e-6 rw in e2, i.e. ~8e-8 rw of the radius, so
// the pad keeps a factor >= 4 at any scene scale (C4: 2e-4 .. 6e-4). C4: 9.5 % fewer node steps and 19 %
// fewer primitive tests.
__device__ __forceinline__ uint16_t f16_out(double v, bool up) {  // smallest half >= v (up) / largest <= v
    uint16_t h = __builtin_bit_cast(uint16_t, (_Float16)(float)v);
    for (int it = 0; it < 4; ++it) {
        const double hv = (double)__builtin_bit_cast(_Float16, h);
        if (up ? hv >= v : hv <= v) break;
        const bool neg = (h & 0x8000u) != 0;
        if ((h & 0x7fffu) == 0) h = up ? 0x0001u : 0x8001u;
        else h = (uint16_t)((neg != up) ? h + 1 : h - 1);
    }
    return h;
}
// Tight box of record j (f32, rounded outward); a record whose M is not positive definite keeps an
// infinite box (the secondary kernel then runs the M forms on the shared tree anyway).
__device__ __forceinline__ void tight_box(const GaussianRecord& g, float diag, float lo[3], float hi[3]) {
    const double m0 = g.m00, m1 = g.m01, m2 = g.m02, m3 = g.m11, m4 = g.m12, m5 = g.m22;
    const double c00 = m3 * m5 - m4 * m4, c11 = m0 * m5 - m2 * m2, c22 = m0 * m3 - m1 * m1;
    const double c01 = m2 * m4 - m1 * m5, c02 = m1 * m4 - m2 * m3;
    const double det = m0 * c00 + m1 * c01 + m2 * c02;
    const double s[3] = {c00 / det, c11 / det, c22 / det};
    const double mean[3] = {g.mx, g.my, g.mz};
    const bool pd = m0 > 0.0 && c22 > 0.0 && det > 0.0 && s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0;
    const double pad = 1.0 + 2e-4 + 3.2e-7 * (double)diag * sqrt(m0 + m3 + m5);
    for (int k = 0; k < 3; ++k) {
        const double h = pd ? 3.0 * sqrt(s[k]) * pad + 1e-6 : INFINITY;
        lo[k] = __double2float_rd(mean[k] - h);
        hi[k] = __double2float_ru(mean[k] + h);
    }
}
// Depth of every 4-wide node (from the parents) and the deepest.
__global__ __launch_bounds__(256) void node_depth_kernel(const int32_t* __restrict__ parent, uint32_t n, uint8_t* __restrict__ depth,
                                                         uint32_t* __restrict__ maxd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t d = 0;
    for (int32_t x = (int32_t)i; x > 0 && d < 255u; x = parent[x] & kNodeIndexMask) ++d;
    depth[i] = (uint8_t)d;
    atomicMax(maxd, d);
}
// One level of the refit, deepest first: every node at `level` gets its children's tight boxes (a leaf:
// the union of its records' boxes; an inner child: the union its own refit left in nbox) as outward
// rounded f16 in the shared tree's normalisation, and leaves the union of them in nbox for its parent.
__global__ __launch_bounds__(256) void refit_kernel(const HNode4* __restrict__ src, HNode4* __restrict__ dst,
                                                    const GaussianRecord* __restrict__ rec, const uint8_t* __restrict__ depth,
                                                    uint32_t level, uint32_t n, float* __restrict__ nbox, float3 hc, float hs,
                                                    float diag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || depth[i] != level) return;
    HNode4 h = src[i];
    float ul[3] = {INFINITY, INFINITY, INFINITY}, uh[3] = {-INFINITY, -INFINITY, -INFINITY};
    const double c[3] = {hc.x, hc.y, hc.z};
    for (int s = 0; s < 4; ++s) {
        const int32_t r = h.c[s];
        if (r == 0) continue;  // empty slot: its NaN box stays
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (r < 0) {
            const uint32_t first = leaf_first(r), cnt = leaf_count(r);
            for (uint32_t j = first; j < first + cnt; ++j) {
                float a[3], b[3];
                tight_box(rec[j], diag, a, b);
                for (int k = 0; k < 3; ++k) {
                    lo[k] = fminf(lo[k], a[k]);
                    hi[k] = fmaxf(hi[k], b[k]);
                }
            }
        } else {
            for (int k = 0; k < 3; ++k) {
                lo[k] = nbox[6 * (size_t)r + k];
                hi[k] = nbox[6 * (size_t)r + 3 + k];
            }
        }
        for (int k = 0; k < 3; ++k) {
            ul[k] = fminf(ul[k], lo[k]);
            uh[k] = fmaxf(uh[k], hi[k]);
            // never wider than the shared tree's box (both hold the child; the tighter one is kept)
            const uint16_t a = f16_out(((double)lo[k] - c[k]) * (double)hs, false);
            const uint16_t b = f16_out(((double)hi[k] - c[k]) * (double)hs, true);
            const float sa = (float)__builtin_bit_cast(_Float16, h.h[s][k]), sb = (float)__builtin_bit_cast(_Float16, h.h[s][3 + k]);
            if ((float)__builtin_bit_cast(_Float16, a) > sa) h.h[s][k] = a;
            if ((float)__builtin_bit_cast(_Float16, b) < sb) h.h[s][3 + k] = b;
        }
    }
    dst[i] = h;
    for (int k = 0; k < 3; ++k) {
        nbox[6 * (size_t)i + k] = ul[k];
        nbox[6 * (size_t)i + 3 + k] = uh[k];
    }
}

// The secondary rays' per-axis node copy: node i's words 4a..4a+3 hold axis a's box bounds as f16
// pairs {min of children 0, 1}, {min of 2, 3}, {max of 0, 1}, {max of 2, 3}; words 12-15 the child refs. A ray
// picks its near and far bound of an axis once per node (the sign of its direction), for all four children at
// once, instead of a min and a max per child and axis (sec_node4v).
__global__ __launch_bounds__(256) void soa_nodes_kernel(const HNode4* __restrict__ src, HNode4* __restrict__ dst, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const HNode4 a = src[i];
    uint32_t w[16];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        w[4 * ax + 0] = (uint32_t)a.h[0][ax] | ((uint32_t)a.h[1][ax] << 16);
        w[4 * ax + 1] = (uint32_t)a.h[2][ax] | ((uint32_t)a.h[3][ax] << 16);
        w[4 * ax + 2] = (uint32_t)a.h[0][3 + ax] | ((uint32_t)a.h[1][3 + ax] << 16);
        w[4 * ax + 3] = (uint32_t)a.h[2][3 + ax] | ((uint32_t)a.h[3][3 + ax] << 16);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) w[12 + k] = (uint32_t)a.c[k];
    uint4* o = reinterpret_cast<uint4*>(dst + i);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
    o[3] = make_uint4(w[12], w[13], w[14], w[15]);
}

// The 4-wide node whose child is each primitive's leaf (record_start_kernel's shortcut, vr_gauss_secondary.hip).
__global__ __launch_bounds__(256) void prim_node_kernel(const HNode4* __restrict__ nodes, uint32_t n, int32_t* __restrict__ map) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4*>(nodes + i)[3];
    const int32_t ref[4] = {c.x, c.y, c.z, c.w};
    for (int s = 0; s < 4; ++s)
        if (ref[s] < 0)
            for (uint32_t j = leaf_first(ref[s]); j < leaf_first(ref[s]) + leaf_count(ref[s]); ++j) map[j] = (int32_t)i;
}

// WRecord of every record (vr_internal.h): Cholesky factor of M = Sigma^-1 in double. A record whose M
// is not positive definite gets NaN factors (wintersect never reports a crossing for it).
__global__ __launch_bounds__(256) void whiten_kernel(const GaussianRecord* __restrict__ rec, WRecord* __restrict__ out,
                                                     uint32_t n, uint32_t* bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const GaussianRecord g = rec[i];
    const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
    const double l00 = sqrt(m00), l01 = m01 / l00, l02 = m02 / l00;
    const double l11 = sqrt(m11 - l01 * l01), l12 = (m12 - l01 * l02) / l11;
    const double l22 = sqrt(m22 - l02 * l02 - l12 * l12);
    const bool pd = l00 > 0.0 && l11 > 0.0 && l22 > 0.0;  // (sqrt of a negative pivot: NaN, fails too)
    if (!pd) atomicAdd(bad, 1u);  // the host then traces the scene's secondary rays with the M forms
    const float nan = __builtin_nanf("");
    const float dn = (float)((double)g.density * (double)g.norm * 1.2533141373155002512);  // sqrt(pi / 2)
    out[i] = WRecord{g.mx, g.my, g.mz, dn, pd ? (float)l00 : nan, (float)l01, (float)l02, (float)l11,
                     (float)l12, (float)l22, 0.0f, 0.0f};
}

}  // namespace dev

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
hipError_t gauss_parents(const HNode4* nodes, uint32_t n, int32_t* parent, int32_t* prim_node, hipStream_t stream) {
    hipLaunchKernelGGL(dev::parents_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, nodes, n, parent);
    if (prim_node != nullptr) hipLaunchKernelGGL(dev::prim_node_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, nodes, n, prim_node);
    return hipGetLastError();
}

// The secondary rays' tree (refit_kernel): nodes 0..n-1 of `src` with tight boxes into `dst`. Scratch:
// depth (n B), nbox (24 n B), maxd (one word, device) and host_maxd (pinned or pageable host word).
hipError_t gauss_refit_secondary(const HNode4* src, HNode4* dst, HNode4* dst_t, uint32_t n, const GaussianRecord* rec,
                                 const int32_t* parent, uint8_t* depth, float* nbox, uint32_t* maxd, const float hc[3], float hs,
                                 float diag, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(maxd, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::node_depth_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, parent, n, depth, maxd);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t md = 0;
    if ((e = hipMemcpyAsync(&md, maxd, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (md >= 255u) return hipErrorNotSupported;
    const float3 c = make_float3(hc[0], hc[1], hc[2]);
    for (int level = (int)md; level >= 0; --level) {
        hipLaunchKernelGGL(dev::refit_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, dst, rec, depth, (uint32_t)level, n,
                           nbox, c, hs, diag);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (dst_t != nullptr) {
        hipLaunchKernelGGL(dev::soa_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, dst, dst_t, n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t gauss_soa_nodes(const HNode4* src, HNode4* dst, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::soa_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, dst, n);
    return hipGetLastError();
}

hipError_t gauss_whiten(const GaussianRecord* rec, WRecord* out, uint32_t n, uint32_t* bad, hipStream_t stream) {
    hipLaunchKernelGGL(dev::whiten_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rec, out, n, bad);
    return hipGetLastError();
}

}  // namespace vr
