// The radiance queries' only prefilter (vr_query_radiance.hip, vr_query_radiance_grad.hip): the interval of t outside
// which no sample point of a ray can be active for a Gaussian.
#pragma once
#include "vr_query_common.h"

namespace vr {
namespace dev {

// The only prefilter: an interval [lo, hi] of t outside which no sample point of the ray can pass sigma_active for
// this Gaussian. False: no sample can (the Gaussian is skipped). It is conservative by the following bound, and where
// the bound's premises fail the interval is the whole row [0, tmax].
//
// In exact arithmetic on the f32 inputs let l(t) = o + t d - mean and Q(t) = l.M l = A t^2 + B t + C. The interval is
// the chord of Q <= 13.5 (not 9), padded by 2^-22 (|lo| + |hi|) >= 2^-22 |B| / A for the roots' own rounding (double,
// then f32). For a sample outside it Q(t) > 13.5, and the kernel's f32 decision differs from Q in two ways:
//   the point: x = fl(o + fl(t d)) is off the line by at most dl = 2^-23 (tmax |d|_inf + |o|_inf) per component
//     (two roundings, u = 2^-24 each, of magnitudes at most |t d| and |t d| + |o|); in the M-norm that is at most
//     s = sqrt(3 tr M) dl, so with p = x - mean: sqrt(p.M p) >= sqrt(13.5) - s;
//   the evaluation: sigma_active rounds p once per component and each term M_ij p_i p_j six more times at most, so its
//     value is p.M p + e with |e| <= 2^-20 m1 |p|^2 <= rho p.M p, m1 = sum_ij |M_ij| >= lambda_max,
//     rho = 2^-20 m1 / lambda_lb, and lambda_lb = 4 det M / (tr M)^2 <= lambda_min (lambda_max lambda_mid <= (tr / 2)^2).
// The premises are s <= 0.1 and rho <= 0.1 (and A > 0, everything finite); then the f32 value is above
// (sqrt(13.5) - 0.1)^2 * 0.9 = 11.4 > 9, and fl(v - 9) <= 0 only if v <= 9: the sample is inactive. rho <= 0.1 also
// bounds the condition number, so the double det and chord carry relative errors far below the slack used here. An
// elongated Gaussian that fails a premise is tested on every valid sample.
__device__ __forceinline__ bool radiance_interval(const GRec& g, const Ray& r, float tmax, float& lo, float& hi) {
    lo = 0.0f;
    hi = tmax;
    const double m00 = g.m00, m01 = g.m01, m02 = g.m02, m11 = g.m11, m12 = g.m12, m22 = g.m22;
    const double tr = m00 + m11 + m22;
    const double m1 = fabs(m00) + fabs(m11) + fabs(m22) + 2.0 * (fabs(m01) + fabs(m02) + fabs(m12));
    const double det = m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02) + m02 * (m01 * m12 - m11 * m02);
    const double dinf = fmax(fabs((double)r.dx), fmax(fabs((double)r.dy), fabs((double)r.dz)));
    const double oinf = fmax(fabs((double)r.ox), fmax(fabs((double)r.oy), fabs((double)r.oz)));
    const double dl = 0x1p-23 * ((double)tmax * dinf + oinf);
    // rho <= 0.1 and s <= 0.1, written so that a NaN fails
    if (!(tr > 0.0 && det > 0.0 && 0x1p-20 * m1 * tr * tr <= 0.4 * det && 3.0 * tr * dl * dl <= 0.01)) return true;
    const double dx = r.dx, dy = r.dy, dz = r.dz;
    const double px = (double)r.ox - (double)g.mx, py = (double)r.oy - (double)g.my, pz = (double)r.oz - (double)g.mz;
    const double mdx = m00 * dx + m01 * dy + m02 * dz, mdy = m01 * dx + m11 * dy + m12 * dz, mdz = m02 * dx + m12 * dy + m22 * dz;
    const double mpx = m00 * px + m01 * py + m02 * pz, mpy = m01 * px + m11 * py + m12 * pz, mpz = m02 * px + m12 * py + m22 * pz;
    const double A = dx * mdx + dy * mdy + dz * mdz;
    const double B = 2.0 * (px * mdx + py * mdy + pz * mdz);
    const double C = px * mpx + py * mpy + pz * mpz - 13.5;
    const double disc = B * B - 4.0 * A * C;
    if (!(A > 0.0) || !(fabs(disc) < INFINITY)) return true;
    if (disc < 0.0) return false;  // the line stays outside Q <= 13.5
    const double sq = sqrt(disc), t0 = (-B - sq) / (2.0 * A), t1 = (-B + sq) / (2.0 * A);
    const double pad = 0x1p-22 * (fabs(t0) + fabs(t1));
    if (!(pad < INFINITY)) return true;
    if (t1 + pad < 0.0 || t0 - pad > (double)tmax) return false;
    lo = fmaxf(lo, (float)(t0 - 2.0 * pad));  // (the conversion's rounding is within the second pad)
    hi = fminf(hi, (float)(t1 + 2.0 * pad));
    return true;
}

}  // namespace dev
}  // namespace vr
