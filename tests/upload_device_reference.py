"""What vr_upload_gaussians_device promises about the one record word it does not share with the host upload, `norm`
(include/vr_hip.h), restated in numpy for tests/test_upload_device_host.py and tests/test_gpu_upload_device.py.

The device computes (float)(K * (double)(float)(1.0 / sqrt((double)det))): det is the f32 determinant of
precompute_gaussian (vr_scene.cpp, Eigen's bruteforce_det3 expansion along row 0, no contraction) and K is
std::pow(2.0f * pi, -1.5f) evaluated in double on the host. Every operation is an IEEE one, so numpy gives the same
bits. The host's norm is (float)(K * (double)powf(det, -0.5f)): libm's powf and the device's f32 rounding of
1 / sqrt are both faithful roundings of det^-1/2 (powf: under 1 ulp; the double quotient carries a relative error of
2^-52, far below half an f32 ulp's distance to a rounding boundary except at ties), so they are equal or neighbours,
and the product with K, rounded once more, moves neighbours at most one further step apart: 2 ulp."""
import math

import numpy as np

import tree_reference as T

F32 = np.float32
K = (2.0 * math.pi) ** -1.5  # libm's pow in double, as the host evaluates it (2.0f * pi is a double)

BANDS = ((0.005, 0.0175), (0.02, 0.12), (0.1, 0.3))  # axis lengths of the seeded covariances, per scale band


def det_f32(cov6):
    """precompute_gaussian's det_cov for (n, 6) float32 covariances xx xy xz yy yz zz, operation by operation."""
    c = np.asarray(cov6, F32)
    m00, m01, m02, m11, m12, m22 = (c[:, k] for k in range(6))
    m10, m20, m21 = m01, m02, m12
    d0 = m00 * (m11 * m22 - m12 * m21)
    d1 = m01 * (m10 * m22 - m12 * m20)
    d2 = m02 * (m10 * m21 - m11 * m20)
    return d0 - d1 + d2


def device_norm(cov6):
    """The `norm` word of every record after vr_upload_gaussians_device, bit for bit."""
    with np.errstate(all="ignore"):
        rs = (1.0 / np.sqrt(det_f32(cov6).astype(np.float64))).astype(F32)
        return (K * rs.astype(np.float64)).astype(F32)


def ulp_apart(a, b):
    """Distance in f32 steps between finite floats of one sign."""
    return np.abs(np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64) -
                  np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64))


def band_cov(band, n, seed):
    lo, hi = BANDS[band]
    return T.rotated_cov(np.random.default_rng(seed), n, lo, hi)
