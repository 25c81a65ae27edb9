// jacobi3.h — the cyclic Jacobi rotation of a symmetric 3 x 3 matrix in fp64 that point_cloud.hip (normals from a neighbourhood's
// covariance) and point_segment.hip (the least-squares plane through a plane's inliers) share, written ONCE.  A sweep is the three
// rotations (0,1), (0,2), (1,2); a caller runs JACOBI_SWEEPS of them, a fixed number, and reads the eigenvalues off the diagonal.
#pragma once
#include "sgam_common.h"

namespace {

// Sweeps of the cyclic Jacobi iteration.  Measured on the test clouds (noisy plane, sphere, cylinder, 2000 points each, k = 16) with
// this loop restated in numpy (tests/cloud_oracle.py: jacobi_eigh) against numpy.linalg.eigh — the largest off-diagonal mass left,
// relative to the trace, and the largest 1 - |n . n_eigh|: 3 sweeps 4e-6 / 2e-12, 4 sweeps 3e-22 / 9e-16 (the rounding floor),
// 5 sweeps 1e-90.  Four are needed; 6 leaves two sweeps of margin (tests/test_cloud_cpu.py asserts both).
constexpr int JACOBI_SWEEPS = 6;

// one Jacobi rotation of the symmetric 3 x 3 A (and of the eigenvector columns p, q of V) that zeroes a_pq; r is the third index
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &apr, double &aqr, double &v0p, double &v0q,
                                              double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double pr = apr, qr = aqr;
    apr = c * pr - s * qr;
    aqr = s * pr + c * qr;
    double a = v0p, b = v0q;
    v0p = c * a - s * b; v0q = s * a + c * b;
    a = v1p; b = v1q;
    v1p = c * a - s * b; v1q = s * a + c * b;
    a = v2p; b = v2q;
    v2p = c * a - s * b; v2q = s * a + c * b;
}

}  // namespace
