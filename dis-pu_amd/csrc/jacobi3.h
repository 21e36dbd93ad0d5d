// The cyclic Jacobi eigen-solver of a symmetric 3x3 matrix in double, for the kernels that fit a plane to a neighbourhood in registers
// (pca_normals_kernel, mls_project_kernel): the rotation here, the sweeps around it in jacobi3_sweep.h.
#pragma once
#include "common.h"

namespace dispu {

// one Jacobi rotation that zeroes a_pq of a symmetric 3x3 matrix; r is the third index: arp, arq its other two off-diagonals
__device__ __forceinline__ void sym3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                            double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

}  // namespace dispu
