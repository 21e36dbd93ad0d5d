// The per-point arithmetic of the training-batch augmentation, shared by augment_kernel (augment.hip: draws handed in by the
// host) and sample_batch_kernel (batch_sampler.hip: draws made on the device) so that both give the same bits on the same draws:
//   p' = ((p + noise) . R) * scale      (row vector times matrix, np.dot(points, R); jitter -> rotate -> scale)
// -ffp-contract=off: the sums below stay three multiplies and two adds in this order.
#pragma once
#include "common.h"

namespace dispu {

__device__ __forceinline__ void augment_jitter(float& x, float& y, float& z, float nx, float ny, float nz) {
    x += nx; y += ny; z += nz;
}

// R: 9 floats row-major (global memory or registers)
__device__ __forceinline__ void augment_rotate_scale(float x, float y, float z, const float* __restrict__ R, float s, float& ox,
                                                     float& oy, float& oz) {
    ox = (x * R[0] + y * R[3]) + z * R[6];
    oy = (x * R[1] + y * R[4]) + z * R[7];
    oz = (x * R[2] + y * R[5]) + z * R[8];
    ox *= s; oy *= s; oz *= s;
}

}  // namespace dispu
