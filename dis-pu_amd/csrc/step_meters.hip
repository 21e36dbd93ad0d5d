// The train loop's per-step meters in ONE launch (DisPU/model.py:215-222: the five AverageMeters of Model.train_one_epoch).
//
//   row = [pu_loss, 1000 CD_coarse, 100 HD_coarse, 1000 CD_fine, 100 HD_fine]
//
// The three loss values are copied from dispu_pu_loss_finalize's output.  The two Hausdorff terms (loss_utils.py:67-84, logged, never
// differentiated) are reduced from the nearest-neighbour distances the step's own Chamfer terms left behind
// (dispu_nn_distance(gt, pred) -> d_gt [b, n_gt], d_pred [b, n_pred]):
//
//   h_b = (1.0f * max_j d_gt[b, j] + max_j d_pred[b, j]) / radius[b]      (IEEE fp32 division)
//   hd  = max_b h_b,   row entry = 100.0f * hd
//
// operation for operation what loss_utils.hausdorff_loss evaluates through dispu_row_mean_max and torch (train._hausdorff_terms), so the
// row is bit-equal to the values the single-process loop logs.  A maximum does not depend on the order it is taken in, which is what
// lets this kernel pick its own traversal.
//
// Shape: the data is a few hundred KB at most (b <= 32 clouds of 1024 distances, twice, per term): the cost is the launch.  One
// workgroup per term; its waves take the clouds round-robin, a wave reads a row with 16-byte loads over the aligned middle of the row
// (scalar loads for the head up to the first 16-byte boundary and for the tail), folds the lanes' maxima with cross-lane shuffles and
// keeps max_b h_b in a register; the waves' values meet in LDS once, at the end.  No atomics, plain vector stores.
#include "common.h"

namespace dispu {

constexpr int kMeterThreads = 512;                 // 8 waves: one cloud per wave at the 8-patch step
constexpr int kMeterWaves = kMeterThreads / kWave;

// max of x[0 .. n) over the wave's 64 lanes, returned in every lane
__device__ __forceinline__ float wave_row_max(const float* __restrict__ x, int n, int lane) {
    float m = -__builtin_inff();
    // elements in front of the first 16-byte boundary (rows of an odd length start anywhere)
    const int head = min(n, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u));
    if (lane < head) m = x[lane];
    const int n4 = (n - head) >> 2;
    const float4* __restrict__ v = reinterpret_cast<const float4*>(x + head);
    for (int i = lane; i < n4; i += kWave) {
        const float4 q = v[i];
        m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    }
    for (int i = head + (n4 << 2) + lane; i < n; i += kWave) m = fmaxf(m, x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
    return m;
}

__global__ __launch_bounds__(kMeterThreads) void step_meters_kernel(int b, int n_gt, int n_pred, const float* __restrict__ d_gt_c,
                                                                    const float* __restrict__ d_pred_c, const float* __restrict__ d_gt_f,
                                                                    const float* __restrict__ d_pred_f, const float* __restrict__ radius,
                                                                    const float* __restrict__ loss_out, float* __restrict__ row) {
    __shared__ float s_hd[kMeterWaves];
    const int term = blockIdx.x;                   // 0: coarse, 1: fine
    const float* __restrict__ d_gt = term ? d_gt_f : d_gt_c;
    const float* __restrict__ d_pred = term ? d_pred_f : d_pred_c;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    float hd = -__builtin_inff();
    for (int c = wave; c < b; c += kMeterWaves) {
        const float mg = wave_row_max(d_gt + (size_t)c * n_gt, n_gt, lane);
        const float mp = wave_row_max(d_pred + (size_t)c * n_pred, n_pred, lane);
        // hausdorff_loss: forward_weight * max(dists_forward) + max(dists_backward), then / radius.  `/` is the correctly rounded
        // division here (hipcc's default for fp32; the build passes no fast-math flag)
        hd = fmaxf(hd, (1.0f * mg + mp) / radius[c]);
    }
    if (lane == 0) s_hd[wave] = hd;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kMeterWaves; ++w) hd = fmaxf(hd, s_hd[w]);
        // loss_out = dispu_pu_loss_finalize's out: 1000 CD_coarse | 1000 CD_fine | repulsion | pu_loss | weight_fine
        if (term == 0) {
            row[0] = loss_out[3];
            row[1] = loss_out[0];
            row[2] = 100.0f * hd;
        } else {
            row[3] = loss_out[1];
            row[4] = 100.0f * hd;
        }
    }
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_step_meters(int b, int n_gt, int n_pred, const float* d_gt_c, const float* d_pred_c, const float* d_gt_f,
                                   const float* d_pred_f, const float* radius, const float* loss_out, float* row, void* stream) {
    if (b <= 0 || n_gt <= 0 || n_pred <= 0 || !d_gt_c || !d_pred_c || !d_gt_f || !d_pred_f || !radius || !loss_out || !row)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(step_meters_kernel, dim3(2), dim3(kMeterThreads), 0, (hipStream_t)stream, b, n_gt, n_pred, d_gt_c, d_pred_c, d_gt_f,
                       d_pred_f, radius, loss_out, row);
    return (int)hipGetLastError();
}
