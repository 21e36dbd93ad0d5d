// Exact k-NN from one cloud into another over a packed ragged batch, and per-point attributes carried across it: behind
// dispu_knn_cross_segments and dispu_transfer_attributes_segments (include/dispu_hip.h, which states every definition).  The reference
// interpolates features over three neighbours of a brute-force search (Common/pointnet_util.py:204-208, tf_interpolate's three_nn); this
// is that interpolation at any k <= 32 on the exact neighbours of the project's rule, for clouds of scan size.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass) TWICE: over the packed references and over the packed queries.  Each wave then
//              holds the 64 queries of one query cell -- spatially coherent, with a box -- and answers through the local index in .w
//   seed       Morton keys are relative to each segment's own bounds: a query cell's number says nothing about the reference cells, and
//              the wave has no cell of its own in the searched cloud.  One sweep of the reference segment's box table, 64 boxes per step,
//              finds the cell s with the smallest (box-to-box lower bound, cell number).  Only this sweep is the kernel's own
//   search     the text of knn_cells_search.h, the one the self-searching kernels include, started at s instead of the wave's own cell:
//              the wave visits s and then its neighbours along the curve (s - 1, s + 1, s - 2, ...) until it has seen k' = min(k, m_c)
//              points, then the bounded table walk: a cell is visited unless its box-to-box bound exceeds the wave's largest k-th
//              distance, or its point-to-box bound exceeds the k-th distance of every lane.  A visit is dense: 64 queries x 64 points
//   output     knn: the sorted list, padded with -1 / +inf beyond k'.  transfer: from the list in registers, in double and in ascending
//              rank: w_j = 1 / max(d2_j, 1e-10), out_f = (sum_j w_j feat[r_j][f]) / (sum_j w_j); or the row of rank 0; labels of rank 0
//
// Why a skip is sound: normals.hip's argument asks of the query box only that lo_query <= q <= hi_query for every query of the wave, and
// of the cell's box that lo_cell <= p <= hi_cell for its points.  It never uses that the query box is a cell of the searched cloud, so
// lb <= d2 bit for bit holds with the box of a query cell from the OTHER pre-pass.  The seeds only fill the lists: whichever cells they
// are, afterwards every cell outside [vlo, vhi] is tested, and skipped only on lb > k-th strictly (k-th = +inf while a list is short).
//
// Ordinary stores only, no atomics of its own, ordering by kernel boundaries only, identical bytes from run to run.
#include "knn_cells.h"

namespace dispu {

struct XferArgs {
    int mode, F;                                                                // mode 0: inverse-distance weights, 1: the nearest row
    const float* feat;
    float* out_feat;
    const int* labels;
    int* out_labels;
};

template <int KMAX, bool XFER>
__global__ __launch_bounds__(kNrmThreads) void knn_cross_kernel(const int* __restrict__ qoff, const int* __restrict__ roff,
                                                                const uint32_t* __restrict__ qsegb, const uint32_t* __restrict__ rsegb,
                                                                const float4* __restrict__ qspt, const float4* __restrict__ rspt,
                                                                const float* __restrict__ qtab, const float* __restrict__ rtab, int k,
                                                                int* __restrict__ idx_out, float* __restrict__ d2_out, XferArgs x,
                                                                int* __restrict__ status) {
#pragma clang fp contract(off)      // pinned here as well as by the build's -ffp-contract=off: the weights below round once per operation
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qb0 = qoff[c], nq = qoff[c + 1] - qb0;
    const int rb0 = roff[c], n = roff[c + 1] - rb0;
    const size_t qbase = (size_t)qb0, rbase = (size_t)rb0;
    const uint32_t bad = qsegb[(size_t)c * 8 + 6] | rsegb[(size_t)c * 8 + 6];
    if (blockIdx.x == 0 && tid == 0) status[c] = bad ? 1 : 0;
    if (bad) return;                                                            // nothing is written for a non-finite segment
    const int KQ = (nq + kNrmCell - 1) / kNrmCell, K = (n + kNrmCell - 1) / kNrmCell;
    const int cb = blockIdx.x * kNrmWaves + wave;
    if (cb >= KQ) return;                                                       // wave-uniform
    const float4* __restrict__ sp = rspt + rbase;
    const float* __restrict__ gt = rtab + fpc_cell_base(rbase, c) * 8;
    const float* __restrict__ qgt = qtab + fpc_cell_base(qbase, c) * 8;
    const int qcnt = min(kNrmCell, nq - cb * kNrmCell);
    const bool valid = lane < qcnt;
    const float4 q = qspt[qbase + (size_t)(cb * kNrmCell + (valid ? lane : 0))];   // idle lanes repeat query 0 and store nothing
    const float4 qlo4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8);
    const float4 qhi4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8 + 4);

    // the seed: the reference cell of the smallest (box-to-box bound, cell number).  Lane 0 always holds cell 0, so s < K
    uint64_t sk = kNrmNone;
    for (int j0 = 0; j0 < K; j0 += kWave) {
        const int j = j0 + lane;
        if (j < K) {
            const float4 a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            const float4 b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            const float lb = cell_box_lb(a, b, qlo4.x, qlo4.y, qlo4.z, qlo4.w, qhi4.x, qhi4.y);
            const uint64_t key = ((uint64_t)__float_as_uint(lb) << 32) | (uint32_t)j;
            sk = key < sk ? key : sk;
        }
    }
    const int s = min((int)(uint32_t)wave_min_u64(sk), K - 1);
#include "knn_cells_search.h"  // the ramp around s and the walk, as text: defines `kp` and `best`
    if (!valid) return;

    const size_t row = qbase + (size_t)__float_as_int(q.w);
    if constexpr (!XFER) {
        const size_t o = row * (size_t)k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) {
                const bool in = j < kp;
                if (idx_out) idx_out[o + j] = in ? (int)(uint32_t)best.b[j] : -1;
                if (d2_out) d2_out[o + j] = in ? __uint_as_float((uint32_t)(best.b[j] >> 32)) : __uint_as_float(0x7F800000u);
            }
    } else {
        const size_t F = (size_t)x.F;
        const size_t r0 = rbase + (size_t)(uint32_t)best.b[0];
        if (x.labels) x.out_labels[row] = x.labels[r0];
        if (!x.feat) return;
        float* __restrict__ out = x.out_feat + row * F;
        if (x.mode == 1) {
            for (size_t f = 0; f < F; ++f) out[f] = x.feat[r0 * F + f];
            return;
        }
        double den = 0.0;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < kp) den += 1.0 / fmax((double)__uint_as_float((uint32_t)(best.b[j] >> 32)), 1e-10);
        for (size_t f = 0; f < F; ++f) {                                        // the weights again per column: 32 doubles would not stay in registers
            double num = 0.0;
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < kp) {
                    const double w = 1.0 / fmax((double)__uint_as_float((uint32_t)(best.b[j] >> 32)), 1e-10);
                    const double t = w * (double)x.feat[(rbase + (size_t)(uint32_t)best.b[j]) * F + f];
                    num += t;
                }
            out[f] = (float)(num / den);
        }
    }
}

static int cross_run(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, const float* queries,
                     const float* refs, int* idx_out, float* d2_out, const XferArgs* x, int width, int* status, void* scratch,
                     size_t scratch_bytes, hipStream_t st) {
    int rc = cells_batch_check(C, qoff_host);
    if (rc == 0) rc = cells_batch_check(C, roff_host);
    if (rc != 0) return rc;
    if (k < 1 || k > 32 || !qoff || !roff || !queries || !refs || !status) return (int)hipErrorInvalidValue;
    if ((long long)qoff_host[C] * (long long)width >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const size_t rbytes = fps_cells_prepass_scratch(C, roff_host), qbytes = fps_cells_prepass_scratch(C, qoff_host);
    if (!rbytes || !qbytes || !scratch || scratch_bytes < rbytes + qbytes || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    const float4 *rspt, *qspt;
    const float *rtab, *qtab;
    const uint32_t *rsegb, *qsegb;
    int kr = 0, kqmax = 0;
    int rp = fps_cells_prepass(C, roff, roff_host, refs, scratch, rbytes, &rspt, &rtab, &rsegb, &kr, st);
    if (rp != 0) return rp;
    rp = fps_cells_prepass(C, qoff, qoff_host, queries, (char*)scratch + rbytes, qbytes, &qspt, &qtab, &qsegb, &kqmax, st);   // rbytes is a multiple of 256
    if (rp != 0) return rp;
    const dim3 grid((kqmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
    dispatch_kmax(k, [&](auto kmax_c) {
        constexpr int KMAX = decltype(kmax_c)::value;
        if (x)
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, true>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab, rtab, k,
                               (int*)nullptr, (float*)nullptr, *x, status);
        else
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, false>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab, rtab, k,
                               idx_out, d2_out, XferArgs{0, 0, nullptr, nullptr, nullptr, nullptr}, status);
    });
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_knn_cross_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    const size_t rbytes = fps_cells_prepass_scratch(C, roff_host), qbytes = fps_cells_prepass_scratch(C, qoff_host);
    return rbytes && qbytes ? rbytes + qbytes : 0;
}

DISPU_EXPORT int dispu_knn_cross_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                                          const float* queries, const float* refs, int* idx_out, float* d2_out, int* status, void* scratch,
                                          size_t scratch_bytes, void* stream) {
    if (!idx_out && !d2_out) return (int)hipErrorInvalidValue;
    return cross_run(C, qoff, qoff_host, roff, roff_host, k, queries, refs, idx_out, d2_out, nullptr, k, status, scratch, scratch_bytes,
                     (hipStream_t)stream);
}

DISPU_EXPORT int dispu_transfer_attributes_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host,
                                                    int k, int mode, const float* queries, const float* refs, int F, const float* feat,
                                                    float* out_feat, const int* labels, int* out_labels, int* status, void* scratch,
                                                    size_t scratch_bytes, void* stream) {
    if (mode < 0 || mode > 1 || F < 1 || (!feat && !labels) || (feat && !out_feat) || (labels && !out_labels))
        return (int)hipErrorInvalidValue;
    const XferArgs x{mode, F, feat, out_feat, labels, out_labels};
    return cross_run(C, qoff, qoff_host, roff, roff_host, k, queries, refs, nullptr, nullptr, &x, k > F ? k : F, status, scratch,
                     scratch_bytes, (hipStream_t)stream);
}
