// Exact k-NN from one cloud into another over a packed ragged batch, and per-point attributes carried across it: behind
// dispu_knn_cross_segments and dispu_transfer_attributes_segments (include/dispu_hip.h, which states every definition).  The reference
// interpolates features over three neighbours of a brute-force search (Common/pointnet_util.py:204-208, tf_interpolate's three_nn); this
// is that interpolation at any k <= 32 on the exact neighbours of the project's rule, for clouds of scan size.
//
// The frame -- two pre-passes, a seed, the shared search -- is the one of every kernel that searches another cloud (mls_project.hip,
// signed_distance.hip); it exists once, the host side in knn_cross.h and the device side in knn_cross_prologue.h, and is described here.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass) TWICE (knn_cross.h): over the packed references and over the packed queries.  Each
//              wave then holds the 64 queries of one query cell -- spatially coherent, with a box -- and answers through the local index in .w
//   seed       (knn_cross_prologue.h) the wave has no cell of its own in the searched cloud: one sweep of the reference segment's box
//              table finds the cell s with the smallest (box-to-box lower bound, cell number)
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
#include "knn_cross.h"

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
    const int* const status_in = nullptr;                                       // no status carried in
#include "knn_cross_prologue.h"  // segment pair, query cell, query, seed, as text: defines c, lane, n, qbase, rbase, sp, gt, valid, q, s ...
#include "knn_cells_search.h"  // the ramp around s and the walk, as text: defines `kp` and `best`
    if (!valid) return;

    const size_t row = qbase + (size_t)__float_as_int(q.w);
    if constexpr (!XFER) {
        const size_t o = row * (size_t)k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) {
                const bool in = j < kp;
                if (idx_out) idx_out[o + j] = in ? (int)best.index(j) : -1;
                if (d2_out) d2_out[o + j] = in ? best.d2(j) : __uint_as_float(0x7F800000u);
            }
    } else {
        const size_t F = (size_t)x.F;
        const size_t r0 = rbase + (size_t)best.index(0);
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
            if (j < kp) den += 1.0 / fmax((double)best.d2(j), 1e-10);
        for (size_t f = 0; f < F; ++f) {                                        // the weights again per column: 32 doubles would not stay in registers
            double num = 0.0;
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < kp) {
                    const double w = 1.0 / fmax((double)best.d2(j), 1e-10);
                    const double t = w * (double)x.feat[(rbase + (size_t)best.index(j)) * F + f];
                    num += t;
                }
            out[f] = (float)(num / den);
        }
    }
}

static int cross_run(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, const float* queries,
                     const float* refs, int* idx_out, float* d2_out, const XferArgs* x, int width, int* status, void* scratch,
                     size_t scratch_bytes, hipStream_t st) {
    CrossPrepass p(C, qoff_host, roff_host);
    if (p.rc != 0) return p.rc;
    if (k < 1 || k > 32 || !qoff || !roff || !queries || !refs || !status) return (int)hipErrorInvalidValue;
    if ((long long)qoff_host[C] * (long long)width >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (!p.fits(scratch, scratch_bytes)) return (int)hipErrorInvalidValue;
    int rp = p.run_refs(roff, refs, scratch, st);
    if (rp == 0) rp = p.run_queries(qoff, queries, scratch, st);
    if (rp != 0) return rp;
    const dim3 grid = p.grid(), block(kNrmThreads);
    dispatch_kmax(k, [&](auto kmax_c) {
        constexpr int KMAX = decltype(kmax_c)::value;
        if (x)
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, true>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt, p.qtab,
                               p.rtab, k, (int*)nullptr, (float*)nullptr, *x, status);
        else
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, false>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt, p.qtab,
                               p.rtab, k, idx_out, d2_out, XferArgs{0, 0, nullptr, nullptr, nullptr, nullptr}, status);
    });
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_knn_cross_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    return CrossPrepass(C, qoff_host, roff_host).bytes();
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
