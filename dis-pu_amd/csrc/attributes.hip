// Exact k-NN from one cloud into another over a packed ragged batch, and per-point attributes carried across it: behind
// dispu_knn_cross_segments and dispu_transfer_attributes_segments (include/dispu_hip.h, which states every definition).  The reference
// interpolates features over three neighbours of a brute-force search (Common/pointnet_util.py:204-208, tf_interpolate's three_nn); this
// is that interpolation at any k <= 32 on the exact neighbours of the project's rule, for clouds of scan size.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass) TWICE: over the packed references and over the packed queries.  Each wave then
//              holds the 64 queries of one query cell -- spatially coherent, with a box -- and answers through the local index in .w
//   seed       Morton keys are relative to each segment's own bounds: a query cell's number says nothing about the reference cells, and
//              the wave has no cell of its own in the searched cloud.  One sweep of the reference segment's box table, 64 boxes per step,
//              finds the cell with the smallest (box-to-box lower bound, cell number); the wave visits it and then its neighbours along
//              the curve (s - 1, s + 1, s - 2, ...) until it has seen k' = min(k, m_c) points
//   walk       the bounded table walk of knn_cells_search.h: a cell is visited unless its box-to-box bound exceeds the wave's largest k-th
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
    const int kp = min(k, n);
    const float4 qlo4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8);
    const float4 qhi4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8 + 4);
    const float qlx = qlo4.x, qly = qlo4.y, qlz = qlo4.z, qhx = qlo4.w, qhy = qhi4.x, qhz = qhi4.y;

    NrmBest<KMAX> best;
    best.init();
    auto visit = [&](int j) {                                                   // j wave-uniform: all 64 queries against cell j
        const int cnt = min(kNrmCell, n - j * kNrmCell);
        const float4 p = sp[j * kNrmCell + min(lane, cnt - 1)];
        for (int i = 0; i < cnt; ++i) {
            const float px = __shfl(p.x, i, kWave), py = __shfl(p.y, i, kWave), pz = __shfl(p.z, i, kWave);
            const uint32_t pi = (uint32_t)__shfl(__float_as_int(p.w), i, kWave);
            const float d = sqdist3<false>(px - q.x, py - q.y, pz - q.z);
            best.push(((uint64_t)__float_as_uint(d) << 32) | pi, k);
        }
    };

    // the seed: the reference cell of the smallest (box-to-box bound, cell number).  Lane 0 always holds cell 0, so s < K
    uint64_t sk = kNrmNone;
    for (int j0 = 0; j0 < K; j0 += kWave) {
        const int j = j0 + lane;
        if (j < K) {
            const float4 a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            const float4 b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            const uint64_t key = ((uint64_t)__float_as_uint(cell_box_lb(a, b, qlx, qly, qlz, qhx, qhy, qhz)) << 32) | (uint32_t)j;
            sk = key < sk ? key : sk;
        }
    }
    const int s = min((int)(uint32_t)wave_min_u64(sk), K - 1);
    visit(s);
    int seen = min(kNrmCell, n - s * kNrmCell), vlo = s, vhi = s;
    for (int d = 1; seen < kp; ++d) {                                           // kp <= n: ends at the latest with every cell visited
        if (s - d >= 0) { visit(s - d); seen += kNrmCell; vlo = s - d; }        // only the last cell of a segment is short, and it
        if (s + d < K) { visit(s + d); seen += min(kNrmCell, n - (s + d) * kNrmCell); vhi = s + d; }   // is never at s - d
    }

    uint32_t wk = (uint32_t)(wave_max_u64(best.thr) >> 32);                     // bits of the wave's largest k-th distance
    for (int j0 = 0; j0 < K; j0 += kWave) {
        const int j = j0 + lane;
        uint32_t lbb = 0xFFFFFFFFu;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        const bool open = j < K && (j < vlo || j > vhi);
        if (open) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            lbb = __float_as_uint(cell_box_lb(a, b, qlx, qly, qlz, qhx, qhy, qhz));
        }
        unsigned long long reach = __ballot(open && lbb <= wk);
        while (reach) {
            const int bl = (int)__builtin_ctzll(reach);
            reach &= reach - 1;
            const uint32_t lb1 = (uint32_t)__shfl((int)lbb, bl, kWave);
            if (lb1 > wk) continue;                                             // the k-th distance shrank since the ballot
            // the same bound per lane, the query point as its own box: a cell no lane can gain from is not visited either
            const float4 a1 = make_float4(__shfl(a.x, bl, kWave), __shfl(a.y, bl, kWave), __shfl(a.z, bl, kWave), __shfl(a.w, bl, kWave));
            const float4 b1 = make_float4(__shfl(b.x, bl, kWave), __shfl(b.y, bl, kWave), 0.f, 0.f);
            if (!__any(__float_as_uint(cell_box_lb(a1, b1, q.x, q.y, q.z, q.x, q.y, q.z)) <= (uint32_t)(best.thr >> 32))) continue;
            visit(j0 + bl);
            wk = (uint32_t)(wave_max_u64(best.thr) >> 32);
        }
    }
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

// -> 0 and the largest cell count of a query segment, or hipErrorInvalidValue: C outside 1 .. 65535, offsets that do not start at 0 or do
// not grow, a segment above 2^24 points, on either side
static int cross_plan(int C, const int* qoff_host, const int* roff_host, int* kqmax) {
    int nall, nserved, krmax;
    const int rc = fpc_plan(C, qoff_host, qoff_host, 0, kCellsFixed64, &nall, &nserved, kqmax);
    if (rc != 0) return rc;
    return fpc_plan(C, roff_host, roff_host, 0, kCellsFixed64, &nall, &nserved, &krmax);
}

static int cross_run(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, const float* queries,
                     const float* refs, int* idx_out, float* d2_out, const XferArgs* x, int width, int* status, void* scratch,
                     size_t scratch_bytes, hipStream_t st) {
    int kqmax = 0;
    const int rc = cross_plan(C, qoff_host, roff_host, &kqmax);
    if (rc != 0) return rc;
    if (k < 1 || k > 32 || !qoff || !roff || !queries || !refs || !status) return (int)hipErrorInvalidValue;
    if ((long long)qoff_host[C] * (long long)width >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const size_t rbytes = fps_cells_prepass_scratch(C, roff_host), qbytes = fps_cells_prepass_scratch(C, qoff_host);
    if (!rbytes || !qbytes || !scratch || scratch_bytes < rbytes + qbytes || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    const float4 *rspt, *qspt;
    const float *rtab, *qtab;
    const uint32_t *rsegb, *qsegb;
    int kr = 0;
    int rp = fps_cells_prepass(C, roff, roff_host, refs, scratch, rbytes, &rspt, &rtab, &rsegb, &kr, st);
    if (rp != 0) return rp;
    rp = fps_cells_prepass(C, qoff, qoff_host, queries, (char*)scratch + rbytes, qbytes, &qspt, &qtab, &qsegb, &kqmax, st);   // rbytes is a multiple of 256
    if (rp != 0) return rp;
    const dim3 grid((kqmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
#define DISPU_CROSS_LAUNCH(KMAX)                                                                                                        \
    do {                                                                                                                                \
        if (x)                                                                                                                          \
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, true>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab, rtab, k, \
                               (int*)nullptr, (float*)nullptr, *x, status);                                                             \
        else                                                                                                                            \
            hipLaunchKernelGGL((knn_cross_kernel<KMAX, false>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab, rtab, k, \
                               idx_out, d2_out, XferArgs{0, 0, nullptr, nullptr, nullptr, nullptr}, status);                            \
    } while (0)
    if (k <= 8)
        DISPU_CROSS_LAUNCH(8);
    else if (k <= 16)
        DISPU_CROSS_LAUNCH(16);
    else
        DISPU_CROSS_LAUNCH(32);
#undef DISPU_CROSS_LAUNCH
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_knn_cross_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    int kqmax;
    if (cross_plan(C, qoff_host, roff_host, &kqmax) != 0) return 0;
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
