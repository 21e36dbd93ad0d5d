// The implicit function of an oriented cloud at arbitrary positions (an IMLS / Hoppe signed distance), over a packed ragged batch of
// (queries, references) pairs: behind dispu_signed_distance_segments (include/dispu_hip.h, which states the operator;
// tests/reconstruct_oracle.py restates it).  reconstruct.hip's lattice takes its values here.  The reference has no counterpart.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass): once over the packed references, once over the packed queries
//   seed       as mls_project_kernel: one sweep of the reference segment's box table for the cell of the smallest (box-to-box bound,
//              cell number)
//   search     the text of knn_cells_search.h started at that cell: the exact k' = min(k, m_c) neighbours of the project's rule
//   sum        in the same kernel, from the list in registers, in double and in ascending rank: Wendland weights over the radius
//              support * sqrt(D), D the k'-th d2; f = sum w_j (x - p_j).n_j / sum w_j, or the nearest point's tangent plane where
//              every weight is zero
//
// No [q, k] tensor reaches memory.  Ordinary stores only, no atomics of its own, every loop bounded, ordering by kernel boundaries only,
// identical bytes from run to run.
#include "knn_cells.h"

namespace dispu {

// The bound is mls_project_kernel's, for its reason: the search alone fits 62 / 94 / 156 VGPRs at KMAX 8 / 16 / 32 and the time goes
// there; the epilogue's doubles (two sums, rho2, the query) may be parked in scratch once per query, after the search.
template <int KMAX>
__global__ __launch_bounds__(kNrmThreads, KMAX == 8 ? 8 : KMAX == 16 ? 5 : 3) void signed_distance_kernel(
    const int* __restrict__ qoff, const int* __restrict__ roff, const uint32_t* __restrict__ qsegb, const uint32_t* __restrict__ rsegb,
    const float4* __restrict__ qspt, const float4* __restrict__ rspt, const float* __restrict__ qtab, const float* __restrict__ rtab,
    const float* __restrict__ refs, const float* __restrict__ nrm, int k, double support2, float* __restrict__ out,
    int* __restrict__ status) {
#pragma clang fp contract(off)      // pinned here as well as by the build's -ffp-contract=off: the sum below rounds once per operation
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

    // D: the d2 of rank k' - 1 (best.thr is rank k - 1, still the empty key in a segment of fewer than k references)
    double Dk = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j == kp - 1) Dk = (double)__uint_as_float((uint32_t)(best.b[j] >> 32));
    const double rho2 = support2 * Dk;
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s0 = 0.0, s1 = 0.0, g0 = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const double r2 = (double)__uint_as_float((uint32_t)(best.b[j] >> 32)) / rho2;
            double w = 0.0;                                                     // D == 0: r2 is NaN and the weight stays 0
            if (r2 < 1.0) {
                const double r = sqrt(r2), a = 1.0 - r, a2 = a * a;
                w = (a2 * a2) * (4.0 * r + 1.0);
            }
            const size_t g = (rbase + (size_t)(uint32_t)best.b[j]) * 3;
            const double ux = cx - (double)refs[g + 0], uy = cy - (double)refs[g + 1], uz = cz - (double)refs[g + 2];
            const double gj = (ux * (double)nrm[g + 0] + uy * (double)nrm[g + 1]) + uz * (double)nrm[g + 2];
            if (j == 0) g0 = gj;
            s0 += w;
            s1 += w * gj;
        }
    out[qbase + (size_t)__float_as_int(q.w)] = (float)(s0 != 0.0 ? s1 / s0 : g0);
}

struct SdfScratch {
    size_t rbytes, qbytes, total;                                               // the two pre-passes
};

static SdfScratch sdf_scratch(int C, const int* qoff_host, const int* roff_host) {
    SdfScratch s{fps_cells_prepass_scratch(C, roff_host), fps_cells_prepass_scratch(C, qoff_host), 0};
    if (s.rbytes && s.qbytes) s.total = s.rbytes + s.qbytes;                    // the pre-pass sizes are multiples of 256
    return s;
}

static bool sdf_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_signed_distance_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    return sdf_scratch(C, qoff_host, roff_host).total;
}

DISPU_EXPORT int dispu_signed_distance_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                                                double support, const float* queries, const float* refs, const float* normals, float* out,
                                                int* status, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = cells_batch_check(C, qoff_host);
    if (rc == 0) rc = cells_batch_check(C, roff_host);
    if (rc != 0) return rc;
    if (k < 1 || k > 32 || !(support >= 1.0 && support <= 4.0)) return (int)hipErrorInvalidValue;
    if (!qoff || !roff || !queries || !refs || !normals || !out || !status) return (int)hipErrorInvalidValue;
    const size_t nq = (size_t)qoff_host[C], nr = (size_t)roff_host[C];
    const SdfScratch s = sdf_scratch(C, qoff_host, roff_host);
    if (!s.total || !scratch || scratch_bytes < s.total || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    const size_t obytes = nq * sizeof(float), rbytes = nr * 3 * sizeof(float);
    if (sdf_overlap(out, obytes, queries, nq * 3 * sizeof(float)) || sdf_overlap(out, obytes, refs, rbytes) ||
        sdf_overlap(out, obytes, normals, rbytes))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)scratch;
    const float4 *rspt, *qspt;
    const float *rtab, *qtab;
    const uint32_t *rsegb, *qsegb;
    int kr = 0, kqmax = 0;
    int rp = fps_cells_prepass(C, roff, roff_host, refs, base, s.rbytes, &rspt, &rtab, &rsegb, &kr, st);
    if (rp != 0) return rp;
    rp = fps_cells_prepass(C, qoff, qoff_host, queries, base + s.rbytes, s.qbytes, &qspt, &qtab, &qsegb, &kqmax, st);
    if (rp != 0) return rp;
    const double support2 = support * support;
    const dim3 grid((kqmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
    dispatch_kmax(k, [&](auto kmax_c) {
        hipLaunchKernelGGL((signed_distance_kernel<decltype(kmax_c)::value>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab,
                           rtab, refs, normals, k, support2, out, status);
    });
    return (int)hipGetLastError();
}
