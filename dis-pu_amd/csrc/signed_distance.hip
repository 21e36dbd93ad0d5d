// The implicit function of an oriented cloud at arbitrary positions (an IMLS / Hoppe signed distance), over a packed ragged batch of
// (queries, references) pairs: behind dispu_signed_distance_segments (include/dispu_hip.h, which states the operator;
// tests/reconstruct_oracle.py restates it).  reconstruct.hip's lattice takes its values here.  The reference has no counterpart.
//
//   search     the frame of every kernel that searches another cloud (attributes.hip describes it; knn_cross.h, knn_cross_prologue.h):
//              a pre-pass over the packed references and one over the packed queries, the seed cell, then the text of
//              knn_cells_search.h started there: the exact k' = min(k, m_c) neighbours of the project's rule
//   sum        in the same kernel, from the list in registers, in double and in ascending rank: Wendland weights over the radius
//              support * sqrt(D), D the k'-th d2; f = sum w_j (x - p_j).n_j / sum w_j, or the nearest point's tangent plane where
//              every weight is zero
//
// No [q, k] tensor reaches memory.  Ordinary stores only, no atomics of its own, every loop bounded, ordering by kernel boundaries only,
// identical bytes from run to run.
#include "knn_cross.h"

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
    const int* const status_in = nullptr;                                       // no status carried in
#include "knn_cross_prologue.h"  // segment pair, query cell, query, seed, as text: defines c, lane, n, qbase, rbase, sp, gt, valid, q, s ...
#include "knn_cells_search.h"  // the ramp around s and the walk, as text: defines `kp` and `best`
    if (!valid) return;

    // D: the d2 of rank k' - 1 (best.thr is rank k - 1, still the empty key in a segment of fewer than k references)
    double Dk = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j == kp - 1) Dk = (double)best.d2(j);
    const double rho2 = support2 * Dk;
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s0 = 0.0, s1 = 0.0, g0 = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const double r2 = (double)best.d2(j) / rho2;
            double w = 0.0;                                                     // D == 0: r2 is NaN and the weight stays 0
            if (r2 < 1.0) {
                const double r = sqrt(r2), a = 1.0 - r, a2 = a * a;
                w = (a2 * a2) * (4.0 * r + 1.0);
            }
            const size_t g = (rbase + (size_t)best.index(j)) * 3;
            const double ux = cx - (double)refs[g + 0], uy = cy - (double)refs[g + 1], uz = cz - (double)refs[g + 2];
            const double gj = (ux * (double)nrm[g + 0] + uy * (double)nrm[g + 1]) + uz * (double)nrm[g + 2];
            if (j == 0) g0 = gj;
            s0 += w;
            s1 += w * gj;
        }
    out[qbase + (size_t)__float_as_int(q.w)] = (float)(s0 != 0.0 ? s1 / s0 : g0);
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_signed_distance_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    return CrossPrepass(C, qoff_host, roff_host).bytes();
}

DISPU_EXPORT int dispu_signed_distance_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                                                double support, const float* queries, const float* refs, const float* normals, float* out,
                                                int* status, void* scratch, size_t scratch_bytes, void* stream) {
    CrossPrepass p(C, qoff_host, roff_host);
    if (p.rc != 0) return p.rc;
    if (k < 1 || k > 32 || !(support >= 1.0 && support <= 4.0)) return (int)hipErrorInvalidValue;
    if (!qoff || !roff || !queries || !refs || !normals || !out || !status) return (int)hipErrorInvalidValue;
    if (!p.fits(scratch, scratch_bytes)) return (int)hipErrorInvalidValue;
    const size_t nq = (size_t)qoff_host[C], obytes = nq * sizeof(float), rbytes = (size_t)roff_host[C] * 3 * sizeof(float);
    if (ranges_overlap(out, obytes, queries, nq * 3 * sizeof(float)) || ranges_overlap(out, obytes, refs, rbytes) ||
        ranges_overlap(out, obytes, normals, rbytes))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    int rp = p.run_refs(roff, refs, scratch, st);
    if (rp == 0) rp = p.run_queries(qoff, queries, scratch, st);
    if (rp != 0) return rp;
    const double support2 = support * support;
    const dim3 grid = p.grid(), block(kNrmThreads);
    dispatch_kmax(k, [&](auto kmax_c) {
        hipLaunchKernelGGL((signed_distance_kernel<decltype(kmax_c)::value>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt,
                           p.qtab, p.rtab, refs, normals, k, support2, out, status);
    });
    return (int)hipGetLastError();
}
