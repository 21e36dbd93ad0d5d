// Moving-least-squares projection of the points of one cloud onto the surface another cloud describes, over a packed ragged batch: behind
// dispu_mls_project_segments (include/dispu_hip.h, which states the operator; tests/mls_oracle.py restates it).  Queries = references
// denoises a cloud; an upsampled cloud against its input snaps the output back onto the input's surface.  The reference has no counterpart.
//
//   search     the frame of every kernel that searches another cloud (attributes.hip describes it; knn_cross.h, knn_cross_prologue.h):
//              the exact k' = min(k, m_c) neighbours of the project's rule.  The pre-pass runs ONCE over the packed references, and
//              before EVERY iteration over the positions that iteration searches from: the skip proof of the walk (normals.hip) needs
//              lo_query <= q <= hi_query for the wave's box, so the query cells and their boxes must be those of the moved positions
//   fit        in the same kernel, from the list in registers, in double and in ascending rank: Wendland weights over the radius
//              support * sqrt(D), D the k'-th d2; the weighted centroid and covariance of u_j = p_j - x; the cyclic Jacobi of the
//              normals (jacobi3.h); the point moves along the eigenvector of the smallest eigenvalue onto the plane through the
//              centroid, or keeps its bits where the neighbourhood defines no plane
//
// The surface stays fixed: every iteration searches the references the call was given, so T iterations are T calls of one.  Positions
// pass from step to step through `out` and one buffer in the scratch, alternately, ending in `out`; a segment's non-finite flag passes
// through two status rows in the scratch, so a segment flagged once stays flagged.
//
// No [q, k] tensor reaches memory unless idx_out is asked for.  Ordinary stores only, no atomics of its own, every loop bounded,
// ordering by kernel boundaries only, identical bytes from run to run.
#include "jacobi3.h"
#include "knn_cross.h"

namespace dispu {

// The search alone fits 62 / 94 / 156 VGPRs at KMAX 8 / 16 / 32 (knn_cross_kernel: 8 / 5 / 3 waves per SIMD); the ten double moments
// beside the list would take 74 / 106 / 170 and a wave of occupancy from the search, where the time goes.  The bound keeps the
// search's occupancy: the compiler then parks 8 / 10 / 2 registers of the fit in scratch, once per query, after the search.
template <int KMAX>
__global__ __launch_bounds__(kNrmThreads, KMAX == 8 ? 8 : KMAX == 16 ? 5 : 3) void mls_project_kernel(
    const int* __restrict__ qoff, const int* __restrict__ roff, const uint32_t* __restrict__ qsegb, const uint32_t* __restrict__ rsegb,
    const float4* __restrict__ qspt, const float4* __restrict__ rspt, const float* __restrict__ qtab, const float* __restrict__ rtab,
    const float* __restrict__ refs, int k, double support2, float* __restrict__ out, int* __restrict__ idx_out,
    const int* __restrict__ status_in, int* __restrict__ status) {
#pragma clang fp contract(off)      // pinned here as well as by the build's -ffp-contract=off: the fit below rounds once per operation
#include "knn_cross_prologue.h"  // segment pair, query cell, query, seed, as text: defines c, lane, n, qbase, rbase, sp, gt, valid, q, s ...
#include "knn_cells_search.h"  // the ramp around s and the walk, as text: defines `kp` and `best`
    if (!valid) return;

    const size_t row = qbase + (size_t)__float_as_int(q.w);
    if (idx_out) {
        int* __restrict__ o = idx_out + row * (size_t)k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) o[j] = j < kp ? (int)best.index(j) : -1;
    }
    // D: the d2 of rank k' - 1 (best.thr is rank k - 1, still the empty key in a segment of fewer than k references)
    double Dk = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j == kp - 1) Dk = (double)best.d2(j);
    const double rho2 = support2 * Dk;
    // weighted moments of u_j = p_j - x in double (the differences of the converted coordinates are exact)
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s0 = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
    int live = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const double r2 = (double)best.d2(j) / rho2;
            double w = 0.0;
            if (!(r2 >= 1.0)) {
                const double r = sqrt(r2), a = 1.0 - r, a2 = a * a;
                w = (a2 * a2) * (4.0 * r + 1.0);
            }
            live += w != 0.0 ? 1 : 0;
            const size_t g = (rbase + (size_t)best.index(j)) * 3;
            const double x = (double)refs[g + 0] - cx, y = (double)refs[g + 1] - cy, z = (double)refs[g + 2] - cz;
            const double wx = w * x, wy = w * y, wz = w * z;
            s0 += w;
            s1x += wx; s1y += wy; s1z += wz;
            sxx += wx * x; syy += wy * y; szz += wz * z;
            sxy += wx * y; sxz += wx * z; syz += wy * z;
        }
    float ox = q.x, oy = q.y, oz = q.z;                                         // the stay rule: the input's bits
    if (kp >= 3 && live >= 3 && Dk != 0.0) {
        const double mx = s1x / s0, my = s1y / s0, mz = s1z / s0;
        double a00 = sxx / s0 - mx * mx, a11 = syy / s0 - my * my, a22 = szz / s0 - mz * mz;
        double a01 = sxy / s0 - mx * my, a02 = sxz / s0 - mx * mz, a12 = syz / s0 - my * mz;
#include "jacobi3_sweep.h"  // the sweeps, as text: the eigenvalues in a00, a11, a22; defines l0, ex, ey, ez
        const double l2 = fmax(a00, fmax(a11, a22));
        const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
        if (!(l2 <= 0.0) && !(l1 <= 1e-12 * l2)) {
            const double r = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
            ex *= r; ey *= r; ez *= r;
            const double t = (mx * ex + my * ey) + mz * ez;                     // the sign of the eigenvector cancels in t * e
            ox = (float)(cx + t * ex); oy = (float)(cy + t * ey); oz = (float)(cz + t * ez);
        }
    }
    out[row * 3 + 0] = ox; out[row * 3 + 1] = oy; out[row * 3 + 2] = oz;
}

// what the scratch holds behind the two pre-passes: one position buffer, two status rows (nothing for a refused batch)
struct MlsBehind {
    size_t pos, st;
    size_t bytes() const { return pos + 2 * st; }
};

static MlsBehind mls_behind(const CrossPrepass& p) {
    if (p.rc != 0) return {0, 0};
    return {align256((size_t)p.qoff_host[p.C] * 3 * sizeof(float)), align256((size_t)p.C * sizeof(int))};
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_mls_project_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    const CrossPrepass p(C, qoff_host, roff_host);
    return p.bytes() + mls_behind(p).bytes();
}

DISPU_EXPORT int dispu_mls_project_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                                            double support, int iterations, const float* queries, const float* refs, float* out,
                                            int* idx_out, int* status, void* scratch, size_t scratch_bytes, void* stream) {
    CrossPrepass p(C, qoff_host, roff_host);
    if (p.rc != 0) return p.rc;
    const MlsBehind s = mls_behind(p);
    if (k < 4 || k > 32 || !(support >= 1.0 && support <= 4.0) || iterations < 1 || iterations > 8) return (int)hipErrorInvalidValue;
    if (!qoff || !roff || !queries || !refs || !out || !status) return (int)hipErrorInvalidValue;
    const size_t nq = (size_t)qoff_host[C], obytes = nq * 3 * sizeof(float);
    if ((long long)nq * (long long)k >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (!p.fits(scratch, scratch_bytes, s.bytes())) return (int)hipErrorInvalidValue;
    if (ranges_overlap(out, obytes, queries, obytes) || ranges_overlap(out, obytes, refs, (size_t)roff_host[C] * 3 * sizeof(float)))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    char* behind = (char*)scratch + p.bytes();
    float* pong = (float*)behind;
    int* flag[2] = {(int*)(behind + s.pos), (int*)(behind + s.pos + s.st)};
    int rp = p.run_refs(roff, refs, scratch, st);
    if (rp != 0) return rp;
    const double support2 = support * support;
    const float* cur = queries;
    for (int it = 0; it < iterations; ++it) {
        // positions alternate between `out` and the scratch buffer so that the last step lands in `out`
        const bool last = it == iterations - 1;
        float* dst = ((iterations - 1 - it) & 1) ? pong : out;
        rp = p.run_queries(qoff, cur, scratch, st);
        if (rp != 0) return rp;
        const dim3 grid = p.grid(), block(kNrmThreads);
        const int* flag_in = it == 0 ? nullptr : flag[(it - 1) & 1];
        int* flag_out = last ? status : flag[it & 1];
        dispatch_kmax(k, [&](auto kmax_c) {
            hipLaunchKernelGGL((mls_project_kernel<decltype(kmax_c)::value>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt,
                               p.qtab, p.rtab, refs, k, support2, dst, last ? idx_out : (int*)nullptr, flag_in, flag_out);
        });
        rp = (int)hipGetLastError();
        if (rp != 0) return rp;
        cur = dst;
    }
    return 0;
}

