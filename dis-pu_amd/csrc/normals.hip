// Unit normals of every point of a packed ragged batch of clouds from the PCA of its exact k nearest neighbours: behind
// dispu_pca_normals_segments (include/dispu_hip.h).  The reference has no counterpart (it reads and writes bare x y z); the neighbourhood
// is pc_util.py:83-92's k-NN made deterministic: the k' = min(k, n_c) points of the query's own segment with the smallest
// (d2, original local index), d2 = ((dx*dx + dy*dy) + dz*dz) in fp32 without contraction, the query itself and duplicates included --
// the rule of dispu_knn_patch_segments, so the two agree bit for bit.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass):: segment boxes and non-finite flags, Morton keys with the segment id on top,
//              one stable dispu_radix_sort_pairs, cells of 64 consecutive sorted positions with their boxes
//   search     (knn_cells.h; the text of knn_cells_prologue.h and knn_cells_search.h, which exists there once for every kernel that
//              searches) one wave per cell, one query per lane; every lane keeps its k best keys (d2 bits << 32 | local index) sorted in
//              registers.  The wave visits its start cell (here its own; knn_cross_prologue.h picks one by a sweep), then the cells at growing Morton offset (c - 1, c + 1, c - 2, ...) until it
//              has seen k' points (every lane sees every point of a visited cell, so all lanes then hold k' candidates), then walks
//              the segment's box table, 64 boxes per step (one per lane), and visits a cell only if its lower bound does not exceed
//              the wave's largest current k-th distance.  A visit is dense: 64 queries x 64 points.
//   normal     in the same kernel, from the neighbourhood in registers: q_j = p_j - p_i, mu = sum q_j / k', Cov = sum q_j q_j^T / k' -
//              mu mu^T, all in double; cyclic Jacobi in double (jacobi3.h); the eigenvector of the smallest eigenvalue, stored as fp32.
//
// Why a skip is sound (of the walk in knn_cells_search.h, the only copy of it): per axis e := max(fl(lo_cell - hi_query), fl(lo_query - hi_cell), 0).  For a point p of the cell and a query q of
// the wave, lo_cell <= p and q <= hi_query, and rounding is monotone, so fl(lo_cell - hi_query) <= fl(p - q); likewise fl(lo_query -
// hi_cell) <= fl(q - p) = -fl(p - q): e <= |fl(p - q)| holds IN floating point.  The bound lb = ((ex*ex + ey*ey) + ez*ez) is the same
// operations in the same order as d2, each of them (product of non-negatives, sum) monotone in its non-negative arguments, so lb <= d2
// bit for bit.  A cell is skipped only on lb > k-th STRICTLY, k-th the largest k-th distance over the wave's lanes: a point at exactly
// the k-th distance with a lower index must still displace.  A lane with fewer than k' candidates has k-th = +inf (the all-ones key).
// A cell that passes is tested once more per lane with the query point as its own box (lo_query = hi_query = q: the same argument)
// against the lane's own k-th distance, and visited if any lane passes: cells of 64 sorted points that straddle a jump of the Morton
// curve have large boxes, and the box-to-box bound alone sends them through most of their surroundings.
// d2 >= +0 and is never NaN for finite coordinates (an overflowing difference gives +inf), so its bits order like its value.
//
// No [n, k] tensor reaches memory unless idx_out is asked for.  Every value is written with ordinary stores; no atomics of its own;
// ordering between the pre-pass and the search by kernel boundaries only; identical bytes from run to run.
#include "jacobi3.h"
#include "knn_cells.h"

namespace dispu {

template <int KMAX>
__global__ __launch_bounds__(kNrmThreads) void pca_normals_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                                  const uint32_t* __restrict__ segb, const float4* __restrict__ spt,
                                                                  const float* __restrict__ tab, int k, int orient_mode,
                                                                  const float* __restrict__ orient, float* __restrict__ normal,
                                                                  float* __restrict__ variation, int* __restrict__ idx_out,
                                                                  int* __restrict__ status) {
#include "knn_cells_prologue.h"  // segment, cell, query, as text: defines c, lane, n, base, cb, sp, gt, valid, q, qlo4, qhi4 ...
    const int s = cb;                                                           // the search starts in the wave's own cell
#include "knn_cells_search.h"    // the search, as text: defines `kp` and `best`
    if (!valid) return;

    const int qi = __float_as_int(q.w);
    const size_t row = base + (size_t)qi;
    if (idx_out) {
        int* __restrict__ o = idx_out + row * (size_t)k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) o[j] = j < kp ? (int)best.index(j) : -1;
    }
    // moments of q_j = p_j - p_i in double (the differences of the converted coordinates are exact)
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const size_t g = (base + (size_t)best.index(j)) * 3;
            const double x = (double)xyz[g + 0] - cx, y = (double)xyz[g + 1] - cy, z = (double)xyz[g + 2] - cz;
            s1x += x; s1y += y; s1z += z;
            sxx += x * x; syy += y * y; szz += z * z;
            sxy += x * y; sxz += x * z; syz += y * z;
        }
    const double inv = 1.0 / (double)kp;
    const double mx = s1x * inv, my = s1y * inv, mz = s1z * inv;
    double a00 = sxx * inv - mx * mx, a11 = syy * inv - my * my, a22 = szz * inv - mz * mz;
    double a01 = sxy * inv - mx * my, a02 = sxz * inv - mx * mz, a12 = syz * inv - my * mz;
#include "jacobi3_sweep.h"  // the sweeps, as text: the eigenvalues in a00, a11, a22; defines l0, ex, ey, ez
    const double l2 = fmax(a00, fmax(a11, a22));
    const double sum = a00 + a11 + a22;
    float nx = 0.f, ny = 0.f, nz = 0.f, var = -1.0f;
    if (kp >= 3 && l2 > 0.0) {
        const double r = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
        ex *= r; ey *= r; ez *= r;
        nx = (float)ex; ny = (float)ey; nz = (float)ez;
        var = (float)(fmax(l0, 0.0) / sum);
        // mode 0: the component of largest magnitude is positive, ties to the lowest axis
        const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
        const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
        bool flip = lead < 0.f;
        if (orient_mode != 0) {
            double dx, dy, dz;
            if (orient_mode == 1) {
                dx = (double)orient[row * 3 + 0]; dy = (double)orient[row * 3 + 1]; dz = (double)orient[row * 3 + 2];
            } else {
                dx = (double)orient[(size_t)c * 3 + 0] - cx; dy = (double)orient[(size_t)c * 3 + 1] - cy;
                dz = (double)orient[(size_t)c * 3 + 2] - cz;
            }
            const double dot = (double)nx * dx + (double)ny * dy + (double)nz * dz;   // of the stored vector, before the sign
            if (dot < 0.0) flip = true;
            else if (dot > 0.0) flip = false;                                   // exactly 0 (or NaN): the mode-0 sign stays
        }
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    }
    normal[row * 3 + 0] = nx; normal[row * 3 + 1] = ny; normal[row * 3 + 2] = nz;
    if (variation) variation[row] = var;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_pca_normals_scratch_bytes(int C, const int* off_host, int k) {
    return k < 4 || k > 32 ? 0 : fps_cells_prepass_scratch(C, off_host);
}

DISPU_EXPORT int dispu_pca_normals_segments(int C, const int* off, const int* off_host, int k, const float* cloud, int orient_mode,
                                            const float* orient, float* normal, float* variation, int* idx_out, int* status,
                                            void* scratch, size_t scratch_bytes, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (k < 4 || k > 32 || orient_mode < 0 || orient_mode > 2 || (orient_mode != 0 && !orient) || !off || !cloud || !normal || !status)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const float4* spt;
    const float* tab;
    const uint32_t* segb;
    int kmax = 0;
    const int rp = fps_cells_prepass(C, off, off_host, cloud, scratch, scratch_bytes, &spt, &tab, &segb, &kmax, st);
    if (rp != 0) return rp;
    const dim3 grid((kmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
    dispatch_kmax(k, [&](auto kmax_c) {
        hipLaunchKernelGGL((pca_normals_kernel<decltype(kmax_c)::value>), grid, block, 0, st, cloud, off, segb, spt, tab, k, orient_mode, orient,
                           normal, variation, idx_out, status);
    });
    return (int)hipGetLastError();
}
