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
//              registers.  The wave visits its start cell (here its own; attributes.hip picks one by a sweep), then the cells at growing Morton offset (c - 1, c + 1, c - 2, ...) until it
//              has seen k' points (every lane sees every point of a visited cell, so all lanes then hold k' candidates), then walks
//              the segment's box table, 64 boxes per step (one per lane), and visits a cell only if its lower bound does not exceed
//              the wave's largest current k-th distance.  A visit is dense: 64 queries x 64 points.
//   normal     in the same kernel, from the neighbourhood in registers: q_j = p_j - p_i, mu = sum q_j / k', Cov = sum q_j q_j^T / k' -
//              mu mu^T, all in double; cyclic Jacobi in double; the eigenvector of the smallest eigenvalue, stored as fp32.
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
#include "knn_cells.h"

namespace dispu {

// one Jacobi rotation that zeroes a_pq of a symmetric 3x3 matrix; r is the third index: arp, arq its other two off-diagonals
__device__ __forceinline__ void nrm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
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
            if (j < k) o[j] = j < kp ? (int)(uint32_t)best.b[j] : -1;
    }
    // moments of q_j = p_j - p_i in double (the differences of the converted coordinates are exact)
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const size_t g = (base + (size_t)(uint32_t)best.b[j]) * 3;
            const double x = (double)xyz[g + 0] - cx, y = (double)xyz[g + 1] - cy, z = (double)xyz[g + 2] - cz;
            s1x += x; s1y += y; s1z += z;
            sxx += x * x; syy += y * y; szz += z * z;
            sxy += x * y; sxz += x * z; syz += y * z;
        }
    const double inv = 1.0 / (double)kp;
    const double mx = s1x * inv, my = s1y * inv, mz = s1z * inv;
    double a00 = sxx * inv - mx * mx, a11 = syy * inv - my * my, a22 = szz * inv - mz * mz;
    double a01 = sxy * inv - mx * my, a02 = sxz * inv - mx * mz, a12 = syz * inv - my * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
    for (int sweep = 0; sweep < 12; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        nrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        nrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        nrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
        const double scale = fabs(a00) + fabs(a11) + fabs(a22);                 // off-diagonals that no longer change the diagonal
        if (fabs(a01) + scale == scale) a01 = 0.0;
        if (fabs(a02) + scale == scale) a02 = 0.0;
        if (fabs(a12) + scale == scale) a12 = 0.0;
    }
    // the column of the smallest eigenvalue (ties: the lowest column), and the three in order
    double l0 = a00, ex = v00, ey = v10, ez = v20;
    if (a11 < l0) { l0 = a11; ex = v01; ey = v11; ez = v21; }
    if (a22 < l0) { l0 = a22; ex = v02; ey = v12; ez = v22; }
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
