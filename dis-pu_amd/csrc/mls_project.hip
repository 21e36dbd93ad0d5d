// Moving-least-squares projection of the points of one cloud onto the surface another cloud describes, over a packed ragged batch: behind
// dispu_mls_project_segments (include/dispu_hip.h, which states the operator; tests/mls_oracle.py restates it).  Queries = references
// denoises a cloud; an upsampled cloud against its input snaps the output back onto the input's surface.  The reference has no counterpart.
//
//   pre-pass   morton_cells.hip (fps_cells_prepass): ONCE over the packed references, and before EVERY iteration over the positions that
//              iteration searches from.  The skip proof of the walk (normals.hip) needs lo_query <= q <= hi_query for the wave's box, so
//              the query cells and their boxes must be those of the moved positions, not of the positions the call started with
//   seed       as knn_cross_kernel (attributes.hip): one sweep of the reference segment's box table for the cell of the smallest
//              (box-to-box bound, cell number)
//   search     the text of knn_cells_search.h started at that cell: the exact k' = min(k, m_c) neighbours of the project's rule
//   fit        in the same kernel, from the list in registers, in double and in ascending rank: Wendland weights over the radius
//              support * sqrt(D), D the k'-th d2; the weighted centroid and covariance of u_j = p_j - x; normals.hip's cyclic Jacobi (same
//              rotation, same 12-sweep cap, same drop rule); the point moves along the eigenvector of the smallest eigenvalue onto the
//              plane through the centroid, or keeps its bits where the neighbourhood defines no plane
//
// The surface stays fixed: every iteration searches the references the call was given, so T iterations are T calls of one.  Positions
// pass from step to step through `out` and one buffer in the scratch, alternately, ending in `out`; a segment's non-finite flag passes
// through two status rows in the scratch, so a segment flagged once stays flagged.
//
// No [q, k] tensor reaches memory unless idx_out is asked for.  Ordinary stores only, no atomics of its own, every loop bounded,
// ordering by kernel boundaries only, identical bytes from run to run.
#include "knn_cells.h"

namespace dispu {

// normals.hip's nrm_rotate, restated: one Jacobi rotation that zeroes a_pq of a symmetric 3x3 matrix; r is the third index
__device__ __forceinline__ void mls_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
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
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qb0 = qoff[c], nq = qoff[c + 1] - qb0;
    const int rb0 = roff[c], n = roff[c + 1] - rb0;
    const size_t qbase = (size_t)qb0, rbase = (size_t)rb0;
    const uint32_t bad = qsegb[(size_t)c * 8 + 6] | rsegb[(size_t)c * 8 + 6] | (status_in ? (uint32_t)status_in[c] : 0u);
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
    if (idx_out) {
        int* __restrict__ o = idx_out + row * (size_t)k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) o[j] = j < kp ? (int)(uint32_t)best.b[j] : -1;
    }
    // D: the d2 of rank k' - 1 (best.thr is rank k - 1, still the empty key in a segment of fewer than k references)
    double Dk = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j == kp - 1) Dk = (double)__uint_as_float((uint32_t)(best.b[j] >> 32));
    const double rho2 = support2 * Dk;
    // weighted moments of u_j = p_j - x in double (the differences of the converted coordinates are exact)
    const double cx = (double)q.x, cy = (double)q.y, cz = (double)q.z;
    double s0 = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
    int live = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) {
            const double r2 = (double)__uint_as_float((uint32_t)(best.b[j] >> 32)) / rho2;
            double w = 0.0;
            if (!(r2 >= 1.0)) {
                const double r = sqrt(r2), a = 1.0 - r, a2 = a * a;
                w = (a2 * a2) * (4.0 * r + 1.0);
            }
            live += w != 0.0 ? 1 : 0;
            const size_t g = (rbase + (size_t)(uint32_t)best.b[j]) * 3;
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
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
        for (int sweep = 0; sweep < 12; ++sweep) {
            if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
            mls_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
            mls_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
            mls_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
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

struct MlsScratch {
    size_t rbytes, qbytes, pos, st, total;                                      // the two pre-passes, one position buffer, two status rows
};

static MlsScratch mls_scratch(int C, const int* qoff_host, const int* roff_host) {
    MlsScratch s{fps_cells_prepass_scratch(C, roff_host), fps_cells_prepass_scratch(C, qoff_host), 0, 0, 0};
    if (!s.rbytes || !s.qbytes) return s;
    s.pos = ((size_t)qoff_host[C] * 3 * sizeof(float) + 255) & ~(size_t)255;
    s.st = ((size_t)C * sizeof(int) + 255) & ~(size_t)255;
    s.total = s.rbytes + s.qbytes + s.pos + 2 * s.st;                           // the pre-pass sizes are multiples of 256
    return s;
}

static bool mls_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_mls_project_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    return mls_scratch(C, qoff_host, roff_host).total;
}

DISPU_EXPORT int dispu_mls_project_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                                            double support, int iterations, const float* queries, const float* refs, float* out,
                                            int* idx_out, int* status, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = cells_batch_check(C, qoff_host);
    if (rc == 0) rc = cells_batch_check(C, roff_host);
    if (rc != 0) return rc;
    if (k < 4 || k > 32 || !(support >= 1.0 && support <= 4.0) || iterations < 1 || iterations > 8) return (int)hipErrorInvalidValue;
    if (!qoff || !roff || !queries || !refs || !out || !status) return (int)hipErrorInvalidValue;
    const size_t nq = (size_t)qoff_host[C], nr = (size_t)roff_host[C];
    if ((long long)nq * (long long)k >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const MlsScratch s = mls_scratch(C, qoff_host, roff_host);
    if (!s.total || !scratch || scratch_bytes < s.total || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    const size_t obytes = nq * 3 * sizeof(float);
    if (mls_overlap(out, obytes, queries, obytes) || mls_overlap(out, obytes, refs, nr * 3 * sizeof(float))) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)scratch;
    float* pong = (float*)(base + s.rbytes + s.qbytes);
    int* flag[2] = {(int*)(base + s.rbytes + s.qbytes + s.pos), (int*)(base + s.rbytes + s.qbytes + s.pos + s.st)};
    const float4 *rspt, *qspt;
    const float *rtab, *qtab;
    const uint32_t *rsegb, *qsegb;
    int kr = 0, kqmax = 0;
    int rp = fps_cells_prepass(C, roff, roff_host, refs, base, s.rbytes, &rspt, &rtab, &rsegb, &kr, st);
    if (rp != 0) return rp;
    const double support2 = support * support;
    const float* cur = queries;
    for (int it = 0; it < iterations; ++it) {
        // positions alternate between `out` and the scratch buffer so that the last step lands in `out`
        const bool last = it == iterations - 1;
        float* dst = ((iterations - 1 - it) & 1) ? pong : out;
        rp = fps_cells_prepass(C, qoff, qoff_host, cur, base + s.rbytes, s.qbytes, &qspt, &qtab, &qsegb, &kqmax, st);
        if (rp != 0) return rp;
        const dim3 grid((kqmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
        const int* flag_in = it == 0 ? nullptr : flag[(it - 1) & 1];
        int* flag_out = last ? status : flag[it & 1];
        dispatch_kmax(k, [&](auto kmax_c) {
            hipLaunchKernelGGL((mls_project_kernel<decltype(kmax_c)::value>), grid, block, 0, st, qoff, roff, qsegb, rsegb, qspt, rspt, qtab,
                               rtab, refs, k, support2, dst, last ? idx_out : (int*)nullptr, flag_in, flag_out);
        });
        rp = (int)hipGetLastError();
        if (rp != 0) return rp;
        cur = dst;
    }
    return 0;
}
