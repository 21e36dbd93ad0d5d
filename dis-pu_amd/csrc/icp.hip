// Rigid registration (ICP) of one cloud onto another over a packed ragged batch of pairs: behind dispu_icp_segments and
// dispu_rigid_apply_segments (include/dispu_hip.h, which states the operator and pins every operation order; tests/icp_oracle.py
// restates it).  The reference has no counterpart.
//
//   apply       rigid_apply_kernel: cur = fp32(T * source), always from the original source and the pair's current T
//   search      icp_accumulate_kernel, the fourth client of the frame of attributes.hip (knn_cross.h, knn_cross_prologue.h,
//               knn_cells_search.h): the target pre-pass ONCE, the source pre-pass before every step on cur, as mls_project.hip does
//               and for its reason.  Only rank 0 is wanted: the search text is instantiated at KMAX = 1, where it compiles unchanged
//   equations   in the same kernel, after the search, from the one key in registers: each of the 29 sums is formed, reduced over the
//               wave by the xor butterfly (o = 32 .. 1: every lane ends with the same bits) and stored by lane 0 before the next one
//               is formed, so no more than one accumulator is live beside p, d and n.  Lanes without a query stay in the butterfly
//               and add zeros.  One row of 32 doubles per source cell in the scratch; no [q] index or distance tensor reaches memory
//   solve       icp_solve_kernel, one workgroup per pair: thread (r, col) = (tid / 32, tid % 32) adds column col of the rows r, r + 32,
//               ... in ascending order (coalesced 256-byte rows), LDS, then ascending r; thread 0 factors and updates T in double
//
// T, the frozen flag and the update count of a pair live in the scratch between the launches; the user's outputs are written by the
// evaluation pass alone (aligned and corr by the accumulate kernel from the sorted query it holds, the rest by the solve kernel), so a
// pair with a non-finite coordinate has nothing written but its status word, which passes from step to step through two scratch rows.
//
// Ordinary stores only, no atomics of its own, every loop bounded, ordering by kernel boundaries only, identical bytes from run to run.
#include "knn_cross.h"

namespace dispu {

constexpr int kIcpRow = 32;                                                     // doubles per partial row: 21 A, 6 b, e, count, 3 unused
// 1024 threads for the sum over the cells: the workgroup is alone with its pair, and a thread's adds are a chain of dependent loads
// (6400 rows at 409 600 points: 198 us with 256 threads, traced)
constexpr int kIcpApply = 256, kIcpSolve = 1024, kIcpSolveRows = kIcpSolve / kIcpRow;

struct IcpState {
    int frozen, iters;                                                          // frozen: 0 running, 1 converged, 2 degenerate
};

__global__ __launch_bounds__(kIcpApply) void rigid_apply_kernel(const int* __restrict__ off, const float* points,
                                                                const double* __restrict__ transform, float* out) {
#pragma clang fp contract(off)
    const int c = blockIdx.y, b0 = off[c], n = off[c + 1] - b0;
    const int i = blockIdx.x * kIcpApply + threadIdx.x;
    if (i >= n) return;
    const double* __restrict__ T = transform + (size_t)c * 16;
    const size_t g = ((size_t)b0 + (size_t)i) * 3;
    const double x = (double)points[g + 0], y = (double)points[g + 1], z = (double)points[g + 2];
    const float ox = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    const float oy = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    const float oz = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
    out[g + 0] = ox; out[g + 1] = oy; out[g + 2] = oz;
}

__global__ __launch_bounds__(256) void icp_init_kernel(int C, const double* __restrict__ init, double* __restrict__ tcur,
                                                       IcpState* __restrict__ state) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    for (int j = 0; j < 16; ++j) tcur[(size_t)c * 16 + j] = init ? init[(size_t)c * 16 + j] : ((j % 5) == 0 ? 1.0 : 0.0);
    state[c] = IcpState{0, 0};
}

// the wave's sum of v by the pinned butterfly, the same bits in every lane
__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// 42 (point) / 44 (plane) VGPRs, no scratch (--save-temps): the search at KMAX = 1 and, after it, one sum at a time.  No occupancy bound
// is asked for: below 64 registers the kernel already runs the 8 waves per SIMD the hardware holds.
template <int KMAX, int MODE>
__global__ __launch_bounds__(kNrmThreads) void icp_accumulate_kernel(
    const int* __restrict__ qoff, const int* __restrict__ roff, const uint32_t* __restrict__ qsegb, const uint32_t* __restrict__ rsegb,
    const float4* __restrict__ qspt, const float4* __restrict__ rspt, const float* __restrict__ qtab, const float* __restrict__ rtab,
    const float* __restrict__ refs, const float* __restrict__ normals, float max_d2, int evaluate, const IcpState* __restrict__ state,
    double* __restrict__ partial, float* __restrict__ aligned, int* __restrict__ corr, const int* __restrict__ status_in,
    int* __restrict__ status) {
#pragma clang fp contract(off)      // pinned here as well as by the build's -ffp-contract=off: the sums below round once per operation
    const int k = 1;
#include "knn_cross_prologue.h"  // segment pair, query cell, query, seed, as text: defines c, lane, n, qbase, rbase, sp, gt, valid, q, s ...
    if (!evaluate && state[c].frozen != 0) return;                              // a frozen pair: block-uniform
#include "knn_cells_search.h"  // the ramp around s and the walk, as text: defines `kp` and `best`
    // no return on !valid: every lane stays in the butterflies below and an idle one adds zeros

    const uint32_t j0 = best.index(0);
    const float d2 = best.d2(0);
    const bool in = valid && d2 <= max_d2;
    if (evaluate && valid) {
        const size_t row = qbase + (size_t)__float_as_int(q.w);
        aligned[row * 3 + 0] = q.x; aligned[row * 3 + 1] = q.y; aligned[row * 3 + 2] = q.z;
        if (corr) corr[row] = in ? (int)j0 : -1;
    }
    const size_t g0 = rbase * 3, g = (rbase + (size_t)j0) * 3;
    const double ox = (double)refs[g0 + 0], oy = (double)refs[g0 + 1], oz = (double)refs[g0 + 2];
    const double px = (double)q.x - ox, py = (double)q.y - oy, pz = (double)q.z - oz;
    const double dx = px - ((double)refs[g + 0] - ox), dy = py - ((double)refs[g + 1] - oy), dz = pz - ((double)refs[g + 2] - oz);
    double* __restrict__ prow = partial + (fpc_cell_base(qbase, c) + (size_t)cb) * kIcpRow;
    int slot = 0;
    auto emit = [&](double v) {                                                 // one sum: formed, reduced, stored
        const double t = icp_wave_sum(in ? v : 0.0);
        if (lane == 0) prow[slot] = t;
        ++slot;
    };
    const double cnt = icp_wave_sum(in ? 1.0 : 0.0);
    auto put = [&](double t) {                                                  // a sum whose terms are all 0 or all 1: the bits the butterfly gives
        if (lane == 0) prow[slot] = t;
        ++slot;
    };
    if constexpr (MODE == 0) {
        emit(py * py + pz * pz); emit(-(px * py)); emit(-(px * pz)); put(0.0); emit(-pz); emit(py);
        emit(px * px + pz * pz); emit(-(py * pz)); emit(pz); put(0.0); emit(-px);
        emit(px * px + py * py); emit(-py); emit(px); put(0.0);
        put(cnt); put(0.0); put(0.0);
        put(cnt); put(0.0);
        put(cnt);
        emit(py * dz - pz * dy); emit(pz * dx - px * dz); emit(px * dy - py * dx); emit(dx); emit(dy); emit(dz);
        emit((dx * dx + dy * dy) + dz * dz);
    } else {
        const double nx = (double)normals[g + 0], ny = (double)normals[g + 1], nz = (double)normals[g + 2];
        const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
        const double r = (dx * nx + dy * ny) + dz * nz;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) emit(J[i] * J[j]);
#pragma unroll
        for (int i = 0; i < 6; ++i) emit(J[i] * r);
        emit(r * r);
    }
    put(cnt);
}

// One workgroup per pair: the sums over the pair's cells, then on thread 0 either the update of T (evaluate 0) or the outputs of the
// returned T (evaluate 1).  `status` is the row the accumulate kernel of this step wrote.
__global__ __launch_bounds__(kIcpSolve) void icp_solve_kernel(const int* __restrict__ qoff, const int* __restrict__ roff,
                                                              const uint32_t* __restrict__ rsegb, const float* __restrict__ refs,
                                                              const double* __restrict__ partial, int mode, double tolerance, int evaluate,
                                                              double* __restrict__ tcur, IcpState* __restrict__ state,
                                                              const int* __restrict__ status, double* __restrict__ transform,
                                                              int* __restrict__ inliers, double* __restrict__ rmse, int* __restrict__ iters,
                                                              int* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ double red[kIcpSolveRows][kIcpRow];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (status[c] != 0) return;                                                 // nothing is written for a non-finite pair
    if (!evaluate && state[c].frozen != 0) return;
    const int qb0 = qoff[c], nq = qoff[c + 1] - qb0;
    const int KQ = (nq + kNrmCell - 1) / kNrmCell;
    const double* __restrict__ rows = partial + fpc_cell_base((size_t)qb0, c) * kIcpRow;
    const int col = tid & (kIcpRow - 1), r0 = tid / kIcpRow;
    double acc = 0.0;
    if (col < 29)
        for (int j = r0; j < KQ; j += kIcpSolveRows) acc += rows[(size_t)j * kIcpRow + col];
    red[r0][col] = acc;
    __syncthreads();
    if (tid != 0) return;
    double S[29];
#pragma unroll
    for (int i = 0; i < 29; ++i) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < kIcpSolveRows; ++r) t += red[r][i];
        S[i] = t;
    }
    const double cnt = S[28], e = S[27];
    double* __restrict__ T = tcur + (size_t)c * 16;
    if (evaluate) {
#pragma unroll
        for (int i = 0; i < 16; ++i) transform[(size_t)c * 16 + i] = T[i];
        inliers[c] = (int)cnt;
        rmse[c] = cnt > 0.0 ? sqrt(e / cnt) : 0.0;
        iters[c] = state[c].iters;
        flag[c] = state[c].frozen;
        return;
    }
    // Cholesky of A (upper entries row by row in S[0 .. 20]), L kept full; ok falls on any rule of the degenerate pair
    double A[6][6], L[6][6], b[6];
    {
        int s = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { A[i][j] = S[s]; A[j][i] = S[s]; ++s; }
#pragma unroll
        for (int i = 0; i < 6; ++i) b[i] = S[21 + i];
    }
    bool ok = cnt >= (mode ? 6.0 : 3.0);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int l = 0; l < j; ++l) d -= L[j][l] * L[j][l];
        if (!(d > 1e-12 * A[j][j]) || !(fabs(d) <= 1.7976931348623157e308)) ok = false;
        const double piv = sqrt(d);
        L[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int l = 0; l < j; ++l) v -= L[i][l] * L[j][l];
            L[i][j] = v / piv;
        }
    }
    double z[6], x[6];                                                          // L z = -b, then L^T x = z
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -b[i];
#pragma unroll
        for (int l = 0; l < i; ++l) v -= L[i][l] * z[l];
        z[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int l = i + 1; l < 6; ++l) v -= L[l][i] * x[l];
        x[i] = v / L[i][i];
    }
    const double wx = x[0], wy = x[1], wz = x[2], tx = x[3], ty = x[4], tz = x[5];
    const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
    double a, cc;
    if (th < 1e-12) {
        a = 1.0 - th2 / 6.0;
        cc = 0.5 - th2 / 24.0;
    } else {
        a = sin(th) / th;
        cc = (1.0 - cos(th)) / th2;
    }
    // R = I + a [w]x + cc [w]x^2, [w]x^2 = w w^T - th2 I
    double R[3][3];
    R[0][0] = 1.0 + cc * (wx * wx - th2); R[0][1] = cc * (wx * wy) - a * wz;    R[0][2] = cc * (wx * wz) + a * wy;
    R[1][0] = cc * (wx * wy) + a * wz;    R[1][1] = 1.0 + cc * (wy * wy - th2); R[1][2] = cc * (wy * wz) - a * wx;
    R[2][0] = cc * (wx * wz) - a * wy;    R[2][1] = cc * (wy * wz) + a * wx;    R[2][2] = 1.0 + cc * (wz * wz - th2);
    const size_t g0 = (size_t)roff[c] * 3;
    const double o[3] = {(double)refs[g0 + 0], (double)refs[g0 + 1], (double)refs[g0 + 2]};
    const double t3[3] = {tx, ty, tz};
    double Tn[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Tn[i * 4 + j] = (R[i][0] * T[0 * 4 + j] + R[i][1] * T[1 * 4 + j]) + R[i][2] * T[2 * 4 + j];
        const double u0 = T[3] - o[0], u1 = T[7] - o[1], u2 = T[11] - o[2];
        Tn[i * 4 + 3] = (((R[i][0] * u0 + R[i][1] * u1) + R[i][2] * u2) + o[i]) + t3[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i)
        if (!(fabs(Tn[i]) <= 1.7976931348623157e308)) ok = false;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!(fabs(x[i]) <= 1.7976931348623157e308)) ok = false;
    if (!ok) {
        state[c].frozen = 2;
        return;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = Tn[i];
    const uint32_t* __restrict__ sb = rsegb + (size_t)c * 8;
    const double ex = (double)ordered_to_f32(sb[3]) - (double)ordered_to_f32(~sb[0]);
    const double ey = (double)ordered_to_f32(sb[4]) - (double)ordered_to_f32(~sb[1]);
    const double ez = (double)ordered_to_f32(sb[5]) - (double)ordered_to_f32(~sb[2]);
    const double D = sqrt((ex * ex + ey * ey) + ez * ez);
    const double tn = sqrt((tx * tx + ty * ty) + tz * tz);
    IcpState st = state[c];
    st.iters += 1;
    if (tolerance > 0.0 && th <= tolerance && tn <= tolerance * D) st.frozen = 1;
    state[c] = st;
}

// what the scratch holds behind the two pre-passes (nothing for a refused batch)
struct IcpBehind {
    size_t cur, st, tcur, state, partial;
    size_t bytes() const { return cur + 2 * st + tcur + state + partial; }
};

static IcpBehind icp_behind(const CrossPrepass& p) {
    if (p.rc != 0) return {0, 0, 0, 0, 0};
    const size_t nq = (size_t)p.qoff_host[p.C], C = (size_t)p.C;
    return {align256(nq * 3 * sizeof(float)), align256(C * sizeof(int)), align256(C * 16 * sizeof(double)), align256(C * sizeof(IcpState)),
            align256((nq / kNrmCell + C) * kIcpRow * sizeof(double))};
}

static int icp_apply(int C, int nmax, const int* off, const float* points, const double* transform, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rigid_apply_kernel, dim3((nmax + kIcpApply - 1) / kIcpApply, C), dim3(kIcpApply), 0, st, off, points, transform, out);
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_icp_scratch_bytes(int C, const int* qoff_host, const int* roff_host) {
    const CrossPrepass p(C, qoff_host, roff_host);
    return p.bytes() + icp_behind(p).bytes();
}

DISPU_EXPORT int dispu_rigid_apply_segments(int C, const int* off, const int* off_host, const float* points, const double* transform,
                                            float* out, void* stream) {
    int nmax = 0;
    const int rc = cells_batch_check(C, off_host, &nmax);
    if (rc != 0) return rc;
    if (!off || !points || !transform || !out) return (int)hipErrorInvalidValue;
    return icp_apply(C, nmax, off, points, transform, out, (hipStream_t)stream);
}

DISPU_EXPORT int dispu_icp_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int mode,
                                    int iterations, float max_d2, double tolerance, const float* source, const float* target,
                                    const float* target_normals, const double* init, double* transform, float* aligned, int* corr,
                                    int* inliers, double* rmse, int* iters, int* flag, int* status, void* scratch, size_t scratch_bytes,
                                    void* stream) {
    CrossPrepass p(C, qoff_host, roff_host);
    if (p.rc != 0) return p.rc;
    const IcpBehind s = icp_behind(p);
    if (mode < 0 || mode > 1 || iterations < 0 || iterations > 128 || !(max_d2 >= 0.f) ||
        !(tolerance >= 0.0 && tolerance <= 1.7976931348623157e308))
        return (int)hipErrorInvalidValue;
    if (!qoff || !roff || !source || !target || (mode == 1 && !target_normals) || !transform || !aligned || !inliers || !rmse || !iters ||
        !flag || !status)
        return (int)hipErrorInvalidValue;
    if (!p.fits(scratch, scratch_bytes, s.bytes())) return (int)hipErrorInvalidValue;
    const size_t nq = (size_t)qoff_host[C], obytes = nq * 3 * sizeof(float);
    if (ranges_overlap(aligned, obytes, source, obytes) || ranges_overlap(aligned, obytes, target, (size_t)roff_host[C] * 3 * sizeof(float)))
        return (int)hipErrorInvalidValue;
    int qmax = 0;
    (void)cells_batch_check(C, qoff_host, &qmax);
    hipStream_t st = (hipStream_t)stream;
    char* behind = (char*)scratch + p.bytes();
    float* cur = (float*)behind;
    int* row[2] = {(int*)(behind + s.cur), (int*)(behind + s.cur + s.st)};
    double* tcur = (double*)(behind + s.cur + 2 * s.st);
    IcpState* state = (IcpState*)(behind + s.cur + 2 * s.st + s.tcur);
    double* partial = (double*)(behind + s.cur + 2 * s.st + s.tcur + s.state);

    int rp = p.run_refs(roff, target, scratch, st);
    if (rp != 0) return rp;
    hipLaunchKernelGGL(icp_init_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, init, tcur, state);
    rp = (int)hipGetLastError();
    if (rp != 0) return rp;
    for (int it = 0; it <= iterations; ++it) {                                  // the last round is the evaluation of the returned T
        const int evaluate = it == iterations ? 1 : 0;
        rp = icp_apply(C, qmax, qoff, source, tcur, cur, st);
        if (rp == 0) rp = p.run_queries(qoff, cur, scratch, st);
        if (rp != 0) return rp;
        const int* flag_in = it == 0 ? nullptr : row[(it - 1) & 1];
        int* flag_out = evaluate ? status : row[it & 1];
        const dim3 grid = p.grid(), block(kNrmThreads);
        if (mode == 0)
            hipLaunchKernelGGL((icp_accumulate_kernel<1, 0>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt, p.qtab, p.rtab,
                               target, target_normals, max_d2, evaluate, state, partial, aligned, corr, flag_in, flag_out);
        else
            hipLaunchKernelGGL((icp_accumulate_kernel<1, 1>), grid, block, 0, st, qoff, roff, p.qsegb, p.rsegb, p.qspt, p.rspt, p.qtab, p.rtab,
                               target, target_normals, max_d2, evaluate, state, partial, aligned, corr, flag_in, flag_out);
        rp = (int)hipGetLastError();
        if (rp != 0) return rp;
        hipLaunchKernelGGL(icp_solve_kernel, dim3(C), dim3(kIcpSolve), 0, st, qoff, roff, p.rsegb, target, partial, mode, tolerance, evaluate,
                           tcur, state, flag_out, transform, inliers, rmse, iters, flag);
        rp = (int)hipGetLastError();
        if (rp != 0) return rp;
    }
    return 0;
}
