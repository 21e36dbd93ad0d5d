// Point-to-surface distance and disk uniformity for the evaluator (gfx950).
// Replaces the CGAL tool evaluation_code/evaluation.cpp of the reference (AABB-tree `locate` + `squared_distance`, :202-214;
// the per-seed disk membership loop, :68-115) and the sklearn post-processing of evaluate.py:53-101 (analyze_uniform).
//
// Point -> mesh: one wave per point, one lane per face.  The faces arrive in Morton-ordered tiles of 64 (dis-pu_amd/mesh.py builds
// them once per mesh) with an fp32 AABB per tile.  The fp32 search keeps a per-lane key (ordered d2 bits << 32 | original face id),
// so the wave minimum is "smallest d2, then lowest face id" whatever order the tiles were visited in.  The pruned path visits the
// tile whose box is nearest first, then every tile whose conservative lower bound is not strictly above the wave's current best:
// a skipped face's fp32 d2 is strictly above a d2 already seen, so it could neither win nor tie, and the pruned and brute-force
// answers are bit-identical.  The winner's closest point and distance are recomputed once in fp64.
//
// Disks: membership is d2 <= fl32(r*r) with d2 in the DISPU_ARITH_PLAIN order (index-exact against an fp32 restatement); the
// member lists are CSR rows in seed-major order (i*R + j), members ascending, built by count -> in-place scan -> fill.
// Uniformity: one workgroup per disk, the nearest OTHER member by a tiled all-pairs scan through LDS (any disk size), fp64 terms
// reduced in a fixed order, then one wave per radius sums the kept disks in ascending seed order.
#include "common.h"
#include "internal.h"

namespace dispu {

constexpr int P2M_TILE = 64;        // faces per tile == lanes per wave
static_assert(P2M_TILE == DISPU_MESH_TILE, "the tile the public header documents");
constexpr int P2M_WAVES = 4;

// Closest point on triangle (a, b, c) to p by Voronoi regions (vertex, edge, face; C. Ericson, Real-Time Collision Detection,
// 5.1.5), with every division guarded: a triangle whose face-region denominator is not positive (zero or negative area in this
// precision) is treated as its three edges.
template <typename T>
__device__ __forceinline__ void seg_closest(T px, T py, T pz, T ax, T ay, T az, T bx, T by, T bz, T& qx, T& qy, T& qz) {
    const T ex = bx - ax, ey = by - ay, ez = bz - az;
    const T ee = ex * ex + ey * ey + ez * ez;
    T t = ee > T(0) ? ((px - ax) * ex + (py - ay) * ey + (pz - az) * ez) / ee : T(0);
    t = t < T(0) ? T(0) : (t > T(1) ? T(1) : t);
    qx = ax + t * ex; qy = ay + t * ey; qz = az + t * ez;
}

template <typename T>
__device__ __forceinline__ T sq3(T x, T y, T z) { return (x * x + y * y) + z * z; }

template <typename T>
__device__ void tri_closest(T px, T py, T pz, T ax, T ay, T az, T bx, T by, T bz, T cx, T cy, T cz, T& qx, T& qy, T& qz) {
    const T abx = bx - ax, aby = by - ay, abz = bz - az;
    const T acx = cx - ax, acy = cy - ay, acz = cz - az;
    const T apx = px - ax, apy = py - ay, apz = pz - az;
    const T d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    if (d1 <= T(0) && d2 <= T(0)) { qx = ax; qy = ay; qz = az; return; }
    const T bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const T d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    if (d3 >= T(0) && d4 <= d3) { qx = bx; qy = by; qz = bz; return; }
    // The face-region weights as triple products with the normal, (ab x ac) . (ap x bp) and its two companions: by Lagrange's identity
    // the d1 d4 - d3 d2 of the book, whose two products of about |ab| |ac| |ap| |bp| cancel down to |ab x ac| |ap x bp| and, in
    // fp32, left nothing but rounding for a sliver (length 1, width 1e-4: the point 0.007 off its own face; found by
    // tests/test_mesh_eval_ops_gpu.py::test_point_to_mesh[rungs]).  Here each cross product is rounded at its own size.
    const T nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const T vc = nx * (apy * bpz - apz * bpy) + ny * (apz * bpx - apx * bpz) + nz * (apx * bpy - apy * bpx);
    if (vc <= T(0) && d1 >= T(0) && d3 <= T(0) && d1 - d3 > T(0)) {
        const T v = d1 / (d1 - d3);
        qx = ax + v * abx; qy = ay + v * aby; qz = az + v * abz; return;
    }
    const T cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const T d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    if (d6 >= T(0) && d5 <= d6) { qx = cx; qy = cy; qz = cz; return; }
    const T vb = nx * (cpy * apz - cpz * apy) + ny * (cpz * apx - cpx * apz) + nz * (cpx * apy - cpy * apx);
    if (vb <= T(0) && d2 >= T(0) && d6 <= T(0) && d2 - d6 > T(0)) {
        const T w = d2 / (d2 - d6);
        qx = ax + w * acx; qy = ay + w * acy; qz = az + w * acz; return;
    }
    const T va = nx * (bpy * cpz - bpz * cpy) + ny * (bpz * cpx - bpx * cpz) + nz * (bpx * cpy - bpy * cpx);
    if (va <= T(0) && (d4 - d3) >= T(0) && (d5 - d6) >= T(0) && (d4 - d3) + (d5 - d6) > T(0)) {
        const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        qx = bx + w * (cx - bx); qy = by + w * (cy - by); qz = bz + w * (cz - bz); return;
    }
    const T den = va + vb + vc;
    if (den > T(0)) {
        const T v = vb / den, w = vc / den;
        qx = ax + abx * v + acx * w; qy = ay + aby * v + acy * w; qz = az + abz * v + acz * w; return;
    }
    // degenerate: the nearest of the three edges (ties -> the first)
    T x0, y0, z0, x1, y1, z1;
    seg_closest(px, py, pz, ax, ay, az, bx, by, bz, qx, qy, qz);
    T best = sq3(px - qx, py - qy, pz - qz);
    seg_closest(px, py, pz, bx, by, bz, cx, cy, cz, x0, y0, z0);
    const T e1 = sq3(px - x0, py - y0, pz - z0);
    if (e1 < best) { best = e1; qx = x0; qy = y0; qz = z0; }
    seg_closest(px, py, pz, cx, cy, cz, ax, ay, az, x1, y1, z1);
    if (sq3(px - x1, py - y1, pz - z1) < best) { qx = x1; qy = y1; qz = z1; }
}

// Conservative lower bound of the fp32 d2 that tri_closest<float> + sq3 can produce for any triangle inside the box:
// (distance to the box - slack)^2, rounded down.  The slack (2^-14 of the coordinate magnitudes involved) is far above the
// rounding error of the closest point and of d2 (a few ulp of those magnitudes), so no face of a skipped tile could have won.
__device__ __forceinline__ float box_lower_bound(float px, float py, float pz, float pmag, const float4* __restrict__ box, int t) {
    const float4 lo = box[2 * t], hi = box[2 * t + 1];
    const float dx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    const float bmag = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y))), fmaxf(fabsf(lo.z), fabsf(hi.z)));
    const float d = sqrtf(sq3(dx, dy, dz)) - 6.103515625e-05f * (pmag + bmag);
    return d > 0.f ? d * d * 0.99999f : 0.f;
}

__device__ __forceinline__ int lane_of_min(uint64_t mine, uint64_t wmin) {
    return (int)__builtin_ctzll(__ballot(mine == wmin));
}

template <bool BRUTE>
__global__ __launch_bounds__(64 * P2M_WAVES) void point_to_mesh_kernel(int n, const float* __restrict__ points, int F,
                                                                         const float4* __restrict__ tris, const int* __restrict__ face_ids,
                                                                         const float4* __restrict__ box, float* __restrict__ dist,
                                                                         float* __restrict__ proj, int* __restrict__ face) {
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * P2M_WAVES + (threadIdx.x >> 6);
    if (pi >= n) return;    // wave-uniform
    const float px = points[pi * 3 + 0], py = points[pi * 3 + 1], pz = points[pi * 3 + 2];
    const int T = (F + P2M_TILE - 1) / P2M_TILE;
    uint64_t best = ~0ull;  // this lane's (ordered d2, face id)
    int best_e = 0;         // its entry in the tile order
    auto visit = [&](int t) {
        const int e = t * P2M_TILE + lane;
        if (e < F) {
            const float4 a = tris[3 * e], b = tris[3 * e + 1], c = tris[3 * e + 2];
            float qx, qy, qz;
            tri_closest<float>(px, py, pz, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, qx, qy, qz);
            const float d2 = sq3(px - qx, py - qy, pz - qz);
            const uint64_t key = ((uint64_t)f32_to_ordered(d2) << 32) | (uint32_t)face_ids[e];
            if (key < best) { best = key; best_e = e; }
        }
    };
    if (BRUTE) {
        for (int t = 0; t < T; ++t) visit(t);
    } else {
        const float pmag = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
        uint64_t near = ~0ull;
        for (int t = lane; t < T; t += 64)
            near = u64_min(near, ((uint64_t)f32_to_ordered(box_lower_bound(px, py, pz, pmag, box, t)) << 32) | (uint32_t)t);
        const int t0 = (int)(uint32_t)wave_min_u64(near);
        visit(t0);
        float wbest = ordered_to_f32((uint32_t)(wave_min_u64(best) >> 32));
        for (int c0 = 0; c0 < T; c0 += 64) {
            const int t = c0 + lane;
            const bool want = t < T && t != t0 && !(box_lower_bound(px, py, pz, pmag, box, min(t, T - 1)) > wbest);
            uint64_t m = __ballot(want);
            while (m) {
                const int tt = c0 + (int)__builtin_ctzll(m);
                m &= m - 1;
                visit(tt);
                wbest = ordered_to_f32((uint32_t)(wave_min_u64(best) >> 32));
            }
        }
    }
    const uint64_t w = wave_min_u64(best);
    const int owner = lane_of_min(best, w);
    const int e = __shfl(best_e, owner, 64);
    if (lane == 0) {
        // the winner again in fp64 (once per point)
        const float4 a = tris[3 * e], b = tris[3 * e + 1], c = tris[3 * e + 2];
        const double dx = px, dy = py, dz = pz;
        double qx, qy, qz;
        tri_closest<double>(dx, dy, dz, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, qx, qy, qz);
        dist[pi] = (float)sqrt(sq3(dx - qx, dy - qy, dz - qz));
        proj[pi * 3 + 0] = (float)qx;
        proj[pi * 3 + 1] = (float)qy;
        proj[pi * 3 + 2] = (float)qz;
        face[pi] = (int)(uint32_t)w;
    }
}

// ---- disks -----------------------------------------------------------------------------------------------------------------
constexpr int DISK_WAVES = 4;

__device__ __forceinline__ float disk_d2(const float* __restrict__ s, const float* __restrict__ p, int q) {
    return sq3(p[q * 3 + 0] - s[0], p[q * 3 + 1] - s[1], p[q * 3 + 2] - s[2]);
}

// offsets[1 + i*R + j] = |{q : d2(seed i, point q) <= fl32(r_j * r_j)}|
__global__ __launch_bounds__(64 * DISK_WAVES) void disk_count_kernel(int S, int n, int R, const float* __restrict__ seeds,
                                                                      const float* __restrict__ points, const float* __restrict__ radii,
                                                                      long long* __restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DISK_WAVES + (threadIdx.x >> 6);
    if (i >= S) return;
    const float* s = seeds + i * 3;
    for (int j = 0; j < R; ++j) {
        const float r2 = radii[j] * radii[j];
        long long cnt = 0;
        for (int q0 = 0; q0 < n; q0 += 64) {
            const int q = q0 + lane;
            cnt += __popcll(__ballot(q < n && disk_d2(s, points, q) <= r2));
        }
        if (lane == 0) offsets[1 + (long long)i * R + j] = cnt;
    }
}

// in place: offsets[1..M] counts -> inclusive sums; offsets[0] = 0.  One workgroup, ascending segments.
constexpr int SCAN_BS = 1024;
__global__ __launch_bounds__(SCAN_BS) void disk_scan_kernel(long long M, long long* __restrict__ offsets) {
    __shared__ long long part[SCAN_BS];
    const long long per = (M + SCAN_BS - 1) / SCAN_BS;
    const long long b = 1 + threadIdx.x * per, e = min(b + per, M + 1);
    long long s = 0;
    for (long long k = b; k < e; ++k) s += offsets[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_BS; o <<= 1) {
        const long long v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (long long k = b; k < e; ++k) { run += offsets[k]; offsets[k] = run; }
    if (threadIdx.x == 0) offsets[0] = 0;
}

__global__ __launch_bounds__(64 * DISK_WAVES) void disk_fill_kernel(int S, int n, int R, const float* __restrict__ seeds,
                                                                     const float* __restrict__ points, const float* __restrict__ radii,
                                                                     const long long* __restrict__ offsets, int* __restrict__ members) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DISK_WAVES + (threadIdx.x >> 6);
    if (i >= S) return;
    const float* s = seeds + i * 3;
    for (int j = 0; j < R; ++j) {
        const float r2 = radii[j] * radii[j];
        const long long k = (long long)i * R + j, end = offsets[k + 1];
        long long pos = offsets[k];
        for (int q0 = 0; q0 < n && pos < end; q0 += 64) {
            const int q = q0 + lane;
            const bool in = q < n && disk_d2(s, points, q) <= r2;
            const uint64_t m = __ballot(in);
            const long long at = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (in && at < end) members[at] = q;
            pos += __popcll(m);
        }
    }
}

// One workgroup per disk k = i*R + j.  Disk term = coverage * mean_a((nn_a - expect_d)^2 / expect_d), nn_a = min over the OTHER
// members of |p_a - p_b| (fp32 d2, sqrt in fp64).  Skipped disks (count < 5) leave kept[k] = 0.
constexpr int UNI_BS = 256;
constexpr int UNI_TILE = 1024;
__global__ __launch_bounds__(UNI_BS) void disk_uniformity_kernel(int R, int n, const float* __restrict__ points,
                                                                  const long long* __restrict__ offsets, const int* __restrict__ members,
                                                                  const double* __restrict__ radii, const double* __restrict__ pct, int N,
                                                                  double* __restrict__ term, int* __restrict__ kept) {
    __shared__ float4 tile[UNI_TILE];
    __shared__ double red[UNI_BS];
    const long long k = blockIdx.x;
    const int j = (int)(k % R);
    const long long o = offsets[k];
    const long long c = offsets[k + 1] - o;
    if (c < 5) {
        if (threadIdx.x == 0) { kept[k] = 0; term[k] = 0.0; }
        return;
    }
    const int* __restrict__ mem = members + o;
    const double expect = pct[j] * (double)N;
    const double coverage = (c - expect) * (c - expect) / expect;
    const double expect_d = sqrt(2.0 * (M_PI * radii[j] * radii[j] / (double)c) / 1.732);
    double acc = 0.0;
    for (long long a0 = 0; a0 < c; a0 += UNI_BS) {
        const long long a = a0 + threadIdx.x;
        const bool act = a < c;
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (act) {
            const int q = min(max(mem[a], 0), n - 1);
            ax = points[q * 3 + 0]; ay = points[q * 3 + 1]; az = points[q * 3 + 2];
        }
        float nn2 = __builtin_inff();
        for (long long b0 = 0; b0 < c; b0 += UNI_TILE) {
            const int len = (int)min((long long)UNI_TILE, c - b0);
            __syncthreads();
            for (int t = threadIdx.x; t < len; t += UNI_BS) {
                const int q = min(max(mem[b0 + t], 0), n - 1);
                tile[t] = make_float4(points[q * 3 + 0], points[q * 3 + 1], points[q * 3 + 2], 0.f);
            }
            __syncthreads();
            if (act) {
                for (int t = 0; t < len; ++t) {
                    const float4 v = tile[t];
                    const float d2 = sq3(v.x - ax, v.y - ay, v.z - az);
                    if (b0 + t != a) nn2 = fminf(nn2, d2);
                }
            }
        }
        if (act) {
            const double e = sqrt((double)nn2) - expect_d;
            acc += e * e / expect_d;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = UNI_BS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) { term[k] = coverage * (red[0] / (double)c); kept[k] = 1; }
}

// out[j] = mean of the kept disk terms of radius j (ascending seeds per lane, fixed butterfly), NaN if none was kept
__global__ __launch_bounds__(64) void disk_uniformity_mean_kernel(int S, int R, const double* __restrict__ term, const int* __restrict__ kept,
                                                                   double* __restrict__ out) {
    const int j = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    int c = 0;
    for (int i = lane; i < S; i += 64) {
        const long long k = (long long)i * R + j;
        if (kept[k]) { s += term[k]; ++c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    if (lane == 0) out[j] = c ? s / c : __builtin_nan("");
}

// per-row mean and population std (ddof 0) over the non-NaN entries, fp64, fixed order; NaN for a row without any
__global__ __launch_bounds__(256) void row_mean_std_kernel(int n, const float* __restrict__ x, double* __restrict__ out) {
    __shared__ double red[256];
    __shared__ long long cnt[256];
    const float* __restrict__ r = x + (size_t)blockIdx.x * n;
    double s = 0.0;
    long long c = 0;
    for (int i = threadIdx.x; i < n; i += 256)
        if (!__builtin_isnan(r[i])) { s += r[i]; ++c; }
    red[threadIdx.x] = s;
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; cnt[threadIdx.x] += cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    const long long total = cnt[0];
    const double mean = total ? red[0] / (double)total : __builtin_nan("");
    __syncthreads();
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256)
        if (!__builtin_isnan(r[i])) { const double d = r[i] - mean; v += d * d; }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = mean;
        out[2 * blockIdx.x + 1] = total ? sqrt(red[0] / (double)total) : __builtin_nan("");
    }
}

// the in-place scan of dispu_disk_count, for the other CSR builders (geodesic.hip)
int disk_scan_launch(long long M, long long* offsets, hipStream_t st) {
    hipLaunchKernelGGL(disk_scan_kernel, dim3(1), dim3(SCAN_BS), 0, st, M, offsets);
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_point_to_mesh(int n, const float* points, int F, const float* tris, const int* face_ids, const float* tile_box,
                                     float* dist, float* proj, int* face, int flags, void* stream) {
    if (n < 0 || F <= 0 || !tris || !face_ids) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const dim3 grid((n + P2M_WAVES - 1) / P2M_WAVES), block(64 * P2M_WAVES);
    const float4* t4 = reinterpret_cast<const float4*>(tris);
    const float4* b4 = reinterpret_cast<const float4*>(tile_box);
    if ((flags & DISPU_MESH_BRUTE_FORCE) || !tile_box)
        hipLaunchKernelGGL(point_to_mesh_kernel<true>, grid, block, 0, (hipStream_t)stream, n, points, F, t4, face_ids, b4, dist, proj, face);
    else
        hipLaunchKernelGGL(point_to_mesh_kernel<false>, grid, block, 0, (hipStream_t)stream, n, points, F, t4, face_ids, b4, dist, proj, face);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_disk_count(int S, int n, int R, const float* seeds, const float* points, const float* radii, long long* offsets,
                                  void* stream) {
    if (S < 0 || n <= 0 || R <= 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) return (int)hipMemsetAsync(offsets, 0, sizeof(long long), st);
    hipLaunchKernelGGL(disk_count_kernel, dim3((S + DISK_WAVES - 1) / DISK_WAVES), dim3(64 * DISK_WAVES), 0, st, S, n, R, seeds, points,
                       radii, offsets);
    DISPU_CHECK_LAUNCH();
    hipLaunchKernelGGL(disk_scan_kernel, dim3(1), dim3(SCAN_BS), 0, st, (long long)S * R, offsets);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_disk_fill(int S, int n, int R, const float* seeds, const float* points, const float* radii, const long long* offsets,
                                 int* members, void* stream) {
    if (S < 0 || n <= 0 || R <= 0) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    hipLaunchKernelGGL(disk_fill_kernel, dim3((S + DISK_WAVES - 1) / DISK_WAVES), dim3(64 * DISK_WAVES), 0, (hipStream_t)stream, S, n, R,
                       seeds, points, radii, offsets, members);
    return (int)hipGetLastError();
}

DISPU_EXPORT size_t dispu_disk_uniformity_scratch_bytes(int S, int R) {
    if (S <= 0 || R <= 0) return 0;
    return (size_t)S * R * (sizeof(double) + sizeof(int));
}

DISPU_EXPORT int dispu_disk_uniformity(int S, int R, int n, const float* points, const long long* offsets, const int* members,
                                       const double* radii, const double* pct, int N, void* scratch, size_t scratch_bytes, double* out,
                                       void* stream) {
    if (S <= 0 || R <= 0 || n <= 0 || N <= 0) return (int)hipErrorInvalidValue;
    if (!scratch || scratch_bytes < dispu_disk_uniformity_scratch_bytes(S, R)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    double* term = static_cast<double*>(scratch);
    int* kept = reinterpret_cast<int*>(term + (size_t)S * R);
    hipLaunchKernelGGL(disk_uniformity_kernel, dim3((unsigned)((long long)S * R)), dim3(UNI_BS), 0, st, R, n, points, offsets, members, radii,
                       pct, N, term, kept);
    DISPU_CHECK_LAUNCH();
    hipLaunchKernelGGL(disk_uniformity_mean_kernel, dim3(R), dim3(64), 0, st, S, R, term, kept, out);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_row_mean_std(int b, int n, const float* x, double* out, void* stream) {
    if (b < 0 || n <= 0) return (int)hipErrorInvalidValue;
    if (b == 0) return 0;
    hipLaunchKernelGGL(row_mean_std_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, n, x, out);
    return (int)hipGetLastError();
}
