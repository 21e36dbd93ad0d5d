// Outlier removal for a packed ragged batch of clouds: behind dispu_knn_mean_dist_segments, dispu_radius_count_segments,
// dispu_outlier_threshold_segments and dispu_compact_segments (include/dispu_hip.h, which states every definition).  The reference has
// no counterpart; these are the two standard filters of point-cloud toolkits, statistical (mean distance to the k nearest neighbours
// against the cloud's mean + ratio * std) and radius (fewer than m neighbours within r), made exact and reproducible.
//
//   mean_dist  the search of knn_cells_search.h at k + 1 (the one behind the normals, morton_cells.hip's pre-pass before it), then from the
//              neighbourhood in registers: s = sum of sqrt((double)d2_j) in ascending rank, mean = (float)(s / max(k' - 1, 1)).
//              No [n, k] tensor reaches memory.
//   count      (the prologue of knn_cells_prologue.h, not the search) one wave per cell, one query per lane; the segment's box table 64 boxes per step (one per lane).  A cell is visited
//              unless its box-to-box lower bound exceeds r2 (cell_box_lb: lb <= d2 bit for bit, so no point within r2 is lost), or the
//              point-to-box bound exceeds r2 on every lane that still counts.  A visit is dense, 64 x 64.  The walk ends once every
//              live lane holds more than `cap` matches, its own (d2 = 0) included; the own match is subtracted at the end.
//   threshold  one workgroup per segment over the stored fp32 mean_dist: two passes in double, every thread four strided partial sums,
//              then a wave tree and a serial sum over the waves: an order that depends on n alone.
//   compact    keep flags -> exclusive_scan_u32 -> a scatter that forms the same flag again: kept points in input order.
//
// Ordinary stores only, no atomics of its own, ordering by kernel boundaries only, identical bytes from run to run.
#include "knn_cells.h"

namespace dispu {

constexpr int kOutThr = 1024, kOutThrWaves = kOutThr / kWave;    // the statistics workgroup
constexpr int kOutCmp = 256;                                     // the compaction kernels

// k: the list length, the caller's k + 1: the neighbourhood includes the point itself
template <int KMAX>
__global__ __launch_bounds__(kNrmThreads) void knn_mean_dist_kernel(const int* __restrict__ off, const uint32_t* __restrict__ segb,
                                                                    const float4* __restrict__ spt, const float* __restrict__ tab, int k,
                                                                    float* __restrict__ mean_dist, int* __restrict__ status) {
#include "knn_cells_prologue.h"  // segment, cell, query, as text
    const int s = cb;                                                           // the search starts in the wave's own cell
#include "knn_cells_search.h"    // the search, as text: defines `kp` and `best`
    if (!valid) return;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < kp) sum += sqrt((double)best.d2(j));
    mean_dist[base + (size_t)__float_as_int(q.w)] = (float)(sum / (double)max(kp - 1, 1));
}

__global__ __launch_bounds__(kNrmThreads) void radius_count_kernel(const int* __restrict__ off, const uint32_t* __restrict__ segb,
                                                                   const float4* __restrict__ spt, const float* __restrict__ tab, float r2,
                                                                   int cap, int* __restrict__ count, int* __restrict__ status) {
#include "knn_cells_prologue.h"  // segment, cell, query, as text
    int raw = 0;                                                                // matches so far, the query's own among them: raw <= n
    for (int j0 = 0; j0 < K && __any(valid && raw <= cap); j0 += kWave) {
        const int j = j0 + lane;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        bool near = false;
        if (j < K) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            near = cell_box_lb(a, b, qlo4.x, qlo4.y, qlo4.z, qlo4.w, qhi4.x, qhi4.y) <= r2;
        }
        unsigned long long reach = __ballot(near);
        while (reach) {
            const int bl = (int)__builtin_ctzll(reach);
            reach &= reach - 1;
            const float4 a1 = make_float4(__shfl(a.x, bl, kWave), __shfl(a.y, bl, kWave), __shfl(a.z, bl, kWave), __shfl(a.w, bl, kWave));
            const float4 b1 = make_float4(__shfl(b.x, bl, kWave), __shfl(b.y, bl, kWave), 0.f, 0.f);
            if (!__any(valid && raw <= cap && cell_box_lb(a1, b1, q.x, q.y, q.z, q.x, q.y, q.z) <= r2)) continue;
            const int cj = j0 + bl, cnt = min(kNrmCell, n - cj * kNrmCell);
            const float4 p = sp[cj * kNrmCell + min(lane, cnt - 1)];
            for (int i = 0; i < cnt; ++i) {
                const float px = __shfl(p.x, i, kWave), py = __shfl(p.y, i, kWave), pz = __shfl(p.z, i, kWave);
                raw += sqdist3<false>(px - q.x, py - q.y, pz - q.z) <= r2 ? 1 : 0;
            }
            if (!__any(valid && raw <= cap)) break;                           // every live lane is past the cap: the outer loop ends too
        }
    }
    if (valid) count[base + (size_t)__float_as_int(q.w)] = min(cap, raw - 1);
}

// sum over the workgroup in a fixed order: a wave tree, then the waves in ascending order; every thread returns the total
__device__ __forceinline__ double out_block_sum(double v, double* red) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    __syncthreads();                                                            // red may still be read from the call before
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kOutThrWaves; ++i) t += red[i];
    return t;
}

__global__ __launch_bounds__(kOutThr) void outlier_threshold_kernel(const int* __restrict__ off, const float* __restrict__ mean_dist,
                                                                    const int* __restrict__ status, double ratio,
                                                                    double* __restrict__ stats) {
    __shared__ double red[kOutThrWaves];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (status[c] != 0) return;                                                 // a flagged segment has no mean_dist
    const int b0 = off[c], n = off[c + 1] - b0;
    const float* __restrict__ p = mean_dist + (size_t)b0;
    double mu = 0.0, tot = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (long long i = tid; i < n; i += 4 * kOutThr) {
            const long long i1 = i + kOutThr, i2 = i + 2 * kOutThr, i3 = i + 3 * kOutThr;
            const double d0 = (double)p[i] - mu;
            const double d1 = i1 < n ? (double)p[i1] - mu : 0.0;
            const double d2 = i2 < n ? (double)p[i2] - mu : 0.0;
            const double d3 = i3 < n ? (double)p[i3] - mu : 0.0;
            if (pass == 0) {
                a0 += d0; a1 += d1; a2 += d2; a3 += d3;
            } else {
                a0 += d0 * d0;
                if (i1 < n) a1 += d1 * d1;
                if (i2 < n) a2 += d2 * d2;
                if (i3 < n) a3 += d3 * d3;
            }
        }
        tot = out_block_sum((a0 + a1) + (a2 + a3), red);
        if (pass == 0) mu = tot / (double)n;
    }
    if (tid == 0) {
        const double sigma = sqrt(tot / (double)max(n - 1, 1));
        stats[(size_t)c * 3 + 0] = mu;
        stats[(size_t)c * 3 + 1] = sigma;
        stats[(size_t)c * 3 + 2] = mu + ratio * sigma;
    }
}

// the keep rule of point g (global row) of segment c.  rule 0: src int32 flags; 1: src fp32 mean_dist against stats[c][2]; 2: src int32
// counts against min_neighbors.  A flagged segment keeps nothing.
__device__ __forceinline__ bool out_keep(int rule, const void* __restrict__ src, const double* __restrict__ stats, int min_neighbors,
                                         const int* __restrict__ status, int c, size_t g) {
    if (status && status[c] != 0) return false;
    if (rule == 1) return (double)static_cast<const float*>(src)[g] <= stats[(size_t)c * 3 + 2];
    if (rule == 2) return static_cast<const int*>(src)[g] >= min_neighbors;
    return static_cast<const int*>(src)[g] != 0;
}

__global__ __launch_bounds__(kOutCmp) void compact_flags_kernel(const int* __restrict__ off, int rule, const void* __restrict__ src,
                                                                const double* __restrict__ stats, int min_neighbors,
                                                                const int* __restrict__ status, uint32_t* __restrict__ flags) {
    const int c = blockIdx.y, b0 = off[c], n = off[c + 1] - b0;
    const long long i = (long long)blockIdx.x * kOutCmp + threadIdx.x;
    if (i >= n) return;
    const size_t g = (size_t)b0 + (size_t)i;
    flags[g] = out_keep(rule, src, stats, min_neighbors, status, c, g) ? 1u : 0u;
}

// pos: the exclusive scan of the flags.  new_off[c] = pos of the segment's first row; new_off[C] is the scan's grand total
__global__ __launch_bounds__(kOutCmp) void compact_scatter_kernel(const int* __restrict__ off, const float* __restrict__ cloud, int rule,
                                                                  const void* __restrict__ src, const double* __restrict__ stats,
                                                                  int min_neighbors, const int* __restrict__ status,
                                                                  const uint32_t* __restrict__ pos, float* __restrict__ out_points,
                                                                  int* __restrict__ out_index, int* __restrict__ new_off) {
    const int c = blockIdx.y, b0 = off[c], n = off[c + 1] - b0;
    const long long i = (long long)blockIdx.x * kOutCmp + threadIdx.x;
    if (i >= n) return;
    const size_t g = (size_t)b0 + (size_t)i;
    const size_t o = (size_t)pos[g];
    if (i == 0) new_off[c] = (int)o;
    if (!out_keep(rule, src, stats, min_neighbors, status, c, g)) return;
    if (out_points) {
        out_points[o * 3 + 0] = cloud[g * 3 + 0];
        out_points[o * 3 + 1] = cloud[g * 3 + 1];
        out_points[o * 3 + 2] = cloud[g * 3 + 2];
    }
    out_index[o] = (int)i;
}

struct CmpScratch {
    uint32_t *flags, *sums;
    size_t total;
};
static CmpScratch cmp_scratch(size_t N, void* base = nullptr) {
    CmpScratch s;
    Carver cv{(char*)base};
    s.flags = cv.ptr<uint32_t>(4 * N);
    s.sums = cv.ptr<uint32_t>(4 * scan_blocks(N));
    s.total = cv.off;
    return s;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_knn_mean_dist_scratch_bytes(int C, const int* off_host, int k) {
    return k < 1 || k > 31 ? 0 : fps_cells_prepass_scratch(C, off_host);
}

DISPU_EXPORT int dispu_knn_mean_dist_segments(int C, const int* off, const int* off_host, int k, const float* cloud, float* mean_dist,
                                              int* status, void* scratch, size_t scratch_bytes, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (k < 1 || k > 31 || !off || !cloud || !mean_dist || !status) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const float4* spt;
    const float* tab;
    const uint32_t* segb;
    int kmax = 0;
    const int rp = fps_cells_prepass(C, off, off_host, cloud, scratch, scratch_bytes, &spt, &tab, &segb, &kmax, st);
    if (rp != 0) return rp;
    const dim3 grid((kmax + kNrmWaves - 1) / kNrmWaves, C), block(kNrmThreads);
    const int k1 = k + 1;
    dispatch_kmax(k1, [&](auto kmax_c) {
        hipLaunchKernelGGL((knn_mean_dist_kernel<decltype(kmax_c)::value>), grid, block, 0, st, off, segb, spt, tab, k1, mean_dist, status);
    });
    return (int)hipGetLastError();
}

DISPU_EXPORT size_t dispu_radius_count_scratch_bytes(int C, const int* off_host) {
    return fps_cells_prepass_scratch(C, off_host);
}

DISPU_EXPORT int dispu_radius_count_segments(int C, const int* off, const int* off_host, float radius, int cap, const float* cloud, int* count,
                                             int* status, void* scratch, size_t scratch_bytes, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (!(radius > 0.f) || !(radius <= 3.4028235e38f) || cap < 1 || !off || !cloud || !count || !status) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const float4* spt;
    const float* tab;
    const uint32_t* segb;
    int kmax = 0;
    const int rp = fps_cells_prepass(C, off, off_host, cloud, scratch, scratch_bytes, &spt, &tab, &segb, &kmax, st);
    if (rp != 0) return rp;
    const float r2 = radius * radius;                                           // one fp32 rounding (the build does not contract)
    hipLaunchKernelGGL(radius_count_kernel, dim3((kmax + kNrmWaves - 1) / kNrmWaves, C), dim3(kNrmThreads), 0, st, off, segb, spt, tab, r2, cap,
                       count, status);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_outlier_threshold_segments(int C, const int* off, const int* off_host, const float* mean_dist, const int* status,
                                                  double ratio, double* stats, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (!off || !mean_dist || !status || !stats || !(ratio >= -1.7976931348623157e308 && ratio <= 1.7976931348623157e308))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(outlier_threshold_kernel, dim3(C), dim3(kOutThr), 0, (hipStream_t)stream, off, mean_dist, status, ratio, stats);
    return (int)hipGetLastError();
}

DISPU_EXPORT size_t dispu_compact_scratch_bytes(int C, const int* off_host) {
    if (cells_batch_check(C, off_host) != 0) return 0;
    return cmp_scratch((size_t)off_host[C]).total;
}

DISPU_EXPORT int dispu_compact_segments(int C, const int* off, const int* off_host, const float* cloud, int rule, const void* src,
                                        const double* stats, int min_neighbors, const int* status, float* out_points, int* out_index,
                                        int* new_off, void* scratch, size_t scratch_bytes, void* stream) {
    int nall;
    const int rc = cells_batch_check(C, off_host, &nall);
    if (rc != 0) return rc;
    if (rule < 0 || rule > 2 || !off || !src || (rule == 1 && !stats) || (out_points && !cloud) || !out_index || !new_off)
        return (int)hipErrorInvalidValue;
    const size_t N = (size_t)off_host[C];
    const CmpScratch s = cmp_scratch(N, scratch);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((nall + kOutCmp - 1) / kOutCmp, C), block(kOutCmp);
    hipLaunchKernelGGL(compact_flags_kernel, grid, block, 0, st, off, rule, src, stats, min_neighbors, status, s.flags);
    DISPU_CHECK_LAUNCH();
    const int rs = exclusive_scan_u32(s.flags, N, s.sums, (uint32_t*)(new_off + C), st);
    if (rs != 0) return rs;
    hipLaunchKernelGGL(compact_scatter_kernel, grid, block, 0, st, off, cloud, rule, src, stats, min_neighbors, status, s.flags, out_points,
                       out_index, new_off);
    return (int)hipGetLastError();
}
