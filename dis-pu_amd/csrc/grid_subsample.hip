// Grid subsampling (gfx950): every point of a cloud that falls into a cube of edge dl is replaced by the cube's barycentre, with the mean
// feature and the most frequent label of the cube.  Replaces libs/cpp_wrappers/cpp_subsampling (grid_subsampling.cpp:5-106,
// grid_subsampling.h:10-80, cloud.cpp:27-67), the KPConv voxel-grid subsampler, bit for bit: the yardstick is the sequential float32
// numpy restatement in tests/grid_subsample_oracle.py, itself held to outputs recorded from the reference's own function.
//
// The reference adds the points of a voxel in ascending point index into an std::unordered_map.  Here the same order comes from a STABLE
// device-wide radix sort of (voxel key, point index): equal keys keep ascending index, so a serial walk along each run of equal keys
// adds in the reference's order.  All arithmetic is fp32 with one rounding per operation (the library is built with -ffp-contract=off,
// divisions are the correctly rounded ones).  No float atomics anywhere: two runs give identical bytes.
//
//   bounds    per-workgroup min / max / non-finite partials, finished by one small workgroup          -> READBACK 1 (7 words)
//   grid      origin, NX, NY, NZ, the key range and the pass count: on the host, in grid_params() ONLY
//   keys      key[i] = iX + NX iY + NX NY iZ - key_min (uint64), val[i] = i (uint32)
//   sort      the stable LSD radix sort of radix_sort.hip, ceil(bits / 8) passes (none when the grid is one cell)
//   heads     head[j] = (j == 0 || key[j] != key[j-1]); an exclusive scan numbers the voxels and gives the start of every run and the
//             voxel count m                                                                            -> READBACK 2 (m)
//   reduce    one lane per (voxel, output column) walks its run from start to end: serial by necessity, the float order is pinned
//   labels    per label column, the same sorter on (voxel id << 32) | (label ^ 0x80000000), then per voxel the longest run of equal
//             keys, the first such run winning: ties go to the smallest label (signed)
//
// Cross-workgroup ordering is by kernel boundaries only: no kernel waits on anything another workgroup writes.  The sorter, the
// device-wide scan and the run heads (RadixSorter, exclusive_scan_u32, run_heads_scan) are those of radix_sort.hip.
// Two small host readbacks per call (dispu_grid_subsample_plan): the bounds with the non-finite flag, and m.
#include "internal.h"
#include <math.h>
#include <float.h>

namespace dispu {

constexpr int kBoundsMaxBlocks = 1024;

// ---- bounds ----------------------------------------------------------------------------------------------------------------------------
struct Bounds {
    float mn[3], mx[3];
    uint32_t bad;
};

__device__ __forceinline__ void bounds_block_reduce(Bounds& b, Bounds* lds) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = __shfl_xor(b.mn[c], o, kWave), z = __shfl_xor(b.mx[c], o, kWave);
            b.mn[c] = a < b.mn[c] ? a : b.mn[c];
            b.mx[c] = z > b.mx[c] ? z : b.mx[c];
        }
        b.bad |= __shfl_xor(b.bad, o, kWave);
    }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) lds[w] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kRsWaves; ++i) {
            for (int c = 0; c < 3; ++c) {
                b.mn[c] = lds[i].mn[c] < b.mn[c] ? lds[i].mn[c] : b.mn[c];
                b.mx[c] = lds[i].mx[c] > b.mx[c] ? lds[i].mx[c] : b.mx[c];
            }
            b.bad |= lds[i].bad;
        }
    }
}

// partial[blockIdx.x] = min / max / non-finite flag of the points this workgroup strides over; every workgroup sees at least one point
__global__ __launch_bounds__(kRsThreads) void bounds_partial_kernel(const float* __restrict__ points, size_t n, Bounds* __restrict__ partial) {
    __shared__ Bounds lds[kRsWaves];
    Bounds b;
    for (int c = 0; c < 3; ++c) b.mn[c] = b.mx[c] = points[c];      // the reference starts from point 0 (cloud.cpp:30,51)
    b.bad = 0;
    for (size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kRsThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = points[3 * i + c];
            b.bad |= !(fabsf(v) <= FLT_MAX);
            b.mn[c] = v < b.mn[c] ? v : b.mn[c];
            b.mx[c] = v > b.mx[c] ? v : b.mx[c];
        }
    }
    bounds_block_reduce(b, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(kRsThreads) void bounds_finish_kernel(const Bounds* __restrict__ partial, int blocks, Bounds* __restrict__ out) {
    __shared__ Bounds lds[kRsWaves];
    Bounds b = partial[0];
    for (int i = threadIdx.x; i < blocks; i += kRsThreads) {
        const Bounds p = partial[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b.mn[c] = p.mn[c] < b.mn[c] ? p.mn[c] : b.mn[c];
            b.mx[c] = p.mx[c] > b.mx[c] ? p.mx[c] : b.mx[c];
        }
        b.bad |= p.bad;
    }
    bounds_block_reduce(b, lds);
    if (threadIdx.x == 0) *out = b;
}

// ---- grid parameters: the ONE place where origin, NX, NY, NZ and the key range are computed (host, fp32, one rounding per operation) ----
struct GridParams {
    float origin[3];
    long long N[3];          // NX, NY, NZ
    long long key_min;       // the smallest key a point can get (0 unless an axis has a point below the rounded origin, see below)
    int bits, passes;
    int status;              // 0, or DISPU_GRID_AXIS_X.. when an axis has more than 2^21 cells
};

static int bit_length_u64(unsigned long long x) {
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

static inline float cell_f(float p, float o, float dl) {
#pragma clang fp contract(off)
    const float t = p - o;
    return floorf(t / dl);
}

static GridParams grid_params(const Bounds& b, float dl) {
#pragma clang fp contract(off)
    GridParams g;
    const float inv = 1.0f / dl;                                  // grid_subsampling.cpp:27: (1/sampleDl) in float
    long long lo[3];
    g.status = 0;
    for (int c = 0; c < 3; ++c) {
        const float s = b.mn[c] * inv;
        g.origin[c] = floorf(s) * dl;
        const float top = cell_f(b.mx[c], g.origin[c], dl);       // :30-32
        const float bot = cell_f(b.mn[c], g.origin[c], dl);
        // in float, before any conversion to an integer: at most 2^21 cells per axis keeps every key below 2^63
        if (!(top + 1.0f <= 2097152.0f) || !(bot >= -2097152.0f)) {
            if (!g.status) g.status = DISPU_GRID_AXIS_X + c;
            g.N[c] = 1;
            lo[c] = 0;
            continue;
        }
        g.N[c] = (long long)top + 1;
        // floor(min * inv) * dl is rounded twice and can land a few ulps ABOVE the minimum; such a point gets cell -1 on that axis.  The
        // reference converts the negative float to size_t and lets the key wrap modulo 2^64, which groups exactly like signed keys do;
        // here keys are signed, and the sorter sees key - key_min >= 0
        lo[c] = (long long)bot;
    }
    g.key_min = lo[0] + g.N[0] * lo[1] + g.N[0] * g.N[1] * lo[2];
    const long long key_max = (g.N[0] - 1) + g.N[0] * (g.N[1] - 1) + g.N[0] * g.N[1] * (g.N[2] - 1);
    g.bits = bit_length_u64((unsigned long long)key_max - (unsigned long long)g.key_min);        // modulo 2^64: no signed overflow
    g.passes = (g.bits + 7) / 8;
    return g;
}

__global__ __launch_bounds__(kRsThreads) void grid_keys_kernel(const float* __restrict__ points, size_t n, float ox, float oy, float oz, float dl,
                                                               long long NX, long long NXY, long long key_min, uint64_t* __restrict__ keys,
                                                               uint32_t* __restrict__ vals) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (i >= n) return;
    const float tx = points[3 * i + 0] - ox, ty = points[3 * i + 1] - oy, tz = points[3 * i + 2] - oz;
    const long long ix = (long long)floorf(__fdiv_rn(tx, dl));    // :53-55, the correctly rounded division
    const long long iy = (long long)floorf(__fdiv_rn(ty, dl));
    const long long iz = (long long)floorf(__fdiv_rn(tz, dl));
    keys[i] = (uint64_t)ix + (uint64_t)NX * (uint64_t)iy + (uint64_t)NXY * (uint64_t)iz - (uint64_t)key_min;   // modulo 2^64, >= 0
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kRsThreads) void iota_kernel(size_t n, uint32_t* __restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (i < n) vals[i] = (uint32_t)i;
}

// ---- runs --------------------------------------------------------------------------------------------------------------------------------
// keys == nullptr: all keys are equal (the zero-pass path).  ex: run_heads_scan's exclusive scan of the heads, replaced in place by the voxel id of every sorted position; start[v] = the first position of voxel
// v, start[m] = n
__global__ __launch_bounds__(kRsThreads) void runs_kernel(const uint64_t* __restrict__ keys, size_t n, uint32_t* __restrict__ ex,
                                                          uint32_t* __restrict__ start) {
    const size_t j = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t h = (j == 0 || (keys && keys[j] != keys[j - 1])) ? 1u : 0u;
    const uint32_t e = ex[j];                        // heads before j: e < n, and e + h <= n
    if (h) start[e] = (uint32_t)j;
    if (j == n - 1) start[e + h] = (uint32_t)n;
    ex[j] = e + h - 1u;
}

// ---- reduce: one lane per (voxel, column), columns = 3 coordinates then fdim features ------------------------------------------------------
// (positions and point indices are clamped to n: a no-op for the sorter's output, it keeps a wrong table from reading outside)
__global__ __launch_bounds__(kRsThreads) void grid_reduce_kernel(uint32_t n, uint32_t m, int fdim, const uint32_t* __restrict__ start,
                                                                 const uint32_t* __restrict__ perm, const float* __restrict__ points,
                                                                 const float* __restrict__ features, float* __restrict__ out_points,
                                                                 float* __restrict__ out_features) {
#pragma clang fp contract(off)
    const int cols = 3 + fdim;
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t >= (size_t)m * cols) return;
    const uint32_t v = (uint32_t)(t / cols);
    const int c = (int)(t % cols);
    const uint32_t lo = start[v], hi = min(start[v + 1], n);
    float acc = 0.0f;                                // SampledData(): point and features start from 0
    if (c < 3) {
        for (uint32_t j = lo; j < hi; ++j) acc += points[3 * (size_t)min(perm[j], n - 1) + c];
        const float r = (float)(1.0 / (double)(int)(hi - lo));     // :87: point * (1.0 / count), the reciprocal in double, then float
        out_points[3 * (size_t)v + c] = acc * r;
    } else {
        for (uint32_t j = lo; j < hi; ++j) acc += features[(size_t)min(perm[j], n - 1) * fdim + (c - 3)];
        out_features[(size_t)v * fdim + (c - 3)] = __fdiv_rn(acc, (float)(int)(hi - lo));   // :94: f / count
    }
}

// ---- labels --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void label_keys_kernel(size_t n, const uint32_t* __restrict__ vid, const uint32_t* __restrict__ perm,
                                                                const int* __restrict__ classes, int ldim, int col,
                                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t j = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t l = (uint32_t)classes[(size_t)min(perm[j], (uint32_t)(n - 1)) * ldim + col] ^ 0x80000000u;      // unsigned order = signed order
    keys[j] = ((uint64_t)vid[j] << 32) | l;
    vals[j] = (uint32_t)j;
}

// keys sorted: voxel v owns [start[v], start[v+1]) again; the longest run of equal keys, the first such run (the smallest label) winning
__global__ __launch_bounds__(kRsThreads) void label_mode_kernel(uint32_t n, uint32_t m, const uint32_t* __restrict__ start, const uint64_t* __restrict__ keys,
                                                                int ldim, int col, int* __restrict__ out_classes) {
    const size_t v = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (v >= m) return;
    const uint32_t lo = min(start[v], n - 1), hi = min(start[v + 1], n);
    uint64_t best = keys[lo], cur = best;
    uint32_t best_n = 0, cur_n = 0;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint64_t k = keys[j];
        if (k != cur) { cur = k; cur_n = 0; }
        ++cur_n;
        if (cur_n > best_n) { best_n = cur_n; best = cur; }
    }
    out_classes[v * ldim + col] = (int)((uint32_t)best ^ 0x80000000u);
}

// ---- scratch of the whole operator -----------------------------------------------------------------------------------------------------------
struct GridScratch {
    RadixSorter sort;
    uint32_t *perm, *vid, *start;
    Bounds *partial, *bounds;                        // bounds: the Bounds result, and the voxel count m 128 bytes behind it
    size_t total;
};
static GridScratch grid_scratch(size_t n, void* base = nullptr) {
    GridScratch s;
    Carver cv{(char*)base};
    s.sort.carve(cv, n);
    s.perm = cv.ptr<uint32_t>(4 * n);
    s.vid = cv.ptr<uint32_t>(4 * n);
    s.start = cv.ptr<uint32_t>(4 * (n + 1));
    s.partial = cv.ptr<Bounds>(sizeof(Bounds) * kBoundsMaxBlocks);
    s.bounds = cv.ptr<Bounds>(256);
    s.total = cv.off;
    return s;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_grid_subsample_scratch_bytes(long long n, int fdim, int ldim) {
    if (n <= 0 || n >= (1ll << 31) || fdim < 0 || ldim < 0) return 0;
    return grid_scratch((size_t)n).total;            // features and labels are read in place: fdim and ldim add nothing
}

DISPU_EXPORT int dispu_grid_subsample_plan(long long n, const float* points, float dl, void* scratch, size_t scratch_bytes, int* m_out,
                                           int* status_out, double* grid_out, void* stream) {
    if (!m_out || !status_out) return (int)hipErrorInvalidValue;
    *m_out = 0;
    *status_out = 0;
    if (n >= (1ll << 31)) { *status_out = DISPU_GRID_TOO_MANY_POINTS; return 0; }   // before anything is touched
    if (n <= 0 || !points || !(dl > 0.0f) || !(dl <= FLT_MAX)) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)n;
    GridScratch s = grid_scratch(N, scratch);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* d_m = (uint32_t*)((char*)s.bounds + 128);

    const int bblocks = (int)(rs_blocks(N) < (unsigned)kBoundsMaxBlocks ? rs_blocks(N) : (unsigned)kBoundsMaxBlocks);
    hipLaunchKernelGGL(bounds_partial_kernel, dim3(bblocks), dim3(kRsThreads), 0, st, points, N, s.partial);
    hipLaunchKernelGGL(bounds_finish_kernel, dim3(1), dim3(kRsThreads), 0, st, (const Bounds*)s.partial, bblocks, s.bounds);
    DISPU_CHECK_LAUNCH();
    Bounds hb;
    DISPU_TRY(hipMemcpyAsync(&hb, s.bounds, sizeof(Bounds), hipMemcpyDeviceToHost, st));      // readback 1
    DISPU_TRY(hipStreamSynchronize(st));
    if (hb.bad) { *status_out = DISPU_GRID_NONFINITE; return 0; }
    const GridParams g = grid_params(hb, dl);
    if (grid_out) {
        for (int c = 0; c < 3; ++c) { grid_out[c] = g.origin[c]; grid_out[3 + c] = (double)g.N[c]; }
        grid_out[6] = g.passes;
        grid_out[7] = (double)g.key_min;
    }
    if (g.status) { *status_out = g.status; return 0; }

    const uint64_t* sorted = nullptr;                // null: one cell, every key equal
    if (g.passes == 0) {
        hipLaunchKernelGGL(iota_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, s.perm);
    } else {
        hipLaunchKernelGGL(grid_keys_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, points, N, g.origin[0], g.origin[1], g.origin[2],
                           dl, g.N[0], g.N[0] * g.N[1], g.key_min, s.sort.k[0], s.sort.v[0]);
        const int rc = s.sort.sort(N, g.passes, st);
        if (rc) return rc;
        sorted = s.sort.keys();
        DISPU_TRY(hipMemcpyAsync(s.perm, s.sort.vals(), 4 * N, hipMemcpyDeviceToDevice, st));
    }
    const int rc = run_heads_scan(sorted, N, s.vid, s.sort.sums, d_m, st);
    if (rc) return rc;
    hipLaunchKernelGGL(runs_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, sorted, N, s.vid, s.start);
    DISPU_CHECK_LAUNCH();
    uint32_t hm = 0;
    DISPU_TRY(hipMemcpyAsync(&hm, d_m, sizeof(hm), hipMemcpyDeviceToHost, st));               // readback 2
    DISPU_TRY(hipStreamSynchronize(st));
    *m_out = (int)hm;
    return 0;
}

DISPU_EXPORT int dispu_grid_subsample_emit(long long n, int m, int fdim, int ldim, const float* points, const float* features,
                                           const int* classes, void* scratch, size_t scratch_bytes, float* out_points, float* out_features,
                                           int* out_classes, void* stream) {
    if (n <= 0 || n >= (1ll << 31) || m <= 0 || m > n || fdim < 0 || ldim < 0 || !points || !out_points) return (int)hipErrorInvalidValue;
    if ((fdim > 0 && (!features || !out_features)) || (ldim > 0 && (!classes || !out_classes))) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)n;
    GridScratch s = grid_scratch(N, scratch);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grid_reduce_kernel, dim3(rs_blocks((size_t)m * (3 + fdim))), dim3(kRsThreads), 0, st, (uint32_t)N, (uint32_t)m, fdim, s.start, s.perm,
                       points, features, out_points, out_features);
    DISPU_CHECK_LAUNCH();
    const int lpasses = (32 + bit_length_u64((unsigned long long)m - 1) + 7) / 8;
    for (int col = 0; col < ldim; ++col) {
        hipLaunchKernelGGL(label_keys_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, s.vid, s.perm, classes, ldim, col, s.sort.k[0],
                           s.sort.v[0]);
        const int rc = s.sort.sort(N, lpasses, st);
        if (rc) return rc;
        hipLaunchKernelGGL(label_mode_kernel, dim3(rs_blocks((size_t)m)), dim3(kRsThreads), 0, st, (uint32_t)N, (uint32_t)m, s.start, s.sort.keys(),
                           ldim, col, out_classes);
    }
    return (int)hipGetLastError();
}
