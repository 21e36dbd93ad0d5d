// The Morton-cell pre-pass over a packed ragged batch of clouds: every segment ordered along a Morton curve and cut into cells of
// consecutive sorted positions, each with its bounding box.  Two clients: the cell-skipping farthest point sampling of fps_cells.hip
// (which describes why a cell can be skipped) and the cell-pruned k-NN of normals.hip.
//
//   device-wide over the whole packed batch (ordering by kernel boundaries only, no kernel waits on another workgroup):
//     bounds   per segment: bounding box and non-finite flag (integer atomics on order-preserving keys: order-free, deterministic)
//     keys     key = segment id << 30 | 30-bit Morton code in the segment's box (cubic voxels, edge = largest extent / 1024; a zero
//              extent gives code 0 on every point: no division by it), value = global point index
//     sort     ONE dispu_radix_sort_pairs over the batch: stable, so equal keys keep ascending index; a segment's sorted positions
//              are its own range [off[c], off[c + 1])
//     cells    one wave per cell: gathers (x, y, z, local index) into sorted order, sets the running distances to 1e38, and writes
//              the cell's box, largest running distance (1e38) and candidate (the point of best tie priority)
#include "morton_cells.h"
#include "fps_keys.h"

namespace dispu {

constexpr int kFpcPre = 256, kFpcChunk = kFpcPre * 16;        // pre-pass: 256 threads, 4096 points per workgroup
constexpr int kFpcMortonBits = 30;

__device__ __forceinline__ uint32_t fpc_spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// segb[c][8]: ~ordered(min) x3, ordered(max) x3, non-finite flag, unused; zero-filled before (the identity of atomicMax / atomicOr)
__global__ __launch_bounds__(kFpcPre) void fpc_bounds_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                             const int* __restrict__ moff, uint32_t* __restrict__ segb, CellsMode mode) {
    __shared__ float red[kFpcPre / kWave][8];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const SegExt e = seg_ext(off, moff, c, 0, 0);
    const int lo = blockIdx.x * kFpcChunk;
    if (!fpc_served(e.n, e.m, mode) || lo >= e.n) return;
    const int hi = min(e.n, lo + kFpcChunk);
    const float* __restrict__ p = xyz + e.base * 3;
    float mn[3] = {3e38f, 3e38f, 3e38f}, mx[3] = {-3e38f, -3e38f, -3e38f};
    uint32_t bad = 0u;
    for (int k = lo + tid; k < hi; k += kFpcPre)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = p[(size_t)k * 3 + a];
            bad |= !(fabsf(v) <= 3.4028235e38f);
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, kWave));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, kWave));
        }
        bad |= __shfl_xor(bad, o, kWave);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[w][a] = mn[a]; red[w][3 + a] = mx[a]; }
        red[w][6] = __uint_as_float(bad);
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kFpcPre / kWave; ++i) {
            for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], red[i][a]); mx[a] = fmaxf(mx[a], red[i][3 + a]); }
            bad |= __float_as_uint(red[i][6]);
        }
        uint32_t* b = segb + (size_t)c * 8;
        for (int a = 0; a < 3; ++a) {
            atomicMax(b + a, ~f32_to_ordered(mn[a]));
            atomicMax(b + 3 + a, f32_to_ordered(mx[a]));
        }
        if (bad) atomicOr(b + 6, 1u);
    }
}

// every point of the batch gets a key (the sort runs over all of it); segments that are not served, or hold a non-finite
// coordinate, get Morton code 0
__global__ __launch_bounds__(kFpcPre) void fpc_keys_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                           const int* __restrict__ moff, const uint32_t* __restrict__ segb,
                                                           unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, CellsMode mode) {
    const int c = blockIdx.y, tid = threadIdx.x;
    const SegExt e = seg_ext(off, moff, c, 0, 0);
    const int lo = blockIdx.x * kFpcChunk;
    if (lo >= e.n) return;
    const int hi = min(e.n, lo + kFpcChunk);
    const float* __restrict__ p = xyz + e.base * 3;
    const uint32_t* b = segb + (size_t)c * 8;
    float l[3] = {0.f, 0.f, 0.f}, scale = 0.f;
    if (fpc_served(e.n, e.m, mode) && !b[6]) {
        float ext = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            l[a] = ordered_to_f32(~b[a]);
            ext = fmaxf(ext, ordered_to_f32(b[3 + a]) - l[a]);
        }
        if (ext > 0.f && ext <= 3.4028235e38f) scale = 1024.0f / ext;          // a degenerate (or overflowing) box: one Morton cell
    }
    const unsigned long long seg = (unsigned long long)c << kFpcMortonBits;
    for (int k = lo + tid; k < hi; k += kFpcPre) {
        uint32_t mort = 0u;
        if (scale > 0.f) {
            uint32_t q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = (uint32_t)min(1023, max(0, (int)((p[(size_t)k * 3 + a] - l[a]) * scale)));
            mort = fpc_spread10(q[0]) | (fpc_spread10(q[1]) << 1) | (fpc_spread10(q[2]) << 2);
        }
        keys[e.base + k] = seg | mort;
        vals[e.base + k] = (uint32_t)(e.base + k);
    }
}

// one wave per cell.  spt[pos] = (x, y, z, local index as bits), td[pos] = 1e38, tab[cell][8] = lo x3, hi x3, 1e38, best tie key
__global__ __launch_bounds__(kFpcPre) void fpc_cells_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                            const int* __restrict__ moff, const uint32_t* __restrict__ segb,
                                                            const uint32_t* __restrict__ perm, float4* __restrict__ spt,
                                                            float* __restrict__ td, float* __restrict__ tab, int cell, CellsMode mode) {
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
    const SegExt e = seg_ext(off, moff, c, 0, 0);
    if (!fpc_served(e.n, e.m, mode) || segb[(size_t)c * 8 + 6]) return;
    const int S = fpc_cell_size_mode(e.n, cell, mode), K = (e.n + S - 1) / S;
    const int cb = blockIdx.x * (kFpcPre / kWave) + tid / kWave;
    if (cb >= K) return;
    const int pb = cb * S, cnt = min(S, e.n - pb);
    const size_t g0 = e.base + pb;
    float mn[3] = {3e38f, 3e38f, 3e38f}, mx[3] = {-3e38f, -3e38f, -3e38f};
    uint32_t bk = 0u;
    for (int i = lane; i < cnt; i += kWave) {
        const int k = max(0, min((int)((long long)perm[g0 + i] - (long long)e.base), e.n - 1));   // the segment's own row, by the key's high bits
        const size_t g = e.base + (size_t)k;
        const float x = xyz[g * 3 + 0], y = xyz[g * 3 + 1], z = xyz[g * 3 + 2];
        spt[g0 + i] = make_float4(x, y, z, __int_as_float(k));
        td[g0 + i] = 1e38f;
        mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
        mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
        mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        const uint32_t key = fps_tiekey(k);
        bk = key > bk ? key : bk;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, kWave));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, kWave));
        }
        const uint32_t ok = (uint32_t)__shfl_xor((int)bk, o, kWave);
        bk = ok > bk ? ok : bk;
    }
    if (lane == 0) {
        float* t = tab + (fpc_cell_base(e.base, c) + cb) * 8;
        *reinterpret_cast<float4*>(t) = make_float4(mn[0], mn[1], mn[2], mx[0]);
        *reinterpret_cast<float4*>(t + 4) = make_float4(mx[1], mx[2], 1e38f, __uint_as_float(bk));
    }
}

FpcScratch fpc_scratch(size_t N, int C) {
    FpcScratch s;
    Carver cv;
    s.kin = cv.take(8 * N);                          // kin, kout adjacent and in this order: spt lies over both
    s.kout = cv.take(8 * N);
    s.vin = cv.take(4 * N);
    s.vout = cv.take(4 * N);
    s.sort_bytes = dispu_radix_sort_scratch_bytes((long long)N);
    s.sort = cv.take(s.sort_bytes);
    s.tab = cv.take(32 * (N / kFpcMinCell + (size_t)C));
    s.segb = cv.take(32 * (size_t)C);
    s.total = cv.off;
    return s;
}

static bool fpc_cell_ok(int cell) {
    return cell == 0 || (cell >= kFpcMinCell && cell <= kFpcMaxCell && (cell & (cell - 1)) == 0);
}

int fpc_plan(int C, const int* off_host, const int* moff_host, int cell, CellsMode mode, int* nall, int* nserved, int* kmax) {
    *nall = *nserved = *kmax = 0;
    if (C <= 0 || C > 65535 || !off_host || !moff_host || off_host[0] != 0 || moff_host[0] != 0 || !fpc_cell_ok(cell))
        return (int)hipErrorInvalidValue;
    for (int c = 0; c < C; ++c) {
        if (off_host[c + 1] <= off_host[c] || moff_host[c + 1] <= moff_host[c]) return (int)hipErrorInvalidValue;
        const int n = off_host[c + 1] - off_host[c], m = moff_host[c + 1] - moff_host[c];
        if (n > *nall) *nall = n;
        if (!fpc_served(n, m, mode)) continue;
        if (n > kFpcMaxN) return (int)hipErrorInvalidValue;
        const int S = fpc_cell_size_mode(n, cell, mode), K = (n + S - 1) / S;
        if (n > *nserved) *nserved = n;
        if (K > *kmax) *kmax = K;
    }
    return 0;
}

size_t fps_cells_scratch(int C, const int* off_host, const int* moff_host, int cell, CellsMode mode) {
    int nall, nserved, kmax;
    if (fpc_plan(C, off_host, moff_host, cell, mode, &nall, &nserved, &kmax) != 0) return 0;
    if (!nserved) return 0;
    return fpc_scratch((size_t)off_host[C], C).total;
}

int fpc_prepass(int C, const int* off, const int* moff, const float* inp, char* base, const FpcScratch& s, size_t N, int nall,
                       int nserved, int kmax, int cell, CellsMode mode, hipStream_t st) {
    unsigned long long* kin = (unsigned long long*)(base + s.kin);
    unsigned long long* kout = (unsigned long long*)(base + s.kout);
    uint32_t* vin = (uint32_t*)(base + s.vin);
    uint32_t* vout = (uint32_t*)(base + s.vout);
    uint32_t* segb = (uint32_t*)(base + s.segb);
    float* tab = (float*)(base + s.tab);
    float4* spt = (float4*)(base + s.kin);            // 16 N bytes over the two key buffers
    float* td = (float*)(base + s.vin);
    int segbits = 0;
    while ((1 << segbits) < C) ++segbits;
    DISPU_TRY(hipMemsetAsync(segb, 0, 32 * (size_t)C, st));
    hipLaunchKernelGGL(fpc_bounds_kernel, dim3((nserved + kFpcChunk - 1) / kFpcChunk, C), dim3(kFpcPre), 0, st, inp, off, moff, segb, mode);
    DISPU_CHECK_LAUNCH();
    hipLaunchKernelGGL(fpc_keys_kernel, dim3((nall + kFpcChunk - 1) / kFpcChunk, C), dim3(kFpcPre), 0, st, inp, off, moff, segb, kin, vin, mode);
    DISPU_CHECK_LAUNCH();
    const int rs = dispu_radix_sort_pairs((long long)N, kFpcMortonBits + segbits, kin, vin, kout, vout, base + s.sort, s.sort_bytes, st);
    if (rs != 0) return rs;
    constexpr int wpb = kFpcPre / kWave;
    hipLaunchKernelGGL(fpc_cells_kernel, dim3((kmax + wpb - 1) / wpb, C), dim3(kFpcPre), 0, st, inp, off, moff, segb, vout, spt, td, tab, cell,
                       mode);
    DISPU_CHECK_LAUNCH();
    return 0;
}

// the pre-pass for a client other than FPS (contract: internal.h)
int cells_batch_check(int C, const int* off_host, int* nall, int* kmax) {
    int na, nserved, km;
    const int rc = fpc_plan(C, off_host, off_host, 0, kCellsFixed64, &na, &nserved, &km);
    if (nall) *nall = na;
    if (kmax) *kmax = km;
    return rc;
}
size_t fps_cells_prepass_scratch(int C, const int* off_host) {
    if (cells_batch_check(C, off_host) != 0) return 0;
    return fpc_scratch((size_t)off_host[C], C).total;
}
int fps_cells_prepass(int C, const int* off, const int* off_host, const float* inp, void* scratch, size_t scratch_bytes,
                      const float4** spt, const float** tab, const uint32_t** segb, int* kmax, hipStream_t st) {
    int nall, nserved;
    const int rc = fpc_plan(C, off_host, off_host, 0, kCellsFixed64, &nall, &nserved, kmax);
    if (rc != 0) return rc;
    if (!off || !inp) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)off_host[C];
    const FpcScratch s = fpc_scratch(N, C);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    char* base = (char*)scratch;
    *spt = (const float4*)(base + s.kin);
    *tab = (const float*)(base + s.tab);
    *segb = (const uint32_t*)(base + s.segb);
    return fpc_prepass(C, off, off, inp, base, s, N, nall, nserved, *kmax, 0, kCellsFixed64, st);
}

}  // namespace dispu
