// Exact farthest point sampling for clouds ABOVE 24576 points (tf_sampling.cpp:94,118; kernel tf_sampling_g.cu:105-170 is the spec)
// with the cloud in global memory and Morton-cell skipping: behind dispu_fps_cells / dispu_fps_segments_auto (include/dispu_hip.h).
//
// fps_mem_kernel (sampling.hip) streams all n points and running distances, 20 B per point, through the one CU that owns the cloud in
// every one of its m - 1 dependent rounds.  Here a pre-pass orders the cloud along a Morton curve and cuts it into cells of S
// consecutive sorted positions; a round then touches only the cells whose bounding box is not farther from the new sample than the
// cell's largest running distance (the test of fps_wave.hip, there per wave of a register-resident cloud).  On a surface a sample
// reaches about pi n / j points after j samples, so all rounds together update about n pi ln m points instead of n m.
//
//   pre-pass, device-wide over the whole packed batch (ordering by kernel boundaries only, no kernel waits on another workgroup):
//     bounds   per segment: bounding box and non-finite flag (integer atomics on order-preserving keys: order-free, deterministic)
//     keys     key = segment id << 30 | 30-bit Morton code in the segment's box (cubic voxels, edge = largest extent / 1024; a zero
//              extent gives code 0 on every point: no division by it), value = global point index
//     sort     ONE dispu_radix_sort_pairs over the batch: stable, so equal keys keep ascending index; a segment's sorted positions
//              are its own range [off[c], off[c + 1])
//     cells    one wave per cell: gathers (x, y, z, local index) into sorted order, sets the running distances to 1e38, and writes
//              the cell's box, largest running distance (1e38) and candidate (the point of best tie priority)
//   sampling, one workgroup of 16 waves per segment; per round:
//     * thread t owns the cells {it * 1024 + lane * 16 + wave}: consecutive cells - neighbours in space - sit on different waves.
//       Their tables (box, largest distance, candidate's tie key: 8 words) live in LDS slot it * 1024 + t, touched by that thread only;
//     * every lane tests its cells' boxes; the ballot of reached cells drives a wave-uniform loop in which the whole wave does the
//       dense update of one cell (sqdist3<FMA>, min, 64-bit key max), the owner lane stores the cell's new largest distance and key;
//     * skipped cells keep their cached candidate; the winner is the maximum of (distance bits << 32 | tie key) over all cells: the
//       reference's order (larger distance, then smaller k mod 512, then smaller k; oracle/dispu_oracle.c:103-137) arithmetically,
//       so the result does not depend on the sort, the cell size or the thread layout.
//
// Why a skip is sound: for a point p of the cell and the sample s, lo <= p <= hi per axis, and rounding is monotone, so
// fl(lo - s) <= fl(p - s) <= fl(hi - s): |fl(p - s)| >= e := max(fl(lo - s), fl(s - hi), 0) holds IN floating point.  The box distance is
// sqdist3<FMA>(ex, ey, ez) - the same operations in the same order as the point distance - and every one of them (product of
// non-negatives, sum, fma) is monotone in its non-negative arguments, so lb <= d(p, s) bit for bit.  lb > largest running distance then
// gives min(td, d) == td for every point of the cell.  This argument is the one relied on; the factor 0.99999 on lb (fps_wave.hip) is
// kept as a reserve only.
//
// One level of boxes: at most kFpcMaxCells = 4096 cells per segment (128 KB of LDS), S = 64 up to 262144 points and doubling above,
// S = 4096 at the largest served segment of 2^24 points (12 * 2^20 merged points is what tools/upsample.py --max-points produces).
#include "common.h"

extern "C" size_t dispu_radix_sort_scratch_bytes(long long n);
extern "C" int dispu_radix_sort_pairs(long long n, int bits, const unsigned long long* keys_in, const unsigned int* vals_in,
                                      unsigned long long* keys_out, unsigned int* vals_out, void* scratch, size_t scratch_bytes, void* stream);

namespace dispu {

constexpr int kFpcThreads = 1024, kFpcWaves = kFpcThreads / kWave;
constexpr int kFpcMinCell = 64, kFpcMaxCell = 4096, kFpcMaxCells = 4096;
constexpr int kFpcMaxN = kFpcMaxCell * kFpcMaxCells;          // 2^24 points per segment
constexpr int kFpcPre = 256, kFpcChunk = kFpcPre * 16;        // pre-pass: 256 threads, 4096 points per workgroup
constexpr int kFpcMortonBits = 30;
static_assert(kFpcWaves == 16, "cell <-> (lane, wave) mapping");

// cell size of a segment of n points: the smallest power of two >= 64 that gives at most 4096 cells, or `cell` when that is larger
__host__ __device__ __forceinline__ int fpc_cell_size(int n, int cell) {
    int s = kFpcMinCell;
    while ((n + s - 1) / s > kFpcMaxCells) s <<= 1;
    return s > cell ? s : cell;
}
// first cell of segment c in the cell table: every segment has at most n_c / 64 + 1 cells
__device__ __forceinline__ size_t fpc_cell_base(size_t base, int c) { return base / kFpcMinCell + (size_t)c; }
// mode 0: every segment; 1: the segments dispu_fps_segments_auto sends here (family 3); 2: every segment, in cells of exactly
// kFpcMinCell points whatever its size (the pre-pass alone, for normals.hip: one query per lane of a wave)
__host__ __device__ __forceinline__ bool fpc_served(int n, int m, int mode) { return mode != 1 || fps_cells_rule(n, m); }
__host__ __device__ __forceinline__ int fpc_cell_size_mode(int n, int cell, int mode) {
    return mode == 2 ? kFpcMinCell : fpc_cell_size(n, cell);
}

__device__ __forceinline__ uint32_t fpc_tiekey(int k) {       // same key as sampling.hip:fps_tiekey
    return 0xFFFFFFFFu - ((((uint32_t)k & 511u) << 22) | ((uint32_t)k >> 9));
}
__device__ __forceinline__ int fpc_key_to_index(uint32_t key) {
    const uint32_t t = 0xFFFFFFFFu - key;
    return (int)(((t & 0x3FFFFFu) << 9) | (t >> 22));
}
__device__ __forceinline__ uint32_t fpc_spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// segb[c][8]: ~ordered(min) x3, ordered(max) x3, non-finite flag, unused; zero-filled before (the identity of atomicMax / atomicOr)
__global__ __launch_bounds__(kFpcPre) void fpc_bounds_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                             const int* __restrict__ moff, uint32_t* __restrict__ segb, int mode) {
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
                                                           unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, int mode) {
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
                                                            float* __restrict__ td, float* __restrict__ tab, int cell, int mode) {
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
        const uint32_t key = fpc_tiekey(k);
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

// LDS: tabl[8][KL] words (KL = 1024 * ceil(K / 1024)), slot it * 1024 + tid <-> cell it * 1024 + lane * 16 + wave
template <bool FMA>
__global__ __launch_bounds__(kFpcThreads) void fps_cells_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                                const int* __restrict__ moff, const uint32_t* __restrict__ segb,
                                                                const float4* __restrict__ spt, float* __restrict__ td,
                                                                const float* __restrict__ tab, int* __restrict__ out,
                                                                int* __restrict__ status, int cell, int mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tabl = reinterpret_cast<float*>(smem);
    __shared__ uint64_t slot[2][kFpcWaves];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const SegExt e = seg_ext(off, moff, c, 0, 0);
    if (!fpc_served(e.n, e.m, mode)) return;
    const uint32_t bad = segb[(size_t)c * 8 + 6];
    if (tid == 0) status[c] = bad ? 1 : 0;
    if (bad) return;                                                            // no indices for a non-finite segment
    const int n = e.n, m = e.m;
    const int S = fpc_cell_size(n, cell), K = (n + S - 1) / S, its = (K + kFpcThreads - 1) / kFpcThreads, KL = its * kFpcThreads;
    const float* __restrict__ p = xyz + e.base * 3;
    const float4* __restrict__ sp = spt + e.base;
    float* __restrict__ t = td + e.base;
    int* __restrict__ o = out + e.obase;
    const float* __restrict__ gt = tab + fpc_cell_base(e.base, c) * 8;
    for (int it = 0; it < its; ++it) {
        const int sl = it * kFpcThreads + tid, cl = it * kFpcThreads + lane * kFpcWaves + wave;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = make_float4(0.f, 0.f, -1.0f, 0.f);       // no cell: -1 is never reached
        if (cl < K) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)cl * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)cl * 8 + 4);
        }
        tabl[0 * KL + sl] = a.x; tabl[1 * KL + sl] = a.y; tabl[2 * KL + sl] = a.z; tabl[3 * KL + sl] = a.w;
        tabl[4 * KL + sl] = b.x; tabl[5 * KL + sl] = b.y; tabl[6 * KL + sl] = b.z; tabl[7 * KL + sl] = b.w;
    }
    if (tid == 0) o[0] = 0;
    float x1 = p[0], y1 = p[1], z1 = p[2];                                     // sample 0 is point 0 (tf_sampling_g.cu:122-124)
    for (int j = 1; j < m; ++j) {
        uint64_t best = 0ull;
        for (int it = 0; it < its; ++it) {
            const int sl = it * kFpcThreads + tid;
            const float ex = fmaxf(fmaxf(tabl[0 * KL + sl] - x1, x1 - tabl[3 * KL + sl]), 0.f);
            const float ey = fmaxf(fmaxf(tabl[1 * KL + sl] - y1, y1 - tabl[4 * KL + sl]), 0.f);
            const float ez = fmaxf(fmaxf(tabl[2 * KL + sl] - z1, z1 - tabl[5 * KL + sl]), 0.f);
            const float lb = sqdist3<FMA>(ex, ey, ez);
            unsigned long long reach = __ballot(lb * 0.99999f <= tabl[6 * KL + sl]);
            while (reach) {                                                     // wave-uniform: the whole wave updates one cell
                const int bl = (int)__builtin_ctzll(reach);
                reach &= reach - 1;
                const int pb = (it * kFpcThreads + bl * kFpcWaves + wave) * S, cnt = min(S, n - pb);
                uint64_t bk = 0ull;
#pragma unroll 4
                for (int i = lane; i < cnt; i += kWave) {
                    const float4 q = sp[pb + i];
                    const float t0 = t[pb + i];
                    const float d = sqdist3<FMA>(q.x - x1, q.y - y1, q.z - z1);
                    const float t1 = fminf(d, t0);
                    if (t1 != t0) t[pb + i] = t1;
                    const uint64_t key = ((uint64_t)__float_as_uint(t1) << 32) | fpc_tiekey(__float_as_int(q.w));
                    bk = key > bk ? key : bk;
                }
                bk = wave_max_u64(bk);
                if (lane == bl) {
                    tabl[6 * KL + sl] = __uint_as_float((uint32_t)(bk >> 32));
                    tabl[7 * KL + sl] = __uint_as_float((uint32_t)bk);
                }
            }
            const float md = tabl[6 * KL + sl];
            const uint64_t key = ((uint64_t)__float_as_uint(md) << 32) | __float_as_uint(tabl[7 * KL + sl]);
            if (md >= 0.f && key > best) best = key;                            // running distances are >= 0: their bits order like them
        }
        best = wave_max_u64(best);
        const int par = j & 1;
        if (lane == 0) slot[par][wave] = best;
        __syncthreads();
        best = wave_max_u64(lane < kFpcWaves ? slot[par][lane] : 0ull);
        const int k = __builtin_amdgcn_readfirstlane(fpc_key_to_index((uint32_t)best));
        if (tid == 0) o[j] = k;
        x1 = p[(size_t)k * 3 + 0]; y1 = p[(size_t)k * 3 + 1]; z1 = p[(size_t)k * 3 + 2];
    }
}

static inline size_t fpc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the sorter's key / value buffers die with the sort: the sorted points reuse both key buffers, the running distances the input values
struct FpcScratch {
    size_t kin, kout, vin, vout, sort, sort_bytes, tab, segb, total;
};
static FpcScratch fpc_scratch(size_t N, int C) {
    FpcScratch s;
    size_t o = 0;
    s.kin = o;  o += fpc_align(8 * N);
    s.kout = o; o += fpc_align(8 * N);
    s.vin = o;  o += fpc_align(4 * N);
    s.vout = o; o += fpc_align(4 * N);
    s.sort_bytes = dispu_radix_sort_scratch_bytes((long long)N);
    s.sort = o; o += fpc_align(s.sort_bytes);
    s.tab = o;  o += fpc_align(32 * (N / kFpcMinCell + (size_t)C));
    s.segb = o; o += fpc_align(32 * (size_t)C);
    s.total = o;
    return s;
}

static bool fpc_cell_ok(int cell) {
    return cell == 0 || (cell >= kFpcMinCell && cell <= kFpcMaxCell && (cell & (cell - 1)) == 0);
}

// -> 0 and: the largest segment, the largest served segment, the largest cell count of a served segment; or hipErrorInvalidValue
static int fpc_plan(int C, const int* off_host, const int* moff_host, int cell, int mode, int* nall, int* nserved, int* kmax) {
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

size_t fps_cells_scratch(int C, const int* off_host, const int* moff_host, int cell, int mode) {
    int nall, nserved, kmax;
    if (fpc_plan(C, off_host, moff_host, cell, mode, &nall, &nserved, &kmax) != 0) return 0;
    if (!nserved) return 0;
    return fpc_scratch((size_t)off_host[C], C).total;
}

// The pre-pass alone: bounds, keys, sort, cells.  scratch as fpc_scratch(off_host[C], C) lays it out; afterwards spt (over the two key
// buffers), td (over the input values), tab and segb hold what the kernels above describe.  nall / nserved / kmax from fpc_plan.
static int fpc_prepass(int C, const int* off, const int* moff, const float* inp, char* base, const FpcScratch& s, size_t N, int nall,
                       int nserved, int kmax, int cell, int mode, hipStream_t st) {
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

// The pre-pass for another kernel family (normals.hip): every segment of the packed batch in cells of exactly 64 sorted points (cell j
// of segment c: sorted positions off[c] + 64 j ...).  -> spt [N] (x, y, z, local index as bits) in sorted order, tab [.][8] the cells'
// boxes (lo x3, hi x3, -, -; segment c's first row is off[c] / 64 + c), segb [C][8] (word 6: the non-finite flag; such a segment has no
// cells), kmax the largest cell count of a segment.  The scratch is refused, untouched, when NULL, misaligned or too small.
size_t fps_cells_prepass_scratch(int C, const int* off_host) {
    int nall, nserved, kmax;
    if (fpc_plan(C, off_host, off_host, 0, 2, &nall, &nserved, &kmax) != 0) return 0;
    return fpc_scratch((size_t)off_host[C], C).total;
}
int fps_cells_prepass(int C, const int* off, const int* off_host, const float* inp, void* scratch, size_t scratch_bytes,
                      const float4** spt, const float** tab, const uint32_t** segb, int* kmax, hipStream_t st) {
    int nall, nserved;
    const int rc = fpc_plan(C, off_host, off_host, 0, 2, &nall, &nserved, kmax);
    if (rc != 0) return rc;
    if (!off || !inp) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)off_host[C];
    const FpcScratch s = fpc_scratch(N, C);
    if (!scratch || scratch_bytes < s.total || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    char* base = (char*)scratch;
    *spt = (const float4*)(base + s.kin);
    *tab = (const float*)(base + s.tab);
    *segb = (const uint32_t*)(base + s.segb);
    return fpc_prepass(C, off, off, inp, base, s, N, nall, nserved, *kmax, 0, 2, st);
}

int fps_cells_run(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* scratch,
                  size_t scratch_bytes, int* out, int* status, int arith, int cell, int mode, hipStream_t st) {
    int nall, nserved, kmax;
    const int rc = fpc_plan(C, off_host, moff_host, cell, mode, &nall, &nserved, &kmax);
    if (rc != 0) return rc;
    if (!nserved) return 0;
    if (!off || !moff || !inp || !out || !status) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)off_host[C];
    const FpcScratch s = fpc_scratch(N, C);
    if (!scratch || scratch_bytes < s.total || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
    char* base = (char*)scratch;
    const uint32_t* segb = (const uint32_t*)(base + s.segb);
    const float* tab = (const float*)(base + s.tab);
    const float4* spt = (const float4*)(base + s.kin);
    float* td = (float*)(base + s.vin);
    const int rp = fpc_prepass(C, off, moff, inp, base, s, N, nall, nserved, kmax, cell, mode, st);
    if (rp != 0) return rp;
    const size_t lds = (size_t)8 * 4 * kFpcThreads * ((kmax + kFpcThreads - 1) / kFpcThreads);
    static DevOnce attr;
    if (attr.needed()) {
        const int cap = 8 * 4 * kFpcMaxCells;
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fps_cells_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fps_cells_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        attr.done();
    }
    if ((arith & DISPU_ARITH_CONTRACT))
        hipLaunchKernelGGL((fps_cells_kernel<true>), dim3(C), dim3(kFpcThreads), lds, st, inp, off, moff, segb, spt, td, tab, out, status, cell,
                           mode);
    else
        hipLaunchKernelGGL((fps_cells_kernel<false>), dim3(C), dim3(kFpcThreads), lds, st, inp, off, moff, segb, spt, td, tab, out, status, cell,
                           mode);
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_fps_cells_wanted(int n, int m) { return fps_cells_rule(n, m) ? 1 : 0; }

DISPU_EXPORT size_t dispu_fps_cells_scratch_bytes(int C, const int* off_host, const int* moff_host, int cell) {
    return fps_cells_scratch(C, off_host, moff_host, cell, 0);
}

DISPU_EXPORT int dispu_fps_cells(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp,
                                 void* scratch, size_t scratch_bytes, int* out, int* status, int arith, int cell, void* stream) {
    if (C < 0) return (int)hipErrorInvalidValue;
    if (C == 0) return 0;
    return fps_cells_run(C, off, moff, off_host, moff_host, inp, scratch, scratch_bytes, out, status, arith, cell, 0, (hipStream_t)stream);
}
