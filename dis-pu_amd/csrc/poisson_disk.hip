// Poisson-disk (blue-noise) selection by greedy dart throwing, in parallel, with an exact count (gfx950).  No reference counterpart
// (the reference's training patches and test clouds were Poisson-disk sampled upstream); the yardstick is the sequential restatement
// in tests/mesh_sample_oracle.py, reproduced exactly.
//
// Semantics (sequential): keep[i] = 1 iff there is no j < i with keep[j] and d2(p_i, p_j) < fl32(r r), d2 in the DISPU_ARITH_PLAIN
// order ((dx dx + dy dy) + dz dz, fp32), the comparison strict; r <= 0 keeps everything.  That set is the lexicographically first
// maximal independent set of the conflict graph, which the rounds below compute: every point is ACTIVE, KEPT or REJECTED; in a round an
// active point looks at its conflicting neighbours of lower index and becomes REJECTED if one of them is KEPT, KEPT if all of them are
// REJECTED, and stays ACTIVE otherwise.  A decision is taken from final states only and a state never changes twice, so the in-place,
// unsynchronised updates inside a round change how many rounds are needed, not the result.  The lowest active index settles in every
// round; typical clouds need 7 - 10 rounds, the loop is bounded by DISPU_POISSON_MAX_ROUNDS and reports through status.
//
// One workgroup of 1024 threads per cloud.  Neighbours come from a uniform grid of 32^3 cells over the cloud's bounding box with cell
// side max(r, extent / 32) (1 + 2^-10): at least the radius, so that conflicts lie in the 27 surrounding cells (the 2^-10 margin is far
// above the rounding of the cell coordinate, a few 2^-23 of at most 32), and capped in number, so that an outlier cannot blow it up.
// It is built once per call by a counting sort: counts by LDS integer atomics (two 16-bit counters per word: n < 65536), an in-place
// exclusive scan, a scatter of (x, y, z, index) into the scratch.  The order inside a cell is whatever the atomics give and does not
// affect any output.  x is the fastest cell axis: the three x-neighbours of a row are ONE contiguous range of the sorted cloud, so a
// point scans 9 ranges.  LDS holds the cell offsets (64 KB), one state byte per point and the bitmap of the final selection; the sorted
// cloud stays in global memory (16 n bytes, L2-resident).
//
// select: the bisection of the radius runs inside the kernel (lo = 0, hi = r_hi; steps times mid = 0.5f (lo + hi), count(mid) >= m ?
// lo = mid : hi = mid, all fp32), then the set at lo is evaluated once more and its first m members are emitted in ascending index
// order (bitmap + workgroup prefix sum).  Every radius tried is <= r_hi, so the one grid serves them all.  No host readback anywhere.
// No float atomics; integer atomics only where the order cannot matter.
#include "common.h"

namespace dispu {

constexpr int PD_BS = 1024;
constexpr int PD_G = 32;
constexpr int PD_CELLS = PD_G * PD_G * PD_G;
constexpr int PD_MISC = 32;                      // words in front of the cell table
constexpr uint8_t PD_ACTIVE = 0, PD_KEPT = 1, PD_REJECTED = 2;
// misc words
constexpr int PD_LO = 0, PD_HI = 3, PD_FLAG = 6, PD_COUNT = 7, PD_WTOT = 8;   // [8, 24): one total per wave

__host__ __device__ constexpr size_t pd_round16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t pd_lds_bytes(int n) {
    return (size_t)PD_MISC * 4 + (size_t)PD_CELLS * 2 + pd_round16((size_t)n) + pd_round16((size_t)((n + 31) >> 5) * 4);
}
static_assert(pd_lds_bytes(DISPU_POISSON_MAX_N) <= 160 * 1024, "the largest cloud must fit the 160 KB of LDS of a CU");
static_assert(DISPU_POISSON_MAX_N < 65536, "cell offsets are 16-bit");

// exclusive prefix sum of v over the workgroup (thread order); total = the sum over all threads.  Two barriers.
__device__ __forceinline__ int pd_block_scan(int v, volatile uint32_t* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wave] = (uint32_t)inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < PD_BS / 64; ++q) {
        const int t = (int)wtot[q];
        if (q < wave) base += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

struct PdGrid {
    float lox, loy, loz, inv;
};

__device__ __forceinline__ int pd_cell1(float x, float lo, float inv) {
    return (int)fminf(fmaxf((x - lo) * inv, 0.0f), (float)(PD_G - 1));       // NaN -> 0; always inside the grid
}

// 16-bit cell table after the scatter: half c holds the END of cell c in the sorted cloud
__device__ __forceinline__ int pd_end(const uint32_t* cells, int c) { return (int)((cells[c >> 1] >> ((c & 1) * 16)) & 0xFFFFu); }
__device__ __forceinline__ int pd_start(const uint32_t* cells, int c) { return c ? pd_end(cells, c - 1) : 0; }

// One evaluation of the keep flags at radius r: leaves them in state[] (by sorted position) and returns their number (workgroup-uniform).
// capped is set when the round limit was hit.
__device__ __forceinline__ int pd_eval(int n, float r, const float4* sorted, const uint32_t* cells, volatile uint8_t* state,
                       volatile uint32_t* misc, const PdGrid& g, int& capped) {
    const int tid = threadIdx.x;
    if (!(r > 0.0f)) {                                                       // uniform: r comes from workgroup-uniform values
        for (int s = tid; s < n; s += PD_BS) state[s] = PD_KEPT;
        __syncthreads();
        return n;
    }
    const float r2 = r * r;
    for (int s = tid; s < n; s += PD_BS) state[s] = PD_ACTIVE;
    __syncthreads();
    for (int round = 0;; ++round) {
        if (round == DISPU_POISSON_MAX_ROUNDS) { capped = 1; break; }        // uniform
        if (tid == 0) misc[PD_FLAG] = 0;
        __syncthreads();
        bool left = false;
        for (int s = tid; s < n; s += PD_BS) {
            if (state[s] != PD_ACTIVE) continue;
            const float4 me = sorted[s];
            const int i = __float_as_int(me.w);
            const int cx = pd_cell1(me.x, g.lox, g.inv), cy = pd_cell1(me.y, g.loy, g.inv), cz = pd_cell1(me.z, g.loz, g.inv);
            const int x0 = max(cx - 1, 0), x1 = min(cx + 1, PD_G - 1);
            bool pending = false, rejected = false;
            for (int zz = max(cz - 1, 0); zz <= min(cz + 1, PD_G - 1) && !rejected; ++zz) {
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, PD_G - 1) && !rejected; ++yy) {
                    const int row = (zz * PD_G + yy) * PD_G;
                    const int e = pd_end(cells, row + x1);
                    for (int t = pd_start(cells, row + x0); t < e; ++t) {
                        const float4 q = sorted[t];
                        if (__float_as_int(q.w) < i && sqdist3<false>(me.x - q.x, me.y - q.y, me.z - q.z) < r2) {
                            const uint8_t st = state[t];
                            if (st == PD_KEPT) { rejected = true; break; }
                            if (st == PD_ACTIVE) pending = true;
                        }
                    }
                }
            }
            if (rejected) state[s] = PD_REJECTED;
            else if (!pending) state[s] = PD_KEPT;
            else left = true;
        }
        if (left) misc[PD_FLAG] = 1;
        __syncthreads();
        const uint32_t more = misc[PD_FLAG];
        __syncthreads();
        if (!more) break;
    }
    if (tid == 0) misc[PD_COUNT] = 0;
    __syncthreads();
    int mine = 0;
    for (int s = tid; s < n; s += PD_BS) mine += state[s] == PD_KEPT;
    if (mine) atomicAdd((uint32_t*)&misc[PD_COUNT], (uint32_t)mine);
    __syncthreads();
    const int c = (int)misc[PD_COUNT];
    __syncthreads();
    return c;
}

template <bool SELECT>
__global__ __launch_bounds__(PD_BS) void poisson_disk_kernel(int n, int m, int steps, const float* __restrict__ points,
                                                             const float* __restrict__ radius, uint8_t* __restrict__ keep,
                                                             int* __restrict__ count_out, int* __restrict__ idx, float* __restrict__ r_out,
                                                             float4* __restrict__ scratch, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pd_smem[];
    volatile uint32_t* misc = pd_smem;
    uint32_t* cells = pd_smem + PD_MISC;                                     // PD_CELLS / 2 words
    volatile uint8_t* state = reinterpret_cast<volatile uint8_t*>(cells + PD_CELLS / 2);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(state) + pd_round16((size_t)n));
    const int tid = threadIdx.x, cloud = blockIdx.x;
    const float* __restrict__ p = points + (size_t)cloud * n * 3;
    float4* __restrict__ sorted = scratch + (size_t)cloud * n;
    const float r_top = radius[cloud];

    // ---- bounding box (ordered-integer min / max: order-free) ----
    if (tid < 3) { misc[PD_LO + tid] = 0xFFFFFFFFu; misc[PD_HI + tid] = 0u; }
    for (int w = tid; w < PD_CELLS / 2; w += PD_BS) cells[w] = 0u;
    __syncthreads();
    {
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        for (int i = tid; i < n; i += PD_BS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = p[(size_t)i * 3 + c];
                lo[c] = fminf(lo[c], v);
                hi[c] = fmaxf(hi[c], v);
            }
        }
        if (tid < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMin((uint32_t*)&misc[PD_LO + c], f32_to_ordered(lo[c]));
                atomicMax((uint32_t*)&misc[PD_HI + c], f32_to_ordered(hi[c]));
            }
        }
    }
    __syncthreads();
    PdGrid g;
    g.lox = ordered_to_f32(misc[PD_LO + 0]); g.loy = ordered_to_f32(misc[PD_LO + 1]); g.loz = ordered_to_f32(misc[PD_LO + 2]);
    {
        const float ex = ordered_to_f32(misc[PD_HI + 0]) - g.lox, ey = ordered_to_f32(misc[PD_HI + 1]) - g.loy,
                    ez = ordered_to_f32(misc[PD_HI + 2]) - g.loz;
        float side = fmaxf(fmaxf(ex, ey), ez) * (1.0f / PD_G);
        if (r_top > side) side = r_top;
        if (!(side > 0.0f)) side = 1.0f;                                     // one point, or all identical with r <= 0
        side *= 1.0009765625f;                                               // 1 + 2^-10
        g.inv = 1.0f / side;
    }
    auto cell_of = [&](float x, float y, float z) {
        return (pd_cell1(z, g.loz, g.inv) * PD_G + pd_cell1(y, g.loy, g.inv)) * PD_G + pd_cell1(x, g.lox, g.inv);
    };

    // ---- counting sort by cell ----
    for (int i = tid; i < n; i += PD_BS) {
        const int c = cell_of(p[(size_t)i * 3 + 0], p[(size_t)i * 3 + 1], p[(size_t)i * 3 + 2]);
        atomicAdd(&cells[c >> 1], 1u << ((c & 1) * 16));
    }
    __syncthreads();
    {
        constexpr int WPT = PD_CELLS / 2 / PD_BS;                            // 16 words = 32 cells per thread
        uint32_t w[WPT];
        int sum = 0;
#pragma unroll
        for (int k = 0; k < WPT; ++k) {
            w[k] = cells[tid * WPT + k];
            sum += (int)(w[k] & 0xFFFFu) + (int)(w[k] >> 16);
        }
        int total;
        int run = pd_block_scan(sum, misc + PD_WTOT, total);
#pragma unroll
        for (int k = 0; k < WPT; ++k) {
            const int c0 = (int)(w[k] & 0xFFFFu), c1 = (int)(w[k] >> 16);
            cells[tid * WPT + k] = (uint32_t)run | ((uint32_t)(run + c0) << 16);   // starts; the scatter turns them into ends
            run += c0 + c1;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += PD_BS) {
        const float x = p[(size_t)i * 3 + 0], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2];
        const int c = cell_of(x, y, z);
        const uint32_t old = atomicAdd(&cells[c >> 1], 1u << ((c & 1) * 16));
        const int pos = (int)((old >> ((c & 1) * 16)) & 0xFFFFu);
        if (pos < n) sorted[pos] = make_float4(x, y, z, __int_as_float(i));
    }
    __threadfence_block();
    __syncthreads();

    int capped = 0;
    if constexpr (!SELECT) {
        const int c = pd_eval(n, r_top, sorted, cells, state, misc, g, capped);
        for (int s = tid; s < n; s += PD_BS) {
            const int i = __float_as_int(sorted[s].w);
            if ((unsigned)i < (unsigned)n) keep[(size_t)cloud * n + i] = state[s] == PD_KEPT ? 1 : 0;
        }
        if (tid == 0) { count_out[cloud] = c; status[cloud] = capped; }
    } else {
        float lo = 0.0f, hi = r_top;
        int c = 0;
        for (int k = 0; k <= steps; ++k) {                                   // the last pass evaluates the set at lo itself
            const bool last = k == steps;
            const float r = last ? lo : 0.5f * (lo + hi);
            c = pd_eval(n, r, sorted, cells, state, misc, g, capped);
            if (!last) { if (c >= m) lo = r; else hi = r; }
        }
        const int nw = (n + 31) >> 5;
        for (int w = tid; w < nw; w += PD_BS) bitmap[w] = 0u;
        __syncthreads();
        for (int s = tid; s < n; s += PD_BS) {
            if (state[s] != PD_KEPT) continue;
            const int i = __float_as_int(sorted[s].w);
            if ((unsigned)i < (unsigned)n) atomicOr(&bitmap[i >> 5], 1u << (i & 31));
        }
        __syncthreads();
        const int per = (nw + PD_BS - 1) / PD_BS;
        const int w0 = min(tid * per, nw), w1 = min(w0 + per, nw);
        int cnt = 0;
        for (int w = w0; w < w1; ++w) cnt += __popc(bitmap[w]);
        int total;
        int pos = pd_block_scan(cnt, misc + PD_WTOT, total);
        for (int w = w0; w < w1 && pos < m; ++w)
            for (uint32_t rest = bitmap[w]; rest && pos < m; rest &= rest - 1u) idx[(size_t)cloud * m + pos++] = w * 32 + (__ffs(rest) - 1);
        if (tid == 0) { count_out[cloud] = c; r_out[cloud] = lo; status[cloud] = capped | (total < m ? 2 : 0); }
    }
}

// ---- rows of int32 ascending, in place: one workgroup per row, bitonic network in LDS over the next power of two ----
constexpr int SORT_BS = 256;
constexpr int SORT_MAX_K = 4096;
__global__ __launch_bounds__(SORT_BS) void sort_rows_i32_kernel(int k, int* __restrict__ idx) {
    __shared__ int v[SORT_MAX_K];
    int* __restrict__ row = idx + (size_t)blockIdx.x * k;
    int P = 1;
    while (P < k) P <<= 1;
    for (int e = threadIdx.x; e < P; e += SORT_BS) v[e] = e < k ? row[e] : 0x7FFFFFFF;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += SORT_BS) {
                const int a = ((t / stride) * stride << 1) + (t % stride), b = a + stride;
                const bool up = (a & size) == 0;
                const int x = v[a], y = v[b];
                if ((x > y) == up) { v[a] = y; v[b] = x; }
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < k; e += SORT_BS) row[e] = v[e];
}

template <bool SELECT>
static int pd_launch(int b, int n, int m, int steps, const float* points, const float* radius, uint8_t* keep, int* count, int* idx,
                     float* r_out, void* scratch, int* status, hipStream_t st) {
    const size_t lds = pd_lds_bytes(n);
    static DevOnce attr;       // opt in to > 64 KB of dynamic LDS, once per device
    if (attr.needed()) {
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(poisson_disk_kernel<SELECT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)pd_lds_bytes(DISPU_POISSON_MAX_N)));
        attr.done();
    }
    hipLaunchKernelGGL(poisson_disk_kernel<SELECT>, dim3((unsigned)b), dim3(PD_BS), lds, st, n, m, steps, points, radius, keep, count, idx,
                       r_out, static_cast<float4*>(scratch), status);
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_poisson_disk_scratch_bytes(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return (size_t)b * (size_t)n * sizeof(float4);
}

DISPU_EXPORT int dispu_poisson_disk_keep(int b, int n, const float* points, const float* radius, unsigned char* keep, int* count,
                                         void* scratch, size_t scratch_bytes, int* status, void* stream) {
    if (b < 0 || n <= 0 || n > DISPU_POISSON_MAX_N || !points || !radius || !keep || !count || !status) return (int)hipErrorInvalidValue;
    if (b == 0) return 0;
    if (!scratch_ok(scratch, scratch_bytes, dispu_poisson_disk_scratch_bytes(b, n))) return (int)hipErrorInvalidValue;
    return pd_launch<false>(b, n, 0, 0, points, radius, keep, count, nullptr, nullptr, scratch, status, (hipStream_t)stream);
}

DISPU_EXPORT int dispu_poisson_disk_select(int b, int n, int m, int steps, const float* points, const float* r_hi, int* idx, float* r_out,
                                           int* count_out, void* scratch, size_t scratch_bytes, int* status, void* stream) {
    if (b < 0 || n <= 0 || n > DISPU_POISSON_MAX_N || m <= 0 || m > n || steps < 0 || !points || !r_hi || !idx || !r_out || !count_out ||
        !status)
        return (int)hipErrorInvalidValue;
    if (b == 0) return 0;
    if (!scratch_ok(scratch, scratch_bytes, dispu_poisson_disk_scratch_bytes(b, n))) return (int)hipErrorInvalidValue;
    return pd_launch<true>(b, n, m, steps, points, r_hi, nullptr, count_out, idx, r_out, scratch, status, (hipStream_t)stream);
}

DISPU_EXPORT int dispu_sort_rows_i32(int b, int k, int* idx, void* stream) {
    if (b < 0 || k <= 0 || k > SORT_MAX_K || !idx) return (int)hipErrorInvalidValue;
    if (b == 0) return 0;
    hipLaunchKernelGGL(sort_rows_i32_kernel, dim3((unsigned)b), dim3(SORT_BS), 0, (hipStream_t)stream, k, idx);
    return (int)hipGetLastError();
}
