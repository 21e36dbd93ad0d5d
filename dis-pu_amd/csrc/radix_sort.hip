// Device-wide stable LSD radix sort of (uint64 key, uint32 value) pairs, the three-step exclusive scan it is built on, and the run
// numbering that follows a sort: behind dispu_radix_sort_pairs (include/dispu_hip.h), and through internal.h (RadixSorter,
// exclusive_scan_u32, run_heads_scan) under grid_subsample.hip (voxel keys, label keys), poisson_disk_cells.hip (cell keys) and
// reconstruct.hip (lattice keys); morton_cells.hip (Morton keys) calls the exported entry.  Stable: equal keys keep their input order,
// which is what every client's determinism rests on.
//
//   8 bits per pass, ceil(bits / 8) passes, ping-pong buffers; per pass:
//     histogram   256 bins per tile of kRsTile elements in LDS (integer LDS atomics: counts are order-free)
//     scan        exclusive scan of the digit-major table [256][tiles]
//     scatter     stable rank inside the tile: lanes of equal digit found by ballots, ranked by lane; waves prefixed in wave
//                 order; wave w owns the contiguous elements [w 512, (w + 1) 512) of the tile, so rank order = index order
//
// Cross-workgroup ordering is by kernel boundaries only: no kernel waits on anything another workgroup writes.  The device-wide scans
// are the plain three-step kind (tile sums, scan of sums, apply).  No float atomics anywhere: two runs give identical bytes.
#include "internal.h"

namespace dispu {

constexpr int kRsItems = 8;                          // elements per thread
constexpr int kRsTile = kRsThreads * kRsItems;       // 2048
constexpr int kRsWaveSpan = kWave * kRsItems;        // 512 contiguous elements per wave
static_assert(kRsTile == DISPU_RADIX_TILE, "the tile the public header documents");

// ---- block helpers (256 threads) ---------------------------------------------------------------------------------------------------
// exclusive prefix of one value per thread in thread order, and the block total; wsum: kRsWaves words of LDS, reusable on return
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += t;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kRsWaves; ++i) {
        const uint32_t s = wsum[i];
        if (i < w) off += s;
        total += s;
    }
    __syncthreads();
    return off + inc - v;
}

// ---- device-wide exclusive scan of uint32 data[L], in place: reduce -> sums -> apply; chunks of kRsTile ------------------------------
__global__ __launch_bounds__(kRsThreads) void scan_reduce_kernel(const uint32_t* __restrict__ data, size_t L, uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[kRsWaves];
    const size_t base = (size_t)blockIdx.x * kRsTile + (size_t)threadIdx.x * kRsItems;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kRsItems; ++k)
        if (base + k < L) s += data[base + k];
    uint32_t total;
    (void)block_excl_scan(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[nb] -> their exclusive prefixes, in place; the grand total -> *total_out (if not null)
__global__ __launch_bounds__(kRsThreads) void scan_sums_kernel(uint32_t* __restrict__ sums, unsigned nb, uint32_t* __restrict__ total_out) {
    __shared__ uint32_t wsum[kRsWaves];
    const unsigned per = (nb + kRsThreads - 1) / kRsThreads;
    const unsigned lo = min(threadIdx.x * per, nb), hi = min(lo + per, nb);
    uint32_t s = 0;
    for (unsigned i = lo; i < hi; ++i) s += sums[i];
    uint32_t total;
    uint32_t run = block_excl_scan(s, wsum, total);
    for (unsigned i = lo; i < hi; ++i) {
        const uint32_t v = sums[i];
        sums[i] = run;
        run += v;
    }
    if (total_out && threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kRsThreads) void scan_apply_kernel(uint32_t* __restrict__ data, size_t L, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[kRsWaves];
    const size_t base = (size_t)blockIdx.x * kRsTile + (size_t)threadIdx.x * kRsItems;
    uint32_t v[kRsItems];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kRsItems; ++k) {
        v[k] = base + k < L ? data[base + k] : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t run = block_excl_scan(s, wsum, total) + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kRsItems; ++k) {
        if (base + k < L) data[base + k] = run;
        run += v[k];
    }
}

size_t scan_blocks(size_t L) { return (L + kRsTile - 1) / kRsTile; }

int exclusive_scan_u32(uint32_t* data, size_t L, uint32_t* sums, uint32_t* total_out, hipStream_t st) {
    const unsigned nb = (unsigned)scan_blocks(L);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kRsThreads), 0, st, data, L, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kRsThreads), 0, st, sums, nb, total_out);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kRsThreads), 0, st, data, L, sums);
    return (int)hipGetLastError();
}

// ---- radix sort ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void radix_hist_kernel(const uint64_t* __restrict__ keys, size_t n, int shift, unsigned tiles,
                                                                uint32_t* __restrict__ table) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kRsTile;
#pragma unroll
    for (int k = 0; k < kRsItems; ++k) {
        const size_t p = base + (size_t)k * kRsThreads + threadIdx.x;
        if (p < n) atomicAdd(&hist[(unsigned)(keys[p] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// table: the SCANNED digit-major table, table[d][tile] = the first output position of digit d of this tile
__global__ __launch_bounds__(kRsThreads) void radix_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                   size_t n, int shift, unsigned tiles, const uint32_t* __restrict__ table,
                                                                   uint64_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t wcount[kRsWaves][256];       // per wave: elements of each digit seen so far, at the end the wave's count
    __shared__ uint32_t wbase[kRsWaves][256];        // first output position of (wave, digit)
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < kRsWaves; ++i) wcount[i][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kRsTile + (size_t)w * kRsWaveSpan + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    volatile uint32_t* wc = wcount[w];               // this wave's row: read by all its lanes, then written by the digit leaders, in order
    uint64_t key[kRsItems];
    uint32_t val[kRsItems], rank[kRsItems];
#pragma unroll
    for (int k = 0; k < kRsItems; ++k) {
        const size_t p = base + (size_t)k * kWave;
        const bool valid = p < n;
        key[k] = valid ? keys[p] : 0ull;
        val[k] = valid ? vals[p] : 0u;
        const unsigned d = (unsigned)(key[k] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);  // the lanes that hold an element of the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t before = wc[d];
        __builtin_amdgcn_wave_barrier();
        rank[k] = before + (uint32_t)__popcll(peers & below);
        if (valid && (peers & below) == 0ull) wc[d] = before + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        uint32_t run = table[(size_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
        for (int i = 0; i < kRsWaves; ++i) {
            wbase[i][threadIdx.x] = run;
            run += wcount[i][threadIdx.x];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRsItems; ++k) {
        const size_t p = base + (size_t)k * kWave;
        if (p < n) {
            const size_t dst = (size_t)wbase[w][(unsigned)(key[k] >> shift) & 255u] + rank[k];
            if (dst < n) {                           // always true for a consistent table; keeps a wrong one from writing outside
                keys_out[dst] = key[k];
                vals_out[dst] = val[k];
            }
        }
    }
}

static inline unsigned rs_tiles(size_t n) { return (unsigned)((n + kRsTile - 1) / kRsTile); }
static size_t rs_table_words(size_t n) { return (size_t)256 * rs_tiles(n); }       // the digit-major histogram table of n pairs

// `passes` stable 8-bit passes from (src_k, src_v), which is only read, alternating into (xk, xv), (yk, yv), (xk, xv), ...: the result
// is in x when passes is odd and in y when it is even (passes >= 1)
static int radix_passes(size_t n, int passes, const uint64_t* src_k, const uint32_t* src_v, uint64_t* xk, uint32_t* xv, uint64_t* yk,
                        uint32_t* yv, uint32_t* table, uint32_t* sums, hipStream_t st) {
    const unsigned tiles = rs_tiles(n);
    const uint64_t* ck = src_k;
    const uint32_t* cv = src_v;
    for (int p = 0; p < passes; ++p) {
        uint64_t* dk = (p & 1) ? yk : xk;
        uint32_t* dv = (p & 1) ? yv : xv;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles), dim3(kRsThreads), 0, st, ck, n, 8 * p, tiles, table);
        const int rc = exclusive_scan_u32(table, rs_table_words(n), sums, nullptr, st);
        if (rc) return rc;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles), dim3(kRsThreads), 0, st, ck, cv, n, 8 * p, tiles, table, dk, dv);
        ck = dk;
        cv = dv;
    }
    return (int)hipGetLastError();
}

static void carve_table_sums(Carver& cv, size_t n, uint32_t*& table, uint32_t*& sums) {
    table = cv.ptr<uint32_t>(4 * rs_table_words(n));
    sums = cv.ptr<uint32_t>(4 * scan_blocks(rs_table_words(n) > n ? rs_table_words(n) : n));
}

void RadixSorter::carve(Carver& cv, size_t n) {
    k[0] = cv.ptr<uint64_t>(8 * n);
    k[1] = cv.ptr<uint64_t>(8 * n);
    v[0] = cv.ptr<uint32_t>(4 * n);
    v[1] = cv.ptr<uint32_t>(4 * n);
    carve_table_sums(cv, n, table, sums);
}

int RadixSorter::sort(size_t n, int passes, hipStream_t st) {
    side = passes & 1;                               // pass p reads side p & 1 and writes the other
    return passes ? radix_passes(n, passes, k[0], v[0], k[1], v[1], k[0], v[0], table, sums, st) : 0;
}

// ---- run numbering ---------------------------------------------------------------------------------------------------------------------
// keys == nullptr: all keys are equal
__global__ __launch_bounds__(kRsThreads) void run_heads_kernel(const uint64_t* __restrict__ keys, size_t n, uint32_t* __restrict__ head) {
    const size_t j = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (j < n) head[j] = (j == 0 || (keys && keys[j] != keys[j - 1])) ? 1u : 0u;
}

int run_heads_scan(const uint64_t* keys, size_t n, uint32_t* ex, uint32_t* sums, uint32_t* count, hipStream_t st) {
    hipLaunchKernelGGL(run_heads_kernel, dim3(rs_blocks(n)), dim3(kRsThreads), 0, st, keys, n, ex);
    return exclusive_scan_u32(ex, n, sums, count, st);
}

// scratch of the exported sorter: alternate keys, alternate payload, table, scan sums
struct SortScratch {
    uint64_t* keys;
    uint32_t *vals, *table, *sums;
    size_t total;
};
static SortScratch sort_scratch(size_t n, void* base = nullptr) {
    SortScratch s;
    Carver cv{(char*)base};
    s.keys = cv.ptr<uint64_t>(8 * n);
    s.vals = cv.ptr<uint32_t>(4 * n);
    carve_table_sums(cv, n, s.table, s.sums);
    s.total = cv.off;
    return s;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_radix_sort_scratch_bytes(long long n) {
    if (n <= 0 || n >= (1ll << 31)) return 0;
    return sort_scratch((size_t)n).total;
}

DISPU_EXPORT int dispu_radix_sort_pairs(long long n, int bits, const unsigned long long* keys_in, const unsigned int* vals_in,
                                        unsigned long long* keys_out, unsigned int* vals_out, void* scratch, size_t scratch_bytes,
                                        void* stream) {
    if (n < 0 || n >= (1ll << 31) || bits < 0 || bits > 64) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!keys_in || !vals_in || !keys_out || !vals_out || keys_in == keys_out || vals_in == vals_out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n;
    const int passes = (bits + 7) / 8;
    if (passes == 0) {
        DISPU_TRY(hipMemcpyAsync(keys_out, keys_in, 8 * N, hipMemcpyDeviceToDevice, st));
        DISPU_TRY(hipMemcpyAsync(vals_out, vals_in, 4 * N, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const SortScratch s = sort_scratch(N, scratch);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    uint64_t* ok = (uint64_t*)keys_out;
    uint32_t* ov = (uint32_t*)vals_out;
    const bool odd = passes & 1;                     // the result lands in x for an odd pass count, in y for an even one
    return radix_passes(N, passes, (const uint64_t*)keys_in, (const uint32_t*)vals_in, odd ? ok : s.keys, odd ? ov : s.vals,
                        odd ? s.keys : ok, odd ? s.vals : ov, s.table, s.sums, st);
}
