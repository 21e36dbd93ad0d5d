// Poisson-disk (blue-noise) selection for whole clouds: the device-wide cell tier behind dispu_poisson_cells_keep / _select (gfx950).
// The definition is the one of csrc/poisson_disk.hip, word for word, and the yardstick is the same sequential restatement in
// tests/mesh_sample_oracle.py, reproduced bit for bit; what differs is that a cloud is not held by one workgroup, so its size is not
// bounded by DISPU_POISSON_MAX_N, and that the input is a packed ragged batch (C segments in one [sum n_c, 3] array, a radius each).
//
// Semantics (sequential): keep[i] = 1 iff there is no j < i with keep[j] and d2(p_i, p_j) < fl32(r r), d2 in the DISPU_ARITH_PLAIN
// order ((dx dx + dy dy) + dz dz, fp32, no contraction), the comparison strict; r <= 0 keeps everything.
//
// Rounds.  Every point is ACTIVE, KEPT or REJECTED (one byte, stored by SORTED position).  In a round, one launch over the still-active
// points, an active point looks at its conflicting neighbours of lower index and becomes REJECTED if one of them is KEPT, KEPT if all of
// them are REJECTED, and stays ACTIVE otherwise.  The states are read and written IN PLACE while other workgroups of the same launch do
// the same, without any ordering between them.  That is safe because
//   - a state byte has ONE writer, the thread that owns the point, and changes at most ONCE, from ACTIVE to its final value;
//   - a decision is taken from FINAL values only: REJECTED needs one neighbour seen KEPT, KEPT needs every neighbour seen REJECTED;
//   - so whatever a reader sees of a neighbour is either its final value or ACTIVE -- a stale copy (another CU's L1, another XCD's L2,
//     a store still in flight) can only be ACTIVE.  ACTIVE never decides anything: it only leaves the reader ACTIVE for another round.
// A stale read therefore delays a decision and never falsifies one; by induction over the index every point ends in the state the
// sequential greedy gives it, whatever the timing, the launch shape or the packing.  Kernel boundaries make every store of a round
// visible to the next, so the lowest active index of every segment settles in every round and the loop ends; it is bounded by
// DISPU_POISSON_MAX_ROUNDS launches, after which the segments that still hold active points get bit 0 of their status word.
// The still-active points are appended to the next round's list by integer atomics (one add per wave); the order of that list differs
// from run to run and no output depends on it.  No float atomics anywhere: two runs give identical bytes.
//
// Grid.  Per segment a uniform grid over its bounding box with cell side max(r_c, extent_c / 1024) (1 + 2^-10): poisson_disk.hip's rule
// with 1024 in place of 32.  The side is at least the radius, so conflicts lie in the 27 surrounding cells (the rounding of a cell
// coordinate is below 1024 * 2^-23 = 2^-13 of a cell per point, far inside the 2^-10 margin), and it is capped in number, so an outlier
// cannot blow the grid up.  The cell key is (segment, z, y, x), x fastest, in a uint64; (key, packed index) goes through the stable
// sorter of radix_sort.hip, so indices ascend inside a cell.  The grid is sparse (1024^3 cells cannot be tabulated): the occupied cells
// are compacted (run_heads_scan of radix_sort.hip), and because x is fastest the three x-neighbours of a row are ONE contiguous range of
// the sorted cloud, so a point scans 9 ranges.  The 9 ranges are found ONCE per occupied cell by binary search over the compacted keys
// and kept as a record of 20 words per cell; every round of every radius of a bisection reads them back (DESIGN section 9 says why
// this variant and what it costs in memory).
//
// select: lo = 0, hi = r_hi; steps times mid = 0.5f (lo + hi), count(mid) >= m ? lo = mid : hi = mid, in fp32 per segment on the
// device; the set at lo is evaluated once more and its first m members are emitted in ascending index order (flags by input index, one
// exclusive scan).  Every radius tried is <= r_hi, so the one grid serves them all, and all segments share every launch.
// Host readbacks: one 4-byte word per chunk of PC_CHUNK rounds (the size of the next list; zero ends the evaluation).
#include "internal.h"
#include <float.h>

namespace dispu {

constexpr int PC_G = 1024;                           // cells per axis, at most
constexpr int PC_AXIS_BITS = 10;
constexpr int PC_CELL_BITS = 3 * PC_AXIS_BITS;       // the segment number sits above them
constexpr int PC_REC = 20;                           // words per occupied cell: 9 x (start, end), the segment, one spare
constexpr int PC_REC_SEG = 18;
constexpr int PC_CHUNK = 6;                          // rounds between two readbacks of the list size
constexpr uint8_t PC_ACTIVE = 0, PC_KEPT = 1, PC_REJECTED = 2;
constexpr int PC_BAD = DISPU_POISSON_CELLS_NONFINITE;                          // status bit 2: a non-finite coordinate or radius
// per-segment tables: segb [C][8] u32 = ordered lo x3, ordered hi x3, bad, -;  segg [C][4] f32 = lo x3, 1 / side;
// segr [C][4] f32 = lo, hi of the bisection, the radius of the current evaluation, -
static_assert(DISPU_POISSON_MAX_ROUNDS + 1 <= 512, "the round counters fit their block");
constexpr int PC_CNT_WORDS = 512;

__device__ __forceinline__ int pc_find_seg(const int* __restrict__ off, int C, uint32_t i) {
    int lo = 0, hi = C;                              // the largest c with off[c] <= i (segments are not empty)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t pc_cell1(float x, float lo, float inv) {
    return (uint32_t)(int)fminf(fmaxf((x - lo) * inv, 0.0f), (float)(PC_G - 1));         // NaN -> 0; always inside the grid
}

// ---- bounds ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void pc_seg_init_kernel(int C, uint32_t* __restrict__ segb, int* __restrict__ status) {
    const int c = blockIdx.x * kRsThreads + threadIdx.x;
    if (c >= C) return;
    status[c] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) segb[8 * c + k] = k < 3 ? 0xFFFFFFFFu : 0u;
}

// ordered-integer min / max per segment: order-free.  A wave that lies inside one segment reduces first and adds once.
__global__ __launch_bounds__(kRsThreads) void pc_bounds_kernel(uint32_t N, int C, const int* __restrict__ off, const float* __restrict__ points,
                                                               uint32_t* __restrict__ segb) {
    const uint32_t i = min((uint32_t)(blockIdx.x * kRsThreads + threadIdx.x), N - 1);     // the surplus lanes repeat the last point
    const int seg = pc_find_seg(off, C, i);
    uint32_t lo[3], hi[3], bad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = points[(size_t)i * 3 + c];
        bad |= !(fabsf(v) <= FLT_MAX);
        lo[c] = hi[c] = f32_to_ordered(v);
    }
    uint32_t* b = segb + 8 * (size_t)seg;
    if (__all(seg == __shfl(seg, 0, kWave))) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = min(lo[c], (uint32_t)__shfl_xor((int)lo[c], o, kWave));
                hi[c] = max(hi[c], (uint32_t)__shfl_xor((int)hi[c], o, kWave));
            }
            bad |= (uint32_t)__shfl_xor((int)bad, o, kWave);
        }
        if ((threadIdx.x & (kWave - 1)) != 0) return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        atomicMin(&b[c], lo[c]);
        atomicMax(&b[3 + c], hi[c]);
    }
    if (bad) atomicOr(&b[6], 1u);
}

__global__ __launch_bounds__(kRsThreads) void pc_grid_kernel(int C, const float* __restrict__ radius, uint32_t* __restrict__ segb,
                                                             float* __restrict__ segg) {
    const int c = blockIdx.x * kRsThreads + threadIdx.x;
    if (c >= C) return;
    uint32_t* b = segb + 8 * (size_t)c;
    const float r = radius[c];
    bool bad = b[6] != 0u || !(fabsf(r) <= FLT_MAX);
    float lox = ordered_to_f32(b[0]), loy = ordered_to_f32(b[1]), loz = ordered_to_f32(b[2]);
    const float ex = ordered_to_f32(b[3]) - lox, ey = ordered_to_f32(b[4]) - loy, ez = ordered_to_f32(b[5]) - loz;
    float side = fmaxf(fmaxf(ex, ey), ez) * (1.0f / PC_G);
    if (r > side) side = r;
    if (!(side > 0.0f)) side = 1.0f;                                         // one point, or all identical with r <= 0
    side *= 1.0009765625f;                                                   // 1 + 2^-10
    if (!(side <= FLT_MAX)) bad = true;                                      // an extent beyond the float range
    float inv = 1.0f / side;
    if (bad) { lox = loy = loz = 0.0f; inv = 0.0f; b[6] = 1u; }              // every point in cell 0, and the radius counts as 0
    segg[4 * c + 0] = lox; segg[4 * c + 1] = loy; segg[4 * c + 2] = loz; segg[4 * c + 3] = inv;
}

// ---- keys, cells, ranges ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void pc_keys_kernel(uint32_t N, int C, const int* __restrict__ off, const float* __restrict__ points,
                                                             const float* __restrict__ segg, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * kRsThreads + threadIdx.x;
    if (i >= N) return;
    const int seg = pc_find_seg(off, C, i);
    const float lox = segg[4 * seg + 0], loy = segg[4 * seg + 1], loz = segg[4 * seg + 2], inv = segg[4 * seg + 3];
    const uint32_t cx = pc_cell1(points[(size_t)i * 3 + 0], lox, inv), cy = pc_cell1(points[(size_t)i * 3 + 1], loy, inv),
                   cz = pc_cell1(points[(size_t)i * 3 + 2], loz, inv);
    keys[i] = ((uint64_t)(uint32_t)seg << PC_CELL_BITS) | (uint64_t)((cz << (2 * PC_AXIS_BITS)) | (cy << PC_AXIS_BITS) | cx);
    vals[i] = i;
}

// ex: run_heads_scan's exclusive scan of the heads, replaced in place by the cell number of every sorted position; cstart[v] = the first position of
// occupied cell v, cstart[ncell] = N; ckey[v] = its key; spt[j] = (x, y, z, packed index as bits) of sorted position j
__global__ __launch_bounds__(kRsThreads) void pc_cells_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t N,
                                                              const float* __restrict__ points, uint32_t* __restrict__ ex,
                                                              uint32_t* __restrict__ cstart, uint64_t* __restrict__ ckey,
                                                              float4* __restrict__ spt) {
    const uint32_t j = blockIdx.x * kRsThreads + threadIdx.x;
    if (j >= N) return;
    const uint64_t key = keys[j];
    const uint32_t h = (j == 0 || key != keys[j - 1]) ? 1u : 0u;
    const uint32_t e = ex[j];                        // heads before j: e < N, and e + h <= N
    if (h) { cstart[e] = j; ckey[e] = key; }
    if (j == N - 1) cstart[e + h] = N;
    ex[j] = e + h - 1u;
    const uint32_t i = min(vals[j], N - 1);          // a no-op for the sorter's output; keeps a wrong one from reading outside
    spt[j] = make_float4(points[(size_t)i * 3 + 0], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2], __uint_as_float(i));
}

// one thread per (occupied cell, row of the 3 x 3 neighbourhood in y, z): the sorted positions of the row's cells x - 1 .. x + 1
__global__ __launch_bounds__(kRsThreads) void pc_ranges_kernel(const uint32_t* __restrict__ ncell_p, uint32_t N, const uint64_t* __restrict__ ckey,
                                                               const uint32_t* __restrict__ cstart, uint32_t* __restrict__ crec) {
    const uint32_t ncell = min(*ncell_p, N);
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t >= (size_t)ncell * 9) return;
    const uint32_t v = (uint32_t)(t / 9);
    const int row = (int)(t % 9);
    const uint64_t key = ckey[v];
    const int x = (int)(key & (PC_G - 1)), y = (int)((key >> PC_AXIS_BITS) & (PC_G - 1)), z = (int)((key >> (2 * PC_AXIS_BITS)) & (PC_G - 1));
    const int yy = y + row % 3 - 1, zz = z + row / 3 - 1;
    uint32_t a = 0, e = 0;
    if (yy >= 0 && yy < PC_G && zz >= 0 && zz < PC_G) {
        const uint64_t base = (key >> PC_CELL_BITS << PC_CELL_BITS) | (uint64_t)(((uint32_t)zz << (2 * PC_AXIS_BITS)) | ((uint32_t)yy << PC_AXIS_BITS));
        const uint64_t klo = base | (uint64_t)max(x - 1, 0), khi = base | (uint64_t)min(x + 1, PC_G - 1);
        uint32_t lo = 0, hi = ncell;                 // the first cell with key >= klo
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ckey[mid] < klo) lo = mid + 1; else hi = mid; }
        a = lo;
        hi = ncell;                                  // the first cell with key > khi (not before a)
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ckey[mid] <= khi) lo = mid + 1; else hi = mid; }
        a = cstart[a];                               // cstart[ncell] = N
        e = cstart[lo];
    }
    crec[(size_t)v * PC_REC + 2 * row] = a;
    crec[(size_t)v * PC_REC + 2 * row + 1] = e;
    if (row == 0) { crec[(size_t)v * PC_REC + PC_REC_SEG] = (uint32_t)(key >> PC_CELL_BITS); crec[(size_t)v * PC_REC + PC_REC_SEG + 1] = 0u; }
}

// ---- one evaluation --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pc_seg_of(const uint32_t* __restrict__ cid, const uint32_t* __restrict__ crec, uint32_t s, int C) {
    return min(crec[(size_t)cid[s] * PC_REC + PC_REC_SEG], (uint32_t)(C - 1));
}

__global__ __launch_bounds__(kRsThreads) void pc_eval_init_kernel(uint32_t N, int C, const uint32_t* __restrict__ cid, const uint32_t* __restrict__ crec,
                                                                  const uint32_t* __restrict__ segb, const float* __restrict__ segr,
                                                                  uint8_t* __restrict__ state, uint32_t* __restrict__ cnt,
                                                                  uint32_t* __restrict__ segc) {
    const uint32_t s = blockIdx.x * kRsThreads + threadIdx.x;
    if (s < (uint32_t)PC_CNT_WORDS) cnt[s] = 0u;
    if (s < (uint32_t)C) segc[s] = 0u;
    if (s >= N) return;
    const uint32_t seg = pc_seg_of(cid, crec, s, C);
    state[s] = (segr[4 * seg + 2] > 0.0f && segb[8 * seg + 6] == 0u) ? PC_ACTIVE : PC_KEPT;
}

// One round.  FIRST: over every sorted position; otherwise over list_in[0 .. cnt[round]).  The still-active points go to list_out,
// their number to cnt[round + 1].  state is read and written in place: the header of this file says why that is safe.
template <bool FIRST>
__global__ __launch_bounds__(kRsThreads) void pc_round_kernel(uint32_t N, int C, int round, const float4* __restrict__ spt,
                                                              const uint32_t* __restrict__ cid, const uint32_t* __restrict__ crec,
                                                              const float* __restrict__ segr, volatile uint8_t* state,
                                                              const uint32_t* __restrict__ list_in, uint32_t* __restrict__ list_out,
                                                              uint32_t* cnt) {
    const uint32_t t = blockIdx.x * kRsThreads + threadIdx.x;
    const uint32_t limit = FIRST ? N : min(cnt[round], N);
    bool left = false;
    uint32_t s = 0;
    if (t < limit) {
        s = FIRST ? t : min(list_in[t], N - 1);
        if (state[s] == PC_ACTIVE) {
            const float4 me = spt[s];
            const uint32_t i = __float_as_uint(me.w);
            const uint32_t* __restrict__ rec = crec + (size_t)cid[s] * PC_REC;
            const float r = segr[4 * min(rec[PC_REC_SEG], (uint32_t)(C - 1)) + 2];
            const float r2 = r * r;
            bool pending = false, rejected = false;
            for (int k = 0; k < 9 && !rejected; ++k) {
                const uint32_t e = min(rec[2 * k + 1], N);
                for (uint32_t u = rec[2 * k]; u < e; ++u) {
                    const float4 q = spt[u];
                    if (__float_as_uint(q.w) < i && sqdist3<false>(me.x - q.x, me.y - q.y, me.z - q.z) < r2) {
                        const uint8_t st = state[u];
                        if (st == PC_KEPT) { rejected = true; break; }
                        if (st == PC_ACTIVE) pending = true;
                    }
                }
            }
            if (rejected) state[s] = PC_REJECTED;
            else if (!pending) state[s] = PC_KEPT;
            else left = true;
        }
    }
    const unsigned long long b = __ballot(left);
    if (b) {
        const int lane = threadIdx.x & (kWave - 1), leader = __ffsll(b) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&cnt[round + 1], (uint32_t)__popcll(b));
        base = (uint32_t)__shfl((int)base, leader, kWave);
        const uint32_t pos = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (left && pos < N) list_out[pos] = s;
    }
}

// the round bound was hit: bit 0 for every segment that still holds an active point
__global__ __launch_bounds__(kRsThreads) void pc_cap_kernel(uint32_t N, int C, const uint32_t* __restrict__ cnt_last, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ cid, const uint32_t* __restrict__ crec,
                                                            int* __restrict__ status) {
    const uint32_t t = blockIdx.x * kRsThreads + threadIdx.x;
    if (t >= min(*cnt_last, N)) return;
    atomicOr(&status[pc_seg_of(cid, crec, min(list[t], N - 1), C)], 1);
}

// segc[c] += the KEPT points of segment c (integer adds: order-free)
__global__ __launch_bounds__(kRsThreads) void pc_count_kernel(uint32_t N, int C, const uint32_t* __restrict__ cid, const uint32_t* __restrict__ crec,
                                                              const uint8_t* __restrict__ state, uint32_t* __restrict__ segc) {
    const uint32_t s = blockIdx.x * kRsThreads + threadIdx.x;
    const bool valid = s < N;
    const uint32_t seg = pc_seg_of(cid, crec, valid ? s : N - 1, C);
    const bool kept = valid && state[s] == PC_KEPT;
    if (__all(seg == (uint32_t)__shfl((int)seg, 0, kWave))) {
        const unsigned long long b = __ballot(kept);
        if (b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&segc[seg], (uint32_t)__popcll(b));
    } else if (kept) {
        atomicAdd(&segc[seg], 1u);
    }
}

// The bisection step after evaluation k (k = -1: before the first), per segment, and the radius of evaluation k + 1:
// the midpoint, or lo itself for the last one (k + 1 == steps).  moff == nullptr: keep, the radius is r_top and nothing moves.
// Thread 0 also records the rounds evaluation k took: the launches that found an active point, at least 1.
__global__ __launch_bounds__(kRsThreads) void pc_bisect_kernel(int C, int k, int steps, const int* __restrict__ moff, const float* __restrict__ r_top,
                                                               float* __restrict__ segr, const uint32_t* __restrict__ segc,
                                                               const uint32_t* __restrict__ cnt, int* __restrict__ rounds) {
    const int c = blockIdx.x * kRsThreads + threadIdx.x;
    if (c == 0 && k >= 0 && rounds) {
        int used = 1;
        while (used <= DISPU_POISSON_MAX_ROUNDS && cnt[used] != 0u) ++used;
        rounds[k] = min(used, DISPU_POISSON_MAX_ROUNDS);
    }
    if (c >= C) return;
    float* s = segr + 4 * (size_t)c;
    if (!moff) { s[0] = 0.0f; s[1] = r_top[c]; s[2] = r_top[c]; return; }
    float lo = s[0], hi = s[1];
    if (k < 0) { lo = 0.0f; hi = r_top[c]; }
    else if (k < steps) {
        if ((int)segc[c] >= moff[c + 1] - moff[c]) lo = s[2]; else hi = s[2];
    }
    s[0] = lo; s[1] = hi;
    s[2] = (k + 1 >= steps) ? lo : 0.5f * (lo + hi);
}

// ---- outputs ---------------------------------------------------------------------------------------------------------------------------
// flags by INPUT index: keep (u8), and for select also the words the scan turns into ranks
__global__ __launch_bounds__(kRsThreads) void pc_flags_kernel(uint32_t N, const float4* __restrict__ spt, const uint8_t* __restrict__ state,
                                                              unsigned char* __restrict__ keep, uint32_t* __restrict__ words) {
    const uint32_t s = blockIdx.x * kRsThreads + threadIdx.x;
    if (s >= N) return;
    const uint32_t i = min(__float_as_uint(spt[s].w), N - 1);
    const uint32_t f = state[s] == PC_KEPT ? 1u : 0u;
    keep[i] = (unsigned char)f;
    if (words) words[i] = f;
}

// (M = the rows of idx: a no-op bound for offsets that match the host's, it keeps wrong ones from writing outside)
__global__ __launch_bounds__(kRsThreads) void pc_emit_kernel(uint32_t N, int C, uint32_t M, const int* __restrict__ off, const int* __restrict__ moff,
                                                             const unsigned char* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                             int* __restrict__ idx) {
    const uint32_t i = blockIdx.x * kRsThreads + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const int seg = pc_find_seg(off, C, i);
    const uint32_t k = rank[i] - rank[off[seg]];     // kept points of the segment before i
    const size_t row = (size_t)(uint32_t)moff[seg] + k;
    if (k < (uint32_t)(moff[seg + 1] - moff[seg]) && row < M) idx[row] = (int)(i - (uint32_t)off[seg]);
}

__global__ __launch_bounds__(kRsThreads) void pc_finish_kernel(int C, const int* __restrict__ moff, const uint32_t* __restrict__ segb,
                                                               const float* __restrict__ segr, const uint32_t* __restrict__ segc,
                                                               int* __restrict__ count, float* __restrict__ r_out, int* __restrict__ status) {
    const int c = blockIdx.x * kRsThreads + threadIdx.x;
    if (c >= C) return;
    int st = 0;
    if (segb[8 * c + 6]) st |= PC_BAD;
    if (moff && (int)segc[c] < moff[c + 1] - moff[c]) st |= 2;
    if (st) atomicOr(&status[c], st);
    count[c] = (int)segc[c];
    if (r_out) r_out[c] = segr[4 * c + 0];
}

// ---- scratch ---------------------------------------------------------------------------------------------------------------------------
struct PcScratch {
    RadixSorter sort;                                // after the sort its value buffers are the two lists of active points
    size_t spt, cid, cstart, ckey, crec, state, flag, words, segb, segg, segr, segc, cnt, total;
};
static PcScratch pc_scratch(size_t N, size_t C, void* base = nullptr) {
    PcScratch s;
    Carver cv{(char*)base};
    s.sort.carve(cv, N);
    s.spt = cv.take(16 * N);
    s.cid = cv.take(4 * N);
    s.cstart = cv.take(4 * (N + 1));
    s.ckey = cv.take(8 * N);
    s.crec = cv.take(4 * (size_t)PC_REC * N);        // one record per occupied cell, at most one cell per point
    s.state = cv.take(N);
    s.flag = cv.take(N);
    s.words = cv.take(4 * N);
    s.segb = cv.take(32 * C);
    s.segg = cv.take(16 * C);
    s.segr = cv.take(16 * C);
    s.segc = cv.take(4 * C);
    s.cnt = cv.take(4 * (size_t)PC_CNT_WORDS + 256); // the round counters, then the cell count
    s.total = cv.off;
    return s;
}

struct PcRun {
    uint32_t N;
    int C;
    hipStream_t st;
    char* base;
    PcScratch s;
    template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
    uint32_t* ncell() const { return at<uint32_t>(s.cnt) + PC_CNT_WORDS; }
};

// bounds, grid, keys, sort, cells, ranges: once per call, for the radii r_top
static int pc_prepare(const PcRun& R, const int* off, const float* points, const float* r_top, int* status) {
    const uint32_t N = R.N;
    const int C = R.C;
    hipStream_t st = R.st;
    RadixSorter sort = R.s.sort;
    uint32_t *segb = R.at<uint32_t>(R.s.segb), *cid = R.at<uint32_t>(R.s.cid), *cstart = R.at<uint32_t>(R.s.cstart);
    float* segg = R.at<float>(R.s.segg);
    hipLaunchKernelGGL(pc_seg_init_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, st, C, segb, status);
    hipLaunchKernelGGL(pc_bounds_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, C, off, points, segb);
    hipLaunchKernelGGL(pc_grid_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, st, C, r_top, segb, segg);
    hipLaunchKernelGGL(pc_keys_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, C, off, points, (const float*)segg, sort.k[0], sort.v[0]);
    DISPU_CHECK_LAUNCH();
    int bits = PC_CELL_BITS;
    for (unsigned c = (unsigned)C - 1u; c; c >>= 1) ++bits;
    int rc = sort.sort(N, (bits + 7) / 8, st);
    if (rc) return rc;
    rc = run_heads_scan(sort.keys(), N, cid, sort.sums, R.ncell(), st);
    if (rc) return rc;
    hipLaunchKernelGGL(pc_cells_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, sort.keys(), sort.vals(), N, points, cid, cstart,
                       R.at<uint64_t>(R.s.ckey), R.at<float4>(R.s.spt));
    hipLaunchKernelGGL(pc_ranges_kernel, dim3(rs_blocks((size_t)N * 9)), dim3(kRsThreads), 0, st, (const uint32_t*)R.ncell(), N,
                       (const uint64_t*)R.at<uint64_t>(R.s.ckey), (const uint32_t*)cstart, R.at<uint32_t>(R.s.crec));
    return (int)hipGetLastError();
}

// the keep states at the radii segr[.][2] -> state (by sorted position) and segc (kept points per segment)
static int pc_eval(const PcRun& R, int* status) {
    const uint32_t N = R.N;
    const int C = R.C;
    hipStream_t st = R.st;
    const float4* spt = R.at<float4>(R.s.spt);
    const uint32_t *cid = R.at<uint32_t>(R.s.cid), *crec = R.at<uint32_t>(R.s.crec);
    const float* segr = R.at<float>(R.s.segr);
    uint8_t* state = R.at<uint8_t>(R.s.state);
    uint32_t *cnt = R.at<uint32_t>(R.s.cnt), *segc = R.at<uint32_t>(R.s.segc);
    uint32_t* const* list = R.s.sort.v;              // round k reads list[k & 1] and fills list[(k + 1) & 1]
    hipLaunchKernelGGL(pc_eval_init_kernel, dim3(rs_blocks(N > (uint32_t)PC_CNT_WORDS ? N : PC_CNT_WORDS)), dim3(kRsThreads), 0, st, N, C, cid,
                       crec, (const uint32_t*)R.at<uint32_t>(R.s.segb), segr, state, cnt, segc);
    uint32_t active = N;                             // an upper bound of the list the next round reads
    int round = 0;
    while (active && round < DISPU_POISSON_MAX_ROUNDS) {
        for (int j = 0; j < PC_CHUNK && round < DISPU_POISSON_MAX_ROUNDS; ++j, ++round) {
            if (round == 0)
                hipLaunchKernelGGL(pc_round_kernel<true>, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, C, round, spt, cid, crec, segr, state,
                                   (const uint32_t*)nullptr, list[1], cnt);
            else
                hipLaunchKernelGGL(pc_round_kernel<false>, dim3(rs_blocks(active)), dim3(kRsThreads), 0, st, N, C, round, spt, cid, crec, segr,
                                   state, (const uint32_t*)list[round & 1], list[(round + 1) & 1], cnt);
        }
        DISPU_CHECK_LAUNCH();
        DISPU_TRY(hipMemcpyAsync(&active, cnt + round, sizeof(active), hipMemcpyDeviceToHost, st));      // one word per chunk
        DISPU_TRY(hipStreamSynchronize(st));
        if (active > N) active = N;
    }
    if (active)
        hipLaunchKernelGGL(pc_cap_kernel, dim3(rs_blocks(active)), dim3(kRsThreads), 0, st, N, C, (const uint32_t*)(cnt + round),
                           (const uint32_t*)list[round & 1], cid, crec, status);
    hipLaunchKernelGGL(pc_count_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, N, C, cid, crec, (const uint8_t*)state, segc);
    return (int)hipGetLastError();
}

static bool pc_args(int C, const int* off, const int* off_host, const void* scratch, size_t scratch_bytes, PcRun* R, void* stream) {
    if (!off || !off_host || cells_batch_check(C, off_host)) return false;            // C in 1 .. 65535, segments of 1 .. 2^24 points
    const long long N = off_host[C];
    if (N <= 0 || N >= (1ll << 31)) return false;
    R->N = (uint32_t)N;
    R->C = C;
    R->st = (hipStream_t)stream;
    R->base = (char*)const_cast<void*>(scratch);
    R->s = pc_scratch((size_t)N, (size_t)C, R->base);
    return scratch_ok(scratch, scratch_bytes, R->s.total);
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_poisson_cells_scratch_bytes(int C, long long total_n) {
    if (C <= 0 || C > 65535 || total_n < C || total_n >= (1ll << 31)) return 0;
    return pc_scratch((size_t)total_n, (size_t)C).total;
}

DISPU_EXPORT int dispu_poisson_cells_keep(int C, const int* off, const int* off_host, const float* points, const float* radius,
                                          unsigned char* keep, int* count, int* rounds, void* scratch, size_t scratch_bytes, int* status,
                                          void* stream) {
    PcRun R;
    if (!points || !radius || !keep || !count || !status || !pc_args(C, off, off_host, scratch, scratch_bytes, &R, stream))
        return (int)hipErrorInvalidValue;
    int rc = pc_prepare(R, off, points, radius, status);
    if (rc) return rc;
    hipLaunchKernelGGL(pc_bisect_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, -1, 0, (const int*)nullptr, radius, R.at<float>(R.s.segr),
                       (const uint32_t*)R.at<uint32_t>(R.s.segc), (const uint32_t*)R.at<uint32_t>(R.s.cnt), rounds);
    rc = pc_eval(R, status);
    if (rc) return rc;
    hipLaunchKernelGGL(pc_bisect_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, 0, 0, (const int*)nullptr, radius, R.at<float>(R.s.segr),
                       (const uint32_t*)R.at<uint32_t>(R.s.segc), (const uint32_t*)R.at<uint32_t>(R.s.cnt), rounds);
    hipLaunchKernelGGL(pc_flags_kernel, dim3(rs_blocks(R.N)), dim3(kRsThreads), 0, R.st, R.N, (const float4*)R.at<float4>(R.s.spt),
                       (const uint8_t*)R.at<uint8_t>(R.s.state), keep, (uint32_t*)nullptr);
    hipLaunchKernelGGL(pc_finish_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, (const int*)nullptr,
                       (const uint32_t*)R.at<uint32_t>(R.s.segb), (const float*)R.at<float>(R.s.segr), (const uint32_t*)R.at<uint32_t>(R.s.segc),
                       count, (float*)nullptr, status);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_poisson_cells_select(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, int steps,
                                            const float* points, const float* r_hi, int* idx, float* r_out, int* count_out, int* rounds,
                                            void* scratch, size_t scratch_bytes, int* status, void* stream) {
    PcRun R;
    if (!points || !r_hi || !idx || !r_out || !count_out || !status || !moff || !moff_host || steps < 0 ||
        !pc_args(C, off, off_host, scratch, scratch_bytes, &R, stream))
        return (int)hipErrorInvalidValue;
    if (moff_host[0] != 0) return (int)hipErrorInvalidValue;
    for (int c = 0; c < C; ++c) {
        const long long m = (long long)moff_host[c + 1] - moff_host[c];
        if (m < 1 || m > (long long)off_host[c + 1] - off_host[c]) return (int)hipErrorInvalidValue;
    }
    int rc = pc_prepare(R, off, points, r_hi, status);
    if (rc) return rc;
    float* segr = R.at<float>(R.s.segr);
    const uint32_t *segc = R.at<uint32_t>(R.s.segc), *cnt = R.at<uint32_t>(R.s.cnt);
    hipLaunchKernelGGL(pc_bisect_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, -1, steps, moff, r_hi, segr, segc, cnt, rounds);
    for (int k = 0; k <= steps; ++k) {               // the last pass evaluates the set at lo itself
        rc = pc_eval(R, status);
        if (rc) return rc;
        hipLaunchKernelGGL(pc_bisect_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, k, steps, moff, r_hi, segr, segc, cnt, rounds);
    }
    unsigned char* flag = R.at<unsigned char>(R.s.flag);
    uint32_t* words = R.at<uint32_t>(R.s.words);
    hipLaunchKernelGGL(pc_flags_kernel, dim3(rs_blocks(R.N)), dim3(kRsThreads), 0, R.st, R.N, (const float4*)R.at<float4>(R.s.spt),
                       (const uint8_t*)R.at<uint8_t>(R.s.state), flag, words);
    rc = exclusive_scan_u32(words, R.N, R.s.sort.sums, nullptr, R.st);
    if (rc) return rc;
    hipLaunchKernelGGL(pc_emit_kernel, dim3(rs_blocks(R.N)), dim3(kRsThreads), 0, R.st, R.N, C, (uint32_t)moff_host[C], off, moff, (const unsigned char*)flag,
                       (const uint32_t*)words, idx);
    hipLaunchKernelGGL(pc_finish_kernel, dim3(rs_blocks(C)), dim3(kRsThreads), 0, R.st, C, moff, (const uint32_t*)R.at<uint32_t>(R.s.segb),
                       (const float*)segr, segc, count_out, r_out, status);
    return (int)hipGetLastError();
}
