// Density-based clustering (exact DBSCAN) of a packed ragged batch of clouds: behind dispu_cluster_segments and
// dispu_cluster_select_segments (include/dispu_hip.h, which states the definition).  The reference has no counterpart.  The yardstick is
// tests/cluster_oracle.py.
//
// The labels are a pure function of the input: core points by an integer count, clusters = connected components of the core points
// under d2 <= r2, numbered by their smallest core input index, a non-core point to the core neighbour with the smallest (d2 bits, input
// index).  So the bytes are the same from run to run whatever order the atomics below land in.
//
//   init      flat over the rows: the cloud of every row (binary search in off), P[x] = x, no border link, no minimum, not core
//   pre-pass  morton_cells.hip (fps_cells_prepass): sorted points in cells of 64, the cells' boxes, the non-finite flags
//   core      the walk of radius_count_kernel (outliers.hip) at cap = min_points - 1, WRITTEN AGAIN here: that kernel stores a clamped
//             count by input index, this one a flag by SORTED row, next to the point the link pass reads; a shared inline walk would have
//             had to take the store as a parameter, and radius_count_kernel's machine code is a measured one that stays as it is.
//   link      one wave per cell, one query per lane, the same walk and bounds without the cap.  A visited cell brings its 64 core flags
//             and, lane-parallel, the current roots of its core points (one find each, not one per pair).  A core lane unites itself with
//             every core point at d2 <= r2 whose root differs from its own cached root; a non-core lane keeps the smallest
//             (d2 bits, input index) among core points and that point's sorted row: the border search costs no third pass.
//             A cell is skipped whole, distances included, when the wave holds no non-core query and every core query and every core
//             point of the cell already show ONE root: in a dense cloud that is most visits of every wave that starts late.
//   union-find  one 32-bit word per sorted row, P[x] <= x always; a root is P[x] == x.  Only roots are hooked, the larger below the
//             smaller, by atomicMin; find strictly descends and halves its path with plain stores of an ancestor.
//             Every load may be stale (the L2 slices of the dies are not coherent inside a launch): a stale word is a FORMER parent, which
//             is still in x's component, so a find may stop short of the root but never leaves the component; the atomicMin's returned
//             word is the truth: it equals the row only if the row WAS a root at that instant, and then the hook stands (a halving store
//             never touches a root: it writes P[x] only after having seen P[x] != x, and a row never becomes a root again).  If it
//             differs, the row had a parent `old` already; the word now holds min(old, b), so x's subtree hangs below one of the two and
//             the thread goes on to unite old with b, which restores whatever the overwrite cut.  A halving store that overwrites such a
//             word puts x back below a former ancestor: the same argument.  Equal roots, however stale, prove one component (they were
//             joined at some instant, and components only grow), so the guard in front of every unite never skips a needed one; unequal
//             stale roots only cost a unite that finds nothing to do.  orient_consistent.hip states the same argument for its guards.
//   Every loop is capped.  A lane that exhausts a cap raises a device flag; the link pass is idempotent (it unites the same pairs
//   again and recomputes the same border links) and is launched kClLinkLaunches times, each launch after the first returning at once
//   unless the one before raised the flag: the shape of orient_jump_kernel.  A flag still up after the last launch sets bit 2 of the
//   cloud's status and nothing is written for that cloud: nothing spins, nothing waits on another thread.
//   flatten   capped pointer jumping, orient's scheme and bound: 64 links per launch, 4 launches, 65^4 > 2^24
//   number    per root the integer atomicMin of its core members' input indices; a flag at that index (input order); exclusive_scan_u32
//             over the packed flags: cluster id = scan at the flag - scan at the cloud's first row
//   label     flat over the sorted rows: core -> its root's id, non-core -> the id of its recorded core row's root, else -1; written at
//             the input index; sizes by integer adds (one word per cluster), the cluster count per cloud
//   select    one workgroup per cloud: `keep` rounds of a fixed-order max reduction over (size, -id) below the round before's winner,
//             then the keep flags of the cloud's points for dispu_compact_segments at rule 0
//
// Why this decomposition: the pair test is the expensive part and the walk that finds the pairs exists; a device-wide union-find turns
// every pair into at most a compare against a register, so linking costs one more search pass, not a graph in memory ([n, degree] at
// eps = 4 spacings is ~50 words per point) and not a round per level of the component tree.
// Integer atomics only (min, add, or): order-free.  No float atomics.
#include "knn_cells.h"

namespace dispu {

constexpr int kClThreads = 256;
constexpr int kClFindIters = 4096, kClUniteIters = 64, kClLinkLaunches = 4;
constexpr int kClJumpIters = 64, kClJumpLaunches = 4;
constexpr int kClSel = 1024, kClSelWaves = kClSel / kWave, kClMaxKeep = 32;
constexpr uint32_t kClNone = 0xFFFFFFFFu;
constexpr uint64_t kClNoKey = ~0ull;
constexpr int kClCap = 2;                                                       // status[c]; 1 (non-finite) is the prologue's
// the head of the scratch, DISPU_CLUSTER_HEAD_INTS ints: [0, 4) the link launches' cap flags, [4, 8) the jump launches', [8] the scan's total
constexpr int kClHeadLink = 0, kClHeadJump = 4, kClHeadTotal = 8;
static_assert(kClLinkLaunches == 4 && kClJumpLaunches == 4 && DISPU_CLUSTER_HEAD_INTS >= 9, "the head's layout is part of the C-ABI");

__device__ __forceinline__ uint32_t cl_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as far as this thread can see it, the path halved on the way.
// Terminates: every word read satisfies P[y] <= y and the loop goes on only while P[y] < y, so x strictly descends: at most x steps.
// Capped at kClFindIters all the same; a lane that runs out sets `capped` and returns the ancestor it reached.
__device__ __forceinline__ uint32_t cl_find(uint32_t* P, uint32_t x, bool& capped) {
    for (int it = 0; it < kClFindIters; ++it) {
        const uint32_t p = cl_ld(&P[x]);
        if (p >= x) return x;                                                   // a root (p > x cannot be: it would end the descent too)
        const uint32_t gp = cl_ld(&P[p]);
        if (gp >= p) return p;
        cl_st(&P[x], gp);                                                       // gp < p < x: an ancestor, never written to a root
        x = gp;
    }
    capped = true;
    return x;
}

// Unite the components of rows a and b; returns a row that was their common root as this thread saw it.
// Terminates: an iteration that does not return replaces the larger row a by `old`, the word the atomicMin displaced, old < a, and the
// finds only descend further: the larger index of the pair strictly decreases, so at most max(a, b) iterations.  Capped at
// kClUniteIters all the same.  No iteration waits for another thread.
__device__ __forceinline__ uint32_t cl_unite(uint32_t* P, uint32_t a, uint32_t b, bool& capped) {
    for (int it = 0; it < kClUniteIters; ++it) {
        a = cl_find(P, a, capped);
        b = cl_find(P, b, capped);
        if (a == b) return a;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(&P[a], b);                               // b < a: P[a] <= a stays true
        if (old == a) return b;                                                 // a was a root at that instant: hooked
        a = old;                                                                // a had a parent already: unite that with b
    }
    capped = true;
    return a < b ? a : b;
}

// arr[r] = min(arr[r], key) over the active lanes: one atomic where the whole wave aims at one word, a guarding load in front of each
__device__ __forceinline__ void cl_min_u32(uint32_t* arr, uint32_t r, uint32_t key, bool act, int lane) {
    const uint64_t m = __ballot(act);
    if (!m) return;
    const int first = __ffsll((unsigned long long)m) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)r, first, kWave);
    if (__ballot(act && r == r0) == m) {
        const uint32_t v = (uint32_t)wave_min_u64(act ? (uint64_t)key : kClNoKey);
        if (lane == first && v < cl_ld(&arr[r0])) atomicMin(&arr[r0], v);
    } else if (act && key < cl_ld(&arr[r])) {
        atomicMin(&arr[r], key);
    }
}

// arr[r] += 1 over the active lanes: one atomic per DISTINCT word of the wave.  A wave is one Morton cell, which holds points of one or
// two clusters as a rule; one add per lane instead made 64 clusters of 6400 points queue 6400 adds on each of 64 words (measured:
// DESIGN section 9, "Clustering").  Terminates: every turn clears at least the bit of `first` from m: at most 64 turns.
__device__ __forceinline__ void cl_count(int* arr, uint32_t r, bool act, int lane) {
    unsigned long long m = __ballot(act);
    while (m) {
        const int first = (int)__builtin_ctzll(m);
        const uint32_t r0 = (uint32_t)__shfl((int)r, first, kWave);
        const unsigned long long same = __ballot(act && r == r0) & m;
        if (lane == first) atomicAdd(&arr[r0], (int)__popcll(same));
        m &= ~same;
    }
}

__global__ __launch_bounds__(kClThreads) void cluster_init_kernel(uint32_t total, int C, const int* __restrict__ off, int* __restrict__ cid,
                                                                  uint32_t* __restrict__ core, uint32_t* __restrict__ P,
                                                                  uint32_t* __restrict__ bnd, uint32_t* __restrict__ rmin,
                                                                  uint32_t* __restrict__ heads) {
    const uint32_t x = blockIdx.x * kClThreads + threadIdx.x;
    if (x >= total) return;
    int lo = 0, hi = C;                                                         // the segment with off[lo] <= x < off[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)off[mid] <= x) lo = mid; else hi = mid;
    }
    cid[x] = lo;
    core[x] = 0u;
    P[x] = x;
    bnd[x] = kClNone;
    rmin[x] = kClNone;
    heads[x] = 0u;
}

// radius_count_kernel's walk (outliers.hip) at cap = min_points - 1; the flag goes to the point's SORTED row
__global__ __launch_bounds__(kNrmThreads) void cluster_core_kernel(const int* __restrict__ off, const uint32_t* __restrict__ segb,
                                                                   const float4* __restrict__ spt, const float* __restrict__ tab, float r2,
                                                                   int cap, uint32_t* __restrict__ core, int* __restrict__ status) {
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
        while (reach) {                                                         // one bit fewer per turn
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
    if (valid) core[base + (size_t)(cb * kNrmCell + lane)] = raw > cap ? 1u : 0u;
}

// The hot path.  flag_prev: the cap flag of the launch before (NULL for the first); last: this is the final launch.
__global__ __launch_bounds__(kNrmThreads) void cluster_link_kernel(const int* __restrict__ off, const uint32_t* __restrict__ segb,
                                                                   const float4* __restrict__ spt, const float* __restrict__ tab, float r2,
                                                                   const uint32_t* __restrict__ core, uint32_t* P, uint32_t* __restrict__ bnd,
                                                                   const int* __restrict__ flag_prev, int* __restrict__ flag_cur,
                                                                   int* __restrict__ capst, int* __restrict__ status, int last) {
    if (flag_prev && *flag_prev == 0) return;                                   // the launch before ran every loop to its end
#include "knn_cells_prologue.h"  // segment, cell, query, as text
    const uint32_t g = (uint32_t)base + (uint32_t)(cb * kNrmCell + (valid ? lane : 0));   // the query's sorted row (idle lanes: query 0's)
    const bool mycore = valid && core[g] != 0u;
    const bool border = valid && !mycore;
    uint32_t myroot = g;                                                        // the lane's root as it last saw it
    uint64_t bkey = kClNoKey;                                                   // a non-core lane: the best (d2 bits, input index) ...
    uint32_t brow = kClNone;                                                    // ... and that core point's sorted row
    bool capped = false;
    for (int j0 = 0; j0 < K; j0 += kWave) {                                     // K <= 2^18 cells: at most 4096 trips
        const int j = j0 + lane;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        bool near = false;
        if (j < K) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            near = cell_box_lb(a, b, qlo4.x, qlo4.y, qlo4.z, qlo4.w, qhi4.x, qhi4.y) <= r2;
        }
        unsigned long long reach = __ballot(near);
        while (reach) {                                                         // one bit fewer per turn: at most 64
            const int bl = (int)__builtin_ctzll(reach);
            reach &= reach - 1;
            const float4 a1 = make_float4(__shfl(a.x, bl, kWave), __shfl(a.y, bl, kWave), __shfl(a.z, bl, kWave), __shfl(a.w, bl, kWave));
            const float4 b1 = make_float4(__shfl(b.x, bl, kWave), __shfl(b.y, bl, kWave), 0.f, 0.f);
            if (!__any(valid && cell_box_lb(a1, b1, q.x, q.y, q.z, q.x, q.y, q.z) <= r2)) continue;
            const int cj = j0 + bl, cnt = min(kNrmCell, n - cj * kNrmCell);
            const uint32_t row0 = (uint32_t)base + (uint32_t)(cj * kNrmCell);
            const uint32_t rowl = row0 + (uint32_t)min(lane, cnt - 1);          // the cell's point this lane fetches
            const float4 p = sp[cj * kNrmCell + min(lane, cnt - 1)];
            const bool pcore = lane < cnt && core[rowl] != 0u;
            const unsigned long long cmask = __ballot(pcore);
            if (!cmask) continue;                                               // a cell without a core point links nothing
            uint32_t rl = pcore ? cl_find(P, rowl, capped) : kClNone;           // the cell's roots, one find per point
            if (mycore) myroot = cl_find(P, myroot, capped);
            if (!__any(border)) {                                               // one root on both sides already: nothing to learn here
                const uint32_t r0 = (uint32_t)__shfl((int)rl, (int)__builtin_ctzll(cmask), kWave);
                if (__ballot(pcore && rl == r0) == cmask && !__any(mycore && myroot != r0)) continue;
            }
            unsigned long long todo = cmask;
            while (todo) {                                                      // one bit fewer per turn: at most 64
                const int i = (int)__builtin_ctzll(todo);
                todo &= todo - 1;
                const float px = __shfl(p.x, i, kWave), py = __shfl(p.y, i, kWave), pz = __shfl(p.z, i, kWave);
                const float d2 = sqdist3<false>(px - q.x, py - q.y, pz - q.z);
                const bool hit = valid && d2 <= r2;
                const uint32_t rowj = row0 + (uint32_t)i;
                const uint32_t inj = (uint32_t)__shfl(__float_as_int(p.w), i, kWave);   // its input index (shuffles stay outside the branches)
                if (border && hit) {
                    const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)inj;
                    if (key < bkey) {
                        bkey = key;
                        brow = rowj;
                    }
                }
                const uint32_t rj = (uint32_t)__shfl((int)rl, i, kWave);
                const bool need = mycore && hit && myroot != rj;                // the guard: equal roots, however stale, are one component
                const unsigned long long m = __ballot(need);
                if (!m) continue;
                const int first = (int)__builtin_ctzll(m);
                const uint32_t m0 = (uint32_t)__shfl((int)myroot, first, kWave);
                if (__ballot(need && myroot == m0) == m) {                      // the whole wave aims at one pair of roots: one unite
                    uint32_t r = 0;
                    if (lane == first) r = cl_unite(P, g, rowj, capped);
                    r = (uint32_t)__shfl((int)r, first, kWave);
                    if (need) myroot = r;
                } else if (need) {
                    myroot = cl_unite(P, g, rowj, capped);
                }
                if (pcore) rl = cl_find(P, rowl, capped);                       // the cell's roots moved: look again
            }
        }
    }
    if (border) bnd[g] = brow;
    if (capped) {
        *flag_cur = 1;                                                          // every writer stores the same value
        if (last) atomicOr(&capst[c], 1);
    }
}

__global__ __launch_bounds__(kClThreads) void cluster_jump_kernel(uint32_t total, uint32_t* P, const int* __restrict__ flag_prev,
                                                                  int* __restrict__ flag_cur, const int* __restrict__ cid,
                                                                  int* __restrict__ capst, int last) {
    if (flag_prev && *flag_prev == 0) return;                                   // the launch before left every word at its root
    const uint32_t x = blockIdx.x * kClThreads + threadIdx.x;
    if (x >= total) return;
    const uint32_t w = cl_ld(&P[x]);
    uint32_t p = w;
    bool done = false;
    for (int it = 0; it < kClJumpIters; ++it) {                                 // bounded: never spins
        if (p >= x) { p = x; done = true; break; }                              // (x itself is a root)
        const uint32_t q = cl_ld(&P[p]);
        if (q >= p) { done = true; break; }
        p = q;
    }
    if (!done) done = cl_ld(&P[p]) >= p;
    if (p != w) cl_st(&P[x], p);
    if (!done) {
        *flag_cur = 1;
        if (last) atomicOr(&capst[cid[x]], 1);
    }
}

// per root the smallest input index among its core members
__global__ __launch_bounds__(kClThreads) void cluster_min_kernel(uint32_t total, const float4* __restrict__ spt, const uint32_t* __restrict__ core,
                                                                 const uint32_t* __restrict__ P, uint32_t* __restrict__ rmin) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t x = blockIdx.x * kClThreads + threadIdx.x;
    const bool act = x < total && core[x] != 0u;                                // core is 0 for every row of a non-finite segment
    uint32_t r = 0, key = 0;
    if (act) {
        r = min(P[x], total - 1);                                               // (the clamp never acts: P[x] <= x)
        key = (uint32_t)__float_as_int(spt[x].w);
    }
    cl_min_u32(rmin, r, key, act, lane);
}

__global__ __launch_bounds__(kClThreads) void cluster_heads_kernel(uint32_t total, const int* __restrict__ off, const int* __restrict__ cid,
                                                                   const uint32_t* __restrict__ core, const uint32_t* __restrict__ P,
                                                                   const uint32_t* __restrict__ rmin, uint32_t* __restrict__ heads) {
    const uint32_t x = blockIdx.x * kClThreads + threadIdx.x;
    if (x >= total || core[x] == 0u || P[x] != x) return;
    const int c = cid[x];
    const uint32_t b0 = (uint32_t)off[c], n = (uint32_t)off[c + 1] - b0, m = rmin[x];
    if (m < n) heads[b0 + m] = 1u;                                              // input order
}

// heads: after the exclusive scan.  sizes: zero-filled [total] or NULL
__global__ __launch_bounds__(kClThreads) void cluster_label_kernel(uint32_t total, int C, const int* __restrict__ off, const int* __restrict__ cid,
                                                                   const uint32_t* __restrict__ segb, const float4* __restrict__ spt,
                                                                   const uint32_t* __restrict__ core, const uint32_t* __restrict__ P,
                                                                   const uint32_t* __restrict__ bnd, const uint32_t* __restrict__ rmin,
                                                                   const uint32_t* __restrict__ heads, const uint32_t* __restrict__ head_total,
                                                                   const int* __restrict__ capst, int* __restrict__ labels,
                                                                   unsigned char* __restrict__ core_out, int* __restrict__ sizes,
                                                                   int* __restrict__ nclusters, int* __restrict__ status) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t x = blockIdx.x * kClThreads + threadIdx.x;
    bool count = false;
    uint32_t slot = 0;
    if (x < total) {
        const int c = cid[x];
        const uint32_t b0 = (uint32_t)off[c], n = (uint32_t)off[c + 1] - b0;
        const bool bad = segb[(size_t)c * 8 + 6] != 0u, cap = capst[c] != 0;
        if (x == b0 && cap && !bad) status[c] = kClCap;                         // (the link pass's prologue wrote 0 or 1)
        if (!bad && !cap) {
            const uint32_t first = heads[b0];
            if (x == b0) nclusters[c] = (int)((c + 1 < C ? heads[b0 + n] : *head_total) - first);
            const uint32_t i = min((uint32_t)__float_as_int(spt[x].w), n - 1);  // the input index (the clamp never acts)
            const bool is_core = core[x] != 0u;
            const uint32_t via = is_core ? x : bnd[x];                          // the core row whose cluster this point takes
            int label = -1;
            if (via < total) {
                const uint32_t m = rmin[min(P[via], total - 1)];
                if (m < n) label = (int)(heads[b0 + m] - first);
            }
            labels[b0 + i] = label;
            if (core_out) core_out[b0 + i] = is_core ? 1 : 0;
            if (sizes && label >= 0 && (uint32_t)label < n) {
                count = true;
                slot = b0 + (uint32_t)label;
            }
        }
    }
    if (sizes) cl_count(sizes, slot, count, lane);
}

// max over the workgroup in a fixed order: a wave reduction, then the waves in ascending order; every thread returns the maximum
__device__ __forceinline__ uint64_t cl_block_max(uint64_t v, uint64_t* red) {
    v = wave_max_u64(v);
    __syncthreads();                                                            // red may still be read from the call before
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    uint64_t t = 0ull;
#pragma unroll
    for (int i = 0; i < kClSelWaves; ++i) t = red[i] > t ? red[i] : t;
    return t;
}

// key of cluster k of size s: larger size first, then the smaller id; 0 = no cluster (s >= 1 makes every real key > 0)
__device__ __forceinline__ uint64_t cl_sel_key(int s, uint32_t k) { return ((uint64_t)(uint32_t)s << 32) | (uint64_t)(kClNone - k); }

__global__ __launch_bounds__(kClSel) void cluster_select_kernel(const int* __restrict__ off, const int* __restrict__ labels,
                                                                const int* __restrict__ sizes, const int* __restrict__ nclusters,
                                                                const int* __restrict__ status, int keep, int min_size,
                                                                int* __restrict__ flags) {
    __shared__ uint64_t red[kClSelWaves];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int b0 = off[c], n = off[c + 1] - b0;
    if (status[c] != 0) {                                                       // a flagged segment keeps nothing
        for (long long i = tid; i < n; i += kClSel) flags[(size_t)b0 + (size_t)i] = 0;
        return;
    }
    const int nc = min(max(nclusters[c], 0), n);
    const int* __restrict__ sz = sizes + (size_t)b0;
    uint64_t thr = kClNoKey;                                                    // the winner of the round before
    for (int r = 0; r < keep; ++r) {                                            // keep <= 32 rounds
        uint64_t best = 0ull;
        for (long long k = tid; k < nc; k += kClSel) {
            const int s = sz[k];
            const uint64_t key = cl_sel_key(s, (uint32_t)k);
            if (s >= min_size && key < thr && key > best) best = key;
        }
        best = cl_block_max(best, red);
        if (best == 0ull) break;                                                // uniform: fewer clusters than keep
        thr = best;
    }
    for (long long i = tid; i < n; i += kClSel) {
        const int l = labels[(size_t)b0 + (size_t)i];
        int f = 0;
        if (l >= 0 && l < nc && thr != kClNoKey) {
            const int s = sz[l];
            f = s >= min_size && cl_sel_key(s, (uint32_t)l) >= thr ? 1 : 0;
        }
        flags[(size_t)b0 + (size_t)i] = f;
    }
}

struct ClLayout {
    int *head, *capst, *cid;
    uint32_t *core, *P, *bnd, *rmin, *heads, *sums;
    char* pre;
    size_t pre_bytes, bytes;
};

static ClLayout cl_layout(int C, const int* off_host, char* base) {
    ClLayout L;
    const size_t total = (size_t)off_host[C];
    Carver cv{base};
    L.head = cv.ptr<int>((size_t)(DISPU_CLUSTER_HEAD_INTS + C) * 4);           // zero-filled together
    L.capst = base ? L.head + DISPU_CLUSTER_HEAD_INTS : nullptr;
    L.pre_bytes = fps_cells_prepass_scratch(C, off_host);
    L.pre = cv.ptr<char>(L.pre_bytes);
    L.cid = cv.ptr<int>(total * 4);
    L.core = cv.ptr<uint32_t>(total * 4);
    L.P = cv.ptr<uint32_t>(total * 4);
    L.bnd = cv.ptr<uint32_t>(total * 4);
    L.rmin = cv.ptr<uint32_t>(total * 4);
    L.heads = cv.ptr<uint32_t>(total * 4);
    L.sums = cv.ptr<uint32_t>(4 * scan_blocks(total));
    L.bytes = cv.off;
    return L;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_cluster_scratch_bytes(int C, const int* off_host) {
    if (cells_batch_check(C, off_host) != 0) return 0;
    return cl_layout(C, off_host, nullptr).bytes;
}

DISPU_EXPORT int dispu_cluster_segments(int C, const int* off, const int* off_host, float eps, int min_points, const float* cloud, int* labels,
                                        unsigned char* core_or_null, int* sizes_or_null, int* nclusters, int* status, void* scratch,
                                        size_t scratch_bytes, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (!(eps > 0.f) || !(eps <= 3.4028235e38f) || min_points < 1 || !off || !cloud || !labels || !nclusters || !status)
        return (int)hipErrorInvalidValue;
    const ClLayout L = cl_layout(C, off_host, (char*)scratch);
    if (!scratch_ok(scratch, scratch_bytes, L.bytes)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t total = (uint32_t)off_host[C];
    const dim3 block(kClThreads), gn((total + kClThreads - 1) / kClThreads);

    DISPU_TRY(hipMemsetAsync(L.head, 0, (size_t)(DISPU_CLUSTER_HEAD_INTS + C) * 4, st));
    if (sizes_or_null) DISPU_TRY(hipMemsetAsync(sizes_or_null, 0, (size_t)total * 4, st));
    hipLaunchKernelGGL(cluster_init_kernel, gn, block, 0, st, total, C, off, L.cid, L.core, L.P, L.bnd, L.rmin, L.heads);
    DISPU_CHECK_LAUNCH();
    const float4* spt;
    const float* tab;
    const uint32_t* segb;
    int kmax = 0;
    const int rp = fps_cells_prepass(C, off, off_host, cloud, L.pre, L.pre_bytes, &spt, &tab, &segb, &kmax, st);
    if (rp != 0) return rp;
    const float r2 = eps * eps;                                                 // one fp32 rounding (the build does not contract)
    const dim3 gcell((kmax + kNrmWaves - 1) / kNrmWaves, C), bcell(kNrmThreads);
    hipLaunchKernelGGL(cluster_core_kernel, gcell, bcell, 0, st, off, segb, spt, tab, r2, min_points - 1, L.core, status);
    DISPU_CHECK_LAUNCH();
    for (int j = 0; j < kClLinkLaunches; ++j) {
        int* fl = L.head + kClHeadLink + j;
        hipLaunchKernelGGL(cluster_link_kernel, gcell, bcell, 0, st, off, segb, spt, tab, r2, L.core, L.P, L.bnd, j ? fl - 1 : nullptr, fl, L.capst,
                           status, j == kClLinkLaunches - 1 ? 1 : 0);
    }
    DISPU_CHECK_LAUNCH();
    for (int j = 0; j < kClJumpLaunches; ++j) {
        int* fl = L.head + kClHeadJump + j;
        hipLaunchKernelGGL(cluster_jump_kernel, gn, block, 0, st, total, L.P, j ? fl - 1 : nullptr, fl, L.cid, L.capst,
                           j == kClJumpLaunches - 1 ? 1 : 0);
    }
    DISPU_CHECK_LAUNCH();
    hipLaunchKernelGGL(cluster_min_kernel, gn, block, 0, st, total, spt, L.core, L.P, L.rmin);
    hipLaunchKernelGGL(cluster_heads_kernel, gn, block, 0, st, total, off, L.cid, L.core, L.P, L.rmin, L.heads);
    DISPU_CHECK_LAUNCH();
    const int rs = exclusive_scan_u32(L.heads, total, L.sums, (uint32_t*)(L.head + kClHeadTotal), st);
    if (rs != 0) return rs;
    hipLaunchKernelGGL(cluster_label_kernel, gn, block, 0, st, total, C, off, L.cid, segb, spt, L.core, L.P, L.bnd, L.rmin, L.heads,
                       (const uint32_t*)(L.head + kClHeadTotal), L.capst, labels, core_or_null, sizes_or_null, nclusters, status);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_cluster_select_segments(int C, const int* off, const int* off_host, const int* labels, const int* sizes,
                                               const int* nclusters, const int* status, int keep, int min_size, int* flags, void* stream) {
    const int rc = cells_batch_check(C, off_host);
    if (rc != 0) return rc;
    if (keep < 1 || keep > kClMaxKeep || min_size < 1 || !off || !labels || !sizes || !nclusters || !status || !flags)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_select_kernel, dim3(C), dim3(kClSel), 0, (hipStream_t)stream, off, labels, sizes, nclusters, status, keep, min_size,
                       flags);
    return (int)hipGetLastError();
}
