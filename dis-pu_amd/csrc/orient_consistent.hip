// Consistent normal orientation of a packed ragged batch of clouds (Hoppe et al. 1992): the sign is propagated along the minimum
// spanning forest of the undirected k-NN graph weighted by 1 - |n_u . n_v|: behind dispu_orient_consistent_segments
// (include/dispu_hip.h).  The reference has no counterpart.  The yardstick is tests/orient_oracle.py.
//
// The forest is unique: edges are strictly ordered by (bits of w, min(u, v), max(u, v)), and a minimum spanning forest under a strict
// total order is unique whatever algorithm finds it.  Here: Boruvka rounds over the n k directed neighbour slots with a parity
// union-find.  Every node x owns ONE 32-bit word P[x] = parent << 1 | parity, parity = the XOR of s(e) = [dot < 0] along the forest path
// from x to its parent; node numbers are rows of the packed batch (< 2^29, as total k < 2^31 and k >= 4).
//
//   init      P[x] = x, the cloud id of every row (binary search in off), the non-finite check of the normals
//   round r   (at most ceil(log2 n_max) of them: every component that still has an outgoing edge merges with another one)
//     propose     every slot (u, v) whose ends have different roots offers key1 = w bits << 32 | min(u, v) to both roots: 64-bit
//                 integer min.  P is a star forest here (every word points at its root), so a root is one load.  Two launches: a row
//                 offers the minimum of its k slots to its OWN root (one atomic per row), then every slot offers to the OTHER root.
//     propose hi  the slots whose key1 won offer max(u, v): 32-bit integer min.  (key1, max) is the whole 88-bit key, exactly.
//     hook        a root reads its winning edge (lo, hi), recomputes s, and hooks itself to the other end's root with parity
//                 par[a] ^ par[b] ^ s.  Under a strict order the only cycles are two components that chose the SAME edge: the lower
//                 root of such a pair stays.  The new words go to H, not to P: every read of this kernel sees the round's star forest.
//     apply       P[x] = H[x] where a hook was written; the proposal tables are cleared
//     jump        in-place pointer jumping, parities composed.  A thread rewrites only its own word, and a word is parent and parity
//                 together, so a reader that races a writer still sees a valid (ancestor, parity to it) pair.  A thread follows at most
//                 kOrJumpIters links per launch; its word then points >= kOrJumpIters + 1 levels up, so a tree of depth d has depth
//                 <= ceil(d / 65) after a launch and 4 launches flatten any tree of 2^24 nodes (65^4 > 2^24).  Launches 2 - 4 return
//                 at once unless the one before left a thread short of its root (a device flag).  A thread still short after the last
//                 launch (a cycle: impossible under the strict order) sets bit 4 of its cloud's status and returns: nothing spins.
//   finish    three passes over the nodes: per root the anchor's (z, y) key, the lowest row, the vote counts, the roots per cloud;
//             then (x, lowest row) among the nodes that hold the (z, y) maximum; then the flips and the outputs.
//
// Rounds end by a device-side counter: the hook kernel counts its hooks in live[r], every later launch of the sequence reads the counter
// of the round before and returns at once when it is 0.  The host never waits (the entry stays asynchronous); flags bit 0 asks instead
// for one 4-byte read-back per round, which ends the launch sequence early and synchronises the stream (tools/orient_bench.py measures
// the two).
//
// Contention: late rounds send millions of proposals to a handful of roots, the finish sends every node of a component to its root.
// Every atomic is guarded twice: a wave whose active lanes all aim at ONE address reduces in the wave first (DPP min / max, ballot
// counts) and issues one atomic; otherwise each lane first loads the current value and skips a proposal that cannot lower (raise) it --
// a stale load is only ever too large (small), so a skip is never wrong.  The early rounds, where nearly every slot is a cross slot, are
// served by the order of the propose launches: the row pass makes one offer per row, and after it the guarding load turns nearly every
// per-slot offer away.  A row whose slots all end inside its own component is marked dead and skipped from then on (components only
// grow).  Measurements and the form this replaced: DESIGN.md section 9, "Consistent orientation".  Only integer min / max / add / or
// atomics: order-free, identical bytes from run to run.  No float atomics.
#include "internal.h"

namespace dispu {

constexpr int kOrThreads = 256;
constexpr int kOrJumpIters = 64, kOrJumpLaunches = 4, kOrMaxRounds = 24;
constexpr uint32_t kOrNone = 0xFFFFFFFFu;
constexpr uint64_t kOrNoKey = ~0ull;
constexpr int kOrBadNormal = 1, kOrBadIndex = 2, kOrCap = 4;                    // bits of status[c]

__device__ __forceinline__ uint32_t or_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t or_ld(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void or_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (n_a . n_b) in plain fp32: one rounding per operation (the library is built with -ffp-contract=off)
__device__ __forceinline__ float or_dot(const float* __restrict__ nrm, uint32_t a, uint32_t b) {
    const float* p = nrm + (size_t)a * 3;
    const float* q = nrm + (size_t)b * 3;
    const float s = p[0] * q[0] + p[1] * q[1];
    return s + p[2] * q[2];
}

// true when every active lane of the wave holds the same index; r0 = that index, first = the lowest active lane.  Wave-uniform result.
__device__ __forceinline__ bool or_uniform(uint32_t r, bool act, uint64_t m, uint32_t& r0, int& first) {
    first = __ffsll((unsigned long long)m) - 1;
    r0 = (uint32_t)__shfl((int)r, first, kWave);
    return __ballot(act && r == r0) == m;
}

__device__ __forceinline__ void or_min_u64(uint64_t* arr, uint32_t r, uint64_t key, bool act, int lane) {
    const uint64_t m = __ballot(act);
    if (!m) return;
    uint32_t r0;
    int first;
    if (or_uniform(r, act, m, r0, first)) {
        const uint64_t v = wave_min_u64(act ? key : kOrNoKey);
        if (lane == first && v < or_ld(&arr[r0])) atomicMin((unsigned long long*)&arr[r0], (unsigned long long)v);
    } else if (act && key < or_ld(&arr[r])) {
        atomicMin((unsigned long long*)&arr[r], (unsigned long long)key);
    }
}

__device__ __forceinline__ void or_max_u64(uint64_t* arr, uint32_t r, uint64_t key, bool act, int lane) {
    const uint64_t m = __ballot(act);
    if (!m) return;
    uint32_t r0;
    int first;
    if (or_uniform(r, act, m, r0, first)) {
        const uint64_t v = wave_max_u64(act ? key : 0ull);
        if (lane == first && v > or_ld(&arr[r0])) atomicMax((unsigned long long*)&arr[r0], (unsigned long long)v);
    } else if (act && key > or_ld(&arr[r])) {
        atomicMax((unsigned long long*)&arr[r], (unsigned long long)key);
    }
}

__device__ __forceinline__ void or_min_u32(uint32_t* arr, uint32_t r, uint32_t key, bool act, int lane) {
    const uint64_t m = __ballot(act);
    if (!m) return;
    uint32_t r0;
    int first;
    if (or_uniform(r, act, m, r0, first)) {
        const uint32_t v = (uint32_t)wave_min_u64(act ? (uint64_t)key : kOrNoKey);
        if (lane == first && v < or_ld(&arr[r0])) atomicMin(&arr[r0], v);
    } else if (act && key < or_ld(&arr[r])) {
        atomicMin(&arr[r], key);
    }
}

// arr[r] += hi_bit << 32 | lo_bit over the active lanes (two counters in one 64-bit word)
__device__ __forceinline__ void or_add2(uint64_t* arr, uint32_t r, bool hi_bit, bool lo_bit, int lane) {
    const bool act = hi_bit || lo_bit;
    const uint64_t m = __ballot(act);
    if (!m) return;
    uint32_t r0;
    int first;
    if (or_uniform(r, act, m, r0, first)) {
        const uint64_t v = ((uint64_t)__popcll((unsigned long long)__ballot(hi_bit)) << 32) | (uint64_t)__popcll((unsigned long long)__ballot(lo_bit));
        if (lane == first) atomicAdd((unsigned long long*)&arr[r0], (unsigned long long)v);
    } else if (act) {
        atomicAdd((unsigned long long*)&arr[r], (unsigned long long)(((uint64_t)hi_bit << 32) | (uint64_t)lo_bit));
    }
}

__device__ __forceinline__ void or_count(int* arr, uint32_t r, bool act, int lane) {
    const uint64_t m = __ballot(act);
    if (!m) return;
    uint32_t r0;
    int first;
    if (or_uniform(r, act, m, r0, first)) {
        if (lane == first) atomicAdd(&arr[r0], (int)__popcll((unsigned long long)m));
    } else if (act) {
        atomicAdd(&arr[r], 1);
    }
}

__device__ __forceinline__ float or_canon(float v) { return v == 0.f ? 0.f : v; }   // -0 and +0 compare equal as fp32

__global__ __launch_bounds__(kOrThreads) void orient_init_kernel(uint32_t total, int C, const int* __restrict__ off,
                                                                 const float* __restrict__ nrm, uint32_t* __restrict__ P,
                                                                 uint32_t* __restrict__ H, uint64_t* __restrict__ best1,
                                                                 uint32_t* __restrict__ best2, uint64_t* __restrict__ k1,
                                                                 uint64_t* __restrict__ k2, uint64_t* __restrict__ cnt,
                                                                 uint32_t* __restrict__ low, int* __restrict__ cid, unsigned char* __restrict__ dead,
                                                                 int* __restrict__ status) {
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    if (x >= total) return;
    int lo = 0, hi = C;                                                         // the segment with off[lo] <= x < off[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)off[mid] <= x) lo = mid; else hi = mid;
    }
    cid[x] = lo;
    dead[x] = 0;
    P[x] = x << 1;
    H[x] = kOrNone;
    best1[x] = kOrNoKey;
    best2[x] = kOrNone;
    k1[x] = 0ull;
    k2[x] = 0ull;
    cnt[x] = 0ull;
    low[x] = kOrNone;
    const float a = nrm[(size_t)x * 3 + 0], b = nrm[(size_t)x * 3 + 1], c = nrm[(size_t)x * 3 + 2];
    if (!(__builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c))) atomicOr(&status[lo], kOrBadNormal);
}

// Propose, first pass: one thread per ROW takes the minimum key1 over its own k slots in registers and offers it to its own root: one
// atomic per row at most, not one per slot.  first: also the range check of the indices.
__global__ __launch_bounds__(kOrThreads) void orient_propose_own_kernel(uint32_t total, int k, const int* __restrict__ off,
                                                                        const int* __restrict__ cid, const int* __restrict__ nbr,
                                                                        const float* __restrict__ nrm, const uint32_t* __restrict__ P,
                                                                        uint64_t* __restrict__ best1, unsigned char* __restrict__ dead,
                                                                        const int* __restrict__ live_prev, int* __restrict__ status,
                                                                        int first) {
    if (live_prev && *live_prev == 0) return;                                   // the round before hooked nothing: the forest is complete
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t u = blockIdx.x * kOrThreads + threadIdx.x;
    uint64_t best = kOrNoKey;
    uint32_t ru = 0;
    if (u < total && !dead[u]) {
        const int c = cid[u];
        const int base = off[c], nc = off[c + 1] - base;
        ru = P[u] >> 1;
        const float ux = nrm[(size_t)u * 3 + 0], uy = nrm[(size_t)u * 3 + 1], uz = nrm[(size_t)u * 3 + 2];
        const int* __restrict__ row = nbr + (size_t)u * k;
        bool bad = false;
#pragma unroll 8
        for (int j = 0; j < k; ++j) {
            const int v = row[j];
            bad |= v < -1 || v >= nc;
            const uint32_t gv = (uint32_t)base + (uint32_t)v;
            if (v >= 0 && v < nc && gv != u && (P[gv] >> 1) != ru) {
                const float* q = nrm + (size_t)gv * 3;
                const float s = ux * q[0] + uy * q[1];                          // or_dot's operations in or_dot's order
                const float dot = s + uz * q[2];
                const float w = fmaxf(0.f, 1.f - fabsf(dot));
                const uint64_t key1 = ((uint64_t)__float_as_uint(w) << 32) | (uint64_t)min(u, gv);
                best = key1 < best ? key1 : best;
            }
        }
        if (first && bad) atomicOr(&status[c], kOrBadIndex);
        if (best == kOrNoKey) dead[u] = 1;                                      // every slot ends inside the row's own component: for good
    }
    or_min_u64(best1, ru, best, best != kOrNoKey, lane);
}

// One thread per SLOT.  PASS 0: key1 to the OTHER end's root -- after the pass above that root's table already holds the minimum over
// its own rows, so the load in front of the atomic turns nearly every offer away (only an edge that the other end does not list itself
// can still lower it);  PASS 1: max(u, v) to the roots whose key1 this slot holds.
template <int PASS>
__global__ __launch_bounds__(kOrThreads) void orient_propose_kernel(uint32_t nslots, int k, const int* __restrict__ off,
                                                                    const int* __restrict__ cid, const int* __restrict__ nbr,
                                                                    const float* __restrict__ nrm, const uint32_t* __restrict__ P,
                                                                    uint64_t* __restrict__ best1, uint32_t* __restrict__ best2,
                                                                    const unsigned char* __restrict__ dead,
                                                                    const int* __restrict__ live_prev) {
    if (live_prev && *live_prev == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t t = blockIdx.x * kOrThreads + threadIdx.x;
    bool cross = false;
    uint32_t rlo = 0, rhi = 0, hi = 0, other = 0;
    uint64_t key1 = kOrNoKey;
    const uint32_t u = t / (uint32_t)k;
    if (t < nslots && !dead[u]) {
        const int c = cid[u];
        const int base = off[c], nc = off[c + 1] - base;
        const int v = nbr[t];
        const uint32_t gv = (uint32_t)base + (uint32_t)v;
        if (v >= 0 && v < nc && gv != u) {
            const uint32_t ru = P[u] >> 1, rv = P[gv] >> 1;
            if (ru != rv) {
                cross = true;
                const float dot = or_dot(nrm, u, gv);
                const float w = fmaxf(0.f, 1.f - fabsf(dot));
                key1 = ((uint64_t)__float_as_uint(w) << 32) | (uint64_t)min(u, gv);
                hi = max(u, gv);
                rlo = min(ru, rv);
                rhi = max(ru, rv);
                other = rv;
            }
        }
    }
    if (PASS == 0) {
        or_min_u64(best1, other, key1, cross, lane);
    } else {
        const bool mlo = cross && best1[rlo] == key1, mhi = cross && best1[rhi] == key1;
        or_min_u32(best2, rlo, hi, mlo, lane);
        or_min_u32(best2, rhi, hi, mhi, lane);
    }
}

__global__ __launch_bounds__(kOrThreads) void orient_hook_kernel(uint32_t total, const float* __restrict__ nrm, const uint32_t* __restrict__ P,
                                                                 uint32_t* __restrict__ H, const uint64_t* __restrict__ best1,
                                                                 const uint32_t* __restrict__ best2, const int* __restrict__ live_prev,
                                                                 int* __restrict__ live_cur) {
    if (live_prev && *live_prev == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    bool hooked = false;
    if (x < total && (P[x] >> 1) == x) {
        const uint64_t b1 = best1[x];
        const uint32_t lo = (uint32_t)b1, hi = best2[x];
        if (b1 != kOrNoKey && hi < total && lo < total) {
            const uint32_t s = or_dot(nrm, lo, hi) < 0.f ? 1u : 0u;
            const uint32_t plo = P[lo], phi = P[hi];
            const bool lo_mine = (plo >> 1) == x;
            const uint32_t pa = lo_mine ? plo : phi, pb = lo_mine ? phi : plo;  // a: the end inside this component, b: the other
            const uint32_t rb = pb >> 1;
            const bool mutual = best1[rb] == b1 && best2[rb] == hi;              // both chose this edge: the lower root stays
            if (rb != x && !(mutual && x < rb)) {
                H[x] = (rb << 1) | (((pa ^ pb) & 1u) ^ s);
                hooked = true;
            }
        }
    }
    const uint64_t m = __ballot(hooked);
    if (m && lane == __ffsll((unsigned long long)m) - 1) atomicAdd(live_cur, (int)__popcll((unsigned long long)m));
}

__global__ __launch_bounds__(kOrThreads) void orient_apply_kernel(uint32_t total, uint32_t* __restrict__ P, uint32_t* __restrict__ H,
                                                                  uint64_t* __restrict__ best1, uint32_t* __restrict__ best2,
                                                                  const int* __restrict__ live_cur) {
    if (*live_cur == 0) return;
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    if (x >= total) return;
    const uint32_t h = H[x];
    if (h != kOrNone) {
        P[x] = h;
        H[x] = kOrNone;
    }
    if (best1[x] != kOrNoKey) {
        best1[x] = kOrNoKey;
        best2[x] = kOrNone;
    }
}

__global__ __launch_bounds__(kOrThreads) void orient_jump_kernel(uint32_t total, uint32_t* P, const int* __restrict__ live_cur,
                                                                 const int* __restrict__ flag_prev, int* __restrict__ flag_cur,
                                                                 const int* __restrict__ cid, int* __restrict__ status, int last) {
    if (*live_cur == 0) return;
    if (flag_prev && *flag_prev == 0) return;                                   // the launch before left every word at its root
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    if (x >= total) return;
    const uint32_t w = or_ld(&P[x]);
    uint32_t p = w >> 1, par = w & 1u;
    bool done = false;
    for (int it = 0; it < kOrJumpIters; ++it) {                                 // bounded: never spins
        if (p == x) { done = true; break; }
        const uint32_t wp = or_ld(&P[p]);
        const uint32_t q = wp >> 1;
        if (q == p) { done = true; break; }
        p = q;
        par ^= wp & 1u;
    }
    if (!done) done = p == x || (or_ld(&P[p]) >> 1) == p;
    const uint32_t nw = (p << 1) | par;
    if (nw != w) or_st(&P[x], nw);
    if (!done) {
        *flag_cur = 1;                                                          // every writer stores the same value
        if (last) atomicOr(&status[cid[x]], kOrCap);
    }
}

__global__ __launch_bounds__(kOrThreads) void orient_finish1_kernel(uint32_t total, const float* __restrict__ pts, const float* __restrict__ nrm,
                                                                    const uint32_t* __restrict__ P, const int* __restrict__ cid,
                                                                    uint64_t* __restrict__ k1, uint64_t* __restrict__ cnt,
                                                                    uint32_t* __restrict__ low, int* __restrict__ ncomp) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    const bool act = x < total;
    uint32_t r = 0, rel = 0, c = 0;
    uint64_t key = 0;
    bool nz = false;
    if (act) {
        const uint32_t w = P[x];
        r = w >> 1;
        rel = w & 1u;
        c = (uint32_t)cid[x];
        key = ((uint64_t)f32_to_ordered(or_canon(pts[(size_t)x * 3 + 2])) << 32) | (uint64_t)f32_to_ordered(or_canon(pts[(size_t)x * 3 + 1]));
        nz = nrm[(size_t)x * 3 + 0] != 0.f || nrm[(size_t)x * 3 + 1] != 0.f || nrm[(size_t)x * 3 + 2] != 0.f;
    }
    or_max_u64(k1, r, key, act, lane);
    or_min_u32(low, r, x, act, lane);
    or_add2(cnt, r, act && nz && rel, act && nz && !rel, lane);
    or_count(ncomp, c, act && r == x, lane);
}

__global__ __launch_bounds__(kOrThreads) void orient_finish2_kernel(uint32_t total, const float* __restrict__ pts, const uint32_t* __restrict__ P,
                                                                    const uint64_t* __restrict__ k1, uint64_t* __restrict__ k2) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    bool act = false;
    uint32_t r = 0;
    uint64_t key = 0;
    if (x < total) {
        r = P[x] >> 1;
        const uint64_t mine = ((uint64_t)f32_to_ordered(or_canon(pts[(size_t)x * 3 + 2])) << 32) | (uint64_t)f32_to_ordered(or_canon(pts[(size_t)x * 3 + 1]));
        act = mine == k1[r];
        key = ((uint64_t)f32_to_ordered(or_canon(pts[(size_t)x * 3 + 0])) << 32) | (uint64_t)(kOrNone - x);   // largest x, then the lowest row
    }
    or_max_u64(k2, r, key, act, lane);
}

__global__ __launch_bounds__(kOrThreads) void orient_finish3_kernel(uint32_t total, const int* __restrict__ off, const int* __restrict__ cid,
                                                                    const float* __restrict__ nrm, const uint32_t* __restrict__ P,
                                                                    const uint64_t* __restrict__ k2, const uint64_t* __restrict__ cnt,
                                                                    const uint32_t* __restrict__ low, const int* __restrict__ ncomp, int vote,
                                                                    const int* __restrict__ status, float* __restrict__ normal_out,
                                                                    unsigned char* __restrict__ flip, int* __restrict__ component,
                                                                    int* __restrict__ n_components) {
    const uint32_t x = blockIdx.x * kOrThreads + threadIdx.x;
    if (x >= total) return;
    const int c = cid[x];
    if (status[c] != 0) return;                                                 // nothing is written for a flagged segment
    const uint32_t base = (uint32_t)off[c];
    if (x == base && n_components) n_components[c] = ncomp[c];
    const uint32_t w = P[x];
    const uint32_t r = w >> 1;
    const uint32_t a = min(kOrNone - (uint32_t)k2[r], total - 1);               // the anchor (the clamp never acts on a complete pass 2)
    const float ax = nrm[(size_t)a * 3 + 0], ay = nrm[(size_t)a * 3 + 1], az = nrm[(size_t)a * 3 + 2];
    const uint32_t f0 = (az != 0.f ? az < 0.f : ay != 0.f ? ay < 0.f : ax < 0.f) ? 1u : 0u;
    uint32_t t = (P[a] & 1u) ^ f0;                                              // flip[x] = parity(x -> root) ^ t
    if (vote == 1) {
        const uint64_t cc = cnt[r];
        const uint32_t c1 = (uint32_t)(cc >> 32), c0 = (uint32_t)cc;            // non-zero normals at parity 1 / 0 to the root
        const uint32_t mine = t ? c0 : c1, other = t ? c1 : c0;                 // flips under t and under its complement
        if (other < mine) t ^= 1u;
    }
    const uint32_t f = (w & 1u) ^ t;
    const float nx = nrm[(size_t)x * 3 + 0], ny = nrm[(size_t)x * 3 + 1], nz = nrm[(size_t)x * 3 + 2];
    normal_out[(size_t)x * 3 + 0] = f ? -nx : nx;
    normal_out[(size_t)x * 3 + 1] = f ? -ny : ny;
    normal_out[(size_t)x * 3 + 2] = f ? -nz : nz;
    if (flip) flip[x] = (unsigned char)f;
    if (component) component[x] = (int)(low[r] - base);
}

struct OrLayout {
    int *live, *jflag, *ncomp, *cid;
    unsigned char* dead;
    uint32_t *P, *H, *best2, *low;
    uint64_t *best1, *k1, *k2, *cnt;
    size_t head_bytes, bytes;
};

static OrLayout or_layout(int C, size_t total, char* base) {
    OrLayout L;
    Carver cv{base};
    L.live = cv.ptr<int>((size_t)(kOrMaxRounds + kOrMaxRounds * kOrJumpLaunches + C) * 4);   // zero-filled together
    L.jflag = L.live + kOrMaxRounds;
    L.ncomp = L.jflag + kOrMaxRounds * kOrJumpLaunches;
    L.head_bytes = cv.off;
    L.best1 = cv.ptr<uint64_t>(total * 8);
    L.k1 = cv.ptr<uint64_t>(total * 8);
    L.k2 = cv.ptr<uint64_t>(total * 8);
    L.cnt = cv.ptr<uint64_t>(total * 8);
    L.P = cv.ptr<uint32_t>(total * 4);
    L.H = cv.ptr<uint32_t>(total * 4);
    L.best2 = cv.ptr<uint32_t>(total * 4);
    L.low = cv.ptr<uint32_t>(total * 4);
    L.cid = cv.ptr<int>(total * 4);
    L.dead = cv.ptr<unsigned char>(total);
    L.bytes = cv.off;
    return L;
}

// 0, or hipErrorInvalidValue; *nmax = the largest segment
static int or_check(int C, const int* off_host, int k, int* nmax) {
    const int rc = cells_batch_check(C, off_host, nmax);
    if (rc != 0) return rc;
    if (k < 4 || k > 32 || (long long)off_host[C] * k >= (1ll << 31)) return (int)hipErrorInvalidValue;
    return 0;
}

// phase timing for profile_host: device events around a phase, the elapsed time added to a slot (synchronises)
struct OrProf {
    float* out;
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int init() {
        if (!out) return 0;
        DISPU_TRY(hipEventCreate(&e0));
        DISPU_TRY(hipEventCreate(&e1));
        return 0;
    }
    int begin() { return out ? (int)hipEventRecord(e0, st) : 0; }
    int end(int slot) {
        if (!out) return 0;
        DISPU_TRY(hipEventRecord(e1, st));
        DISPU_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        DISPU_TRY(hipEventElapsedTime(&ms, e0, e1));
        out[slot] += ms;
        return 0;
    }
    ~OrProf() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_orient_consistent_scratch_bytes(int C, const int* off_host, int k) {
    int nmax = 0;
    if (or_check(C, off_host, k, &nmax) != 0) return 0;
    return or_layout(C, (size_t)off_host[C], nullptr).bytes;
}

DISPU_EXPORT int dispu_orient_consistent_segments(int C, const int* off, const int* off_host, int k, const float* points,
                                                  const float* normal_in, const int* neighbors, int vote, int flags, float* normal_out,
                                                  unsigned char* flip, int* component, int* n_components, int* status, void* scratch,
                                                  size_t scratch_bytes, float* profile_host, void* stream) {
    int nmax = 0;
    const int rc = or_check(C, off_host, k, &nmax);
    if (rc != 0) return rc;
    if (!off || !points || !normal_in || !neighbors || !normal_out || !status || normal_out == normal_in || vote < 0 || vote > 1 ||
        (flags & ~DISPU_ORIENT_HOST_ROUNDS) != 0)
        return (int)hipErrorInvalidValue;
    const uint32_t total = (uint32_t)off_host[C];
    const OrLayout L = or_layout(C, total, (char*)scratch);
    if (!scratch_ok(scratch, scratch_bytes, L.bytes)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nslots = total * (uint32_t)k;
    const dim3 block(kOrThreads), gn((total + kOrThreads - 1) / kOrThreads), gs((nslots + kOrThreads - 1) / kOrThreads);
    int rounds = 0;
    while ((1 << rounds) < nmax) ++rounds;                                      // ceil(log2 n_max) <= 24
    OrProf prof{profile_host, st};
    if (profile_host)
        for (int i = 0; i < DISPU_ORIENT_PROFILE_FLOATS; ++i) profile_host[i] = 0.f;
    const int pi = prof.init();
    if (pi != 0) return pi;

    DISPU_TRY((hipError_t)prof.begin());
    DISPU_TRY(hipMemsetAsync(L.live, 0, L.head_bytes, st));
    DISPU_TRY(hipMemsetAsync(status, 0, (size_t)C * 4, st));
    hipLaunchKernelGGL(orient_init_kernel, gn, block, 0, st, total, C, off, normal_in, L.P, L.H, L.best1, L.best2, L.k1, L.k2, L.cnt, L.low,
                       L.cid, L.dead, status);
    DISPU_CHECK_LAUNCH();
    DISPU_TRY((hipError_t)prof.end(1));

    int launched = 0;
    for (int r = 0; r < rounds; ++r) {
        const int* prev = r ? L.live + r - 1 : nullptr;
        int* cur = L.live + r;
        DISPU_TRY((hipError_t)prof.begin());
        hipLaunchKernelGGL(orient_propose_own_kernel, gn, block, 0, st, total, k, off, L.cid, neighbors, normal_in, L.P, L.best1, L.dead, prev, status,
                           r == 0 ? 1 : 0);
        hipLaunchKernelGGL((orient_propose_kernel<0>), gs, block, 0, st, nslots, k, off, L.cid, neighbors, normal_in, L.P, L.best1, L.best2, L.dead,
                           prev);
        hipLaunchKernelGGL((orient_propose_kernel<1>), gs, block, 0, st, nslots, k, off, L.cid, neighbors, normal_in, L.P, L.best1, L.best2, L.dead,
                           prev);
        DISPU_CHECK_LAUNCH();
        DISPU_TRY((hipError_t)prof.end(2));
        DISPU_TRY((hipError_t)prof.begin());
        hipLaunchKernelGGL(orient_hook_kernel, gn, block, 0, st, total, normal_in, L.P, L.H, L.best1, L.best2, prev, cur);
        hipLaunchKernelGGL(orient_apply_kernel, gn, block, 0, st, total, L.P, L.H, L.best1, L.best2, cur);
        DISPU_CHECK_LAUNCH();
        DISPU_TRY((hipError_t)prof.end(3));
        ++launched;
        if (flags & DISPU_ORIENT_HOST_ROUNDS) {                                 // one 4-byte read-back: this round hooked nothing, stop here
            int h = 0;
            DISPU_TRY(hipMemcpyAsync(&h, cur, 4, hipMemcpyDeviceToHost, st));
            DISPU_TRY(hipStreamSynchronize(st));
            if (h == 0) break;
        }
        DISPU_TRY((hipError_t)prof.begin());
        for (int j = 0; j < kOrJumpLaunches; ++j) {
            int* fl = L.jflag + r * kOrJumpLaunches + j;
            hipLaunchKernelGGL(orient_jump_kernel, gn, block, 0, st, total, L.P, cur, j ? fl - 1 : nullptr, fl, L.cid, status,
                               j == kOrJumpLaunches - 1 ? 1 : 0);
        }
        DISPU_CHECK_LAUNCH();
        DISPU_TRY((hipError_t)prof.end(4));
    }

    DISPU_TRY((hipError_t)prof.begin());
    hipLaunchKernelGGL(orient_finish1_kernel, gn, block, 0, st, total, points, normal_in, L.P, L.cid, L.k1, L.cnt, L.low, L.ncomp);
    hipLaunchKernelGGL(orient_finish2_kernel, gn, block, 0, st, total, points, L.P, L.k1, L.k2);
    hipLaunchKernelGGL(orient_finish3_kernel, gn, block, 0, st, total, off, L.cid, normal_in, L.P, L.k2, L.cnt, L.low, L.ncomp, vote, status,
                       normal_out, flip, component, n_components);
    DISPU_CHECK_LAUNCH();
    DISPU_TRY((hipError_t)prof.end(5));
    if (profile_host) {                                                         // rounds that hooked something, and the rounds issued
        int live[kOrMaxRounds];
        DISPU_TRY(hipMemcpyAsync(live, L.live, sizeof(live), hipMemcpyDeviceToHost, st));
        DISPU_TRY(hipStreamSynchronize(st));
        int took = 0;
        for (int r = 0; r < rounds; ++r) took += live[r] > 0;
        profile_host[0] = (float)took;
        profile_host[6] = (float)launched;
    }
    return (int)hipGetLastError();
}
