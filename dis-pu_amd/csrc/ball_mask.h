// The ball query's hit decision for a wave that holds 64 candidates per block, one per lane (csrc/grouping.hip: the wave-per-query
// kernels; csrc/uniform_loss.hip: the balls of get_uniform_loss).
// hit <=> max(sqrtf(d2), 1e-20f) < radius (tf_grouping_g.cu:20-27), decided WITHOUT the correctly rounded square root for all but the
// candidates within 4e-6 (relative) of radius^2: sqrt is monotone and correctly rounded, radius^2 is rounded once, so d2 below
// r2 (1 - 2^-18) is a hit and d2 above r2 (1 + 2^-18) is a miss whatever the roundings; a wave computes the exact form only when one
// of its lanes falls into that band (or is unordered: NaN coordinates take the reference's path).  The square root with its fix-up
// was ~2/3 of the instructions of a candidate.
#pragma once
#include "common.h"

namespace dispu {

struct QbBand {
    float rad, lo, hi;
    bool always_exact;
};
__device__ __forceinline__ QbBand qb_band(float rad) {
    const float r2 = rad * rad;
    return QbBand{rad, r2 * (1.0f - 3.8146973e-6f), r2 * (1.0f + 3.8146973e-6f), !(rad > 1e-19f) || !(r2 > 1e-30f) || !(r2 < 1e30f)};
}
// The hit masks of R 64-candidate blocks at once: R independent compares and ballots, ONE band test for all of them (block by block
// a query was a chain of scalar branches, each waiting for a vector compare).
template <int R>
__device__ __forceinline__ void qb_masks(const QbBand& b, const float (&d2)[R], int base, int lane, int n, unsigned long long (&mk)[R]) {
    // every predicate is a vector compare written straight to a scalar mask; the rest is scalar logic (as per-lane bools the masks cost
    // ~6 vector instructions per block on top of the distance: 450 vector instructions per query, which is what bounded the kernel)
    unsigned long long band = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        mk[r] = __ballot(d2[r] < b.lo);
        band |= ~mk[r] & __ballot(!(d2[r] > b.hi));                      // includes unordered (NaN) distances
    }
    if (b.always_exact || band) {                                        // wave-uniform, rare
#pragma unroll
        for (int r = 0; r < R; ++r) mk[r] = __ballot(fmaxf(sqrtf(d2[r]), 1e-20f) < b.rad);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {                                        // candidates past n (clamped loads): masked out, scalar
        const int left = n - (base + 64 * r);
        mk[r] &= left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
    }
}

}  // namespace dispu
