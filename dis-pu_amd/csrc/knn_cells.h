// The exact cell-pruned k-NN search over the Morton cells of morton_cells.hip, shared by its clients (normals.hip: the PCA normals;
// outliers.hip: the mean neighbour distance, the radius count; attributes.hip, mls_project.hip, signed_distance.hip: the search from one
// cloud into another): here the sorted-register candidate list and the box bound.  The search itself -- the list, the visit, the
// Morton-offset ramp around a start cell, then the box-table walk -- exists once, in knn_cells_search.h, included as text inside each
// kernel; likewise once the prologue of the kernels that search their own segment (segment, cell, query), in knn_cells_prologue.h, and
// that of the kernels that search another cloud (segment pair, query cell, query, seed cell), in knn_cross_prologue.h, whose host side
// (two pre-passes, the scratch they share, the grid) is knn_cross.h.
// normals.hip's header comment describes the search and proves why a skip is sound; cell_box_lb below is the bound it speaks of.
#pragma once
#include "morton_cells.h"

namespace dispu {

constexpr int kNrmThreads = 256, kNrmWaves = kNrmThreads / kWave, kNrmCell = 64;
constexpr uint64_t kNrmNone = ~0ull;
static_assert(kNrmCell == kFpcMinCell && kNrmCell == kWave, "kCellsFixed64: one query per lane, the cell table indexed as the pre-pass wrote it");

template <int KMAX>
struct NrmBest {
    uint64_t b[KMAX];
    uint64_t thr;                                                     // b[k - 1]: the lane's current k-th key
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) b[j] = kNrmNone;
        thr = kNrmNone;
    }
    __device__ __forceinline__ void push(uint64_t key, int k) {
        if (key < thr) {
#pragma unroll
            for (int j = KMAX - 1; j > 0; --j) b[j] = key < b[j - 1] ? b[j - 1] : (key < b[j] ? key : b[j]);
            b[0] = key < b[0] ? key : b[0];
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j == k - 1) thr = b[j];
        }
    }
    // the two halves of key j: the point's local index, its d2
    __device__ __forceinline__ uint32_t index(int j) const { return (uint32_t)b[j]; }
    __device__ __forceinline__ float d2(int j) const { return __uint_as_float((uint32_t)(b[j] >> 32)); }
    // (the d2 of a rank that is no constant -- the k'-th of mls_project_kernel and signed_distance_kernel -- stays a loop written out in
    // those kernels: as a method or a function here it changed both kernels' register allocation)
};

// lower bound of d2 between any point of the box (lo, hi) and any point of the cell whose table row is (a, b) = (lo x3, hi.x | hi.y,
// hi.z, -, -): lb <= d2 bit for bit (normals.hip); a query point is the box lo = hi = q.  knn_cells_search.h spells the same operations
// out instead of calling this: with the call, the six shuffles of the per-lane bound issue in another order and the normals and mean-distance
// kernels compile to other machine code than the measured one; the seed sweep of knn_cross_prologue.h and the radius count call it
__device__ __forceinline__ float cell_box_lb(const float4& a, const float4& b, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float ex = fmaxf(fmaxf(a.x - hx, lx - a.w), 0.f);
    const float ey = fmaxf(fmaxf(a.y - hy, ly - b.x), 0.f);
    const float ez = fmaxf(fmaxf(a.z - hz, lz - b.y), 0.f);
    return sqdist3<false>(ex, ey, ez);
}

}  // namespace dispu
