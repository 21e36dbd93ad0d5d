// What the Morton-cell pre-pass (morton_cells.hip) leaves behind, for the kernels that read it (fps_cells.hip, normals.hip): the cell
// sizes, where a segment's cells start in the cell table, which segments a mode serves, and the layout of the scratch.
#pragma once
#include "internal.h"

namespace dispu {

constexpr int kFpcMinCell = 64, kFpcMaxCell = 4096, kFpcMaxCells = 4096;
constexpr int kFpcMaxN = kFpcMaxCell * kFpcMaxCells;          // 2^24 points per segment

// cell size of a segment of n points: the smallest power of two >= 64 that gives at most 4096 cells, or `cell` when that is larger
__host__ __device__ __forceinline__ int fpc_cell_size(int n, int cell) {
    int s = kFpcMinCell;
    while ((n + s - 1) / s > kFpcMaxCells) s <<= 1;
    return s > cell ? s : cell;
}
// first cell of segment c in the cell table: every segment has at most n_c / 64 + 1 cells
__device__ __forceinline__ size_t fpc_cell_base(size_t base, int c) { return base / kFpcMinCell + (size_t)c; }
__host__ __device__ __forceinline__ bool fpc_served(int n, int m, CellsMode mode) { return mode != kCellsAuto || fps_cells_rule(n, m); }
__host__ __device__ __forceinline__ int fpc_cell_size_mode(int n, int cell, CellsMode mode) {
    return mode == kCellsFixed64 ? kFpcMinCell : fpc_cell_size(n, cell);
}

// the sorter's key / value buffers die with the sort: the sorted points reuse both key buffers, the running distances the input values
struct FpcScratch {
    size_t kin, kout, vin, vout, sort, sort_bytes, tab, segb, total;
};

}  // namespace dispu
