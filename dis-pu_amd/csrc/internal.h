// Every function of libdispu_hip.so that is defined in one translation unit and called from another, declared ONCE: the defining file
// and every caller include this header, so the compiler checks each definition and each call against the same prototype (default
// arguments live here only).  Declarations, the sorter's handle and one template; the exported C-ABI is include/dispu_hip.h.
#pragma once
#include <type_traits>

#include "common.h"

namespace dispu {

// ---- train_gemm.hip --------------------------------------------------------------------------------------------------------------------
// the one-shot sink dispu_tn_defer arms for the NEXT TN product on this thread; taking it disarms it
dispu_tn_reduce_desc* tn_take_defer();

// ---- linear_skinny.hip -----------------------------------------------------------------------------------------------------------------
// host only: the unroll depth (2, 8, 16, 24) the register-resident path takes for the shape, or 0 when the shape is outside it
int linear_skinny_rule(int M, int K, int N, const float* X, long ldx, const float* W, long ldw, int transb);
// one launch at the depth linear_skinny_rule returned
int linear_skinny_launch(int ng, int M, int K, int N, const float* X, long ldx, const float* W, long ldw, int transb, const float* bias,
                         int act, float* Y, long ldy, const float* R1, long ldr1, const float* Mk, long ldm, int mcols,
                         hipStream_t st);

// ---- knn_wave.hip: wave-per-query fast paths; the dispatchers return -1 when the shape is outside their range --------------------------
int knn_xyz_wave_dispatch(int b, int n, int m, int k, const float* s, const float* q, int* idx, float* dist, int arith,
                          hipStream_t st);
int knn_feat_wave_dispatch(int b, int n, int m, int c, int k, int ldp, int ldq, const float* p, const float* q, float* dist,
                           int* idx, hipStream_t st, long pstride = 0);
size_t knn_feat_chunked_scratch(int b, int n, int m, int c, int k);
int knn_feat_chunked_dispatch(int b, int n, int m, int c, int k, int ldp, int ldq, const float* p, const float* q, float* dist, int* idx,
                              void* scratch, size_t scratch_bytes, hipStream_t st);
// 1024 < n <= 8192, k <= 32: per-chunk wave kernel + merge; needs caller scratch (1024 < n <= 4096: one pass with the cloud in LDS)
size_t knn_xyz_chunked_scratch(int b, int n, int m, int k);
int knn_xyz_lds_dispatch(int b, int n, int m, int k, const float* s, const float* q, int* idx, float* dist, int arith, hipStream_t st);
int knn_xyz_chunked_dispatch(int b, int n, int m, int k, const float* s, const float* q, int* idx, float* dist, void* scratch,
                             size_t scratch_bytes, int arith, hipStream_t st);

// ---- knn_general.hip -------------------------------------------------------------------------------------------------------------------
// any k <= 4096, c <= 4096, any n; mode 0/1 xyz plain/contract, 2 knn_point, 3 knn_point_2.  off / qoff: a ragged batch of b segments
// (at most n points and m queries each), of which the kernel serves those above seg_nmin points
int knn_general_launch(int mode, int b, int n, int m, int c, int k, long ldp, long ldq, const float* points, const float* queries,
                       float* dist, int* idx, int neg, hipStream_t st, const int* off = nullptr, const int* qoff = nullptr,
                       int seg_nmin = 0);

// ---- grouping.hip ----------------------------------------------------------------------------------------------------------------------
// out[r, :] = points[cloud(r), idx[r], :], rows x c, shared by dispu_group_point and dispu_gather_point (c == 3: 12-byte loads per lane,
// LDS-staged float4 stores)
int launch_gather_rows(size_t rows, int n, int c, size_t rows_per_cloud, const float* points, const int* idx, float* out,
                       hipStream_t st);

// ---- mesh_eval.hip ---------------------------------------------------------------------------------------------------------------------
// the in-place scan of dispu_disk_count, for the other CSR builders
int disk_scan_launch(long long M, long long* offsets, hipStream_t st);

// ---- fps_wave.hip: exact sampling with wave-level skipping for 4096 < n <= 24576, m >= 64 (scratch = the sorted permutation) -----------
bool fps_wave_wants_scratch(int n, int m);
// -1: shape outside this path (or no scratch for the permutation)
int fps_wave_dispatch(int b, int n, int m, const float* xyz, void* temp, int* out, int arith, hipStream_t s);
// off / moff: a ragged batch of b segments of at most n points each, of which the kernels serve those of family 1
int fps_wave_launch(int b, int n, int m, const float* xyz, int* perm, int* out, int arith, hipStream_t s, const int* off, const int* moff);

// ---- radix_sort.hip: the device-wide stable LSD radix sort of (uint64 key, uint32 value) pairs and its three-step scan -----------------
constexpr int kRsThreads = 256, kRsWaves = kRsThreads / kWave;       // the block size of the sorter, its scans and its clients' kernels
size_t scan_blocks(size_t L);                                        // words of `sums` a scan over L words needs
// exclusive scan of data[L] in place; sums: scan_blocks(L) words; the grand total -> *total_out (device, if not null)
int exclusive_scan_u32(uint32_t* data, size_t L, uint32_t* sums, uint32_t* total_out, hipStream_t st);
static inline unsigned rs_blocks(size_t work) { return (unsigned)((work + kRsThreads - 1) / kRsThreads); }   // one lane per item
// The sorter as its in-library clients hold it: both sides of the ping-pong, the histogram table and the scan's block sums.  A client
// writes its pairs to k[0], v[0], calls sort() and reads keys(), vals(); which side that is stays in here.  All four buffers are
// overwritten by a sort and are the client's again afterwards.
struct RadixSorter {
    uint64_t* k[2];
    uint32_t* v[2];
    uint32_t *table, *sums;
    int side = 0;                                    // where the last sort() left its result
    // the regions for n pairs, in the order k[0], k[1], v[0], v[1], table, sums.  THE sizing rule -- table: 256 words per tile of n;
    // sums: scan_blocks of the larger of that and n, so it also serves any scan over up to n words (run_heads_scan)
    void carve(Carver& cv, size_t n);
    // `passes` >= 0 stable 8-bit passes over (k[0], v[0]); 0 leaves the pairs where they are
    int sort(size_t n, int passes, hipStream_t st);
    const uint64_t* keys() const { return k[side]; }
    const uint32_t* vals() const { return v[side]; }
};
// Run numbering over sorted keys: ex[j] = the number of run heads (j == 0 or keys[j] != keys[j - 1]) before position j, the run count
// -> *count (device).  keys == nullptr: all keys are equal, one run.  sums: scan_blocks(n) words (a RadixSorter's do)
int run_heads_scan(const uint64_t* keys, size_t n, uint32_t* ex, uint32_t* sums, uint32_t* count, hipStream_t st);
// The step after it -- start[e] = j at a head, start[the run count] = n, ex[j] -> the number of j's run -- stays written out in its two
// kernels (runs_kernel, pc_cells_kernel): as a shared __forceinline__ function, with or without __restrict__, it changed both kernels' code

// ---- morton_cells.hip: the Morton-cell pre-pass over a packed ragged batch (bounds, keys, ONE sort, cells) -----------------------------
// Which segments the pre-pass (and the sampling kernel behind it) serves, and in what cells.  An int underneath: it is a kernel argument.
enum CellsMode : int {
    kCellsAll = 0,      // every segment, in cells of fpc_cell_size(n, cell) points (dispu_fps_cells)
    kCellsAuto = 1,     // only the segments fps_cells_rule names: family 3 of dispu_fps_segments_auto
    kCellsFixed64 = 2,  // every segment, in cells of exactly 64 points whatever its size (normals.hip: one query per lane of a wave)
};
struct FpcScratch;      // byte offsets of the pre-pass's buffers inside the caller's scratch (morton_cells.h)
// -> 0 and: the largest segment, the largest served segment, the largest cell count of a served segment; or hipErrorInvalidValue
int fpc_plan(int C, const int* off_host, const int* moff_host, int cell, CellsMode mode, int* nall, int* nserved, int* kmax);
FpcScratch fpc_scratch(size_t N, int C);
// The pre-pass alone: bounds, keys, sort, cells.  scratch as fpc_scratch(off_host[C], C) lays it out; afterwards spt (over the two key
// buffers), td (over the input values), tab and segb hold what the kernels of morton_cells.hip describe.  nall / nserved / kmax from
// fpc_plan.
int fpc_prepass(int C, const int* off, const int* moff, const float* inp, char* base, const FpcScratch& s, size_t N, int nall,
                int nserved, int kmax, int cell, CellsMode mode, hipStream_t st);
// bytes of scratch the pre-pass needs for the batch, 0 when it serves no segment (or refuses the offsets)
size_t fps_cells_scratch(int C, const int* off_host, const int* moff_host, int cell, CellsMode mode);
// The pre-pass for a client other than FPS (normals.hip): every segment of the packed batch in cells of exactly 64 sorted points (cell j
// of segment c: sorted positions off[c] + 64 j ...).  -> spt [N] (x, y, z, local index as bits) in sorted order, tab [.][8] the cells'
// boxes (lo x3, hi x3, -, -; segment c's first row is off[c] / 64 + c), segb [C][8] (word 6: the non-finite flag; such a segment has no
// cells), kmax the largest cell count of a segment.  The scratch is refused, untouched, when NULL, misaligned or too small.
size_t fps_cells_prepass_scratch(int C, const int* off_host);
// What every entry over such a batch checks first: fpc_plan for cells of 64 (C in 1 .. 65535, offsets that start at 0 and grow, at most
// 2^24 points per segment) -> 0 and, where asked for, the largest segment and the largest cell count of a segment; or hipErrorInvalidValue
int cells_batch_check(int C, const int* off_host, int* nall = nullptr, int* kmax = nullptr);
// The capacity of the search's register list (knn_cells.h: NrmBest<KMAX>) for a list of k <= 32 keys: f(integral_constant<int, 8 | 16 | 32>)
template <class F>
void dispatch_kmax(int k, F&& f) {
    if (k <= 8)
        f(std::integral_constant<int, 8>{});
    else if (k <= 16)
        f(std::integral_constant<int, 16>{});
    else
        f(std::integral_constant<int, 32>{});
}
int fps_cells_prepass(int C, const int* off, const int* off_host, const float* inp, void* scratch, size_t scratch_bytes,
                      const float4** spt, const float** tab, const uint32_t** segb, int* kmax, hipStream_t st);

// ---- fps_cells.hip ---------------------------------------------------------------------------------------------------------------------
// the pre-pass and the cell-skipping sampling kernel over the segments `mode` names; scratch as fps_cells_scratch sizes it
int fps_cells_run(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* scratch,
                  size_t scratch_bytes, int* out, int* status, int arith, int cell, CellsMode mode, hipStream_t st);

}  // namespace dispu
