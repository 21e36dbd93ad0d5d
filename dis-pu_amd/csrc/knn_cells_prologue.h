// The prologue of a kernel that searches a segment's own Morton cells (pca_normals_kernel, knn_mean_dist_kernel, radius_count_kernel):
// which segment, which cell, which query.  Included as TEXT at the top of the kernel body, like knn_cells_search.h and for its reason: a
// helper that returned these values in a struct cost four VGPRs across the search (98 for 94 at KMAX 16, a wave of occupancy).
//
// Reads the kernel's parameters (grid: cells / kNrmWaves x segments, kNrmThreads threads):
//   const int* off             the segments' device offsets                const uint32_t* segb   the pre-pass's segment words
//   const float4* spt          its sorted points                           const float* tab       its cell table
//   int* status                [C]: 1 for a segment with a non-finite coordinate, else 0 (written here)
// Returns from the kernel for such a segment (nothing else is written for it) and for a wave beyond the segment's cells.  Defines:
//   int c, tid, lane, wave     segment, thread, lane, wave (uniform)       int b0, n; size_t base   the segment's first row and points
//   int K, cb                  the segment's cells, the wave's own cell    const float4* sp; const float* gt   the segment's sorted points, table rows
//   int qcnt; bool valid       queries of the cell; lane < qcnt            float4 q                 the lane's query (idle lanes repeat query 0)
//   float4 qlo4, qhi4          the own cell's table row: lo x3, hi.x | hi.y, hi.z, -, -
// No include guard on purpose: once per kernel.
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = off[c], n = off[c + 1] - b0;
    const size_t base = (size_t)b0;
    const uint32_t bad = segb[(size_t)c * 8 + 6];
    if (blockIdx.x == 0 && tid == 0) status[c] = bad ? 1 : 0;
    if (bad) return;                                                            // nothing is written for a non-finite segment
    const int K = (n + kNrmCell - 1) / kNrmCell;
    const int cb = blockIdx.x * kNrmWaves + wave;
    if (cb >= K) return;                                                        // wave-uniform
    const float4* __restrict__ sp = spt + base;
    const float* __restrict__ gt = tab + fpc_cell_base(base, c) * 8;
    const int qcnt = min(kNrmCell, n - cb * kNrmCell);
    const bool valid = lane < qcnt;
    const float4 q = sp[cb * kNrmCell + (valid ? lane : 0)];                    // idle lanes repeat query 0 and store nothing
    const float4 qlo4 = *reinterpret_cast<const float4*>(gt + (size_t)cb * 8);
    const float4 qhi4 = *reinterpret_cast<const float4*>(gt + (size_t)cb * 8 + 4);
