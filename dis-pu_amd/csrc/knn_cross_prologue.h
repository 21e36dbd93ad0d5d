// The prologue of a kernel that searches ANOTHER cloud's Morton cells (knn_cross_kernel, mls_project_kernel, signed_distance_kernel,
// icp_accumulate_kernel):
// which pair of segments, which query cell, which query, and the reference cell the search starts at.  Included as TEXT at the top of the
// kernel body, like knn_cells_prologue.h and for its reason.
//
// Reads the kernel's parameters (grid: query cells / kNrmWaves x segments, kNrmThreads threads) -- q*: the pre-pass over the packed
// queries, r*: the one over the packed references:
//   const int* qoff, roff      the segments' device offsets                const uint32_t* qsegb, rsegb   the pre-passes' segment words
//   const float4* qspt, rspt   their sorted points                         const float* qtab, rtab        their cell tables
//   const int* status_in       [C] or NULL: a status word carried in from an earlier step, folded into this one's (a kernel without
//                              one declares `const int* const status_in = nullptr;` before the include)
//   int* status                [C]: 1 for a pair with a non-finite coordinate on either side or a carried word, else 0 (written here)
// Returns from the kernel for such a pair (nothing else is written for it) and for a wave beyond the query segment's cells.  Defines:
//   int c, tid, lane, wave     segment, thread, lane, wave (uniform)       int qb0, nq, rb0, n; size_t qbase, rbase   first rows, points
//   int KQ, K, cb              query cells, reference cells, the wave's query cell
//   const float4* sp; const float* gt, qgt   the REFERENCE segment's sorted points and table rows (what knn_cells_search.h reads), the
//                                            query segment's table rows
//   int qcnt; bool valid       queries of the cell; lane < qcnt            float4 q                 the lane's query (idle lanes repeat query 0)
//   float4 qlo4, qhi4          the query cell's table row: lo x3, hi.x | hi.y, hi.z, -, -
//   int s                      the seed, 0 <= s < K: Morton keys are relative to each segment's own bounds, so a query cell's number says
//                              nothing about the reference cells; one sweep of the reference segment's box table, 64 boxes per step,
//                              finds the cell of the smallest (box-to-box lower bound, cell number)
// Why the search may start anywhere, and why a skip stays sound with the box of a query cell from the other pre-pass: attributes.hip.
// No include guard on purpose: once per kernel.
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qb0 = qoff[c], nq = qoff[c + 1] - qb0;
    const int rb0 = roff[c], n = roff[c + 1] - rb0;
    const size_t qbase = (size_t)qb0, rbase = (size_t)rb0;
    const uint32_t bad = qsegb[(size_t)c * 8 + 6] | rsegb[(size_t)c * 8 + 6] | (status_in ? (uint32_t)status_in[c] : 0u);
    if (blockIdx.x == 0 && tid == 0) status[c] = bad ? 1 : 0;
    if (bad) return;                                                            // nothing is written for a non-finite segment
    const int KQ = (nq + kNrmCell - 1) / kNrmCell, K = (n + kNrmCell - 1) / kNrmCell;
    const int cb = blockIdx.x * kNrmWaves + wave;
    if (cb >= KQ) return;                                                       // wave-uniform
    const float4* __restrict__ sp = rspt + rbase;
    const float* __restrict__ gt = rtab + fpc_cell_base(rbase, c) * 8;
    const float* __restrict__ qgt = qtab + fpc_cell_base(qbase, c) * 8;
    const int qcnt = min(kNrmCell, nq - cb * kNrmCell);
    const bool valid = lane < qcnt;
    const float4 q = qspt[qbase + (size_t)(cb * kNrmCell + (valid ? lane : 0))];   // idle lanes repeat query 0 and store nothing
    const float4 qlo4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8);
    const float4 qhi4 = *reinterpret_cast<const float4*>(qgt + (size_t)cb * 8 + 4);

    // the seed.  Lane 0 always holds cell 0, so s < K
    uint64_t sk = kNrmNone;
    for (int j0 = 0; j0 < K; j0 += kWave) {
        const int j = j0 + lane;
        if (j < K) {
            const float4 a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            const float4 b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            const float lb = cell_box_lb(a, b, qlo4.x, qlo4.y, qlo4.z, qlo4.w, qhi4.x, qhi4.y);
            const uint64_t key = ((uint64_t)__float_as_uint(lb) << 32) | (uint32_t)j;
            sk = key < sk ? key : sk;
        }
    }
    const int s = min((int)(uint32_t)wave_min_u64(sk), K - 1);
