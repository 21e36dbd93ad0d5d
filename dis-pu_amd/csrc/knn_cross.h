// The host side of an entry that searches one packed batch from another (attributes.hip, mls_project.hip, signed_distance.hip, icp.hip): the two
// Morton-cell pre-passes, their regions at the front of the caller's scratch -- references first, then queries, then whatever the
// operator adds behind -- and the launch grid.  The device side is knn_cross_prologue.h.  Host only: nothing of it is a kernel argument.
#pragma once
#include "knn_cells.h"

namespace dispu {

struct CrossPrepass {
    int C, rc;                                                                  // rc: what cells_batch_check says of the two offset tables
    const int *qoff_host, *roff_host;
    size_t rbytes = 0, qbytes = 0;                                              // multiples of 256, both 0 when either side is refused
    const float4 *rspt = nullptr, *qspt = nullptr;
    const float *rtab = nullptr, *qtab = nullptr;
    const uint32_t *rsegb = nullptr, *qsegb = nullptr;
    int kqmax = 0;

    CrossPrepass(int C, const int* qoff_host, const int* roff_host)
        : C(C), rc(cells_batch_check(C, qoff_host)), qoff_host(qoff_host), roff_host(roff_host) {
        if (rc == 0) rc = cells_batch_check(C, roff_host);
        if (rc != 0) return;
        rbytes = fps_cells_prepass_scratch(C, roff_host);
        qbytes = fps_cells_prepass_scratch(C, qoff_host);
    }
    size_t bytes() const { return rbytes + qbytes; }
    // whether `scratch` holds the two regions and `extra` bytes behind them
    bool fits(const void* scratch, size_t scratch_bytes, size_t extra = 0) const {
        return rc == 0 && scratch_ok(scratch, scratch_bytes, bytes() + extra);
    }
    int run_refs(const int* roff, const float* refs, void* scratch, hipStream_t st) {
        int kr = 0;
        return fps_cells_prepass(C, roff, roff_host, refs, scratch, rbytes, &rspt, &rtab, &rsegb, &kr, st);
    }
    int run_queries(const int* qoff, const float* queries, void* scratch, hipStream_t st) {   // again for every set of positions searched from
        return fps_cells_prepass(C, qoff, qoff_host, queries, (char*)scratch + rbytes, qbytes, &qspt, &qtab, &qsegb, &kqmax, st);
    }
    dim3 grid() const { return dim3((kqmax + kNrmWaves - 1) / kNrmWaves, C); }  // after run_queries: one wave per query cell
};

}  // namespace dispu
