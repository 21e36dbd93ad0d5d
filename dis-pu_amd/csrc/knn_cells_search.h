// The body of the exact cell-pruned k-NN search (knn_cells.h), included as TEXT inside a kernel template <int KMAX>: not a header in its
// own right.  As a __forceinline__ function -- with the list passed by reference (more registers: 98 for 94 VGPRs at KMAX 16), or returned
// by value (the same register counts) -- the same statements compiled to a normals kernel 2 - 8 % slower on single clouds of 8192 ..
// 1228800 points (and 6 % faster on 64 x 8192) than the form written out in the kernel, the two measured alternately in one run (DESIGN
// section 9).  Textual inclusion leaves the normals kernels' machine code exactly as it was.
//
// The one copy of the search: the kernels that search a segment's own cells (normals.hip, outliers.hip) start it at the wave's own cell,
// s = cb after knn_cells_prologue.h; knn_cross_kernel (attributes.hip), whose queries come from another cloud, at the cell its seed
// sweep picked.  Whatever s is, every cell outside the ramp [vlo, vhi] goes through the walk, so the result does not depend on it.
//
// Reads, from the including scope (one wave, one query per lane; all but lane and q wave-uniform):
//   const float4* sp   the searched segment's sorted points (x, y, z, local index as bits)   const float* gt   its rows of the cell table
//   int n, K           the searched segment's points and cells                               int s             the start cell, 0 <= s < K
//   float4 q           the lane's query                                                      int lane, k       k: the list length
//   float4 qlo4, qhi4  a box around the wave's 64 queries, as a table row (lo x3, hi.x | hi.y, hi.z, -, -)
// Defines int kp = min(k, n) and NrmBest<KMAX> best: every lane's kp smallest keys (d2 bits << 32 | local index) over the segment,
// ascending.  No include guard on purpose: once per kernel.
    const int kp = min(k, n);
    const float qlx = qlo4.x, qly = qlo4.y, qlz = qlo4.z, qhx = qlo4.w, qhy = qhi4.x, qhz = qhi4.y;

    NrmBest<KMAX> best;
    best.init();
    auto visit = [&](int j) {                                                   // j wave-uniform: all 64 queries against cell j
        const int cnt = min(kNrmCell, n - j * kNrmCell);
        const float4 p = sp[j * kNrmCell + min(lane, cnt - 1)];
        for (int i = 0; i < cnt; ++i) {
            const float px = __shfl(p.x, i, kWave), py = __shfl(p.y, i, kWave), pz = __shfl(p.z, i, kWave);
            const uint32_t pi = (uint32_t)__shfl(__float_as_int(p.w), i, kWave);
            const float d = sqdist3<false>(px - q.x, py - q.y, pz - q.z);
            best.push(((uint64_t)__float_as_uint(d) << 32) | pi, k);
        }
    };
    visit(s);
    int seen = min(kNrmCell, n - s * kNrmCell), vlo = s, vhi = s;
    for (int d = 1; seen < kp; ++d) {                                           // kp <= n: ends at the latest with every cell visited
        if (s - d >= 0) { visit(s - d); seen += kNrmCell; vlo = s - d; }        // only the last cell of a segment is short, and it
        if (s + d < K) { visit(s + d); seen += min(kNrmCell, n - (s + d) * kNrmCell); vhi = s + d; }   // is never at s - d
    }
    uint32_t wk = (uint32_t)(wave_max_u64(best.thr) >> 32);                     // bits of the wave's largest k-th distance
    for (int j0 = 0; j0 < K; j0 += kWave) {
        const int j = j0 + lane;
        uint32_t lbb = 0xFFFFFFFFu;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        const bool open = j < K && (j < vlo || j > vhi);
        if (open) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)j * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)j * 8 + 4);
            const float ex = fmaxf(fmaxf(a.x - qhx, qlx - a.w), 0.f);
            const float ey = fmaxf(fmaxf(a.y - qhy, qly - b.x), 0.f);
            const float ez = fmaxf(fmaxf(a.z - qhz, qlz - b.y), 0.f);
            lbb = __float_as_uint(sqdist3<false>(ex, ey, ez));
        }
        unsigned long long reach = __ballot(open && lbb <= wk);
        while (reach) {
            const int bl = (int)__builtin_ctzll(reach);
            reach &= reach - 1;
            const uint32_t lb1 = (uint32_t)__shfl((int)lbb, bl, kWave);
            if (lb1 > wk) continue;                                             // the k-th distance shrank since the ballot
            // the same bound per lane, the query point as its own box: a cell no lane can gain from is not visited either
            const float ex = fmaxf(fmaxf(__shfl(a.x, bl, kWave) - q.x, q.x - __shfl(a.w, bl, kWave)), 0.f);
            const float ey = fmaxf(fmaxf(__shfl(a.y, bl, kWave) - q.y, q.y - __shfl(b.x, bl, kWave)), 0.f);
            const float ez = fmaxf(fmaxf(__shfl(a.z, bl, kWave) - q.z, q.z - __shfl(b.y, bl, kWave)), 0.f);
            if (!__any(__float_as_uint(sqdist3<false>(ex, ey, ez)) <= (uint32_t)(best.thr >> 32))) continue;
            visit(j0 + bl);
            wk = (uint32_t)(wave_max_u64(best.thr) >> 32);
        }
    }
