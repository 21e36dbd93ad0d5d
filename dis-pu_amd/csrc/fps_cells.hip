// Exact farthest point sampling for clouds ABOVE 24576 points (tf_sampling.cpp:94,118; kernel tf_sampling_g.cu:105-170 is the spec)
// with the cloud in global memory and Morton-cell skipping: behind dispu_fps_cells / dispu_fps_segments_auto (include/dispu_hip.h).
//
// fps_mem_kernel (sampling.hip) streams all n points and running distances, 20 B per point, through the one CU that owns the cloud in
// every one of its m - 1 dependent rounds.  Here a pre-pass orders the cloud along a Morton curve and cuts it into cells of S
// consecutive sorted positions; a round then touches only the cells whose bounding box is not farther from the new sample than the
// cell's largest running distance (the test of fps_wave.hip, there per wave of a register-resident cloud).  On a surface a sample
// reaches about pi n / j points after j samples, so all rounds together update about n pi ln m points instead of n m.
//
//   pre-pass (morton_cells.hip): per segment the bounding box and non-finite flag, Morton keys with the segment id on top, ONE stable
//     radix sort over the batch, then one wave per cell gathers (x, y, z, local index) into sorted order, sets the running distances
//     to 1e38, and writes the cell's box, largest running distance (1e38) and candidate (the point of best tie priority)
//   sampling, one workgroup of 16 waves per segment; per round:
//     * thread t owns the cells {it * 1024 + lane * 16 + wave}: consecutive cells - neighbours in space - sit on different waves.
//       Their tables (box, largest distance, candidate's tie key: 8 words) live in LDS slot it * 1024 + t, touched by that thread only;
//     * every lane tests its cells' boxes; the ballot of reached cells drives a wave-uniform loop in which the whole wave does the
//       dense update of one cell (sqdist3<FMA>, min, 64-bit key max), the owner lane stores the cell's new largest distance and key;
//     * skipped cells keep their cached candidate; the winner is the maximum of (distance bits << 32 | tie key) over all cells: the
//       reference's order (larger distance, then smaller k mod 512, then smaller k; oracle/dispu_oracle.c:103-137) arithmetically,
//       so the result does not depend on the sort, the cell size or the thread layout.
//
// Why a skip is sound: for a point p of the cell and the sample s, lo <= p <= hi per axis, and rounding is monotone, so
// fl(lo - s) <= fl(p - s) <= fl(hi - s): |fl(p - s)| >= e := max(fl(lo - s), fl(s - hi), 0) holds IN floating point.  The box distance is
// sqdist3<FMA>(ex, ey, ez) - the same operations in the same order as the point distance - and every one of them (product of
// non-negatives, sum, fma) is monotone in its non-negative arguments, so lb <= d(p, s) bit for bit.  lb > largest running distance then
// gives min(td, d) == td for every point of the cell.  This argument is the one relied on; the factor 0.99999 on lb (fps_wave.hip) is
// kept as a reserve only.
//
// One level of boxes: at most kFpcMaxCells = 4096 cells per segment (128 KB of LDS), S = 64 up to 262144 points and doubling above,
// S = 4096 at the largest served segment of 2^24 points (12 * 2^20 merged points is what tools/upsample.py --max-points produces).
#include "morton_cells.h"
#include "fps_keys.h"

namespace dispu {

constexpr int kFpcThreads = 1024, kFpcWaves = kFpcThreads / kWave;
static_assert(kFpcWaves == 16, "cell <-> (lane, wave) mapping");


// LDS: tabl[8][KL] words (KL = 1024 * ceil(K / 1024)), slot it * 1024 + tid <-> cell it * 1024 + lane * 16 + wave
template <bool FMA>
__global__ __launch_bounds__(kFpcThreads) void fps_cells_kernel(const float* __restrict__ xyz, const int* __restrict__ off,
                                                                const int* __restrict__ moff, const uint32_t* __restrict__ segb,
                                                                const float4* __restrict__ spt, float* __restrict__ td,
                                                                const float* __restrict__ tab, int* __restrict__ out,
                                                                int* __restrict__ status, int cell, CellsMode mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tabl = reinterpret_cast<float*>(smem);
    __shared__ uint64_t slot[2][kFpcWaves];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const SegExt e = seg_ext(off, moff, c, 0, 0);
    if (!fpc_served(e.n, e.m, mode)) return;
    const uint32_t bad = segb[(size_t)c * 8 + 6];
    if (tid == 0) status[c] = bad ? 1 : 0;
    if (bad) return;                                                            // no indices for a non-finite segment
    const int n = e.n, m = e.m;
    const int S = fpc_cell_size(n, cell), K = (n + S - 1) / S, its = (K + kFpcThreads - 1) / kFpcThreads, KL = its * kFpcThreads;
    const float* __restrict__ p = xyz + e.base * 3;
    const float4* __restrict__ sp = spt + e.base;
    float* __restrict__ t = td + e.base;
    int* __restrict__ o = out + e.obase;
    const float* __restrict__ gt = tab + fpc_cell_base(e.base, c) * 8;
    for (int it = 0; it < its; ++it) {
        const int sl = it * kFpcThreads + tid, cl = it * kFpcThreads + lane * kFpcWaves + wave;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = make_float4(0.f, 0.f, -1.0f, 0.f);       // no cell: -1 is never reached
        if (cl < K) {
            a = *reinterpret_cast<const float4*>(gt + (size_t)cl * 8);
            b = *reinterpret_cast<const float4*>(gt + (size_t)cl * 8 + 4);
        }
        tabl[0 * KL + sl] = a.x; tabl[1 * KL + sl] = a.y; tabl[2 * KL + sl] = a.z; tabl[3 * KL + sl] = a.w;
        tabl[4 * KL + sl] = b.x; tabl[5 * KL + sl] = b.y; tabl[6 * KL + sl] = b.z; tabl[7 * KL + sl] = b.w;
    }
    if (tid == 0) o[0] = 0;
    float x1 = p[0], y1 = p[1], z1 = p[2];                                     // sample 0 is point 0 (tf_sampling_g.cu:122-124)
    for (int j = 1; j < m; ++j) {
        uint64_t best = 0ull;
        for (int it = 0; it < its; ++it) {
            const int sl = it * kFpcThreads + tid;
            const float ex = fmaxf(fmaxf(tabl[0 * KL + sl] - x1, x1 - tabl[3 * KL + sl]), 0.f);
            const float ey = fmaxf(fmaxf(tabl[1 * KL + sl] - y1, y1 - tabl[4 * KL + sl]), 0.f);
            const float ez = fmaxf(fmaxf(tabl[2 * KL + sl] - z1, z1 - tabl[5 * KL + sl]), 0.f);
            const float lb = sqdist3<FMA>(ex, ey, ez);
            unsigned long long reach = __ballot(lb * 0.99999f <= tabl[6 * KL + sl]);
            while (reach) {                                                     // wave-uniform: the whole wave updates one cell
                const int bl = (int)__builtin_ctzll(reach);
                reach &= reach - 1;
                const int pb = (it * kFpcThreads + bl * kFpcWaves + wave) * S, cnt = min(S, n - pb);
                uint64_t bk = 0ull;
#pragma unroll 4
                for (int i = lane; i < cnt; i += kWave) {
                    const float4 q = sp[pb + i];
                    const float t0 = t[pb + i];
                    const float d = sqdist3<FMA>(q.x - x1, q.y - y1, q.z - z1);
                    const float t1 = fminf(d, t0);
                    if (t1 != t0) t[pb + i] = t1;
                    const uint64_t key = ((uint64_t)__float_as_uint(t1) << 32) | fps_tiekey(__float_as_int(q.w));
                    bk = key > bk ? key : bk;
                }
                bk = wave_max_u64(bk);
                if (lane == bl) {
                    tabl[6 * KL + sl] = __uint_as_float((uint32_t)(bk >> 32));
                    tabl[7 * KL + sl] = __uint_as_float((uint32_t)bk);
                }
            }
            const float md = tabl[6 * KL + sl];
            const uint64_t key = ((uint64_t)__float_as_uint(md) << 32) | __float_as_uint(tabl[7 * KL + sl]);
            if (md >= 0.f && key > best) best = key;                            // running distances are >= 0: their bits order like them
        }
        best = wave_max_u64(best);
        const int par = j & 1;
        if (lane == 0) slot[par][wave] = best;
        __syncthreads();
        best = wave_max_u64(lane < kFpcWaves ? slot[par][lane] : 0ull);
        const int k = __builtin_amdgcn_readfirstlane(fps_key_to_index((uint32_t)best));
        if (tid == 0) o[j] = k;
        x1 = p[(size_t)k * 3 + 0]; y1 = p[(size_t)k * 3 + 1]; z1 = p[(size_t)k * 3 + 2];
    }
}


int fps_cells_run(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* scratch,
                  size_t scratch_bytes, int* out, int* status, int arith, int cell, CellsMode mode, hipStream_t st) {
    int nall, nserved, kmax;
    const int rc = fpc_plan(C, off_host, moff_host, cell, mode, &nall, &nserved, &kmax);
    if (rc != 0) return rc;
    if (!nserved) return 0;
    if (!off || !moff || !inp || !out || !status) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)off_host[C];
    const FpcScratch s = fpc_scratch(N, C);
    if (!scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    char* base = (char*)scratch;
    const uint32_t* segb = (const uint32_t*)(base + s.segb);
    const float* tab = (const float*)(base + s.tab);
    const float4* spt = (const float4*)(base + s.kin);
    float* td = (float*)(base + s.vin);
    const int rp = fpc_prepass(C, off, moff, inp, base, s, N, nall, nserved, kmax, cell, mode, st);
    if (rp != 0) return rp;
    const size_t lds = (size_t)8 * 4 * kFpcThreads * ((kmax + kFpcThreads - 1) / kFpcThreads);
    static DevOnce attr;
    if (attr.needed()) {
        const int cap = 8 * 4 * kFpcMaxCells;
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fps_cells_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fps_cells_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        attr.done();
    }
    if ((arith & DISPU_ARITH_CONTRACT))
        hipLaunchKernelGGL((fps_cells_kernel<true>), dim3(C), dim3(kFpcThreads), lds, st, inp, off, moff, segb, spt, td, tab, out, status, cell,
                           mode);
    else
        hipLaunchKernelGGL((fps_cells_kernel<false>), dim3(C), dim3(kFpcThreads), lds, st, inp, off, moff, segb, spt, td, tab, out, status, cell,
                           mode);
    return (int)hipGetLastError();
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_fps_cells_wanted(int n, int m) { return fps_cells_rule(n, m) ? 1 : 0; }

DISPU_EXPORT size_t dispu_fps_cells_scratch_bytes(int C, const int* off_host, const int* moff_host, int cell) {
    return fps_cells_scratch(C, off_host, moff_host, cell, kCellsAll);
}

DISPU_EXPORT int dispu_fps_cells(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp,
                                 void* scratch, size_t scratch_bytes, int* out, int* status, int arith, int cell, void* stream) {
    if (C < 0) return (int)hipErrorInvalidValue;
    if (C == 0) return 0;
    return fps_cells_run(C, off, moff, off_host, moff_host, inp, scratch, scratch_bytes, out, status, arith, cell, kCellsAll, (hipStream_t)stream);
}
