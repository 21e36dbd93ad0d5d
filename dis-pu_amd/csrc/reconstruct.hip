// Surface reconstruction from an oriented cloud, the lattice and contouring stages: behind dispu_lattice_* and dispu_contour_*
// (include/dispu_hip.h, which states every definition; tests/reconstruct_oracle.py restates them).  The values at the lattice vertices
// come from dispu_signed_distance_segments (signed_distance.hip) between the two groups.  The reference has no counterpart.
//
//   keys       a lattice index (i, j, l) per axis in +-(2^20 - 1), stored biased in 21 bits each: key = l << 42 | j << 21 | i, so the
//              unsigned order of the keys is ascending (l, j, i), z slowest
//   unique     the sorted unique set of a key buffer: radix_sort.hip's stable sorter (8 passes), run heads, its three-step scan, a
//              compaction.  Used three times: occupied voxels, the dilated (active) voxels, the corners (lattice vertices)
//   corners    [nvox, 8] lattice-vertex numbers by binary search, once, for both contouring passes
//   count      one lane per active voxel: six sign masks, the triangles of kTetCase, a plain store of 1 per used edge slot
//              (slot = 7 * lattice number of the lower endpoint + direction code - 1); then two scans number vertices and faces
//   emit       one lane per slot places its vertex (in double, from the lower endpoint), one lane per voxel writes its faces
//
// A count that sizes the caller's next buffer reaches the host at the end of the entry that finds it (one 4- or 8-byte read-back
// each).  Ordinary stores only, no float atomics, every loop bounded, ordering by kernel boundaries only, identical bytes from run to
// run.
#include "internal.h"
#include <math.h>
#include <float.h>

namespace dispu {

constexpr int kLatBias = (1 << 20) - 1;              // index i is stored as i + kLatBias: voxels 0 .. 2^21 - 2, corners up to 2^21 - 1
constexpr int kLatSJ = 21, kLatSL = 42;
constexpr uint64_t kLatMask = (1ull << 21) - 1;
constexpr int kLatPasses = 8;                        // 63 key bits

// Kuhn's six tetrahedra around the diagonal 0 -> 7, corner b = bx + 2 by + 4 bz: (0, e_a, e_a + e_b, 7), axis permutations in
// lexicographic order
__constant__ uint8_t kTet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// [tet][sign mask: bit i = tet vertex i negative] -> triangle count, then its edges as (A << 3) | d: A the corner of the edge's lower
// endpoint, d = B - A.  Orientation (from the negative to the positive corners) is baked in from the edge midpoints in the unit cube;
// tests/reconstruct_oracle.py:case_bytes() derives the same bytes from the rule and a CPU test compares them with this text
__constant__ uint8_t kTetCase[6][16][7] = {
    {{0,0,0,0,0,0,0}, {1,1,3,7,0,0,0}, {1,1,14,10,0,0,0}, {2,3,7,14,3,14,10}, {1,3,10,28,0,0,0}, {2,1,28,7,1,10,28}, {2,1,14,28,1,28,3}, {1,7,14,28,0,0,0}, {1,7,28,14,0,0,0}, {2,1,3,28,1,28,14}, {2,1,28,10,1,7,28}, {1,3,28,10,0,0,0}, {2,3,10,14,3,14,7}, {1,1,10,14,0,0,0}, {1,1,7,3,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,1,7,5,0,0,0}, {1,1,12,14,0,0,0}, {2,5,14,7,5,12,14}, {1,5,42,12,0,0,0}, {2,1,7,42,1,42,12}, {2,1,42,14,1,5,42}, {1,7,42,14,0,0,0}, {1,7,14,42,0,0,0}, {2,1,42,5,1,14,42}, {2,1,12,42,1,42,7}, {1,5,12,42,0,0,0}, {2,5,14,12,5,7,14}, {1,1,14,12,0,0,0}, {1,1,5,7,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,2,7,3,0,0,0}, {1,2,17,21,0,0,0}, {2,3,21,7,3,17,21}, {1,3,28,17,0,0,0}, {2,2,7,28,2,28,17}, {2,2,28,21,2,3,28}, {1,7,28,21,0,0,0}, {1,7,21,28,0,0,0}, {2,2,28,3,2,21,28}, {2,2,17,28,2,28,7}, {1,3,17,28,0,0,0}, {2,3,21,17,3,7,21}, {1,2,21,17,0,0,0}, {1,2,3,7,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,2,6,7,0,0,0}, {1,2,21,20,0,0,0}, {2,6,7,21,6,21,20}, {1,6,20,49,0,0,0}, {2,2,49,7,2,20,49}, {2,2,21,49,2,49,6}, {1,7,21,49,0,0,0}, {1,7,49,21,0,0,0}, {2,2,6,49,2,49,21}, {2,2,49,20,2,7,49}, {1,6,49,20,0,0,0}, {2,6,20,21,6,21,7}, {1,2,20,21,0,0,0}, {1,2,7,6,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,4,5,7,0,0,0}, {1,4,35,33,0,0,0}, {2,5,7,35,5,35,33}, {1,5,33,42,0,0,0}, {2,4,42,7,4,33,42}, {2,4,35,42,4,42,5}, {1,7,35,42,0,0,0}, {1,7,42,35,0,0,0}, {2,4,5,42,4,42,35}, {2,4,42,33,4,7,42}, {1,5,42,33,0,0,0}, {2,5,33,35,5,35,7}, {1,4,33,35,0,0,0}, {1,4,7,5,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,4,7,6,0,0,0}, {1,4,34,35,0,0,0}, {2,6,35,7,6,34,35}, {1,6,49,34,0,0,0}, {2,4,7,49,4,49,34}, {2,4,49,35,4,6,49}, {1,7,49,35,0,0,0}, {1,7,35,49,0,0,0}, {2,4,49,6,4,35,49}, {2,4,34,49,4,49,7}, {1,6,34,49,0,0,0}, {2,6,35,34,6,7,35}, {1,4,35,34,0,0,0}, {1,4,6,7,0,0,0}, {0,0,0,0,0,0,0}}};

// ---- the sorted unique set of a key buffer -----------------------------------------------------------------------------------------------
// the entry writes its n keys to sort.k[0]
struct UniqScratch {
    RadixSorter sort;
    uint32_t *head, *small;                          // small: the count; 16 words in, two flag words of the entry that owns the scratch
    size_t total;
};
static UniqScratch uniq_scratch(size_t n, void* base = nullptr) {
    UniqScratch s;
    Carver cv{(char*)base};
    s.sort.carve(cv, n);
    s.head = cv.ptr<uint32_t>(4 * n);
    s.small = cv.ptr<uint32_t>(256);
    s.total = cv.off;
    return s;
}

// ex: the exclusive scan of the heads; a head's key goes to its number (below n: at most n heads)
__global__ __launch_bounds__(kRsThreads) void recon_compact_kernel(const uint64_t* __restrict__ keys, size_t n, const uint32_t* __restrict__ ex,
                                                                   uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (j >= n) return;
    if ((j == 0 || keys[j] != keys[j - 1]) && ex[j] < n) out[ex[j]] = keys[j];
}

// s.sort.k[0] [n] (overwritten) -> out [<= n] sorted unique, the count -> *count_host (the stream is synchronised)
static int sorted_unique(UniqScratch& s, size_t n, uint64_t* out, uint32_t* count_host, hipStream_t st) {
    DISPU_TRY(hipMemsetAsync(s.sort.v[0], 0, 4 * n, st));      // the sorter carries values along; nobody reads them here
    int rc = s.sort.sort(n, kLatPasses, st);
    if (rc) return rc;
    rc = run_heads_scan(s.sort.keys(), n, s.head, s.sort.sums, s.small, st);
    if (rc) return rc;
    hipLaunchKernelGGL(recon_compact_kernel, dim3(rs_blocks(n)), dim3(kRsThreads), 0, st, s.sort.keys(), n, (const uint32_t*)s.head, out);
    DISPU_CHECK_LAUNCH();
    DISPU_TRY(hipMemcpyAsync(count_host, s.small, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DISPU_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---- key generation ------------------------------------------------------------------------------------------------------------------------
// flags[0] = 1: a non-finite coordinate; flags[1] = 1: an index that leaves +-(2^20 - 1 - band).  Many lanes may store the same 1
__global__ __launch_bounds__(kRsThreads) void recon_point_keys_kernel(const float* __restrict__ points, size_t n, float h, float limit,
                                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ flags) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
    bool nonfinite = false, range = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = points[3 * i + c];
        nonfinite |= !(fabsf(v) <= FLT_MAX);
        const float fi = floorf(__fdiv_rn(v, h));
        const bool in = fabsf(fi) <= limit;          // false for a NaN
        range |= !in;
        key |= (uint64_t)((in ? (int)fi : 0) + kLatBias) << (21 * c);
    }
    if (nonfinite) flags[0] = 1u;
    else if (range) flags[1] = 1u;
    keys[i] = key;
}

// every occupied voxel and its (2 band + 1)^3 Chebyshev neighbours; the point keys left room for the band, so no field carries
__global__ __launch_bounds__(kRsThreads) void recon_dilate_keys_kernel(const uint64_t* __restrict__ occ, size_t nocc, int band,
                                                                       uint64_t* __restrict__ keys) {
    const int w = 2 * band + 1, w3 = w * w * w;
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t >= nocc * (size_t)w3) return;
    const int o = (int)(t % w3);
    const int64_t di = o % w - band, dj = (o / w) % w - band, dl = o / (w * w) - band;
    keys[t] = occ[t / w3] + (uint64_t)(di + dj * (1ll << kLatSJ) + dl * (1ll << kLatSL));
}

__device__ __forceinline__ uint64_t recon_step_key(uint64_t key, int b) {           // the key of corner b (or direction code b) of `key`
    return key + (uint64_t)(b & 1) + ((uint64_t)((b >> 1) & 1) << kLatSJ) + ((uint64_t)(b >> 2) << kLatSL);
}

__global__ __launch_bounds__(kRsThreads) void recon_corner_keys_kernel(const uint64_t* __restrict__ act, size_t nvox, uint64_t* __restrict__ keys) {
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t < nvox * 8) keys[t] = recon_step_key(act[t >> 3], (int)(t & 7));
}

// the number of `key` in the sorted unique lat [nlat], or nlat when it is absent; at most 33 halvings
__device__ __forceinline__ uint32_t recon_find(const uint64_t* __restrict__ lat, uint32_t nlat, uint64_t key) {
    uint32_t lo = 0, hi = nlat;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (lat[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < nlat && lat[lo] == key) ? lo : nlat;
}

__global__ __launch_bounds__(kRsThreads) void recon_corner_table_kernel(const uint64_t* __restrict__ act, size_t nvox, const uint64_t* __restrict__ lat,
                                                                        uint32_t nlat, int* __restrict__ corner) {
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t < nvox * 8) corner[t] = (int)recon_find(lat, nlat, recon_step_key(act[t >> 3], (int)(t & 7)));
}

__device__ __forceinline__ float recon_axis(uint64_t key, int c, float h) {
#pragma clang fp contract(off)
    return (float)((int)((key >> (21 * c)) & kLatMask) - kLatBias) * h;
}

__global__ __launch_bounds__(kRsThreads) void recon_positions_kernel(const uint64_t* __restrict__ lat, size_t nlat, float h, float* __restrict__ pos) {
    const size_t t = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (t >= nlat) return;
    const uint64_t key = lat[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[3 * t + c] = recon_axis(key, c, h);
}

// ---- contouring ----------------------------------------------------------------------------------------------------------------------------
// (a corner number is clamped to nlat - 1: a no-op for dispu_lattice_corners' table, it keeps a wrong one from reading outside)
__device__ __forceinline__ uint32_t recon_corner(const int* __restrict__ corner, size_t v, int b, uint32_t nlat) {
    return min((uint32_t)corner[v * 8 + b], nlat - 1);
}

__device__ __forceinline__ uint32_t recon_voxel_mask(const int* __restrict__ corner, const float* __restrict__ f, size_t v, uint32_t nlat) {
    uint32_t mask = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) mask |= (f[recon_corner(corner, v, b, nlat)] < 0.0f ? 1u : 0u) << b;   // an exact zero is not negative
    return mask;
}

__device__ __forceinline__ uint32_t recon_tet_mask(uint32_t vmask, int t) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m |= ((vmask >> kTet[t][i]) & 1u) << i;
    return m;
}

__global__ __launch_bounds__(kRsThreads) void recon_count_kernel(const int* __restrict__ corner, const float* __restrict__ f, size_t nvox,
                                                                 uint32_t nlat, uint32_t* __restrict__ used, uint32_t* __restrict__ ntri) {
    const size_t v = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (v >= nvox) return;
    const uint32_t vmask = recon_voxel_mask(corner, f, v, nlat);
    uint32_t cnt = 0;
    if (vmask != 0u && vmask != 255u) {
        for (int t = 0; t < 6; ++t) {
            const uint8_t* cs = kTetCase[t][recon_tet_mask(vmask, t)];
            const int m = cs[0];
            cnt += (uint32_t)m;
            for (int e = 0; e < 3 * m; ++e) {
                const int code = cs[1 + e];
                used[(size_t)7 * recon_corner(corner, v, code >> 3, nlat) + (code & 7) - 1] = 1u;       // code & 7 in 1 .. 7
            }
        }
    }
    ntri[v] = cnt;
}

// num: the exclusive scan of the used flags.  Slot s is used iff its number differs from the next one's (nverts after the last)
__global__ __launch_bounds__(kRsThreads) void recon_vertices_kernel(const uint64_t* __restrict__ lat, uint32_t nlat, const float* __restrict__ f,
                                                                    float h, const uint32_t* __restrict__ num, uint32_t nverts,
                                                                    float* __restrict__ verts) {
#pragma clang fp contract(off)
    const size_t s = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    const size_t slots = (size_t)7 * nlat;
    if (s >= slots) return;
    const uint32_t e = num[s], next = s + 1 < slots ? num[s + 1] : nverts;
    if (next == e || e >= nverts) return;
    const uint32_t A = (uint32_t)(s / 7);
    const int d = (int)(s % 7) + 1;
    const uint64_t ka = lat[A], kb = recon_step_key(ka, d);
    uint32_t B = recon_find(lat, nlat, kb);
    if (B == nlat) B = A;                            // cannot happen for a used slot: both ends are corners of one active voxel
    const double fa = (double)f[A], fb = (double)f[B];
    const double t = fa / (fa - fb);                 // fa < 0 <= fb or the reverse
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = (double)recon_axis(ka, c, h), b = (double)recon_axis(kb, c, h);
        verts[3 * (size_t)e + c] = (float)(a + t * (b - a));
    }
}

__global__ __launch_bounds__(kRsThreads) void recon_faces_kernel(const int* __restrict__ corner, const float* __restrict__ f, size_t nvox, uint32_t nlat,
                                                                 const uint32_t* __restrict__ num, const uint32_t* __restrict__ tri_start,
                                                                 uint32_t nfaces, int* __restrict__ faces) {
    const size_t v = (size_t)blockIdx.x * kRsThreads + threadIdx.x;
    if (v >= nvox) return;
    const uint32_t vmask = recon_voxel_mask(corner, f, v, nlat);
    if (vmask == 0u || vmask == 255u) return;
    size_t o = tri_start[v];
    for (int t = 0; t < 6; ++t) {
        const uint8_t* cs = kTetCase[t][recon_tet_mask(vmask, t)];
        const int m = cs[0];
        for (int i = 0; i < m && o < nfaces; ++i, ++o)
            for (int e = 0; e < 3; ++e) {
                const int code = cs[1 + 3 * i + e];
                faces[3 * o + e] = (int)num[(size_t)7 * recon_corner(corner, v, code >> 3, nlat) + (code & 7) - 1];
            }
    }
}

constexpr long long kReconMaxKeys = (1ll << 31) - 1;

static long long dilate_keys(long long nocc, int band) {
    if (nocc <= 0 || nocc > (1ll << 24) || band < 1 || band > 3) return 0;
    const long long w = 2 * band + 1, nk = nocc * w * w * w;
    return nk <= kReconMaxKeys ? nk : 0;
}

struct ContourScratch {
    uint32_t *sums, *tot;
    size_t total;
};
static ContourScratch contour_scratch(size_t nvox, size_t nlat, void* base = nullptr) {
    ContourScratch s;
    Carver cv{(char*)base};
    s.sums = cv.ptr<uint32_t>(4 * scan_blocks(7 * nlat > nvox ? 7 * nlat : nvox));
    s.tot = cv.ptr<uint32_t>(256);
    s.total = cv.off;
    return s;
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT size_t dispu_lattice_voxels_scratch_bytes(long long n) {
    return (n <= 0 || n > (1ll << 24)) ? 0 : uniq_scratch((size_t)n).total;
}

DISPU_EXPORT int dispu_lattice_voxels(long long n, const float* points, float voxel, int band, unsigned long long* occ_out, int* count_host,
                                      int* status_host, void* scratch, size_t scratch_bytes, void* stream) {
    if (n <= 0 || n > (1ll << 24) || !points || !occ_out || !count_host || !status_host) return (int)hipErrorInvalidValue;
    if (!(voxel > 0.0f) || !(voxel <= FLT_MAX) || band < 1 || band > 3) return (int)hipErrorInvalidValue;
    const size_t N = (size_t)n;
    UniqScratch s = uniq_scratch(N, scratch);
    if (!s.total || !scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    if (ranges_overlap(occ_out, 8 * N, points, 12 * N)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* flags = s.small + 16;
    *count_host = 0;
    *status_host = 0;
    DISPU_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(recon_point_keys_kernel, dim3(rs_blocks(N)), dim3(kRsThreads), 0, st, points, N, voxel, (float)(kLatBias - band), s.sort.k[0], flags);
    DISPU_CHECK_LAUNCH();
    uint32_t hf[2] = {0, 0};
    DISPU_TRY(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    DISPU_TRY(hipStreamSynchronize(st));
    if (hf[0] || hf[1]) { *status_host = hf[0] ? DISPU_LATTICE_NONFINITE : DISPU_LATTICE_RANGE; return 0; }
    uint32_t cnt = 0;
    const int rc = sorted_unique(s, N, (uint64_t*)occ_out, &cnt, st);
    if (rc) return rc;
    *count_host = (int)cnt;
    return 0;
}

DISPU_EXPORT size_t dispu_lattice_dilate_scratch_bytes(long long nocc, int band) {
    const long long nk = dilate_keys(nocc, band);
    return nk ? uniq_scratch((size_t)nk).total : 0;
}

DISPU_EXPORT int dispu_lattice_dilate(long long nocc, const unsigned long long* occ, int band, unsigned long long* act_out,
                                      long long* count_host, void* scratch, size_t scratch_bytes, void* stream) {
    const long long nk = dilate_keys(nocc, band);
    if (!nk || !occ || !act_out || !count_host) return (int)hipErrorInvalidValue;
    const size_t NK = (size_t)nk;
    UniqScratch s = uniq_scratch(NK, scratch);
    if (!s.total || !scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    if (ranges_overlap(act_out, 8 * NK, occ, 8 * (size_t)nocc)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    *count_host = 0;
    hipLaunchKernelGGL(recon_dilate_keys_kernel, dim3(rs_blocks(NK)), dim3(kRsThreads), 0, st, (const uint64_t*)occ, (size_t)nocc, band, s.sort.k[0]);
    uint32_t cnt = 0;
    const int rc = sorted_unique(s, NK, (uint64_t*)act_out, &cnt, st);
    if (rc) return rc;
    *count_host = (long long)cnt;
    return 0;
}

DISPU_EXPORT size_t dispu_lattice_corners_scratch_bytes(long long nvox) {
    return (nvox <= 0 || nvox * 8 > kReconMaxKeys) ? 0 : uniq_scratch((size_t)nvox * 8).total;
}

DISPU_EXPORT int dispu_lattice_corners(long long nvox, const unsigned long long* act, unsigned long long* lat_out, int* corner_out,
                                       long long* count_host, void* scratch, size_t scratch_bytes, void* stream) {
    if (nvox <= 0 || nvox * 8 > kReconMaxKeys || !act || !lat_out || !corner_out || !count_host) return (int)hipErrorInvalidValue;
    const size_t NK = (size_t)nvox * 8;
    UniqScratch s = uniq_scratch(NK, scratch);
    if (!s.total || !scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    if (ranges_overlap(lat_out, 8 * NK, act, 8 * (size_t)nvox) || ranges_overlap(corner_out, 4 * NK, act, 8 * (size_t)nvox) ||
        ranges_overlap(lat_out, 8 * NK, corner_out, 4 * NK))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    *count_host = 0;
    hipLaunchKernelGGL(recon_corner_keys_kernel, dim3(rs_blocks(NK)), dim3(kRsThreads), 0, st, (const uint64_t*)act, (size_t)nvox, s.sort.k[0]);
    uint32_t cnt = 0;
    const int rc = sorted_unique(s, NK, (uint64_t*)lat_out, &cnt, st);
    if (rc) return rc;
    hipLaunchKernelGGL(recon_corner_table_kernel, dim3(rs_blocks(NK)), dim3(kRsThreads), 0, st, (const uint64_t*)act, (size_t)nvox,
                       (const uint64_t*)lat_out, cnt, corner_out);
    DISPU_CHECK_LAUNCH();
    *count_host = (long long)cnt;
    return 0;
}

DISPU_EXPORT int dispu_lattice_positions(long long nlat, const unsigned long long* lat, float voxel, float* pos_out, void* stream) {
    if (nlat <= 0 || nlat > (1ll << 24) || !lat || !pos_out || !(voxel > 0.0f) || !(voxel <= FLT_MAX)) return (int)hipErrorInvalidValue;
    if (ranges_overlap(pos_out, 12 * (size_t)nlat, lat, 8 * (size_t)nlat)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(recon_positions_kernel, dim3(rs_blocks((size_t)nlat)), dim3(kRsThreads), 0, (hipStream_t)stream, (const uint64_t*)lat,
                       (size_t)nlat, voxel, pos_out);
    return (int)hipGetLastError();
}

DISPU_EXPORT size_t dispu_contour_count_scratch_bytes(long long nvox, long long nlat) {
    if (nvox <= 0 || nvox * 8 > kReconMaxKeys || nlat <= 0 || nlat > (1ll << 24)) return 0;
    return contour_scratch((size_t)nvox, (size_t)nlat).total;
}

DISPU_EXPORT int dispu_contour_count(long long nvox, long long nlat, const int* corner, const float* values, unsigned* slot_number,
                                     unsigned* tri_start, long long* nverts_host, long long* nfaces_host, void* scratch, size_t scratch_bytes,
                                     void* stream) {
    if (nvox <= 0 || nvox * 8 > kReconMaxKeys || nlat <= 0 || nlat > (1ll << 24)) return (int)hipErrorInvalidValue;
    if (!corner || !values || !slot_number || !tri_start || !nverts_host || !nfaces_host) return (int)hipErrorInvalidValue;
    const size_t NV = (size_t)nvox, NL = (size_t)nlat;
    const ContourScratch s = contour_scratch(NV, NL, scratch);
    if (!s.total || !scratch_ok(scratch, scratch_bytes, s.total)) return (int)hipErrorInvalidValue;
    const void* ins[2] = {corner, values};
    const size_t inb[2] = {32 * NV, 4 * NL};
    for (int i = 0; i < 2; ++i)
        if (ranges_overlap(slot_number, 28 * NL, ins[i], inb[i]) || ranges_overlap(tri_start, 4 * NV, ins[i], inb[i])) return (int)hipErrorInvalidValue;
    if (ranges_overlap(slot_number, 28 * NL, tri_start, 4 * NV)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    *nverts_host = 0;
    *nfaces_host = 0;
    DISPU_TRY(hipMemsetAsync(slot_number, 0, 28 * NL, st));
    hipLaunchKernelGGL(recon_count_kernel, dim3(rs_blocks(NV)), dim3(kRsThreads), 0, st, corner, values, NV, (uint32_t)NL, (uint32_t*)slot_number,
                       (uint32_t*)tri_start);
    DISPU_CHECK_LAUNCH();
    int rc = exclusive_scan_u32((uint32_t*)slot_number, 7 * NL, s.sums, s.tot, st);
    if (rc == 0) rc = exclusive_scan_u32((uint32_t*)tri_start, NV, s.sums, s.tot + 1, st);
    if (rc) return rc;
    uint32_t tot[2] = {0, 0};
    DISPU_TRY(hipMemcpyAsync(tot, s.tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    DISPU_TRY(hipStreamSynchronize(st));
    *nverts_host = (long long)tot[0];
    *nfaces_host = (long long)tot[1];
    return 0;
}

DISPU_EXPORT int dispu_contour_emit(long long nvox, long long nlat, float voxel, const unsigned long long* lat, const int* corner,
                                    const float* values, const unsigned* slot_number, const unsigned* tri_start, long long nverts,
                                    long long nfaces, float* verts_out, int* faces_out, void* stream) {
    if (nvox <= 0 || nvox * 8 > kReconMaxKeys || nlat <= 0 || nlat > (1ll << 24) || !(voxel > 0.0f) || !(voxel <= FLT_MAX)) return (int)hipErrorInvalidValue;
    if (nverts <= 0 || nverts > 7 * nlat || nfaces <= 0 || nfaces > 12 * nvox || 3 * nfaces > kReconMaxKeys) return (int)hipErrorInvalidValue;
    if (!lat || !corner || !values || !slot_number || !tri_start || !verts_out || !faces_out) return (int)hipErrorInvalidValue;
    const size_t NV = (size_t)nvox, NL = (size_t)nlat, vb = 12 * (size_t)nverts, fb = 12 * (size_t)nfaces;
    const void* ins[5] = {lat, corner, values, slot_number, tri_start};
    const size_t inb[5] = {8 * NL, 32 * NV, 4 * NL, 28 * NL, 4 * NV};
    for (int i = 0; i < 5; ++i)
        if (ranges_overlap(verts_out, vb, ins[i], inb[i]) || ranges_overlap(faces_out, fb, ins[i], inb[i])) return (int)hipErrorInvalidValue;
    if (ranges_overlap(verts_out, vb, faces_out, fb)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(recon_vertices_kernel, dim3(rs_blocks(7 * NL)), dim3(kRsThreads), 0, st, (const uint64_t*)lat, (uint32_t)NL, values, voxel,
                       (const uint32_t*)slot_number, (uint32_t)nverts, verts_out);
    hipLaunchKernelGGL(recon_faces_kernel, dim3(rs_blocks(NV)), dim3(kRsThreads), 0, st, corner, values, NV, (uint32_t)NL, (const uint32_t*)slot_number,
                       (const uint32_t*)tri_start, (uint32_t)nfaces, faces_out);
    return (int)hipGetLastError();
}
