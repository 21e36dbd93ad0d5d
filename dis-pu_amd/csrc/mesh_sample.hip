// Area-weighted surface sampling of a triangle mesh (gfx950): the candidate clouds of the Poisson-disk selection (poisson_disk.hip)
// and of the training patches (dis-pu_amd/mesh_sample.py).  No reference counterpart: the reference's data was sampled upstream with
// tools that are in neither tree; the yardstick is the float64 numpy restatement in tests/mesh_sample_oracle.py.
//
// One thread per sample, no state: sample i is a function of (mesh, seed, i) only, so it does not depend on the launch shape and sample
// i of a count = n call is sample i of any larger call.
//   draw     Philox4x32-10, counter (i lo, i hi, 0, kStreamSurface), key (seed lo, seed hi) -> w0..w3.  The batch sampler's counters
//            carry an epoch >= 0 in their last word (batch_sampler.hip); kStreamSurface has the top bit set, so the two never meet
//   face     u = ((w0 << 21) | (w1 >> 11)) 2^-53 (53 bits, exact in fp64); the largest f in [0, F) with cum[f] <= u by binary search
//            over the normalised cumulative areas (mesh.Mesh.cum_areas): a face of zero area has cum[f] == cum[f + 1], so f + 1
//            qualifies whenever f does and f is never the largest
//   bary     r1 = u01(w2), r2 = u01(w3) (24 bits), s = sqrt((double)r1) correctly rounded, b = (1 - s, s (1 - r2), s r2): uniform on
//            the triangle (Osada et al., "Shape distributions", 2002)
//   point    (b0 v0 + b1 v1) + b2 v2 per coordinate in fp64 from the fp32 vertices, every product and sum rounded on its own (the
//            library is built with -ffp-contract=off and the expression is spelled out), then rounded to fp32 once
#include "common.h"
#include "philox.h"

namespace dispu {

constexpr uint32_t kStreamSurface = 0xD15C5A3Du;
constexpr int kMeshSampleThreads = 256;

__device__ __forceinline__ double bary_mix(double b0, double b1, double b2, float v0, float v1, float v2) {
#pragma clang fp contract(off)      // pinned here as well as by the build's -ffp-contract=off: three products, two sums, five roundings
    const double t0 = b0 * (double)v0;
    const double t1 = b1 * (double)v1;
    const double t2 = b2 * (double)v2;
    const double s01 = t0 + t1;
    return s01 + t2;
}

__global__ __launch_bounds__(kMeshSampleThreads) void mesh_sample_kernel(int count, int V, int F, const float* __restrict__ verts,
                                                                         const int* __restrict__ faces, const double* __restrict__ cum,
                                                                         uint32_t k0, uint32_t k1, float* __restrict__ points,
                                                                         int* __restrict__ face, double* __restrict__ bary) {
#pragma clang fp contract(off)      // the barycentrics below: one rounding per operation, whatever the build's flags
    const unsigned long long i = (unsigned long long)blockIdx.x * kMeshSampleThreads + threadIdx.x;
    if (i >= (unsigned long long)count) return;
    uint32_t w[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, kStreamSurface, k0, k1, w);
    const double u = (double)(((uint64_t)w[0] << 21) | (uint64_t)(w[1] >> 11)) * 1.1102230246251565e-16;   // 2^-53
    int lo = 0, hi = F;                                   // first f in [0, F) with cum[f] > u, F when there is none
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum[mid] <= u) lo = mid + 1; else hi = mid;
    }
    const int f = min(max(lo - 1, 0), F - 1);
    const double r1 = (double)philox_u01(w[2]), r2 = (double)philox_u01(w[3]);
    const double s = __dsqrt_rn(r1);
    const double b0 = 1.0 - s;
    const double omr2 = 1.0 - r2;
    const double b1 = s * omr2;
    const double b2 = s * r2;
    const int a0 = min(max(faces[3 * (size_t)f + 0], 0), V - 1);
    const int a1 = min(max(faces[3 * (size_t)f + 1], 0), V - 1);
    const int a2 = min(max(faces[3 * (size_t)f + 2], 0), V - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        points[3 * (size_t)i + c] = (float)bary_mix(b0, b1, b2, verts[3 * (size_t)a0 + c], verts[3 * (size_t)a1 + c], verts[3 * (size_t)a2 + c]);
    face[i] = f;
    if (bary) { bary[3 * (size_t)i + 0] = b0; bary[3 * (size_t)i + 1] = b1; bary[3 * (size_t)i + 2] = b2; }
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_mesh_sample(int V, int F, const float* verts, const int* faces, const double* cum, int count,
                                   unsigned long long seed, float* points, int* face, double* bary, void* stream) {
    if (V <= 0 || F <= 0 || count < 0 || !verts || !faces || !cum || !points || !face) return (int)hipErrorInvalidValue;
    if (count == 0) return 0;
    const unsigned grid = (unsigned)(((long long)count + kMeshSampleThreads - 1) / kMeshSampleThreads);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(grid), dim3(kMeshSampleThreads), 0, (hipStream_t)stream, count, V, F, verts, faces, cum,
                       (uint32_t)seed, (uint32_t)(seed >> 32), points, face, bary);
    return (int)hipGetLastError();
}
