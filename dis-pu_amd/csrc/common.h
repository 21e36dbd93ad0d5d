// Shared device helpers for libdispu_hip.so (gfx950 / CDNA4 only, wave64).
// Compiled with -ffp-contract=off: every fused multiply-add in this library is an explicit
// __builtin_fmaf, so the arithmetic is pinned (see DESIGN.md "Pinned arithmetic").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../../include/dispu_hip.h"   // the public C-ABI: every exported definition is checked against its prototype

#define DISPU_EXPORT extern "C" __attribute__((visibility("default")))

#define DISPU_CHECK_LAUNCH()                         \
    do {                                             \
        hipError_t e__ = hipGetLastError();          \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

#define DISPU_TRY(expr)                              \
    do {                                             \
        hipError_t e__ = (expr);                     \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

// dispu_tn_reduce_desc (include/dispu_hip.h): the split reduction a TN (weight-gradient) product leaves undone under dispu_tn_defer
static_assert(sizeof(dispu_tn_reduce_desc) == 72, "descriptor layout is part of the C-ABI");

namespace dispu {

constexpr int kWave = 64;

// byte offsets inside a caller's scratch buffer advance in steps of 256
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// A scratch layout, region by region: take(bytes) is the offset of the next region and steps past it to the next multiple of 256; after
// the last region `off` is the size of the whole.  Every region is rounded on its own, so the total does not depend on their order.
// base: the buffer the regions lie in, for ptr(); null where a layout is only sized.
struct Carver {
    char* base = nullptr;
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += align256(bytes);
        return o;
    }
    template <class T>
    T* ptr(size_t bytes) {                           // the region itself; null without a base
        const size_t o = take(bytes);
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};

// what every entry asks of a caller's scratch: not null, 16-byte aligned, at least `need` bytes
static inline bool scratch_ok(const void* scratch, size_t have, size_t need) {
    return scratch && have >= need && !((uintptr_t)scratch & 15);
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte: what an entry refuses between an output and anything it still reads
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// "done once per DEVICE" flag for hipFuncSetAttribute (function attributes are per device: a process that drives several
// GPUs must opt every one of them in to > 64 KB of dynamic LDS).  Two threads racing through the first call both set the
// attribute, which is idempotent.
struct DevOnce {
    std::atomic<unsigned long long> mask{0};
    static int cur() { int d = 0; (void)hipGetDevice(&d); return d & 63; }
    bool needed() const { return !((mask.load(std::memory_order_acquire) >> cur()) & 1ull); }
    void done() { mask.fetch_or(1ull << cur(), std::memory_order_release); }
};

// Extents of workgroup g's cloud in a kernel that serves both batch layouts.  off == nullptr: a uniform batch, cloud g owns the
// points [g n, (g + 1) n) and the outputs [g m, (g + 1) m).  Otherwise a packed ragged batch (the dispu_*_segments entries): the
// points [off[g], off[g + 1]) and the outputs [ooff[g], ooff[g + 1]) (device int32 offsets, scalar loads).
struct SegExt {
    size_t base, obase;
    int n, m;
};
__device__ __forceinline__ SegExt seg_ext(const int* __restrict__ off, const int* __restrict__ ooff, int g, int n, int m) {
    if (!off) return {(size_t)g * n, (size_t)g * m, n, m};
    const int b = off[g], ob = ooff[g];
    return {(size_t)b, (size_t)ob, off[g + 1] - b, ooff[g + 1] - ob};
}

// The kernel family a cloud of n points sampled to m takes in dispu_fps_ws (with scratch) and dispu_fps_segments: 0 the register
// kernels of sampling.hip, 1 the region-skipping kernels of fps_wave.hip, 2 the streaming kernel.  Every family returns the same
// indices (the tie rule is arithmetic), so the choice only sets the speed.
__host__ __device__ __forceinline__ int fps_family(int n, int m) { return n > 24576 ? 2 : (n > 4096 && m >= 64) ? 1 : 0; }

// dispu_fps_segments_auto adds family 3, the cell-skipping kernels of fps_cells.hip, for the segments above 24576 points that
// fps_cells_rule names: THE rule for when the cell path beats the streaming kernel (dispu_fps_cells_wanted returns it), read off
// profiles/fps_large_bench.json (tools/fps_large_bench.py).  The pre-pass costs a fixed 0.1 - 0.2 ms and the first rounds reach every
// cell, so a short sampling does not repay it: at n = 30000 the cell path loses at m = 32 (0.245 against 0.184 ms), wins at m = 64
// by no more than its own spread (0.323 - 0.343 against 0.365 - 0.368 ms) and clearly from m = 128 (0.45 against 0.74 ms); at n = 122880 it loses at m = 16 (0.40 against 0.36 ms) and
// wins from m = 32, clearly from m = 64 (0.62 against 1.41 ms).  Between the two measured sizes the stricter bound holds.
__host__ __device__ __forceinline__ bool fps_cells_rule(int n, int m) { return n > 24576 && m >= (n >= 122880 ? 64 : 128); }
__host__ __device__ __forceinline__ int fps_family4(int n, int m, bool with_cells) {
    return (with_cells && fps_cells_rule(n, m)) ? 3 : fps_family(n, m);
}

template <bool FMA>
__device__ __forceinline__ float sqdist3(float dx, float dy, float dz) {
    if constexpr (FMA) {
        return __builtin_fmaf(dz, dz, __builtin_fmaf(dx, dx, dy * dy));
    } else {
        const float s = dx * dx + dy * dy;
        return s + dz * dz;
    }
}

// Two distances per instruction on the packed fp32 ops (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32); element-wise the arithmetic is
// sqdist3's, operation for operation.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool FMA>
__device__ __forceinline__ f32x2 sqdist3_x2(f32x2 dx, f32x2 dy, f32x2 dz) {
    if constexpr (FMA) {
        return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dx, dx, dy * dy));
    } else {
        const f32x2 s = dx * dx + dy * dy;
        return s + dz * dz;
    }
}

// A cloud [n][3] into LDS once per workgroup of NT threads (coalesced float4, UB per thread in flight), for the wave-per-query kernels
// whose lanes keep R candidates each in registers: per-lane global loads (3 R strided dwords per lane, the same 12 KB in every wave of
// the launch) cost a quarter of such a kernel (knn_xyz_wave_kernel: 8.8 k of 40 k cycles per wave).  Caller: __syncthreads() after.
template <int NT, int UB>
__device__ __forceinline__ void stage_cloud_xyz(float* sl, const float* __restrict__ s, int n) {
    const int nf = 3 * n;
    if ((((uintptr_t)s) & 15) == 0) {
        const int nf4 = nf >> 2;
        for (int e0 = threadIdx.x; e0 < nf4; e0 += UB * NT) {
            float4 v[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) v[u] = *reinterpret_cast<const float4*>(s + (size_t)min(e0 + u * NT, nf4 - 1) * 4);
#pragma unroll
            for (int u = 0; u < UB; ++u)
                if (e0 + u * NT < nf4) *reinterpret_cast<float4*>(sl + (e0 + u * NT) * 4) = v[u];
        }
        for (int e = (nf4 << 2) + threadIdx.x; e < nf; e += NT) sl[e] = s[e];
    } else {
        for (int e = threadIdx.x; e < nf; e += NT) sl[e] = s[e];
    }
}

// ---- DPP wave64 reductions (result valid in lane 63; use readlane to broadcast) ---------------
// row_shr:1,2,4,8 leave each 16-lane row's reduction in its lane 15; row_bcast:15 / :31 fold the
// four rows into lane 63.  `old` (identity) fills lanes that have no DPP source.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t identity, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xF, false);
}

constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118,
              DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

__device__ __forceinline__ uint64_t u64_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint64_t dpp_step_max_u64(uint64_t v) {
    const uint32_t hi = dpp_u32<CTRL, ROW_MASK>(0u, (uint32_t)(v >> 32));
    const uint32_t lo = dpp_u32<CTRL, ROW_MASK>(0u, (uint32_t)v);
    return u64_max(v, ((uint64_t)hi << 32) | lo);
}

// Wave-wide maximum of an unsigned 64-bit key, returned wave-uniform (in SGPRs).
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = dpp_step_max_u64<DPP_ROW_SHR1>(v);
    v = dpp_step_max_u64<DPP_ROW_SHR2>(v);
    v = dpp_step_max_u64<DPP_ROW_SHR4>(v);
    v = dpp_step_max_u64<DPP_ROW_SHR8>(v);
    v = dpp_step_max_u64<DPP_ROW_BCAST15, 0xA>(v);
    v = dpp_step_max_u64<DPP_ROW_BCAST31, 0xC>(v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t u64_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint64_t dpp_step_min_u64(uint64_t v) {
    const uint32_t hi = dpp_u32<CTRL, ROW_MASK>(0xFFFFFFFFu, (uint32_t)(v >> 32));
    const uint32_t lo = dpp_u32<CTRL, ROW_MASK>(0xFFFFFFFFu, (uint32_t)v);
    return u64_min(v, ((uint64_t)hi << 32) | lo);
}

// Wave-wide minimum of an unsigned 64-bit key, returned wave-uniform.
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    v = dpp_step_min_u64<DPP_ROW_SHR1>(v);
    v = dpp_step_min_u64<DPP_ROW_SHR2>(v);
    v = dpp_step_min_u64<DPP_ROW_SHR4>(v);
    v = dpp_step_min_u64<DPP_ROW_SHR8>(v);
    v = dpp_step_min_u64<DPP_ROW_BCAST15, 0xA>(v);
    v = dpp_step_min_u64<DPP_ROW_BCAST31, 0xC>(v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
    return ((uint64_t)hi << 32) | lo;
}

// float <-> unsigned key whose unsigned order is the float order (handles negative values)
__device__ __forceinline__ uint32_t f32_to_ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_f32(uint32_t u) {
    const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    return __uint_as_float(b);
}

// v_mfma_f32_32x32x2_f32 with the accumulator pinned to the ACC register file.  hipcc prefers VGPR accumulators when
// the budget allows; a wave issuing back-to-back MFMAs then reads and writes 16 VGPRs x 64 lanes per instruction and
// keeps the VGPR ports of its SIMD busy, so that the OTHER wave on the SIMD (a loader / helper wave) needs ~340
// cycles to issue one global load instead of ~40 (tools/micro/gemm_lab.hip, "AGPR acc").  The compiler does not see
// an MFMA in the asm statement: call mfma_acc_settle() once before the accumulators are read.
typedef float dispu_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void mfma_acc(dispu_f32x16& acc, float a, float b) {
    asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_acc_settle() {   // >= 18 wait states between the last 16-pass MFMA and a read of its result
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
}

// 16-byte non-temporal store (global_store_dwordx4 ... nt): streamed outputs that are not re-read by the kernel
typedef float dispu_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt4(float* dst, float4 v) {
    __builtin_nontemporal_store(dispu_f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<dispu_f32x4*>(dst));
}

// Workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2).  xcd_block() turns the hardware id into a
// logical block index such that every XCD works on ONE contiguous range of logical blocks: blocks that gather from
// the same cloud then share an L2 instead of pulling the cloud's rows into all eight.
__device__ __forceinline__ unsigned xcd_block(unsigned bid, unsigned grid) {
    const unsigned per = grid >> 3;
    return (grid & 7u) ? bid : (bid & 7u) * per + (bid >> 3);
}

__device__ __forceinline__ float wave_sum_f32(float v) {
    // butterfly; order fixed (xor 32,16,8,4,2,1) so the result is deterministic
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace dispu
