// The key arithmetic every farthest-point-sampling family shares (sampling.hip, fps_wave.hip, fps_cells.hip, morton_cells.hip).  The
// reference's winner rule (max d, ties -> lowest k mod 512, then lowest k; tf_sampling_g.cu:146,158) is the unsigned maximum of
//   key = float_bits(d) << 32 | (0xFFFFFFFF - ((k & 511) << 22 | k >> 9))
// independent of a kernel's thread layout: all families return the same indices because they all use THIS copy.
#pragma once
#include "common.h"

namespace dispu {

__device__ __forceinline__ uint32_t fps_tiekey(int k) {
    return 0xFFFFFFFFu - ((((uint32_t)k & 511u) << 22) | ((uint32_t)k >> 9));
}
// the index of a tie key; the distance bits of a 64-bit key are ignored
__device__ __forceinline__ int fps_key_to_index(uint64_t key) {
    const uint32_t t = 0xFFFFFFFFu - (uint32_t)key;
    return (int)(((t & 0x3FFFFFu) << 9) | (t >> 22));
}

// Running distances are >= 0 (or -1 = "no point"): as unsigned keys (bits + 1, 0 for "no point") they order like the floats, and
// an unsigned max folds into ONE v_max_u32_dpp per step (a float max costs a DPP move plus two canonicalising v_max per step; the
// 64-bit key two DPP moves, a 64-bit compare and two selects: wave_max_u64, ~45 dependent-ish instructions per round).
__device__ __forceinline__ uint32_t fps_dkey(float d) { return d >= 0.f ? __float_as_uint(d) + 1u : 0u; }
__device__ __forceinline__ float fps_dkey_value(uint32_t k) { return k ? __uint_as_float(k - 1u) : -1.0f; }

template <int CTRL, int RM = 0xF>
__device__ __forceinline__ uint32_t fps_umax_step(uint32_t v) {
    const uint32_t o = dpp_u32<CTRL, RM>(0u, v);
    return v > o ? v : o;
}
// wave-wide unsigned maximum, returned wave-uniform
__device__ __forceinline__ uint32_t fps_wave_max_u32(uint32_t v) {
    v = fps_umax_step<DPP_ROW_SHR1>(v);
    v = fps_umax_step<DPP_ROW_SHR2>(v);
    v = fps_umax_step<DPP_ROW_SHR4>(v);
    v = fps_umax_step<DPP_ROW_SHR8>(v);
    v = fps_umax_step<DPP_ROW_BCAST15, 0xA>(v);
    v = fps_umax_step<DPP_ROW_BCAST31, 0xC>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// unsigned maximum over lanes 0 .. W - 1 of DPP row 0 (one slot per wave of a workgroup), returned wave-uniform
template <int W>
__device__ __forceinline__ uint32_t fps_row0_max_u32(uint32_t v) {
    static_assert(W <= 16, "one DPP row");
    v = fps_umax_step<DPP_ROW_SHR1>(v);
    if (W > 2) v = fps_umax_step<DPP_ROW_SHR2>(v);
    if (W > 4) v = fps_umax_step<DPP_ROW_SHR4>(v);
    if (W > 8) v = fps_umax_step<DPP_ROW_SHR8>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, W <= 2 ? 1 : W <= 4 ? 3 : W <= 8 ? 7 : 15);
}

}  // namespace dispu
