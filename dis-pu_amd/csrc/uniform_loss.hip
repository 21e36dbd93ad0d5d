// The uniform term of the training loss for gfx950: get_uniform_loss (Common/loss_utils.py:238-267, DisPU/model.py:86) value AND
// gradient in one launch, behind dispu_uniform_loss_grad; and dispu_pu_loss_finalize_u, the loss finalize that adds the term.
//
// The reference composes the term per level from farthest_point_sample, query_ball_point, group_point, knn_point(2) and moments: with
// the five default levels that is more than 25 launches for 51 seeds x 5 radii x <= 12 members per cloud.  Here a WAVE owns a seed
// (one single-wave workgroup per (cloud, seed)): the cloud goes through it in 64-candidate blocks, one distance per candidate serves
// every level, a level's hits are a ballot mask and a hit's slot is count + popcount(lower lanes) -- the ball query of
// query_ball_wave_kernel (csrc/grouping.hip) with its hit decision (ball_mask.h), so the slots are dispu_query_ball's bit for bit.
// The members of a ball then sit one per lane (ns <= 64) and a member's nearest other member is ns broadcast steps.
//
// A hit lane drops its candidate's coordinates and index into LDS at its slot, so the second phase reads no global memory.
// Work per wave: ceil(n / 64) blocks x (1 distance + L mask tests), eight blocks' loads in flight at a time, then per level ns
// broadcast steps and <= 6 ns atomics: at (8, 1024) that is 408 waves of 16 blocks each; the launch's time is the latency of one
// wave's chain.
#include "ball_mask.h"
#include "common.h"

namespace dispu {

constexpr int UL_MAX_LEVELS = 8;

// the level tables, by value in the kernel arguments (the caller's host arrays are read when the entry is called)
struct UlLevels {
    int nlevels;
    int ns[UL_MAX_LEVELS];
    float rad[UL_MAX_LEVELS], expect[UL_MAX_LEVELS], vfac[UL_MAX_LEVELS], gfac[UL_MAX_LEVELS];
    long idx_off[UL_MAX_LEVELS];          // first element of level l in idx_out: sum over l' < l of balls * ns[l']
};

__device__ __forceinline__ float lane_f32(float v, int t) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t)); }

constexpr int UL_BLOCKS = 8;              // 64-candidate blocks whose loads are in flight together (the scan is a chain of load latencies)

template <bool FMA>
__global__ __launch_bounds__(64) void uniform_loss_grad_kernel(int n, int npoint, long balls, UlLevels lv, const float* __restrict__ pcd,
                                                               const int* __restrict__ seeds, float* __restrict__ partial,
                                                               float* __restrict__ dpcd, int* __restrict__ idx_out, int* __restrict__ cnt_out) {
    __shared__ float4 s_mem[UL_MAX_LEVELS][64];                     // a ball's members: x, y, z, index (as bits); slot 0 = the first hit
    __shared__ int s_cnt[UL_MAX_LEVELS];
    const int lane = threadIdx.x;
    const long ball = blockIdx.x;                                   // cloud * npoint + seed slot
    const long cloud = ball / npoint;
    const float* __restrict__ p = pcd + (size_t)cloud * n * 3;
    const int L = lv.nlevels;
    const int seed = min(max(seeds[ball], 0), n - 1);               // a seed outside the cloud must not become an address
    const float x2 = p[(size_t)seed * 3 + 0], y2 = p[(size_t)seed * 3 + 1], z2 = p[(size_t)seed * 3 + 2];

    // ---- the L ball queries in one pass over the cloud: the counts are wave-uniform, a hit lane drops its candidate into LDS ----
    int cnt[UL_MAX_LEVELS];
    QbBand band[UL_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < UL_MAX_LEVELS; ++l) {
        cnt[l] = 0;
        band[l] = qb_band(l < L ? lv.rad[l] : 1.0f);
    }
    const int blocks = (int)(((long)n + 63) / 64);
    for (int blk = 0; blk < blocks; blk += UL_BLOCKS) {
        bool open = false;
#pragma unroll
        for (int l = 0; l < UL_MAX_LEVELS; ++l) open = open || (l < L && cnt[l] < lv.ns[l]);
        if (!open) break;                                           // every row is full: the scan is in index order
        const int c0 = blk * 64;
        float cx[UL_BLOCKS], cy[UL_BLOCKS], cz[UL_BLOCKS], d2[UL_BLOCKS];
#pragma unroll
        for (int r = 0; r < UL_BLOCKS; ++r) {                       // (c0 < 2^31, but c0 + 64 r + lane may pass it: clamp as long)
            const size_t q = (size_t)min((long)c0 + 64 * r + lane, (long)n - 1);
            cx[r] = p[q * 3 + 0]; cy[r] = p[q * 3 + 1]; cz[r] = p[q * 3 + 2];
        }
#pragma unroll
        for (int r = 0; r < UL_BLOCKS; ++r) d2[r] = sqdist3<FMA>(x2 - cx[r], y2 - cy[r], z2 - cz[r]);
#pragma unroll
        for (int l = 0; l < UL_MAX_LEVELS; ++l) {
            if (l < L && cnt[l] < lv.ns[l]) {
                unsigned long long mk[UL_BLOCKS];
                qb_masks<UL_BLOCKS>(band[l], d2, c0, lane, n, mk);
#pragma unroll
                for (int r = 0; r < UL_BLOCKS; ++r) {
                    if (mk[r] && cnt[l] < lv.ns[l]) {               // scalar values
                        const int pos = cnt[l] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk[r] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk[r], 0u));
                        if (((mk[r] >> lane) & 1ull) && pos < lv.ns[l])
                            s_mem[l][pos] = make_float4(cx[r], cy[r], cz[r], __int_as_float(c0 + 64 * r + lane));
                        cnt[l] = min(lv.ns[l], cnt[l] + (int)__popcll(mk[r]));
                    }
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < UL_MAX_LEVELS; ++l) s_cnt[l] = cnt[l];
    }
    __syncthreads();                                                // single-wave workgroup: orders the wave's own LDS stores and loads

    // ---- per level: slot i of the ball in lane i; its nearest other slot; value partial and gradient ----
    for (int l = 0; l < L; ++l) {
        const int ns = lv.ns[l], c = s_cnt[l];
        const bool act = lane < ns;
        float part = __builtin_nanf("");                            // a ball without any hit (NaN coordinates): the reference's slots are undefined
        if (c > 0) {
            // first hit replicated into the unused tail, as the ball query does
            const float4 m = s_mem[l][(act && lane < c) ? lane : 0];
            const float ax = m.x, ay = m.y, az = m.z;
            const int a = __float_as_int(m.w);
            if (idx_out && act) idx_out[lv.idx_off[l] + ball * ns + lane] = a;
            // D_i = min over slots t != i of |x_a - x_idx[t]|^2 from coordinate differences; strict '<' in slot order: the lowest slot wins ties
            float best = __builtin_inff(), gx = 0.f, gy = 0.f, gz = 0.f;
            int partner = a;
            for (int t = 0; t < ns; ++t) {
                const float dx = ax - lane_f32(ax, t), dy = ay - lane_f32(ay, t), dz = az - lane_f32(az, t);
                const int ti = __builtin_amdgcn_readlane(a, t);
                const float d = sqdist3<false>(dx, dy, dz);
                if (t != lane && d < best) { best = d; partner = ti; gx = dx; gy = dy; gz = dz; }
            }
            const float e = lv.expect[l], den = e + 1e-8f;
            const float u = sqrtf(best + 1e-8f), du = u - e;
            const float qv = act ? (du * du) / den : 0.f;
            float s = 0.f;
            for (int t = 0; t < ns; ++t) s += lane_f32(qv, t);      // fixed slot order: the value is reproducible
            part = s * lv.vfac[l];
            if (dpcd && act && partner != a) {                      // a padded slot whose partner is the member itself adds nothing
                const float w = (lv.gfac[l] * (du / (den * u))) * 2.0f;
                float* __restrict__ da = dpcd + ((size_t)cloud * n + a) * 3;
                float* __restrict__ dc = dpcd + ((size_t)cloud * n + partner) * 3;
                const float wx = w * gx, wy = w * gy, wz = w * gz;
                unsafeAtomicAdd(da + 0, wx); unsafeAtomicAdd(da + 1, wy); unsafeAtomicAdd(da + 2, wz);
                unsafeAtomicAdd(dc + 0, -wx); unsafeAtomicAdd(dc + 1, -wy); unsafeAtomicAdd(dc + 2, -wz);
            }
        }
        if (lane == 0) {
            partial[(size_t)l * balls + ball] = part;
            if (cnt_out) cnt_out[(size_t)l * balls + ball] = c;
        }
    }
}

// dispu_pu_loss_finalize's five outputs (the same sums in the same order: pu_loss_finalize_kernel, csrc/train_fused.hip) plus the
// uniform term: out[5] = uniform_w * mean(upart), added to out[3].  One workgroup, fixed order.
__device__ __forceinline__ float block_sum_1024(const float* __restrict__ v, long count, float* red) {
    float s = 0.f;
    if (v)
        for (long i = threadIdx.x; i < count; i += 1024) s += v[i];
    s = wave_sum_f32(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    float a = 0.f;
    for (int w = 0; w < 16; ++w) a += red[w];
    return a;
}

__global__ __launch_bounds__(1024) void pu_loss_finalize_u_kernel(const float* __restrict__ cd, const float* __restrict__ rep, long nrep, float wf,
                                                                   float rep_w, const float* __restrict__ upart, long nupart, float uniform_w,
                                                                   float* __restrict__ out) {
    __shared__ float red[16];
    const float a = block_sum_1024(rep, nrep, red);
    const float ua = block_sum_1024(upart, nupart, red);
    if (threadIdx.x == 0) {
        const float r = rep ? rep_w * (a / ((float)nrep * 4.0f)) : 0.f;
        const float c = 1000.0f * cd[0], f = 1000.0f * cd[1];
        const float un = uniform_w * (ua / (float)nupart);
        out[0] = c; out[1] = f; out[2] = r; out[3] = ((c + wf * f) + r) + un; out[4] = wf; out[5] = un;
    }
}

// the loss head with the EMD term (model.py:77 enabled): the sums of pu_loss_finalize_u_kernel in the same order (upart may be NULL:
// no uniform term), plus out[6] = e = emd_w * mean_b(cost_b / radius_b / m) (earth_mover, loss_utils.py:170-176; radius NULL: 1) and
// pu_loss = ((c + wf * (f + e)) + r) [+ u]: the term sits INSIDE the weight_fine parenthesis, next to dis_fine_cd.
__global__ __launch_bounds__(1024) void pu_loss_finalize_e_kernel(const float* __restrict__ cd, const float* __restrict__ rep, long nrep, float wf,
                                                                   float rep_w, const float* __restrict__ upart, long nupart, float uniform_w,
                                                                   const float* __restrict__ emd_cost, const float* __restrict__ radius, int b, int m,
                                                                   float emd_w, float* __restrict__ out) {
    __shared__ float red[16];
    __shared__ float per[1024];
    const float a = block_sum_1024(rep, nrep, red);
    const float ua = block_sum_1024(upart, nupart, red);
    float es = 0.f;
    for (int i = threadIdx.x; i < b; i += 1024) es += (emd_cost[i] / (radius ? radius[i] : 1.0f)) / (float)m;
    per[threadIdx.x] = es;
    __syncthreads();
    if (threadIdx.x == 0) {
        float ea = per[0];
        const int cnt = b < 1024 ? b : 1024;
        for (int i = 1; i < cnt; ++i) ea += per[i];                     // clouds in ascending order (b <= 1024: exactly the sequential mean)
        const float r = rep ? rep_w * (a / ((float)nrep * 4.0f)) : 0.f;
        const float c = 1000.0f * cd[0], f = 1000.0f * cd[1];
        const float un = upart ? uniform_w * (ua / (float)nupart) : 0.f;
        const float e = emd_w * (ea / (float)b);
        float pu = (c + wf * (f + e)) + r;
        if (upart) pu = pu + un;
        out[0] = c; out[1] = f; out[2] = r; out[3] = pu; out[4] = wf; out[5] = un; out[6] = e;
    }
}

}  // namespace dispu

using namespace dispu;

// get_uniform_loss (loss_utils.py:238-267; model.py:86) on given seeds: ball queries, nearest other member, value partials and gradient.
DISPU_EXPORT int dispu_uniform_loss_grad(int b, int n, int npoint, int nlevels, const int* ns, const float* levels, const float* pcd,
                                         const int* seeds, float* partial, float* dpcd, int* idx_out, int* cnt_out, int arith, void* stream) {
    if (b < 0 || n < 1 || npoint < 1 || nlevels < 1 || nlevels > UL_MAX_LEVELS || !ns || !levels || !pcd || !seeds || !partial)
        return (int)hipErrorInvalidValue;
    const long balls = (long)b * npoint;
    if (balls > 0x7fffffffl) return (int)hipErrorInvalidValue;      // one workgroup per ball
    UlLevels lv = {};
    lv.nlevels = nlevels;
    long off = 0;
    for (int l = 0; l < nlevels; ++l) {
        if (ns[l] < 2 || ns[l] > 64 || ns[l] > n) return (int)hipErrorInvalidValue;
        lv.ns[l] = ns[l];
        lv.rad[l] = levels[4 * l + 0]; lv.expect[l] = levels[4 * l + 1]; lv.vfac[l] = levels[4 * l + 2]; lv.gfac[l] = levels[4 * l + 3];
        lv.idx_off[l] = off;
        off += balls * ns[l];
    }
    if (b == 0) return 0;
    if (arith & DISPU_ARITH_CONTRACT)
        hipLaunchKernelGGL((uniform_loss_grad_kernel<true>), dim3((unsigned)balls), dim3(64), 0, (hipStream_t)stream, n, npoint, balls, lv, pcd,
                           seeds, partial, dpcd, idx_out, cnt_out);
    else
        hipLaunchKernelGGL((uniform_loss_grad_kernel<false>), dim3((unsigned)balls), dim3(64), 0, (hipStream_t)stream, n, npoint, balls, lv, pcd,
                           seeds, partial, dpcd, idx_out, cnt_out);
    return (int)hipGetLastError();
}

// dispu_pu_loss_finalize + the uniform term (model.py:86-87): upart [nlevels, nu] = dispu_uniform_loss_grad's partials.
DISPU_EXPORT int dispu_pu_loss_finalize_u(const float* cd, const float* rep, long nrep, float wf, float rep_w, const float* upart, int nlevels,
                                          long nu, float uniform_w, float* out, void* stream) {
    if (!cd || !out || (rep && nrep <= 0) || !upart || nlevels < 1 || nlevels > UL_MAX_LEVELS || nu < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pu_loss_finalize_u_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cd, rep, nrep, wf, rep_w, upart,
                       (long)nlevels * nu, uniform_w, out);
    return (int)hipGetLastError();
}

// dispu_pu_loss_finalize(_u) + the EMD term (model.py:77): emd_cost [b] = dispu_emd_loss_grad's raw costs of (fine, gt), m points per cloud.
DISPU_EXPORT int dispu_pu_loss_finalize_e(const float* cd, const float* rep, long nrep, float wf, float rep_w, const float* upart, int nlevels,
                                          long nu, float uniform_w, const float* emd_cost, const float* radius, int b, int m, float emd_w,
                                          float* out, void* stream) {
    if (!cd || !out || (rep && nrep <= 0) || !emd_cost || b < 1 || m < 1) return (int)hipErrorInvalidValue;
    if (upart && (nlevels < 1 || nlevels > UL_MAX_LEVELS || nu < 1)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pu_loss_finalize_e_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cd, rep, nrep, wf, rep_w, upart,
                       upart ? (long)nlevels * nu : 0l, uniform_w, emd_cost, radius, b, m, emd_w, out);
    return (int)hipGetLastError();
}
