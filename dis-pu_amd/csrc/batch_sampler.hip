// One training batch per launch, every random draw made on the device (DisPU/dataset.py:113-143 and the functions of
// Common/point_operation.py it calls -- nonuniform_sampling :10-18, jitter :74-86, z rotation :32-71, scale :107-123 -- run in numpy on
// a background thread in the reference; dataset.Fetcher repeats those host draws, 5 - 20 ms per batch in front of a 1.5 - 4.7 ms step).
//
// One workgroup of 256 threads per patch.  Patch i of the batch sits at POSITION p = start + i of the epoch's permutation and uses the
// dataset row perm[p].  Every draw comes from Philox4x32-10 with key = seed and counter = (block number, stream id, p, epoch), so a
// patch's draws depend on (seed, epoch, position) only -- not on the batch size, the launch shape or which call produced it:
//   stream 0, block 0      w0 -> loc = u 0.8 + 0.1,  w1 -> angle = u 2 pi,  w2 -> scale = 0.8 + u 0.4   (w3 unused)
//   stream 1, block d      index candidate number d:  z = sqrt(-2 ln(1 - u(w0))) cos(2 pi u(w1)),  a = (int)((loc + 0.3 z) G)
//   stream 2, block k      jitter of input point k:   (n0, n1) = sqrt(-2 ln(1 - u(w0))) (cos, sin)(2 pi u(w1)),
//                                                      n2 = sqrt(-2 ln(1 - u(w2))) cos(2 pi u(w3));  noise = clamp(sigma n, -clip, clip)
// with u(w) = (w >> 8) 2^-24 and the precise logf / sincosf / cosf.
//
// Sub-sample (wave 0): the reference's sequential rejection loop over the candidate sequence a_0, a_1, ... -- skip a < 0 or a >= G,
// collect distinct values until P are held -- evaluated 64 candidates per round.  (int) truncates toward zero like Python's int(), so
// a draw in (-1, 0) is index 0.  Per round: every lane tests the membership bitmap (G bits in LDS); among the lanes that carry the same
// new value the lowest one owns it (LDS atomicMin on a per-index slot: order-free, hence deterministic); a ballot of the owners plus a
// prefix count gives each owner its rank among the round's new values in draw order, and an owner is accepted only while
// held + rank <= P -- exactly the candidates the sequential loop would have taken before the draw that completes the set.  The loop is
// bounded (DISPU_SAMPLER_MAX_ROUNDS); on exhaustion the lowest unused indices fill the set and status[0] is set.  The chosen
// indices are emitted in ascending order (bitmap scan + workgroup prefix sum), then all four waves stream the P + G rows through
// the augmentation of augment_point.h with 16-byte stores.  No atomics on global memory; status is written with plain stores.
#include "augment_point.h"
#include "philox.h"

namespace dispu {

constexpr int kSamplerThreads = 256;
constexpr uint32_t kStreamPatch = 0, kStreamIndex = 1, kStreamJitter = 2;
constexpr float kTwoPi = 6.283185307179586f;

struct SamplerArgs {
    const float* gt_data; const float* input_data; const int* perm;
    float* input; float* gt; float* radius; int* status;
    int* idx_out; float* rot_out; float* scale_out; float* noise_out; uint32_t* raw_out;
    int L, G, P, start, epoch, augment;
    uint32_t k0, k1;
    float sigma, clip;
};

__device__ __forceinline__ float bm_radius(uint32_t w) { return sqrtf(-2.0f * logf(1.0f - philox_u01(w))); }

__device__ __forceinline__ void jitter3(const SamplerArgs& a, uint32_t k, uint32_t p, float& nx, float& ny, float& nz) {
    uint32_t w[4];
    philox4x32_10(k, kStreamJitter, p, (uint32_t)a.epoch, a.k0, a.k1, w);
    float sn, cs;
    sincosf(kTwoPi * philox_u01(w[1]), &sn, &cs);
    const float r0 = bm_radius(w[0]), r1 = bm_radius(w[2]);
    const float n0 = r0 * cs, n1 = r0 * sn, n2 = r1 * cosf(kTwoPi * philox_u01(w[3]));
    nx = fminf(fmaxf(a.sigma * n0, -a.clip), a.clip);
    ny = fminf(fmaxf(a.sigma * n1, -a.clip), a.clip);
    nz = fminf(fmaxf(a.sigma * n2, -a.clip), a.clip);
}

// one point of the output row: the source point (x, y, z), jittered when NOISE (draws of input point k), rotated and scaled
template <bool NOISE>
__device__ __forceinline__ void sample_point(const SamplerArgs& a, float x, float y, float z, int k, uint32_t p, const float* R, float s,
                                             float* o, float* nz) {
    if constexpr (NOISE) {
        jitter3(a, (uint32_t)k, p, nz[0], nz[1], nz[2]);
        augment_jitter(x, y, z, nz[0], nz[1], nz[2]);
    }
    augment_rotate_scale(x, y, z, R, s, o[0], o[1], o[2]);
}

// out[k] = augment(src[sidx ? sidx[k] : k]) for k < n, all threads of the workgroup; 4 points (three 16-byte stores) per thread and
// step where the row allows it.  nout: this row of noise_out or NULL (verification only: scalar stores).
template <bool NOISE>
__device__ __forceinline__ void stream_row(const SamplerArgs& a, const float* __restrict__ src, const int* sidx, int n,
                                           float* __restrict__ out, uint32_t p, const float* R, float s, float* __restrict__ nout) {
    const int tid = threadIdx.x;
    const bool vec = (n & 3) == 0 && (((uintptr_t)out) & 15) == 0 && (sidx || (((uintptr_t)src) & 15) == 0);
    if (vec) {
        for (int q = tid; q < (n >> 2); q += kSamplerThreads) {
            float v[12], o[12], nz[12];
            if (sidx) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t si = (size_t)sidx[4 * q + j] * 3;
                    v[3 * j + 0] = src[si + 0]; v[3 * j + 1] = src[si + 1]; v[3 * j + 2] = src[si + 2];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float4 t = *reinterpret_cast<const float4*>(src + (size_t)q * 12 + 4 * j);
                    v[4 * j + 0] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                sample_point<NOISE>(a, v[3 * j], v[3 * j + 1], v[3 * j + 2], 4 * q + j, p, R, s, o + 3 * j, nz + 3 * j);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                *reinterpret_cast<float4*>(out + (size_t)q * 12 + 4 * j) = make_float4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            if (NOISE && nout) {
#pragma unroll
                for (int j = 0; j < 12; ++j) nout[(size_t)q * 12 + j] = nz[j];
            }
        }
    } else {
        for (int k = tid; k < n; k += kSamplerThreads) {
            float o[3], nz[3];
            const size_t si = (size_t)(sidx ? sidx[k] : k) * 3;
            sample_point<NOISE>(a, src[si + 0], src[si + 1], src[si + 2], k, p, R, s, o, nz);
            out[(size_t)k * 3 + 0] = o[0]; out[(size_t)k * 3 + 1] = o[1]; out[(size_t)k * 3 + 2] = o[2];
            if (NOISE && nout) { nout[(size_t)k * 3 + 0] = nz[0]; nout[(size_t)k * 3 + 1] = nz[1]; nout[(size_t)k * 3 + 2] = nz[2]; }
        }
    }
}

__global__ __launch_bounds__(kSamplerThreads) void sample_batch_kernel(SamplerArgs a) {
    extern __shared__ int smem[];
    __shared__ int wave_tot[kSamplerThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, G = a.G, P = a.P;
    const uint32_t p = (uint32_t)(a.start + i);
    const int W = (G + 31) >> 5;                      // bitmap words (<= 256: one per thread in the emit phase)
    volatile int* bitmap = smem;                      // [W]
    volatile int* tab = smem + W;                     // [G] owner slots during selection, then the P chosen indices
    const bool random = a.input_data == nullptr;

    int row = a.perm[p];
    if ((unsigned)row >= (unsigned)a.L) {             // never index the dataset with a bad permutation entry
        row = 0;
        if (tid == 0) a.status[1] = 1;
    }

    // patch scalars (every thread computes the same values: one Philox block, one sincosf)
    uint32_t w[4];
    philox4x32_10(0u, kStreamPatch, p, (uint32_t)a.epoch, a.k0, a.k1, w);
    const float loc = philox_u01(w[0]) * 0.8f + 0.1f;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    float scale = 1.0f;
    if (a.augment) {
        float sn, cs;
        sincosf(kTwoPi * philox_u01(w[1]), &sn, &cs);
        R[0] = cs; R[1] = -sn; R[3] = sn; R[4] = cs;   // Rz of point_operation.py:48-50, applied as p . R
        scale = 0.8f + philox_u01(w[2]) * 0.4f;
    }
    if (tid == 0) {
        a.radius[i] = 1.0f;
        if (a.scale_out) a.scale_out[i] = scale;
        if (a.raw_out) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a.raw_out[(size_t)i * 4 + j] = w[j];
        }
        if (a.rot_out) {
#pragma unroll
            for (int j = 0; j < 9; ++j) a.rot_out[(size_t)i * 9 + j] = R[j];
        }
    }

    if (random) {
        for (int e = tid; e < W; e += kSamplerThreads) bitmap[e] = 0;
        for (int e = tid; e < G; e += kSamplerThreads) tab[e] = 64;
        __syncthreads();
        if (wave == 0) {
            int held = 0;
            const float fG = (float)G;
            for (int round = 0; round < DISPU_SAMPLER_MAX_ROUNDS && held < P; ++round) {
                uint32_t c[4];
                philox4x32_10((uint32_t)(round * 64 + lane), kStreamIndex, p, (uint32_t)a.epoch, a.k0, a.k1, c);
                const float z = bm_radius(c[0]) * cosf(kTwoPi * philox_u01(c[1]));
                const float x = (loc + 0.3f * z) * fG;
                const bool valid = x > -1.0f && x < fG;                  // (int)x is then in [0, G); false for NaN
                const int v = valid ? (int)x : 0;
                const bool fresh = valid && !((bitmap[v >> 5] >> (v & 31)) & 1);
                if (fresh) atomicMin((int*)&tab[v], lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
                const bool owner = fresh && tab[v] == lane;
                const unsigned long long m = __ballot(owner);
                const int before = __popcll(m & ((1ull << lane) - 1ull));
                if (owner) {
                    if (held + before < P) atomicOr((int*)&bitmap[v >> 5], 1 << (v & 31));
                    tab[v] = 64;
                }
                held = min(P, held + (int)__popcll(m));
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            if (held < P && lane == 0) {                                 // bounded loop exhausted: lowest unused indices, and say so
                int need = P - held;
                for (int e = 0; e < W && need; ++e) {
                    int word = bitmap[e];
                    const int lim = min(32, G - 32 * e);
                    for (int b = 0; b < lim && need; ++b)
                        if (!((word >> b) & 1)) { word |= 1 << b; --need; }
                    bitmap[e] = word;
                }
                a.status[0] = 1;
            }
        }
        __syncthreads();
        // ascending emit: thread t owns bitmap word t; exclusive prefix sum of the popcounts over the workgroup
        const uint32_t word = tid < W ? (uint32_t)bitmap[tid] : 0u;
        const int cnt = __popc(word);
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();                                                 // (also: every thread has read its bitmap word / tab is free)
        int pos = inc - cnt;
        for (int q = 0; q < wave; ++q) pos += wave_tot[q];
        for (uint32_t rest = word; rest; rest &= rest - 1u) tab[pos++] = tid * 32 + (__ffs(rest) - 1);
        __syncthreads();
        if (a.idx_out)
            for (int k = tid; k < P; k += kSamplerThreads) a.idx_out[(size_t)i * P + k] = tab[k];
    } else if (a.idx_out) {
        for (int k = tid; k < P; k += kSamplerThreads) a.idx_out[(size_t)i * P + k] = k;
    }

    const float* grow = a.gt_data + (size_t)row * G * 3;
    float* nout = a.noise_out ? a.noise_out + (size_t)i * P * 3 : nullptr;
    float* xout = a.input + (size_t)i * P * 3;
    const float* xsrc = random ? grow : a.input_data + (size_t)row * P * 3;
    const int* sidx = random ? (const int*)smem + W : nullptr;
    if (a.augment) stream_row<true>(a, xsrc, sidx, P, xout, p, R, scale, nout);
    else stream_row<false>(a, xsrc, sidx, P, xout, p, R, scale, nullptr);
    stream_row<false>(a, grow, nullptr, G, a.gt + (size_t)i * G * 3, p, R, scale, nullptr);
}

}  // namespace dispu

using namespace dispu;

DISPU_EXPORT int dispu_sample_batch(int L, int G, int P, const float* gt_data, const float* input_data, const int* perm, int start, int B,
                                    unsigned long long seed, int epoch, float jitter_sigma, float jitter_clip, int augment, float* input,
                                    float* gt, float* radius, int* status, int* idx_out, float* rot_out, float* scale_out,
                                    float* noise_out, unsigned int* raw_out, void* stream) {
    if (L <= 0 || G <= 0 || P <= 0 || P > G || G > DISPU_SAMPLER_MAX_G || B < 0 || start < 0 || (long)start + B > (long)L || epoch < 0)
        return (int)hipErrorInvalidValue;
    if (!gt_data || !perm || !input || !gt || !radius || !status || (augment && !(jitter_clip > 0.0f)) || (noise_out && !augment))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    SamplerArgs a;
    a.gt_data = gt_data; a.input_data = input_data; a.perm = perm;
    a.input = input; a.gt = gt; a.radius = radius; a.status = status;
    a.idx_out = idx_out; a.rot_out = rot_out; a.scale_out = scale_out; a.noise_out = noise_out; a.raw_out = raw_out;
    a.L = L; a.G = G; a.P = P; a.start = start; a.epoch = epoch; a.augment = augment ? 1 : 0;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.sigma = jitter_sigma; a.clip = jitter_clip;
    const size_t lds = ((size_t)((G + 31) >> 5) + (size_t)G) * sizeof(int);       // <= 33 KB
    hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)B), dim3(kSamplerThreads), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
