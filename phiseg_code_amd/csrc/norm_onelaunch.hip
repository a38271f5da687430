// One-launch normalisation layers for small maps: k_bn_small_* and k_bn_wide_* (batch norm), k_norm_wave_* (group / instance norm).
#include <stdlib.h>
#include <type_traits>

#include "vec_io.h"

// =================================================================================================
// Small-map batch norm (P = B*H*W <= 4096 pixels: the H <= 8 levels).  There the three-launch forward (statistics,
// finalisation + apply) and two-launch backward (reduction, apply) are a chain of 5-10 us latency-bound launches for a
// tensor of at most 1.5 MB.  Here ONE launch does the whole layer: a block owns 16 channels (a 32-byte slice of every
// pixel row) for ALL pixels, keeps its slice in registers (NIT x 16 B per thread), and reduces over pixels inside the
// block -- no atomics, no second launch, exact two-pass variance.  1024 threads = 512 pixel lanes x 2 channel vectors.

// sum of s[0..NV) over the 512 pixel lanes that share this thread's channel vector (threadIdx.x & 1); red: [17][2][NV]
template <int NV>
__device__ __forceinline__ void small_block_sum(float s[NV], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 2; m < 64; m <<= 1)
#pragma unroll
        for (int j = 0; j < NV; ++j) s[j] += __shfl_xor(s[j], m);
    __syncthreads();                                   // red may still be read from the previous call
    if (lane < 2)
#pragma unroll
        for (int j = 0; j < NV; ++j) red[(wave * 2 + lane) * NV + j] = s[j];
    __syncthreads();
    float* tot = red + 16 * 2 * NV;                    // [2][NV]
    if (threadIdx.x < 2 * NV) {
        const int vv = threadIdx.x / NV, j = threadIdx.x % NV;
        float a = 0.f;
        for (int w = 0; w < 16; ++w) a += red[(w * 2 + vv) * NV + j];
        tot[vv * NV + j] = a;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = tot[(threadIdx.x & 1) * NV + j];
}

// XF32 (round 5): the pre-normalisation tensor x is fp32 -- what the split-K convolution of these small maps leaves (its fp32 slices,
// summed) -- and the statistics and the normalisation run on the UNROUNDED values.  A batch-norm layer at 2 x 2 / 4 x 4 normalises a
// few dozen to a few hundred values per channel; when their spread is small against their mean, the bf16 rounding of x (2^-9 of the
// MEAN) is a large fraction of the spread the normalisation blows up to unit variance: measured as a +40 % bias of the two coarsest
// KL terms after 200 training steps (tools/convergence_study.py).  These tensors are < 1 MB: fp32 is free.
template <bool XF32>
struct BnsVec {                                        // eight channels of one pixel in registers: packed bf16 or fp32
    uint4 r; float f[XF32 ? 8 : 1];
    __device__ __forceinline__ void zero() {
        r = make_uint4(0, 0, 0, 0);
        if constexpr (XF32) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = 0.f;
        }
    }
    __device__ __forceinline__ void load(const void* x, size_t i) {
        if constexpr (XF32) {
            typedef __attribute__((ext_vector_type(4))) float f32x4_t;
            const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>((const float*)x + i), a1 = *reinterpret_cast<const f32x4_t*>((const float*)x + i + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[j] = a0[j]; f[4 + j] = a1[j]; }
        } else r = *reinterpret_cast<const uint4*>((const bf16_t*)x + i);
    }
    __device__ __forceinline__ void unpack(float o[8]) const {
        if constexpr (XF32) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = f[j];
        } else bf16x8_unpack(r, o);
    }
};
template <int NIT, bool XF32>
__global__ __launch_bounds__(1024) void k_bn_small_fwd(const void* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, bf16_t* __restrict__ y,
                                                       float* mean_out, float* rstd_out, float* scale_out,
                                                       float* shift_out, float* moving_mean, float* moving_var,
                                                       float momentum, int P, int C, int act) {
    __shared__ float red[17 * 2 * 8];
    const int v = threadIdx.x & 1, pl = threadIdx.x >> 1;
    const int c0 = blockIdx.x * 16 + v * 8;
    BnsVec<XF32> r[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = pl + it * 512;
        r[it].zero();
        if (p < P) r[it].load(x, (size_t)p * C + c0);
    }
    float s[8], mu[8], gm[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; gm[j] = gamma[c0 + j]; be[j] = beta[c0 + j]; }   // (loaded ahead of the reductions)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {                  // (pixels past P hold zeros)
        float f[8];
        r[it].unpack(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += f[j];
    }
    small_block_sum<8>(s, red);
    const float invP = 1.f / (float)P;
#pragma unroll
    for (int j = 0; j < 8; ++j) { mu[j] = s[j] * invP; s[j] = 0.f; }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (pl + it * 512 < P) {
            float f[8];
            r[it].unpack(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = f[j] - mu[j]; s[j] = fmaf(d, d, s[j]); }
        }
    }
    small_block_sum<8>(s, red);
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        const float var = s[j] * invP, rs = rsqrtf(var + eps);
        sc[j] = gm[j] * rs;
        sh[j] = be[j] - mu[j] * sc[j];
        if (pl == 0) {
            mean_out[c] = mu[j];
            rstd_out[c] = rs;
            scale_out[c] = sc[j];
            shift_out[c] = sh[j];
            if (momentum > 0.f && moving_mean) {          // TF1 fused-batch-norm moving update (unbiased variance)
                const float m = (float)P;
                moving_mean[c] -= (moving_mean[c] - mu[j]) * momentum;
                moving_var[c] -= (moving_var[c] - var * (m / fmaxf(m - 1.f, 1.f))) * momentum;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = pl + it * 512;
        if (p < P) {
            float f[8];
            r[it].unpack(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = act_fwd(fmaf(f[j], sc[j], sh[j]), act);
            VecIO<bf16_t, 8>::store(y, (size_t)p * C + c0, f);
        }
    }
}

template <int NIT, bool XF32>
__global__ __launch_bounds__(1024) void k_bn_small_bwd(const bf16_t* __restrict__ dA, const void* __restrict__ x,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, bf16_t* __restrict__ dx,
                                                       float* dgamma, float* dbeta, int P, int C, int act) {
    __shared__ float red[17 * 2 * 16];
    const int v = threadIdx.x & 1, pl = threadIdx.x >> 1;
    const int c0 = blockIdx.x * 16 + v * 8;
    // the slice stays in registers between the two passes when that is <= 4 x 16 B per thread; larger slices are read
    // again (from L2) -- 2 x 8 x 16 B per thread on top of the unpacked working set does not fit 128 registers
    constexpr bool KEEP = NIT <= 2;
    constexpr int NB = KEEP ? NIT : 2;                 // register buffers (reads go two pixels at a time when not kept)
    BnsVec<XF32> rx[NB];
    uint4 rd[NB];
    auto fetch = [&](int it) {
        const int p = pl + it * 512;
        rx[it % NB].zero();
        rd[it % NB] = make_uint4(0, 0, 0, 0);
        if (p < P) {
            rx[it % NB].load(x, (size_t)p * C + c0);
            rd[it % NB] = *reinterpret_cast<const uint4*>(dA + (size_t)p * C + c0);
        }
    };
    if constexpr (KEEP) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) fetch(it);
    }
    float sc[8], sh[8], mu[8], rs[8], gmv[8], s[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; rs[j] = rstd[c]; gmv[j] = gamma[c];
        s[j] = s[8 + j] = 0.f;
    }
    auto accumulate = [&](int it) {                     // (pixels past P: dA = 0 -> g = 0)
        float xf[8], df[8];
        rx[it % NB].unpack(xf);
        bf16x8_unpack(rd[it % NB], df);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float g = df[j] * act_grad_pre(fmaf(xf[j], sc[j], sh[j]), act);
            s[j] += g;
            s[8 + j] = fmaf(g * (xf[j] - mu[j]), rs[j], s[8 + j]);
        }
    };
    if constexpr (KEEP) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) accumulate(it);
    } else {
#pragma unroll 1
        for (int it = 0; it < NIT; it += 2) { fetch(it); fetch(it + 1); accumulate(it); accumulate(it + 1); }
    }
    small_block_sum<16>(s, red);
    const float inv_m = 1.f / (float)P;
    float ca[8], cb[8], cc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        const float gm = gmv[j];
        ca[j] = rs[j] * gm;
        cc[j] = -rs[j] * rs[j] * gm * s[8 + j] * inv_m;
        cb[j] = -rs[j] * gm * s[j] * inv_m - cc[j] * mu[j];
        if (pl == 0) {                                  // (accumulate: a variable may be used by several layers)
            atomicAdd(&dbeta[c], s[j]);
            atomicAdd(&dgamma[c], s[8 + j]);
        }
    }
    auto apply = [&](int it) {
        const int p = pl + it * 512;
        if (p < P) {
            float xf[8], df[8], o[8];
            rx[it % NB].unpack(xf);
            bf16x8_unpack(rd[it % NB], df);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float gq = df[j] * act_grad_pre(fmaf(xf[j], sc[j], sh[j]), act);
                o[j] = fmaf(ca[j], gq, fmaf(cc[j], xf[j], cb[j]));
            }
            VecIO<bf16_t, 8>::store(dx, (size_t)p * C + c0, o);
        }
    };
    if constexpr (KEEP) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) apply(it);
    } else {
#pragma unroll 1
        for (int it = 0; it < NIT; it += 2) { fetch(it); fetch(it + 1); apply(it); apply(it + 1); }
    }
}

// ---- the WIDE form of the one-launch batch norm (round 5): P <= 1024 pixels (the 2 x 2 / 4 x 4 levels at batch 64), fp32
// pre-normalisation tensor given as the nz split-K slices the convolution left -- this launch is also the split-K finishing pass.
// A block of 256 threads owns FOUR channels of all pixels (one float4 per pixel and slice), so a 192-channel layer is 48 blocks on
// 48 CUs instead of 12: the layer is a few hundred KB to a few MB of slices, and what a launch of this size costs is the number of
// loads a CU has in flight, not arithmetic (k_splitk_finish + k_bn_small_fwd: 4.8 + 10.6 us and a launch boundary; this: one launch).
// The slices are added in slice order, as k_splitk_finish adds them: xsum (written for the backward pass when nz > 1) is bit-identical.
__device__ __forceinline__ f32x4 wide_block_sum(f32x4 s, float* red /* [4 waves][4] */) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += __shfl_xor(s[j], m);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<f32x4*>(red + wave * 4) = s;
    __syncthreads();
    f32x4 t = *reinterpret_cast<const f32x4*>(red);
#pragma unroll
    for (int w = 1; w < 4; ++w) t += *reinterpret_cast<const f32x4*>(red + w * 4);
    return t;
}
template <int NPT>
__global__ __launch_bounds__(256) void k_bn_wide_fwd(const float* __restrict__ xs, int nz, size_t zstride, float* __restrict__ xsum,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     bf16_t* __restrict__ y, float* mean_out, float* rstd_out, float* scale_out,
                                                     float* shift_out, float* moving_mean, float* moving_var, float momentum,
                                                     int P, int C, int act) {
    __shared__ __attribute__((aligned(16))) float red[2][16];
    const int c0 = blockIdx.x * 4;
    f32x4 v[NPT];
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
        const int p = threadIdx.x + it * 256;
        v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < P) v[it] = *reinterpret_cast<const f32x4*>(xs + (size_t)p * C + c0);
    }
    for (int z0 = 1; z0 < nz; z0 += 4) {                 // four slices of every pixel in flight; added in slice order
        f32x4 t[NPT][4];
#pragma unroll
        for (int it = 0; it < NPT; ++it) {
            const int p = threadIdx.x + it * 256;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                t[it][k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (p < P && z0 + k < nz) t[it][k] = *reinterpret_cast<const f32x4*>(xs + (size_t)(z0 + k) * zstride + (size_t)p * C + c0);
            }
        }
#pragma unroll
        for (int it = 0; it < NPT; ++it)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (z0 + k < nz) v[it] += t[it][k];
    }
    if (nz > 1 && xsum != nullptr) {
#pragma unroll
        for (int it = 0; it < NPT; ++it) {
            const int p = threadIdx.x + it * 256;
            if (p < P) *reinterpret_cast<f32x4*>(xsum + (size_t)p * C + c0) = v[it];
        }
    }
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c0), be = *reinterpret_cast<const f32x4*>(beta + c0);
    f32x4 s = v[0];
#pragma unroll
    for (int it = 1; it < NPT; ++it) s += v[it];                         // (pixels past P hold zeros)
    const float invP = 1.f / (float)P;
    const f32x4 mu = wide_block_sum(s, red[0]) * invP;
    s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < NPT; ++it)
        if ((int)threadIdx.x + it * 256 < P) { const f32x4 d = v[it] - mu; s += d * d; }
    const f32x4 var = wide_block_sum(s, red[1]) * invP;
    f32x4 sc, sh;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float rs = rsqrtf(var[j] + eps);
        sc[j] = gm[j] * rs;
        sh[j] = be[j] - mu[j] * sc[j];
        if (threadIdx.x == 0) {
            const int c = c0 + j;
            mean_out[c] = mu[j];
            rstd_out[c] = rs;
            scale_out[c] = sc[j];
            shift_out[c] = sh[j];
            if (momentum > 0.f && moving_mean) {          // TF1 fused-batch-norm moving update (unbiased variance)
                const float m = (float)P;
                moving_mean[c] -= (moving_mean[c] - mu[j]) * momentum;
                moving_var[c] -= (moving_var[c] - var[j] * (m / fmaxf(m - 1.f, 1.f))) * momentum;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
        const int p = threadIdx.x + it * 256;
        if (p < P) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = act_fwd(fmaf(v[it][j], sc[j], sh[j]), act);
            *reinterpret_cast<uint2*>(y + (size_t)p * C + c0) = make_uint2(f2bf_pk(o[0], o[1]), f2bf_pk(o[2], o[3]));
        }
    }
}
// ... and its backward: dA (bf16, or the nzd fp32 split-K slices the consumer's data gradient left -- das != NULL), the fp32 x
template <int NPT>
__global__ __launch_bounds__(256) void k_bn_wide_bwd(const bf16_t* __restrict__ dA, const float* __restrict__ das, int nzd, size_t zstride,
                                                     const float* __restrict__ x, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     bf16_t* __restrict__ dx, float* dgamma, float* dbeta, int P, int C, int act) {
    __shared__ __attribute__((aligned(16))) float red[2][16];
    const int c0 = blockIdx.x * 4;
    f32x4 xv[NPT], g[NPT];
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
        const int p = threadIdx.x + it * 256;
        xv[it] = g[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < P) {
            xv[it] = *reinterpret_cast<const f32x4*>(x + (size_t)p * C + c0);
            if (das == nullptr) {
                const uint2 r = *reinterpret_cast<const uint2*>(dA + (size_t)p * C + c0);
                g[it] = f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
            } else g[it] = *reinterpret_cast<const f32x4*>(das + (size_t)p * C + c0);
        }
    }
    if (das != nullptr) {
        for (int z0 = 1; z0 < nzd; z0 += 4) {
            f32x4 t[NPT][4];
#pragma unroll
            for (int it = 0; it < NPT; ++it) {
                const int p = threadIdx.x + it * 256;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    t[it][k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (p < P && z0 + k < nzd) t[it][k] = *reinterpret_cast<const f32x4*>(das + (size_t)(z0 + k) * zstride + (size_t)p * C + c0);
                }
            }
#pragma unroll
            for (int it = 0; it < NPT; ++it)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (z0 + k < nzd) g[it] += t[it][k];
        }
        // (the bf16 tensor the finishing pass would have written is what every other consumer of this gradient sees: round the
        // same way, so that the two forms of this launch agree bit for bit)
#pragma unroll
        for (int it = 0; it < NPT; ++it) {
            const unsigned w0 = f2bf_pk(g[it][0], g[it][1]), w1 = f2bf_pk(g[it][2], g[it][3]);
            g[it] = f32x4{__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u), __uint_as_float(w1 << 16), __uint_as_float(w1 & 0xffff0000u)};
        }
    }
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c0), sh = *reinterpret_cast<const f32x4*>(shift + c0);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c0), rs = *reinterpret_cast<const f32x4*>(rstd + c0);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c0);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < NPT; ++it) {                  // (pixels past P: dA = 0 -> g = 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[it][j] *= act_grad_pre(fmaf(xv[it][j], sc[j], sh[j]), act);
            s1[j] += g[it][j];
            s2[j] = fmaf(g[it][j] * (xv[it][j] - mu[j]), rs[j], s2[j]);
        }
    }
    s1 = wide_block_sum(s1, red[0]);
    s2 = wide_block_sum(s2, red[1]);
    const float inv_m = 1.f / (float)P;
    f32x4 ca, cb, cc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ca[j] = rs[j] * gm[j];
        cc[j] = -rs[j] * rs[j] * gm[j] * s2[j] * inv_m;
        cb[j] = -rs[j] * gm[j] * s1[j] * inv_m - cc[j] * mu[j];
        if (threadIdx.x == 0) {                         // (accumulate: a variable may be used by several layers)
            atomicAdd(&dbeta[c0 + j], s1[j]);
            atomicAdd(&dgamma[c0 + j], s2[j]);
        }
    }
#pragma unroll
    for (int it = 0; it < NPT; ++it) {
        const int p = threadIdx.x + it * 256;
        if (p < P) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf(ca[j], g[it][j], fmaf(cc[j], xv[it][j], cb[j]));
            *reinterpret_cast<uint2*>(dx + (size_t)p * C + c0) = make_uint2(f2bf_pk(o[0], o[1]), f2bf_pk(o[2], o[3]));
        }
    }
}

// =================================================================================================
// Group / instance norm on small maps (a sample has P = H*W <= 256 pixels: the H <= 16 levels), bf16 NHWC: the whole layer
// in one launch, like k_bn_small_* -- but the statistics are per SAMPLE, so nothing is reduced across waves: a wave owns
// (sample, 16-channel slice) pairs, lane = (sample slot, pixel lane, channel vector); LPS pixel lanes per sample (4, 16 or
// 32 -> 8, 2 or 1 samples per wave pass), NIT pixels per lane, reductions by wave shuffles only, no barrier in the forward
// pass.  MODE 0: one statistic per channel (instance norm); MODE 1: one per 16-channel group = the whole slice (group_norm2D's
// default groups for C >= 32).  A block (4 waves) walks a run of samples; the backward pass keeps dgamma / dbeta / dbias of
// its run in registers and adds them once per block.
template <int LPS> struct NormWaveMap {
    static constexpr int SPW = 32 / LPS;               // samples per wave pass
    int v, q, ss;
    __device__ __forceinline__ NormWaveMap() {
        const int l = threadIdx.x & 63;
        v = l & 1;
        q = (l >> 1) & (LPS - 1);
        ss = l / (2 * LPS);
    }
};
template <int LPS, int NV>
__device__ __forceinline__ void wave_pixel_sum(float s[NV]) {     // over the LPS pixel lanes of a sample slot (lane bits 1..)
#pragma unroll
    for (int m = 2; m <= LPS; m <<= 1)
#pragma unroll
        for (int j = 0; j < NV; ++j) s[j] += __shfl_xor(s[j], m);
}
__device__ __forceinline__ float slice16_total(const float t[8]) {   // sum over the 16 channels of the slice (both channel vectors)
    float g = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    return g + __shfl_xor(g, 1);
}

template <int LPS, int NIT, int MODE, bool SLICES>
__global__ __launch_bounds__(256) void k_norm_wave_fwd(bf16_t* __restrict__ x, const float* __restrict__ ws, int nz,
                                                      const float* __restrict__ bias, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, bf16_t* __restrict__ y,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                      float* __restrict__ scale_out, float* __restrict__ shift_out, int NS,
                                                      int P, int C, int passes, int act) {
    const NormWaveMap<LPS> m;
    constexpr int SPW = NormWaveMap<LPS>::SPW;
    const int wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 16 + m.v * 8;
    const int G = gridDim.x;
    float gm[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { gm[j] = gamma[c0 + j]; be[j] = beta[c0 + j]; }
    const float inv_m = 1.f / ((float)P * (MODE == 1 ? 16.f : 1.f));
    const float lo = act == PHX_ACT_RELU ? 0.f : -INFINITY;     // (uniform activation: see k_norm_wave_bwd)
    auto run = [&](auto softc) {
    constexpr bool SOFT = decltype(softc)::value;
    for (int i = 0; i < passes; ++i) {
        const int ns = ((blockIdx.y * passes + i) * 4 + wave) * SPW + m.ss;
        const bool live = ns < NS;
        const size_t base = (size_t)ns * P * C + c0;
        uint4 r[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = m.q + it * LPS;
            r[it] = make_uint4(0, 0, 0, 0);
            if (live && p < P) {
                if constexpr (SLICES) {
                    typedef __attribute__((ext_vector_type(4))) float f32x4_t;
                    const size_t zs = (size_t)NS * P * C;
                    const float* qp = ws + base + (size_t)p * C;
                    f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(qp), a1 = *reinterpret_cast<const f32x4_t*>(qp + 4);
                    for (int z = 1; z < nz; ++z) {
                        a0 += *reinterpret_cast<const f32x4_t*>(qp + (size_t)z * zs);
                        a1 += *reinterpret_cast<const f32x4_t*>(qp + (size_t)z * zs + 4);
                    }
                    if (bias) {
                        a0 += *reinterpret_cast<const f32x4_t*>(bias + c0);
                        a1 += *reinterpret_cast<const f32x4_t*>(bias + c0 + 4);
                    }
                    r[it] = make_uint4(f2bf_pk(a0[0], a0[1]), f2bf_pk(a0[2], a0[3]), f2bf_pk(a1[0], a1[1]), f2bf_pk(a1[2], a1[3]));
                    *reinterpret_cast<uint4*>(x + base + (size_t)p * C) = r[it];
                } else {
                    r[it] = *reinterpret_cast<const uint4*>(x + base + (size_t)p * C);
                }
            }
        }
        float s[8], mu[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {                  // (pixels past P hold zeros)
            float f[8];
            bf16x8_unpack(r[it], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += f[j];
        }
        wave_pixel_sum<LPS, 8>(s);
        if constexpr (MODE == 1) {
            const float g = slice16_total(s);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = g;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { mu[j] = s[j] * inv_m; s[j] = 0.f; }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (m.q + it * LPS < P) {
                float f[8];
                bf16x8_unpack(r[it], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = f[j] - mu[j]; s[j] = fmaf(d, d, s[j]); }
            }
        }
        wave_pixel_sum<LPS, 8>(s);
        if constexpr (MODE == 1) {
            const float g = slice16_total(s);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = g;
        }
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            const float rs = rsqrtf(s[j] * inv_m + eps);
            sc[j] = gm[j] * rs;
            sh[j] = be[j] - mu[j] * sc[j];
            if (live && m.q == 0) {
                if constexpr (MODE == 1) {
                    if (m.v == 0 && j == 0) {
                        mean_out[(size_t)ns * G + blockIdx.x] = mu[j];
                        rstd_out[(size_t)ns * G + blockIdx.x] = rs;
                    }
                } else {
                    mean_out[(size_t)ns * C + c] = mu[j];
                    rstd_out[(size_t)ns * C + c] = rs;
                }
                scale_out[(size_t)ns * C + c] = sc[j];
                shift_out[(size_t)ns * C + c] = sh[j];
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = m.q + it * LPS;
            if (live && p < P) {
                float f[8];
                bf16x8_unpack(r[it], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float v = fmaf(f[j], sc[j], sh[j]); f[j] = SOFT ? act_fwd(v, PHX_ACT_SOFTPLUS) : fmaxf(v, lo); }
                VecIO<bf16_t, 8>::store(y, base + (size_t)p * C, f);
            }
        }
    }
    };
    if (act == PHX_ACT_SOFTPLUS) run(std::true_type()); else run(std::false_type());
}

// dbias: the gradient of a convolution bias in front of the normalisation, sum over samples and pixels of dx, in closed form
// per sample (a * sum g + c * sum (x - mean) - P * rstd * S0 / m; identically zero in MODE 0, not computed there)
template <int LPS, int NIT, int MODE>
__global__ __launch_bounds__(256) void k_norm_wave_bwd(const bf16_t* __restrict__ dA, const bf16_t* __restrict__ x,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, bf16_t* __restrict__ dx,
                                                      float* dgamma, float* dbeta, float* dbias, int NS, int P, int C,
                                                      int passes, int act) {
    constexpr int NA = MODE == 1 ? 24 : 16;
    const NormWaveMap<LPS> m;
    constexpr int SPW = NormWaveMap<LPS>::SPW;
    __shared__ float red[4 * SPW * 2 * NA];
    const int wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 16 + m.v * 8;
    const int G = gridDim.x;
    float gmv[8], acc[NA];
#pragma unroll
    for (int j = 0; j < 8; ++j) gmv[j] = gamma[c0 + j];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.f;
    const float inv_m = 1.f / ((float)P * (MODE == 1 ? 16.f : 1.f));
    // The activation is uniform per launch: ReLU / identity through a threshold, softplus in its own copy of the loop.  With
    // act_grad_pre(pre, act) per element this kernel carried two scalar branches per element (585 in the 256-pixel instantiation,
    // 8 777 instructions; 90 and 5 143 now).  NOT done in the streaming kernels below: measured slower there.
    const float thr = act == PHX_ACT_RELU ? 0.f : -INFINITY;
    auto run = [&](auto softc) {
    constexpr bool SOFT = decltype(softc)::value;
    for (int i = 0; i < passes; ++i) {
        const int ns = ((blockIdx.y * passes + i) * 4 + wave) * SPW + m.ss;
        const bool live = ns < NS;
        const size_t base = (size_t)ns * P * C + c0;
        uint4 rx[NIT], rd[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = m.q + it * LPS;
            rx[it] = rd[it] = make_uint4(0, 0, 0, 0);
            if (live && p < P) {
                rx[it] = *reinterpret_cast<const uint4*>(x + base + (size_t)p * C);
                rd[it] = *reinterpret_cast<const uint4*>(dA + base + (size_t)p * C);
            }
        }
        float sc[8], sh[8], mu[8], rs[8], s[NA];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            const size_t si = MODE == 1 ? (size_t)ns * G + blockIdx.x : (size_t)ns * C + c;
            sc[j] = live ? scale[(size_t)ns * C + c] : 0.f;
            sh[j] = live ? shift[(size_t)ns * C + c] : 0.f;
            mu[j] = live ? mean[si] : 0.f;
            rs[j] = live ? rstd[si] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NA; ++j) s[j] = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {              // (pixels past P: dA = 0 -> g = 0)
            float xf[8], df[8];
            bf16x8_unpack(rx[it], xf);
            bf16x8_unpack(rd[it], df);
            const bool in = live && m.q + it * LPS < P;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float pre = fmaf(xf[j], sc[j], sh[j]);
                const float g = SOFT ? df[j] * act_grad_pre(pre, PHX_ACT_SOFTPLUS) : (pre > thr ? df[j] : 0.f);
                s[j] += g;
                s[8 + j] = fmaf(g * (xf[j] - mu[j]), rs[j], s[8 + j]);
                if constexpr (MODE == 1) s[16 + j] += in ? xf[j] - mu[j] : 0.f;
            }
        }
        wave_pixel_sum<LPS, NA>(s);
        float S0[8], S1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { S0[j] = gmv[j] * s[j]; S1[j] = gmv[j] * s[8 + j]; }
        if constexpr (MODE == 1) {                      // S = sum over the group's 16 channels of gamma_c * {sum g, sum g xhat}
            const float a = slice16_total(S0), bq = slice16_total(S1);
#pragma unroll
            for (int j = 0; j < 8; ++j) { S0[j] = a; S1[j] = bq; }
        }
        float ca[8], cb[8], cc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ca[j] = rs[j] * gmv[j];
            cc[j] = -rs[j] * rs[j] * S1[j] * inv_m;
            cb[j] = -rs[j] * S0[j] * inv_m - cc[j] * mu[j];
            acc[j] += s[j];
            acc[8 + j] += s[8 + j];
            if constexpr (MODE == 1) acc[16 + j] += fmaf(ca[j], s[j], fmaf(cc[j], s[16 + j], -(float)P * rs[j] * S0[j] * inv_m));
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = m.q + it * LPS;
            if (live && p < P) {
                float xf[8], df[8], o[8];
                bf16x8_unpack(rx[it], xf);
                bf16x8_unpack(rd[it], df);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float pre = fmaf(xf[j], sc[j], sh[j]);
                    const float gq = SOFT ? df[j] * act_grad_pre(pre, PHX_ACT_SOFTPLUS) : (pre > thr ? df[j] : 0.f);
                    o[j] = fmaf(ca[j], gq, fmaf(cc[j], xf[j], cb[j]));
                }
                VecIO<bf16_t, 8>::store(dx, base + (size_t)p * C, o);
            }
        }
    }
    };
    if (act == PHX_ACT_SOFTPLUS) run(std::true_type()); else run(std::false_type());
    // the block's run of samples: one add per channel (every pixel lane of a slot holds the slot's totals; lane q == 0 speaks)
    if (m.q == 0)
#pragma unroll
        for (int j = 0; j < NA; ++j) red[((wave * SPW + m.ss) * 2 + m.v) * NA + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 2 * NA) {
        const int vv = threadIdx.x / NA, j = threadIdx.x % NA;
        float a = 0.f;
        for (int w = 0; w < 4 * SPW; ++w) a += red[(w * 2 + vv) * NA + j];
        const int c = blockIdx.x * 16 + vv * 8 + (j & 7);
        if (j < 8) atomicAdd(&dbeta[c], a);
        else if (j < 16) atomicAdd(&dgamma[c], a);
        else if (dbias) atomicAdd(&dbias[c], a);
    }
}

extern "C" {

int phx_bn_small_supported(int P, int C, int dt) { return dt == PHX_BF16 && P >= 1 && P <= 4096 && C % 16 == 0; }

int phx_bn_small_fwd(const void* x, int x_dt, const float* gamma, const float* beta, float eps, void* y, float* mean, float* rstd,
                     float* scale, float* shift, float* moving_mean, float* moving_var, float momentum, int P, int C,
                     int act, void* stream) {
    PHX_REQUIRE(phx_bn_small_supported(P, C, PHX_BF16), PHX_E_SHAPE, "bn_small_fwd: needs bf16 output, P <= 4096, C % 16 == 0");
    PHX_REQUIRE(x_dt == PHX_BF16 || (x_dt == PHX_F32 && P <= 1024), PHX_E_INVAL, "bn_small_fwd: x is bf16, or fp32 with P <= 1024");
#define BNS_F(NITv, XFv)                                                                                              \
    hipLaunchKernelGGL((k_bn_small_fwd<NITv, XFv>), dim3(C / 16), dim3(1024), 0, (hipStream_t)stream, x, gamma, beta, eps, \
                       (bf16_t*)y, mean, rstd, scale, shift, moving_mean, moving_var, momentum, P, C, act)
    if (x_dt == PHX_F32) { if (P <= 512) BNS_F(1, true); else BNS_F(2, true); }
    else if (P <= 512) BNS_F(1, false); else if (P <= 1024) BNS_F(2, false); else if (P <= 2048) BNS_F(4, false); else BNS_F(8, false);
#undef BNS_F
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_bn_small_bwd(const void* dA, const void* x, int x_dt, const float* scale, const float* shift, const float* mean,
                     const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, int P, int C, int act,
                     void* stream) {
    PHX_REQUIRE(phx_bn_small_supported(P, C, PHX_BF16), PHX_E_SHAPE, "bn_small_bwd: needs bf16 gradients, P <= 4096, C % 16 == 0");
    PHX_REQUIRE(x_dt == PHX_BF16 || (x_dt == PHX_F32 && P <= 1024), PHX_E_INVAL, "bn_small_bwd: x is bf16, or fp32 with P <= 1024");
#define BNS_B(NITv, XFv)                                                                                              \
    hipLaunchKernelGGL((k_bn_small_bwd<NITv, XFv>), dim3(C / 16), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)dA, \
                       x, scale, shift, mean, rstd, gamma, (bf16_t*)dx, dgamma, dbeta, P, C, act)
    if (x_dt == PHX_F32) { if (P <= 512) BNS_B(1, true); else BNS_B(2, true); }
    else if (P <= 512) BNS_B(1, false); else if (P <= 1024) BNS_B(2, false); else if (P <= 2048) BNS_B(4, false); else BNS_B(8, false);
#undef BNS_B
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

// the wide form (k_bn_wide_*): fp32 x given as nz split-K slices xs[z][P][C] (nz >= 1), 4 channels per block
int phx_bn_wide_supported(int P, int C) { return (P >= 1 && P <= 1024 && C % 4 == 0) ? 1 : 0; }
int phx_bn_wide_fwd(const float* xs, int nz, float* xsum, const float* gamma, const float* beta, float eps, void* y, float* mean,
                    float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var, float momentum, int P, int C,
                    int act, void* stream) {
    PHX_REQUIRE(phx_bn_wide_supported(P, C) && nz >= 1, PHX_E_SHAPE, "bn_wide_fwd: needs P <= 1024, C % 4 == 0, nz >= 1");
    PHX_REQUIRE(xs && y && mean && rstd && scale && shift && (nz == 1 || xsum), PHX_E_INVAL, "bn_wide_fwd: null argument (xsum is required when nz > 1)");
    PHX_REQUIRE((((uintptr_t)xs | (uintptr_t)xsum | (uintptr_t)y) & 15) == 0, PHX_E_ALIGN, "bn_wide_fwd: 16-byte alignment");
#define BNW_F(NPTv)                                                                                                    \
    hipLaunchKernelGGL((k_bn_wide_fwd<NPTv>), dim3(C / 4), dim3(256), 0, (hipStream_t)stream, xs, nz, (size_t)P * C, xsum, gamma, \
                       beta, eps, (bf16_t*)y, mean, rstd, scale, shift, moving_mean, moving_var, momentum, P, C, act)
    if (P <= 256) BNW_F(1); else if (P <= 512) BNW_F(2); else BNW_F(4);
#undef BNW_F
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_bn_wide_bwd(const void* dA, const float* dA_slices, int nzd, const float* x, const float* scale, const float* shift,
                    const float* mean, const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, int P, int C,
                    int act, void* stream) {
    PHX_REQUIRE(phx_bn_wide_supported(P, C), PHX_E_SHAPE, "bn_wide_bwd: needs P <= 1024, C % 4 == 0");
    PHX_REQUIRE((dA != nullptr) != (dA_slices != nullptr) && (dA_slices == nullptr || nzd >= 1) && x && dx, PHX_E_INVAL,
                "bn_wide_bwd: exactly one of dA / dA_slices");
#define BNW_B(NPTv)                                                                                                    \
    hipLaunchKernelGGL((k_bn_wide_bwd<NPTv>), dim3(C / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dA, dA_slices, nzd, \
                       (size_t)P * C, x, scale, shift, mean, rstd, gamma, (bf16_t*)dx, dgamma, dbeta, P, C, act)
    if (P <= 256) BNW_B(1); else if (P <= 512) BNW_B(2); else BNW_B(4);
#undef BNW_B
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

// ---- group / instance norm, one launch per layer on maps of up to 256 pixels (k_norm_wave_*) ----
int phx_norm_small_supported(int NS, int P, int C, int G, int dt) {
    return dt == PHX_BF16 && NS >= 1 && P >= 1 && P <= 256 && C % 16 == 0 && (G == C || G * 16 == C);
}
// pixel lanes per sample (4, 16, 32), samples per block pass, block passes and sample blocks for the (C / 16, nsb) grid
static void norm_wave_plan(int NS, int P, int C, int* lps, int* passes, int* nsb) {
    *lps = P <= 4 ? 4 : P <= 16 ? 16 : 32;
    const int spb = 4 * (32 / *lps);                           // samples per block pass (4 waves)
    const int need = (NS + spb - 1) / spb;                     // block passes in all
    int want = 512 / (C / 16);                                 // sample blocks for ~512 blocks
    if (want < 1) want = 1;
    if (phx_deterministic()) want = 1;                         // one block per slice: a fixed order for dgamma / dbeta / dbias
    *nsb = need < want ? need : want;
    *passes = (need + *nsb - 1) / *nsb;
    *nsb = (need + *passes - 1) / *passes;
}
#define PHX_NW_SWITCH(P, ...)                                                                                        \
    do {                                                                                                             \
        if ((P) <= 4) { constexpr int LPSv = 4, NITv = 1; __VA_ARGS__; }                                             \
        else if ((P) <= 16) { constexpr int LPSv = 16, NITv = 1; __VA_ARGS__; }                                      \
        else if ((P) <= 32) { constexpr int LPSv = 32, NITv = 1; __VA_ARGS__; }                                      \
        else if ((P) <= 64) { constexpr int LPSv = 32, NITv = 2; __VA_ARGS__; }                                      \
        else if ((P) <= 128) { constexpr int LPSv = 32, NITv = 4; __VA_ARGS__; }                                     \
        else { constexpr int LPSv = 32, NITv = 8; __VA_ARGS__; }                                                     \
    } while (0)

int phx_norm_small_fwd(void* x, const float* ws, int nz, const float* bias, const float* gamma, const float* beta, float eps,
                       void* y, float* mean, float* rstd, float* scale, float* shift, int NS, int P, int C, int G, int act,
                       void* stream) {
    PHX_REQUIRE(phx_norm_small_supported(NS, P, C, G, PHX_BF16), PHX_E_SHAPE,
                "norm_small_fwd: needs bf16, P <= 256, C % 16 == 0, per-channel statistics or 16-channel groups");
    PHX_REQUIRE(x != nullptr && (ws == nullptr || nz >= 1), PHX_E_INVAL, "norm_small_fwd: x (and nz >= 1 with ws)");
    PHX_REQUIRE(ws != nullptr || bias == nullptr, PHX_E_INVAL, "norm_small_fwd: bias only with split-K slices");
    int lps, passes, nsb;
    norm_wave_plan(NS, P, C, &lps, &passes, &nsb);
    PHX_REQUIRE(passes < 65536 && nsb < 65536, PHX_E_SHAPE, "norm_small_fwd: too many samples");
    const dim3 grid(C / 16, nsb);
#define NW_F(SLv, Mv)                                                                                                           \
    PHX_NW_SWITCH(P, hipLaunchKernelGGL((k_norm_wave_fwd<LPSv, NITv, Mv, SLv>), grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, ws, \
                                        nz, bias, gamma, beta, eps, (bf16_t*)y, mean, rstd, scale, shift, NS, P, C, passes, act))
    if (ws) { if (G == C) NW_F(true, 0); else NW_F(true, 1); }
    else { if (G == C) NW_F(false, 0); else NW_F(false, 1); }
#undef NW_F
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_small_bwd(const void* dA, const void* x, const float* scale, const float* shift, const float* mean,
                       const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, float* dbias, int NS, int P,
                       int C, int G, int act, void* stream) {
    PHX_REQUIRE(phx_norm_small_supported(NS, P, C, G, PHX_BF16), PHX_E_SHAPE,
                "norm_small_bwd: needs bf16, P <= 256, C % 16 == 0, per-channel statistics or 16-channel groups");
    int lps, passes, nsb;
    norm_wave_plan(NS, P, C, &lps, &passes, &nsb);
    PHX_REQUIRE(passes < 65536 && nsb < 65536, PHX_E_SHAPE, "norm_small_bwd: too many samples");
    const dim3 grid(C / 16, nsb);
#define NW_B(Mv)                                                                                                                \
    PHX_NW_SWITCH(P, hipLaunchKernelGGL((k_norm_wave_bwd<LPSv, NITv, Mv>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dA,   \
                                        (const bf16_t*)x, scale, shift, mean, rstd, gamma, (bf16_t*)dx, dgamma, dbeta, dbias, NS, P, C, passes, act))
    if (G == C) NW_B(0); else NW_B(1);                  // (per-channel statistics: the bias gradient is identically zero)
#undef NW_B
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
