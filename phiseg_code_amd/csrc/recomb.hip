// prob_unet2D's recombination chain for n samples per image in ONE launch (reference likelihoods.py:147-157):
//   concat[feat, broadcast z] -> three 1x1 conv units (KF + Z -> 32 -> 32 -> 32, inference-mode norm folded to scale / shift, ReLU) -> 1x1 head
//   [-> soft-max], with the U-Net's feature map read once per pixel tile and shared by the tile's samples.
//
// The chain is written transposed -- channels on the MFMA rows, pixels on the lanes:  A_l^T [cout][pixel] = W_l^T [cout][k] . A_{l-1}^T
// [k][pixel].  A 32 x 32 fp32 accumulator of v_mfma_f32_32x32x16_bf16 holds column (pixel) lane & 31 and rows (channels)
// (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); registers 8s .. 8s + 7, converted pairwise to bf16, ARE the B fragment of k-step s of the
// next product, in the permuted k order  k(s, h, j) = 16 s + 8 (j >> 2) + 4 h + (j & 3)  -- so the filters of layers 1 and 2 are
// loaded as A fragments in that same order (layer 0 reads the feature map from memory: natural order on both sides).  No activation
// ever touches LDS or memory.
//
// Rounding points of the PHX_BF16 form (include/phx.h): W0[:KF], W1, W2 and a0, a1 are rounded to bf16 (round to nearest even);
// everything else -- the z term W0[KF:]^T z, scale / shift, a2, the head and the soft-max -- is fp32.  The PHX_F32 form is an fp32
// FMA chain throughout.
#include "phx_common.h"

#define RC_K 32
#define RC_CHUNK_MAX 16       // samples per block (the z-term table of a block lives in LDS)

__device__ __forceinline__ int rc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// relu(s * x + t) of one accumulator tile; s, t: LDS vectors indexed by channel (row)
__device__ __forceinline__ void rc_affine_relu(f32x16& x, const float* s, const float* t, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 sv = *(const f32x4*)(s + 8 * g + 4 * h);
        const f32x4 tv = *(const f32x4*)(t + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[4 * g + i] = fmaxf(fmaf(sv[i], x[4 * g + i], tv[i]), 0.f);
    }
}

// registers 8s .. 8s + 7 of an accumulator tile -> the bf16 fragment of k-step s
__device__ __forceinline__ bf16x8 rc_pack(const f32x16& x, int s) {
    unsigned u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = f2bf_pk(x[8 * s + 2 * i], x[8 * s + 2 * i + 1]);
    return __builtin_bit_cast(bf16x8, u);
}

// A fragment (rows = output channels) of k-step s of the fp32 HWIO 1x1 filter w [k][32]; perm: the accumulator's k order
__device__ __forceinline__ bf16x8 rc_wfrag(const float* __restrict__ w, int s, int r, int h, bool perm) {
    unsigned u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = 2 * i;
        const int k0 = perm ? 16 * s + 8 * (j >> 2) + 4 * h + (j & 3) : 16 * s + 8 * h + j;
        u[i] = f2bf_pk(w[(size_t)k0 * RC_K + r], w[(size_t)(k0 + 1) * RC_K + r]);       // (j even: j + 1 is the next k in both orders)
    }
    return __builtin_bit_cast(bf16x8, u);
}

struct RcArgs {
    const void* feat;
    const float *z, *W0, *W1, *W2, *W3, *b3;
    const float *s[3], *t[3];
    float *logits, *sm;
    int B, n, P, KF, Z, chunk;      // KF: channels of feat (the hidden width of the chain is RC_K)
};

// shared by both forms: scale / shift vectors (scale 1 where the pointer is NULL), the head filter padded to 8 outputs, its bias
template <int C>
__device__ __forceinline__ void rc_stage_small(const RcArgs& a, float (*st)[RC_K], float (*w3)[8], float* b3, int tid, int nthr) {
    for (int i = tid; i < 6 * RC_K; i += nthr) {
        const int l = i / (2 * RC_K), which = (i / RC_K) & 1, c = i % RC_K;
        st[2 * l + which][c] = which ? a.t[l][c] : (a.s[l] ? a.s[l][c] : 1.f);
    }
    for (int i = tid; i < RC_K * 8; i += nthr) w3[i >> 3][i & 7] = (i & 7) < C ? a.W3[(i >> 3) * C + (i & 7)] : 0.f;
    if (tid < 8) b3[tid] = tid < C ? a.b3[tid] : 0.f;
}

template <int C>
__device__ __forceinline__ void rc_softmax(float (&v)[C]) {
    float m = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - m); sum += v[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] *= inv;
}

// grid (pixel tiles / 4, sample chunks, B), 256 threads: a wave owns one 32-pixel tile and walks the block's samples
template <int C, int KS>         // KS = KF / 16: k-steps of the feature half of layer 0
__global__ __launch_bounds__(256) void k_recomb_bf16(RcArgs a) {
    __shared__ __attribute__((aligned(16))) float s_st[6][RC_K];
    __shared__ __attribute__((aligned(16))) float s_w3[RC_K][8];
    __shared__ float s_b3[8];
    __shared__ __attribute__((aligned(16))) float s_v[RC_CHUNK_MAX][RC_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, k0 = blockIdx.y * a.chunk;
    const int nk = min(a.chunk, a.n - k0);
    rc_stage_small<C>(a, s_st, s_w3, s_b3, tid, 256);
    // the sample-dependent half of layer 0: v[k][cout] = sum_zi W0[KF + zi][cout] z[b n + k][zi], fp32 from the fp32 filter rows
    for (int i = tid; i < nk * RC_K; i += 256) {
        const int kk = i >> 5, co = i & 31;
        const float* zr = a.z + (size_t)((size_t)b * a.n + k0 + kk) * a.Z;
        float v = 0.f;
        for (int zi = 0; zi < a.Z; ++zi) v = fmaf(zr[zi], a.W0[(size_t)(a.KF + zi) * RC_K + co], v);
        s_v[kk][co] = v;
    }
    __syncthreads();
    const int tile = blockIdx.x * 4 + wave;
    if ((size_t)tile * 32 >= (size_t)a.P) return;           // (wave-uniform; no barrier below)
    const int p = tile * 32 + r;
    const bool valid = p < a.P;
    bf16x8 w1[2], w2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        w1[s] = rc_wfrag(a.W1, s, r, h, true);
        w2[s] = rc_wfrag(a.W2, s, r, h, true);
    }
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // the sample-independent half of layer 0, once per tile: F = W0[:KF]^T feat (both operands from memory, natural k order)
    f32x16 F = zero;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        uint4 q = {0u, 0u, 0u, 0u};
        if (valid) q = *(const uint4*)((const bf16_t*)a.feat + ((size_t)b * a.P + p) * (16 * KS) + 16 * s + 8 * h);
        F = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rc_wfrag(a.W0, s, r, h, false), __builtin_bit_cast(bf16x8, q), F, 0, 0, 0);
    }
    for (int kk = 0; kk < nk; ++kk) {
        f32x16 x;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 vv = *(const f32x4*)(&s_v[kk][8 * g + 4 * h]);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * g + i] = F[4 * g + i] + vv[i];
        }
        rc_affine_relu(x, s_st[0], s_st[1], h);
        f32x16 y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1[0], rc_pack(x, 0), zero, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1[1], rc_pack(x, 1), y, 0, 0, 0);
        rc_affine_relu(y, s_st[2], s_st[3], h);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2[0], rc_pack(y, 0), zero, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2[1], rc_pack(y, 1), x, 0, 0, 0);
        rc_affine_relu(x, s_st[4], s_st[5], h);
        // head: this lane holds 16 of its pixel's 32 channels, the other lane half the rest
        float lg[C];
#pragma unroll
        for (int c = 0; c < C; ++c) lg[c] = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float* wr = s_w3[rc_row(reg, h)];
#pragma unroll
            for (int c = 0; c < C; ++c) lg[c] = fmaf(x[reg], wr[c], lg[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) lg[c] = lg[c] + __shfl_xor(lg[c], 32, 64) + s_b3[c];
        if (valid) {
            const size_t o = (((size_t)b * a.n + k0 + kk) * a.P + p) * C;
            if (h == 0) {                                   // lower lane half: logits; upper: soft-max
                if (a.logits) {
#pragma unroll
                    for (int c = 0; c < C; ++c) a.logits[o + c] = lg[c];
                }
            } else if (a.sm) {
                rc_softmax<C>(lg);
#pragma unroll
                for (int c = 0; c < C; ++c) a.sm[o + c] = lg[c];
            }
        }
    }
}

// one KIN -> 32 layer of the fp32 form: v[:32] = relu(s * (w^T v[:KIN] [+ extra]) + t), w [KIN][32] in LDS
template <int KIN, int KV>
__device__ __forceinline__ void rc_layer_f32(float (&v)[KV], const float* w, const float* extra, const float* s, const float* t) {
    float acc[RC_K];
#pragma unroll
    for (int c = 0; c < RC_K; ++c) acc[c] = 0.f;
#pragma unroll
    for (int k = 0; k < KIN; ++k) {
#pragma unroll
        for (int c = 0; c < RC_K; ++c) acc[c] = fmaf(v[k], w[k * RC_K + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < RC_K; ++c) v[c] = fmaxf(fmaf(s[c], extra ? acc[c] + extra[c] : acc[c], t[c]), 0.f);
}

// the parity form: one thread per (sample row, pixel), filters in LDS
template <int C, int KF>
__global__ __launch_bounds__(128) void k_recomb_f32(RcArgs a, size_t total) {
    __shared__ __attribute__((aligned(16))) float s_w0[(KF + 32) * RC_K];
    __shared__ __attribute__((aligned(16))) float s_w1[RC_K * RC_K];
    __shared__ __attribute__((aligned(16))) float s_w2[RC_K * RC_K];
    __shared__ __attribute__((aligned(16))) float s_st[6][RC_K];
    __shared__ __attribute__((aligned(16))) float s_w3[RC_K][8];
    __shared__ float s_b3[8];
    const int tid = threadIdx.x;
    for (int i = tid; i < (KF + a.Z) * RC_K; i += 128) s_w0[i] = a.W0[i];
    for (int i = tid; i < RC_K * RC_K; i += 128) { s_w1[i] = a.W1[i]; s_w2[i] = a.W2[i]; }
    rc_stage_small<C>(a, s_st, s_w3, s_b3, tid, 128);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * 128 + tid;
    if (idx >= total) return;
    const size_t row = idx / (size_t)a.P, p = idx % (size_t)a.P, b = row / (size_t)a.n;
    float v[KF], zt[RC_K];
    const f32x4* fp = (const f32x4*)((const float*)a.feat + (b * a.P + p) * KF);
#pragma unroll
    for (int q = 0; q < KF / 4; ++q) {
        const f32x4 f = fp[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * q + i] = f[i];
    }
#pragma unroll
    for (int c = 0; c < RC_K; ++c) zt[c] = 0.f;
    for (int zi = 0; zi < a.Z; ++zi) {
        const float zv = a.z[row * a.Z + zi];
#pragma unroll
        for (int c = 0; c < RC_K; ++c) zt[c] = fmaf(zv, s_w0[(KF + zi) * RC_K + c], zt[c]);
    }
    rc_layer_f32<KF>(v, s_w0, zt, s_st[0], s_st[1]);
    rc_layer_f32<RC_K>(v, s_w1, nullptr, s_st[2], s_st[3]);
    rc_layer_f32<RC_K>(v, s_w2, nullptr, s_st[4], s_st[5]);
    float lg[C];
#pragma unroll
    for (int c = 0; c < C; ++c) lg[c] = 0.f;
#pragma unroll
    for (int k = 0; k < RC_K; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) lg[c] = fmaf(v[k], s_w3[k][c], lg[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) lg[c] += s_b3[c];
    const size_t o = idx * C;
    if (a.logits) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.logits[o + c] = lg[c];
    }
    if (a.sm) {
        rc_softmax<C>(lg);
#pragma unroll
        for (int c = 0; c < C; ++c) a.sm[o + c] = lg[c];
    }
}

#define RC_C_SWITCH(c, Cv, ...)                                \
    do {                                                       \
        switch (c) {                                           \
            case 2: { constexpr int Cv = 2; __VA_ARGS__; } break; \
            case 3: { constexpr int Cv = 3; __VA_ARGS__; } break; \
            case 4: { constexpr int Cv = 4; __VA_ARGS__; } break; \
            case 5: { constexpr int Cv = 5; __VA_ARGS__; } break; \
            case 6: { constexpr int Cv = 6; __VA_ARGS__; } break; \
            case 7: { constexpr int Cv = 7; __VA_ARGS__; } break; \
            default: { constexpr int Cv = 8; __VA_ARGS__; } break; \
        }                                                      \
    } while (0)

int phx_recomb_samples(const void* feat, int feat_dt, const float* z, const float* W0, const float* W1, const float* W2,
                       const float* W3, const float* b3, const float* s0, const float* t0, const float* s1, const float* t1,
                       const float* s2, const float* t2, float* logits, float* sm, int B, int n, int P, int KF, int K, int Z, int C,
                       void* stream) {
    PHX_REQUIRE(K == RC_K, PHX_E_SHAPE, "recomb_samples: K = 32");
    PHX_REQUIRE(KF == 32 || KF == 64, PHX_E_SHAPE, "recomb_samples: KF = 32 or 64");
    PHX_REQUIRE(Z >= 1 && Z <= 32, PHX_E_SHAPE, "recomb_samples: 1 <= Z <= 32");
    PHX_REQUIRE(C >= 2 && C <= 8, PHX_E_SHAPE, "recomb_samples: 2 <= C <= 8");
    PHX_REQUIRE(B >= 1 && n >= 1 && P >= 1 && B <= 65535, PHX_E_SHAPE, "recomb_samples: 1 <= B <= 65535, n >= 1, P >= 1");
    PHX_REQUIRE(feat_dt == PHX_F32 || feat_dt == PHX_BF16, PHX_E_INVAL, "recomb_samples: feat is PHX_F32 or PHX_BF16");
    PHX_REQUIRE(feat && z && W0 && W1 && W2 && W3 && b3 && t0 && t1 && t2, PHX_E_INVAL, "recomb_samples: null input");
    PHX_REQUIRE(logits || sm, PHX_E_INVAL, "recomb_samples: logits and sm are both NULL");
    PHX_REQUIRE(((uintptr_t)feat & 15) == 0, PHX_E_ALIGN, "recomb_samples: feat must be 16-byte aligned");
    RcArgs a;
    a.feat = feat; a.z = z; a.W0 = W0; a.W1 = W1; a.W2 = W2; a.W3 = W3; a.b3 = b3;
    a.s[0] = s0; a.s[1] = s1; a.s[2] = s2; a.t[0] = t0; a.t[1] = t1; a.t[2] = t2;
    a.logits = logits; a.sm = sm; a.B = B; a.n = n; a.P = P; a.KF = KF; a.Z = Z; a.chunk = 1;
    if (feat_dt == PHX_F32) {
        const size_t total = (size_t)B * n * P;
        const size_t blocks = (total + 127) / 128;
        PHX_REQUIRE(blocks <= 0x7fffffffu, PHX_E_SHAPE, "recomb_samples: B n P too large");
        if (KF == 32) RC_C_SWITCH(C, Cv, hipLaunchKernelGGL((k_recomb_f32<Cv, 32>), dim3((unsigned)blocks), dim3(128), 0, (hipStream_t)stream, a, total));
        else RC_C_SWITCH(C, Cv, hipLaunchKernelGGL((k_recomb_f32<Cv, 64>), dim3((unsigned)blocks), dim3(128), 0, (hipStream_t)stream, a, total));
    } else {
        // samples are spread over blocks as well as pixels: about a thousand blocks (four per CU) where n allows, at most RC_CHUNK_MAX
        // samples per block
        const size_t tiles = ((size_t)P + 31) / 32, tblocks = (tiles + 3) / 4;
        PHX_REQUIRE(tblocks <= 0x7fffffffu, PHX_E_SHAPE, "recomb_samples: P too large");
        size_t want = (1024 + tblocks * B - 1) / (tblocks * B);
        if (want < 1) want = 1;
        if (want > (size_t)n) want = n;
        int chunk = (int)(((size_t)n + want - 1) / want);
        if (chunk > RC_CHUNK_MAX) chunk = RC_CHUNK_MAX;
        const int nchunks = (n + chunk - 1) / chunk;
        PHX_REQUIRE(nchunks <= 65535, PHX_E_SHAPE, "recomb_samples: n too large");
        a.chunk = chunk;
        if (KF == 32) RC_C_SWITCH(C, Cv, hipLaunchKernelGGL((k_recomb_bf16<Cv, 2>), dim3((unsigned)tblocks, nchunks, B), dim3(256), 0, (hipStream_t)stream, a));
        else RC_C_SWITCH(C, Cv, hipLaunchKernelGGL((k_recomb_bf16<Cv, 4>), dim3((unsigned)tblocks, nchunks, B), dim3(256), 0, (hipStream_t)stream, a));
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
