// Normalisation forward (batch / group / instance), streaming form: statistics pass, partial reductions, finalisation, inference
// scale / shift, affine + activation, and the fused apply passes (plain, with a 1x1 head, depth-to-space, with the 2 x 2 average pool).
// The backward passes: norm_bwd.hip; the one-launch layers of the small maps: norm_onelaunch.hip.
#include <stdlib.h>
#include <type_traits>

#include "norm_common.h"

// =================================================================================================
// normalisation statistics: sums[ns][c][2] += {sum x, sum x^2} over the P pixels of sample-group ns
template <typename T, int V>
__global__ void k_norm_stats(const T* __restrict__ x, float* __restrict__ sums, float* __restrict__ pivot, int P,
                             int C, int PL, int chunk) {
    const int CV = C / V;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    extern __shared__ float red[];   // [PL][C][2]
    float s1[V], s2[V], pv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = pv[j] = 0.f;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    if (pl < PL) {
        if (pivot) {      // shifted sums: pivot = first pixel of the sample-group -> no catastrophic cancellation
            VecIO<T, V>::load(x, ((size_t)ns * P) * C + (size_t)cv * V, pv);
            if (blockIdx.x == 0 && pl == 0) {
#pragma unroll
                for (int j = 0; j < V; ++j) pivot[(size_t)ns * C + cv * V + j] = pv[j];
            }
        }
        // four pixels per trip, loads first: a thread's trips are serially dependent, so the loads in flight per
        // thread -- not the block count -- set the speed on the mid-size maps
        int p = p0 + pl;
        for (; p + 3 * PL < p1; p += 4 * PL) {
            float v[4][V];
#pragma unroll
            for (int u = 0; u < 4; ++u) VecIO<T, V>::load(x, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) { const float d = v[u][j] - pv[j]; s1[j] += d; s2[j] += d * d; }
        }
        for (; p < p1; p += PL) {
            float v[V];
            VecIO<T, V>::load(x, ((size_t)ns * P + p) * C + (size_t)cv * V, v);
#pragma unroll
            for (int j = 0; j < V; ++j) { const float d = v[j] - pv[j]; s1[j] += d; s2[j] += d * d; }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            red[(pl * C + cv * V + j) * 2 + 0] = s1[j];
            red[(pl * C + cv * V + j) * 2 + 1] = s2[j];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
        float a = 0.f;
        for (int q = 0; q < PL; ++q) a += red[q * 2 * C + i];
        atomicAdd(&sums[(size_t)ns * 2 * C + i], a);
    }
}

// partial[T][2][C] -> sums[c][2]
__global__ void k_reduce_partials(const float* __restrict__ partial, int T, int C, float* __restrict__ sums) {
    const int i = blockIdx.x;                 // 0 .. 2C-1 : (which, c)
    const int which = i / C, c = i % C;
    // (four independent chains: the plain loop compiled to load / wait / add per tile, 16 serial round trips at 4 096 tiles)
    const float* p = partial + (size_t)which * C + c;
    const int st = blockDim.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int t = threadIdx.x;
    for (; t + 3 * st < T; t += 4 * st) {
        a0 += p[(size_t)t * 2 * C];
        a1 += p[(size_t)(t + st) * 2 * C];
        a2 += p[(size_t)(t + 2 * st) * 2 * C];
        a3 += p[(size_t)(t + 3 * st) * 2 * C];
    }
    for (; t < T; t += st) a0 += p[(size_t)t * 2 * C];
    float a = (a0 + a1) + (a2 + a3);
    __shared__ float sh[4];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) sums[c * 2 + which] = sh[0] + sh[1] + sh[2] + sh[3];
}

// per-sample form (group / instance norm): partial[ns * T + t][2][C] -> sums[ns][c][2], T pixel tiles per sample; a thread owns one
// (which, c) entry of one sample and walks its T tiles (coalesced across the block)
__global__ void k_reduce_partials_ns(const float* __restrict__ partial, int T, int C, float* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, ns = blockIdx.y;
    if (i >= 2 * C) return;
    const float* p = partial + (size_t)ns * T * 2 * C + i;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;             // four independent chains: the T loads of a thread overlap
    int t = 0;
    for (; t + 3 < T; t += 4) {
        a0 += p[(size_t)t * 2 * C];
        a1 += p[(size_t)(t + 1) * 2 * C];
        a2 += p[(size_t)(t + 2) * 2 * C];
        a3 += p[(size_t)(t + 3) * 2 * C];
    }
    for (; t < T; ++t) a0 += p[(size_t)t * 2 * C];
    const int which = i / C, c = i % C;
    sums[((size_t)ns * C + c) * 2 + which] = (a0 + a1) + (a2 + a3);
}

// per (ns, g): mean / rstd; per (ns, c): scale / shift; optional TF1 fused-batch-norm moving update
__global__ void k_norm_finalize(const float* __restrict__ sums, const float* __restrict__ pivot,
                                const float* __restrict__ gamma,
                                const float* __restrict__ beta, float eps, int NS, int P, int C, int G,
                                float* mean, float* rstd, float* scale, float* shift, float* moving_mean,
                                float* moving_var, float momentum) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= NS * G) return;
    const int ns = idx / G, g = idx % G, cg = C / G;
    // per-channel mean / variance from the (pivot-shifted) sums, then the stable parallel-variance combination
    // over the channels of the group: var_g = mean_c[var_c + (mu_c - mu_g)^2]
    const float invP = 1.f / (float)P;
    if (cg == 1) {                            // batch / instance norm: the fused apply kernels' arithmetic, bit for bit (chan_coeffs)
        float mu1, var1, rs1, sc1, sh1;
        chan_coeffs(sums[((size_t)ns * C + g) * 2], sums[((size_t)ns * C + g) * 2 + 1], pivot ? pivot[(size_t)ns * C + g] : 0.f, invP, eps,
                    &mu1, &var1, &rs1);
        chan_scale_shift(gamma[g], beta[g], mu1, rs1, &sc1, &sh1);
        mean[idx] = mu1;
        rstd[idx] = rs1;
        scale[(size_t)ns * C + g] = sc1;
        shift[(size_t)ns * C + g] = sh1;
        if (momentum > 0.f && moving_mean) moving_update(&moving_mean[g], &moving_var[g], mu1, var1, (float)P, momentum);
        return;
    }
    float mu = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
        const float pv = pivot ? pivot[(size_t)ns * C + c] : 0.f;
        mu += pv + sums[((size_t)ns * C + c) * 2] * invP;
    }
    mu /= (float)cg;
    float var = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
        const float pv = pivot ? pivot[(size_t)ns * C + c] : 0.f;
        const float d1 = sums[((size_t)ns * C + c) * 2] * invP;
        float vc = sums[((size_t)ns * C + c) * 2 + 1] * invP - d1 * d1;
        vc = vc > 0.f ? vc : 0.f;
        const float dm = pv + d1 - mu;
        var += vc + dm * dm;
    }
    var /= (float)cg;
    const float m = (float)P * (float)cg;
    const float rs = rsqrtf(var + eps);
    mean[idx] = mu;
    rstd[idx] = rs;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
        const float sc = gamma[c] * rs;
        scale[(size_t)ns * C + c] = sc;
        shift[(size_t)ns * C + c] = beta[c] - mu * sc;
    }
    if (momentum > 0.f && moving_mean) {      // batch norm only (NS == 1, G == C): tf.contrib.layers.batch_norm
        const float unbiased = var * (m / fmaxf(m - 1.f, 1.f));
        moving_mean[g] -= (moving_mean[g] - mu) * momentum;
        moving_var[g] -= (moving_var[g] - unbiased) * momentum;
    }
}

__global__ void k_bn_infer_scale_shift(const float* gamma, const float* beta, const float* mm, const float* mv,
                                       float eps, int C, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] * rsqrtf(mv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - mm[c] * sc;
}

struct BnInferDesc {
    const float *gamma, *beta, *mm, *mv;
    float *scale, *shift;
    int C;
    float eps;
};
__global__ void k_bn_infer_scale_shift_multi(const BnInferDesc* __restrict__ descs) {
    const BnInferDesc d = descs[blockIdx.y];
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < d.C; c += gridDim.x * blockDim.x) {
        const float sc = d.gamma[c] * rsqrtf(d.mv[c] + d.eps);
        d.scale[c] = sc;
        d.shift[c] = d.beta[c] - d.mm[c] * sc;
    }
}

// y = act(x*scale[ns][c] + shift[ns][c]).  A thread owns one channel vector (cv) and walks over pixels, so the
// per-channel coefficients live in registers; blockDim = CV * PL (as for the statistics kernels).
template <typename TI, typename TO, int V>
__global__ void k_affine_act(const TI* __restrict__ x, const float* __restrict__ scale,
                             const float* __restrict__ shift, TO* __restrict__ y, int P, int C, int PL, int chunk,
                             int act) {
    const int CV = C / V;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    if (pl >= PL) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sc[j] = scale[(size_t)ns * C + cv * V + j];
        sh[j] = shift[(size_t)ns * C + cv * V + j];
    }
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    int p = p0 + pl;
    for (; p + 3 * PL < p1; p += 4 * PL) {       // four pixels per trip, loads first (see k_norm_stats)
        float v[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) VecIO<TI, V>::load(x, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = act_fwd(fmaf(v[u][j], sc[j], sh[j]), act);
            VecIO<TO, V>::store(y, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, v[u]);
        }
    }
    for (; p < p1; p += PL) {
        const size_t off = ((size_t)ns * P + p) * C + (size_t)cv * V;
        float v[V];
        VecIO<TI, V>::load(x, off, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = act_fwd(fmaf(v[j], sc[j], sh[j]), act);
        VecIO<TO, V>::store(y, off, v);
    }
}

// ---- fused variants: the per-(ns, g) finalisation is recomputed by every thread for its own channels (a handful of
// loads), so the two tiny "finalize" launches per layer disappear; block (0, ns) publishes the statistics.
// HN > 0: a 1x1 head with HN outputs reads a = act(norm(x)) and nothing else does (the likelihood's top layer feeding y_lvl0,
// likelihoods.py:220): its forward is computed here from the values just produced -- yh[p][o] = bh[o] + sum_c a[p][c] wh[c][o], the
// sum over the channel vectors of a pixel by lane shuffles (C / V a power of two <= 64) -- instead of by a pass of its own over a.
struct HeadFw {
    const float *w, *b;
    float* y;
    int ph, pw;          // > 0: x is in the packed pixel order of the phase-form convolution (csrc/upconv.hip: [B][ph][pw][(a, b)] pixels), y is
                         // written as the hi-res map [B][2 ph][2 pw] -- the depth-to-space permutation rides on the apply pass
};
// The statistics of sample group blockIdx.y finalised ONCE per block, cooperatively, into LDS: gst[G][2] = mean, rstd, cof[C][2] = scale,
// shift; block (0, ns) publishes them and does the moving update.  (Every thread deriving the eight channels it streams -- 30-50 loads
// of the same few cache lines per thread -- made the prologue 4-5 us per block and a launch with many blocks a hot spot in one L2
// channel: these kernels ran at 2.4-4.7 TB/s where a plain copy of the same tensor reaches 6-7.)
// In two parts, so that a kernel can put its first data loads between them: norm_apply_loads issues what this thread's first channel
// needs (sums, pivot, gamma, beta -- loads return in issue order, so issued first they are waited for alone; a thread past C loads
// channel C - 1 and discards it: no branch), norm_apply_prologue derives the coefficients and ends with the block's barrier.
struct NormChanLoads {
    float2 sq;           // {sum, sum of squares} (pivot-shifted), replica 0
    float pv, gm, bt;
};
__device__ __forceinline__ NormChanLoads norm_apply_loads(const float* __restrict__ sums, const float* __restrict__ pivot,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int C, int c) {
    NormChanLoads k;
    const size_t nc = (size_t)blockIdx.y * C + c;
    k.sq = *reinterpret_cast<const float2*>(sums + nc * 2);
    k.pv = pivot ? pivot[nc] : 0.f;
    k.gm = gamma[c];
    k.bt = beta[c];
    return k;
}
__device__ __forceinline__ void norm_apply_prologue(const NormChanLoads& k0, const float* __restrict__ sums, const float* __restrict__ pivot,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                    float* mean_out, float* rstd_out, float* scale_out, float* shift_out,
                                                    float* moving_mean, float* moving_var, float momentum, int P, int C, int G, int nrep,
                                                    float* gst, float* cof) {
    const int cg = C / G, ns = blockIdx.y;
    const float invP = 1.f / (float)P;
    const bool pub = blockIdx.x == 0;
    if (cg == 1) {
        // batch / instance norm, one channel per statistic: thread c has issued everything channel c needs together and derives
        // mean / rstd / scale / shift on its own -- one memory round trip and one barrier
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const size_t nc = (size_t)ns * C + c;
            NormChanLoads k = k0;
            if (c != (int)threadIdx.x) k = norm_apply_loads(sums, pivot, gamma, beta, C, c);      // (C > 256 only)
            float2 sq = k.sq;
            for (int r = 1; r < nrep; ++r) {                    // (replicated accumulators: nrep is 1 on every shipped path)
                const float2 q = *reinterpret_cast<const float2*>(sums + (((size_t)r * gridDim.y + ns) * C + c) * 2);
                sq.x += q.x; sq.y += q.y;
            }
            float mu, var, rs1, scv, shv;
            chan_coeffs(sq.x, sq.y, k.pv, invP, eps, &mu, &var, &rs1);
            const float rs = rsqrtf(var + eps);
            chan_scale_shift(k.gm, k.bt, mu, rs, &scv, &shv);
            cof[2 * c] = scv;
            cof[2 * c + 1] = shv;
            if (pub) {
                mean_out[nc] = mu;
                rstd_out[nc] = rs;
                if (momentum > 0.f && moving_mean)            // batch norm (G == C): TF1 fused-batch-norm moving update
                    moving_update(&moving_mean[c], &moving_var[c], mu, var, (float)P * (float)cg, momentum);
                scale_out[nc] = scv;
                shift_out[nc] = shv;
            }
        }
        __syncthreads();
        return;
    }
    // group norm: thread g derives (mean, rstd) of statistic g, thread c the (scale, shift) of channel c (its first channel's gamma /
    // beta are there already)
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float mu, var;
        group_stats(sums, pivot, ns, C, g, cg, invP, eps, &mu, &var);
        const float rs = rsqrtf(var + eps);
        gst[2 * g] = mu;
        gst[2 * g + 1] = rs;
        if (pub) {
            mean_out[ns * G + g] = mu;
            rstd_out[ns * G + g] = rs;
            if (momentum > 0.f && moving_mean) moving_update(&moving_mean[g], &moving_var[g], mu, var, (float)P * (float)cg, momentum);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const int g = c / cg;
        const bool first = c == (int)threadIdx.x;
        float scv, shv;
        chan_scale_shift(first ? k0.gm : gamma[c], first ? k0.bt : beta[c], gst[2 * g], gst[2 * g + 1], &scv, &shv);
        cof[2 * c] = scv;
        cof[2 * c + 1] = shv;
        if (pub) {
            scale_out[(size_t)ns * C + c] = scv;
            shift_out[(size_t)ns * C + c] = shv;
        }
    }
    __syncthreads();
}

template <typename TI, typename TO, int V, int HN = 0>
__global__ void k_norm_apply_fused(const TI* __restrict__ x, const float* __restrict__ sums,
                                   const float* __restrict__ pivot, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float eps, TO* __restrict__ y, float* mean_out,
                                   float* rstd_out, float* scale_out, float* shift_out, float* moving_mean,
                                   float* moving_var, float momentum, int P, int C, int G, int PL, int chunk, int act, int nrep,
                                   HeadFw hd) {
    const int CV = C / V;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    extern __shared__ float lds_f[];
    float* gst = lds_f;                          // [G][2]  mean, rstd
    float* cof = lds_f + 2 * G;                  // [C][2]  scale, shift
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    // EARLY (bf16 input, 16-byte vectors): the first trip's loads are issued ahead of the finalisation and held packed until the
    // coefficients are there -- the streamed data depend on nothing, and a block's first loads miss L2 (the producer ran on another
    // XCD), so behind the prologue they were a round trip of their own.  Pixels past the block's range are clamped to its last pixel
    // (a valid address: no block has an empty range, see the launcher) and their values discarded.
    constexpr bool EARLY = V == 8 && std::is_same<TI, bf16_t>::value;
    const NormChanLoads k0 = norm_apply_loads(sums, pivot, gamma, beta, C, min((int)threadIdx.x, C - 1));
    uint4 xe[EARLY ? 4 : 1];
    if constexpr (EARLY) {                       // (no branch around the loads: a merge would wait for them)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            xe[u] = *reinterpret_cast<const uint4*>(x + ((size_t)ns * P + min(p0 + pl + u * PL, p1 - 1)) * C + (size_t)cv * V);
    }
    float hw[V][HN > 0 ? HN : 1];
    if constexpr (HN > 0) {                      // (the head's filter rows: independent loads, out with the first trip's)
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int o = 0; o < HN; ++o) hw[j][o] = hd.w[(size_t)(cv * V + j) * HN + o];
    }
    norm_apply_prologue(k0, sums, pivot, gamma, beta, eps, mean_out, rstd_out, scale_out, shift_out, moving_mean, moving_var, momentum, P, C,
                        G, nrep, gst, cof);
    if (pl >= PL) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sc[j] = cof[2 * (cv * V + j)];
        sh[j] = cof[2 * (cv * V + j) + 1];
    }
    auto head = [&](size_t pix, const float (&a)[V]) {     // (all CV lanes of the pixel are active together)
        if constexpr (HN > 0) {
            float part[HN];
#pragma unroll
            for (int o = 0; o < HN; ++o) part[o] = 0.f;
#pragma unroll
            for (int j = 0; j < V; j += 2) {                   // the head reads a as it is stored (bf16)
                const unsigned w2 = f2bf_pk(a[j], a[j + 1]);
                const float a0 = __uint_as_float(w2 << 16), a1 = __uint_as_float(w2 & 0xffff0000u);
#pragma unroll
                for (int o = 0; o < HN; ++o) part[o] = fmaf(a1, hw[j + 1][o], fmaf(a0, hw[j][o], part[o]));
            }
            for (int m = 1; m < CV; m <<= 1)
#pragma unroll
                for (int o = 0; o < HN; ++o) part[o] += __shfl_xor(part[o], m, 64);
            if (cv == 0)
#pragma unroll
                for (int o = 0; o < HN; ++o) hd.y[pix * HN + o] = part[o] + hd.b[o];
        }
    };
    auto yoff = [&](size_t pix) -> size_t { return (hd.pw > 0 ? packed_to_hi_pixel(pix, hd.ph, hd.pw) : pix) * C + (size_t)cv * V; };
    int p = p0 + pl;
    if constexpr (EARLY) {                       // the first four pixels: loaded ahead of the prologue
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u * PL < p1) {
                float v[V];
                bf16x8_unpack(xe[u], v);
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = act_fwd(fmaf(v[j], sc[j], sh[j]), act);
                if (HN == 0 || y != nullptr) VecIO<TO, V>::store(y, yoff((size_t)ns * P + p + u * PL), v);
                head((size_t)ns * P + p + u * PL, v);
            }
        }
        p += 4 * PL;
    }
    for (; p + 3 * PL < p1; p += 4 * PL) {       // four pixels per trip, loads first (see k_norm_stats)
        float v[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) VecIO<TI, V>::load(x, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = act_fwd(fmaf(v[u][j], sc[j], sh[j]), act);
            // (HN > 0, y == NULL: a is not written at all -- in a training plan its only other reader, the head's filter gradient,
            // re-forms it from x: 268 MB less to write for the likelihood's top layer)
            if (HN == 0 || y != nullptr) VecIO<TO, V>::store(y, yoff((size_t)ns * P + p + u * PL), v[u]);
            head((size_t)ns * P + p + u * PL, v[u]);
        }
    }
    for (; p < p1; p += PL) {
        const size_t off = ((size_t)ns * P + p) * C + (size_t)cv * V;
        float v[V];
        VecIO<TI, V>::load(x, off, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = act_fwd(fmaf(v[j], sc[j], sh[j]), act);
        if (HN == 0 || y != nullptr) VecIO<TO, V>::store(y, yoff((size_t)ns * P + p), v);
        head((size_t)ns * P + p, v);
    }
}

// The apply pass of a layer whose output also feeds a 2 x 2 average pool (round 5; posteriors.py:80-82, priors.py:76-78: averagepool2D
// of pre_z[i - 1] in front of every encoder level): a thread takes a 2 x 2 pixel quad -- four loads, four stores of a = act(norm(x)) and
// ONE store of their average -- so the pooled tensor costs no pass of its own over a (tfwrapper/layers.py:44-54, tf.nn.avg_pool 2x2
// stride 2; H and W even).  The average is taken of the values AS STORED (bf16), in k_avgpool_fwd's order: bit-identical to the two
// launches.  bf16 in / out, 16-byte channel vectors; statistics finalised once per block as in k_norm_apply_fused.
__global__ void k_norm_apply_pool(const bf16_t* __restrict__ x, const float* __restrict__ sums, const float* __restrict__ pivot,
                                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, bf16_t* __restrict__ y,
                                  bf16_t* __restrict__ ypool, float* mean_out, float* rstd_out, float* scale_out, float* shift_out,
                                  float* moving_mean, float* moving_var, float momentum, int P, int C, int G, int H, int W, int PL,
                                  int chunk, int act) {
    constexpr int V = 8;
    const int CV = C / V;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    extern __shared__ float lds_f[];
    float* gst = lds_f;                          // [G][2]  mean, rstd
    float* cof = lds_f + 2 * G;                  // [C][2]  scale, shift
    const int Hh = H >> 1, Wh = W >> 1, Q = P >> 2;               // quads of this sample group (P = images x H x W)
    const int q0 = blockIdx.x * chunk, q1 = min(Q, q0 + chunk);
    auto quad_pixels = [&](int q, size_t (&off)[4]) {             // k_avgpool_fwd's order: (0,0), (0,1), (1,0), (1,1)
        const int bl = q / (Hh * Wh), r = q - bl * (Hh * Wh);
        const int yq = r / Wh, xq = r - yq * Wh;
        const size_t p00 = (size_t)ns * P + ((size_t)bl * H + 2 * yq) * W + 2 * xq;
        off[0] = p00; off[1] = p00 + 1; off[2] = p00 + W; off[3] = p00 + W + 1;
    };
    // (the first quad's loads stay behind the finalisation here: held packed across it they cost the kernel a wave per SIMD -- 74
    // registers against 72 -- and these kernels lose more from occupancy than from a round trip)
    const NormChanLoads k0 = norm_apply_loads(sums, pivot, gamma, beta, C, min((int)threadIdx.x, C - 1));
    norm_apply_prologue(k0, sums, pivot, gamma, beta, eps, mean_out, rstd_out, scale_out, shift_out, moving_mean, moving_var, momentum, P, C,
                        G, 1, gst, cof);
    if (pl >= PL) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sc[j] = cof[2 * (cv * V + j)];
        sh[j] = cof[2 * (cv * V + j) + 1];
    }
    for (int q = q0 + pl; q < q1; q += PL) {
        size_t off[4];
        quad_pixels(q, off);
        float v[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) VecIO<bf16_t, V>::load(x, off[u] * C + (size_t)cv * V, v[u]);
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < V; j += 2) {
                const float a0 = act_fwd(fmaf(v[u][j], sc[j], sh[j]), act), a1 = act_fwd(fmaf(v[u][j + 1], sc[j + 1], sh[j + 1]), act);
                w[j >> 1] = f2bf_pk(a0, a1);
                acc[j] += __uint_as_float(w[j >> 1] << 16);                      // the values as stored
                acc[j + 1] += __uint_as_float(w[j >> 1] & 0xffff0000u);
            }
            *reinterpret_cast<uint4*>(y + off[u] * C + (size_t)cv * V) = make_uint4(w[0], w[1], w[2], w[3]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] *= 0.25f;
        const size_t po = (size_t)ns * Q + q;
        VecIO<bf16_t, V>::store(ypool, po * C + (size_t)cv * V, acc);
    }
}

extern "C" {

int phx_norm_stats(const void* x, int dt, float* sums, float* pivot, int NS, int P, int C, void* stream) {
    PHX_REQUIRE(NS > 0 && P > 0 && C > 0, PHX_E_SHAPE, "norm_stats: bad shape");
    PHX_DT_SWITCH(dt, T, PHX_VEC_SWITCH(C, V, {
        int PL, threads, chunk, nchunks;
        PHX_REQUIRE(norm_geometry(P, C, V, &PL, &threads, &chunk, &nchunks, NS) == 0, PHX_E_SHAPE, "norm_stats: C too large");
        if (phx_deterministic()) { chunk = P; nchunks = 1; }       // one block per sample group: no cross-block atomics
        hipLaunchKernelGGL((k_norm_stats<T, V>), dim3(nchunks, NS), dim3(threads), (size_t)PL * C * 2 * sizeof(float),
                           (hipStream_t)stream, (const T*)x, sums, pivot, P, C, PL, chunk);
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_reduce_partials(const float* partial, int T, int C, float* sums, void* stream) {
    hipLaunchKernelGGL(k_reduce_partials, dim3(2 * C), dim3(256), 0, (hipStream_t)stream, partial, T, C, sums);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_reduce_partials_ns(const float* partial, int T, int NS, int C, float* sums, void* stream) {
    PHX_REQUIRE(partial && sums && T > 0 && NS > 0 && NS < 65536 && C > 0, PHX_E_INVAL, "norm_reduce_partials_ns: bad argument");
    hipLaunchKernelGGL(k_reduce_partials_ns, dim3((2 * C + 255) / 256, NS), dim3(256), 0, (hipStream_t)stream, partial, T, C, sums);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_finalize(const float* sums, const float* pivot, const float* gamma, const float* beta, float eps, int NS,
                      int P, int C, int G,
                      float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                      float momentum, void* stream) {
    PHX_REQUIRE(G > 0 && C % G == 0, PHX_E_SHAPE, "norm_finalize: C % G != 0");
    PHX_REQUIRE(momentum == 0.f || (NS == 1 && G == C), PHX_E_INVAL, "moving update only for batch norm");
    const int n = NS * G;
    hipLaunchKernelGGL(k_norm_finalize, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, sums, pivot, gamma, beta, eps,
                       NS, P, C, G, mean, rstd, scale, shift, moving_mean, moving_var, momentum);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_bn_infer_scale_shift(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                             float eps, int C, float* scale, float* shift, void* stream) {
    hipLaunchKernelGGL(k_bn_infer_scale_shift, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, gamma, beta,
                       moving_mean, moving_var, eps, C, scale, shift);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_bn_infer_scale_shift_multi(const void* descs_dev, int n, void* stream) {
    if (n <= 0) return PHX_OK;
    PHX_REQUIRE(descs_dev != nullptr, PHX_E_INVAL, "bn_infer_scale_shift_multi: null descriptor table");
    hipLaunchKernelGGL(k_bn_infer_scale_shift_multi, dim3(2, n), dim3(128), 0, (hipStream_t)stream, (const BnInferDesc*)descs_dev);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_affine_act(const void* x, int x_dt, const float* scale, const float* shift, void* y, int y_dt, int NS, int P,
                   int C, int act, void* stream) {
    PHX_DT_SWITCH(x_dt, TI, PHX_DT_SWITCH(y_dt, TO, PHX_VEC_SWITCH(C, V, {
        int PL, threads, chunk, nchunks;
        PHX_REQUIRE(stream_geometry(P, C, V, &PL, &threads, &chunk, &nchunks, NS) == 0, PHX_E_SHAPE, "affine_act: C too large");
        hipLaunchKernelGGL((k_affine_act<TI, TO, V>), dim3(nchunks, NS), dim3(threads), 0, (hipStream_t)stream,
                           (const TI*)x, scale, shift, (TO*)y, P, C, PL, chunk, act);
    })));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

static int norm_apply_impl(const void* x, int x_dt, const float* sums, int nrep, const float* pivot, const float* gamma,
                           const float* beta, float eps, void* y, int y_dt, float* mean, float* rstd, float* scale,
                           float* shift, float* moving_mean, float* moving_var, float momentum, int NS, int P, int C,
                           int G, int act, HeadFw hd, int hn, void* stream) {
    PHX_REQUIRE(G > 0 && C % G == 0, PHX_E_SHAPE, "norm_apply_fused: C % G != 0");
    PHX_REQUIRE(nrep == 1 || (nrep > 1 && G == C && pivot == nullptr), PHX_E_INVAL, "norm_apply_fused: replicas only for one channel per statistic, no pivot");
    PHX_REQUIRE(hn > 0 || momentum == 0.f || (NS == 1 && G == C), PHX_E_INVAL, "moving update only for batch norm");
    // the one launch site of k_norm_apply_fused; hn > 0 (the head form): bf16 and C % 8 == 0, checked by the caller
    int PL = 0, threads = 0, chunk = 0, nchunks = 0;
    const int too_large = stream_geometry(P, C, C % 8 == 0 ? 8 : 1, &PL, &threads, &chunk, &nchunks, NS);
#define NA_LAUNCH(TI, TO, Vv, HNv)                                                                                                \
    do {                                                                                                                          \
        PHX_REQUIRE(too_large == 0, PHX_E_SHAPE, hn > 0 ? "norm_apply_fused_head: C too large" : "norm_apply_fused: C too large"); \
        PHX_REQUIRE(block_ranges_nonempty(P, chunk, nchunks), PHX_E_SHAPE, "norm_apply_fused: a block without pixels");           \
        hipLaunchKernelGGL((k_norm_apply_fused<TI, TO, Vv, HNv>), dim3(nchunks, NS), dim3(threads), (size_t)2 * (C + G) * sizeof(float), \
                           (hipStream_t)stream, (const TI*)x, sums, pivot, gamma, beta, eps, (TO*)y, mean, rstd, scale, shift,     \
                           moving_mean, moving_var, momentum, P, C, G, PL, chunk, act, nrep, hd);                                 \
    } while (0)
    if (hn == 2) NA_LAUNCH(bf16_t, bf16_t, 8, 2);
    else if (hn > 0) NA_LAUNCH(bf16_t, bf16_t, 8, 4);
    else PHX_DT_SWITCH(x_dt, TI, PHX_DT_SWITCH(y_dt, TO, PHX_VEC_SWITCH(C, V, NA_LAUNCH(TI, TO, V, 0))));
#undef NA_LAUNCH
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_norm_head_supported(int C, int nout, int x_dt, int y_dt) {
    const int cv = C / 8;
    return (x_dt == PHX_BF16 && y_dt == PHX_BF16 && C % 8 == 0 && (nout == 2 || nout == 4) && cv >= 1 && cv <= 64 && (cv & (cv - 1)) == 0) ? 1 : 0;
}
int phx_norm_apply_fused_head(const void* x, int x_dt, const float* sums, const float* pivot, const float* gamma,
                              const float* beta, float eps, void* y, int y_dt, float* mean, float* rstd, float* scale,
                              float* shift, float* moving_mean, float* moving_var, float momentum, int NS, int P, int C,
                              int G, int act, const float* w_head, const float* b_head, int nout, float* y_head, void* stream) {
    PHX_REQUIRE(phx_norm_head_supported(C, nout, x_dt, y_dt) && w_head && b_head && y_head, PHX_E_SHAPE,
                "norm_apply_fused_head: bf16, C / 8 a power of two <= 64, nout in {2, 4}");
    return norm_apply_impl(x, x_dt, sums, 1, pivot, gamma, beta, eps, y, y_dt, mean, rstd, scale, shift, moving_mean, moving_var, momentum,
                           NS, P, C, G, act, HeadFw{w_head, b_head, y_head}, nout, stream);
}
/* the apply pass + the 2 x 2 average pool of its output in one launch (bf16, C % 8 == 0, H and W even; P = images per statistic x H x W) */
int phx_norm_apply_pool_supported(int H, int W, int C) { return (H % 2 == 0 && W % 2 == 0 && C % 8 == 0 && C / 8 <= 256) ? 1 : 0; }
int phx_norm_apply_pool(const void* x, const float* sums, const float* pivot, const float* gamma, const float* beta, float eps, void* y,
                        void* y_pool, float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                        float momentum, int NS, int P, int C, int G, int H, int W, int act, void* stream) {
    PHX_REQUIRE(phx_norm_apply_pool_supported(H, W, C) && G > 0 && C % G == 0 && P % (H * W) == 0, PHX_E_SHAPE,
                "norm_apply_pool: H, W even, C % 8 == 0, C % G == 0, P a multiple of H * W");
    PHX_REQUIRE(x && y && y_pool && sums, PHX_E_INVAL, "norm_apply_pool: null argument");
    PHX_REQUIRE(momentum == 0.f || (NS == 1 && G == C), PHX_E_INVAL, "moving update only for batch norm");
    int PL, threads, chunk, nchunks;
    PHX_REQUIRE(stream_geometry(P / 4, C, 8, &PL, &threads, &chunk, &nchunks, NS) == 0, PHX_E_SHAPE, "norm_apply_pool: C too large");    hipLaunchKernelGGL(k_norm_apply_pool, dim3(nchunks, NS), dim3(threads), (size_t)2 * (C + G) * sizeof(float), (hipStream_t)stream,
                       (const bf16_t*)x, sums, pivot, gamma, beta, eps, (bf16_t*)y, (bf16_t*)y_pool, mean, rstd, scale, shift, moving_mean,
                       moving_var, momentum, P, C, G, H, W, PL, chunk, act);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_norm_apply_fused(const void* x, int x_dt, const float* sums, const float* pivot, const float* gamma,
                         const float* beta, float eps, void* y, int y_dt, float* mean, float* rstd, float* scale,
                         float* shift, float* moving_mean, float* moving_var, float momentum, int NS, int P, int C,
                         int G, int act, void* stream) {
    return norm_apply_impl(x, x_dt, sums, 1, pivot, gamma, beta, eps, y, y_dt, mean, rstd, scale, shift, moving_mean, moving_var, momentum,
                           NS, P, C, G, act, HeadFw{nullptr, nullptr, nullptr}, 0, stream);
}

/* the phase-form convolution's layer (csrc/upconv.hip): x in the packed pixel order, y written as the hi-res map */
int phx_norm_apply_fused_d2s(const void* x, int x_dt, const float* sums, const float* pivot, const float* gamma, const float* beta, float eps,
                             void* y, int y_dt, float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                             float momentum, int NS, int P, int C, int G, int act, int h, int w, void* stream) {
    PHX_REQUIRE(h > 0 && w > 0 && ((size_t)NS * P) % ((size_t)4 * h * w) == 0 && (NS == 1 || P == 4 * h * w), PHX_E_SHAPE,
                "norm_apply_fused_d2s: NS * P = images x 4 h w, a sample group = one image or all of them");
    return norm_apply_impl(x, x_dt, sums, 1, pivot, gamma, beta, eps, y, y_dt, mean, rstd, scale, shift, moving_mean, moving_var, momentum,
                           NS, P, C, G, act, HeadFw{nullptr, nullptr, nullptr, h, w}, 0, stream);
}

}  // extern "C"
