// The class-aware kernels for 9 <= C <= 256 classes: residual multinoulli loss, eval_xent map, GED / NCC / Dice scoring.
// The entries for C <= 8 (losses_opt.hip, mc_stats.hip, metrics.hip, eval_metrics.hip) hold one pixel's classes in registers and stay
// as they are; this file shares no code with them, so their kernels and results cannot move.  Here the classes are walked in chunks of
// WD_CH, per-thread state does not grow with C, every sum that crosses a block is stored per block and added in a fixed order (no
// floating-point atomics): two calls on the same input give the same bits whether or not PHX_DETERMINISTIC is set.
#include "phx_common.h"

#define WD_MAXL 8
#define WD_MAXC 256
#define WD_CH 8                              // classes per chunk: two 16-byte words
#define WD_MAXM 8
#define WD_NMOM (2 + 3 * WD_MAXM)            // sum a, sum a^2, then per annotator j: sum v_j, sum v_j^2, sum a v_j
#define WD_FIN 256

// classes c0 .. c0 + n - 1 of one pixel (p -> class c0); lanes beyond n read `fill`.  16-byte loads where the chunk is whole and aligned.
__device__ __forceinline__ void wd_load(const float* __restrict__ p, int n, float fill, float (&v)[WD_CH]) {
    if (n >= WD_CH && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int c = 0; c < WD_CH; ++c) v[c] = c < n ? p[c] : fill;
    }
}
__device__ __forceinline__ void wd_store(float* __restrict__ p, int n, const float (&v)[WD_CH]) {
    if (n >= WD_CH && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int c = 0; c < WD_CH; ++c)
            if (c < n) p[c] = v[c];
    }
}

// ---- residual multinoulli loss (phiseg_model.py:229-262), any 9 <= C <= 256 ---------------------------------------------------------
struct WDArgs {
    const float* s[WD_MAXL];
    float* ds[WD_MAXL];
    int shift[WD_MAXL];
};

// block = 16 x 16 pixel tile of one image, 4 waves, each an 8 x 8 sub-tile (lane = ly * 8 + lx), as k_residual_ce: the f x f blocks of
// the coarse levels reduce with wave shuffles and every ds element has one writer.
// pass 1: per level a running max, sum of exponentials and the label's logit over the class chunks (A_l = sum_{l' >= l} s_l' is formed
//         chunk by chunk, coarsest level first) -> the level losses, one partial per block and level in `part`;
// pass 2: A_l re-formed per chunk (the second read comes from cache), G_l = (softmax(A_l) - onehot) * gscale from the stored max and
//         sum, ds_k = f x f block sum of sum_{l <= k} G_l; s_out / sm_out from A_0.
template <bool GRAD>
__global__ __launch_bounds__(256) void k_residual_ce_wide(WDArgs a, int L, const uint8_t* __restrict__ labels, int B, int H, int W, int C,
                                                          float gscale, float inv_batch, float* __restrict__ part,
                                                          float* __restrict__ s_out, float* __restrict__ sm_out) {
    const int tiles_x = (W + 15) >> 4, tiles_y = (H + 15) >> 4;
    const int tile = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int px = ((tile % tiles_x) << 4) + ((wave & 1) << 3) + (lane & 7);
    const int py = ((tile / tiles_x) << 4) + ((wave >> 1) << 3) + (lane >> 3);
    const bool valid = px < W && py < H;
    const int lab = (valid && labels) ? labels[((size_t)b * H + py) * W + px] : 0;
    const float* sp[WD_MAXL];                                       // this pixel's class row of every level
#pragma unroll
    for (int l = 0; l < WD_MAXL; ++l) {
        sp[l] = nullptr;
        if (l < L && valid) {
            const int sh = a.shift[l];
            sp[l] = a.s[l] + (((size_t)b * (H >> sh) + (py >> sh)) * (W >> sh) + (px >> sh)) * C;
        }
    }
    float mx[WD_MAXL], se[WD_MAXL], al[WD_MAXL];
#pragma unroll
    for (int l = 0; l < WD_MAXL; ++l) { mx[l] = -INFINITY; se[l] = 0.f; al[l] = 0.f; }

    // ---- pass 1 ----
    if (valid) {
        for (int c0 = 0; c0 < C; c0 += WD_CH) {
            const int n = C - c0;
            float A[WD_CH];
#pragma unroll
            for (int c = 0; c < WD_CH; ++c) A[c] = 0.f;
#pragma unroll
            for (int l = WD_MAXL - 1; l >= 0; --l) {
                if (l >= L) continue;
                float v[WD_CH];
                wd_load(sp[l] + c0, n, 0.f, v);
                float cm = -INFINITY;
#pragma unroll
                for (int c = 0; c < WD_CH; ++c) {
                    A[c] += v[c];
                    if (c < n) cm = fmaxf(cm, A[c]);
                    al[l] = (c0 + c == lab) ? A[c] : al[l];
                }
                const float nm = fmaxf(mx[l], cm);
                float s = se[l] * expf(mx[l] - nm);                 // (first chunk: 0 * exp(-inf) = 0)
#pragma unroll
                for (int c = 0; c < WD_CH; ++c)
                    if (c < n) s += expf(A[c] - nm);
                mx[l] = nm; se[l] = s;
            }
        }
    }
    if (part) {
        __shared__ float wl[4][WD_MAXL];
#pragma unroll
        for (int l = 0; l < WD_MAXL; ++l) {
            if (l >= L) continue;
            const float t = wave_sum(valid ? (mx[l] + logf(se[l])) - al[l] : 0.f);
            if (lane == 0) wl[wave][l] = t;
        }
        __syncthreads();
        if (threadIdx.x < L) {
            const int l = threadIdx.x;
            part[(size_t)blockIdx.x * WD_MAXL + l] = ((wl[0][l] + wl[1][l]) + (wl[2][l] + wl[3][l])) * inv_batch;
        }
    }
    if (!GRAD && !s_out && !sm_out) return;

    // ---- pass 2 ----
    float inv[WD_MAXL];
#pragma unroll
    for (int l = 0; l < WD_MAXL; ++l) inv[l] = valid ? 1.f / se[l] : 0.f;
    const size_t opix = (((size_t)b * H + py) * W + px) * C;
    for (int c0 = 0; c0 < C; c0 += WD_CH) {                         // (uniform: the barriers below are reached by every thread)
        const int n = C - c0;
        float A[WD_CH], G[GRAD ? WD_MAXL : 1][WD_CH];
#pragma unroll
        for (int c = 0; c < WD_CH; ++c) A[c] = 0.f;
#pragma unroll
        for (int l = WD_MAXL - 1; l >= 0; --l) {
            if (l >= L) continue;
            if (valid) {
                float v[WD_CH];
                wd_load(sp[l] + c0, n, 0.f, v);
#pragma unroll
                for (int c = 0; c < WD_CH; ++c) A[c] += v[c];
            }
            if (GRAD) {
#pragma unroll
                for (int c = 0; c < WD_CH; ++c)
                    G[GRAD ? l : 0][c] = (valid && c < n) ? (expf(A[c] - mx[l]) * inv[l] - (c0 + c == lab ? 1.f : 0.f)) * gscale : 0.f;
            }
        }
        if (valid && s_out) wd_store(s_out + opix + c0, n, A);
        if (valid && sm_out) {
            float e[WD_CH];
#pragma unroll
            for (int c = 0; c < WD_CH; ++c) e[c] = expf(A[c] - mx[0]) / se[0];
            wd_store(sm_out + opix + c0, n, e);
        }
        if (GRAD) {
            float run[WD_CH];
#pragma unroll
            for (int c = 0; c < WD_CH; ++c) run[c] = 0.f;
#pragma unroll
            for (int k = 0; k < WD_MAXL; ++k) {
                if (k >= L) continue;
#pragma unroll
                for (int c = 0; c < WD_CH; ++c) run[c] += G[GRAD ? k : 0][c];
                if (!a.ds[k]) continue;
                const int sh = a.shift[k];
                const int hh = H >> sh, ww = W >> sh;
                const int rb = sh < 3 ? sh : 3;                     // bits reducible inside the 8 x 8 wave tile
                float v[WD_CH];
#pragma unroll
                for (int c = 0; c < WD_CH; ++c) {
                    v[c] = run[c];
                    for (int bit = 0; bit < rb; ++bit) {
                        v[c] += __shfl_xor(v[c], 1 << bit, 64);     // x neighbours
                        v[c] += __shfl_xor(v[c], 8 << bit, 64);     // y neighbours
                    }
                }
                if (sh == 4) {
                    // the 16 x 16 block is this work-group's tile (a level of shift 4 divides H and W by 16: the tile is whole):
                    // the four wave sums meet in LDS and are added in a fixed order, thread c writes class c0 + c
                    __shared__ float wsum[4][WD_CH];
                    if (lane == 0) {
#pragma unroll
                        for (int c = 0; c < WD_CH; ++c) wsum[wave][c] = v[c];
                    }
                    __syncthreads();
                    if ((int)threadIdx.x < WD_CH && (int)threadIdx.x < n) {
                        const int c = threadIdx.x;
                        const int ty = (tile / tiles_x), tx = (tile % tiles_x);
                        a.ds[k][(((size_t)b * hh + ty) * ww + tx) * C + c0 + c] = (wsum[0][c] + wsum[1][c]) + (wsum[2][c] + wsum[3][c]);
                    }
                    __syncthreads();
                } else {
                    const int m = (1 << rb) - 1;
                    const bool leader = ((lane & 7) & m) == 0 && ((lane >> 3) & m) == 0;
                    if (leader && valid) wd_store(a.ds[k] + (((size_t)b * hh + (py >> sh)) * ww + (px >> sh)) * C + c0, n, v);
                }
            }
        }
    }
}

// losses[l] = sum over the blocks' partials, in double, in a fixed order (thread t takes blocks t, t + 256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void k_reduce_loss_parts_wide(const float* __restrict__ part, int nblk, int L, float* __restrict__ losses) {
    __shared__ double red[256];
    for (int l = 0; l < L; ++l) {
        double a = 0.0;
        for (int j = threadIdx.x; j < nblk; j += 256) a += (double)part[(size_t)j * WD_MAXL + l];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) losses[l] = (float)red[0];
        __syncthreads();
    }
}

// ---- eval_xent (phiseg_model.py:111): out[p] = logsumexp(logits[p][:]) - logits[p][labels[p]], online over the class chunks ----------
__global__ void k_softmax_xent_map_wide(const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                                        float* __restrict__ out, size_t npix, int C) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int lab = labels[p];
    const float* row = logits + p * C;
    float mx = -INFINITY, se = 0.f, ll = row[0];                    // (a label >= C reads class 0, as the narrow kernel does)
    for (int c0 = 0; c0 < C; c0 += WD_CH) {
        const int n = C - c0;
        float v[WD_CH];
        wd_load(row + c0, n, -INFINITY, v);
        float cm = v[0];
#pragma unroll
        for (int c = 1; c < WD_CH; ++c) cm = fmaxf(cm, v[c]);
        const float nm = fmaxf(mx, cm);
        float s = se * expf(mx - nm);
#pragma unroll
        for (int c = 0; c < WD_CH; ++c) {
            s += expf(v[c] - nm);                                   // (beyond C: exp(-inf) = 0)
            ll = (c0 + c == lab) ? v[c] : ll;
        }
        mx = nm; se = s;
    }
    out[p] = mx + logf(se) - ll;
}

// ---- GED / variance-NCC / Dice for 9 <= C <= 256 (definitions: phx_eval_metrics) -----------------------------------------------------
// maps[img][mask][P] u8 label maps: masks 0 .. N-1 the samples' arg-max, N the arg-max of the mean soft-max, N+1 .. N+M the annotations,
//                                   N+1+M the Dice reference (an annotation chosen by index, or a map of its own)
// mom[img][block][WD_NMOM]:  this block's sums over its 256 pixels of a, a^2, v_j, v_j^2, a v_j  (a = E_ss map, v_j = E_sy[j] map)
// One thread per pixel.  Sweep 1 walks the samples and, per sample, the class chunks: the sample's arg-max.  Sweep 2 walks the class chunks
// and, per chunk, the samples: sum sm[c] and sum log(sm[c] + eps) in double for WD_CH classes at a time, folded at once into the E_ss
// value, the running arg-max of the mean and the annotators' E_sy values -- nothing a thread keeps grows with C.
__global__ __launch_bounds__(256) void k_metrics_wide_pixel(const float* __restrict__ sm, const unsigned char* __restrict__ labels,
                                                            long lab_annot_stride, long lab_pixel_stride,
                                                            const unsigned char* __restrict__ sref_map,
                                                            const unsigned char* __restrict__ sref_annot, unsigned char* __restrict__ maps,
                                                            double* __restrict__ mom, int N, int M, int P, int C) {
    const int img = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool in = p < P;
    const int K2 = N + M + 2;
    unsigned char* mp = maps + (size_t)img * K2 * P;
    const float* base = sm + ((size_t)img * N * P + (in ? p : 0)) * C;       // sample 0 of this pixel; sample k: + k * P * C
    int g[WD_MAXM];
    double vj[WD_MAXM], ess = 0.0;
#pragma unroll
    for (int j = 0; j < WD_MAXM; ++j) { g[j] = -1; vj[j] = 0.0; }
    if (in) {
        for (int k = 0; k < N; ++k) {
            const float* row = base + (size_t)k * P * C;
            float bv = row[0];
            int best = 0;
            for (int c0 = 0; c0 < C; c0 += WD_CH) {
                float v[WD_CH];
                wd_load(row + c0, C - c0, -INFINITY, v);
#pragma unroll
                for (int c = 0; c < WD_CH; ++c)
                    if (v[c] > bv) { bv = v[c]; best = c0 + c; }    // first maximum wins, like np.argmax
            }
            mp[(size_t)k * P + p] = (unsigned char)best;
        }
        const unsigned char* lp = labels + (size_t)img * M * P + (size_t)p * lab_pixel_stride;
#pragma unroll
        for (int j = 0; j < WD_MAXM; ++j)
            if (j < M) {
                g[j] = (int)lp[(size_t)j * lab_annot_stride];
                mp[(size_t)(N + 1 + j) * P + p] = (unsigned char)g[j];
            }
        int ref = 0;
        if (sref_map) ref = (int)sref_map[(size_t)img * P + p];
        else if (sref_annot) { const int an = (int)sref_annot[img]; ref = (int)lp[(size_t)(an < M ? an : M - 1) * lab_annot_stride]; }
        mp[(size_t)(N + 1 + M) * P + p] = (unsigned char)ref;

        const double invn = 1.0 / (double)N;
        double bm = -1.0;
        int bmi = 0;
        for (int c0 = 0; c0 < C; c0 += WD_CH) {
            const int n = C - c0;
            double sa[WD_CH], sl[WD_CH];
#pragma unroll
            for (int c = 0; c < WD_CH; ++c) { sa[c] = 0.0; sl[c] = 0.0; }
            for (int k = 0; k < N; ++k) {
                float v[WD_CH];
                wd_load(base + (size_t)k * P * C + c0, n, 0.f, v);
#pragma unroll
                for (int c = 0; c < WD_CH; ++c) {
                    sa[c] += (double)v[c];
                    sl[c] += (double)logf(v[c] + 1e-8f);
                }
            }
#pragma unroll
            for (int c = 0; c < WD_CH; ++c)
                if (c < n) {
                    const double mc = sa[c] * invn;
                    ess -= mc * sl[c];
                    if (mc > bm) { bm = mc; bmi = c0 + c; }
#pragma unroll
                    for (int j = 0; j < WD_MAXM; ++j)
                        if (g[j] == c0 + c) vj[j] = -sl[c] * invn;
                }
        }
        ess *= invn;
        mp[(size_t)N * P + p] = (unsigned char)bmi;
    }
    // the block's moment sums: wave shuffles, then the four waves in wave order
    __shared__ double red[4][WD_NMOM];
    auto put_sum = [&](int k, double d) {                           // pixels beyond P hold 0
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if (lane == 0) red[w][k] = d;
    };
    put_sum(0, ess);
    put_sum(1, ess * ess);
#pragma unroll
    for (int j = 0; j < WD_MAXM; ++j)
        if (j < M) {
            put_sum(2 + 3 * j, vj[j]);
            put_sum(3 + 3 * j, vj[j] * vj[j]);
            put_sum(4 + 3 * j, ess * vj[j]);
        }
    __syncthreads();
    if ((int)threadIdx.x < 2 + 3 * M) {
        const int k = threadIdx.x;
        mom[((size_t)img * gridDim.x + blockIdx.x) * WD_NMOM + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// pair index -> masks a < b among {N samples, M annotations} (K = N + M)
__device__ __forceinline__ void wd_pair(int idx, int K, int& a, int& b) {
    a = 0;
    while (idx >= K - 1 - a) { idx -= K - 1 - a; ++a; }
    b = a + 1 + idx;
}

// one wave per (mask a, mask b) pair: per-label counts |a = c|, |b = c|, |a = b = c| in the wave's own LDS histogram (integer adds) -> the
// pair's IoU distance over labels label0 .. C-1.  Wave npairs (only with a Dice reference): the Dice per label of (arg-max of the mean
// soft-max, reference map) -> out[img][2 ..].
__global__ __launch_bounds__(256) void k_metrics_wide_pairs(const unsigned char* __restrict__ maps, double* __restrict__ dist,
                                                            float* __restrict__ out, int N, int M, int P, int C, int label0, int nwork) {
    __shared__ int hist[4][3][WD_MAXC];
    const int img = blockIdx.y, K = N + M, npairs = K * (K - 1) / 2;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + wv;
    const bool active = pair < nwork;                               // (idle waves stay for the block barriers)
    const bool dice = pair == npairs;
    int ia = 0, ib = 0;
    if (active && !dice) {
        int a, b;
        wd_pair(pair, K, a, b);
        ia = a < N ? a : a + 1;                                     // the annotations sit behind the mean-arg-max map
        ib = b < N ? b : b + 1;
    } else if (dice) {
        ia = N;
        ib = N + 1 + M;
    }
    const unsigned char* pa = maps + ((size_t)img * (K + 2) + ia) * P;
    const unsigned char* pb = maps + ((size_t)img * (K + 2) + ib) * P;
    int (*h)[WD_MAXC] = hist[wv];
    for (int c = lane; c < WD_MAXC; c += 64) { h[0][c] = 0; h[1][c] = 0; h[2][c] = 0; }
    __syncthreads();
    if (active)
        for (int p = lane; p < P; p += 64) {
            const int la = pa[p], lb = pb[p];
            atomicAdd(&h[0][la], 1);
            atomicAdd(&h[1][lb], 1);
            if (la == lb) atomicAdd(&h[2][la], 1);
        }
    __syncthreads();
    if (!active) return;
    double iou = 0.0;
    for (int c = (dice ? 0 : label0) + lane; c < C; c += 64) {
        const int x = h[0][c], y = h[1][c], z = h[2][c];
        if (dice)
            out[(size_t)img * (2 + C) + 2 + c] = (x == 0 && y == 0) ? 1.f : ((x == 0 || y == 0) ? 0.f : (float)(2.0 * z / (double)(x + y)));
        else if (x == 0 && y == 0)
            iou += 1.0;                                             // both empty counts 1, exactly one empty counts 0
        else if (x != 0 && y != 0)
            iou += (double)z / (double)(x + y - z);
    }
    if (dice) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) iou += __shfl_xor(iou, o, 64);
    if (lane == 0) dist[(size_t)img * npairs + pair] = 1.0 - iou / (double)(C - label0);
}

// one block per image: GED from the pair distances, NCC from the blocks' moment partials, both added in a fixed order
__global__ __launch_bounds__(WD_FIN) void k_metrics_wide_final(const double* __restrict__ dist, const double* __restrict__ mom, int N, int M,
                                                               int P, int nblk, int C, int has_dice, float* __restrict__ out) {
    const int img = blockIdx.x, K = N + M, npairs = K * (K - 1) / 2, t = threadIdx.x;
    __shared__ double red[3][WD_FIN];
    __shared__ double msum[WD_FIN / 32][32];
    double sy = 0.0, ss = 0.0, yy = 0.0;
    for (int pr = t; pr < npairs; pr += WD_FIN) {
        int a, b;
        wd_pair(pr, K, a, b);
        const double d = dist[(size_t)img * npairs + pr];
        if (b < N) ss += d; else if (a >= N) yy += d; else sy += d;
    }
    red[0][t] = sy; red[1][t] = ss; red[2][t] = yy;
    const int k = t & 31, prt = t >> 5;
    double m = 0.0;
    if (k < 2 + 3 * M)
        for (int b = prt; b < nblk; b += WD_FIN / 32) m += mom[((size_t)img * nblk + b) * WD_NMOM + k];
    msum[prt][k] = m;
    __syncthreads();
    if (t < 32) {
        double s = 0.0;
        for (int q = 0; q < WD_FIN / 32; ++q) s += msum[q][t];
        msum[0][t] = s;
    }
    __syncthreads();
    float* o = out + (size_t)img * (2 + C);
    if (!has_dice)
        for (int c = t; c < C; c += WD_FIN) o[2 + c] = 0.f;         // without a Dice reference the Dice slots read 0
    if (t != 0) return;
    double t0 = 0, t1 = 0, t2 = 0;
    for (int q = 0; q < WD_FIN; ++q) { t0 += red[0][q]; t1 += red[1][q]; t2 += red[2][q]; }
    // the reference sums over ordered pairs including i == j (distance 0): ordered sums = 2 x unordered sums
    o[0] = (float)(2.0 / ((double)N * M) * t0 - 2.0 * t1 / ((double)N * N) - 2.0 * t2 / ((double)M * M));
    const double* ac = msum[0];
    const double n = (double)P, ma = ac[0] / n, va = ac[1] / n - ma * ma;
    double ncc = 0.0;
    for (int j = 0; j < M; ++j) {
        const double mv = ac[2 + 3 * j] / n, vv = ac[3 + 3 * j] / n - mv * mv, cav = ac[4 + 3 * j] / n - ma * mv;
        ncc += cav / (sqrt(va) * sqrt(vv));
    }
    o[1] = (float)(ncc / M);
}

static size_t wd_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t wd_maps_bytes(int I, int N, int M, int P) { return wd_align((size_t)I * (N + M + 2) * P); }
static size_t wd_mom_bytes(int I, int P) { return wd_align((size_t)I * ((P + 255) / 256) * WD_NMOM * sizeof(double)); }
static size_t wd_dist_bytes(int I, int N, int M) {
    const size_t K = (size_t)N + M;
    return wd_align((size_t)I * (K * (K - 1) / 2) * sizeof(double));
}

extern "C" {

size_t phx_residual_ce_wide_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * ((H + 15) / 16) * ((W + 15) / 16) * WD_MAXL * sizeof(float);
}

int phx_residual_ce_wide(const float* const* s, float* const* ds, const int* shift, int L, const uint8_t* labels, int B, int H, int W,
                         int C, float weight, float inv_batch, float* losses, float* s_out, float* sm_out, void* work,
                         size_t work_bytes, void* stream) {
    PHX_REQUIRE(L >= 1 && L <= WD_MAXL, PHX_E_SHAPE, "residual_ce_wide: 1 <= L <= 8");
    PHX_REQUIRE(C >= 9 && C <= WD_MAXC, PHX_E_SHAPE, "residual_ce_wide: 9 <= C <= 256 (phx_residual_ce takes 2 <= C <= 8)");
    PHX_REQUIRE(B >= 1 && H >= 1 && W >= 1 && s && shift, PHX_E_SHAPE, "residual_ce_wide: empty input");
    WDArgs a;
    int any_ds = 0;
    for (int l = 0; l < WD_MAXL; ++l) {
        a.s[l] = l < L ? s[l] : nullptr;
        a.ds[l] = (l < L && ds) ? ds[l] : nullptr;
        if (a.ds[l]) any_ds = 1;
        a.shift[l] = l < L ? shift[l] : 0;
        if (l < L) {
            PHX_REQUIRE(a.shift[l] >= 0 && a.shift[l] <= 4 && (H >> a.shift[l]) << a.shift[l] == H && (W >> a.shift[l]) << a.shift[l] == W,
                        PHX_E_SHAPE, "residual_ce_wide: level size must divide the image, factor <= 16");
            PHX_REQUIRE(a.s[l] != nullptr, PHX_E_INVAL, "residual_ce_wide: null level");
        }
    }
    PHX_REQUIRE(!losses || labels, PHX_E_INVAL, "residual_ce_wide: losses without labels");
    PHX_REQUIRE(!losses || (work && work_bytes >= phx_residual_ce_wide_ws_bytes(B, H, W) && ((uintptr_t)work & 3) == 0), PHX_E_INVAL,
                "residual_ce_wide: losses need a workspace of phx_residual_ce_wide_ws_bytes bytes");
    const size_t nblk = (size_t)B * ((H + 15) / 16) * ((W + 15) / 16);
    PHX_REQUIRE(nblk <= 0x7fffffffu, PHX_E_SHAPE, "residual_ce_wide: too many tiles");
    float* part = losses ? (float*)work : nullptr;
    const float gscale = weight * inv_batch;
    if (any_ds)
        hipLaunchKernelGGL(k_residual_ce_wide<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, a, L, labels, B, H, W, C,
                           gscale, inv_batch, part, s_out, sm_out);
    else
        hipLaunchKernelGGL(k_residual_ce_wide<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, a, L, labels, B, H, W, C,
                           gscale, inv_batch, part, s_out, sm_out);
    PHX_CHECK_LAUNCH();
    if (part) {
        hipLaunchKernelGGL(k_reduce_loss_parts_wide, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)part, (int)nblk, L, losses);
        PHX_CHECK_LAUNCH();
    }
    return PHX_OK;
}

int phx_softmax_xent_map_wide(const float* logits, const unsigned char* labels, float* out, size_t npix, int C, void* stream) {
    PHX_REQUIRE(npix > 0 && npix <= (size_t)0x7fffffff * 256 && C >= 9 && C <= WD_MAXC, PHX_E_SHAPE,
                "softmax_xent_map_wide: 9 <= C <= 256 (phx_softmax_xent_map takes 2 <= C <= 8)");
    PHX_REQUIRE(logits && labels && out, PHX_E_INVAL, "softmax_xent_map_wide: null pointer");
    hipLaunchKernelGGL(k_softmax_xent_map_wide, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, labels,
                       out, npix, C);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

size_t phx_metrics_wide_ws_bytes(int I, int N, int M, int P, int C) {
    if (I <= 0 || N <= 0 || M <= 0 || P <= 0 || C <= 0) return 0;
    return wd_maps_bytes(I, N, M, P) + wd_mom_bytes(I, P) + wd_dist_bytes(I, N, M);
}

int phx_metrics_wide(const float* sm, const unsigned char* labels, size_t lab_annot_stride, size_t lab_pixel_stride,
                     const unsigned char* sref_map, const unsigned char* sref_annot, void* work, size_t work_bytes, int I, int N, int M,
                     int P, int C, int label0, float* out, void* stream) {
    PHX_REQUIRE(I > 0 && N > 0 && M > 0 && P > 0 && I <= 65535, PHX_E_SHAPE, "metrics_wide: empty input (or more than 65535 images)");
    PHX_REQUIRE(C >= 9 && C <= WD_MAXC && M <= WD_MAXM && label0 >= 0 && label0 < C, PHX_E_SHAPE,
                "metrics_wide: 9 <= C <= 256, M <= 8, 0 <= label0 < C");
    PHX_REQUIRE((size_t)N + M <= 32768, PHX_E_SHAPE, "metrics_wide: N + M <= 32768 (the pair count is an int)");
    PHX_REQUIRE(sm != nullptr && labels != nullptr && out != nullptr && work != nullptr, PHX_E_INVAL, "metrics_wide: null pointer");
    PHX_REQUIRE(!(sref_map && sref_annot), PHX_E_INVAL, "metrics_wide: the Dice reference is a map or an annotator index, not both");
    PHX_REQUIRE((lab_annot_stride == (size_t)P && lab_pixel_stride == 1) || (lab_annot_stride == 1 && lab_pixel_stride == (size_t)M),
                PHX_E_INVAL, "metrics_wide: labels are [I][M][P] (strides P, 1) or [I][P][M] (strides 1, M)");
    PHX_REQUIRE(work_bytes >= phx_metrics_wide_ws_bytes(I, N, M, P, C), PHX_E_INVAL, "metrics_wide: workspace too small");
    PHX_REQUIRE(((uintptr_t)sm % 4) == 0 && ((uintptr_t)work % 8) == 0, PHX_E_ALIGN,
                "metrics_wide: samples must be aligned to 4 bytes, the workspace to 8");
    const int K = N + M, npairs = K * (K - 1) / 2, nblk = (P + 255) / 256;
    const int has_dice = (sref_map || sref_annot) ? 1 : 0, nwork = npairs + has_dice;
    unsigned char* maps = (unsigned char*)work;
    double* mom = (double*)((char*)work + wd_maps_bytes(I, N, M, P));
    double* dist = (double*)((char*)mom + wd_mom_bytes(I, P));
    hipLaunchKernelGGL(k_metrics_wide_pixel, dim3((unsigned)nblk, (unsigned)I), dim3(256), 0, (hipStream_t)stream, sm, labels,
                       (long)lab_annot_stride, (long)lab_pixel_stride, sref_map, sref_annot, maps, mom, N, M, P, C);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_metrics_wide_pairs, dim3((unsigned)((nwork + 3) / 4), (unsigned)I), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)maps, dist, out, N, M, P, C, label0, nwork);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_metrics_wide_final, dim3((unsigned)I), dim3(WD_FIN), 0, (hipStream_t)stream, (const double*)dist,
                       (const double*)mom, N, M, P, nblk, C, has_dice, out);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
