// Test-set scoring on the device (phiseg_test_quantitative.py / phiseg_test_predictions.py of the reference, scored per image as
// phiseg_model._do_validation does): generalised energy distance, variance-NCC and per-label Dice of I images with N Monte-Carlo
// samples each, read from the buffers the sampling pass and the data provider already keep in HBM:
//   sm      [I * N][P][C] f32    a sampling plan's soft-max output, rows i * N + k, in place
//   labels  [I][P][M] u8         annotator innermost, as DeviceBatchProvider.labels_dev keeps a split (read strided, no transpose pass)
//   sref    [I] u8               per image, the annotator whose map the Dice is taken against (NULL: no Dice)
// Same definitions and the same out layout as phx_validation_metrics (csrc/metrics.hip, which stays as it is: this file shares no code
// with it so that its kernels and results cannot move); what differs is the shape of the pixel pass and how sums are formed:
//   * a block owns 64 pixels and its EV_WAVES waves take the samples round-robin, U at a time, loads first, as k_mc_stats does -- at
//     P = 16 384 that is 256 blocks of 8 waves where k_metrics_pixel has 64 blocks whose threads walk all N samples serially;
//   * sum sm[c] and sum log(sm[c] + eps) are double sums (the waves' partials meet in LDS in wave order), the maps are formed in double;
//   * no floating-point atomics: every block stores its moment partials, the final kernel adds them in a fixed order -- two calls on
//     the same input give the same bits.
// Label maps are bit planes, one 64-bit ballot per (mask, label, 64 pixels); every (mask, mask) pair is one wave of popcounts.
#include "phx_common.h"

#define EV_MAXC 8
#define EV_MAXM 8
#define EV_WAVES 8
#define EV_CHUNK 8                         // accumulators per LDS round: (EV_WAVES - 1) * EV_CHUNK * 64 doubles = 28 KB
#define EV_NMOM (2 + 3 * EV_MAXM)          // sum a, sum a^2, then per annotator j: sum v_j, sum v_j^2, sum a v_j
#define EV_FIN 256                         // threads of the final kernel

template <int CT> __device__ __forceinline__ void ev_load(const float* __restrict__ base, size_t pix, int Cr, bool ok, float (&v)[CT]) {
#pragma unroll
    for (int c = 0; c < CT; ++c) v[c] = 0.f;
    if (!ok) return;
    if (CT == 2) {
        const float2 t = *reinterpret_cast<const float2*>(base + pix * 2);
        v[0] = t.x; v[1] = t.y;
    } else if (CT == 4) {
        const float4 t = *reinterpret_cast<const float4*>(base + pix * 4);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < Cr) v[c] = base[pix * Cr + c];
    }
}

// ---- A: per pixel -- arg-max planes of the samples, of the mean soft-max and of the annotations; the NCC maps and their moments -------
// planes[img][mask][c][word]: bit l of word b = (label of mask at pixel 64 b + l == c); masks 0 .. N-1 samples, N the arg-max of the mean
//                             soft-max, N+1 .. N+M the annotations
// mom[img][block][EV_NMOM]:   this block's sums over its 64 pixels of a, a^2, v_j, v_j^2, a v_j  (a = E_ss map, v_j = E_sy[j] map)
template <int CT, int U>
__global__ __launch_bounds__(EV_WAVES * 64) void k_eval_pixel(const float* __restrict__ sm, const unsigned char* __restrict__ labels,
                                                              unsigned long long* __restrict__ planes, double* __restrict__ mom, int N,
                                                              int M, int P, int C) {
    const int img = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane, W64 = gridDim.x, word = blockIdx.x;
    const bool in = p < P;
    const int Cr = CT == EV_MAXC ? C : CT;
    unsigned long long* pl = planes + (size_t)img * (N + 1 + M) * Cr * W64;
    auto put_planes = [&](int mask, int label) {                   // whole wave; label < 0: pixel beyond P
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < Cr) {
                const unsigned long long bits = __ballot(label == c);
                if (lane == 0) pl[((size_t)mask * Cr + c) * W64 + word] = bits;
            }
    };
    double a[2 * CT];                                              // [c] sum sm[c], [CT + c] sum log(sm[c] + eps)
#pragma unroll
    for (int k = 0; k < 2 * CT; ++k) a[k] = 0.0;
    const size_t img0 = (size_t)img * N * P;                       // pixel index of (img, sample 0, pixel 0)

    for (int n0 = w * U; n0 < N; n0 += EV_WAVES * U) {
        float v[U][CT];
#pragma unroll
        for (int u = 0; u < U; ++u) ev_load<CT>(sm, img0 + (size_t)(n0 + u) * P + p, Cr, in && n0 + u < N, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (n0 + u >= N) break;                                // uniform
            int best = -1;
            if (in) {
                best = 0;
                float bv = v[u][0];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < Cr) {
                        a[c] += (double)v[u][c];
                        a[CT + c] += (double)logf(v[u][c] + 1e-8f);
                        if (v[u][c] > bv) { bv = v[u][c]; best = c; }   // first maximum wins, like np.argmax
                    }
            }
            put_planes(n0 + u, best);
        }
    }

    // ---- the waves' partial sums -> wave 0, in wave order, EV_CHUNK accumulators per round ----
    constexpr int CH = 2 * CT < EV_CHUNK ? 2 * CT : EV_CHUNK;
    __shared__ double red[EV_WAVES - 1][CH][64];
#pragma unroll
    for (int k0 = 0; k0 < 2 * CT; k0 += CH) {
        if (w > 0) {
#pragma unroll
            for (int j = 0; j < CH; ++j) red[w - 1][j][lane] = a[k0 + j];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int j = 0; j < CH; ++j)
#pragma unroll
                for (int ww = 0; ww < EV_WAVES - 1; ++ww) a[k0 + j] += red[ww][j][lane];
        }
        __syncthreads();
    }
    if (w != 0) return;

    // ---- wave 0: arg-max of the mean, the annotations' planes, the cross-entropy maps of this pixel and their sums over the block ----
    const double invn = 1.0 / (double)N;
    int bmi = -1, g[EV_MAXM];
    double ess = 0.0;
    if (in) {
        double bm = a[0] * invn;
        bmi = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < Cr) {
                const double mc = a[c] * invn;
                ess -= mc * a[CT + c];
                if (mc > bm) { bm = mc; bmi = c; }
            }
        ess *= invn;
    }
    put_planes(N, bmi);
#pragma unroll
    for (int j = 0; j < EV_MAXM; ++j) {
        g[j] = -1;
        if (j < M) {                                               // uniform
            if (in) g[j] = (int)labels[((size_t)img * P + p) * M + j];
            put_planes(N + 1 + j, g[j]);
        }
    }
    double* mo = mom + ((size_t)img * W64 + word) * EV_NMOM;
    auto put_sum = [&](int k, double d) {                          // lanes beyond P hold 0
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if (lane == 0) mo[k] = d;
    };
    put_sum(0, ess);
    put_sum(1, ess * ess);
#pragma unroll
    for (int j = 0; j < EV_MAXM; ++j)
        if (j < M) {                                               // uniform
            double sl = 0.0;
#pragma unroll
            for (int c = 0; c < CT; ++c) sl = (c == g[j]) ? a[CT + c] : sl;
            const double v = in ? -sl * invn : 0.0;
            put_sum(2 + 3 * j, v);
            put_sum(3 + 3 * j, v * v);
            put_sum(4 + 3 * j, ess * v);
        }
}

// pair index -> masks a < b among {N samples, M annotations} (K = N + M)
__device__ __forceinline__ void ev_pair(int idx, int K, int& a, int& b) {
    a = 0;
    while (idx >= K - 1 - a) { idx -= K - 1 - a; ++a; }
    b = a + 1 + idx;
}

// ---- B: one wave per (mask a, mask b) pair -- popcounts over the bit planes -> the pair's IoU distance over labels label0 .. C-1;
// wave npairs (only launched with sref): the Dice per label of (arg-max of the mean soft-max, annotation sref[img]) -> out[img][2 ..] ----
__global__ void k_eval_pairs(const unsigned long long* __restrict__ planes, const unsigned char* __restrict__ sref,
                             double* __restrict__ dist, float* __restrict__ out, int N, int M, int W64, int C, int label0, int nwork) {
    const int img = blockIdx.y, K = N + M, npairs = K * (K - 1) / 2;
    const int pair = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= nwork) return;
    const bool dice = pair == npairs;
    int ia, ib;
    if (!dice) {
        int a, b;
        ev_pair(pair, K, a, b);
        ia = a < N ? a : a + 1;                       // plane index: the annotations sit behind the mean-arg-max plane
        ib = b < N ? b : b + 1;
    } else {
        const int an = (int)sref[img];
        ia = N;
        ib = N + 1 + (an < M ? an : M - 1);           // (an annotator index beyond M - 1 reads the last annotation, never past the planes)
    }
    const unsigned long long* pa = planes + ((size_t)img * (K + 1) + ia) * C * W64;
    const unsigned long long* pb = planes + ((size_t)img * (K + 1) + ib) * C * W64;
    double iou = 0.0;
    for (int c = dice ? 0 : label0; c < C; ++c) {     // the GED only looks at labels label0 .. C-1
        int x = 0, y = 0, z = 0;
        for (int wd = lane; wd < W64; wd += 64) {
            const unsigned long long ua = pa[(size_t)c * W64 + wd], ub = pb[(size_t)c * W64 + wd];
            x += __popcll(ua);
            y += __popcll(ub);
            z += __popcll(ua & ub);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            x += __shfl_xor(x, o, 64);
            y += __shfl_xor(y, o, 64);
            z += __shfl_xor(z, o, 64);
        }
        if (dice) {
            if (lane == 0)
                out[(size_t)img * (2 + EV_MAXC) + 2 + c] =
                    (x == 0 && y == 0) ? 1.f : ((x == 0 || y == 0) ? 0.f : (float)(2.0 * z / (double)(x + y)));
        } else if (x == 0 && y == 0) {
            iou += 1.0;                               // both empty counts 1, exactly one empty counts 0
        } else if (x != 0 && y != 0) {
            iou += (double)z / (double)(x + y - z);
        }
    }
    if (!dice && lane == 0) dist[(size_t)img * npairs + pair] = 1.0 - iou / (double)(C - label0);
}

// ---- C: one block per image -- GED from the pair distances, NCC from the blocks' moment partials, both added in a fixed order ---------
__global__ __launch_bounds__(EV_FIN) void k_eval_final(const double* __restrict__ dist, const double* __restrict__ mom, int N, int M,
                                                       int P, int W64, int C, int has_dice, float* __restrict__ out) {
    const int img = blockIdx.x, K = N + M, npairs = K * (K - 1) / 2, t = threadIdx.x;
    __shared__ double red[3][EV_FIN];
    __shared__ double msum[EV_FIN / 32][32];
    double sy = 0.0, ss = 0.0, yy = 0.0;
    for (int pr = t; pr < npairs; pr += EV_FIN) {
        int a, b;
        ev_pair(pr, K, a, b);
        const double d = dist[(size_t)img * npairs + pr];
        if (b < N) ss += d; else if (a >= N) yy += d; else sy += d;
    }
    red[0][t] = sy; red[1][t] = ss; red[2][t] = yy;
    // moment k = t % 32 of blocks t / 32, t / 32 + 8, ...: eight strided partial sums per moment, joined in order below
    const int k = t & 31, part = t >> 5;
    double m = 0.0;
    if (k < 2 + 3 * M)                                   // (the blocks store no more than that)
        for (int b = part; b < W64; b += EV_FIN / 32) m += mom[((size_t)img * W64 + b) * EV_NMOM + k];
    msum[part][k] = m;
    __syncthreads();
    if (t < 32) {
        double s = 0.0;
        for (int q = 0; q < EV_FIN / 32; ++q) s += msum[q][t];
        msum[0][t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    double t0 = 0, t1 = 0, t2 = 0;
    for (int q = 0; q < EV_FIN; ++q) { t0 += red[0][q]; t1 += red[1][q]; t2 += red[2][q]; }
    // the reference sums over ordered pairs including i == j (distance 0): ordered sums = 2 x unordered sums
    const double ged = 2.0 / ((double)N * M) * t0 - 2.0 * t1 / ((double)N * N) - 2.0 * t2 / ((double)M * M);
    float* o = out + (size_t)img * (2 + EV_MAXC);
    o[0] = (float)ged;
    const double* ac = msum[0];
    const double n = (double)P, ma = ac[0] / n, va = ac[1] / n - ma * ma;
    double ncc = 0.0;
    for (int j = 0; j < M; ++j) {
        const double mv = ac[2 + 3 * j] / n, vv = ac[3 + 3 * j] / n - mv * mv, cav = ac[4 + 3 * j] / n - ma * mv;
        ncc += cav / (sqrt(va) * sqrt(vv));
    }
    o[1] = (float)(ncc / M);
    for (int c = has_dice ? C : 0; c < EV_MAXC; ++c) o[2 + c] = 0.f;      // unused Dice slots (all of them without sref) read 0
}

static size_t ev_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t ev_planes_bytes(int I, int N, int M, int P, int C) { return ev_align((size_t)I * (N + 1 + M) * C * ((P + 63) / 64) * 8); }
static size_t ev_mom_bytes(int I, int P) { return ev_align((size_t)I * ((P + 63) / 64) * EV_NMOM * sizeof(double)); }
static size_t ev_dist_bytes(int I, int N, int M) {
    const size_t K = (size_t)N + M;
    return ev_align((size_t)I * (K * (K - 1) / 2) * sizeof(double));
}

extern "C" {

size_t phx_eval_metrics_ws_bytes(int I, int N, int M, int P, int C) {
    if (I <= 0 || N <= 0 || M <= 0 || P <= 0 || C <= 0) return 0;
    return ev_planes_bytes(I, N, M, P, C) + ev_mom_bytes(I, P) + ev_dist_bytes(I, N, M);
}

int phx_eval_metrics(const float* sm, const unsigned char* labels, const unsigned char* sref_annot, void* work, size_t work_bytes,
                     int I, int N, int M, int P, int C, int label0, float* out, void* stream) {
    PHX_REQUIRE(I > 0 && N > 0 && M > 0 && P > 0 && I <= 65535, PHX_E_SHAPE, "eval_metrics: empty input (or more than 65535 images)");
    PHX_REQUIRE(C >= 2 && C <= EV_MAXC && M <= EV_MAXM && label0 >= 0 && label0 < C, PHX_E_SHAPE,
                "eval_metrics: 2 <= C <= 8, M <= 8, 0 <= label0 < C");
    PHX_REQUIRE((size_t)N + M <= 32768, PHX_E_SHAPE, "eval_metrics: N + M <= 32768 (the pair count is an int)");
    PHX_REQUIRE(sm != nullptr && labels != nullptr && out != nullptr && work != nullptr, PHX_E_INVAL, "eval_metrics: null pointer");
    PHX_REQUIRE(work_bytes >= phx_eval_metrics_ws_bytes(I, N, M, P, C), PHX_E_INVAL, "eval_metrics: workspace too small");
    const size_t al = C == 2 ? 8 : (C == 4 ? 16 : 4);
    PHX_REQUIRE(((uintptr_t)sm % al) == 0 && ((uintptr_t)work % 8) == 0, PHX_E_ALIGN,
                "eval_metrics: samples must be aligned to one pixel's classes, the workspace to 8 bytes");
    const int K = N + M, npairs = K * (K - 1) / 2, W64 = (P + 63) / 64, nwork = npairs + (sref_annot != nullptr ? 1 : 0);
    unsigned long long* planes = (unsigned long long*)work;
    double* mom = (double*)((char*)work + ev_planes_bytes(I, N, M, P, C));
    double* dist = (double*)((char*)mom + ev_mom_bytes(I, P));
    const dim3 grid((unsigned)W64, (unsigned)I), block(EV_WAVES * 64);
#define EV_LAUNCH(CT, U) \
    hipLaunchKernelGGL((k_eval_pixel<CT, U>), grid, block, 0, (hipStream_t)stream, sm, labels, planes, mom, N, M, P, C)
    if (C == 2) EV_LAUNCH(2, 4);
    else if (C == 3) EV_LAUNCH(3, 4);
    else if (C == 4) EV_LAUNCH(4, 4);
    else EV_LAUNCH(EV_MAXC, 2);
#undef EV_LAUNCH
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eval_pairs, dim3((unsigned)((nwork + 3) / 4), (unsigned)I), dim3(256), 0, (hipStream_t)stream, planes,
                       sref_annot, dist, out, N, M, W64, C, label0, nwork);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eval_final, dim3((unsigned)I), dim3(EV_FIN), 0, (hipStream_t)stream, dist, mom, N, M, P, W64, C,
                       sref_annot != nullptr ? 1 : 0, out);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
