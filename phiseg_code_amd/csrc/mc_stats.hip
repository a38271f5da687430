// Per-pixel Monte-Carlo sample statistics (the uncertainty maps of the reference's inference API, phiseg_model.py:378-475, and the
// error maps of phiseg_generate_samples.py:46-82) in ONE pass over the N samples of I images.  Every map is a function of
// per-pixel sums over the samples:
//   sum y[c], sum y[c] y[d]            y = sm - sm(sample 0): the pivot shift keeps the second moments at the scale of the spread, so
//                                       a variance near zero does not drown in the rounding of sum x^2 (double sums on top of it)
//   sum log(sm[c] + eps)               once over all N samples, once over the first M (the reference's E_yy indexes samples)
//   sum t[c], sum t[c]^2               t = clip(logit, 1e-5, 1 - 1e-5) - the same of sample 0
//   sum (logsumexp(l) - l[sref])
// A block owns 64 pixels; its MC_WAVES waves take the samples round-robin (U at a time, loads first) and combine through LDS; wave 0
// forms the maps.  At the LIDC shape (P = 16 384, I = 1) that is 256 blocks of 8 waves instead of one wave per CU.
#include "phx_common.h"

#define MC_MAXC 8
#define MC_MAXM 8
#define MC_WAVES 8
#define MC_CHUNK 8            // accumulators per LDS round: (MC_WAVES - 1) * MC_CHUNK * 64 doubles = 28 KB

template <int CT> struct McAcc {
    static constexpr int NP = CT * (CT + 1) / 2;
    static constexpr int SY = 0, SYY = CT, SLOG = CT + NP, SLOGM = SLOG + CT, LG = SLOGM + CT, LGG = LG + CT - 1, XENT = LGG + CT - 1,
                         K = XENT + 1;
    __host__ __device__ static constexpr int pair(int c, int d) { return SYY + c * CT - c * (c - 1) / 2 + (d - c); }   // c <= d
};

template <int CT> __device__ __forceinline__ void mc_load(const float* __restrict__ base, size_t pix, int Cr, bool ok, float (&v)[CT]) {
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

__device__ __forceinline__ float mc_clip(float l) { return fminf(fmaxf(l, 1e-5f), 1.f - 1e-5f); }

template <int CT, int U>
__global__ __launch_bounds__(MC_WAVES * 64) void k_mc_stats(const float* __restrict__ logits, const float* __restrict__ sm,
                                                            const unsigned char* __restrict__ gt, const unsigned char* __restrict__ sref,
                                                            int N, int M, int P, int C, unsigned mask, float* __restrict__ mean_sm,
                                                            unsigned char* __restrict__ amax, float* __restrict__ maps) {
    typedef McAcc<CT> A;
    const int img = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const bool in = p < P;
    const int Cr = CT == MC_MAXC ? C : CT;
    const bool has_sm = sm != nullptr, has_lg = logits != nullptr;
    const bool want_cov = (mask & ((1u << PHX_MC_COV_DET) | (1u << PHX_MC_COV_DET_DROP_LAST))) != 0;
    const bool want_log = (mask & ((1u << PHX_MC_E_SS) | (1u << PHX_MC_E_SY) | (1u << PHX_MC_E_YY))) != 0;
    const bool want_xent = (mask & (1u << PHX_MC_XENT_MEAN)) != 0;
    double a[A::K];
#pragma unroll
    for (int k = 0; k < A::K; ++k) a[k] = 0.0;
    const size_t img0 = (size_t)img * N * P;                       // pixel index of (img, sample 0, pixel 0)
    float piv[CT], pivl[CT];
    mc_load<CT>(sm, img0 + p, Cr, in && has_sm, piv);
    mc_load<CT>(logits, img0 + p, Cr, in && has_lg, pivl);
#pragma unroll
    for (int c = 0; c < CT; ++c) pivl[c] = mc_clip(pivl[c]);
    const int lab = (in && sref != nullptr) ? (int)sref[(size_t)img * P + p] : 0;

    for (int n0 = w * U; n0 < N; n0 += MC_WAVES * U) {
        float vs[U][CT], vl[U][CT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = in && n0 + u < N;
            mc_load<CT>(sm, img0 + (size_t)(n0 + u) * P + p, Cr, ok && has_sm, vs[u]);
            mc_load<CT>(logits, img0 + (size_t)(n0 + u) * P + p, Cr, ok && has_lg, vl[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (n0 + u >= N) break;                                // uniform
            if (has_sm) {
                double y[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    y[c] = (double)vs[u][c] - (double)piv[c];
                    a[A::SY + c] += y[c];
                    a[A::pair(c, c)] += y[c] * y[c];
                }
                if (want_cov) {
#pragma unroll
                    for (int c = 0; c < CT; ++c)
#pragma unroll
                        for (int d = c + 1; d < CT; ++d) a[A::pair(c, d)] += y[c] * y[d];
                }
                if (want_log) {
                    const bool first = n0 + u < M;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const double lg = (double)logf(vs[u][c] + 1e-8f);
                        a[A::SLOG + c] += lg;
                        if (first) a[A::SLOGM + c] += lg;
                    }
                }
            }
            if (has_lg) {
#pragma unroll
                for (int c = 0; c < CT - 1; ++c) {
                    const double t = (double)mc_clip(vl[u][c]) - (double)pivl[c];
                    a[A::LG + c] += t;
                    a[A::LGG + c] += t * t;
                }
                if (want_xent) {
                    float mx = vl[u][0], ll = vl[u][0];
#pragma unroll
                    for (int c = 1; c < CT; ++c)
                        if (c < Cr) mx = fmaxf(mx, vl[u][c]);
                    float se = 0.f;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < Cr) {
                            se += expf(vl[u][c] - mx);
                            ll = (c == lab) ? vl[u][c] : ll;
                        }
                    a[A::XENT] += (double)(mx + logf(se)) - (double)ll;
                }
            }
        }
    }

    // ---- the waves' partial sums -> wave 0, MC_CHUNK accumulators per round ----
    __shared__ double red[MC_WAVES - 1][MC_CHUNK][64];
#pragma unroll
    for (int k0 = 0; k0 < A::K; k0 += MC_CHUNK) {
        if (w > 0) {
#pragma unroll
            for (int j = 0; j < MC_CHUNK; ++j)
                if (k0 + j < A::K) red[w - 1][j][lane] = a[k0 + j];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int j = 0; j < MC_CHUNK; ++j)
                if (k0 + j < A::K) {
#pragma unroll
                    for (int ww = 0; ww < MC_WAVES - 1; ++ww) a[k0 + j] += red[ww][j][lane];
                }
        }
        __syncthreads();
    }
    if (w != 0 || !in) return;

    // ---- maps of this pixel ----
    const double invn = 1.0 / (double)N;
    float* mp = maps + (size_t)img * PHX_MC_NMAPS * P + p;
    if (has_sm) {
        double mean[CT], sd = 0.0;
        int best = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            mean[c] = 0.0;
            if (c < Cr) {
                const double my = a[A::SY + c] * invn;
                mean[c] = (double)piv[c] + my;
                const double var = a[A::pair(c, c)] * invn - my * my;
                sd += sqrt(var > 0.0 ? var : 0.0);
            }
        }
        double bm = mean[0];
#pragma unroll
        for (int c = 1; c < CT; ++c)
            if (c < Cr && mean[c] > bm) { bm = mean[c]; best = c; }   // first maximum wins, like np.argmax
        if (mean_sm != nullptr) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < Cr) mean_sm[((size_t)img * P + p) * Cr + c] = (float)mean[c];
        }
        if (amax != nullptr) amax[(size_t)img * P + p] = (unsigned char)best;
        if (mask & (1u << PHX_MC_STD_MEAN)) mp[(size_t)PHX_MC_STD_MEAN * P] = (float)(sd / (double)Cr);
        if (want_cov) {
            // unbiased covariance of the samples; symmetric elimination without pivoting (positive semi-definite: every pivot is a
            // Schur complement <= its diagonal entry).  The product of the first n - 1 pivots is the determinant without the last class.
            double m[CT][CT];
            const double inv1 = 1.0 / (double)(N - 1);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int d = c; d < CT; ++d) {
                    const double v = (a[A::pair(c, d)] - a[A::SY + c] * a[A::SY + d] * invn) * inv1;
                    m[c][d] = v;
                    m[d][c] = v;
                }
            double det = 1.0, det_drop = 1.0;
#pragma unroll
            for (int k = 0; k < CT; ++k)
                if (k < Cr) {
                    const double pv = m[k][k];
                    if (k == Cr - 1) det_drop = det;
                    det *= pv;
                    if (pv != 0.0) {
                        const double ipv = 1.0 / pv;
#pragma unroll
                        for (int i = k + 1; i < CT; ++i)
                            if (i < Cr) {
                                const double f = m[i][k] * ipv;
#pragma unroll
                                for (int j = k + 1; j < CT; ++j) m[i][j] -= f * m[k][j];
                            }
                    }
                }
            if (mask & (1u << PHX_MC_COV_DET)) mp[(size_t)PHX_MC_COV_DET * P] = (float)det;
            if (mask & (1u << PHX_MC_COV_DET_DROP_LAST)) mp[(size_t)PHX_MC_COV_DET_DROP_LAST * P] = (float)det_drop;
        }
        if (mask & (1u << PHX_MC_E_SS)) {
            double e = 0.0;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < Cr) e -= mean[c] * a[A::SLOG + c];
            mp[(size_t)PHX_MC_E_SS * P] = (float)(e * invn);
        }
        if ((mask & ((1u << PHX_MC_E_SY) | (1u << PHX_MC_E_YY))) && gt != nullptr) {
            double esy = 0.0, eyy = 0.0;
            for (int j = 0; j < M; ++j) {
                const int g = gt[((size_t)img * M + j) * P + p];
                double sl = 0.0, slm = 0.0;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    sl = (c == g) ? a[A::SLOG + c] : sl;
                    slm = (c == g) ? a[A::SLOGM + c] : slm;
                }
                esy -= sl;
                eyy -= slm;
            }
            if (mask & (1u << PHX_MC_E_SY)) mp[(size_t)PHX_MC_E_SY * P] = (float)(esy * invn / (double)M);
            if (mask & (1u << PHX_MC_E_YY)) mp[(size_t)PHX_MC_E_YY * P] = (float)(eyy / ((double)M * (double)M));
        }
    }
    if (has_lg) {
        if (mask & (1u << PHX_MC_XENT_MEAN)) mp[(size_t)PHX_MC_XENT_MEAN * P] = (float)(a[A::XENT] * invn);
        if (mask & (1u << PHX_MC_COV_TRACE)) {
            double tr = 0.0;
#pragma unroll
            for (int c = 0; c < CT - 1; ++c)
                if (c < Cr - 1) {
                    const double mt = a[A::LG + c] * invn;
                    tr += a[A::LGG + c] * invn - mt * mt;
                }
            mp[(size_t)PHX_MC_COV_TRACE * P] = (float)tr;
        }
    }
}

// eval_xent of one graph instance (phiseg_model.py:111): out[p] = logsumexp(l[p]) - l[p][label[p]]
__global__ void k_softmax_xent_map(const float* __restrict__ logits, const unsigned char* __restrict__ labels, float* __restrict__ out,
                                   size_t npix, int C) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int lab = labels[p];
    float v[MC_MAXC];
#pragma unroll
    for (int c = 0; c < MC_MAXC; ++c) v[c] = c < C ? logits[p * C + c] : -INFINITY;
    float mx = v[0], ll = v[0], se = 0.f;
#pragma unroll
    for (int c = 1; c < MC_MAXC; ++c) mx = fmaxf(mx, v[c]);
#pragma unroll
    for (int c = 0; c < MC_MAXC; ++c)
        if (c < C) {
            se += expf(v[c] - mx);
            ll = (c == lab) ? v[c] : ll;
        }
    out[p] = mx + logf(se) - ll;
}

extern "C" {

size_t phx_mc_stats_ws_bytes(int I, int N, int M, int P, int C) {
    (void)I; (void)N; (void)M; (void)P; (void)C;
    return 0;                                     // the samples are combined inside the block: no scratch
}

int phx_mc_stats(const float* logits, const float* sm, const unsigned char* gt, const unsigned char* sref, int I, int N, int M, int P,
                 int C, unsigned map_mask, float* mean_sm, unsigned char* amax, float* maps, void* work, size_t work_bytes,
                 void* stream) {
    (void)work; (void)work_bytes;
    PHX_REQUIRE(I > 0 && P > 0 && I <= 65535, PHX_E_SHAPE, "mc_stats: empty input (or more than 65535 images)");
    PHX_REQUIRE(C >= 2 && C <= MC_MAXC && N >= 2 && N <= 1024, PHX_E_SHAPE, "mc_stats: 2 <= C <= 8, 2 <= N <= 1024");
    PHX_REQUIRE(gt == nullptr || (M >= 1 && M <= MC_MAXM), PHX_E_SHAPE, "mc_stats: 1 <= M <= 8");
    PHX_REQUIRE(logits != nullptr || sm != nullptr, PHX_E_INVAL, "mc_stats: neither logits nor soft-max given");
    PHX_REQUIRE((map_mask >> PHX_MC_NMAPS) == 0, PHX_E_INVAL, "mc_stats: unknown map plane");
    PHX_REQUIRE(map_mask == 0 || maps != nullptr, PHX_E_INVAL, "mc_stats: maps requested without an output buffer");
    PHX_REQUIRE(map_mask != 0 || mean_sm != nullptr || amax != nullptr, PHX_E_INVAL, "mc_stats: nothing requested");
    const unsigned need_sm = (1u << PHX_MC_STD_MEAN) | (1u << PHX_MC_COV_DET) | (1u << PHX_MC_COV_DET_DROP_LAST) | (1u << PHX_MC_E_SS) |
                             (1u << PHX_MC_E_SY) | (1u << PHX_MC_E_YY);
    const unsigned need_gt = (1u << PHX_MC_E_SY) | (1u << PHX_MC_E_YY);
    const unsigned need_lg = (1u << PHX_MC_XENT_MEAN) | (1u << PHX_MC_COV_TRACE);
    PHX_REQUIRE(sm != nullptr || ((map_mask & need_sm) == 0 && mean_sm == nullptr && amax == nullptr), PHX_E_INVAL,
                "mc_stats: a requested output needs the soft-max samples");
    PHX_REQUIRE(gt != nullptr || (map_mask & need_gt) == 0, PHX_E_INVAL, "mc_stats: E_SY / E_YY need the annotations");
    PHX_REQUIRE(logits != nullptr || (map_mask & need_lg) == 0, PHX_E_INVAL, "mc_stats: XENT_MEAN / COV_TRACE need the logits");
    PHX_REQUIRE(sref != nullptr || (map_mask & (1u << PHX_MC_XENT_MEAN)) == 0, PHX_E_INVAL, "mc_stats: XENT_MEAN needs sref");
    PHX_REQUIRE((map_mask & (1u << PHX_MC_E_YY)) == 0 || N >= M, PHX_E_INVAL, "mc_stats: E_YY reads the first M samples (N >= M)");
    const size_t al = C == 2 ? 8 : (C == 4 ? 16 : 4);
    PHX_REQUIRE(((uintptr_t)logits % al) == 0 && ((uintptr_t)sm % al) == 0, PHX_E_ALIGN, "mc_stats: samples must be aligned to one pixel's classes");
    const dim3 grid((unsigned)((P + 63) / 64), (unsigned)I), block(MC_WAVES * 64);
    if (gt == nullptr) M = 0;
#define MC_LAUNCH(CT, U)                                                                                                            \
    hipLaunchKernelGGL((k_mc_stats<CT, U>), grid, block, 0, (hipStream_t)stream, logits, sm, gt, sref, N, M, P, C, map_mask, mean_sm, \
                       amax, maps)
    if (C == 2) MC_LAUNCH(2, 4);
    else if (C == 3) MC_LAUNCH(3, 4);
    else if (C == 4) MC_LAUNCH(4, 4);
    else MC_LAUNCH(MC_MAXC, 2);
#undef MC_LAUNCH
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_softmax_xent_map(const float* logits, const unsigned char* labels, float* out, size_t npix, int C, void* stream) {
    PHX_REQUIRE(npix > 0 && C >= 2 && C <= MC_MAXC, PHX_E_SHAPE, "softmax_xent_map: 2 <= C <= 8");
    hipLaunchKernelGGL(k_softmax_xent_map, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, labels, out,
                       npix, C);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
