// Layer normalisation (tfwrapper/normalisation.py:39-68 as layers.conv2D calls it: no gamma / beta, axes (1, 2, 3)): per sample b over
// all N = H W C values of y,
//     m = mean(y_b)   v = mean((y_b - m)^2)   r = 1 / sqrt(v + eps)   pre = (y - m) r   a = act(pre)
//     g = dA act'(pre)   dy = r (g - mean(g) - pre mean(g pre)).
// A sample is N contiguous values whatever C is: the kernels are flat 16-byte streams with ONE pair of sums per sample -- none of the
// per-channel machinery of norm.hip / norm_bwd.hip (no [NS][C][2] sums, no scale / shift vectors, no dgamma / dbeta reductions).
//
// Two forms per direction, chosen from N alone:
//   one launch  N <= phx_layer_norm_one_launch_max(): a block owns a sample -- sums, block reduction, then a second read of the sample
//               (it comes from cache) that writes the result;
//   split       above: the sample is cut into chunks of ln_chunk() elements.  Launch 1: a block reduces a chunk to a pair in
//               ws[b][t][2].  Launch 2: every block re-reduces its sample's partials in a fixed order (wave 0: lane l adds partials
//               l, l + 64, ... in index order, then the xor tree), then streams its chunk.  No third launch.
// The chunk length, the block sizes and every summation order depend on N only -- never on B -- and there is no float atomic anywhere:
// repeats are bit-identical, PHX_DETERMINISTIC needs no branch, and a sample's result does not depend on the batch it sits in (given
// the same alignment phase of its first element: with N % 8 == 0 every sample starts on a vector boundary).
//
// Statistics: shifted sums with the sample's first value as the pivot (as k_norm_stats) in fp32 -- E[y^2] - m^2 on the raw values
// loses everything to cancellation when |m| >> sigma.  `pre` is formed by ONE expression, ln_pre(), in the forward pass, the backward
// reduction and the backward apply, so the ReLU mask of the sums and of dy agree (the slip in k_bn_bwd_onepass).
//
// Access: a span [lo, hi) of absolute element indices = scalar head up to the next multiple of 8 elements, 8-element vectors (16 bytes
// of bf16, two 16-byte words of fp32), scalar tail.  All tensors of a call share the element offset, so one split serves them all; a
// base pointer off 16-byte alignment turns the whole span scalar.
#include "norm_common.h"

namespace {

#ifndef PHX_LN_ONE_LAUNCH_MAX
#define PHX_LN_ONE_LAUNCH_MAX 32768      // measured crossover, B = 64 bf16 (LABBOOK: tools/bench_layer_norm.py --kernels)
#endif
#ifndef PHX_LN_CHUNK
#define PHX_LN_CHUNK 8192                // measured at B = 64, N = 524 288 (same table)
#endif
#ifdef PHX_DEBUG_BUILD                   // libphx_dbg.so: settable, so that both forms can be timed and tested on one shape
static int g_ln_one_max = PHX_LN_ONE_LAUNCH_MAX, g_ln_chunk = PHX_LN_CHUNK;
#else
static constexpr int g_ln_one_max = PHX_LN_ONE_LAUNCH_MAX, g_ln_chunk = PHX_LN_CHUNK;
#endif

struct Span {
    size_t lo, body, nvec, tail, hi;     // head [lo, body), vectors body + 8 k (k < nvec), tail [tail, hi)
};
__device__ __forceinline__ Span make_span(size_t lo, size_t hi, int vec) {
    Span s;
    s.lo = lo;
    s.hi = hi;
    size_t body = vec ? ((lo + 7) & ~(size_t)7) : hi;
    s.body = body < hi ? body : hi;
    s.nvec = (hi - s.body) >> 3;
    s.tail = s.body + (s.nvec << 3);
    return s;
}
// fs(i): one element; fv(i): the eight elements i .. i + 7 (i a multiple of 8)
template <class FS, class FV> __device__ __forceinline__ void span_loop(const Span& s, FS fs, FV fv) {
    for (size_t i = s.lo + threadIdx.x; i < s.body; i += blockDim.x) fs(i);
#pragma unroll 2
    for (size_t k = threadIdx.x; k < s.nvec; k += blockDim.x) fv(s.body + (k << 3));
    for (size_t i = s.tail + threadIdx.x; i < s.hi; i += blockDim.x) fs(i);
}

// (a, b) <- their sums over the block, the same bits in every thread: xor tree per wave, one LDS hop, the waves added in index order
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * w] = a;
        red[2 * w + 1] = b;
    }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
    for (int i = 0; i < nw; ++i) {
        sa += red[2 * i];
        sb += red[2 * i + 1];
    }
    a = sa;
    b = sb;
}
// the nch partial pairs of one sample, in a fixed order (see the head of the file); the same bits in every thread of every block
__device__ __forceinline__ void partial_sum2(const float* __restrict__ part, int nch, float* red, float& a, float& b) {
    if (threadIdx.x < 64) {
        float sa = 0.f, sb = 0.f;
        for (int i = threadIdx.x; i < nch; i += 64) {
            sa += part[2 * i];
            sb += part[2 * i + 1];
        }
        sa = wave_sum(sa);
        sb = wave_sum(sb);
        if (threadIdx.x == 0) {
            red[0] = sa;
            red[1] = sb;
        }
    }
    __syncthreads();
    a = red[0];
    b = red[1];
}

// -m r, rounded once: ln_pre(y) = fma(y, r, nmr) is THE pre-activation value of every kernel below
__device__ __forceinline__ float ln_nmr(float m, float r) { return __fmul_rn(-m, r); }
__device__ __forceinline__ float ln_pre(float y, float r, float nmr) { return fmaf(y, r, nmr); }

template <typename TY> __device__ __forceinline__ void ln_fwd_sums(const TY* __restrict__ y, const Span& s, float pv, float& s1, float& s2) {
    float a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;        // two chains per sum
    span_loop(s,
              [&](size_t i) {
                  const float d = ldf<TY>(y, i) - pv;
                  a1 += d;
                  a2 = fmaf(d, d, a2);
              },
              [&](size_t i) {
                  float v[8];
                  VecIO<TY, 8>::load(y, i, v);
#pragma unroll
                  for (int k = 0; k < 8; k += 2) {
                      const float d0 = v[k] - pv, d1 = v[k + 1] - pv;
                      a1 += d0;
                      b1 += d1;
                      a2 = fmaf(d0, d0, a2);
                      b2 = fmaf(d1, d1, b2);
                  }
              });
    s1 = a1 + b1;
    s2 = a2 + b2;
}
__device__ __forceinline__ void ln_coeffs(float s1, float s2, float pv, float invN, float eps, float* mu, float* rs) {
    float var;
    chan_coeffs(s1, s2, pv, invN, eps, mu, &var, rs);
}
template <typename TY, typename TA>
__device__ __forceinline__ void ln_fwd_stream(const TY* __restrict__ y, TA* __restrict__ a, const Span& s, float rs, float nmr, int act) {
    span_loop(s, [&](size_t i) { stf<TA>(a, i, act_fwd(ln_pre(ldf<TY>(y, i), rs, nmr), act)); },
              [&](size_t i) {
                  float v[8];
                  VecIO<TY, 8>::load(y, i, v);
#pragma unroll
                  for (int k = 0; k < 8; ++k) v[k] = act_fwd(ln_pre(v[k], rs, nmr), act);
                  VecIO<TA, 8>::store(a, i, v);
              });
}

template <typename TD, typename TY>
__device__ __forceinline__ void ln_bwd_sums(const TD* __restrict__ dA, const TY* __restrict__ y, const Span& s, float rs, float nmr, int act,
                                            float& t1, float& t2) {
    float a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
    span_loop(s,
              [&](size_t i) {
                  const float pre = ln_pre(ldf<TY>(y, i), rs, nmr);
                  const float g = ldf<TD>(dA, i) * act_grad_pre(pre, act);
                  a1 += g;
                  a2 = fmaf(g, pre, a2);
              },
              [&](size_t i) {
                  float v[8], d[8];
                  VecIO<TY, 8>::load(y, i, v);
                  VecIO<TD, 8>::load(dA, i, d);
#pragma unroll
                  for (int k = 0; k < 8; k += 2) {
                      const float p0 = ln_pre(v[k], rs, nmr), p1 = ln_pre(v[k + 1], rs, nmr);
                      const float g0 = d[k] * act_grad_pre(p0, act), g1 = d[k + 1] * act_grad_pre(p1, act);
                      a1 += g0;
                      b1 += g1;
                      a2 = fmaf(g0, p0, a2);
                      b2 = fmaf(g1, p1, b2);
                  }
              });
    t1 = a1 + b1;
    t2 = a2 + b2;
}
// dy = r (g - c1 - pre c2) with c1 = mean(g), c2 = mean(g pre)
__device__ __forceinline__ float ln_dy(float d, float yv, float rs, float nmr, float c1, float c2, int act) {
    const float pre = ln_pre(yv, rs, nmr);
    const float g = d * act_grad_pre(pre, act);
    return rs * fmaf(-pre, c2, g - c1);
}
template <typename TD, typename TY, typename TG>
__device__ __forceinline__ void ln_bwd_stream(const TD* __restrict__ dA, const TY* __restrict__ y, TG* __restrict__ dy, const Span& s, float rs,
                                              float nmr, float c1, float c2, int act) {
    span_loop(s, [&](size_t i) { stf<TG>(dy, i, ln_dy(ldf<TD>(dA, i), ldf<TY>(y, i), rs, nmr, c1, c2, act)); },
              [&](size_t i) {
                  float v[8], d[8];
                  VecIO<TY, 8>::load(y, i, v);
                  VecIO<TD, 8>::load(dA, i, d);
#pragma unroll
                  for (int k = 0; k < 8; ++k) d[k] = ln_dy(d[k], v[k], rs, nmr, c1, c2, act);
                  VecIO<TG, 8>::store(dy, i, d);
              });
}

// ---- one launch: block b owns sample b ---------------------------------------------------------------------------------------------
template <typename TY, typename TA>
__global__ void __launch_bounds__(1024) k_layer_norm_fwd_one(const TY* __restrict__ y, TA* __restrict__ a, float* __restrict__ mean,
                                                             float* __restrict__ rstd, size_t N, float invN, float eps, int act, int vec) {
    __shared__ float red[32];
    const size_t lo = (size_t)blockIdx.x * N;
    const Span s = make_span(lo, lo + N, vec);
    const float pv = ldf<TY>(y, lo);
    float s1, s2, mu, rs;
    ln_fwd_sums<TY>(y, s, pv, s1, s2);
    block_sum2(s1, s2, red);
    ln_coeffs(s1, s2, pv, invN, eps, &mu, &rs);
    if (threadIdx.x == 0) {
        mean[blockIdx.x] = mu;
        rstd[blockIdx.x] = rs;
    }
    ln_fwd_stream<TY, TA>(y, a, s, rs, ln_nmr(mu, rs), act);
}
template <typename TD, typename TY, typename TG>
__global__ void __launch_bounds__(1024) k_layer_norm_bwd_one(const TD* __restrict__ dA, const TY* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, TG* __restrict__ dy, size_t N, float invN, int act,
                                                             int vec) {
    __shared__ float red[32];
    const size_t lo = (size_t)blockIdx.x * N;
    const Span s = make_span(lo, lo + N, vec);
    const float rs = rstd[blockIdx.x], nmr = ln_nmr(mean[blockIdx.x], rs);
    float t1, t2;
    ln_bwd_sums<TD, TY>(dA, y, s, rs, nmr, act, t1, t2);
    block_sum2(t1, t2, red);
    ln_bwd_stream<TD, TY, TG>(dA, y, dy, s, rs, nmr, t1 * invN, t2 * invN, act);
}

// ---- split: block (b, t) = blockIdx.x / nch, blockIdx.x % nch owns chunk t of sample b -----------------------------------------------
__device__ __forceinline__ Span chunk_span(size_t N, int nch, int chunk, int vec, int* b, int* t) {
    *b = blockIdx.x / nch;
    *t = blockIdx.x - *b * nch;
    const size_t base = (size_t)(*b) * N, lo = (size_t)(*t) * chunk;
    const size_t hi = lo + chunk < N ? lo + chunk : N;
    return make_span(base + lo, base + hi, vec);
}
template <typename TY>
__global__ void __launch_bounds__(256) k_layer_norm_fwd_partial(const TY* __restrict__ y, float* __restrict__ ws, size_t N, int nch, int chunk,
                                                                int vec) {
    __shared__ float red[8];
    int b, t;
    const Span s = chunk_span(N, nch, chunk, vec, &b, &t);
    const float pv = ldf<TY>(y, (size_t)b * N);          // every chunk of a sample shifts by the sample's first value: the partials add
    float s1, s2;
    ln_fwd_sums<TY>(y, s, pv, s1, s2);
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        ws[2 * (size_t)blockIdx.x] = s1;
        ws[2 * (size_t)blockIdx.x + 1] = s2;
    }
}
template <typename TY, typename TA>
__global__ void __launch_bounds__(256) k_layer_norm_fwd_apply(const TY* __restrict__ y, const float* __restrict__ ws, TA* __restrict__ a,
                                                              float* __restrict__ mean, float* __restrict__ rstd, size_t N, float invN,
                                                              float eps, int nch, int chunk, int act, int vec) {
    __shared__ float red[2];
    int b, t;
    const Span s = chunk_span(N, nch, chunk, vec, &b, &t);
    const float pv = ldf<TY>(y, (size_t)b * N);
    float s1, s2, mu, rs;
    partial_sum2(ws + 2 * (size_t)b * nch, nch, red, s1, s2);
    ln_coeffs(s1, s2, pv, invN, eps, &mu, &rs);
    if (t == 0 && threadIdx.x == 0) {
        mean[b] = mu;
        rstd[b] = rs;
    }
    ln_fwd_stream<TY, TA>(y, a, s, rs, ln_nmr(mu, rs), act);
}
template <typename TD, typename TY>
__global__ void __launch_bounds__(256) k_layer_norm_bwd_partial(const TD* __restrict__ dA, const TY* __restrict__ y, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ ws, size_t N, int nch,
                                                                int chunk, int act, int vec) {
    __shared__ float red[8];
    int b, t;
    const Span s = chunk_span(N, nch, chunk, vec, &b, &t);
    const float rs = rstd[b], nmr = ln_nmr(mean[b], rs);
    float t1, t2;
    ln_bwd_sums<TD, TY>(dA, y, s, rs, nmr, act, t1, t2);
    block_sum2(t1, t2, red);
    if (threadIdx.x == 0) {
        ws[2 * (size_t)blockIdx.x] = t1;
        ws[2 * (size_t)blockIdx.x + 1] = t2;
    }
}
template <typename TD, typename TY, typename TG>
__global__ void __launch_bounds__(256) k_layer_norm_bwd_apply(const TD* __restrict__ dA, const TY* __restrict__ y, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ ws, TG* __restrict__ dy,
                                                              size_t N, float invN, int nch, int chunk, int act, int vec) {
    __shared__ float red[2];
    int b, t;
    const Span s = chunk_span(N, nch, chunk, vec, &b, &t);
    const float rs = rstd[b], nmr = ln_nmr(mean[b], rs);
    float t1, t2;
    partial_sum2(ws + 2 * (size_t)b * nch, nch, red, t1, t2);
    ln_bwd_stream<TD, TY, TG>(dA, y, dy, s, rs, nmr, t1 * invN, t2 * invN, act);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline bool ln_dt_ok(int dt) { return dt == PHX_F32 || dt == PHX_BF16; }
inline bool ln_one_launch(size_t N) { return N <= (size_t)g_ln_one_max; }
inline size_t ln_nchunks(size_t N) { return (N + (size_t)g_ln_chunk - 1) / (size_t)g_ln_chunk; }
// threads of a one-launch block: about four vectors per thread, 64 .. 1024 (a function of N alone)
inline int ln_one_threads(size_t N) {
    int th = 64;
    while (th < 1024 && (size_t)th * 32 < N) th *= 2;
    return th;
}
inline int ln_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// what every entry point checks before it launches anything
inline int ln_check(int B, size_t N, int act, int phase, bool dts_ok, bool ptrs_ok, bool need_ws, const float* ws) {
    PHX_REQUIRE(B > 0 && N > 0, PHX_E_INVAL, "layer_norm: empty tensor");
    PHX_REQUIRE(dts_ok, PHX_E_INVAL, "layer_norm: dtypes are fp32 (0) or bf16 (1)");
    PHX_REQUIRE(ptrs_ok, PHX_E_INVAL, "layer_norm: null argument");
    PHX_REQUIRE(act == PHX_ACT_ID || act == PHX_ACT_RELU || act == PHX_ACT_SOFTPLUS, PHX_E_INVAL, "layer_norm: unknown activation code");
    PHX_REQUIRE(phase == 0 || ((phase == 1 || phase == 2) && need_ws), PHX_E_INVAL, "layer_norm: phase 0 (the layer), or 1 / 2 (one launch of the split form)");
    PHX_REQUIRE(!need_ws || ws != nullptr, PHX_E_INVAL, "layer_norm: the split forms need the workspace of phx_layer_norm_ws_floats");
    PHX_REQUIRE(need_ws ? (size_t)B * ln_nchunks(N) <= (size_t)0x7fffffff : true, PHX_E_SHAPE, "layer_norm: too many chunks for one grid");
    return PHX_OK;
}

}  // namespace

extern "C" {

int phx_layer_norm_one_launch_max(void) { return g_ln_one_max; }

size_t phx_layer_norm_ws_floats(int B, size_t N) {
    if (B <= 0 || N == 0 || ln_one_launch(N)) return 0;
    return (size_t)B * ln_nchunks(N) * 2;
}

int phx_layer_norm_fwd(const void* y, int y_dt, float eps, void* a, int a_dt, float* mean, float* rstd, float* ws, int B, size_t N, int act,
                       int phase, void* stream) {
    const bool one = ln_one_launch(N);
    const int rc = ln_check(B, N, act, phase, ln_dt_ok(y_dt) && ln_dt_ok(a_dt), y && a && mean && rstd, !one, ws);
    if (rc != PHX_OK) return rc;
    const int vec = ln_aligned16(y) && ln_aligned16(a);
    const float invN = 1.f / (float)N;
    hipStream_t S = (hipStream_t)stream;
    if (one) {
        PHX_DT_SWITCH(y_dt, TY, PHX_DT_SWITCH(a_dt, TA, {
            hipLaunchKernelGGL((k_layer_norm_fwd_one<TY, TA>), dim3(B), dim3(ln_one_threads(N)), 0, S, (const TY*)y, (TA*)a, mean, rstd, N, invN,
                               eps, act, vec);
        }));
        PHX_CHECK_LAUNCH();
        return PHX_OK;
    }
    const int nch = (int)ln_nchunks(N), chunk = g_ln_chunk;
    if (phase != 2) PHX_DT_SWITCH(y_dt, TY, {
        hipLaunchKernelGGL((k_layer_norm_fwd_partial<TY>), dim3(B * nch), dim3(256), 0, S, (const TY*)y, ws, N, nch, chunk, vec);
    });
    PHX_CHECK_LAUNCH();
    if (phase != 1) PHX_DT_SWITCH(y_dt, TY, PHX_DT_SWITCH(a_dt, TA, {
        hipLaunchKernelGGL((k_layer_norm_fwd_apply<TY, TA>), dim3(B * nch), dim3(256), 0, S, (const TY*)y, (const float*)ws, (TA*)a, mean, rstd, N,
                           invN, eps, nch, chunk, act, vec);
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_layer_norm_bwd(const void* dA, int dA_dt, const void* y, int y_dt, const float* mean, const float* rstd, void* dy, int dy_dt, float* ws,
                       int B, size_t N, int act, int phase, void* stream) {
    const bool one = ln_one_launch(N);
    const int rc = ln_check(B, N, act, phase, ln_dt_ok(dA_dt) && ln_dt_ok(y_dt) && ln_dt_ok(dy_dt), dA && y && mean && rstd && dy, !one, ws);
    if (rc != PHX_OK) return rc;
    const int vec = ln_aligned16(dA) && ln_aligned16(y) && ln_aligned16(dy);
    const float invN = 1.f / (float)N;
    hipStream_t S = (hipStream_t)stream;
    if (one) {
        PHX_DT_SWITCH(dA_dt, TD, PHX_DT_SWITCH(y_dt, TY, PHX_DT_SWITCH(dy_dt, TG, {
            hipLaunchKernelGGL((k_layer_norm_bwd_one<TD, TY, TG>), dim3(B), dim3(ln_one_threads(N)), 0, S, (const TD*)dA, (const TY*)y, mean, rstd,
                               (TG*)dy, N, invN, act, vec);
        })));
        PHX_CHECK_LAUNCH();
        return PHX_OK;
    }
    const int nch = (int)ln_nchunks(N), chunk = g_ln_chunk;
    if (phase != 2) PHX_DT_SWITCH(dA_dt, TD, PHX_DT_SWITCH(y_dt, TY, {
        hipLaunchKernelGGL((k_layer_norm_bwd_partial<TD, TY>), dim3(B * nch), dim3(256), 0, S, (const TD*)dA, (const TY*)y, mean, rstd, ws, N, nch,
                           chunk, act, vec);
    }));
    PHX_CHECK_LAUNCH();
    if (phase != 1) PHX_DT_SWITCH(dA_dt, TD, PHX_DT_SWITCH(y_dt, TY, PHX_DT_SWITCH(dy_dt, TG, {
        hipLaunchKernelGGL((k_layer_norm_bwd_apply<TD, TY, TG>), dim3(B * nch), dim3(256), 0, S, (const TD*)dA, (const TY*)y, mean, rstd,
                           (const float*)ws, (TG*)dy, N, invN, nch, chunk, act, vec);
    })));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

#ifdef PHX_DEBUG_BUILD
int phx_debug_layer_norm_policy(int one_launch_max, int chunk) {
    PHX_REQUIRE(one_launch_max >= 0 && chunk >= 8 && chunk % 8 == 0, PHX_E_INVAL, "debug_layer_norm_policy: one_launch_max >= 0, chunk a positive multiple of 8");
    g_ln_one_max = one_launch_max;
    g_ln_chunk = chunk;
    return PHX_OK;
}
#endif

}  // extern "C"
