// Batch renormalisation (tfnorm.batch_renorm; tf.contrib.layers.batch_norm(renorm=True)), training mode:
//   k_renorm_apply_fused   the generic forward: finalisation from the accumulated sums + correction (r, d) + apply + activation
//   k_renorm_small_fwd     the whole forward of a small map (P <= 4096 pixels) in one launch
//   k_renorm_tail          ONE launch per training step over a table of layers: corrected dgamma / dbeta, the six state updates
// The forward kernels only READ the renorm variables and derive the clip bounds from the device step counter; every write of the state
// is in the tail launch, after the last reader of the step.  Inference is batch norm's (phx_bn_infer_scale_shift + phx_affine_act), the
// backward pass is batch norm's with gamma_eff = gamma * r in place of gamma (norm_bwd.hip, norm_onelaunch.hip).
#include <stdlib.h>

#include "norm_common.h"

// the reference's clipping schedule (tfwrapper/normalisation.py:82-126), fp32 like tf.to_float(global_step)
__device__ __forceinline__ void renorm_clip(int t, float* rmax, float* dmax) {
#pragma clang fp contract(off)
    const float x = (float)t;
    *rmax = x < 500.f ? 1.f : (x > 4000.f ? 3.f : (x - 500.f) * 2.f / 3500.f + 1.f);
    *dmax = x < 500.f ? 0.f : (x > 2500.f ? 5.f : (x - 500.f) * 5.f / 2000.f);
}

struct RenormState {                       // the four renorm variables of a layer (read-only in the forward kernels)
    const float *mean, *mean_w, *stddev, *stddev_w;
};
struct RenormOut {                         // per-channel vectors a forward kernel publishes beside mean / rstd / scale / shift
    float *r, *d, *gamma_eff;
};

// r, d and the affine coefficients of one channel: y = x * scale + shift = gamma ((x - mu) / sigma * r + d) + beta.  One definition,
// contraction off: the two forward routes agree bit for bit given the same (mu, var), and a fresh state (all zero) gives r == 1, d == 0
// and batch norm's own (scale, shift) exactly.
__device__ __forceinline__ void renorm_coeffs(float mu, float var, float rs, float eps, float gamma, float beta, float rm, float rmw,
                                              float rsd, float rsw, float rmax, float dmax, float* r, float* d, float* geff,
                                              float* sc, float* sh) {
#pragma clang fp contract(off)
    const float sigma = sqrtf(var + eps);
    const float wm = 1.f - rmw, ws = 1.f - rsw;
    const float mix_mean = rm + wm * mu;
    const float mix_sigma = rsd + ws * sigma;
    const float rv = fminf(sigma / mix_sigma, rmax);                     // no lower clip: the reference passes no 'rmin'
    const float dv = fminf(fmaxf((mu - mix_mean) / mix_sigma, -dmax), dmax);
    const float ge = gamma * rv;
    const float scv = ge * rs;
    const float gd = gamma * dv;
    const float b2 = beta + gd;
    const float t = mu * scv;
    *r = rv; *d = dv; *geff = ge; *sc = scv; *sh = b2 - t;
}

// ---- generic route: x [P][C], sums [C][2] (shifted by pivot when given) -> y = act(renorm(x)).  The geometry and the streaming loop are
// k_norm_apply_fused's; every block derives all channels' coefficients into LDS, block 0 publishes them.
template <typename TI, typename TO, int V>
__global__ void k_renorm_apply_fused(const TI* __restrict__ x, const float* __restrict__ sums, const float* __restrict__ pivot,
                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps, TO* __restrict__ y,
                                     float* mean_out, float* rstd_out, float* scale_out, float* shift_out, RenormOut ro, RenormState st,
                                     const int* __restrict__ step, int P, int C, int PL, int chunk, int act) {
    const int CV = C / V;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    extern __shared__ float cof[];               // [C][2]  scale, shift
    const float invP = 1.f / (float)P;
    const bool pub = blockIdx.x == 0;
    float rmax, dmax;
    renorm_clip(step[0], &rmax, &dmax);
    const float rmw = st.mean_w[0], rsw = st.stddev_w[0];
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float2 sq = *reinterpret_cast<const float2*>(sums + (size_t)c * 2);
        float mu, var, rs, r, d, ge, scv, shv;
        chan_coeffs(sq.x, sq.y, pivot ? pivot[c] : 0.f, invP, eps, &mu, &var, &rs);
        renorm_coeffs(mu, var, rs, eps, gamma[c], beta[c], st.mean[c], rmw, st.stddev[c], rsw, rmax, dmax, &r, &d, &ge, &scv, &shv);
        cof[2 * c] = scv;
        cof[2 * c + 1] = shv;
        if (pub) {
            mean_out[c] = mu; rstd_out[c] = rs; scale_out[c] = scv; shift_out[c] = shv;
            ro.r[c] = r; ro.d[c] = d; ro.gamma_eff[c] = ge;
        }
    }
    __syncthreads();
    if (pl >= PL) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sc[j] = cof[2 * (cv * V + j)];
        sh[j] = cof[2 * (cv * V + j) + 1];
    }
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    int p = p0 + pl;
    for (; p + 3 * PL < p1; p += 4 * PL) {       // four pixels per trip, loads first (see k_norm_stats)
        float v[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) VecIO<TI, V>::load(x, (size_t)(p + u * PL) * C + (size_t)cv * V, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = act_fwd(fmaf(v[u][j], sc[j], sh[j]), act);
            VecIO<TO, V>::store(y, (size_t)(p + u * PL) * C + (size_t)cv * V, v[u]);
        }
    }
    for (; p < p1; p += PL) {
        const size_t off = (size_t)p * C + (size_t)cv * V;
        float v[V];
        VecIO<TI, V>::load(x, off, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = act_fwd(fmaf(v[j], sc[j], sh[j]), act);
        VecIO<TO, V>::store(y, off, v);
    }
}

// ---- one-launch route (the H <= 8 levels): a block of 256 pixel lanes owns EIGHT channels (one 16-byte bf16 / two 16-byte fp32 words
// of every pixel row) for all P <= 4096 pixels and reduces over the pixels inside the block -- no atomics, exact two-pass variance.
// NIT > 0: the slice (P <= 256 NIT pixels) stays in registers between the three passes; NIT == 0: it is read again (from L2).
__device__ __forceinline__ void renorm_block_sum8(float s[8], float* red) {       // red: [4][8] + [8]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = wave_sum(s[j]);
    __syncthreads();                                   // red may still be read from the previous call
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave * 8 + j] = s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = (red[j] + red[8 + j]) + (red[16 + j] + red[24 + j]);
}

template <typename TI, typename TO, int NIT>
__global__ __launch_bounds__(256) void k_renorm_small_fwd(const TI* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, TO* __restrict__ y, float* mean_out,
                                                          float* rstd_out, float* scale_out, float* shift_out, RenormOut ro,
                                                          RenormState st, const int* __restrict__ step, int P, int C, int act) {
    __shared__ float red[32];
    constexpr int NR = NIT > 0 ? NIT : 1;
    const int pl = threadIdx.x, c0 = blockIdx.x * 8;
    const int nit = NIT > 0 ? NIT : (P + 255) / 256;
    float f[NR][8];
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    if constexpr (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = pl + it * 256;
#pragma unroll
            for (int j = 0; j < 8; ++j) f[it][j] = 0.f;
            if (p < P) VecIO<TI, 8>::load(x, (size_t)p * C + c0, f[it]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += f[it][j];
        }
    } else {
        for (int it = 0; it < nit; ++it) {
            const int p = pl + it * 256;
            if (p < P) {
                VecIO<TI, 8>::load(x, (size_t)p * C + c0, f[0]);
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += f[0][j];
            }
        }
    }
    renorm_block_sum8(s, red);
    const float invP = 1.f / (float)P;
    float mu[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { mu[j] = s[j] * invP; s[j] = 0.f; }
    if constexpr (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (pl + it * 256 < P) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float dd = f[it][j] - mu[j]; s[j] = fmaf(dd, dd, s[j]); }
            }
        }
    } else {
        for (int it = 0; it < nit; ++it) {
            const int p = pl + it * 256;
            if (p < P) {
                VecIO<TI, 8>::load(x, (size_t)p * C + c0, f[0]);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float dd = f[0][j] - mu[j]; s[j] = fmaf(dd, dd, s[j]); }
            }
        }
    }
    renorm_block_sum8(s, red);
    float rmax, dmax;
    renorm_clip(step[0], &rmax, &dmax);
    const float rmw = st.mean_w[0], rsw = st.stddev_w[0];
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        const float var = s[j] * invP, rs = rsqrtf(var + eps);
        float r, d, ge;
        renorm_coeffs(mu[j], var, rs, eps, gamma[c], beta[c], st.mean[c], rmw, st.stddev[c], rsw, rmax, dmax, &r, &d, &ge, &sc[j], &sh[j]);
        if (pl == 0) {
            mean_out[c] = mu[j]; rstd_out[c] = rs; scale_out[c] = sc[j]; shift_out[c] = sh[j];
            ro.r[c] = r; ro.d[c] = d; ro.gamma_eff[c] = ge;
        }
    }
    if constexpr (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int p = pl + it * 256;
            if (p < P) {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[it][j] = act_fwd(fmaf(f[it][j], sc[j], sh[j]), act);
                VecIO<TO, 8>::store(y, (size_t)p * C + c0, f[it]);
            }
        }
    } else {
        for (int it = 0; it < nit; ++it) {
            const int p = pl + it * 256;
            if (p < P) {
                VecIO<TI, 8>::load(x, (size_t)p * C + c0, f[0]);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[0][j] = act_fwd(fmaf(f[0][j], sc[j], sh[j]), act);
                VecIO<TO, 8>::store(y, (size_t)p * C + c0, f[0]);
            }
        }
    }
}

// ---- the tail of a training step: one block per layer record.  dgs / dbs are what the backward kernels accumulated for gamma_eff / the
// shift (dgamma', dbeta'); the true gradients dgamma = r dgamma' + d dbeta', dbeta = dbeta' are ADDED to the gradient arena.  Then the six
// state updates from the saved (mean, rstd).  The two weights are one scalar per layer that every thread reads: all threads read them
// BEFORE the block barrier, thread 0 writes them after it, and no other block touches this layer -- reads and writes are ordered.
struct RenormTailDesc {
    const float *mean, *rstd, *r, *d, *dgs, *dbs;
    float *dgamma, *dbeta;
    float *renorm_mean, *renorm_mean_w, *renorm_stddev, *renorm_stddev_w, *moving_mean, *moving_var;
    int C;
    float eps, renorm_momentum, moving_momentum;           // momentum = 1 - decay
};
__global__ __launch_bounds__(256) void k_renorm_tail(const RenormTailDesc* __restrict__ descs) {
#pragma clang fp contract(off)
    const RenormTailDesc t = descs[blockIdx.x];
    const float wm0 = t.renorm_mean_w[0], ws0 = t.renorm_stddev_w[0];
    const float wm = wm0 - (wm0 - 1.f) * t.renorm_momentum, ws = ws0 - (ws0 - 1.f) * t.renorm_momentum;
    for (int c = threadIdx.x; c < t.C; c += blockDim.x) {
        if (t.dgs != nullptr) {
            const float dg = t.dgs[c], db = t.dbs[c];
            atomicAdd(&t.dgamma[c], t.r[c] * dg + t.d[c] * db);      // (accumulate: a variable may be used by several layers)
            atomicAdd(&t.dbeta[c], db);
        }
        const float mu = t.mean[c], sigma = 1.f / t.rstd[c];
        const float rm0 = t.renorm_mean[c], rs0 = t.renorm_stddev[c];
        const float rm = rm0 - (rm0 - mu) * t.renorm_momentum, rsd = rs0 - (rs0 - sigma) * t.renorm_momentum;
        const float new_mean = rm / wm, new_sigma = rsd / ws;
        const float mm0 = t.moving_mean[c], mv0 = t.moving_var[c];
        t.renorm_mean[c] = rm;
        t.renorm_stddev[c] = rsd;
        t.moving_mean[c] = mm0 - (mm0 - new_mean) * t.moving_momentum;
        t.moving_var[c] = mv0 - (mv0 - (new_sigma * new_sigma - t.eps)) * t.moving_momentum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        t.renorm_mean_w[0] = wm;
        t.renorm_stddev_w[0] = ws;
    }
}

extern "C" {

int phx_renorm_apply_fused(const void* x, int x_dt, const float* sums, const float* pivot, const float* gamma, const float* beta, float eps,
                           void* y, int y_dt, float* mean, float* rstd, float* scale, float* shift, float* r, float* d, float* gamma_eff,
                           const float* renorm_mean, const float* renorm_mean_weight, const float* renorm_stddev,
                           const float* renorm_stddev_weight, const int32_t* step_dev, int P, int C, int act, void* stream) {
    PHX_REQUIRE(x && sums && gamma && beta && y && mean && rstd && scale && shift && r && d && gamma_eff && renorm_mean && renorm_mean_weight
                && renorm_stddev && renorm_stddev_weight && step_dev, PHX_E_INVAL, "renorm_apply_fused: null argument");
    PHX_REQUIRE(P > 0 && C > 0, PHX_E_SHAPE, "renorm_apply_fused: bad shape");
    int PL = 0, threads = 0, chunk = 0, nchunks = 0;
    PHX_REQUIRE(stream_geometry(P, C, C % 8 == 0 ? 8 : 1, &PL, &threads, &chunk, &nchunks, 1) == 0, PHX_E_SHAPE, "renorm_apply_fused: C too large");
    const RenormOut ro{r, d, gamma_eff};
    const RenormState st{renorm_mean, renorm_mean_weight, renorm_stddev, renorm_stddev_weight};
    PHX_DT_SWITCH(x_dt, TI, PHX_DT_SWITCH(y_dt, TO, PHX_VEC_SWITCH(C, V, {
        hipLaunchKernelGGL((k_renorm_apply_fused<TI, TO, V>), dim3(nchunks), dim3(threads), (size_t)2 * C * sizeof(float), (hipStream_t)stream,
                           (const TI*)x, sums, pivot, gamma, beta, eps, (TO*)y, mean, rstd, scale, shift, ro, st, (const int*)step_dev, P, C,
                           PL, chunk, act);
    })));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_renorm_small_supported(int P, int C, int x_dt, int y_dt) {
    return ((x_dt == PHX_F32 || x_dt == PHX_BF16) && (y_dt == PHX_F32 || y_dt == PHX_BF16) && P >= 1 && P <= 4096 && C >= 8 && C % 8 == 0) ? 1 : 0;
}

int phx_renorm_small_fwd(const void* x, int x_dt, const float* gamma, const float* beta, float eps, void* y, int y_dt, float* mean,
                         float* rstd, float* scale, float* shift, float* r, float* d, float* gamma_eff, const float* renorm_mean,
                         const float* renorm_mean_weight, const float* renorm_stddev, const float* renorm_stddev_weight,
                         const int32_t* step_dev, int P, int C, int act, void* stream) {
    PHX_REQUIRE(phx_renorm_small_supported(P, C, x_dt, y_dt), PHX_E_INVAL, "renorm_small_fwd: fp32 / bf16, 1 <= P <= 4096, C % 8 == 0");
    PHX_REQUIRE(x && gamma && beta && y && mean && rstd && scale && shift && r && d && gamma_eff && renorm_mean && renorm_mean_weight
                && renorm_stddev && renorm_stddev_weight && step_dev, PHX_E_INVAL, "renorm_small_fwd: null argument");
    const RenormOut ro{r, d, gamma_eff};
    const RenormState st{renorm_mean, renorm_mean_weight, renorm_stddev, renorm_stddev_weight};
#define RS_LAUNCH(TI, TO, NITv)                                                                                                    \
    hipLaunchKernelGGL((k_renorm_small_fwd<TI, TO, NITv>), dim3(C / 8), dim3(256), 0, (hipStream_t)stream, (const TI*)x, gamma, beta, eps, \
                       (TO*)y, mean, rstd, scale, shift, ro, st, (const int*)step_dev, P, C, act)
    PHX_DT_SWITCH(x_dt, TI, PHX_DT_SWITCH(y_dt, TO, {
        if (P <= 256) RS_LAUNCH(TI, TO, 1);
        else if (P <= 1024) RS_LAUNCH(TI, TO, 4);
        else RS_LAUNCH(TI, TO, 0);
    }));
#undef RS_LAUNCH
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_renorm_tail_desc_bytes(void) { return (int)sizeof(RenormTailDesc); }

int phx_renorm_tail_multi(const void* descs_dev, int n, void* stream) {
    if (n <= 0) return PHX_OK;
    PHX_REQUIRE(descs_dev != nullptr, PHX_E_INVAL, "renorm_tail_multi: null descriptor table");
    hipLaunchKernelGGL(k_renorm_tail, dim3(n), dim3(256), 0, (hipStream_t)stream, (const RenormTailDesc*)descs_dev);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
