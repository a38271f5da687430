// Normalisation backward (batch / group / instance), streaming form: the reduce + apply pair with its head, rider, space-to-depth
// and bias forms, the one-pass batch-norm backward with its grid barrier, and the stand-alone finalize + apply pair.
#include <stdlib.h>
#include <type_traits>

#include "norm_common.h"

// HN > 0 (backward of the layer whose only reader is a 1x1 head, see HeadFw in norm.hip): the upstream gradient dA = dyh wh^T is a rank-HN
// function of the head's tiny gradient -- it is formed here per element (rounded to the storage type, as the head's data-gradient
// launch would have stored it) instead of being written by that launch and read back by the two backward passes.
struct HeadBw {
    const float *dy, *w;
    int ph, pw, pc;      // pw > 0: x / dx are in the packed pixel order of the phase-form convolution, dA is the hi-res map [B][2 ph][2 pw][pc]
};
// dv = bf16(d wh^T): the head-derived upstream gradient of one pixel's V channels from the head's gradient d[HN]
template <int V, int HN>
__device__ __forceinline__ void da_from_head(const float (&d)[HN], const float (&hw)[V][HN], float (&dv)[V]) {
#pragma unroll
    for (int j = 0; j < V; j += 2) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int o = 0; o < HN; ++o) { a0 = fmaf(d[o], hw[j][o], a0); a1 = fmaf(d[o], hw[j + 1][o], a1); }
        const unsigned w2 = f2bf_pk(a0, a1);          // stored precision of dA (v_cvt_pk_bf16_f32: round to nearest even)
        dv[j] = __uint_as_float(w2 << 16);
        dv[j + 1] = __uint_as_float(w2 & 0xffff0000u);
    }
}
template <typename TD, int V, int HN>
__device__ __forceinline__ void load_da(const TD* __restrict__ dA, size_t off, const HeadBw& hb, size_t pix,
                                        const float (&hw)[V][HN > 0 ? HN : 1], float (&dv)[V]) {
    if constexpr (HN == 0) {
        if (hb.pw > 0) off = packed_to_hi_pixel(pix, hb.ph, hb.pw) * hb.pc + (off - pix * hb.pc);      // (space-to-depth on the fly)
        VecIO<TD, V>::load(dA, off, dv);
    } else {
        static_assert(HN == 0 || (V % 2 == 0 && std::is_same<TD, bf16_t>::value), "head-derived dA: bf16, even vector width");
        float d[HN];                                      // one 8- / 16-byte load per pixel
        if constexpr (HN == 2) {
            const float2 q = *reinterpret_cast<const float2*>(hb.dy + pix * 2);
            d[0] = q.x; d[1] = q.y;
        } else {
            const float4 q = *reinterpret_cast<const float4*>(hb.dy + pix * 4);
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        }
        da_from_head<V, HN>(d, hw, dv);
    }
}

// HR > 0 (rider of the backward reduction): a 1x1 head with HR outputs reads this unit's activation a = act(x * scale + shift) -- its
// filter and bias gradient dw[c][o] = sum_p a[p][c] dy[p][o], db[o] = sum_p dy[p][o] are accumulated on the (x, scale, shift) the reduction
// has loaded anyway (a rounded to bf16, as the stored activation and phx_head1x1_wgrad_multi's xscale form have it), instead of a
// second pass over x by the head's own filter-gradient job.  acc[nrep][C + 1][HR]: replica blockIdx.x % nrep, row C = the bias
// gradient; zero before the launch, folded into (dw, db) by block 0 of the apply launch (HeadFold).
struct HeadRider {
    const float* dy;     // [P][HR] fp32 (HN > 0: the same tensor as HeadBw::dy)
    float* acc;
};
struct HeadFold {
    const float* acc;    // NULL: nothing to fold
    float *dw, *db;
    int hr;
};
template <int HR>
__device__ __forceinline__ void load_head_dy(const float* __restrict__ dy, size_t pix, float (&d)[HR > 0 ? HR : 1]) {
    if constexpr (HR == 2) {
        const float2 q = *reinterpret_cast<const float2*>(dy + pix * 2);
        d[0] = q.x; d[1] = q.y;
    } else if constexpr (HR == 4) {
        const float4 q = *reinterpret_cast<const float4*>(dy + pix * 4);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
}
// acc[j][o] += bf16(act(x[j] * sc[j] + sh[j])) * d[o]
template <int V, int HR>
__device__ __forceinline__ void head_rider_fma(const float (&xv)[V], const float (&sc)[V], const float (&sh)[V], int act,
                                               const float (&d)[HR > 0 ? HR : 1], float (&acc)[V][HR > 0 ? HR : 1]) {
    static_assert(V % 2 == 0, "head rider: even vector width");
#pragma unroll
    for (int j = 0; j < V; j += 2) {
        const unsigned w2 = f2bf_pk(act_fwd(fmaf(xv[j], sc[j], sh[j]), act), act_fwd(fmaf(xv[j + 1], sc[j + 1], sh[j + 1]), act));
        const float a0 = __uint_as_float(w2 << 16), a1 = __uint_as_float(w2 & 0xffff0000u);
#pragma unroll
        for (int o = 0; o < HR; ++o) {
            acc[j][o] = fmaf(a0, d[o], acc[j][o]);
            acc[j + 1][o] = fmaf(a1, d[o], acc[j + 1][o]);
        }
    }
}

// what k_norm_bwd_apply_fused's one-stage finalisation reads for one channel
struct BwdChanLoads {
    float gm, rs, mu, sc, sh, fs, fp;
    float2 v[4];         // {sum g, sum g * xhat} of four accumulator replicas
};
template <typename TD, typename TX, typename TO, int V, int HN = 0>
__global__ void k_norm_bwd_apply_fused(const TD* __restrict__ dA, const TX* __restrict__ x,
                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                       const float* __restrict__ gamma, const float* __restrict__ sums2,
                                       TO* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, int P,
                                       int C, int G, int PL, int chunk, int act, int nrep,
                                       const float* __restrict__ fsums, const float* __restrict__ fpivot,
                                       float* __restrict__ dbias, HeadBw hb, HeadFold hf) {
    const int CV = C / V, cg = C / G;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    float hw[V][HN > 0 ? HN : 1];
    if constexpr (HN > 0) {
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int o = 0; o < HN; ++o) hw[j][o] = hb.w[(size_t)(cv * V + j) * HN + o];
    }
    // finalisation once per block, cooperatively, through LDS (see k_norm_apply_fused):
    //   st[c][2]  = sum over the accumulator replicas of {sum g, sum g * xhat}
    //   sg[g][2]  = S0, S1 = sum over the statistic's channels of gamma_c * st[c]
    //   cof[c][5] = a, b, c of dx = a * g + b + c * x, and the layer's (scale, shift) for the activation gradient
    extern __shared__ float st[];
    float* sg = st + 2 * C;
    float* cof = sg + 2 * G;
    // EARLY (bf16 tensors, 16-byte vectors, dA a tensor): the first trip's (x, dA) loads are issued ahead of the finalisation and held
    // packed until the coefficients are there -- the streamed data depend on nothing.  Pixels past the block's range are clamped to its
    // last pixel (a valid address: no block has an empty range, see the launcher) and their values discarded.
    constexpr bool EARLY = V == 8 && HN == 0 && std::is_same<TD, bf16_t>::value && std::is_same<TX, bf16_t>::value;
    // (the fp32 instantiations keep the three-stage finalisation for every G: with the one-stage form they spill more)
    constexpr bool ONE_STAGE = std::is_same<TD, bf16_t>::value && std::is_same<TX, bf16_t>::value;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    const size_t rstride = (size_t)gridDim.y * 2 * C;        // sums2[nrep][NS][C][2]
    // everything the one-stage finalisation reads for channel c, issued together (fs, fp: the bias form, block 0 only)
    auto load4 = [&](int c, int r0, float2 (&v)[4]) {         // replicas r0 .. r0 + 3 (clamped to the last: always a valid address)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float2*>(sums2 + min(r0 + q, nrep - 1) * rstride + ((size_t)ns * C + c) * 2);
    };
    auto chan_loads = [&](int c) {
        BwdChanLoads k;
        const size_t nc = (size_t)ns * C + c;
        k.gm = gamma[c]; k.rs = rstd[nc]; k.mu = mean[nc]; k.sc = scale[nc]; k.sh = shift[nc];
        const bool bias = blockIdx.x == 0 && dbias;
        k.fs = bias ? fsums[nc * 2] : 0.f;
        k.fp = bias && fpivot ? fpivot[nc] : 0.f;
        load4(c, 0, k.v);
        return k;
    };
    // The loads of this thread's first channel go out AHEAD of the data loads: loads return in issue order, so the finalisation waits
    // for them alone and runs while the data are still in flight.  (A thread past C loads channel C - 1 and discards it: no branch.)
    BwdChanLoads k0 = {};
    if (ONE_STAGE && cg == 1) k0 = chan_loads(min((int)threadIdx.x, C - 1));
    uint4 xe[EARLY ? 4 : 1], de[EARLY ? 4 : 1];
    if constexpr (EARLY) {                       // (no branch around the loads: a merge would wait for them)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t pix = (size_t)ns * P + min(p0 + pl + u * PL, p1 - 1);
            const size_t off = pix * C + (size_t)cv * V;
            xe[u] = *reinterpret_cast<const uint4*>(x + off);
            de[u] = *reinterpret_cast<const uint4*>(dA + (hb.pw > 0 ? packed_to_hi_pixel(pix, hb.ph, hb.pw) * hb.pc + (size_t)cv * V : off));
        }
    }
    const float inv_m = 1.f / ((float)P * (float)cg);
    // the bias form's closed-form sum (block 0 only), from loads already in registers
    auto publish = [&](int c, float t0, float t1, float ca, float cc, float rs, float mu, float S0, float fs, float fp) {
        atomicAdd(&dbeta[c], t0);
        atomicAdd(&dgamma[c], t1);
        if (dbias) {
            // gradient of the bias the producing convolution adds BEFORE the normalisation (group / instance norm keep it,
            // layers.py:126-132): sum_p dx[ns, p, c] = a * sum g + P * b + c * sum x, in closed form from the per-channel
            // sums of both passes -- no pass over dx.  (sum x - P * mean from the shifted forward sums: no cancellation.)
            const float dsum = fs + (float)P * (fp - mu);
            atomicAdd(&dbias[c], fmaf(ca, t0, fmaf(cc, dsum, -(float)P * rs * S0 * inv_m)));
        }
    };
    if (ONE_STAGE && cg == 1) {
        // batch / instance norm, one channel per statistic: S0, S1 are gamma * st of the SAME channel, so thread c takes channel c from
        // the accumulator replicas to the coefficients on its own -- every per-channel load issued together, one LDS stage, one barrier
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const bool first = c == (int)threadIdx.x;        // this thread's first channel: loaded ahead of the data, above
            BwdChanLoads k = k0;
            if (!first) k = chan_loads(c);
            const float gm = k.gm, rs = k.rs, mu = k.mu, scv = k.sc, shv = k.sh, fs = k.fs, fp = k.fp;
            float t0 = 0.f, t1 = 0.f;
            for (int r0 = 0; r0 < nrep; r0 += 4) {           // four replicas in flight, added in replica order
                if (r0 > 0) load4(c, r0, k.v);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (r0 + q < nrep) { t0 += k.v[q].x; t1 += k.v[q].y; }
            }
            float S0 = 0.f, S1 = 0.f;
            S0 += gm * t0;
            S1 += gm * t1;
            const float ca = rs * gm;
            const float cc = -rs * rs * S1 * inv_m;
            cof[5 * c] = ca;
            cof[5 * c + 1] = -rs * S0 * inv_m - cc * mu;
            cof[5 * c + 2] = cc;
            cof[5 * c + 3] = scv;
            cof[5 * c + 4] = shv;
            if (blockIdx.x == 0) publish(c, t0, t1, ca, cc, rs, mu, S0, fs, fp);
        }
    } else {
        // group norm: the statistic's sums cross channels -- three stages (replica sums, per-group S0 / S1, coefficients)
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
            float a = 0.f;
            for (int r = 0; r < nrep; ++r) a += sums2[r * rstride + (size_t)ns * 2 * C + i];
            st[i] = a;
        }
        __syncthreads();
        for (int g = threadIdx.x; g < G; g += blockDim.x) {
            float S0 = 0.f, S1 = 0.f;
            for (int q = g * cg; q < (g + 1) * cg; ++q) {
                const float gm = gamma[q];
                S0 += gm * st[2 * q];
                S1 += gm * st[2 * q + 1];
            }
            sg[2 * g] = S0;
            sg[2 * g + 1] = S1;
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const int g = c / cg, sgi = ns * G + g;
            const float rs = rstd[sgi], mu = mean[sgi], S0 = sg[2 * g], S1 = sg[2 * g + 1];
            const float ca = rs * gamma[c];
            const float cc = -rs * rs * S1 * inv_m;
            cof[5 * c] = ca;
            cof[5 * c + 1] = -rs * S0 * inv_m - cc * mu;
            cof[5 * c + 2] = cc;
            cof[5 * c + 3] = scale[(size_t)ns * C + c];
            cof[5 * c + 4] = shift[(size_t)ns * C + c];
            if (blockIdx.x == 0)                                 // st[2 c ..]: this channel's {sum g, sum g * xhat}
                publish(c, st[2 * c], st[2 * c + 1], ca, cc, rs, mu, S0, dbias ? fsums[((size_t)ns * C + c) * 2] : 0.f,
                        dbias && fpivot ? fpivot[(size_t)ns * C + c] : 0.f);
        }
    }
    if (hf.acc != nullptr && blockIdx.x == 0 && blockIdx.y == 0) {
        // the head rider of the reduction launch (HeadRider): replicas summed in order, added into the head's filter / bias gradient
        const int nw = C * hf.hr, na = nw + hf.hr;
        for (int i = threadIdx.x; i < na; i += blockDim.x) {
            float a = 0.f;
            for (int r = 0; r < nrep; ++r) a += hf.acc[(size_t)r * na + i];
            atomicAdd(i < nw ? &hf.dw[i] : &hf.db[i - nw], a);
        }
    }
    __syncthreads();
    if (pl >= PL) return;
    float sc[V], sh[V], ca[V], cb[V], cc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float* q = cof + 5 * (cv * V + j);
        ca[j] = q[0]; cb[j] = q[1]; cc[j] = q[2]; sc[j] = q[3]; sh[j] = q[4];
    }
    int p = p0 + pl;
    if constexpr (EARLY) {                       // the first four pixels: loaded ahead of the prologue
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u * PL < p1) {
                float xv[V], dv[V], o[V];
                bf16x8_unpack(xe[u], xv);
                bf16x8_unpack(de[u], dv);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float gq = dv[j] * act_grad_pre(fmaf(xv[j], sc[j], sh[j]), act);
                    o[j] = fmaf(ca[j], gq, fmaf(cc[j], xv[j], cb[j]));
                }
                VecIO<TO, V>::store(dx, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, o);
            }
        }
        p += 4 * PL;
    }
    for (; p + 3 * PL < p1; p += 4 * PL) {       // four pixels per trip, loads first (see k_norm_stats)
        float xv[4][V], dv[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t off = ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V;
            VecIO<TX, V>::load(x, off, xv[u]);
            load_da<TD, V, HN>(dA, off, hb, (size_t)ns * P + p + u * PL, hw, dv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float gq = dv[u][j] * act_grad_pre(fmaf(xv[u][j], sc[j], sh[j]), act);
                o[j] = fmaf(ca[j], gq, fmaf(cc[j], xv[u][j], cb[j]));
            }
            VecIO<TO, V>::store(dx, ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V, o);
        }
    }
    for (; p < p1; p += PL) {
        const size_t off = ((size_t)ns * P + p) * C + (size_t)cv * V;
        float xv[V], dv[V], o[V];
        VecIO<TX, V>::load(x, off, xv);
        load_da<TD, V, HN>(dA, off, hb, (size_t)ns * P + p, hw, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float gq = dv[j] * act_grad_pre(fmaf(xv[j], sc[j], sh[j]), act);
            o[j] = fmaf(ca[j], gq, fmaf(cc[j], xv[j], cb[j]));
        }
        VecIO<TO, V>::store(dx, off, o);
    }
}

// sums2[ns][c][2] += {sum g, sum g*xhat},  g = dA * act'(x*scale+shift), xhat = (x-mean)*rstd
// ACT >= 0 (the rider's launches): the activation is a constant of the instantiation -- no per-element dispatch on `act` in the loops
template <typename TD, typename TX, int V, int HN = 0, int HR = 0, int ACT = -1>
__global__ __launch_bounds__(256, HR == 2 ? 2 : 1) void k_norm_bwd_reduce(const TD* __restrict__ dA, const TX* __restrict__ x,
                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                  float* __restrict__ sums2, int P, int C, int G, int PL, int chunk, int act, int nrep, HeadBw hb,
                                  HeadRider hr) {
    const int CV = C / V;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    float hw[V][HN > 0 ? HN : 1];
    if constexpr (HN > 0) {
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int o = 0; o < HN; ++o) hw[j][o] = hb.w[(size_t)(cv * V + j) * HN + o];
    }
    extern __shared__ float red[];
    // Same-address fp32 atomics retire at ~1 per 45 ns on MI355X (memory-side), so with a thousand blocks the adds into
    // one sums2 entry -- not the streaming -- set the kernel time: block b adds into replica b % nrep, the consumer
    // (k_norm_bwd_apply_fused) sums the replicas.
    sums2 += (size_t)(blockIdx.x % nrep) * gridDim.y * 2 * C;
    const int av = ACT < 0 ? act : ACT;
    float s1[V], s2[V], sc[V], sh[V], mu[V], rs[V];
    float racc[V][HR > 0 ? HR : 1], rb[HR > 0 ? HR : 1];      // the head rider's sums (HR > 0)
    if constexpr (HR > 0) {
#pragma unroll
        for (int o = 0; o < HR; ++o) {
            rb[o] = 0.f;
#pragma unroll
            for (int j = 0; j < V; ++j) racc[j][o] = 0.f;
        }
    }
    const int cg = C / G;
    // per-channel constants through LDS: one load per channel and block instead of one per channel and thread (red is reused
    // for the block reduction below, after the barrier that ends the streaming loop)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        red[4 * c] = scale[(size_t)ns * C + c];
        red[4 * c + 1] = shift[(size_t)ns * C + c];
        red[4 * c + 2] = mean[(size_t)ns * G + c / cg];
        red[4 * c + 3] = rstd[(size_t)ns * G + c / cg];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int c = cv * V + j;
        s1[j] = s2[j] = 0.f;
        sc[j] = red[4 * c]; sh[j] = red[4 * c + 1]; mu[j] = red[4 * c + 2]; rs[j] = red[4 * c + 3];
    }
    __syncthreads();                             // constants read: red is free for the partial sums
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    if (pl < PL) {
        int p = p0 + pl;
        for (; p + 3 * PL < p1; p += 4 * PL) {   // four pixels per trip, loads first (see k_norm_stats)
            float xv[4][V], dv[4][V], hd[4][HR > 0 ? HR : 1];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t off = ((size_t)ns * P + p + u * PL) * C + (size_t)cv * V;
                VecIO<TX, V>::load(x, off, xv[u]);
                if constexpr (HR > 0) load_head_dy<HR>(hr.dy, (size_t)ns * P + p + u * PL, hd[u]);
                if constexpr (HR > 0 && HN > 0) da_from_head<V, HN>(hd[u], hw, dv[u]);      // (the same head: one load of its gradient)
                else load_da<TD, V, HN>(dA, off, hb, (size_t)ns * P + p + u * PL, hw, dv[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float g = dv[u][j] * act_grad_pre(xv[u][j] * sc[j] + sh[j], av);
                    s1[j] += g;
                    s2[j] += g * (xv[u][j] - mu[j]) * rs[j];
                }
                if constexpr (HR > 0) {
                    head_rider_fma<V, HR>(xv[u], sc, sh, av, hd[u], racc);
#pragma unroll
                    for (int o = 0; o < HR; ++o) rb[o] += hd[u][o];
                }
            }
        }
        for (; p < p1; p += PL) {
            float xv[V], dv[V];
            const size_t off = ((size_t)ns * P + p) * C + (size_t)cv * V;
            VecIO<TX, V>::load(x, off, xv);
            float hd[HR > 0 ? HR : 1];
            if constexpr (HR > 0) load_head_dy<HR>(hr.dy, (size_t)ns * P + p, hd);
            if constexpr (HR > 0 && HN > 0) da_from_head<V, HN>(hd, hw, dv);
            else load_da<TD, V, HN>(dA, off, hb, (size_t)ns * P + p, hw, dv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float g = dv[j] * act_grad_pre(xv[j] * sc[j] + sh[j], av);
                s1[j] += g;
                s2[j] += g * (xv[j] - mu[j]) * rs[j];
            }
            if constexpr (HR > 0) {
                head_rider_fma<V, HR>(xv, sc, sh, av, hd, racc);
#pragma unroll
                for (int o = 0; o < HR; ++o) rb[o] += hd[o];
            }
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
        atomicAdd(&sums2[(size_t)ns * 2 * C + i], a);
    }
    if constexpr (HR > 0) {
        // the rider's sums through the same LDS rows, two head outputs per round: red[pl][c][2]
        float* hacc = hr.acc + (size_t)(blockIdx.x % nrep) * (C + 1) * HR;
#pragma unroll
        for (int o0 = 0; o0 < HR; o0 += 2) {
            __syncthreads();
            if (pl < PL) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    red[(pl * C + cv * V + j) * 2 + 0] = racc[j][o0];
                    red[(pl * C + cv * V + j) * 2 + 1] = racc[j][o0 + 1];
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
                float a = 0.f;
                for (int q = 0; q < PL; ++q) a += red[q * 2 * C + i];
                atomicAdd(&hacc[(i >> 1) * HR + o0 + (i & 1)], a);
            }
        }
        __syncthreads();
        if (cv == 0 && pl < PL) {
#pragma unroll
            for (int o = 0; o < HR; ++o) red[pl * HR + o] = rb[o];
        }
        __syncthreads();
        if (threadIdx.x < HR) {
            float a = 0.f;
            for (int q = 0; q < PL; ++q) a += red[q * HR + threadIdx.x];
            atomicAdd(&hacc[C * HR + threadIdx.x], a);
        }
    }
}

// ---- one-pass batch-norm backward (round 6) ------------------------------------------------------------------------------------
// k_norm_bwd_reduce + k_norm_bwd_apply_fused read dA and x twice (two launches, 4 + 6 B per element).  For tensors that fit the
// register file -- up to 256 blocks x 256 threads x NSLOT pixels x 8 channels -- ONE launch reads them once: every thread keeps its
// (dA, x) vectors packed in registers, the block adds its per-channel partial sums into sums2, a GRID BARRIER follows, and the
// gradient is formed from the registers (4 + 2 B per element, one launch).  Batch norm only (one statistic per channel), bf16.
// Grid barrier (cdna_hip_programming.md, Guideline 16): eight arrival shards (block % 8: one per XCD when blocks land round-robin --
// a speed heuristic, never a correctness assumption) and a top word counting finished shards; every word is an agent-scope atomic,
// zeroed before the launch by the caller (the plan's per-step memset); release fence + drained vmcnt before the arrival, one relaxed
// poll loop with s_sleep, one acquire fence after it.  RESIDENCY: the grid is at most 256 blocks (one per CU) of 256 threads with at
// most 256 registers and < 40 KB of LDS, so that TWO such launches -- the engine replays two lanes side by side -- are resident
// together and neither waits for a block the other one keeps off the chip; the spin is bounded and reports through bar[PHX_BAR_TIMEOUT].
#define PHX_BAR_STRIDE 32
#define PHX_BAR_TOP (8 * PHX_BAR_STRIDE)
#define PHX_BAR_TIMEOUT (9 * PHX_BAR_STRIDE)
#define PHX_BAR_WORDS (10 * PHX_BAR_STRIDE)
// PLAIN_STORES: the blocks exchange data written by plain stores (needs the L2 write-back of a release fence, ~1.7 us and more with
// dirty lines); false: everything exchanged went through agent-scope atomics, which are performed at the coherence point already.
template <bool PLAIN_STORES>
__device__ __forceinline__ void phx_grid_barrier(unsigned* __restrict__ bar, int nblocks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every wave: its stores / atomics have left
    __syncthreads();
    if (threadIdx.x == 0) {
        if (PLAIN_STORES) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the fence's own wait: restated)
        }
        unsigned want;
        if (nblocks <= 64) {                                  // few blocks: one level (one atomic round trip less)
            __hip_atomic_fetch_add(bar + PHX_BAR_TOP, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            want = (unsigned)nblocks;
        } else {
            const int shard = blockIdx.x & 7;
            const unsigned nshard = (unsigned)((nblocks - shard + 7) >> 3);
            const unsigned prev = __hip_atomic_fetch_add(bar + shard * PHX_BAR_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev + 1 == nshard) __hip_atomic_fetch_add(bar + PHX_BAR_TOP, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            want = 8u;
        }
        unsigned spins = 0;
        while (__hip_atomic_load(bar + PHX_BAR_TOP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
            __builtin_amdgcn_s_sleep(4);
            if (++spins > (1u << 21)) {                       // ~ seconds: never on a healthy launch; the result is then wrong, not hung
                __hip_atomic_store(bar + PHX_BAR_TIMEOUT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

template <int NSLOT, int ACT>
__global__ __launch_bounds__(256, 2) void k_bn_bwd_onepass(const bf16_t* __restrict__ dA, const bf16_t* __restrict__ x,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, float* __restrict__ sums2,
                                                            unsigned* __restrict__ bar, bf16_t* __restrict__ dx,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta, int P, int C, int PL,
                                                            int chunk, int nrep) {
    constexpr int act = ACT;          // (a run-time activation code makes every element evaluate all three derivatives)
    constexpr int V = 8;
    const int CV = C / V;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    // LDS: keep[C][3] = gamma, mean, rstd of channel c -- written once in the prologue by the thread that turns them into the channel's
    // coefficients after the barrier (in place: no load and no exchange behind the barrier); work = phase 1: [C][2] scale, shift, then
    // [PL][2C] partial sums
    extern __shared__ float red[];
    float* keep = red;
    float* work = red + 3 * C;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    // Every load of the prologue is issued before the first wait -- ONE memory round trip ahead of the sums instead of two (constants,
    // barrier, then data).  The constants go first: loads return in issue order, so the staging below waits for them alone and runs
    // while the slot loads are still in flight.
    const int c0 = threadIdx.x;
    float k0[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < C) { k0[0] = gamma[c0]; k0[1] = mean[c0]; k0[2] = rstd[c0]; k0[3] = scale[c0]; k0[4] = shift[c0]; }
    uint4 xq[NSLOT], dq[NSLOT];                  // (no branch around the loads: a merge would wait for them)
#pragma unroll
    for (int u = 0; u < NSLOT; ++u) {
        const int p = p0 + pl + u * PL;
        const size_t off = (size_t)(p < p1 ? p : p1 - 1) * C + (size_t)cv * V;      // (clamped: always a valid address)
        xq[u] = *reinterpret_cast<const uint4*>(x + off);
        dq[u] = *reinterpret_cast<const uint4*>(dA + off);
    }
    if (c0 < C) {
        keep[3 * c0] = k0[0]; keep[3 * c0 + 1] = k0[1]; keep[3 * c0 + 2] = k0[2];
        work[2 * c0] = k0[3]; work[2 * c0 + 1] = k0[4];
    }
    for (int c = c0 + blockDim.x; c < C; c += blockDim.x) {      // (C > 256 only)
        keep[3 * c] = gamma[c]; keep[3 * c + 1] = mean[c]; keep[3 * c + 2] = rstd[c];
        work[2 * c] = scale[c]; work[2 * c + 1] = shift[c];
    }
    __syncthreads();
    float sc[V], sh[V], mu[V], rs[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int c = cv * V + j;
        sc[j] = work[2 * c]; sh[j] = work[2 * c + 1]; mu[j] = keep[3 * c + 1]; rs[j] = keep[3 * c + 2];
    }
    __syncthreads();                             // constants read: work is free for the partial sums
    if (pl < PL) {
        float s1[V], s2[V];
#pragma unroll
        for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
        for (int u = 0; u < NSLOT; ++u) {
            if (p0 + pl + u * PL >= p1) dq[u] = make_uint4(0u, 0u, 0u, 0u);              // dA = 0: contributes nothing
            const unsigned xw[4] = {xq[u].x, xq[u].y, xq[u].z, xq[u].w}, dw[4] = {dq[u].x, dq[u].y, dq[u].z, dq[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x0 = __uint_as_float(xw[k] << 16), x1 = __uint_as_float(xw[k] & 0xffff0000u);
                const float d0 = __uint_as_float(dw[k] << 16), d1 = __uint_as_float(dw[k] & 0xffff0000u);
                const float g0 = d0 * act_grad_pre(x0 * sc[2 * k] + sh[2 * k], act);
                const float g1 = d1 * act_grad_pre(x1 * sc[2 * k + 1] + sh[2 * k + 1], act);
                s1[2 * k] += g0;
                s2[2 * k] += g0 * (x0 - mu[2 * k]) * rs[2 * k];
                s1[2 * k + 1] += g1;
                s2[2 * k + 1] += g1 * (x1 - mu[2 * k + 1]) * rs[2 * k + 1];
            }
            __builtin_amdgcn_sched_barrier(0);           // slot by slot: the unpacked values of one slot are dead before the next is opened
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            work[(pl * C + cv * V + j) * 2 + 0] = s1[j];
            work[(pl * C + cv * V + j) * 2 + 1] = s2[j];
        }
    }
    __syncthreads();
    float* srep = sums2 + (size_t)(blockIdx.x % nrep) * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
        float a = 0.f;
        for (int q = 0; q < PL; ++q) a += work[q * 2 * C + i];
        atomicAdd(&srep[i], a);
    }
    phx_grid_barrier<false>(bar, gridDim.x);      // (the only exchanged data are the atomically added sums)
    // (the packed registers are opaque from here on: otherwise the compiler keeps phase 1's unpacked x and g values alive across the
    // barrier -- 16 floats per slot instead of 8 packed registers -- and spills)
#pragma unroll
    for (int u = 0; u < NSLOT; ++u)
        asm volatile("" : "+v"(xq[u].x), "+v"(xq[u].y), "+v"(xq[u].z), "+v"(xq[u].w), "+v"(dq[u].x), "+v"(dq[u].y), "+v"(dq[u].z), "+v"(dq[u].w));
    // every block finalises for itself (k_norm_bwd_apply_fused's arithmetic, one statistic per channel: S0 = gamma t0, S1 = gamma t1):
    // thread c reads the replicas of ITS channel's two sums -- four at a time in flight, added in replica order -- and turns keep[c]
    // into the channel's coefficients in place: one round trip and one LDS stage behind the barrier
    float* cof = keep;
    const float inv_m = 1.f / (float)P;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float t0 = 0.f, t1 = 0.f;
        for (int r0 = 0; r0 < nrep; r0 += 4) {
            float v0[4], v1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* q = sums2 + (size_t)min(r0 + k, nrep - 1) * 2 * C + 2 * c;
                v0[k] = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v1[k] = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r0 + k < nrep) { t0 += v0[k]; t1 += v1[k]; }
        }
        const float gm = keep[3 * c], m_ = keep[3 * c + 1], r_ = keep[3 * c + 2];
        const float S0 = gm * t0, S1 = gm * t1;
        const float ca = r_ * gm;
        const float cc = -r_ * r_ * S1 * inv_m;
        cof[3 * c] = ca;
        cof[3 * c + 1] = -r_ * S0 * inv_m - cc * m_;
        cof[3 * c + 2] = cc;
        if (blockIdx.x == 0) {
            atomicAdd(&dbeta[c], t0);
            atomicAdd(&dgamma[c], t1);
        }
    }
    __syncthreads();
    if (pl >= PL) return;
    float ca[V], cb[V], cc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float* q = cof + 3 * (cv * V + j);
        ca[j] = q[0]; cb[j] = q[1]; cc[j] = q[2];
    }
#pragma unroll
    for (int u = 0; u < NSLOT; ++u) {
        const int p = p0 + pl + u * PL;
        if (p < p1) {
            const unsigned xw[4] = {xq[u].x, xq[u].y, xq[u].z, xq[u].w}, dw[4] = {dq[u].x, dq[u].y, dq[u].z, dq[u].w};
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x0 = __uint_as_float(xw[k] << 16), x1 = __uint_as_float(xw[k] & 0xffff0000u);
                const float d0 = __uint_as_float(dw[k] << 16), d1 = __uint_as_float(dw[k] & 0xffff0000u);
                const float g0 = d0 * act_grad_pre(fmaf(x0, sc[2 * k], sh[2 * k]), act);
                const float g1 = d1 * act_grad_pre(fmaf(x1, sc[2 * k + 1], sh[2 * k + 1]), act);
                o[k] = f2bf_pk(fmaf(ca[2 * k], g0, fmaf(cc[2 * k], x0, cb[2 * k])), fmaf(ca[2 * k + 1], g1, fmaf(cc[2 * k + 1], x1, cb[2 * k + 1])));
            }
            *reinterpret_cast<uint4*>(dx + (size_t)p * C + (size_t)cv * V) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ void k_norm_bwd_finalize(const float* __restrict__ sums2, const float* __restrict__ gamma, float* S,
                                    float* dgamma, float* dbeta, int NS, int C, int G) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int cg = C / G;
    if (idx < NS * G) {
        const int ns = idx / G, g = idx % G;
        float a = 0.f, b = 0.f;
        for (int c = g * cg; c < (g + 1) * cg; ++c) {
            a += gamma[c] * sums2[((size_t)ns * C + c) * 2];
            b += gamma[c] * sums2[((size_t)ns * C + c) * 2 + 1];
        }
        S[idx * 2] = a;
        S[idx * 2 + 1] = b;
    }
    if (idx < C) {
        float a = 0.f, b = 0.f;
        for (int ns = 0; ns < NS; ++ns) {
            a += sums2[((size_t)ns * C + idx) * 2];
            b += sums2[((size_t)ns * C + idx) * 2 + 1];
        }
        dbeta[idx] += a;
        dgamma[idx] += b;
    }
}

// dx = rstd*(gamma*g - S0/m - xhat*S1/m) folded to dx = a*g + b + c*x with per-(ns, channel) coefficients in
// registers:  a = rstd*gamma,  c = -rstd^2*S1/m,  b = -rstd*S0/m - c*mean;  g = dA * act'(x*scale+shift).
template <typename TD, typename TX, typename TO, int V>
__global__ void k_norm_bwd_apply(const TD* __restrict__ dA, const TX* __restrict__ x,
                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                 const float* __restrict__ gamma, const float* __restrict__ S, TO* __restrict__ dx,
                                 int P, int C, int G, int PL, int chunk, int act) {
    const int CV = C / V, cg = C / G;
    const int ns = blockIdx.y;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    if (pl >= PL) return;
    const float inv_m = 1.f / ((float)P * (float)cg);
    float sc[V], sh[V], ca[V], cb[V], cc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int c = cv * V + j;
        const int sg = ns * G + c / cg;
        const float rs = rstd[sg], mu = mean[sg];
        sc[j] = scale[(size_t)ns * C + c];
        sh[j] = shift[(size_t)ns * C + c];
        ca[j] = rs * gamma[c];
        cc[j] = -rs * rs * S[sg * 2 + 1] * inv_m;
        cb[j] = -rs * S[sg * 2] * inv_m - cc[j] * mu;
    }
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    for (int p = p0 + pl; p < p1; p += PL) {
        const size_t off = ((size_t)ns * P + p) * C + (size_t)cv * V;
        float xv[V], dv[V], o[V];
        VecIO<TX, V>::load(x, off, xv);
        VecIO<TD, V>::load(dA, off, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float g = dv[j] * act_grad_pre(fmaf(xv[j], sc[j], sh[j]), act);
            o[j] = fmaf(ca[j], g, fmaf(cc[j], xv[j], cb[j]));
        }
        VecIO<TO, V>::store(dx, off, o);
    }
}

extern "C" {

// ---- the reduce + apply pair: ONE host launcher per kernel template; the entry points below validate their own arguments ----------
// hn: outputs of the head dA is derived from (0: dA is a tensor); hrn: outputs of the riding head (0: none).  hn > 0 or hrn > 0: bf16
// tensors and C % 8 == 0, checked by the entry point.  e_large / who_large: code and message of "C too large" (the rider forms answer
// PHX_E_INVAL where the others answer PHX_E_SHAPE); it is raised behind the dtype dispatch, where every entry point had it.
static int norm_bwd_reduce_launch(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, float* sums2, int NS, int P, int C, int G, int act, int nrep,
                                  HeadBw hb, int hn, HeadRider hr, int hrn, int e_large, const char* who_large, void* stream) {
    int PL = 0, threads = 0, chunk = 0, nchunks = 0;
    const int too_large = norm_geometry(P, C, C % 8 == 0 ? 8 : 1, &PL, &threads, &chunk, &nchunks, NS, nrep);
    if (phx_deterministic() && nchunks > nrep) {               // block b owns replica b: one add per accumulator, the consumer
        chunk = (P + nrep - 1) / nrep;                         // sums the replicas in a fixed order
        nchunks = (P + chunk - 1) / chunk;
    }
    const size_t lds = (size_t)(PL > 2 ? PL : 2) * C * 2 * sizeof(float);
#define NBR_LAUNCH(TD, TX, Vv, HNv, HRv, ACTv)                                                                                    \
    do {                                                                                                                          \
        PHX_REQUIRE(too_large == 0, e_large, who_large);                                                                          \
        hipLaunchKernelGGL((k_norm_bwd_reduce<TD, TX, Vv, HNv, HRv, ACTv>), dim3(nchunks, NS), dim3(threads), lds, (hipStream_t)stream, \
                           (const TD*)dA, (const TX*)x, scale, shift, mean, rstd, sums2, P, C, G, PL, chunk, act, nrep, hb, hr);   \
    } while (0)
#define NBR_LAUNCH_ACT(HNv)                          /* the activation a constant of the instantiation (ACT >= 0) */               \
    do {                                                                                                                          \
        if (act == PHX_ACT_RELU) NBR_LAUNCH(bf16_t, bf16_t, 8, HNv, HNv, PHX_ACT_RELU);                                           \
        else if (act == PHX_ACT_ID) NBR_LAUNCH(bf16_t, bf16_t, 8, HNv, HNv, PHX_ACT_ID);                                          \
        else NBR_LAUNCH(bf16_t, bf16_t, 8, HNv, HNv, -1);                                                                         \
    } while (0)
    if (hn == 0 && hrn == 0) PHX_DT_SWITCH(da_dt, TD, PHX_DT_SWITCH(x_dt, TX, PHX_VEC_SWITCH(C, V, NBR_LAUNCH(TD, TX, V, 0, 0, -1))));
    else if (hrn == 0) { if (hn == 2) NBR_LAUNCH(bf16_t, bf16_t, 8, 2, 0, -1); else NBR_LAUNCH(bf16_t, bf16_t, 8, 4, 0, -1); }
    // (dA a tensor: the specialised copies need more registers than two waves per SIMD leave -- the run-time dispatch stays)
    else if (hn == 0) { if (hrn == 2) NBR_LAUNCH(bf16_t, bf16_t, 8, 0, 2, -1); else NBR_LAUNCH(bf16_t, bf16_t, 8, 0, 4, -1); }
    else if (hn == 2) NBR_LAUNCH_ACT(2);
    else NBR_LAUNCH_ACT(4);
#undef NBR_LAUNCH_ACT
#undef NBR_LAUNCH
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
static int norm_bwd_apply_launch(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, const float* gamma, const float* sums2, void* dx,
                                 float* dgamma, float* dbeta, const float* fwd_sums, const float* fwd_pivot, float* dbias, int NS,
                                 int P, int C, int G, int act, int nrep, HeadBw hb, int hn, HeadFold hf, int e_large,
                                 const char* who_large, void* stream) {
    int PL = 0, threads = 0, chunk = 0, nchunks = 0;
    const int too_large = stream_geometry(P, C, C % 8 == 0 ? 8 : 1, &PL, &threads, &chunk, &nchunks, NS);
    const size_t lds = (size_t)(7 * C + 2 * G) * sizeof(float);
#define NBA_LAUNCH(TD, TX, Vv, HNv)                                                                                               \
    do {                                                                                                                          \
        PHX_REQUIRE(too_large == 0, e_large, who_large);                                                                          \
        PHX_REQUIRE(block_ranges_nonempty(P, chunk, nchunks), PHX_E_SHAPE, "norm_bwd_apply_fused: a block without pixels");       \
        hipLaunchKernelGGL((k_norm_bwd_apply_fused<TD, TX, TD, Vv, HNv>), dim3(nchunks, NS), dim3(threads), lds, (hipStream_t)stream, \
                           (const TD*)dA, (const TX*)x, scale, shift, mean, rstd, gamma, sums2, (TD*)dx, dgamma, dbeta, P, C, G,   \
                           PL, chunk, act, nrep, fwd_sums, fwd_pivot, dbias, hb, hf);                                             \
    } while (0)
    if (hn == 2) NBA_LAUNCH(bf16_t, bf16_t, 8, 2);
    else if (hn > 0) NBA_LAUNCH(bf16_t, bf16_t, 8, 4);
    else PHX_DT_SWITCH(da_dt, TD, PHX_DT_SWITCH(x_dt, TX, PHX_VEC_SWITCH(C, V, NBA_LAUNCH(TD, TX, V, 0))));
#undef NBA_LAUNCH
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_bwd_reduce(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                        const float* mean, const float* rstd, float* sums2, int NS, int P, int C, int G, int act,
                        int nrep, void* stream) {
    PHX_REQUIRE(nrep >= 1, PHX_E_INVAL, "norm_bwd_reduce: nrep >= 1");
    return norm_bwd_reduce_launch(dA, da_dt, x, x_dt, scale, shift, mean, rstd, sums2, NS, P, C, G, act, nrep, HeadBw{nullptr, nullptr, 0, 0, C},
                                  0, HeadRider{nullptr, nullptr}, 0, PHX_E_SHAPE, "norm_bwd_reduce: C too large", stream);
}
int phx_norm_bwd_reduce_s2d(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                            const float* mean, const float* rstd, float* sums2, int NS, int P, int C, int G, int act, int nrep, int h,
                            int w, void* stream) {
    PHX_REQUIRE(h > 0 && w > 0 && ((size_t)NS * P) % ((size_t)4 * h * w) == 0 && (NS == 1 || P == 4 * h * w), PHX_E_SHAPE,
                "norm_bwd_reduce_s2d: NS * P = images x 4 h w, a sample group = one image or all of them");
    PHX_REQUIRE(nrep >= 1, PHX_E_INVAL, "norm_bwd_reduce: nrep >= 1");
    return norm_bwd_reduce_launch(dA, da_dt, x, x_dt, scale, shift, mean, rstd, sums2, NS, P, C, G, act, nrep, HeadBw{nullptr, nullptr, h, w, C},
                                  0, HeadRider{nullptr, nullptr}, 0, PHX_E_SHAPE, "norm_bwd_reduce: C too large", stream);
}

// dx's side of the generic entry points (ph, pw > 0: the phase-form convolution's layer)
static int norm_bwd_apply_generic(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, const float* gamma, const float* sums2, void* dx,
                                  int dx_dt, float* dgamma, float* dbeta, const float* fwd_sums, const float* fwd_pivot,
                                  float* dbias, int NS, int P, int C, int G, int act, int nrep, int ph, int pw, void* stream) {
    PHX_REQUIRE(da_dt == dx_dt, PHX_E_INVAL, "norm_bwd_apply_fused: dA and dx dtypes must match");
    PHX_REQUIRE(dbias == nullptr || fwd_sums != nullptr, PHX_E_INVAL, "norm_bwd_apply_fused_bias: dbias needs the forward sums");
    PHX_REQUIRE(nrep >= 1, PHX_E_INVAL, "norm_bwd_apply_fused: nrep >= 1");
    return norm_bwd_apply_launch(dA, da_dt, x, x_dt, scale, shift, mean, rstd, gamma, sums2, dx, dgamma, dbeta, fwd_sums, fwd_pivot, dbias,
                                 NS, P, C, G, act, nrep, HeadBw{nullptr, nullptr, ph, pw, C}, 0, HeadFold{nullptr, nullptr, nullptr, 0},
                                 PHX_E_SHAPE, "norm_bwd_apply_fused: C too large", stream);
}
int phx_norm_bwd_apply_fused(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                             const float* mean, const float* rstd, const float* gamma, const float* sums2, void* dx,
                             int dx_dt, float* dgamma, float* dbeta, int NS, int P, int C, int G, int act, int nrep,
                             void* stream) {
    return phx_norm_bwd_apply_fused_bias(dA, da_dt, x, x_dt, scale, shift, mean, rstd, gamma, sums2, dx, dx_dt, dgamma, dbeta,
                                         nullptr, nullptr, nullptr, NS, P, C, G, act, nrep, stream);
}
int phx_norm_bwd_apply_fused_bias(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, const float* gamma, const float* sums2, void* dx,
                                  int dx_dt, float* dgamma, float* dbeta, const float* fwd_sums, const float* fwd_pivot,
                                  float* dbias, int NS, int P, int C, int G, int act, int nrep, void* stream) {
    return norm_bwd_apply_generic(dA, da_dt, x, x_dt, scale, shift, mean, rstd, gamma, sums2, dx, dx_dt, dgamma, dbeta, fwd_sums, fwd_pivot,
                                  dbias, NS, P, C, G, act, nrep, 0, 0, stream);
}
/* the phase-form convolution's layer: dA is the hi-res map, x and dx are in the packed pixel order (fwd_sums / fwd_pivot / dbias as
 * phx_norm_bwd_apply_fused_bias) */
int phx_norm_bwd_apply_fused_s2d(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, const float* gamma, const float* sums2, void* dx, int dx_dt,
                                 float* dgamma, float* dbeta, const float* fwd_sums, const float* fwd_pivot, float* dbias, int NS, int P,
                                 int C, int G, int act, int nrep, int h, int w, void* stream) {
    PHX_REQUIRE(h > 0 && w > 0 && ((size_t)NS * P) % ((size_t)4 * h * w) == 0 && (NS == 1 || P == 4 * h * w), PHX_E_SHAPE,
                "norm_bwd_apply_fused_s2d: NS * P = images x 4 h w, a sample group = one image or all of them");
    return norm_bwd_apply_generic(dA, da_dt, x, x_dt, scale, shift, mean, rstd, gamma, sums2, dx, dx_dt, dgamma, dbeta, fwd_sums, fwd_pivot,
                                  dbias, NS, P, C, G, act, nrep, h, w, stream);
}
/* backward of a normalisation layer whose only reader is a 1x1 head (phx_norm_apply_fused_head): the upstream gradient is
 * dA = dy_head w_head^T (rounded to bf16), formed on the fly from dy_head [NS * P][nout] -- the head's data-gradient launch, its
 * [NS * P][C] output and the two reads of it disappear.  bf16 tensors, C % 8 == 0, nout in {2, 4}. */
int phx_norm_bwd_reduce_head(const float* dy_head, const float* w_head, int nout, const void* x, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* sums2, int NS, int P, int C, int G, int act, int nrep,
                             void* stream) {
    PHX_REQUIRE(dy_head && w_head && (nout == 2 || nout == 4) && C % 8 == 0 && nrep >= 1, PHX_E_INVAL, "norm_bwd_reduce_head: bad arguments");
    return norm_bwd_reduce_launch(nullptr, PHX_BF16, x, PHX_BF16, scale, shift, mean, rstd, sums2, NS, P, C, G, act, nrep, HeadBw{dy_head, w_head},
                                  nout, HeadRider{nullptr, nullptr}, 0, PHX_E_SHAPE, "norm_bwd_reduce_head: C too large", stream);
}
int phx_norm_bwd_apply_fused_head(const float* dy_head, const float* w_head, int nout, const void* x, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, const float* gamma, const float* sums2,
                                  void* dx, float* dgamma, float* dbeta, const float* fwd_sums, const float* fwd_pivot, float* dbias,
                                  int NS, int P, int C, int G, int act, int nrep, void* stream) {
    PHX_REQUIRE(dy_head && w_head && (nout == 2 || nout == 4) && C % 8 == 0 && nrep >= 1, PHX_E_INVAL, "norm_bwd_apply_fused_head: bad arguments");
    PHX_REQUIRE(dbias == nullptr || fwd_sums != nullptr, PHX_E_INVAL, "norm_bwd_apply_fused_head: dbias needs the forward sums");
    return norm_bwd_apply_launch(nullptr, PHX_BF16, x, PHX_BF16, scale, shift, mean, rstd, gamma, sums2, dx, dgamma, dbeta, fwd_sums, fwd_pivot,
                                 dbias, NS, P, C, G, act, nrep, HeadBw{dy_head, w_head}, nout, HeadFold{nullptr, nullptr, nullptr, 0},
                                 PHX_E_SHAPE, "norm_bwd_apply_fused_head: C too large", stream);
}

/* The reduce + apply pair of a BATCH-norm layer (one statistic per channel, bf16 tensors) with the filter / bias gradient of a 1x1 head
 * that reads the layer's activation riding on it (HeadRider / HeadFold above): phx_norm_head_supported's domain, everything else is
 * PHX_E_INVAL.  dA == NULL: the head is the layer's only reader and dA = dy_head w_head^T is formed on the fly (the _head entry points'
 * arithmetic); else dA is the tensor and w_head is not read. */
static int norm_rider_check(const void* x, const float* dy_head, const float* w_head, const void* dA, int nout, const float* hacc, int P,
                            int C, int nrep, const char* who) {
    PHX_REQUIRE(x && dy_head && hacc && (dA || w_head) && P >= 1 && nrep >= 1, PHX_E_INVAL, who);
    PHX_REQUIRE(C >= 8 && phx_norm_head_supported(C, nout, PHX_BF16, PHX_BF16), PHX_E_INVAL, who);
    return PHX_OK;
}
int phx_norm_bwd_reduce_rider(const void* dA, const float* dy_head, const float* w_head, int nout, const void* x, const float* scale,
                              const float* shift, const float* mean, const float* rstd, float* sums2, float* head_acc, int P, int C,
                              int act, int nrep, void* stream) {
    if (int rc = norm_rider_check(x, dy_head, w_head, dA, nout, head_acc, P, C, nrep,
                                  "norm_bwd_reduce_rider: bf16, C / 8 a power of two <= 64, nout in {2, 4}, non-null arguments")) return rc;
    return norm_bwd_reduce_launch(dA, PHX_BF16, x, PHX_BF16, scale, shift, mean, rstd, sums2, 1, P, C, C, act, nrep, HeadBw{dy_head, w_head, 0, 0, C},
                                  dA ? 0 : nout, HeadRider{dy_head, head_acc}, nout, PHX_E_INVAL, "norm_bwd_reduce_rider: C too large", stream);
}
int phx_norm_bwd_apply_fused_rider(const void* dA, const float* dy_head, const float* w_head, int nout, const void* x, const float* scale,
                                   const float* shift, const float* mean, const float* rstd, const float* gamma, const float* sums2,
                                   void* dx, float* dgamma, float* dbeta, const float* head_acc, float* dw_head, float* db_head, int P,
                                   int C, int act, int nrep, void* stream) {
    if (int rc = norm_rider_check(x, dy_head, w_head, dA, nout, head_acc, P, C, nrep,
                                  "norm_bwd_apply_fused_rider: bf16, C / 8 a power of two <= 64, nout in {2, 4}, non-null arguments")) return rc;
    PHX_REQUIRE(dx && dw_head && db_head, PHX_E_INVAL, "norm_bwd_apply_fused_rider: null output");
    return norm_bwd_apply_launch(dA, PHX_BF16, x, PHX_BF16, scale, shift, mean, rstd, gamma, sums2, dx, dgamma, dbeta, nullptr, nullptr, nullptr,
                                 1, P, C, C, act, nrep, HeadBw{dy_head, w_head, 0, 0, C}, dA ? 0 : nout, HeadFold{head_acc, dw_head, db_head, nout},
                                 PHX_E_INVAL, "norm_bwd_apply_fused_rider: C too large", stream);
}

// one-pass batch-norm backward: geometry (at most 256 blocks of <= 256 threads; slots = pixels per thread)
static bool bn_onepass_geometry(int P, int C, int* PL, int* threads, int* chunk, int* nblocks, int* nslot) {
    if (C % 8 != 0 || C / 8 > 256 || P < 1) return false;
    const int CV = C / 8;
    *PL = 256 / CV;
    *threads = CV * (*PL);
    int want = (P + (*PL) * 8 - 1) / ((*PL) * 8);            // ~8 pixels per thread ...
    if (want > 256) want = 256;                               // ... on at most one block per CU
    if (want < 1) want = 1;
    *chunk = (P + want - 1) / want;
    *nblocks = (P + *chunk - 1) / (*chunk);
    const int slots = (*chunk + *PL - 1) / (*PL);
    *nslot = slots <= 4 ? 4 : slots <= 8 ? 8 : slots <= 16 ? 16 : 0;
    return *nslot != 0 && (size_t)(*PL) * C * 2 * sizeof(float) <= 40 * 1024 && (size_t)5 * C * sizeof(float) <= 40 * 1024;
}
int phx_bn_bwd_onepass_supported(int P, int C, int act) {
    int PL, threads, chunk, nblocks, nslot;
    return (act == PHX_ACT_RELU && !phx_deterministic()
            && bn_onepass_geometry(P, C, &PL, &threads, &chunk, &nblocks, &nslot)) ? 1 : 0;
}
int phx_bn_bwd_onepass_barrier_words(void) { return PHX_BAR_WORDS; }
int phx_bn_bwd_onepass(const void* dA, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                       const float* gamma, float* sums2, unsigned* barrier, void* dx, float* dgamma, float* dbeta, int P, int C, int act,
                       int nrep, void* stream) {
    int PL, threads, chunk, nblocks, nslot;
    PHX_REQUIRE(dA && x && sums2 && barrier && dx && nrep >= 1, PHX_E_INVAL, "bn_bwd_onepass: null pointer");
    PHX_REQUIRE(bn_onepass_geometry(P, C, &PL, &threads, &chunk, &nblocks, &nslot), PHX_E_SHAPE,
                "bn_bwd_onepass: the tensor does not fit 256 blocks x 16 pixels per thread (phx_bn_bwd_onepass_supported)");
    const size_t lds = (size_t)(3 + 2 * PL) * C * sizeof(float);       // keep[C][3] + max([C][2], [PL][2C]), PL >= 1
    PHX_REQUIRE(lds <= 40 * 1024 && (size_t)(nblocks - 1) * chunk < (size_t)P, PHX_E_SHAPE, "bn_bwd_onepass: LDS above 40 KB or an empty block");
#define PHX_ONEPASS(NS_, ACT_)                                                                                                      \
    hipLaunchKernelGGL((k_bn_bwd_onepass<NS_, ACT_>), dim3(nblocks), dim3(threads), lds, (hipStream_t)stream, (const bf16_t*)dA,     \
                       (const bf16_t*)x, scale, shift, mean, rstd, gamma, sums2, barrier, (bf16_t*)dx, dgamma, dbeta, P, C, PL, chunk, nrep)
    PHX_REQUIRE(act == PHX_ACT_RELU, PHX_E_INVAL, "bn_bwd_onepass: relu layers only (every conv + batch norm of the zoo)");
    if (nslot == 4) PHX_ONEPASS(4, PHX_ACT_RELU); else if (nslot == 8) PHX_ONEPASS(8, PHX_ACT_RELU); else PHX_ONEPASS(16, PHX_ACT_RELU);
#undef PHX_ONEPASS
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_bwd_finalize(const float* sums2, const float* gamma, float* S, float* dgamma, float* dbeta, int NS, int C,
                          int G, void* stream) {
    const int n = NS * G > C ? NS * G : C;
    hipLaunchKernelGGL(k_norm_bwd_finalize, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, sums2, gamma, S,
                       dgamma, dbeta, NS, C, G);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_norm_bwd_apply(const void* dA, int da_dt, const void* x, int x_dt, const float* scale, const float* shift,
                       const float* mean, const float* rstd, const float* gamma, const float* S, void* dx, int dx_dt,
                       int NS, int P, int C, int G, int act, void* stream) {
    PHX_REQUIRE(da_dt == dx_dt, PHX_E_INVAL, "norm_bwd_apply: dA and dx dtypes must match");
    PHX_DT_SWITCH(da_dt, TD, PHX_DT_SWITCH(x_dt, TX, PHX_VEC_SWITCH(C, V, {
        int PL, threads, chunk, nchunks;
        PHX_REQUIRE(stream_geometry(P, C, V, &PL, &threads, &chunk, &nchunks, NS) == 0, PHX_E_SHAPE, "norm_bwd_apply: C too large");
        hipLaunchKernelGGL((k_norm_bwd_apply<TD, TX, TD, V>), dim3(nchunks, NS), dim3(threads), 0,
                           (hipStream_t)stream, (const TD*)dA, (const TX*)x, scale, shift, mean, rstd, gamma, S, (TD*)dx,
                           P, C, G, PL, chunk, act);
    })));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
