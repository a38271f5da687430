// The 2-D layers with explicit geometry: VALID (or SAME) padding for conv2D / dilated_conv2D / transposed_conv2D, any legal
// output_shape of tf.nn.conv2d_transpose, and max / average pooling with any window, stride and padding (tfwrapper/layers.py:18-54,
// 94-145, 197-258, 378-425).  NHWC activations (fp32 or bf16 through ldf / stf), fp32 filters, fp32 accumulation, no floating-point
// atomics: every reduction has a fixed order, so repeats are bit-identical in every mode.
//
// The design is that of conv3d.hip reduced to two dimensions, with the geometry handed in instead of derived.  A "big" tensor
// [B, Hb, Wb, Ca] and a "small" one [B, Hs, Ws, Cb] are tied by  big index = small index * s + tap * d - pad  through a filter
// [kh][kw][Ca][Cb]:
//     convolution             fwd = DOWN (big -> small), dgrad = UP (small -> big),  filter HWIO = [..][Cin][Cout]
//     transposed convolution  fwd = UP   (small -> big), dgrad = DOWN,               filter HWOI = [..][Cout][Cin]
// The host passes pt / pl, the strides, the dilations and both extents (phx_conv2d_geometry has TF's rule); the kernels compute no
// padding rule of their own and test every index they form against the extents, so any geometry is memory-safe.
//
// Fast path of DOWN and UP (reduction channels % 4 == 0 in fp32, % 8 == 0 in bf16; any stride, any dilation): a thread keeps 8 output
// channels of 4 pixels along W in registers, reads the reduction channels in 16-byte vectors, and takes the filter from LDS, staged per
// block in slices [tap][8 reduction channels][output channels padded to 8].  A 16-lane group of a ds_read_b128 then reads consecutive
// 32-byte pieces of one 256-byte bank row: conflict-free up to 64 output channels, two-way beyond.  Any other channel count takes the
// scalar kernels (one thread per output element): correct, not fast.
//
// Filter gradient dw[tap][a][b] += sum over small pixels of big[.., a] small[.., b], one kernel for both layers, in two stages: the
// small pixels are cut into contiguous chunks; a block owns (chunk, tap, 32 x 32 channel tile), stages 32 pixels of both operands in
// LDS at a time and keeps a 4 x 4 register tile per thread (four pixel groups of 64 threads, summed through LDS in a fixed order); the
// chunk sums go to a workspace and a second launch adds them to dw in chunk order.  With one chunk the first stage adds to dw itself.
#include "phx_common.h"

namespace {

struct P2 {
    int B, Hb, Wb, Ca, Hs, Ws, Cb, kh, kw, sh, sw, dh, dw, pt, pl;
};

constexpr int P2_VPT = 4;          // pixels along W per thread
constexpr int P2_CPT = 8;          // output channels per thread
constexpr int P2_RK = 8;           // reduction channels per staged slice
constexpr int P2_LDS = 8192;       // floats of filter staging (32 KiB)

// 8 consecutive channels of `p` at element offset `o` (o * sizeof(T) is a multiple of 16); `second`: channels 4..7 exist (fp32)
template <typename T> __device__ __forceinline__ void p2_ld8(const T* p, size_t o, bool second, float* v);
template <> __device__ __forceinline__ void p2_ld8<float>(const float* p, size_t o, bool second, float* v) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + o);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    if (second) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p + o + 4);
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
        v[4] = v[5] = v[6] = v[7] = 0.f;
    }
}
template <> __device__ __forceinline__ void p2_ld8<bf16_t>(const bf16_t* p, size_t o, bool, float* v) {
    const uint4 a = *reinterpret_cast<const uint4*>(p + o);
    const unsigned u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = __uint_as_float(u[k] << 16);
        v[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
    }
}

// UP = false: out = small [.., Cb], reduce over Ca of big.  UP = true: out = big [.., Ca], reduce over Cb of small.
template <typename TI, typename TO, bool UP>
__global__ __launch_bounds__(256) void k_p2_vec(const TI* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                TO* __restrict__ out, P2 g, int act) {
    __shared__ __attribute__((aligned(16))) float wl[P2_LDS];
    const int Cr = UP ? g.Cb : g.Ca, Cq = UP ? g.Ca : g.Cb;
    const int Hi = UP ? g.Hs : g.Hb, Wi = UP ? g.Ws : g.Wb;
    const int Ho = UP ? g.Hb : g.Hs, Wo = UP ? g.Wb : g.Ws;
    const int ncg = (Cq + P2_CPT - 1) / P2_CPT, cqp = ncg * P2_CPT;
    const int nxg = (Wo + P2_VPT - 1) / P2_VPT;
    const int ntap = g.kh * g.kw;
    const int tk = min(ntap, P2_LDS / (P2_RK * cqp));                       // taps per staged slice (>= 1: checked by the host)
    const size_t nitem = (size_t)g.B * Ho * nxg * ncg;
    const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = item < nitem;
    const int cg = (int)(item % ncg);
    size_t r = item / ncg;
    const int x0 = (int)(r % nxg) * P2_VPT; r /= nxg;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);

    float acc[P2_VPT][P2_CPT];
#pragma unroll
    for (int v = 0; v < P2_VPT; ++v)
#pragma unroll
        for (int c = 0; c < P2_CPT; ++c) acc[v][c] = 0.f;

    for (int r0 = 0; r0 < Cr; r0 += P2_RK) {
        const bool second = r0 + 4 < Cr;
        for (int t0 = 0; t0 < ntap; t0 += tk) {
            const int nt = min(tk, ntap - t0);
            __syncthreads();
            for (int e = threadIdx.x; e < nt * P2_RK * cqp; e += 256) {
                int q, j, tl;
                if (!UP) { q = e % cqp; j = (e / cqp) % P2_RK; tl = e / (cqp * P2_RK); }      // global reads contiguous along Cb
                else { j = e % P2_RK; q = (e / P2_RK) % cqp; tl = e / (cqp * P2_RK); }
                const int rr = r0 + j;
                float val = 0.f;
                if (q < Cq && rr < Cr) {
                    const size_t a = UP ? (size_t)q : (size_t)rr, bb = UP ? (size_t)rr : (size_t)q;
                    val = w[((size_t)(t0 + tl) * g.Ca + a) * g.Cb + bb];
                }
                wl[(tl * P2_RK + j) * cqp + q] = val;
            }
            __syncthreads();
            if (!live) continue;
            for (int tl = 0; tl < nt; ++tl) {
                const int tap = t0 + tl;
                const int kx = tap % g.kw, ky = tap / g.kw;
                int iy;
                if (!UP) {
                    iy = oy * g.sh + ky * g.dh - g.pt;
                    if (iy < 0 || iy >= Hi) continue;
                } else {
                    const int ty = oy + g.pt - ky * g.dh;
                    if (ty < 0 || ty % g.sh != 0) continue;
                    iy = ty / g.sh;
                    if (iy >= Hi) continue;
                }
                const size_t row = ((size_t)b * Hi + iy) * Wi;
                float xin[P2_VPT][P2_RK];
                bool any = false;
#pragma unroll
                for (int v = 0; v < P2_VPT; ++v) {
                    const int ox = x0 + v;
                    int ix;
                    bool ok = ox < Wo;
                    if (!UP) {
                        ix = ox * g.sw + kx * g.dw - g.pl;
                        ok = ok && ix >= 0 && ix < Wi;
                    } else {
                        const int tx = ox + g.pl - kx * g.dw;
                        ix = tx / g.sw;
                        ok = ok && tx >= 0 && tx % g.sw == 0 && ix < Wi;
                    }
                    if (ok) {
                        p2_ld8<TI>(in, (row + ix) * Cr + r0, second, xin[v]);
                        any = true;
                    } else {
#pragma unroll
                        for (int j = 0; j < P2_RK; ++j) xin[v][j] = 0.f;
                    }
                }
                if (!any) continue;
                const float* wp = wl + tl * P2_RK * cqp + cg * P2_CPT;
#pragma unroll
                for (int j = 0; j < P2_RK; ++j) {
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + j * cqp);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + j * cqp + 4);
#pragma unroll
                    for (int v = 0; v < P2_VPT; ++v) {
                        const float xv = xin[v][j];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            acc[v][c] = fmaf(xv, w0[c], acc[v][c]);
                            acc[v][4 + c] = fmaf(xv, w1[c], acc[v][4 + c]);
                        }
                    }
                }
            }
        }
    }
    if (!live) return;
    const size_t orow = ((size_t)b * Ho + oy) * Wo;
#pragma unroll
    for (int v = 0; v < P2_VPT; ++v) {
        const int ox = x0 + v;
        if (ox >= Wo) continue;
#pragma unroll
        for (int c = 0; c < P2_CPT; ++c) {
            const int q = cg * P2_CPT + c;
            if (q < Cq) stf<TO>(out, (orow + ox) * Cq + q, act_fwd(acc[v][c] + (bias ? bias[q] : 0.f), act));
        }
    }
}

// scalar routes: one thread per output element (gconv.hip's kernels with the geometry handed in)
template <typename TI, typename TO>
__global__ void k_p2_down(const TI* __restrict__ big, const float* __restrict__ w, const float* __restrict__ bias,
                          TO* __restrict__ small, P2 g, int act) {
    const size_t n = (size_t)g.B * g.Hs * g.Ws * g.Cb;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int cb = (int)(i % g.Cb);
        size_t r = i / g.Cb;
        const int ox = (int)(r % g.Ws); r /= g.Ws;
        const int oy = (int)(r % g.Hs);
        const int b = (int)(r / g.Hs);
        float acc = bias ? bias[cb] : 0.f;
        for (int ky = 0; ky < g.kh; ++ky) {
            const int iy = oy * g.sh + ky * g.dh - g.pt;
            if (iy < 0 || iy >= g.Hb) continue;
            for (int kx = 0; kx < g.kw; ++kx) {
                const int ix = ox * g.sw + kx * g.dw - g.pl;
                if (ix < 0 || ix >= g.Wb) continue;
                const size_t xo = (((size_t)b * g.Hb + iy) * g.Wb + ix) * g.Ca;
                const float* wp = w + (size_t)(ky * g.kw + kx) * g.Ca * g.Cb + cb;
                for (int ca = 0; ca < g.Ca; ++ca) acc = fmaf(ldf<TI>(big, xo + ca), wp[(size_t)ca * g.Cb], acc);
            }
        }
        stf<TO>(small, i, act_fwd(acc, act));
    }
}

template <typename TI, typename TO>
__global__ void k_p2_up(const TI* __restrict__ small, const float* __restrict__ w, const float* __restrict__ bias,
                        TO* __restrict__ big, P2 g, int act) {
    const size_t n = (size_t)g.B * g.Hb * g.Wb * g.Ca;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int ca = (int)(i % g.Ca);
        size_t r = i / g.Ca;
        const int ix = (int)(r % g.Wb); r /= g.Wb;
        const int iy = (int)(r % g.Hb);
        const int b = (int)(r / g.Hb);
        float acc = bias ? bias[ca] : 0.f;
        for (int ky = 0; ky < g.kh; ++ky) {
            const int ty = iy + g.pt - ky * g.dh;
            if (ty < 0 || ty % g.sh != 0 || ty / g.sh >= g.Hs) continue;
            for (int kx = 0; kx < g.kw; ++kx) {
                const int tx = ix + g.pl - kx * g.dw;
                if (tx < 0 || tx % g.sw != 0 || tx / g.sw >= g.Ws) continue;
                const size_t yo = (((size_t)b * g.Hs + ty / g.sh) * g.Ws + tx / g.sw) * g.Cb;
                const float* wp = w + ((size_t)(ky * g.kw + kx) * g.Ca + ca) * g.Cb;
                for (int cb = 0; cb < g.Cb; ++cb) acc = fmaf(ldf<TI>(small, yo + cb), wp[cb], acc);
            }
        }
        stf<TO>(big, i, act_fwd(acc, act));
    }
}

// ---- filter gradient -------------------------------------------------------------------------------------------------------------
constexpr int WG_T = 32;           // channel tile (both operands) and pixels staged at a time
constexpr int WG_BLOCKS = 2048;    // blocks the first stage aims at
constexpr int WG_MAXCHUNK = 256;

// block (tile, chunk): tile = (tap, a-tile, b-tile).  Thread t: a-channels 4 (t & 7) .. + 3, b-channels 4 ((t >> 3) & 7) .. + 3,
// pixel group t >> 6 (pixels 8 pg .. 8 pg + 7 of the 32 staged).  dst: the chunk's slice of the workspace, or dw itself (one chunk).
template <typename TB, typename TS>
__global__ __launch_bounds__(256) void k_p2_wgrad(const TB* __restrict__ big, const TS* __restrict__ small, float* __restrict__ dst,
                                                  P2 g, int per_chunk, int to_dw) {
    __shared__ __attribute__((aligned(16))) float la[WG_T][WG_T];           // [pixel][a]
    __shared__ __attribute__((aligned(16))) float lb[WG_T][WG_T];           // [pixel][b]
    __shared__ __attribute__((aligned(16))) float red[3][64][16];
    const int nta = (g.Ca + WG_T - 1) / WG_T, ntb = (g.Cb + WG_T - 1) / WG_T;
    int tile = blockIdx.x;
    const int tb = tile % ntb; tile /= ntb;
    const int ta = tile % nta;
    const int tap = tile / nta, ky = tap / g.kw, kx = tap % g.kw;
    const int chunk = blockIdx.y;
    const int P = g.B * g.Hs * g.Ws;                                         // (< 2^31: checked by the host)
    const int p_begin = chunk * per_chunk, p_end = min(P, p_begin + per_chunk);
    const int t = threadIdx.x, a4 = (t & 7) * 4, b4 = ((t >> 3) & 7) * 4, pg = t >> 6;

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int p0 = p_begin; p0 < p_end; p0 += WG_T) {
        __syncthreads();
#pragma unroll
        for (int e = t; e < WG_T * WG_T; e += 256) {
            const int c = e & (WG_T - 1), pp = e / WG_T, p = p0 + pp;
            float va = 0.f, vb = 0.f;
            if (p < p_end) {
                const int ox = p % g.Ws, oy = (p / g.Ws) % g.Hs, b = p / (g.Ws * g.Hs);
                const int iy = oy * g.sh + ky * g.dh - g.pt, ix = ox * g.sw + kx * g.dw - g.pl;
                const int ca = ta * WG_T + c, cb = tb * WG_T + c;
                if (iy >= 0 && iy < g.Hb && ix >= 0 && ix < g.Wb) {          // (a padded tap: va = 0 kills the pixel's products)
                    if (ca < g.Ca) va = ldf<TB>(big, (((size_t)b * g.Hb + iy) * g.Wb + ix) * g.Ca + ca);
                    if (cb < g.Cb) vb = ldf<TS>(small, (size_t)p * g.Cb + cb);
                }
            }
            la[pp][c] = va;
            lb[pp][c] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(&la[pg * 8 + q][a4]);
            const f32x4 vb = *reinterpret_cast<const f32x4*>(&lb[pg * 8 + q][b4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(va[i], vb[j], acc[i][j]);
        }
    }
    // pixel groups 1..3 hand their tiles to group 0, which adds them in group order
    if (pg > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[pg - 1][t & 63][i * 4 + j] = acc[i][j];
    }
    __syncthreads();
    if (pg > 0) return;
    float* o = dst + (to_dw ? (size_t)0 : (size_t)chunk * g.kh * g.kw * g.Ca * g.Cb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ca = ta * WG_T + a4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = tb * WG_T + b4 + j;
            float s = acc[i][j];
            for (int k = 0; k < 3; ++k) s += red[k][t][i * 4 + j];
            if (ca < g.Ca && cb < g.Cb) {
                const size_t idx = ((size_t)tap * g.Ca + ca) * g.Cb + cb;
                o[idx] = to_dw ? o[idx] + s : s;
            }
        }
    }
}

// dw[i] += ws[0][i] + ws[1][i] + ... in chunk order
__global__ void k_p2_wgrad_sum(const float* __restrict__ ws, float* __restrict__ dw, int n, int nchunk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += ws[(size_t)c * n + i];
    dw[i] += s;
}

// small pixels per chunk (a multiple of WG_T) and the number of chunks
void wg_split(const P2& g, int* per_chunk, int* nchunk) {
    const long long P = (long long)g.B * g.Hs * g.Ws;
    const long long tiles = (long long)g.kh * g.kw * ((g.Ca + WG_T - 1) / WG_T) * ((g.Cb + WG_T - 1) / WG_T);
    long long want = (WG_BLOCKS + tiles - 1) / tiles;
    if (want > WG_MAXCHUNK) want = WG_MAXCHUNK;
    const long long groups = (P + WG_T - 1) / WG_T;                           // chunks are whole 32-pixel groups
    if (want > groups) want = groups;
    if (want < 1) want = 1;
    const long long gpc = (groups + want - 1) / want;
    *per_chunk = (int)(gpc * WG_T);
    *nchunk = (int)((groups + gpc - 1) / gpc);
}

// x_big: the layer's input is the big side (convolution); otherwise the small side (transposed convolution)
int make_p2(P2* g, bool x_big, int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo,
            int pt, int pl) {
    PHX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0 && Ho > 0 &&
                Wo > 0 && pt >= 0 && pl >= 0, PHX_E_SHAPE, "conv2d_pad: bad shape");
    g->B = B; g->kh = kh; g->kw = kw; g->sh = sh; g->sw = sw; g->dh = dh; g->dw = dw; g->pt = pt; g->pl = pl;
    if (x_big) { g->Hb = H; g->Wb = W; g->Ca = Cin; g->Hs = Ho; g->Ws = Wo; g->Cb = Cout; }
    else { g->Hs = H; g->Ws = W; g->Cb = Cin; g->Hb = Ho; g->Wb = Wo; g->Ca = Cout; }
    const long long lim = 1ll << 31;
    PHX_REQUIRE((long long)kh * kw * g->Ca < lim && (long long)B * g->Hs * g->Ws < lim && (long long)B * g->Hb * g->Wb < lim &&
                (long long)g->Hs * sh + (long long)kh * dh + pt < lim && (long long)g->Ws * sw + (long long)kw * dw + pl < lim &&
                (long long)g->Hb + pt < lim && (long long)g->Wb + pl < lim, PHX_E_SHAPE, "conv2d_pad: shape too large");
    return PHX_OK;
}

bool p2_vec_ok(int in_dt, int Cr, int Cq) {
    const int cqp = (Cq + P2_CPT - 1) / P2_CPT * P2_CPT;
    return Cr % (in_dt == PHX_BF16 ? 8 : 4) == 0 && P2_RK * cqp <= P2_LDS;
}

template <bool UP>
int p2_launch(const void* in, int in_dt, const float* w, const float* bias, void* out, int out_dt, const P2& g, int act, void* stream) {
    PHX_REQUIRE(in && w && out, PHX_E_INVAL, "conv2d_pad: null pointer");
    const int Cr = UP ? g.Cb : g.Ca, Cq = UP ? g.Ca : g.Cb;
    const int Ho = UP ? g.Hb : g.Hs, Wo = UP ? g.Wb : g.Ws;
    if (p2_vec_ok(in_dt, Cr, Cq)) {
        const size_t nitem = (size_t)g.B * Ho * ((Wo + P2_VPT - 1) / P2_VPT) * ((Cq + P2_CPT - 1) / P2_CPT);
        const size_t nblk = (nitem + 255) / 256;
        PHX_REQUIRE(nblk < (1ull << 31), PHX_E_SHAPE, "conv2d_pad: shape too large");
        PHX_DT_SWITCH(in_dt, TI, PHX_DT_SWITCH(out_dt, TO, {
            hipLaunchKernelGGL((k_p2_vec<TI, TO, UP>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const TI*)in, w, bias,
                               (TO*)out, g, act);
        }));
    } else {
        const size_t n = (size_t)g.B * Ho * Wo * Cq;
        PHX_DT_SWITCH(in_dt, TI, PHX_DT_SWITCH(out_dt, TO, {
            if (UP)
                hipLaunchKernelGGL((k_p2_up<TI, TO>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const TI*)in,
                                   w, bias, (TO*)out, g, act);
            else
                hipLaunchKernelGGL((k_p2_down<TI, TO>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                   (const TI*)in, w, bias, (TO*)out, g, act);
        }));
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int p2_wgrad(const void* big, int big_dt, const void* small, int small_dt, float* dw, float* ws, const P2& g, void* stream) {
    PHX_REQUIRE(big && small && dw, PHX_E_INVAL, "conv2d_pad wgrad: null pointer");
    int per_chunk, nchunk;
    wg_split(g, &per_chunk, &nchunk);
    PHX_REQUIRE(nchunk == 1 || ws, PHX_E_INVAL, "conv2d_pad wgrad: the workspace is missing (phx_conv2d_pad_wgrad_ws_floats)");
    const int n = g.kh * g.kw * g.Ca * g.Cb;                                  // (kh kw Ca < 2^31 / Cb is not implied: checked here)
    PHX_REQUIRE((long long)g.kh * g.kw * g.Ca * g.Cb < (1ll << 31), PHX_E_SHAPE, "conv2d_pad wgrad: filter too large");
    const int tiles = g.kh * g.kw * ((g.Ca + WG_T - 1) / WG_T) * ((g.Cb + WG_T - 1) / WG_T);
    float* dst = nchunk == 1 ? dw : ws;
    PHX_DT_SWITCH(big_dt, TB, PHX_DT_SWITCH(small_dt, TS, {
        hipLaunchKernelGGL((k_p2_wgrad<TB, TS>), dim3(tiles, nchunk), dim3(256), 0, (hipStream_t)stream, (const TB*)big, (const TS*)small,
                           dst, g, per_chunk, nchunk == 1 ? 1 : 0);
    }));
    PHX_CHECK_LAUNCH();
    if (nchunk > 1) {
        hipLaunchKernelGGL(k_p2_wgrad_sum, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dw, n, nchunk);
        PHX_CHECK_LAUNCH();
    }
    return PHX_OK;
}

// ---- pooling: window kh x kw, stride (sh, sw), top / left padding (pt, pl), output Ho x Wo ------------------------------------------
struct PL {
    int B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo;
};

// the first maximum of window (oy, ox) in row-major order over the taps inside the map -> its tap index (-1: no tap inside)
template <typename T>
__device__ __forceinline__ int pool_argmax(const T* __restrict__ x, const PL& g, int b, int oy, int ox, int c) {
    float m = -INFINITY;
    int am = -1;
    for (int ky = 0; ky < g.kh; ++ky) {
        const int iy = oy * g.sh + ky - g.pt;
        if (iy < 0 || iy >= g.H) continue;
        for (int kx = 0; kx < g.kw; ++kx) {
            const int ix = ox * g.sw + kx - g.pl;
            if (ix < 0 || ix >= g.W) continue;
            const float v = ldf<T>(x, (((size_t)b * g.H + iy) * g.W + ix) * g.C + c);
            if (am < 0 || v > m) { m = v; am = ky * g.kw + kx; }
        }
    }
    return am;
}
// number of taps of window (oy, ox) inside the map
__device__ __forceinline__ int pool_count(const PL& g, int oy, int ox) {
    const int y0 = max(oy * g.sh - g.pt, 0), y1 = min(oy * g.sh - g.pt + g.kh, g.H);
    const int x0 = max(ox * g.sw - g.pl, 0), x1 = min(ox * g.sw - g.pl + g.kw, g.W);
    return max(y1 - y0, 0) * max(x1 - x0, 0);
}

template <typename T, bool MAX>
__global__ void k_pool2_fwd(const T* __restrict__ x, T* __restrict__ y, PL g) {
    const size_t n = (size_t)g.B * g.Ho * g.Wo * g.C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % g.C);
        size_t r = i / g.C;
        const int ox = (int)(r % g.Wo); r /= g.Wo;
        const int oy = (int)(r % g.Ho);
        const int b = (int)(r / g.Ho);
        float m = MAX ? -INFINITY : 0.f;
        int cnt = 0;
        for (int ky = 0; ky < g.kh; ++ky) {
            const int iy = oy * g.sh + ky - g.pt;
            if (iy < 0 || iy >= g.H) continue;
            for (int kx = 0; kx < g.kw; ++kx) {
                const int ix = ox * g.sw + kx - g.pl;
                if (ix < 0 || ix >= g.W) continue;
                const float v = ldf<T>(x, (((size_t)b * g.H + iy) * g.W + ix) * g.C + c);
                m = MAX ? fmaxf(m, v) : m + v;
                ++cnt;
            }
        }
        stf<T>(y, i, MAX ? (cnt ? m : 0.f) : (cnt ? m / (float)cnt : 0.f));  // (a window wholly in the padding: no legal geometry has one)
    }
}

// a gather per input element over the windows that hold it, oy then ox ascending: overlapping windows need no atomics, and every
// element of dx is written
template <typename T, bool MAX, bool ACC>
__global__ void k_pool2_bwd(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, PL g) {
    const size_t n = (size_t)g.B * g.H * g.W * g.C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % g.C);
        size_t r = i / g.C;
        const int ix = (int)(r % g.W); r /= g.W;
        const int iy = (int)(r % g.H);
        const int b = (int)(r / g.H);
        // windows with oy s - pt <= iy <= oy s - pt + k - 1
        const int ty = iy + g.pt, tx = ix + g.pl;
        const int oy0 = ty >= g.kh ? (ty - g.kh + g.sh) / g.sh : 0, oy1 = min(ty / g.sh, g.Ho - 1);
        const int ox0 = tx >= g.kw ? (tx - g.kw + g.sw) / g.sw : 0, ox1 = min(tx / g.sw, g.Wo - 1);
        float acc = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                const float gv = ldf<T>(dy, (((size_t)b * g.Ho + oy) * g.Wo + ox) * g.C + c);
                if (MAX) {
                    const int mine = (ty - oy * g.sh) * g.kw + (tx - ox * g.sw);
                    if (pool_argmax<T>(x, g, b, oy, ox, c) == mine) acc += gv;
                } else {
                    acc += gv / (float)pool_count(g, oy, ox);
                }
            }
        stf<T>(dx, i, ACC ? ldf<T>(dx, i) + acc : acc);
    }
}

int make_pl(PL* g, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int pt, int pl, int Ho, int Wo, int mode) {
    PHX_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && Ho > 0 && Wo > 0 && pt >= 0 && pl >= 0,
                PHX_E_SHAPE, "pool2d: bad shape");
    PHX_REQUIRE(mode == PHX_POOL_MAX || mode == PHX_POOL_AVG, PHX_E_INVAL, "pool2d: mode is PHX_POOL_MAX or PHX_POOL_AVG");
    const long long lim = 1ll << 31;
    PHX_REQUIRE((long long)Ho * sh + kh + pt < lim && (long long)Wo * sw + kw + pl < lim && (long long)H + pt + sh < lim &&
                (long long)W + pl + sw < lim && (long long)kh * kw < lim, PHX_E_SHAPE, "pool2d: shape too large");
    *g = PL{B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo};
    return PHX_OK;
}

template <bool ACC>
int pool_bwd(const void* x, const void* dy, int dt, void* dx, int mode, const PL& g, void* stream) {
    PHX_REQUIRE(dy && dx && (x || mode == PHX_POOL_AVG), PHX_E_INVAL, "pool2d: null pointer");
    const size_t n = (size_t)g.B * g.H * g.W * g.C;
    PHX_DT_SWITCH(dt, T, {
        if (mode == PHX_POOL_MAX)
            hipLaunchKernelGGL((k_pool2_bwd<T, true, ACC>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)x, (const T*)dy, (T*)dx, g);
        else
            hipLaunchKernelGGL((k_pool2_bwd<T, false, ACC>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)x, (const T*)dy, (T*)dx, g);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int axis_geometry(int n, int k, int s, int d, int padding, int* out, int* before) {
    const long long ke = (long long)(k - 1) * d + 1;
    if (padding == PHX_PAD_VALID) {
        if (n < ke) return PHX_E_SHAPE;
        *out = (int)((n - ke) / s + 1);
        *before = 0;
    } else {
        const long long o = ((long long)n + s - 1) / s, total = (o - 1) * s + ke - n;
        *out = (int)o;
        *before = (int)((total > 0 ? total : 0) / 2);
    }
    return PHX_OK;
}

}  // namespace

extern "C" {

int phx_conv2d_geometry(int H, int W, int kh, int kw, int sh, int sw, int dh, int dw, int padding, int* Ho, int* Wo, int* pt, int* pl) {
    PHX_REQUIRE(Ho && Wo && pt && pl && (padding == PHX_PAD_SAME || padding == PHX_PAD_VALID), PHX_E_INVAL,
                "conv2d_geometry: bad argument");
    PHX_REQUIRE(H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0, PHX_E_SHAPE, "conv2d_geometry: bad shape");
    PHX_REQUIRE(axis_geometry(H, kh, sh, dh, padding, Ho, pt) == PHX_OK && axis_geometry(W, kw, sw, dw, padding, Wo, pl) == PHX_OK,
                PHX_E_SHAPE, "conv2d_geometry: VALID padding needs an input at least as large as the (dilated) window");
    return PHX_OK;
}

int phx_conv2d_pad_fwd(const void* x, int x_dt, const float* w_hwio, const float* bias, void* y, int y_dt, int B, int H, int W, int Cin,
                       int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, int act, void* stream) {
    P2 g;
    const int rc = make_p2(&g, true, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_launch<false>(x, x_dt, w_hwio, bias, y, y_dt, g, act, stream);
}

int phx_conv2d_pad_dgrad(const void* dy, int dy_dt, const float* w_hwio, void* dx, int dx_dt, int B, int H, int W, int Cin, int Cout,
                         int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, void* stream) {
    P2 g;
    const int rc = make_p2(&g, true, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_launch<true>(dy, dy_dt, w_hwio, nullptr, dx, dx_dt, g, PHX_ACT_ID, stream);
}

size_t phx_conv2d_pad_wgrad_ws_floats(int B, int Hs, int Ws, int Ca, int Cb, int kh, int kw) {
    if (B <= 0 || Hs <= 0 || Ws <= 0 || Ca <= 0 || Cb <= 0 || kh <= 0 || kw <= 0) return 0;
    P2 g = {};
    g.B = B; g.Hs = Hs; g.Ws = Ws; g.Ca = Ca; g.Cb = Cb; g.kh = kh; g.kw = kw;
    int per_chunk, nchunk;
    wg_split(g, &per_chunk, &nchunk);
    return nchunk == 1 ? 0 : (size_t)nchunk * kh * kw * Ca * Cb;
}

int phx_conv2d_pad_wgrad(const void* x, int x_dt, const void* dy, int dy_dt, float* dw_hwio, float* ws, int B, int H, int W, int Cin,
                         int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, void* stream) {
    P2 g;
    const int rc = make_p2(&g, true, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_wgrad(x, x_dt, dy, dy_dt, dw_hwio, ws, g, stream);
}

int phx_tconv2d_pad_fwd(const void* x, int x_dt, const float* w_hwoi, const float* bias, void* y, int y_dt, int B, int H, int W, int Cin,
                        int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, int act, void* stream) {
    P2 g;
    const int rc = make_p2(&g, false, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_launch<true>(x, x_dt, w_hwoi, bias, y, y_dt, g, act, stream);
}

int phx_tconv2d_pad_dgrad(const void* dy, int dy_dt, const float* w_hwoi, void* dx, int dx_dt, int B, int H, int W, int Cin, int Cout,
                          int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, void* stream) {
    P2 g;
    const int rc = make_p2(&g, false, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_launch<false>(dy, dy_dt, w_hwoi, nullptr, dx, dx_dt, g, PHX_ACT_ID, stream);
}

int phx_tconv2d_pad_wgrad(const void* x, int x_dt, const void* dy, int dy_dt, float* dw_hwoi, float* ws, int B, int H, int W, int Cin,
                          int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int Ho, int Wo, int pt, int pl, void* stream) {
    P2 g;
    const int rc = make_p2(&g, false, B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl);
    if (rc != PHX_OK) return rc;
    return p2_wgrad(dy, dy_dt, x, x_dt, dw_hwoi, ws, g, stream);
}

int phx_pool2d_fwd(const void* x, int dt, void* y, int mode, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int pt, int pl,
                   int Ho, int Wo, void* stream) {
    PL g;
    const int rc = make_pl(&g, B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo, mode);
    if (rc != PHX_OK) return rc;
    PHX_REQUIRE(x && y, PHX_E_INVAL, "pool2d: null pointer");
    const size_t n = (size_t)B * Ho * Wo * C;
    PHX_DT_SWITCH(dt, T, {
        if (mode == PHX_POOL_MAX)
            hipLaunchKernelGGL((k_pool2_fwd<T, true>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                               (T*)y, g);
        else
            hipLaunchKernelGGL((k_pool2_fwd<T, false>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                               (T*)y, g);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_pool2d_bwd(const void* x, const void* dy, int dt, void* dx, int mode, int B, int H, int W, int C, int kh, int kw, int sh, int sw,
                   int pt, int pl, int Ho, int Wo, void* stream) {
    PL g;
    const int rc = make_pl(&g, B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo, mode);
    if (rc != PHX_OK) return rc;
    return pool_bwd<false>(x, dy, dt, dx, mode, g, stream);
}

int phx_pool2d_bwd_acc(const void* x, const void* dy, int dt, void* dx, int mode, int B, int H, int W, int C, int kh, int kw, int sh,
                       int sw, int pt, int pl, int Ho, int Wo, void* stream) {
    PL g;
    const int rc = make_pl(&g, B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo, mode);
    if (rc != PHX_OK) return rc;
    return pool_bwd<true>(x, dy, dt, dx, mode, g, stream);
}

}  // extern "C"
