// The 3-D layer family of tfwrapper/layers.py: conv3D (layers.py:148-194), transposed_conv3D (261-323), maxpool3D (31-41),
// bilinear_upsample3D (348-376) and the 5-D centre crop of crop_and_concat (609-612).  NDHWC activations (fp32 or bf16 through
// ldf / stf), fp32 filters, fp32 accumulation, no floating-point atomics: every reduction has a fixed order, so repeats are
// bit-identical in every mode.
//
// [TF 1.12 semantics] SAME per axis: out = ceil(in / s), total = max((out - 1) s + k - in, 0), before = total / 2 (the extra plane
// goes to the far side).  tf.nn.conv3d_transpose is the input gradient of the stride-s SAME convolution that maps its OUTPUT
// (in * s) back to its input, so its padding is total = max(k - s, 0), before = total / 2 per axis.
//
// One geometry serves both layers.  A "big" tensor [B, Db, Hb, Wb, Ca] and a "small" one [B, Ds, Hs, Ws, Cb] are tied by
// big index = small index * s + tap - pad, through a filter [kd][kh][kw][Ca][Cb]:
//     conv3D             fwd = DOWN (big -> small), dgrad = UP (small -> big),  filter [..][Cin][Cout]
//     transposed_conv3D  fwd = UP   (small -> big), dgrad = DOWN,               filter [..][Cout][Cin]
// and the filter gradient dw[tap][a][b] += sum over small voxels of big[.., a] small[.., b] is one kernel for both.
//
// DOWN and UP carry the FLOPs (27 taps against 9 in 2-D).  Fast path (reduction channels % 4 == 0 in fp32, % 8 == 0 in bf16):
// a thread keeps 8 output channels of 4 voxels along W in registers, reads the reduction channels in 16-byte vectors, and takes
// the filter from LDS, staged per block in slices [tap][8 reduction channels][output channels padded to 8].  A 16-lane group of a
// ds_read_b128 then reads consecutive 32-byte pieces of one 256-byte bank row: conflict-free up to 64 output channels, two-way
// beyond.  Any other channel count takes the scalar kernels (one thread per output element): correct, not fast.
#include "phx_common.h"

namespace {

struct V3 {
    int B, Db, Hb, Wb, Ca, Ds, Hs, Ws, Cb, kd, kh, kw, sd, sh, sw, pd, pt, pl;
};

constexpr int V3_VPT = 4;          // voxels along W per thread
constexpr int V3_CPT = 8;          // output channels per thread
constexpr int V3_RK = 8;           // reduction channels per staged slice
constexpr int V3_LDS = 8192;       // floats of filter staging (32 KiB)

// 8 consecutive channels of `p` at element offset `o` (o * sizeof(T) is a multiple of 16); `second`: channels 4..7 exist (fp32)
template <typename T> __device__ __forceinline__ void ld8(const T* p, size_t o, bool second, float* v);
template <> __device__ __forceinline__ void ld8<float>(const float* p, size_t o, bool second, float* v) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + o);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    if (second) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p + o + 4);
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
        v[4] = v[5] = v[6] = v[7] = 0.f;
    }
}
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, size_t o, bool, float* v) {
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
__global__ __launch_bounds__(256) void k_conv3_vec(const TI* __restrict__ in, const float* __restrict__ w,
                                                   const float* __restrict__ bias, TO* __restrict__ out, V3 g, int act) {
    __shared__ __attribute__((aligned(16))) float wl[V3_LDS];
    const int Cr = UP ? g.Cb : g.Ca, Cq = UP ? g.Ca : g.Cb;
    const int Di = UP ? g.Ds : g.Db, Hi = UP ? g.Hs : g.Hb, Wi = UP ? g.Ws : g.Wb;
    const int Do = UP ? g.Db : g.Ds, Ho = UP ? g.Hb : g.Hs, Wo = UP ? g.Wb : g.Ws;
    const int ncg = (Cq + V3_CPT - 1) / V3_CPT, cqp = ncg * V3_CPT;
    const int nxg = (Wo + V3_VPT - 1) / V3_VPT;
    const int ntap = g.kd * g.kh * g.kw;
    const int tk = min(ntap, V3_LDS / (V3_RK * cqp));                       // taps per staged slice (>= 1: checked by the host)
    const size_t nitem = (size_t)g.B * Do * Ho * nxg * ncg;
    const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = item < nitem;
    const int cg = (int)(item % ncg);
    size_t r = item / ncg;
    const int x0 = (int)(r % nxg) * V3_VPT; r /= nxg;
    const int oy = (int)(r % Ho); r /= Ho;
    const int oz = (int)(r % Do);
    const int b = (int)(r / Do);

    float acc[V3_VPT][V3_CPT];
#pragma unroll
    for (int v = 0; v < V3_VPT; ++v)
#pragma unroll
        for (int c = 0; c < V3_CPT; ++c) acc[v][c] = 0.f;

    for (int r0 = 0; r0 < Cr; r0 += V3_RK) {
        const bool second = r0 + 4 < Cr;
        for (int t0 = 0; t0 < ntap; t0 += tk) {
            const int nt = min(tk, ntap - t0);
            __syncthreads();
            for (int e = threadIdx.x; e < nt * V3_RK * cqp; e += 256) {
                int q, j, tl;
                if (!UP) { q = e % cqp; j = (e / cqp) % V3_RK; tl = e / (cqp * V3_RK); }      // global reads contiguous along Cb
                else { j = e % V3_RK; q = (e / V3_RK) % cqp; tl = e / (cqp * V3_RK); }
                const int rr = r0 + j;
                float val = 0.f;
                if (q < Cq && rr < Cr) {
                    const size_t a = UP ? (size_t)q : (size_t)rr, bb = UP ? (size_t)rr : (size_t)q;
                    val = w[((size_t)(t0 + tl) * g.Ca + a) * g.Cb + bb];
                }
                wl[(tl * V3_RK + j) * cqp + q] = val;
            }
            __syncthreads();
            if (!live) continue;
            for (int tl = 0; tl < nt; ++tl) {
                const int tap = t0 + tl;
                const int kx = tap % g.kw, ky = (tap / g.kw) % g.kh, kz = tap / (g.kw * g.kh);
                int iz, iy;
                if (!UP) {
                    iz = oz * g.sd + kz - g.pd;
                    iy = oy * g.sh + ky - g.pt;
                    if (iz < 0 || iz >= Di || iy < 0 || iy >= Hi) continue;
                } else {
                    const int tz = oz + g.pd - kz, ty = oy + g.pt - ky;
                    if (tz < 0 || ty < 0 || tz % g.sd != 0 || ty % g.sh != 0) continue;
                    iz = tz / g.sd;
                    iy = ty / g.sh;
                    if (iz >= Di || iy >= Hi) continue;
                }
                const size_t row = (((size_t)b * Di + iz) * Hi + iy) * Wi;
                float xin[V3_VPT][V3_RK];
                bool any = false;
#pragma unroll
                for (int v = 0; v < V3_VPT; ++v) {
                    const int ox = x0 + v;
                    int ix;
                    bool ok = ox < Wo;
                    if (!UP) {
                        ix = ox * g.sw + kx - g.pl;
                        ok = ok && ix >= 0 && ix < Wi;
                    } else {
                        const int tx = ox + g.pl - kx;
                        ix = tx / g.sw;
                        ok = ok && tx >= 0 && tx % g.sw == 0 && ix < Wi;
                    }
                    if (ok) {
                        ld8<TI>(in, (row + ix) * Cr + r0, second, xin[v]);
                        any = true;
                    } else {
#pragma unroll
                        for (int j = 0; j < V3_RK; ++j) xin[v][j] = 0.f;
                    }
                }
                if (!any) continue;
                const float* wp = wl + tl * V3_RK * cqp + cg * V3_CPT;
#pragma unroll
                for (int j = 0; j < V3_RK; ++j) {
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + j * cqp);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + j * cqp + 4);
#pragma unroll
                    for (int v = 0; v < V3_VPT; ++v) {
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
    const size_t orow = (((size_t)b * Do + oz) * Ho + oy) * Wo;
#pragma unroll
    for (int v = 0; v < V3_VPT; ++v) {
        const int ox = x0 + v;
        if (ox >= Wo) continue;
#pragma unroll
        for (int c = 0; c < V3_CPT; ++c) {
            const int q = cg * V3_CPT + c;
            if (q < Cq) stf<TO>(out, (orow + ox) * Cq + q, act_fwd(acc[v][c] + (bias ? bias[q] : 0.f), act));
        }
    }
}

// scalar fallbacks: one thread per output element
template <typename TI, typename TO>
__global__ void k_conv3_down(const TI* __restrict__ big, const float* __restrict__ w, const float* __restrict__ bias,
                             TO* __restrict__ small, V3 g, int act) {
    const size_t n = (size_t)g.B * g.Ds * g.Hs * g.Ws * g.Cb;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int cb = (int)(i % g.Cb);
        size_t r = i / g.Cb;
        const int ox = (int)(r % g.Ws); r /= g.Ws;
        const int oy = (int)(r % g.Hs); r /= g.Hs;
        const int oz = (int)(r % g.Ds);
        const int b = (int)(r / g.Ds);
        float acc = bias ? bias[cb] : 0.f;
        for (int kz = 0; kz < g.kd; ++kz) {
            const int iz = oz * g.sd + kz - g.pd;
            if (iz < 0 || iz >= g.Db) continue;
            for (int ky = 0; ky < g.kh; ++ky) {
                const int iy = oy * g.sh + ky - g.pt;
                if (iy < 0 || iy >= g.Hb) continue;
                for (int kx = 0; kx < g.kw; ++kx) {
                    const int ix = ox * g.sw + kx - g.pl;
                    if (ix < 0 || ix >= g.Wb) continue;
                    const size_t xo = ((((size_t)b * g.Db + iz) * g.Hb + iy) * g.Wb + ix) * g.Ca;
                    const float* wp = w + (size_t)((kz * g.kh + ky) * g.kw + kx) * g.Ca * g.Cb + cb;
                    for (int ca = 0; ca < g.Ca; ++ca) acc = fmaf(ldf<TI>(big, xo + ca), wp[(size_t)ca * g.Cb], acc);
                }
            }
        }
        stf<TO>(small, i, act_fwd(acc, act));
    }
}

template <typename TI, typename TO>
__global__ void k_conv3_up(const TI* __restrict__ small, const float* __restrict__ w, const float* __restrict__ bias,
                           TO* __restrict__ big, V3 g, int act) {
    const size_t n = (size_t)g.B * g.Db * g.Hb * g.Wb * g.Ca;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int ca = (int)(i % g.Ca);
        size_t r = i / g.Ca;
        const int ix = (int)(r % g.Wb); r /= g.Wb;
        const int iy = (int)(r % g.Hb); r /= g.Hb;
        const int iz = (int)(r % g.Db);
        const int b = (int)(r / g.Db);
        float acc = bias ? bias[ca] : 0.f;
        for (int kz = 0; kz < g.kd; ++kz) {
            const int tz = iz + g.pd - kz;
            if (tz < 0 || tz % g.sd != 0 || tz / g.sd >= g.Ds) continue;
            for (int ky = 0; ky < g.kh; ++ky) {
                const int ty = iy + g.pt - ky;
                if (ty < 0 || ty % g.sh != 0 || ty / g.sh >= g.Hs) continue;
                for (int kx = 0; kx < g.kw; ++kx) {
                    const int tx = ix + g.pl - kx;
                    if (tx < 0 || tx % g.sw != 0 || tx / g.sw >= g.Ws) continue;
                    const size_t yo = ((((size_t)b * g.Ds + tz / g.sd) * g.Hs + ty / g.sh) * g.Ws + tx / g.sw) * g.Cb;
                    const float* wp = w + ((size_t)((kz * g.kh + ky) * g.kw + kx) * g.Ca + ca) * g.Cb;
                    for (int cb = 0; cb < g.Cb; ++cb) acc = fmaf(ldf<TI>(small, yo + cb), wp[cb], acc);
                }
            }
        }
        stf<TO>(big, i, act_fwd(acc, act));
    }
}

// dw[tap][a][b] += sum over small voxels of big[b., o s + tap - pad, a] small[b., o, b]: one block per (tap, a), threads = 32
// channels b x 8 lanes along W; the rows (b, oz, oy) are walked in order by all lanes, then a fixed-order LDS reduction
template <typename TB, typename TS>
__global__ __launch_bounds__(256) void k_conv3_wgrad(const TB* __restrict__ big, const TS* __restrict__ small,
                                                     float* __restrict__ dw, V3 g) {
    const int ca = blockIdx.x % g.Ca, tap = blockIdx.x / g.Ca;
    const int kx = tap % g.kw, ky = (tap / g.kw) % g.kh, kz = tap / (g.kw * g.kh);
    const int rows = g.B * g.Ds * g.Hs;                                      // (< 2^31: checked by the host)
    __shared__ float red[256];
    for (int cb0 = 0; cb0 < g.Cb; cb0 += 32) {
        const int cb = cb0 + (threadIdx.x & 31), lane = threadIdx.x >> 5;
        float acc = 0.f;
        if (cb < g.Cb)
            for (int row = 0; row < rows; ++row) {
                const int oy = row % g.Hs, oz = (row / g.Hs) % g.Ds, b = row / (g.Hs * g.Ds);
                const int iz = oz * g.sd + kz - g.pd, iy = oy * g.sh + ky - g.pt;
                if (iz < 0 || iz >= g.Db || iy < 0 || iy >= g.Hb) continue;
                const size_t brow = (((size_t)b * g.Db + iz) * g.Hb + iy) * g.Wb, srow = (size_t)row * g.Ws;
                for (int ox = lane; ox < g.Ws; ox += 8) {
                    const int ix = ox * g.sw + kx - g.pl;
                    if (ix < 0 || ix >= g.Wb) continue;
                    acc = fmaf(ldf<TB>(big, (brow + ix) * g.Ca + ca), ldf<TS>(small, (srow + ox) * g.Cb + cb), acc);
                }
            }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x < 32 && cb < g.Cb) {
            float t = 0.f;
            for (int q = 0; q < 8; ++q) t += red[q * 32 + threadIdx.x];
            dw[((size_t)tap * g.Ca + ca) * g.Cb + cb] += t;
        }
        __syncthreads();
    }
}

int v3_common(V3* g, int B, int Ca, int Cb, int kd, int kh, int kw, int sd, int sh, int sw) {
    g->B = B; g->Ca = Ca; g->Cb = Cb; g->kd = kd; g->kh = kh; g->kw = kw; g->sd = sd; g->sh = sh; g->sw = sw;
    const long long taps = (long long)kd * kh * kw;
    PHX_REQUIRE(taps * Ca < (1ll << 31) && (long long)B * g->Ds * g->Hs < (1ll << 31) && (long long)B * g->Db * g->Hb < (1ll << 31),
                PHX_E_SHAPE, "conv3d: shape too large");
    return PHX_OK;
}

// conv3D: x [B, D, H, W, Cin] is the big side
int make_gconv3(V3* g, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw) {
    PHX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && kd > 0 && kh > 0 && kw > 0 && sd > 0 && sh > 0 && sw > 0,
                PHX_E_SHAPE, "gconv3d: bad shape");
    g->Db = D; g->Hb = H; g->Wb = W;
    g->Ds = (D + sd - 1) / sd; g->Hs = (H + sh - 1) / sh; g->Ws = (W + sw - 1) / sw;
    const int td = (g->Ds - 1) * sd + kd - D, th = (g->Hs - 1) * sh + kh - H, tw = (g->Ws - 1) * sw + kw - W;
    g->pd = (td > 0 ? td : 0) / 2; g->pt = (th > 0 ? th : 0) / 2; g->pl = (tw > 0 ? tw : 0) / 2;
    return v3_common(g, B, Cin, Cout, kd, kh, kw, sd, sh, sw);
}

// transposed_conv3D: x [B, D, H, W, Cin] is the SMALL side, y [B, D sd, H sh, W sw, Cout] the big one
int make_tconv3(V3* g, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw) {
    PHX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && kd > 0 && kh > 0 && kw > 0 && sd > 0 && sh > 0 && sw > 0,
                PHX_E_SHAPE, "tconv3d: bad shape");
    PHX_REQUIRE((long long)D * sd < (1ll << 31) && (long long)H * sh < (1ll << 31) && (long long)W * sw < (1ll << 31), PHX_E_SHAPE,
                "tconv3d: shape too large");
    g->Ds = D; g->Hs = H; g->Ws = W;
    g->Db = D * sd; g->Hb = H * sh; g->Wb = W * sw;
    g->pd = (kd > sd ? kd - sd : 0) / 2; g->pt = (kh > sh ? kh - sh : 0) / 2; g->pl = (kw > sw ? kw - sw : 0) / 2;
    return v3_common(g, B, Cout, Cin, kd, kh, kw, sd, sh, sw);
}

bool v3_vec_ok(int in_dt, int Cr, int Cq) {
    const int cqp = (Cq + V3_CPT - 1) / V3_CPT * V3_CPT;
    return Cr % (in_dt == PHX_BF16 ? 8 : 4) == 0 && V3_RK * cqp <= V3_LDS;
}

template <bool UP>
int v3_launch(const void* in, int in_dt, const float* w, const float* bias, void* out, int out_dt, const V3& g, int act, void* stream) {
    PHX_REQUIRE(in && w && out, PHX_E_INVAL, "conv3d: null pointer");
    const int Cr = UP ? g.Cb : g.Ca, Cq = UP ? g.Ca : g.Cb;
    const int Do = UP ? g.Db : g.Ds, Ho = UP ? g.Hb : g.Hs, Wo = UP ? g.Wb : g.Ws;
    if (v3_vec_ok(in_dt, Cr, Cq)) {
        const size_t nitem = (size_t)g.B * Do * Ho * ((Wo + V3_VPT - 1) / V3_VPT) * ((Cq + V3_CPT - 1) / V3_CPT);
        const size_t nblk = (nitem + 255) / 256;
        PHX_REQUIRE(nblk < (1ull << 31), PHX_E_SHAPE, "conv3d: shape too large");
        PHX_DT_SWITCH(in_dt, TI, PHX_DT_SWITCH(out_dt, TO, {
            hipLaunchKernelGGL((k_conv3_vec<TI, TO, UP>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const TI*)in, w, bias,
                               (TO*)out, g, act);
        }));
    } else {
        const size_t n = (size_t)g.B * Do * Ho * Wo * Cq;
        PHX_DT_SWITCH(in_dt, TI, PHX_DT_SWITCH(out_dt, TO, {
            if (UP)
                hipLaunchKernelGGL((k_conv3_up<TI, TO>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                   (const TI*)in, w, bias, (TO*)out, g, act);
            else
                hipLaunchKernelGGL((k_conv3_down<TI, TO>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                   (const TI*)in, w, bias, (TO*)out, g, act);
        }));
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int v3_wgrad(const void* big, int big_dt, const void* small, int small_dt, float* dw, const V3& g, void* stream) {
    PHX_REQUIRE(big && small && dw, PHX_E_INVAL, "conv3d wgrad: null pointer");
    PHX_DT_SWITCH(big_dt, TB, PHX_DT_SWITCH(small_dt, TS, {
        hipLaunchKernelGGL((k_conv3_wgrad<TB, TS>), dim3(g.kd * g.kh * g.kw * g.Ca), dim3(256), 0, (hipStream_t)stream, (const TB*)big,
                           (const TS*)small, dw, g);
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

// ---- max pool, window = stride = (pd, ph, pw), each 1 or 2, SAME (far-side padding only); first maximum in (d, h, w) order wins ----
struct P3 {
    int B, D, H, W, C, pd, ph, pw, Do, Ho, Wo;
};
template <typename T, bool BWD>
__global__ void k_maxpool3(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out, P3 g) {
    const size_t n = (size_t)g.B * g.Do * g.Ho * g.Wo * g.C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % g.C);
        size_t r = i / g.C;
        const int ox = (int)(r % g.Wo); r /= g.Wo;
        const int oy = (int)(r % g.Ho); r /= g.Ho;
        const int oz = (int)(r % g.Do);
        const int b = (int)(r / g.Do);
        float m = -INFINITY;
        int am = 0;
        for (int q = 0; q < 8; ++q) {
            const int dz = q >> 2, dyy = (q >> 1) & 1, dx = q & 1;
            const int iz = g.pd * oz + dz, iy = g.ph * oy + dyy, ix = g.pw * ox + dx;
            if (dz >= g.pd || dyy >= g.ph || dx >= g.pw || iz >= g.D || iy >= g.H || ix >= g.W) continue;
            const float v = ldf<T>(x, ((((size_t)b * g.D + iz) * g.H + iy) * g.W + ix) * g.C + c);
            if (BWD) { if (v > m) { m = v; am = q; } }
            else m = fmaxf(m, v);
        }
        if (!BWD) {
            stf<T>(out, i, m);
            continue;
        }
        const float gv = ldf<T>(dy, i);
        for (int q = 0; q < 8; ++q) {
            const int dz = q >> 2, dyy = (q >> 1) & 1, dx = q & 1;
            const int iz = g.pd * oz + dz, iy = g.ph * oy + dyy, ix = g.pw * ox + dx;
            if (dz >= g.pd || dyy >= g.ph || dx >= g.pw || iz >= g.D || iy >= g.H || ix >= g.W) continue;
            stf<T>(out, ((((size_t)b * g.D + iz) * g.H + iy) * g.W + ix) * g.C + c, q == am ? gv : 0.f);
        }
    }
}
int make_p3(P3* g, int B, int D, int H, int W, int C, int pd, int ph, int pw) {
    PHX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && C > 0, PHX_E_SHAPE, "maxpool3d: bad shape");
    PHX_REQUIRE((pd == 1 || pd == 2) && (ph == 1 || ph == 2) && (pw == 1 || pw == 2), PHX_E_SHAPE, "maxpool3d: window entries 1 or 2");
    g->B = B; g->D = D; g->H = H; g->W = W; g->C = C; g->pd = pd; g->ph = ph; g->pw = pw;
    g->Do = (D + pd - 1) / pd; g->Ho = (H + ph - 1) / ph; g->Wo = (W + pw - 1) / pw;
    return PHX_OK;
}

// ---- bilinear up-sampling by 2 on three axes, legacy coordinates: up[2k] = x[k], up[2k + 1] = (x[k] + x[min(k + 1, n - 1)]) / 2 ----
template <typename T>
__global__ void k_up3_fwd(const T* __restrict__ x, T* __restrict__ y, int B, int D, int H, int W, int C) {
    const size_t n = (size_t)B * D * H * W * C * 8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int X = (int)(r % (2 * W)); r /= 2 * W;
        const int Y = (int)(r % (2 * H)); r /= 2 * H;
        const int Z = (int)(r % (2 * D));
        const int b = (int)(r / (2 * D));
        const int x0 = X >> 1, x1 = (X & 1) ? min(x0 + 1, W - 1) : x0;
        const int y0 = Y >> 1, y1 = (Y & 1) ? min(y0 + 1, H - 1) : y0;
        const int z0 = Z >> 1, z1 = (Z & 1) ? min(z0 + 1, D - 1) : z0;
        float pz[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const size_t zb = (size_t)b * D + (a ? z1 : z0);
            const size_t r0 = (zb * H + y0) * W, r1 = (zb * H + y1) * W;
            const float t = 0.5f * (ldf<T>(x, (r0 + x0) * C + c) + ldf<T>(x, (r0 + x1) * C + c));
            const float u = 0.5f * (ldf<T>(x, (r1 + x0) * C + c) + ldf<T>(x, (r1 + x1) * C + c));
            pz[a] = 0.5f * (t + u);
        }
        stf<T>(y, i, 0.5f * (pz[0] + pz[1]));
    }
}
// per axis, input k is read by outputs 2k (weight 1), 2k + 1 (1/2, or 1 at the clamped end k = n - 1) and 2k - 1 (1/2, k >= 1)
__device__ __forceinline__ void up3_taps(int k, int n, int* idx, float* wt) {
    idx[0] = 2 * k;     wt[0] = 1.f;
    idx[1] = 2 * k + 1; wt[1] = k == n - 1 ? 1.f : 0.5f;
    idx[2] = 2 * k - 1; wt[2] = k >= 1 ? 0.5f : 0.f;
}
template <typename T, bool ACC>
__global__ void k_up3_bwd(const T* __restrict__ dy, T* __restrict__ dx, int B, int D, int H, int W, int C) {
    const size_t n = (size_t)B * D * H * W * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H); r /= H;
        const int z = (int)(r % D);
        const int b = (int)(r / D);
        int iz[3], iy[3], ix[3];
        float wz[3], wy[3], wx[3];
        up3_taps(z, D, iz, wz);
        up3_taps(y, H, iy, wy);
        up3_taps(x, W, ix, wx);
        float acc = 0.f;
        for (int a = 0; a < 3; ++a) {
            if (wz[a] == 0.f) continue;
            for (int e = 0; e < 3; ++e) {
                if (wy[e] == 0.f) continue;
                const size_t row = (((size_t)b * 2 * D + iz[a]) * 2 * H + iy[e]) * 2 * W;
                float s = 0.f;
                for (int f = 0; f < 3; ++f)
                    if (wx[f] != 0.f) s = fmaf(wx[f], ldf<T>(dy, (row + ix[f]) * C + c), s);
                acc = fmaf(wz[a] * wy[e], s, acc);
            }
        }
        stf<T>(dx, i, ACC ? ldf<T>(dx, i) + acc : acc);
    }
}

// dst[b, z, y, x, :] = src[b, z + oz, y + oy, x + ox, :] inside the source, 0 outside
struct W3 {
    int B, Ds, Hs, Ws, Dd, Hd, Wd, C, oz, oy, ox;
};
template <typename T>
__global__ void k_window3(const T* __restrict__ src, T* __restrict__ dst, W3 g) {
    const size_t n = (size_t)g.B * g.Dd * g.Hd * g.Wd * g.C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % g.C);
        size_t r = i / g.C;
        const int x = (int)(r % g.Wd); r /= g.Wd;
        const int y = (int)(r % g.Hd); r /= g.Hd;
        const int z = (int)(r % g.Dd);
        const int b = (int)(r / g.Dd);
        const int sz = z + g.oz, sy = y + g.oy, sx = x + g.ox;
        const bool in = sz >= 0 && sz < g.Ds && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
        stf<T>(dst, i, in ? ldf<T>(src, ((((size_t)b * g.Ds + sz) * g.Hs + sy) * g.Ws + sx) * g.C + c) : 0.f);
    }
}

// moving pair of a batch norm on a rank-5 tensor: tf.contrib.layers.batch_norm takes its non-fused path there, whose moving
// variance follows the BIASED batch variance.  mean / rstd are the vectors the layer's apply launch published.
__global__ void k_bn_moving_biased(const float* __restrict__ mean, const float* __restrict__ rstd, float eps, float* __restrict__ mm,
                                   float* __restrict__ mv, float momentum, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float rs = rstd[c];
    const float var = fmaxf(1.f / (rs * rs) - eps, 0.f);
    mm[c] -= (mm[c] - mean[c]) * momentum;
    mv[c] -= (mv[c] - var) * momentum;
}

}  // namespace

extern "C" {

int phx_gconv3d_out_size(int D, int H, int W, int sd, int sh, int sw, int* Do, int* Ho, int* Wo) {
    PHX_REQUIRE(D > 0 && H > 0 && W > 0 && sd > 0 && sh > 0 && sw > 0 && Do && Ho && Wo, PHX_E_INVAL, "gconv3d_out_size: bad argument");
    *Do = (D + sd - 1) / sd;
    *Ho = (H + sh - 1) / sh;
    *Wo = (W + sw - 1) / sw;
    return PHX_OK;
}

int phx_gconv3d_fwd(const void* x, int x_dt, const float* w_dhwio, const float* bias, void* y, int y_dt, int B, int D, int H, int W,
                    int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int act, void* stream) {
    V3 g;
    const int rc = make_gconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_launch<false>(x, x_dt, w_dhwio, bias, y, y_dt, g, act, stream);
}

int phx_gconv3d_dgrad(const void* dy, int dy_dt, const float* w_dhwio, void* dx, int dx_dt, int B, int D, int H, int W, int Cin,
                      int Cout, int kd, int kh, int kw, int sd, int sh, int sw, void* stream) {
    V3 g;
    const int rc = make_gconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_launch<true>(dy, dy_dt, w_dhwio, nullptr, dx, dx_dt, g, PHX_ACT_ID, stream);
}

int phx_gconv3d_wgrad(const void* x, int x_dt, const void* dy, int dy_dt, float* dw_dhwio, int B, int D, int H, int W, int Cin,
                      int Cout, int kd, int kh, int kw, int sd, int sh, int sw, void* stream) {
    V3 g;
    const int rc = make_gconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_wgrad(x, x_dt, dy, dy_dt, dw_dhwio, g, stream);
}

int phx_tconv3d_fwd(const void* x, int x_dt, const float* w_dhwoi, const float* bias, void* y, int y_dt, int B, int D, int H, int W,
                    int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int act, void* stream) {
    V3 g;
    const int rc = make_tconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_launch<true>(x, x_dt, w_dhwoi, bias, y, y_dt, g, act, stream);
}

int phx_tconv3d_dgrad(const void* dy, int dy_dt, const float* w_dhwoi, void* dx, int dx_dt, int B, int D, int H, int W, int Cin,
                      int Cout, int kd, int kh, int kw, int sd, int sh, int sw, void* stream) {
    V3 g;
    const int rc = make_tconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_launch<false>(dy, dy_dt, w_dhwoi, nullptr, dx, dx_dt, g, PHX_ACT_ID, stream);
}

int phx_tconv3d_wgrad(const void* x, int x_dt, const void* dy, int dy_dt, float* dw_dhwoi, int B, int D, int H, int W, int Cin,
                      int Cout, int kd, int kh, int kw, int sd, int sh, int sw, void* stream) {
    V3 g;
    const int rc = make_tconv3(&g, B, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw);
    if (rc != PHX_OK) return rc;
    return v3_wgrad(dy, dy_dt, x, x_dt, dw_dhwoi, g, stream);
}

int phx_maxpool3d_fwd(const void* x, int dt, void* y, int B, int D, int H, int W, int C, int pd, int ph, int pw, void* stream) {
    P3 g;
    const int rc = make_p3(&g, B, D, H, W, C, pd, ph, pw);
    if (rc != PHX_OK) return rc;
    PHX_REQUIRE(x && y, PHX_E_INVAL, "maxpool3d: null pointer");
    const size_t n = (size_t)B * g.Do * g.Ho * g.Wo * C;
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_maxpool3<T, false>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)nullptr, (T*)y, g);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_maxpool3d_bwd(const void* x, const void* dy, int dt, void* dx, int B, int D, int H, int W, int C, int pd, int ph, int pw,
                      void* stream) {
    P3 g;
    const int rc = make_p3(&g, B, D, H, W, C, pd, ph, pw);
    if (rc != PHX_OK) return rc;
    PHX_REQUIRE(x && dy && dx, PHX_E_INVAL, "maxpool3d: null pointer");
    const size_t n = (size_t)B * g.Do * g.Ho * g.Wo * C;
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_maxpool3<T, true>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)dy, (T*)dx, g);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_bilinear_up2x_3d_fwd(const void* x, int dt, void* y, int B, int D, int H, int W, int C, void* stream) {
    PHX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && C > 0 && x && y, PHX_E_SHAPE, "bilinear_up2x_3d: bad shape");
    PHX_REQUIRE(D < (1 << 30) && H < (1 << 30) && W < (1 << 30), PHX_E_SHAPE, "bilinear_up2x_3d: shape too large");
    const size_t n = (size_t)B * D * H * W * C * 8;
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_up3_fwd<T>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, B, D,
                           H, W, C);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

static int up3_bwd(const void* dy, int dt, void* dx, int B, int D, int H, int W, int C, bool acc, void* stream) {
    PHX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && C > 0 && dy && dx, PHX_E_SHAPE, "bilinear_up2x_3d: bad shape");
    PHX_REQUIRE(D < (1 << 30) && H < (1 << 30) && W < (1 << 30), PHX_E_SHAPE, "bilinear_up2x_3d: shape too large");
    const size_t n = (size_t)B * D * H * W * C;
    PHX_DT_SWITCH(dt, T, {
        if (acc)
            hipLaunchKernelGGL((k_up3_bwd<T, true>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                               (T*)dx, B, D, H, W, C);
        else
            hipLaunchKernelGGL((k_up3_bwd<T, false>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                               (T*)dx, B, D, H, W, C);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_bilinear_up2x_3d_bwd(const void* dy, int dt, void* dx, int B, int D, int H, int W, int C, void* stream) {
    return up3_bwd(dy, dt, dx, B, D, H, W, C, false, stream);
}
int phx_bilinear_up2x_3d_bwd_acc(const void* dy, int dt, void* dx, int B, int D, int H, int W, int C, void* stream) {
    return up3_bwd(dy, dt, dx, B, D, H, W, C, true, stream);
}

int phx_spatial_window3d(const void* src, void* dst, int dt, int B, int Ds, int Hs, int Ws, int Dd, int Hd, int Wd, int C, int off_z,
                         int off_y, int off_x, void* stream) {
    PHX_REQUIRE(B > 0 && Ds > 0 && Hs > 0 && Ws > 0 && Dd > 0 && Hd > 0 && Wd > 0 && C > 0 && src && dst, PHX_E_SHAPE,
                "spatial_window3d: bad shape");
    const W3 g = {B, Ds, Hs, Ws, Dd, Hd, Wd, C, off_z, off_y, off_x};
    const size_t n = (size_t)B * Dd * Hd * Wd * C;
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_window3<T>), dim3(phx_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, g);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_bn_moving_update_biased(const float* mean, const float* rstd, float eps, float* moving_mean, float* moving_var, float momentum,
                                int C, void* stream) {
    PHX_REQUIRE(mean && rstd && moving_mean && moving_var && C > 0 && momentum > 0.f && momentum <= 1.f, PHX_E_INVAL,
                "bn_moving_update_biased: bad argument");
    hipLaunchKernelGGL(k_bn_moving_biased, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, rstd, eps, moving_mean,
                       moving_var, momentum, C);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
