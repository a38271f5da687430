// Images with more than one channel (exp_config.image_size = (H, W, Cx), 2 <= Cx <= 16): the three kernels that met the image as a
// [pixels] array -- the posterior's input concat[x, one_hot(s) - 0.5], the mini-batch producer and the image grid of the summaries.
// Cx = 1 stays with the entries it always had (csrc/elementwise.hip, augment.hip, augment_nearest.hip, summary.hip): this file shares no
// code with them, their kernels and results cannot move, and every entry here refuses Cx = 1.  DESIGN.md section 7l.
//
// Producer: a block per (output image, channel).  The block reads its channel as a strided plane of images [N][X][Y][Cx], keeps ONE fp32
// plane as the intermediate in LDS and writes its channel strided into x_out [B][X][Y][Cx] -- so the LDS budget, the workspace rule and
// every operation of a channel are those of the single-channel kernels, whose arithmetic is restated here step by step (no FMA
// contraction): a channel is resampled with the coordinates and weights of the single-channel path, which is what OpenCV does with a
// multi-channel Mat in warpAffine / resize / remap.  The label map does not depend on the image: the blocks of channel 0 write it.
// The OpenCV rules themselves are restated from its published algorithms -- believed, not executable here (OpenCV is not installed): see
// csrc/augment.hip and csrc/augment_nearest.hip, oracle/augment.py, tests/elastic_ref.py and tests/augment_nearest_ref.py.
#pragma clang fp contract(off)

#include "phx_common.h"

struct PhxAugParamM {          // the record of csrc/augment.hip (phx_augment_param_bytes)
    int src, annot, flags;
    int r_y, p_x, p_y;
    double iM[6];
};

namespace {

constexpr int MC_MAX_CX = 16;
constexpr int AM_ROT = 1, AM_SCALE = 2, AM_FLIPLR = 4, AM_FLIPUD = 8, AM_ELASTIC = 16;
constexpr int AM_THREADS = 1024;
constexpr size_t AM_LDS = 160 * 1024;

// ---- posterior input ---------------------------------------------------------------------------------------------------------------------
// one thread per OUTPUT element (coalesced stores of the [npix][Cx + nlabels] rows)
template <typename TO>
__global__ void __launch_bounds__(256) k_posterior_input_mc(const float* __restrict__ x, const uint8_t* __restrict__ s, TO* __restrict__ out,
                                                            size_t npix, int Cx, int nlabels) {
    const size_t C = (size_t)(Cx + nlabels), n = npix * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / C;
        const int k = (int)(i - p * C);
        const float v = k < Cx ? x[p * Cx + k] : ((k - Cx == (int)s[p] ? 1.f : 0.f) - 0.5f);
        stf<TO>(out, i, v);
    }
}

// ---- the producer: the arithmetic of csrc/augment.hip and csrc/augment_nearest.hip ---------------------------------------------------------
__device__ __forceinline__ void am_resize_coeff(int d, int src, int dst, int* s0, int* s1, float* a0, float* a1) {
    const double scale = (double)src / (double)dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    *s0 = s;
    *s1 = min(s + 1, src - 1);
    *a0 = 1.f - f;
    *a1 = f;
}

__device__ __forceinline__ void am_warp_taps(const PhxAugParamM& p, int x, int y, int* sx, int* sy, float w[4]) {
    const long rd = 1024 / 32 / 2;
    const long adelta = (long)rint(p.iM[0] * (double)x * 1024.0), bdelta = (long)rint(p.iM[3] * (double)x * 1024.0);
    const long X0 = (long)rint((p.iM[1] * (double)y + p.iM[2]) * 1024.0) + rd;
    const long Y0 = (long)rint((p.iM[4] * (double)y + p.iM[5]) * 1024.0) + rd;
    const long XX = (X0 + adelta) >> 5, YY = (Y0 + bdelta) >> 5;
    *sx = (int)(XX >> 5);
    *sy = (int)(YY >> 5);
    const float wx1 = (float)(int)(XX & 31) * (1.0f / 32.0f), wy1 = (float)(int)(YY & 31) * (1.0f / 32.0f);
    const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    w[0] = wy0 * wx0; w[1] = wy0 * wx1; w[2] = wy1 * wx0; w[3] = wy1 * wx1;
}

__device__ __forceinline__ void am_cubic_coeff(int d, double scale, int* s_out, float c[4]) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f = f - (float)s;
    const float A = -0.75f, g = f + 1.f, h = 1.f - f;
    c[0] = ((A * g - 5.f * A) * g + 8.f * A) * g - 4.f * A;
    c[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
    c[2] = ((A + 2.f) * h - (A + 3.f)) * h * h + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
    *s_out = s;
}

__device__ __forceinline__ double am_sel3(double v0, double v1, double v2, int k) { return k <= 0 ? v0 : (k == 1 ? v1 : v2); }

__device__ __forceinline__ double am_cubic_field(const double* m, int cx, const float a[4], int ry, const float b[4]) {
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double m0 = m[3 * r], m1 = m[3 * r + 1], m2 = m[3 * r + 2];
        h[r] = am_sel3(m0, m1, m2, cx) * (double)a[0] + am_sel3(m0, m1, m2, cx + 1) * (double)a[1] + am_sel3(m0, m1, m2, cx + 2) * (double)a[2] +
               am_sel3(m0, m1, m2, cx + 3) * (double)a[3];
    }
    return am_sel3(h[0], h[1], h[2], ry) * (double)b[0] + am_sel3(h[0], h[1], h[2], ry + 1) * (double)b[1] +
           am_sel3(h[0], h[1], h[2], ry + 2) * (double)b[2] + am_sel3(h[0], h[1], h[2], ry + 3) * (double)b[3];
}

// cv::borderInterpolate(p, n, BORDER_REFLECT) in closed form: always inside [0, n)
__device__ __forceinline__ int am_reflect(int p, int n) {
    const int m = 2 * n;
    int q = p % m;
    if (q < 0) q += m;
    return q < n ? q : m - 1 - q;
}

__device__ __forceinline__ int am_fixed_map(float v) { return (int)rintf(fminf(fmaxf(v * 32.f, -1.0e9f), 1.0e9f)); }
__device__ __forceinline__ int am_round_map(float v) { return (int)rintf(fminf(fmaxf(v, -1.0e9f), 1.0e9f)); }

// ---- labels, one-hot route (nlabels <= 4): the intermediate (rotated) map at (y, x), one-hot planes in double, arg-max
__device__ __forceinline__ int am_mid_label(const PhxAugParamM& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int nlabels,
                                            int y, int x) {
    if (!(p.flags & AM_ROT)) return lbl[(size_t)(y * Y + x) * A];
    int sx, sy;
    float w[4];
    am_warp_taps(p, x, y, &sx, &sy, w);
    double cls[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yy = sy + (t >> 1), xx = sx + (t & 1);
        if (yy >= 0 && yy < X && xx >= 0 && xx < Y) {
            const int l = lbl[(size_t)(yy * Y + xx) * A];
            if (l < 4) cls[l] += (double)w[t];
        }
    }
    int best = 0;
    for (int c = 1; c < nlabels; ++c)
        if (cls[c] > cls[best]) best = c;
    return best;
}

// label of the crop-scaled map at (y, x), one-hot route
__device__ __forceinline__ int am_scaled_label(const PhxAugParamM& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int nlabels,
                                               int y, int x) {
    if (!(p.flags & AM_SCALE)) return am_mid_label(p, lbl, X, Y, A, nlabels, y, x);
    int y0, y1, x0, x1;
    float b0, b1, a0, a1;
    am_resize_coeff(y, p.r_y, X, &y0, &y1, &b0, &b1);
    am_resize_coeff(x, p.r_y, Y, &x0, &x1, &a0, &a1);
    const int l00 = am_mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y0, p.p_x + x0), l01 = am_mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y0, p.p_x + x1);
    const int l10 = am_mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y1, p.p_x + x0), l11 = am_mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y1, p.p_x + x1);
    double cls[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double g0 = (double)(l00 == c) * (double)a0 + (double)(l01 == c) * (double)a1;
        const double g1 = (double)(l10 == c) * (double)a0 + (double)(l11 == c) * (double)a1;
        cls[c] = g0 * (double)b0 + g1 * (double)b1;
    }
    int best = 0;
    for (int c = 1; c < nlabels; ++c)
        if (cls[c] > cls[best]) best = c;
    return best;
}

// ---- labels, nearest route (nlabels >= 5): the coordinate chain of csrc/augment_nearest.hip
__device__ __forceinline__ int am_label_rot(const PhxAugParamM& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int y, int x) {
    if (!(p.flags & AM_ROT)) return lbl[(size_t)(y * Y + x) * A];
    const long rd = 1024 / 2;
    const long adelta = (long)rint(p.iM[0] * (double)x * 1024.0), bdelta = (long)rint(p.iM[3] * (double)x * 1024.0);
    const long X0 = (long)rint((p.iM[1] * (double)y + p.iM[2]) * 1024.0) + rd;
    const long Y0 = (long)rint((p.iM[4] * (double)y + p.iM[5]) * 1024.0) + rd;
    const long sx = (X0 + adelta) >> 10, sy = (Y0 + bdelta) >> 10;
    if (sx < 0 || sx >= Y || sy < 0 || sy >= X) return 0;
    return lbl[(size_t)((int)sy * Y + (int)sx) * A];
}
__device__ __forceinline__ int am_label_scale(const PhxAugParamM& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int y, int x) {
    if (!(p.flags & AM_SCALE)) return am_label_rot(p, lbl, X, Y, A, y, x);
    const int sy = min((int)floor((double)y * ((double)p.r_y / (double)X)), p.r_y - 1);
    const int sx = min((int)floor((double)x * ((double)p.r_y / (double)Y)), p.r_y - 1);
    return am_label_rot(p, lbl, X, Y, A, p.p_y + sy, p.p_x + sx);
}

// Block (b, c): channel c of output image b; the blocks with c == 0 also write the label map of image b.
// LDS: timg [X][Y] f32; with the elastic stage and no workspace, img2 [X][Y] f32 behind it and (one-hot route) lab2 [X][Y] u8 behind that.
// Workspace form: ws_img [B][Cx][X][Y] f32, ws_lbl [B][X][Y] u8 (one-hot route only).
template <bool NEAREST>
__global__ __launch_bounds__(AM_THREADS) void k_augment_mc(const float* __restrict__ images, const unsigned char* __restrict__ labels,
                                                           const PhxAugParamM* __restrict__ params, const double* __restrict__ ctrl,
                                                           float* __restrict__ x_out, unsigned char* __restrict__ s_out, float* ws_img,
                                                           unsigned char* ws_lbl, int X, int Y, int A, int Cx, int nlabels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* timg = reinterpret_cast<float*>(smem);
    const int b = blockIdx.x, ch = blockIdx.y;
    const PhxAugParamM p = params[b];
    const int npix = X * Y;
    const float* img = images + (size_t)p.src * npix * Cx + ch;                  // pixel i at img[i * Cx]
    const unsigned char* lbl = labels + (size_t)p.src * npix * A + p.annot;      // element (y, x) at (y * Y + x) * A
    const bool elastic = ctrl != nullptr && (p.flags & AM_ELASTIC) != 0;         // uniform over the block
    const bool lab = ch == 0;
    float* img2 = ws_img ? ws_img + ((size_t)b * Cx + ch) * npix : timg + npix;
    unsigned char* lab2 = NEAREST ? nullptr : (ws_img ? ws_lbl + (size_t)b * npix : reinterpret_cast<unsigned char*>(timg + 2 * (size_t)npix));

    // ---- pass 1: rotation (cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT 0) or copy -> timg
    if (p.flags & AM_ROT) {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const int y = i / Y, x = i - y * Y;
            int sx, sy;
            float w[4];
            am_warp_taps(p, x, y, &sx, &sy, w);
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int yy = sy + (t >> 1), xx = sx + (t & 1);
                const bool ok = yy >= 0 && yy < X && xx >= 0 && xx < Y;
                const float s = ok ? img[(size_t)(yy * Y + xx) * Cx] : 0.f;
                v = t == 0 ? s * w[0] : v + s * w[t];
            }
            timg[i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) timg[i] = img[(size_t)i * Cx];
    }
    __syncthreads();

    // ---- pass 2: crop + cv2.resize INTER_LINEAR back to X x Y (or copy); flips on the way out
    float* xo = x_out + (size_t)b * npix * Cx + ch;
    unsigned char* so = s_out + (size_t)b * npix;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        float v;
        if (p.flags & AM_SCALE) {
            int y0, y1, x0, x1;
            float b0, b1, a0, a1;
            am_resize_coeff(y, p.r_y, X, &y0, &y1, &b0, &b1);
            am_resize_coeff(x, p.r_y, Y, &x0, &x1, &a0, &a1);
            const int r0 = (p.p_y + y0) * Y + p.p_x, r1 = (p.p_y + y1) * Y + p.p_x;
            const float h0 = timg[r0 + x0] * a0 + timg[r0 + x1] * a1;
            const float h1 = timg[r1 + x0] * a0 + timg[r1 + x1] * a1;
            v = h0 * b0 + h1 * b1;
        } else {
            v = timg[i];
        }
        if (elastic) {
            img2[i] = v;
            if (!NEAREST && lab) lab2[i] = (unsigned char)am_scaled_label(p, lbl, X, Y, A, nlabels, y, x);
        } else {
            const int oy = (p.flags & AM_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AM_FLIPLR) ? Y - 1 - x : x;
            xo[(size_t)(oy * Y + ox) * Cx] = v;
            if (lab)
                so[oy * Y + ox] = (unsigned char)(NEAREST ? am_label_scale(p, lbl, X, Y, A, y, x) : am_scaled_label(p, lbl, X, Y, A, nlabels, y, x));
        }
    }
    if (!elastic) return;
    __syncthreads();

    // ---- pass 3: out(y, x) = in(y + dy(y, x), x + dx(y, x)), cv2.remap INTER_LINEAR on 1/32-pixel fixed-point maps, BORDER_REFLECT
    double m[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) m[k] = ctrl[(size_t)b * 18 + k];
    const double scale_x = 3.0 / (double)Y, scale_y = 3.0 / (double)X;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        int cx, ry;
        float a[4], bb[4];
        am_cubic_coeff(x, scale_x, &cx, a);
        am_cubic_coeff(y, scale_y, &ry, bb);
        const float map_x = (float)((double)x + am_cubic_field(m, cx - 1, a, ry - 1, bb));
        const float map_y = (float)((double)y + am_cubic_field(m + 9, cx - 1, a, ry - 1, bb));
        const int ix = am_fixed_map(map_x), iy = am_fixed_map(map_y);
        const float wx1 = (float)(ix & 31) * (1.0f / 32.0f), wy1 = (float)(iy & 31) * (1.0f / 32.0f);
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float w[4] = {wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
        const int x0 = am_reflect(ix >> 5, Y), x1 = am_reflect((ix >> 5) + 1, Y), y0 = am_reflect(iy >> 5, X), y1 = am_reflect((iy >> 5) + 1, X);
        const int t[4] = {y0 * Y + x0, y0 * Y + x1, y1 * Y + x0, y1 * Y + x1};
        const float v = img2[t[0]] * w[0] + img2[t[1]] * w[1] + img2[t[2]] * w[2] + img2[t[3]] * w[3];
        const int oy = (p.flags & AM_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AM_FLIPLR) ? Y - 1 - x : x;
        xo[(size_t)(oy * Y + ox) * Cx] = v;
        if (!lab) continue;
        int best;
        if (NEAREST) {
            const int ly = am_reflect(am_round_map(map_y), X), lx = am_reflect(am_round_map(map_x), Y);
            best = am_label_scale(p, lbl, X, Y, A, ly, lx);
        } else {
            double cls[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l = lab2[t[k]];
                if (l < 4) cls[l] += (double)w[k];
            }
            best = 0;
            for (int c = 1; c < nlabels; ++c)
                if (cls[c] > cls[best]) best = c;
        }
        so[oy * Y + ox] = (unsigned char)best;
    }
}

// ---- image grid of the summaries -----------------------------------------------------------------------------------------------------------
// float -> unsigned key whose unsigned order is the float order (as csrc/summary.hip)
__device__ __forceinline__ unsigned mc_f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mc_key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// min / max over all n values of the tensor, every channel (integer atomics on ordered keys: no order dependence)
__global__ void __launch_bounds__(256) k_grid_minmax_mc(const float* __restrict__ src, size_t n, unsigned* __restrict__ keys) {
    __shared__ unsigned red[2][4];
    float mn = INFINITY, mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = src[i];
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mc_f2key(mx);
        red[1][threadIdx.x >> 6] = ~mc_f2key(mn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, b = 0;
        for (int w = 0; w < 4; ++w) {
            a = max(a, red[0][w]);
            b = max(b, red[1][w]);
        }
        atomicMax(&keys[0], a);
        atomicMax(&keys[1], b);
    }
}

// one thread per output PIXEL: Cout bytes each
__global__ void __launch_bounds__(256) k_grid_write_mc(const float* __restrict__ src, int H, int W, int Cx, int Cout, int gy_n, int gx_n,
                                                       const unsigned* __restrict__ keys, unsigned char* __restrict__ out) {
    const int Y = H + 2, X = W + 2;
    const size_t rows = (size_t)Y * gy_n, cols = (size_t)X * gx_n;
    const float mx = mc_key2f(keys[0]), mn = mc_key2f(~keys[1]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / cols), c = (int)(i % cols);
        const int gy = r / Y, y = r % Y, gx = c / X, x = c % X;
        const bool inside = y > 0 && y < Y - 1 && x > 0 && x < X - 1;          // else the pad of 1 around every tile
        const size_t pix = inside ? ((size_t)(gx * gy_n + gy) * H + (y - 1)) * W + (x - 1) : 0;
        for (int k = 0; k < Cout; ++k) {
            unsigned char o = 0;
            if (inside) {
                float f = src[pix * Cx + k] - mn;                               // the reference's 'image' branch, step by step in fp32
                f = f / mx;
                f = f * 254.0f;
                o = !(f == f) ? 0 : (f <= 0.f ? 0 : (f >= 255.f ? 255 : (unsigned char)f));     // NaN -> 0, saturate, else truncate
            }
            out[i * Cout + k] = o;
        }
    }
}

}  // namespace

extern "C" {

int phx_posterior_input_mc(const float* x, const uint8_t* s, void* out, int out_dt, size_t npix, int Cx, int nlabels, void* stream) {
    PHX_REQUIRE(x && s && out, PHX_E_INVAL, "posterior_input_mc: null argument");
    PHX_REQUIRE(out_dt == PHX_F32 || out_dt == PHX_BF16, PHX_E_INVAL, "posterior_input_mc: out_dt is PHX_F32 or PHX_BF16");
    PHX_REQUIRE(Cx >= 2 && Cx <= MC_MAX_CX, PHX_E_SHAPE, "posterior_input_mc: 2 <= Cx <= 16 (phx_posterior_input takes Cx = 1)");
    PHX_REQUIRE(nlabels >= 1 && nlabels <= 256, PHX_E_SHAPE, "posterior_input_mc: 1 <= nlabels <= 256");
    PHX_REQUIRE(npix < ((size_t)1 << 40), PHX_E_SHAPE, "posterior_input_mc: fewer than 2^40 pixels");
    if (npix == 0) return PHX_OK;
    const size_t n = npix * (size_t)(Cx + nlabels);
    PHX_DT_SWITCH(out_dt, TO, {
        hipLaunchKernelGGL((k_posterior_input_mc<TO>), dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, s, (TO*)out, npix, Cx,
                           nlabels);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

size_t phx_augment_batch_mc_ws_bytes(int B, int X, int Y, int Cx, int nlabels, int elastic) {
    if (B <= 0 || X <= 0 || Y <= 0 || Cx <= 0 || !elastic) return 0;
    const size_t npix = (size_t)X * Y;
    if (nlabels <= 4) return npix * 9 <= AM_LDS ? 0 : (size_t)B * Cx * npix * 4 + (size_t)B * npix;
    return npix * 8 <= AM_LDS ? 0 : (size_t)B * Cx * npix * 4;
}

int phx_augment_batch_mc(const float* images, const unsigned char* labels, const void* params_dev, const double* ctrl_dev, float* x_out,
                         unsigned char* s_out, void* workspace, size_t workspace_bytes, int B, int X, int Y, int A, int Cx, int nlabels,
                         void* stream) {
    PHX_REQUIRE(images && labels && params_dev && x_out && s_out, PHX_E_INVAL, "augment_batch_mc: null argument");
    PHX_REQUIRE(Cx >= 2 && Cx <= MC_MAX_CX, PHX_E_SHAPE, "augment_batch_mc: 2 <= Cx <= 16 (the single-channel entries take Cx = 1)");
    PHX_REQUIRE(nlabels >= 1 && nlabels <= 256, PHX_E_SHAPE, "augment_batch_mc: 1 <= nlabels <= 256");
    PHX_REQUIRE(X > 0 && Y > 0 && A > 0 && (size_t)X * Y * 4 <= AM_LDS, PHX_E_SHAPE,
                "augment_batch_mc: the intermediate plane has to fit LDS (X * Y <= 40960)");
    if (B <= 0) return PHX_OK;
    const bool el = ctrl_dev != nullptr, nearest = nlabels > 4;
    const size_t npix = (size_t)X * Y, need = phx_augment_batch_mc_ws_bytes(B, X, Y, Cx, nlabels, el ? 1 : 0);
    PHX_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0), PHX_E_INVAL,
                "augment_batch_mc: workspace missing, misaligned or smaller than phx_augment_batch_mc_ws_bytes");
    float* ws_img = need ? (float*)workspace : nullptr;
    unsigned char* ws_lbl = (need && !nearest) ? (unsigned char*)workspace + (size_t)B * Cx * npix * 4 : nullptr;
    const size_t lds = (el && need == 0) ? npix * (nearest ? 8 : 9) : npix * 4;
    static bool attr = false;
    if (!attr) {
        PHX_CHECK_HIP(hipFuncSetAttribute((const void*)k_augment_mc<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AM_LDS));
        PHX_CHECK_HIP(hipFuncSetAttribute((const void*)k_augment_mc<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AM_LDS));
        attr = true;
    }
    const PhxAugParamM* par = (const PhxAugParamM*)params_dev;
    if (nearest)
        hipLaunchKernelGGL(k_augment_mc<true>, dim3(B, Cx), dim3(AM_THREADS), lds, (hipStream_t)stream, images, labels, par, ctrl_dev, x_out,
                           s_out, ws_img, ws_lbl, X, Y, A, Cx, nlabels);
    else
        hipLaunchKernelGGL(k_augment_mc<false>, dim3(B, Cx), dim3(AM_THREADS), lds, (hipStream_t)stream, images, labels, par, ctrl_dev, x_out,
                           s_out, ws_img, ws_lbl, X, Y, A, Cx, nlabels);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_summary_grid_image_mc(const float* src, int B, int H, int W, int Cx, int Cout, int grid_y, int grid_x, unsigned char* out, void* work,
                              void* stream) {
    PHX_REQUIRE(src && out && work, PHX_E_INVAL, "summary_grid_image_mc: null pointer");
    PHX_REQUIRE(Cx >= 2 && Cx <= MC_MAX_CX, PHX_E_SHAPE, "summary_grid_image_mc: 2 <= Cx <= 16 (phx_summary_grid_u8 takes one channel)");
    PHX_REQUIRE((Cout == 1 || Cout == 3 || Cout == 4) && Cout <= Cx, PHX_E_SHAPE, "summary_grid_image_mc: Cout in {1, 3, 4}, Cout <= Cx");
    PHX_REQUIRE(B > 0 && H > 0 && W > 0 && grid_y > 0 && grid_x > 0 && grid_y * grid_x == B, PHX_E_SHAPE,
                "summary_grid_image_mc: grid_y * grid_x == B");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W * Cx;
    const size_t nout = (size_t)(H + 2) * grid_y * (size_t)(W + 2) * grid_x;
    PHX_REQUIRE(nout < ((size_t)1 << 38), PHX_E_SHAPE, "summary_grid_image_mc: grid too large");
    PHX_CHECK_HIP(hipMemsetAsync(work, 0, PHX_SUMMARY_GRID_WS_BYTES, st));
    hipLaunchKernelGGL(k_grid_minmax_mc, dim3(phx_grid_for(n, 256, 1024)), dim3(256), 0, st, src, n, (unsigned*)work);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_write_mc, dim3(phx_grid_for(nout, 256)), dim3(256), 0, st, src, H, W, Cx, Cout, grid_y, grid_x,
                       (const unsigned*)work, out);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
