// Mini-batch producer for label maps with MORE than four labels: the reference's `nlabels > 4` branch (data/batch_provider.py:204-208,
// 221-224, 245-248), where OpenCV can no longer interpolate one-hot planes and the label map is resampled with cv2.INTER_NEAREST.
// The image takes the linear path of csrc/augment.hip (rotate, crop-scale, elastic, flips; same arithmetic, restated here: this file
// shares no code with augment.hip, whose two entries keep refusing nlabels > 4 and whose kernels and results cannot move).
//
// A nearest-neighbour stage reads ONE source pixel, so the label stages compose into a chain of coordinates and need no intermediate
// map: destination pixel -> (elastic) -> (crop-scale) -> (rotate) -> source label.  The rules are restated from OpenCV's published
// algorithms -- believed, not executable here (OpenCV is not installed; the same standing as oracle/augment.py for the linear path):
//   cv2.warpAffine(..., INTER_NEAREST)             the fixed-point grid of the linear path with round_delta = AB_SCALE / 2 (AB_BITS = 10):
//                                                  source pixel (X0 + adelta[x]) >> 10, BORDER_CONSTANT 0 outside
//   cv2.resize(crop, INTER_NEAREST)                sx = min(floor(dx * (src / dst)), src - 1) per axis in double; no half-pixel centre
//   cv2.remap(INTER_NEAREST, BORDER_REFLECT)       on the float32 maps of deformation_to_transformation (do_optimisation=False: no
//                                                  convertMaps): cvRound (half to even) of each map value, reflect-including-edge
// tests/augment_nearest_ref.py restates the same rules in numpy.
#pragma clang fp contract(off)

#include "phx_common.h"

struct PhxAugParamN {          // the record of csrc/augment.hip (phx_augment_param_bytes)
    int src, annot, flags;
    int r_y, p_x, p_y;
    double iM[6];
};

namespace {

constexpr int AN_ROT = 1, AN_SCALE = 2, AN_FLIPLR = 4, AN_FLIPUD = 8, AN_ELASTIC = 16;
constexpr int AN_THREADS = 1024;
constexpr size_t AN_LDS = 160 * 1024;

// ---- the image path: the arithmetic of csrc/augment.hip ---------------------------------------------------------------------------------
__device__ __forceinline__ void an_resize_coeff(int d, int src, int dst, int* s0, int* s1, float* a0, float* a1) {
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

__device__ __forceinline__ void an_warp_taps(const PhxAugParamN& p, int x, int y, int* sx, int* sy, float w[4]) {
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

__device__ __forceinline__ void an_cubic_coeff(int d, double scale, int* s_out, float c[4]) {
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

__device__ __forceinline__ double an_sel3(double v0, double v1, double v2, int k) { return k <= 0 ? v0 : (k == 1 ? v1 : v2); }

__device__ __forceinline__ double an_cubic_field(const double* m, int cx, const float a[4], int ry, const float b[4]) {
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double m0 = m[3 * r], m1 = m[3 * r + 1], m2 = m[3 * r + 2];
        h[r] = an_sel3(m0, m1, m2, cx) * (double)a[0] + an_sel3(m0, m1, m2, cx + 1) * (double)a[1] + an_sel3(m0, m1, m2, cx + 2) * (double)a[2] +
               an_sel3(m0, m1, m2, cx + 3) * (double)a[3];
    }
    return an_sel3(h[0], h[1], h[2], ry) * (double)b[0] + an_sel3(h[0], h[1], h[2], ry + 1) * (double)b[1] +
           an_sel3(h[0], h[1], h[2], ry + 2) * (double)b[2] + an_sel3(h[0], h[1], h[2], ry + 3) * (double)b[3];
}

// cv::borderInterpolate(p, n, BORDER_REFLECT) in closed form: always inside [0, n)
__device__ __forceinline__ int an_reflect(int p, int n) {
    const int m = 2 * n;
    int q = p % m;
    if (q < 0) q += m;
    return q < n ? q : m - 1 - q;
}

__device__ __forceinline__ int an_fixed_map(float v) { return (int)rintf(fminf(fmaxf(v * 32.f, -1.0e9f), 1.0e9f)); }
// cvRound of a map value (half to even); the clamp keeps a non-finite value inside int
__device__ __forceinline__ int an_round_map(float v) { return (int)rintf(fminf(fmaxf(v, -1.0e9f), 1.0e9f)); }

// ---- the label chain ------------------------------------------------------------------------------------------------------------------------
// label of the rotated map at (y, x): cv2.warpAffine INTER_NEAREST, 0 outside; without rotation the source label.  (y, x) inside the map.
__device__ __forceinline__ int an_label_rot(const PhxAugParamN& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int y, int x) {
    if (!(p.flags & AN_ROT)) return lbl[(size_t)(y * Y + x) * A];
    const long rd = 1024 / 2;
    const long adelta = (long)rint(p.iM[0] * (double)x * 1024.0), bdelta = (long)rint(p.iM[3] * (double)x * 1024.0);
    const long X0 = (long)rint((p.iM[1] * (double)y + p.iM[2]) * 1024.0) + rd;
    const long Y0 = (long)rint((p.iM[4] * (double)y + p.iM[5]) * 1024.0) + rd;
    const long sx = (X0 + adelta) >> 10, sy = (Y0 + bdelta) >> 10;
    if (sx < 0 || sx >= Y || sy < 0 || sy >= X) return 0;
    return lbl[(size_t)((int)sy * Y + (int)sx) * A];
}
// label of the crop-scaled map at (y, x): cv2.resize INTER_NEAREST of the r_y x r_y crop at (p_y, p_x); without it the rotated map
__device__ __forceinline__ int an_label_scale(const PhxAugParamN& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int y, int x) {
    if (!(p.flags & AN_SCALE)) return an_label_rot(p, lbl, X, Y, A, y, x);
    const int sy = min((int)floor((double)y * ((double)p.r_y / (double)X)), p.r_y - 1);
    const int sx = min((int)floor((double)x * ((double)p.r_y / (double)Y)), p.r_y - 1);
    return an_label_rot(p, lbl, X, Y, A, p.p_y + sy, p.p_x + sx);
}

// One block per output image.  Image: pass 1 (rotate or copy -> timg in LDS), pass 2 (crop-scale or copy -> out, or img2 when the record
// carries the elastic bit), pass 3 (elastic: the fixed-point bilinear remap from img2).  Labels: the coordinate chain, per output pixel.
// ctrl NULL: the elastic bit is ignored (the plain producer).  img2: LDS behind timg where 8 X Y bytes fit, else the caller's workspace.
__global__ __launch_bounds__(AN_THREADS) void k_augment_nearest(const float* __restrict__ images, const unsigned char* __restrict__ labels,
                                                                const PhxAugParamN* __restrict__ params, const double* __restrict__ ctrl,
                                                                float* __restrict__ x_out, unsigned char* __restrict__ s_out, float* ws_img,
                                                                int X, int Y, int A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* timg = reinterpret_cast<float*>(smem);
    const PhxAugParamN p = params[blockIdx.x];
    const float* img = images + (size_t)p.src * X * Y;
    const unsigned char* lbl = labels + (size_t)p.src * X * Y * A + p.annot;      // element (y, x) at (y * Y + x) * A
    const int npix = X * Y;
    const bool elastic = ctrl != nullptr && (p.flags & AN_ELASTIC) != 0;         // uniform over the block
    float* img2 = ws_img ? ws_img + (size_t)blockIdx.x * npix : timg + npix;

    // ---- pass 1
    if (p.flags & AN_ROT) {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const int y = i / Y, x = i - y * Y;
            int sx, sy;
            float w[4];
            an_warp_taps(p, x, y, &sx, &sy, w);
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int yy = sy + (t >> 1), xx = sx + (t & 1);
                const bool ok = yy >= 0 && yy < X && xx >= 0 && xx < Y;
                const float s = ok ? img[yy * Y + xx] : 0.f;
                v = t == 0 ? s * w[0] : v + s * w[t];
            }
            timg[i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) timg[i] = img[i];
    }
    __syncthreads();

    // ---- pass 2 (and the labels of the records without the elastic stage), flips on the way out
    float* xo = x_out + (size_t)blockIdx.x * npix;
    unsigned char* so = s_out + (size_t)blockIdx.x * npix;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        float v;
        if (p.flags & AN_SCALE) {
            int y0, y1, x0, x1;
            float b0, b1, a0, a1;
            an_resize_coeff(y, p.r_y, X, &y0, &y1, &b0, &b1);
            an_resize_coeff(x, p.r_y, Y, &x0, &x1, &a0, &a1);
            const int r0 = (p.p_y + y0) * Y + p.p_x, r1 = (p.p_y + y1) * Y + p.p_x;
            const float h0 = timg[r0 + x0] * a0 + timg[r0 + x1] * a1;
            const float h1 = timg[r1 + x0] * a0 + timg[r1 + x1] * a1;
            v = h0 * b0 + h1 * b1;
        } else {
            v = timg[i];
        }
        if (elastic) {
            img2[i] = v;
        } else {
            const int oy = (p.flags & AN_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AN_FLIPLR) ? Y - 1 - x : x;
            xo[oy * Y + ox] = v;
            so[oy * Y + ox] = (unsigned char)an_label_scale(p, lbl, X, Y, A, y, x);
        }
    }
    if (!elastic) return;
    __syncthreads();

    // ---- pass 3: out(y, x) = in(y + dy(y, x), x + dx(y, x))
    double m[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) m[k] = ctrl[(size_t)blockIdx.x * 18 + k];
    const double scale_x = 3.0 / (double)Y, scale_y = 3.0 / (double)X;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        int cx, ry;
        float a[4], b[4];
        an_cubic_coeff(x, scale_x, &cx, a);
        an_cubic_coeff(y, scale_y, &ry, b);
        const float map_x = (float)((double)x + an_cubic_field(m, cx - 1, a, ry - 1, b));
        const float map_y = (float)((double)y + an_cubic_field(m + 9, cx - 1, a, ry - 1, b));
        const int ix = an_fixed_map(map_x), iy = an_fixed_map(map_y);
        const float wx1 = (float)(ix & 31) * (1.0f / 32.0f), wy1 = (float)(iy & 31) * (1.0f / 32.0f);
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float w[4] = {wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
        const int x0 = an_reflect(ix >> 5, Y), x1 = an_reflect((ix >> 5) + 1, Y), y0 = an_reflect(iy >> 5, X), y1 = an_reflect((iy >> 5) + 1, X);
        const float v = img2[y0 * Y + x0] * w[0] + img2[y0 * Y + x1] * w[1] + img2[y1 * Y + x0] * w[2] + img2[y1 * Y + x1] * w[3];
        const int ly = an_reflect(an_round_map(map_y), X), lx = an_reflect(an_round_map(map_x), Y);
        const int oy = (p.flags & AN_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AN_FLIPLR) ? Y - 1 - x : x;
        xo[oy * Y + ox] = v;
        so[oy * Y + ox] = (unsigned char)an_label_scale(p, lbl, X, Y, A, ly, lx);
    }
}

}  // namespace

extern "C" {

// Bytes of global workspace: 0 without the elastic stage or where the two fp32 images (8 X Y bytes) fit the 160 KiB of LDS, else B
// second images [B][X][Y] f32.
size_t phx_augment_batch_nearest_ws_bytes(int B, int X, int Y, int elastic) {
    if (B <= 0 || X <= 0 || Y <= 0 || !elastic || (size_t)X * Y * 8 <= AN_LDS) return 0;
    return (size_t)B * X * Y * 4;
}

int phx_augment_batch_nearest(const float* images, const unsigned char* labels, const void* params_dev, const double* ctrl_dev,
                              float* x_out, unsigned char* s_out, void* workspace, size_t workspace_bytes, int B, int X, int Y, int A,
                              int nlabels, void* stream) {
    PHX_REQUIRE(images && labels && params_dev && x_out && s_out, PHX_E_INVAL, "augment_batch_nearest: null argument");
    PHX_REQUIRE(nlabels >= 5 && nlabels <= 256, PHX_E_SHAPE,
                "augment_batch_nearest: 5 <= nlabels <= 256 (phx_augment_batch / phx_augment_batch_elastic take nlabels <= 4)");
    PHX_REQUIRE(X > 0 && Y > 0 && A > 0 && (size_t)X * Y * 4 <= AN_LDS, PHX_E_SHAPE,
                "augment_batch_nearest: the intermediate image has to fit LDS (X * Y <= 40960)");
    if (B <= 0) return PHX_OK;
    const size_t npix = (size_t)X * Y, need = phx_augment_batch_nearest_ws_bytes(B, X, Y, ctrl_dev != nullptr);
    PHX_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0), PHX_E_INVAL,
                "augment_batch_nearest: workspace missing, misaligned or smaller than phx_augment_batch_nearest_ws_bytes");
    static bool attr = false;
    if (!attr) {
        PHX_CHECK_HIP(hipFuncSetAttribute((const void*)k_augment_nearest, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AN_LDS));
        attr = true;
    }
    const size_t lds = (ctrl_dev != nullptr && need == 0) ? npix * 8 : npix * 4;
    hipLaunchKernelGGL(k_augment_nearest, dim3(B), dim3(AN_THREADS), lds, (hipStream_t)stream, images, labels,
                       (const PhxAugParamN*)params_dev, ctrl_dev, x_out, s_out, need ? (float*)workspace : nullptr, X, Y, A);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
