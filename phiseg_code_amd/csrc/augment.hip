// Mini-batch producer on the device: gather + random-annotator selection + augmentation (rotation, crop-scale, flips) of
// LIDC-shaped training data that lives in HBM -- what the reference does per step on the training thread with numpy / OpenCV
// (data/batch_provider.py:43-67 next_batch, 131-137 _select_random_label, 140-272 _augmentation_function; image helpers
// utils.py:18-38).  At > 4 k images/s the reference's synchronous host pipeline would be the wall.
//
// One block per output image.  The two resamplings of the reference are two PASSES with an intermediate image (rotate, then
// crop + resize: each interpolates on its own grid, they do not compose into one), the intermediate lives in LDS (128 x 128
// fp32 = 64 KiB, 192 x 192 = 144 KiB).  Arithmetic follows OpenCV's published algorithms step by step so that the result is
// reproducible against the CPU restatement (oracle/augment.py): cv2.warpAffine's 1/32-pixel fixed-point source grid with
// float32 table weights and BORDER_CONSTANT 0; cv2.resize INTER_LINEAR with float32 coefficients, horizontal then vertical
// pass; label maps are interpolated as one-hot planes in double (CV_64F) and arg-maxed (utils.py:24-38).  No FMA contraction.
//
// k_augment_elastic adds the reference's fifth augmentation, the random elastic deformation (batch_provider.py:226-248 on utils.py:40-67),
// as a THIRD pass for the samples flagged for it: pass 2 then leaves its image and label map in memory (LDS; a global workspace past
// 160 KiB) and pass 3 gathers through a dense map whose two displacement fields -- cv2.resize INTER_CUBIC of 3 x 3 control points -- are
// evaluated per pixel; cv2.convertMaps' 1/32-pixel fixed point and cv2.remap INTER_LINEAR with BORDER_REFLECT restated the same way
// (tests/elastic_ref.py).  Passes 1 and 2 are the same device code for both kernels.
#pragma clang fp contract(off)

#include "phx_common.h"

struct PhxAugParam {
    int src;            // index into the resident data set
    int annot;          // annotator whose mask is used (lidc: 0 .. 3)
    int flags;          // bit 0 rotate, 1 crop-scale, 2 fliplr, 3 flipud, 4 elastic (phx_augment_batch_elastic only)
    int r_y, p_x, p_y;  // crop-scale: square side and origin (batch_provider.py:216-219)
    double iM[6];       // rotation: inverse of cv2.getRotationMatrix2D((cols/2, rows/2), angle, 1), row major 2 x 3
};

namespace {

constexpr int AUG_ROT = 1, AUG_SCALE = 2, AUG_FLIPLR = 4, AUG_FLIPUD = 8, AUG_ELASTIC = 16;
// k_augment_elastic: one block per image and per CU (LDS), so 16 waves per block to keep the four SIMDs busy through the double-precision
// coordinate arithmetic.  Every pixel is computed on its own: the block size does not enter the result.  (k_augment keeps its 256.)
constexpr int AUG_EL_THREADS = 1024;

__device__ __forceinline__ void resize_coeff(int d, int src, int dst, int* s0, int* s1, float* a0, float* a1) {
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

// fixed-point source grid of cv2.warpAffine for destination pixel (x, y): top-left source pixel and the four float32 weights
__device__ __forceinline__ void warp_taps(const PhxAugParam& p, int x, int y, int* sx, int* sy, float w[4]) {
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

// label of the INTERMEDIATE (rotated) map at (y, x): one-hot planes interpolated in double, arg-max (utils.py:24-27); without
// rotation the source label.  Recomputed where pass 2 needs it (four taps per output pixel) instead of being kept in LDS,
// which then holds the fp32 image alone: 192 x 192 fits.
__device__ __forceinline__ int mid_label(const PhxAugParam& p, const unsigned char* __restrict__ lbl, int X, int Y, int A, int nlabels,
                                         int y, int x) {
    if (!(p.flags & AUG_ROT)) return lbl[(size_t)(y * Y + x) * A];
    int sx, sy;
    float w[4];
    warp_taps(p, x, y, &sx, &sy, w);
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

// ---- pass 1: rotation (cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT 0) or copy -> timg (LDS); the caller synchronises
__device__ __forceinline__ void aug_pass1(const PhxAugParam& p, const float* __restrict__ img, float* timg, int X, int Y) {
    const int npix = X * Y;
    if (p.flags & AUG_ROT) {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const int y = i / Y, x = i - y * Y;
            int sx, sy;
            float w[4];
            warp_taps(p, x, y, &sx, &sy, w);
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
}

// ---- pass 2, one destination pixel i = (y, x): crop + cv2.resize INTER_LINEAR back to X x Y (or copy) -> value and label
__device__ __forceinline__ void aug_pass2_pixel(const PhxAugParam& p, const float* timg, const unsigned char* __restrict__ lbl, int X, int Y,
                                                int A, int nlabels, int i, int y, int x, float* v_out, int* best_out) {
    float v;
    int best;
    if (p.flags & AUG_SCALE) {
        int y0, y1, x0, x1;
        float b0, b1, a0, a1;
        resize_coeff(y, p.r_y, X, &y0, &y1, &b0, &b1);
        resize_coeff(x, p.r_y, Y, &x0, &x1, &a0, &a1);
        const int r0 = (p.p_y + y0) * Y + p.p_x, r1 = (p.p_y + y1) * Y + p.p_x;
        const float h0 = timg[r0 + x0] * a0 + timg[r0 + x1] * a1;
        const float h1 = timg[r1 + x0] * a0 + timg[r1 + x1] * a1;
        v = h0 * b0 + h1 * b1;
        const int l00 = mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y0, p.p_x + x0), l01 = mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y0, p.p_x + x1);
        const int l10 = mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y1, p.p_x + x0), l11 = mid_label(p, lbl, X, Y, A, nlabels, p.p_y + y1, p.p_x + x1);
        double cls[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double g0 = (double)(l00 == c) * (double)a0 + (double)(l01 == c) * (double)a1;
            const double g1 = (double)(l10 == c) * (double)a0 + (double)(l11 == c) * (double)a1;
            cls[c] = g0 * (double)b0 + g1 * (double)b1;
        }
        best = 0;
        for (int c = 1; c < nlabels; ++c)
            if (cls[c] > cls[best]) best = c;
    } else {
        v = timg[i];
        best = mid_label(p, lbl, X, Y, A, nlabels, y, x);
    }
    *v_out = v;
    *best_out = best;
}

__global__ __launch_bounds__(256) void k_augment(const float* __restrict__ images, const unsigned char* __restrict__ labels,
                                                 const PhxAugParam* __restrict__ params, float* __restrict__ x_out,
                                                 unsigned char* __restrict__ s_out, int X, int Y, int A, int nlabels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* timg = reinterpret_cast<float*>(smem);                     // [X][Y] intermediate image
    const PhxAugParam p = params[blockIdx.x];
    const float* img = images + (size_t)p.src * X * Y;
    const unsigned char* lbl = labels + (size_t)p.src * X * Y * A + p.annot;      // element (y, x) at (y * Y + x) * A
    const int npix = X * Y;

    aug_pass1(p, img, timg, X, Y);
    __syncthreads();

    // ---- pass 2, flips on the way out
    float* xo = x_out + (size_t)blockIdx.x * npix;
    unsigned char* so = s_out + (size_t)blockIdx.x * npix;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        float v;
        int best;
        aug_pass2_pixel(p, timg, lbl, X, Y, A, nlabels, i, y, x, &v, &best);
        const int oy = (p.flags & AUG_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AUG_FLIPLR) ? Y - 1 - x : x;
        xo[oy * Y + ox] = v;
        so[oy * Y + ox] = (unsigned char)best;
    }
}

// ---- elastic deformation (batch_provider.py:226-248, utils.py:40-67) -----------------------------------------------------
// cv2.resize INTER_CUBIC of a 3-sample axis to `dst` samples, destination index d: first tap s - 1 and the four float32
// coefficients (A = -0.75).  f and s are NOT clamped for cubic; the tap indices are (replicate).
__device__ __forceinline__ void cubic_coeff(int d, double scale, int* s_out, float c[4]) {
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

__device__ __forceinline__ double sel3(double v0, double v1, double v2, int k) { return k <= 0 ? v0 : (k == 1 ? v1 : v2); }

// one displacement field at one pixel: the 4 x 4 cubic stencil over the 3 x 3 control matrix m (row major), horizontal pass
// (column taps cx .. cx + 3, coefficients a) then vertical pass (row taps ry .. ry + 3, coefficients b); products and sums in
// double, taps added in order 0 .. 3.  Only three distinct (clamped) rows exist, so the horizontal pass runs three times.
__device__ __forceinline__ double cubic_field(const double* m, int cx, const float a[4], int ry, const float b[4]) {
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double m0 = m[3 * r], m1 = m[3 * r + 1], m2 = m[3 * r + 2];
        h[r] = sel3(m0, m1, m2, cx) * (double)a[0] + sel3(m0, m1, m2, cx + 1) * (double)a[1] + sel3(m0, m1, m2, cx + 2) * (double)a[2] +
               sel3(m0, m1, m2, cx + 3) * (double)a[3];
    }
    return sel3(h[0], h[1], h[2], ry) * (double)b[0] + sel3(h[0], h[1], h[2], ry + 1) * (double)b[1] +
           sel3(h[0], h[1], h[2], ry + 2) * (double)b[2] + sel3(h[0], h[1], h[2], ry + 3) * (double)b[3];
}

// cv::borderInterpolate(p, n, BORDER_REFLECT): p < 0 -> -p - 1, p >= n -> 2 n - p - 1, repeated until in range -- in closed form
// (the reflections have period 2 n), so that no coordinate, however far out, takes more than one step or leaves [0, n)
__device__ __forceinline__ int reflect(int p, int n) {
    const int m = 2 * n;
    int q = p % m;
    if (q < 0) q += m;
    return q < n ? q : m - 1 - q;
}

// cv2.convertMaps(CV_16SC2): cvRound(map * 32) (round half to even); the clamp changes no value a finite field can give and keeps
// a non-finite one inside int
__device__ __forceinline__ int fixed_map(float v) { return (int)rintf(fminf(fmaxf(v * 32.f, -1.0e9f), 1.0e9f)); }

// k_augment plus a third pass for the samples whose flags carry AUG_ELASTIC: pass 2 leaves its (pre-flip) image and label map
// in img2 / lab2 -- LDS behind timg where 9 X Y bytes fit, the caller's workspace (ws_img != NULL) otherwise -- and pass 3 gathers
// from them through the dense map (cv2.remap INTER_LINEAR on 1/32-pixel fixed-point maps, BORDER_REFLECT), flips on the way out.
// ctrl [B][2][3][3]: control points of dx (columns) then dy (rows); the fields are evaluated per pixel, never stored.
__global__ __launch_bounds__(AUG_EL_THREADS) void k_augment_elastic(const float* __restrict__ images, const unsigned char* __restrict__ labels,
                                                                    const PhxAugParam* __restrict__ params, const double* __restrict__ ctrl,
                                                                    float* __restrict__ x_out, unsigned char* __restrict__ s_out, float* ws_img,
                                                                    unsigned char* ws_lbl, int X, int Y, int A, int nlabels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* timg = reinterpret_cast<float*>(smem);
    const PhxAugParam p = params[blockIdx.x];
    const float* img = images + (size_t)p.src * X * Y;
    const unsigned char* lbl = labels + (size_t)p.src * X * Y * A + p.annot;
    const int npix = X * Y;
    const bool elastic = (p.flags & AUG_ELASTIC) != 0;                 // uniform over the block
    float* img2 = ws_img ? ws_img + (size_t)blockIdx.x * npix : timg + npix;
    unsigned char* lab2 = ws_img ? ws_lbl + (size_t)blockIdx.x * npix : reinterpret_cast<unsigned char*>(timg + 2 * (size_t)npix);

    aug_pass1(p, img, timg, X, Y);
    __syncthreads();

    float* xo = x_out + (size_t)blockIdx.x * npix;
    unsigned char* so = s_out + (size_t)blockIdx.x * npix;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / Y, x = i - y * Y;
        float v;
        int best;
        aug_pass2_pixel(p, timg, lbl, X, Y, A, nlabels, i, y, x, &v, &best);
        if (elastic) {
            img2[i] = v;
            lab2[i] = (unsigned char)best;
        } else {
            const int oy = (p.flags & AUG_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AUG_FLIPLR) ? Y - 1 - x : x;
            xo[oy * Y + ox] = v;
            so[oy * Y + ox] = (unsigned char)best;
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
        cubic_coeff(x, scale_x, &cx, a);
        cubic_coeff(y, scale_y, &ry, b);
        const float map_x = (float)((double)x + cubic_field(m, cx - 1, a, ry - 1, b));
        const float map_y = (float)((double)y + cubic_field(m + 9, cx - 1, a, ry - 1, b));
        const int ix = fixed_map(map_x), iy = fixed_map(map_y);
        const float wx1 = (float)(ix & 31) * (1.0f / 32.0f), wy1 = (float)(iy & 31) * (1.0f / 32.0f);
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float w[4] = {wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
        const int x0 = reflect(ix >> 5, Y), x1 = reflect((ix >> 5) + 1, Y), y0 = reflect(iy >> 5, X), y1 = reflect((iy >> 5) + 1, X);
        const int t[4] = {y0 * Y + x0, y0 * Y + x1, y1 * Y + x0, y1 * Y + x1};
        const float v = img2[t[0]] * w[0] + img2[t[1]] * w[1] + img2[t[2]] * w[2] + img2[t[3]] * w[3];
        double cls[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = lab2[t[k]];
            if (l < 4) cls[l] += (double)w[k];
        }
        int best = 0;
        for (int c = 1; c < nlabels; ++c)
            if (cls[c] > cls[best]) best = c;
        const int oy = (p.flags & AUG_FLIPUD) ? X - 1 - y : y, ox = (p.flags & AUG_FLIPLR) ? Y - 1 - x : x;
        xo[oy * Y + ox] = v;
        so[oy * Y + ox] = (unsigned char)best;
    }
}

}  // namespace

extern "C" {

int phx_augment_param_bytes(void) { return (int)sizeof(PhxAugParam); }

// images [N][X][Y] f32, labels [N][X][Y][A] u8 (the HDF5 layout of data/lidc_data_loader.py:92-104), params: B records in
// DEVICE memory -> x_out [B][X][Y] (= [B,X,Y,1]) f32, s_out [B][X][Y] u8.  nlabels <= 4 (the one-hot interpolation branch of
// batch_provider.py:204-206,222-224).
int phx_augment_batch(const float* images, const unsigned char* labels, const void* params_dev, float* x_out,
                      unsigned char* s_out, int B, int X, int Y, int A, int nlabels, void* stream) {
    PHX_REQUIRE(images && labels && params_dev && x_out && s_out, PHX_E_INVAL, "augment_batch: null argument");
    PHX_REQUIRE(nlabels >= 1 && nlabels <= 4, PHX_E_SHAPE, "augment_batch: 1 <= nlabels <= 4 (one-hot interpolation)");
    PHX_REQUIRE(X > 0 && Y > 0 && A > 0 && (size_t)X * Y * 4 <= 160 * 1024, PHX_E_SHAPE,
                "augment_batch: the intermediate image has to fit LDS (X * Y <= 40960)");
    if (B <= 0) return PHX_OK;
    const size_t sh = (size_t)X * Y * 4;
    static bool attr = false;
    if (!attr) {
        PHX_CHECK_HIP(hipFuncSetAttribute((const void*)k_augment, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
    }
    hipLaunchKernelGGL(k_augment, dim3(B), dim3(256), sh, (hipStream_t)stream, images, labels, (const PhxAugParam*)params_dev, x_out,
                       s_out, X, Y, A, nlabels);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

// Bytes of global workspace phx_augment_batch_elastic needs: 0 where the three intermediates (two fp32 images and the u8 label map,
// 9 X Y bytes) fit the 160 KiB of LDS, else B second images [B][X][Y] f32 followed by B label maps [B][X][Y] u8.
size_t phx_augment_batch_elastic_ws_bytes(int B, int X, int Y) {
    if (B <= 0 || X <= 0 || Y <= 0 || (size_t)X * Y * 9 <= 160 * 1024) return 0;
    return (size_t)B * X * Y * 5;
}

// phx_augment_batch plus the reference's random elastic deformation (batch_provider.py:226-248) for the records whose flags carry
// bit 16: after rotation and crop-scale, before the flips.  ctrl_dev [B][2][3][3] f64: the 3 x 3 control points of dx then dy,
// already multiplied by sigma (read for flagged records only).  Records without the bit give what phx_augment_batch gives.
int phx_augment_batch_elastic(const float* images, const unsigned char* labels, const void* params_dev, const double* ctrl_dev,
                              float* x_out, unsigned char* s_out, void* workspace, size_t workspace_bytes, int B, int X, int Y, int A,
                              int nlabels, void* stream) {
    PHX_REQUIRE(images && labels && params_dev && ctrl_dev && x_out && s_out, PHX_E_INVAL, "augment_batch_elastic: null argument");
    PHX_REQUIRE(nlabels >= 1 && nlabels <= 4, PHX_E_SHAPE, "augment_batch_elastic: 1 <= nlabels <= 4 (one-hot interpolation)");
    PHX_REQUIRE(X > 0 && Y > 0 && A > 0 && (size_t)X * Y * 4 <= 160 * 1024, PHX_E_SHAPE,
                "augment_batch_elastic: the intermediate image has to fit LDS (X * Y <= 40960)");
    if (B <= 0) return PHX_OK;
    const size_t npix = (size_t)X * Y, need = phx_augment_batch_elastic_ws_bytes(B, X, Y);
    PHX_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0), PHX_E_INVAL,
                "augment_batch_elastic: workspace missing, misaligned or smaller than phx_augment_batch_elastic_ws_bytes");
    float* ws_img = need ? (float*)workspace : nullptr;
    unsigned char* ws_lbl = need ? (unsigned char*)workspace + (size_t)B * npix * 4 : nullptr;
    static bool attr = false;
    if (!attr) {
        PHX_CHECK_HIP(hipFuncSetAttribute((const void*)k_augment_elastic, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
    }
    hipLaunchKernelGGL(k_augment_elastic, dim3(B), dim3(AUG_EL_THREADS), need ? npix * 4 : npix * 9, (hipStream_t)stream, images, labels,
                       (const PhxAugParam*)params_dev, ctrl_dev, x_out, s_out, ws_img, ws_lbl, X, Y, A, nlabels);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
