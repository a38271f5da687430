// Segmentation losses of the reference's tfwrapper/losses.py on the device: get_dice / dice_loss (losses.py:8-119), cross_entropy_loss
// (:123-131) and pixel_wise_cross_entropy_loss_weighted (:135-159), with their gradients with respect to the logits, and the adjoint
// of the nearest-neighbour resize (likelihoods.py:221) that carries a gradient on the summed logits down to the coarse levels.
//   logits  [B][H][W][C] f32, 2 <= C <= 8 (logit heads are fp32 in bf16 plans too)
//   labels  [B][H][W] u8 class indices; the one-hot of the reference is folded into the read (a label >= C matches no class)
// A thread owns whole pixels and reads a pixel's classes as one 8- or 16-byte word where C allows it.  Every sum is formed in a fixed
// order -- wave shuffles, the block's four waves in LDS, one partial record per block, a finishing launch that adds the records in
// block order (in double) -- and there is no floating-point atomic in this file: two calls on the same input give the same bits,
// whatever PHX_DETERMINISTIC says.
#include "phx_common.h"

#define SL_MAXC 8
#define SL_BLOCK 256
#define SL_PPT 4                                   // pixels per thread
#define SL_TILE (SL_BLOCK * SL_PPT)                // pixels per block
#define SL_NQ 5                                    // sums per (image, class): i, l (soft), r, i_hard, l_hard

template <int C> __device__ __forceinline__ void sl_load(const float* __restrict__ base, size_t pix, float (&v)[C]) {
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(base + pix * C)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else if constexpr (C % 2 == 0) {
#pragma unroll
        for (int q = 0; q < C / 2; ++q) {
            const float2 t = reinterpret_cast<const float2*>(base + pix * C)[q];
            v[2 * q] = t.x; v[2 * q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = base[pix * C + c];
    }
}

template <int C, bool ADD> __device__ __forceinline__ void sl_store(float* __restrict__ base, size_t pix, const float (&v)[C]) {
    float o[C];
    if (ADD) {
        sl_load<C>(base, pix, o);
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] += v[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = v[c];
    }
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int q = 0; q < C / 4; ++q)
            reinterpret_cast<float4*>(base + pix * C)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else if constexpr (C % 2 == 0) {
#pragma unroll
        for (int q = 0; q < C / 2; ++q) reinterpret_cast<float2*>(base + pix * C)[q] = make_float2(o[2 * q], o[2 * q + 1]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) base[pix * C + c] = o[c];
    }
}

// soft-max of one pixel; returns the maximum, `best` = arg-max of the LOGITS (first maximum wins, as tf.argmax breaks ties)
template <int C> __device__ __forceinline__ float sl_softmax(const float (&v)[C], float (&sm)[C], int& best, float& se) {
    float mx = v[0];
    best = 0;
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (v[c] > mx) { mx = v[c]; best = c; }
    se = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { sm[c] = expf(v[c] - mx); se += sm[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) sm[c] = sm[c] / se;
    return mx;
}

__device__ __forceinline__ int sl_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- Dice sums: block (x, b) owns SL_TILE pixels of image b -> one partial record ---------------------------------------------
//   fpart[b * nblk + x][2][C] = {sum sm*y, sum sm};  ipart[b * nblk + x][3][C] = {sum y, sum hard*y, sum hard} (exact counts)
template <int C>
__global__ __launch_bounds__(SL_BLOCK) void k_dice_sums(const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                                                        float* __restrict__ fpart, int* __restrict__ ipart, int P) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t img0 = (size_t)b * P;
    float v[SL_PPT][C];
    int lab[SL_PPT];
#pragma unroll
    for (int k = 0; k < SL_PPT; ++k) {                               // loads first
        const int p = blockIdx.x * SL_TILE + k * SL_BLOCK + threadIdx.x;
        lab[k] = -1;
        if (p < P) {
            sl_load<C>(logits, img0 + p, v[k]);
            lab[k] = (int)labels[img0 + p];
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) v[k][c] = 0.f;
        }
    }
    float fi[C], fl[C];
    int cr[C], ci[C], cl[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { fi[c] = fl[c] = 0.f; cr[c] = ci[c] = cl[c] = 0; }
#pragma unroll
    for (int k = 0; k < SL_PPT; ++k) {
        const int p = blockIdx.x * SL_TILE + k * SL_BLOCK + threadIdx.x;
        if (p < P) {
            float sm[C], se;
            int best;
            sl_softmax<C>(v[k], sm, best, se);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool y = c == lab[k], h = c == best;
                fl[c] += sm[c];
                fi[c] += y ? sm[c] : 0.f;
                cr[c] += y ? 1 : 0;
                cl[c] += h ? 1 : 0;
                ci[c] += (y && h) ? 1 : 0;
            }
        }
    }
    __shared__ float sf[SL_BLOCK / 64][2 * C];
    __shared__ int si[SL_BLOCK / 64][3 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a0 = wave_sum(fi[c]), a1 = wave_sum(fl[c]);
        const int b0 = sl_wave_sum_i(cr[c]), b1 = sl_wave_sum_i(ci[c]), b2 = sl_wave_sum_i(cl[c]);
        if (lane == 0) {
            sf[w][c] = a0; sf[w][C + c] = a1;
            si[w][c] = b0; si[w][C + c] = b1; si[w][2 * C + c] = b2;
        }
    }
    __syncthreads();
    const size_t rec = (size_t)b * gridDim.x + blockIdx.x;
    const int t = threadIdx.x;
    if (t < 2 * C) fpart[rec * (2 * C) + t] = (sf[0][t] + sf[1][t]) + (sf[2][t] + sf[3][t]);
    if (t >= 64 && t < 64 + 3 * C) ipart[rec * (3 * C) + (t - 64)] = (si[0][t - 64] + si[1][t - 64]) + (si[2][t - 64] + si[3][t - 64]);
}

// ---- Dice finish: ONE block.  Adds the partial records in block order (double / exact integers) -> sums[b][q][c], then the Dice of
// every (image | batch, class | all classes) group, the table, the scalar loss and the backward coefficients. -----------------------
struct DiceFlags {
    int hard, sol, sob, fg;                        // use_hard_pred (table only), sum_over_labels, sum_over_batches, only_foreground
    double eps, inv_batch;
};
__global__ __launch_bounds__(SL_BLOCK) void k_dice_finish(const float* __restrict__ fpart, const int* __restrict__ ipart,
                                                          double* __restrict__ sums, double* __restrict__ grp, int B, int C, int nblk,
                                                          DiceFlags f, float* __restrict__ table, float* __restrict__ loss,
                                                          float* __restrict__ coef) {
    const int t = threadIdx.x;
    for (int e = t; e < B * SL_NQ * C; e += SL_BLOCK) {
        const int b = e / (SL_NQ * C), q = (e / C) % SL_NQ, c = e % C;
        double a = 0.0;
        if (q < 2) {
            for (int k = 0; k < nblk; ++k) a += (double)fpart[((size_t)b * nblk + k) * (2 * C) + q * C + c];
        } else {
            long long n = 0;
            for (int k = 0; k < nblk; ++k) n += ipart[((size_t)b * nblk + k) * (3 * C) + (q - 2) * C + c];
            a = (double)n;
        }
        sums[e] = a;
    }
    __threadfence_block();
    __syncthreads();
    // group g = (gb, gc): gb = image (one group with sum_over_batches), gc = class (one group with sum_over_labels)
    const int GB = f.sob ? 1 : B, GC = f.sol ? 1 : C;
    for (int g = t; g < GB * GC; g += SL_BLOCK) {
        const int gb = g / GC, gc = g % GC;
        double I = 0, Lq = 0, R = 0, Ih = 0, Lh = 0;
        for (int b = f.sob ? 0 : gb; b < (f.sob ? B : gb + 1); ++b)
            for (int c = f.sol ? 0 : gc; c < (f.sol ? C : gc + 1); ++c) {
                const double* s = sums + (size_t)b * SL_NQ * C + c;
                I += s[0]; Lq += s[C]; R += s[2 * C]; Ih += s[3 * C]; Lh += s[4 * C];
            }
        const double D = Lq + R + f.eps;
        grp[3 * g] = 2.0 * I / D;                   // the soft Dice: what the loss is made of
        grp[3 * g + 1] = D;
        grp[3 * g + 2] = I;
        if (table) table[g] = (float)(f.hard ? 2.0 * Ih / (Lh + R + f.eps) : 2.0 * I / D);
    }
    __threadfence_block();
    __syncthreads();
    const int c0 = (f.fg && !f.sol) ? 1 : 0;       // only_foreground: classes 1 .. C-1 enter the mean
    const double nmean = f.sol ? 1.0 : (double)(C - c0);
    const double k = (f.sob ? f.inv_batch * B : f.inv_batch) / nmean;
    if (coef)
        for (int e = t; e < B * C; e += SL_BLOCK) {
            const int b = e / C, c = e % C, g = (f.sob ? 0 : b) * GC + (f.sol ? 0 : c);
            const double D = grp[3 * g + 1], I = grp[3 * g + 2];
            const bool in = f.sol || c >= c0;
            coef[2 * e] = in ? (float)(-k * 2.0 / D) : 0.f;                  // d loss / d sm[p][c] = alpha * y[p][c] + beta
            coef[2 * e + 1] = in ? (float)(k * 2.0 * I / (D * D)) : 0.f;
        }
    if (loss && t == 0) {
        double acc = 0.0;
        for (int gb = 0; gb < GB; ++gb) {
            double m = 0.0;
            for (int gc = (f.sol ? 0 : c0); gc < GC; ++gc) m += grp[3 * (gb * GC + gc)];
            acc += 1.0 - m / nmean;
        }
        *loss = (float)((f.sob ? f.inv_batch * B : f.inv_batch) * acc);
    }
}

// ---- Dice gradient: dlogits[p][k] (+)= scale * sm[k] * (g[k] - sum_c g[c] sm[c]),  g[c] = alpha[b][c] * y[p][c] + beta[b][c] --------
template <int C, bool ADD>
__global__ __launch_bounds__(SL_BLOCK) void k_dice_grad(const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                                                        const float* __restrict__ coef, float scale, float* __restrict__ dlogits, int P) {
    const int b = blockIdx.y;
    const size_t img0 = (size_t)b * P;
    float al[C], be[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { al[c] = coef[((size_t)b * C + c) * 2]; be[c] = coef[((size_t)b * C + c) * 2 + 1]; }
#pragma unroll
    for (int k = 0; k < SL_PPT; ++k) {
        const int p = blockIdx.x * SL_TILE + k * SL_BLOCK + threadIdx.x;
        if (p >= P) continue;
        float v[C], sm[C], g[C], se;
        int best;
        sl_load<C>(logits, img0 + p, v);
        const int lab = (int)labels[img0 + p];
        sl_softmax<C>(v, sm, best, se);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { g[c] = (c == lab ? al[c] : 0.f) + be[c]; dot += g[c] * sm[c]; }
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = scale * (sm[c] * (g[c] - dot));
        sl_store<C, ADD>(dlogits, img0 + p, g);
    }
}

// ---- cross-entropy family: loss partial per block and the gradient in the same pass --------------------------------------------
//   soft-max form:  sum_p w[label] * (logsumexp - logit[label]),  dlogits (+)= gs * w[label] * (sm - y)
//   sigmoid form:   sum_{p,c} max(x,0) - x*y + log1p(exp(-|x|)),  dlogits (+)= gs * (sigmoid(x) - y)
template <int C, bool ADD, bool SIGMOID>
__global__ __launch_bounds__(SL_BLOCK) void k_seg_xent(const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                                                       const float* __restrict__ cw, float gs, float* __restrict__ part,
                                                       float* __restrict__ dlogits, size_t N) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float wc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) wc[c] = cw ? cw[c] : 1.f;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SL_PPT; ++k) {
        const size_t p = (size_t)blockIdx.x * SL_TILE + k * SL_BLOCK + threadIdx.x;
        if (p >= N) continue;
        float v[C], g[C];
        sl_load<C>(logits, p, v);
        const int lab = (int)labels[p];
        if (SIGMOID) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float x = v[c], y = c == lab ? 1.f : 0.f, e = expf(-fabsf(x));
                acc += fmaxf(x, 0.f) - x * y + log1pf(e);
                const float s = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                g[c] = gs * (s - y);
            }
        } else {
            float sm[C], se, xl = 0.f, wl = 0.f;
            int best;
            const float mx = sl_softmax<C>(v, sm, best, se);
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c == lab) { xl = v[c]; wl = wc[c]; }
            if (lab < C) acc += wl * ((mx - xl) + logf(se));          // (a label >= C has an all-zero one-hot row: no loss, no weight)
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = gs * wl * (sm[c] - (c == lab ? 1.f : 0.f));
        }
        if (dlogits) sl_store<C, ADD>(dlogits, p, g);
    }
    __shared__ float sw[SL_BLOCK / 64];
    acc = wave_sum(acc);
    if (lane == 0) sw[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// ONE block: thread t adds records t, t + 256, ... in double, thread 0 adds the 256 strided sums in order
__global__ __launch_bounds__(SL_BLOCK) void k_seg_xent_finish(const float* __restrict__ part, int nblk, double mul, float* __restrict__ loss) {
    __shared__ double red[SL_BLOCK];
    double a = 0.0;
    for (int k = threadIdx.x; k < nblk; k += SL_BLOCK) a += (double)part[k];
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int q = 0; q < SL_BLOCK; ++q) s += red[q];
    *loss = (float)(s * mul);
}

// ---- adjoint of the nearest-neighbour resize: one thread per coarse element, the f x f block row by row -------------------------
template <bool ADD>
__global__ void k_nn_resize_adjoint(const float* __restrict__ dfine, float* __restrict__ dcoarse, int h, int w, int C, int shift, size_t n) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int c = (int)(e % C);
    const size_t pc = e / C;
    const int x = (int)(pc % w), y = (int)((pc / w) % h);
    const size_t b = pc / ((size_t)w * h);
    const int f = 1 << shift, W = w << shift, H = h << shift;
    const float* src = dfine + ((b * H + ((size_t)y << shift)) * W + ((size_t)x << shift)) * C + c;
    float a = 0.f;
    for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) a += src[((size_t)dy * W + dx) * C];
    dcoarse[e] = ADD ? dcoarse[e] + a : a;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static size_t sl_align(size_t v) { return (v + 255) & ~(size_t)255; }
static bool sl_shape_ok(int B, int H, int W, int C) {
    return B > 0 && H > 0 && W > 0 && C >= 2 && C <= SL_MAXC && B <= 65535 && (size_t)H * W < ((size_t)1 << 31) - SL_TILE &&
           (size_t)B * H * W < ((size_t)1 << 31) * SL_TILE / 2;
}
static int sl_nblk(size_t pixels) { return (int)((pixels + SL_TILE - 1) / SL_TILE); }
static size_t sl_fpart_bytes(int B, int P, int C) { return sl_align((size_t)B * sl_nblk(P) * 2 * C * sizeof(float)); }
static size_t sl_ipart_bytes(int B, int P, int C) { return sl_align((size_t)B * sl_nblk(P) * 3 * C * sizeof(int)); }
static size_t sl_sums_bytes(int B, int C) { return sl_align((size_t)B * SL_NQ * C * sizeof(double)); }
static size_t sl_grp_bytes(int B, int C) { return sl_align((size_t)B * C * 3 * sizeof(double)); }
static bool sl_aligned(const void* p, int C) { return ((uintptr_t)p % (C % 4 == 0 ? 16 : (C % 2 == 0 ? 8 : 4))) == 0; }

#define SL_SWITCH_C(C, ...)                                  \
    switch (C) {                                             \
        case 2: { constexpr int CT = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int CT = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int CT = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int CT = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int CT = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int CT = 7; __VA_ARGS__; } break; \
        default: { constexpr int CT = 8; __VA_ARGS__; } break; \
    }

extern "C" {

size_t phx_dice_ws_bytes(int B, int H, int W, int C) {
    if (!sl_shape_ok(B, H, W, C)) return 0;
    return sl_fpart_bytes(B, H * W, C) + sl_ipart_bytes(B, H * W, C) + sl_sums_bytes(B, C) + sl_grp_bytes(B, C);
}

int phx_dice_sums(const float* logits, const uint8_t* labels, void* workspace, size_t workspace_bytes, int B, int H, int W, int C,
                  void* stream) {
    PHX_REQUIRE(sl_shape_ok(B, H, W, C), PHX_E_INVAL, "dice_sums: fp32 logits [B,H,W,C] with 2 <= C <= 8 (B <= 65535)");
    PHX_REQUIRE(logits != nullptr && labels != nullptr && workspace != nullptr, PHX_E_INVAL, "dice_sums: null pointer");
    PHX_REQUIRE(workspace_bytes >= phx_dice_ws_bytes(B, H, W, C), PHX_E_INVAL, "dice_sums: workspace too small");
    PHX_REQUIRE(sl_aligned(logits, C) && ((uintptr_t)workspace % 8) == 0, PHX_E_ALIGN,
                "dice_sums: logits must be aligned to the vector read of one pixel's classes, the workspace to 8 bytes");
    const int P = H * W;
    float* fpart = (float*)workspace;
    int* ipart = (int*)((char*)workspace + sl_fpart_bytes(B, P, C));
    const dim3 grid((unsigned)sl_nblk(P), (unsigned)B);
    SL_SWITCH_C(C, hipLaunchKernelGGL((k_dice_sums<CT>), grid, dim3(SL_BLOCK), 0, (hipStream_t)stream, logits, labels, fpart, ipart, P));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_dice_finish(void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int use_hard_pred, int sum_over_labels,
                    int sum_over_batches, int only_foreground, float epsilon, float inv_batch, float* dice, float* loss, float* coef,
                    void* stream) {
    PHX_REQUIRE(sl_shape_ok(B, H, W, C), PHX_E_INVAL, "dice_finish: fp32 logits [B,H,W,C] with 2 <= C <= 8 (B <= 65535)");
    PHX_REQUIRE(workspace != nullptr && (dice != nullptr || loss != nullptr || coef != nullptr), PHX_E_INVAL, "dice_finish: null pointer");
    PHX_REQUIRE(workspace_bytes >= phx_dice_ws_bytes(B, H, W, C), PHX_E_INVAL, "dice_finish: workspace too small");
    PHX_REQUIRE(!(only_foreground && sum_over_labels), PHX_E_INVAL,
                "dice_finish: only_foreground needs a label axis (the reference slices [:, 1:] and fails with sum_over_labels)");
    const int P = H * W;
    char* ws = (char*)workspace;
    const float* fpart = (const float*)ws;
    const int* ipart = (const int*)(ws + sl_fpart_bytes(B, P, C));
    double* sums = (double*)(ws + sl_fpart_bytes(B, P, C) + sl_ipart_bytes(B, P, C));
    double* grp = (double*)((char*)sums + sl_sums_bytes(B, C));
    DiceFlags f;
    f.hard = use_hard_pred != 0; f.sol = sum_over_labels != 0; f.sob = sum_over_batches != 0; f.fg = only_foreground != 0;
    f.eps = (double)epsilon; f.inv_batch = (double)inv_batch;
    hipLaunchKernelGGL(k_dice_finish, dim3(1), dim3(SL_BLOCK), 0, (hipStream_t)stream, fpart, ipart, sums, grp, B, C, sl_nblk(P), f, dice,
                       loss, coef);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_dice_grad(const float* logits, const uint8_t* labels, const float* coef, float scale, int add, float* dlogits, int B, int H,
                  int W, int C, void* stream) {
    PHX_REQUIRE(sl_shape_ok(B, H, W, C), PHX_E_INVAL, "dice_grad: fp32 logits [B,H,W,C] with 2 <= C <= 8 (B <= 65535)");
    PHX_REQUIRE(logits != nullptr && labels != nullptr && coef != nullptr && dlogits != nullptr, PHX_E_INVAL, "dice_grad: null pointer");
    PHX_REQUIRE(sl_aligned(logits, C) && sl_aligned(dlogits, C), PHX_E_ALIGN,
                "dice_grad: logits / dlogits must be aligned to the vector access of one pixel's classes");
    const int P = H * W;
    const dim3 grid((unsigned)sl_nblk(P), (unsigned)B);
    if (add) {
        SL_SWITCH_C(C, hipLaunchKernelGGL((k_dice_grad<CT, true>), grid, dim3(SL_BLOCK), 0, (hipStream_t)stream, logits, labels, coef, scale, dlogits, P));
    } else {
        SL_SWITCH_C(C, hipLaunchKernelGGL((k_dice_grad<CT, false>), grid, dim3(SL_BLOCK), 0, (hipStream_t)stream, logits, labels, coef, scale, dlogits, P));
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

size_t phx_seg_xent_ws_bytes(int B, int H, int W, int C) {
    if (!sl_shape_ok(B, H, W, C)) return 0;
    return sl_align((size_t)sl_nblk((size_t)B * H * W) * sizeof(float));
}

int phx_seg_xent(const float* logits, const uint8_t* labels, const float* class_weights, int use_sigmoid, float inv_batch,
                 float grad_scale, int add, float* loss, float* dlogits, void* workspace, size_t workspace_bytes, int B, int H, int W,
                 int C, void* stream) {
    PHX_REQUIRE(sl_shape_ok(B, H, W, C), PHX_E_INVAL, "seg_xent: fp32 logits [B,H,W,C] with 2 <= C <= 8 (B <= 65535)");
    PHX_REQUIRE(logits != nullptr && labels != nullptr && loss != nullptr && workspace != nullptr, PHX_E_INVAL, "seg_xent: null pointer");
    PHX_REQUIRE(!(use_sigmoid && class_weights != nullptr), PHX_E_INVAL, "seg_xent: class weights belong to the soft-max form");
    PHX_REQUIRE(workspace_bytes >= phx_seg_xent_ws_bytes(B, H, W, C), PHX_E_INVAL, "seg_xent: workspace too small");
    PHX_REQUIRE(sl_aligned(logits, C) && (dlogits == nullptr || sl_aligned(dlogits, C)) && ((uintptr_t)workspace % 4) == 0, PHX_E_ALIGN,
                "seg_xent: logits / dlogits must be aligned to the vector access of one pixel's classes");
    const size_t N = (size_t)B * H * W;
    const int nblk = sl_nblk(N);
    // mean over the B*H*W pixels (over B*H*W*C elements in the sigmoid form) of the GLOBAL batch: inv_batch = 1 / (B * world)
    const double mul = (double)inv_batch / ((double)H * W * (use_sigmoid ? C : 1));
    const float gs = (float)((double)grad_scale * mul);
    float* part = (float*)workspace;
    const dim3 grid((unsigned)nblk), block(SL_BLOCK);
#define SL_XENT(ADD, SIG) \
    SL_SWITCH_C(C, hipLaunchKernelGGL((k_seg_xent<CT, ADD, SIG>), grid, block, 0, (hipStream_t)stream, logits, labels, class_weights, gs, part, dlogits, N))
    if (use_sigmoid) { if (add) { SL_XENT(true, true); } else { SL_XENT(false, true); } }
    else { if (add) { SL_XENT(true, false); } else { SL_XENT(false, false); } }
#undef SL_XENT
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_xent_finish, dim3(1), block, 0, (hipStream_t)stream, part, nblk, mul, loss);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_nn_resize_adjoint(const float* dfine, float* dcoarse, int B, int h, int w, int C, int shift, int add, void* stream) {
    PHX_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && shift >= 0 && shift <= 4, PHX_E_INVAL, "nn_resize_adjoint: empty tensor or shift > 4");
    PHX_REQUIRE(dfine != nullptr && dcoarse != nullptr, PHX_E_INVAL, "nn_resize_adjoint: null pointer");
    const size_t n = (size_t)B * h * w * C;
    PHX_REQUIRE((n << (2 * shift)) < ((size_t)1 << 40) && (n + 255) / 256 < ((size_t)1 << 31), PHX_E_INVAL, "nn_resize_adjoint: tensor too large");
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (add) hipLaunchKernelGGL(k_nn_resize_adjoint<true>, grid, block, 0, (hipStream_t)stream, dfine, dcoarse, h, w, C, shift, n);
    else hipLaunchKernelGGL(k_nn_resize_adjoint<false>, grid, block, 0, (hipStream_t)stream, dfine, dcoarse, h, w, C, shift, n);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
