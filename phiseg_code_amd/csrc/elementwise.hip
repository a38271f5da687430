// HBM-bound element-wise kernels of the PHiSeg step: activation gradient, pooling, TF1 bilinear resize, concat/split, add,
// casts, posterior input assembly, global pooling, broadcasts.  (The normalisation layer: norm.hip, norm_bwd.hip, norm_onelaunch.hip.)
// All are streaming kernels: 16-byte vector access along the NHWC channel axis when C % 8 == 0.
#include <stdlib.h>

#include "vec_io.h"

template <typename TD, typename TY, typename TO>
__global__ void k_act_bwd(const TD* __restrict__ dy, const TY* __restrict__ y, TO* __restrict__ dpre, size_t n, int act) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        stf<TO>(dpre, i, ldf<TD>(dy, i) * act_grad_out(ldf<TY>(y, i), act));
}

// =================================================================================================
// tf.nn.avg_pool 2x2 stride 2 SAME
template <typename T, int V>
__global__ void k_avgpool_fwd(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C) {
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, CV = C / V;
    const size_t items = (size_t)B * OH * OW * CV;
    for (size_t it = blockIdx.x * (size_t)blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int cv = (int)(it % CV);
        size_t r = it / CV;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH);
        const int b = (int)(r / OH);
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        int cnt = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int iy = 2 * oy + dy, ix = 2 * ox + dx;
                if (iy < H && ix < W) {
                    float v[V];
                    VecIO<T, V>::load(x, (((size_t)b * H + iy) * W + ix) * C + (size_t)cv * V, v);
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] += v[j];
                    ++cnt;
                }
            }
        const float inv = 1.f / (float)cnt;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] *= inv;
        VecIO<T, V>::store(y, it * V, acc);
    }
}

template <typename T, int V>
__global__ void k_avgpool_bwd(const T* __restrict__ dy, T* __restrict__ dx, int B, int H, int W, int C, int accumulate) {
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, CV = C / V;
    const size_t items = (size_t)B * H * W * CV;
    for (size_t it = blockIdx.x * (size_t)blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int cv = (int)(it % CV);
        size_t r = it / CV;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        const int oy = iy >> 1, ox = ix >> 1;
        const int cnt = ((2 * oy + 1 < H) ? 2 : 1) * ((2 * ox + 1 < W) ? 2 : 1);
        float v[V];
        VecIO<T, V>::load(dy, (((size_t)b * OH + oy) * OW + ox) * C + (size_t)cv * V, v);
        const float inv = 1.f / (float)cnt;
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] *= inv;
        if (accumulate) {                            // dx already holds another reader's gradient contribution
            float o[V];
            VecIO<T, V>::load(dx, it * V, o);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] += o[j];
        }
        VecIO<T, V>::store(dx, it * V, v);
    }
}

// Block order of the two resize kernels.  Their items share rows with their vertical neighbours (the forward pass reads input row
// y0 + 1, the adjoint output rows 2 iy - 1 .. 2 iy + 1), and a row of items is several blocks long -- dispatched round-robin over the
// eight XCDs, neighbouring rows land in different L2s and every shared row is fetched from HBM once per L2 (measured, round 5:
// the adjoint fetched 1.7x, the forward pass 2.1x its input).  Banded: XCD k (blockIdx % 8) walks the k-th contiguous eighth of each
// grid sweep in order, so vertically adjacent items meet in ONE L2 a few blocks apart.  (Any grid that is not a multiple of 8 keeps
// the plain order; the item -> value map does not change, only who computes it.)
__device__ __forceinline__ size_t xcd_banded_block() {
    const unsigned nb = gridDim.x, b = blockIdx.x;
    return (!(PHX_TILE_BANDS & 2) || (nb & 7u)) ? b : (b & 7u) * (nb >> 3) + (b >> 3);
}

// TF 1.12 ResizeBilinear x2, legacy coordinates: out[2k] = in[k], out[2k+1] = (in[k] + in[min(k+1,n-1)])/2
template <typename T, int V>
__global__ void k_bilinear_up2x_fwd(const T* __restrict__ x, T* __restrict__ y, int B, int h, int w, int C) {
    // One item = one channel vector of one INPUT pixel and the 2 x 2 output pixels it anchors (TF1 legacy resize, layers.py:336-345:
    // out[2k] = in[k], out[2k + 1] = (in[k] + in[min(k + 1, n - 1)]) / 2 per axis): four loads for four stores.  (One item per OUTPUT
    // vector re-loaded the four neighbours for each of them and ran at 3.1 TB/s on 64 x 64 x 64 x 192; a copy reaches 6.5.)
    const int OW = 2 * w, CV = C / V;
    const size_t items = (size_t)B * h * w * CV;
    for (size_t it = xcd_banded_block() * (size_t)blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int cv = (int)(it % CV);
        size_t r = it / CV;
        const int x0 = (int)(r % w); r /= w;
        const int y0 = (int)(r % h);
        const size_t base = (r / h) * h;                   // b * h
        const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
        float a[V], bb[V], c[V], d[V], o00[V], o01[V], o10[V], o11[V];
        VecIO<T, V>::load(x, ((base + y0) * w + x0) * C + (size_t)cv * V, a);
        VecIO<T, V>::load(x, ((base + y0) * w + x1) * C + (size_t)cv * V, bb);
        VecIO<T, V>::load(x, ((base + y1) * w + x0) * C + (size_t)cv * V, c);
        VecIO<T, V>::load(x, ((base + y1) * w + x1) * C + (size_t)cv * V, d);
#pragma unroll
        for (int j = 0; j < V; ++j) {                      // (the expressions of the per-output form, fx / fy in {0, 0.5})
            const float top = a[j] + (bb[j] - a[j]) * 0.5f;
            const float bot = c[j] + (d[j] - c[j]) * 0.5f;
            o00[j] = a[j] + (c[j] - a[j]) * 0.f;
            o01[j] = top + (bot - top) * 0.f;
            o10[j] = a[j] + (c[j] - a[j]) * 0.5f;
            o11[j] = top + (bot - top) * 0.5f;
        }
        const size_t orow = ((base * 2 + 2 * y0) * OW + 2 * x0) * C + (size_t)cv * V;
        VecIO<T, V>::store(y, orow, o00);
        VecIO<T, V>::store(y, orow + C, o01);
        VecIO<T, V>::store(y, orow + (size_t)OW * C, o10);
        VecIO<T, V>::store(y, orow + (size_t)OW * C + C, o11);
    }
}

// adjoint (gather): 1-D taps of input k: (2k, 1), (2k+1, 1/2 [+1/2 if k == n-1]), (2k-1, 1/2 if k >= 1)
template <typename T, int V>
__global__ void k_bilinear_up2x_bwd(const T* __restrict__ dy, T* __restrict__ dx, int B, int h, int w, int C, int accumulate) {
    const int OH = 2 * h, OW = 2 * w, CV = C / V;
    const size_t items = (size_t)B * h * w * CV;
    for (size_t it = xcd_banded_block() * (size_t)blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int cv = (int)(it % CV);
        size_t r = it / CV;
        const int ix = (int)(r % w); r /= w;
        const int iy = (int)(r % h);
        const int b = (int)(r / h);
        int ty[3], tx[3];
        float wy[3], wx[3];
        ty[0] = 2 * iy; wy[0] = 1.f;
        ty[1] = 2 * iy + 1; wy[1] = (iy == h - 1) ? 1.f : 0.5f;
        ty[2] = 2 * iy - 1; wy[2] = (iy >= 1) ? 0.5f : 0.f;
        tx[0] = 2 * ix; wx[0] = 1.f;
        tx[1] = 2 * ix + 1; wx[1] = (ix == w - 1) ? 1.f : 0.5f;
        tx[2] = 2 * ix - 1; wx[2] = (ix >= 1) ? 0.5f : 0.f;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        if (accumulate) VecIO<T, V>::load(dx, it * V, acc);
        for (int a = 0; a < 3; ++a) {
            if (wy[a] == 0.f) continue;
            for (int c = 0; c < 3; ++c) {
                if (wx[c] == 0.f) continue;
                float v[V];
                VecIO<T, V>::load(dy, (((size_t)b * OH + ty[a]) * OW + tx[c]) * C + (size_t)cv * V, v);
                const float ww = wy[a] * wx[c];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += ww * v[j];
            }
        }
        VecIO<T, V>::store(dx, it * V, acc);
    }
}

// channel concat / split of two NHWC tensors
template <typename T>
__global__ void k_concat2(const T* __restrict__ a, int Ca, const T* __restrict__ b, int Cb, T* __restrict__ out, size_t npix) {
    const int C = Ca + Cb;
    const size_t n = npix * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / C;
        const int c = (int)(i - p * C);
        out[i] = c < Ca ? a[p * Ca + c] : b[p * Cb + (c - Ca)];
    }
}
template <typename T>
__global__ void k_split2(const T* __restrict__ in, T* __restrict__ a, int Ca, T* __restrict__ b, int Cb, size_t npix) {
    const int C = Ca + Cb;
    const size_t n = npix * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / C;
        const int c = (int)(i - p * C);
        if (c < Ca) { if (a) a[p * Ca + c] = in[i]; }
        else { if (b) b[p * Cb + (c - Ca)] = in[i]; }
    }
}
// 16-byte-chunk variants (Ca, Cb multiples of 8 elements for bf16 / 4 for f32): T16 = uint4
__global__ void k_concat2_v16(const uint4* __restrict__ a, int Ca16, const uint4* __restrict__ b, int Cb16,
                              uint4* __restrict__ out, size_t npix) {
    const int C = Ca16 + Cb16;
    const size_t n = npix * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / C;
        const int c = (int)(i - p * C);
        out[i] = c < Ca16 ? a[p * Ca16 + c] : b[p * Cb16 + (c - Ca16)];
    }
}
__global__ void k_split2_v16(const uint4* __restrict__ in, uint4* __restrict__ a, int Ca16, uint4* __restrict__ b,
                             int Cb16, size_t npix) {
    const int C = Ca16 + Cb16;
    const size_t n = npix * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / C;
        const int c = (int)(i - p * C);
        if (c < Ca16) { if (a) a[p * Ca16 + c] = in[i]; }
        else { if (b) b[p * Cb16 + (c - Ca16)] = in[i]; }
    }
}

template <typename T>
__global__ void k_add_inplace(T* __restrict__ dst, const T* __restrict__ src, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        stf<T>(dst, i, ldf<T>(dst, i) + ldf<T>(src, i));
}
// 8-element vectors (16-byte accesses), four per thread and trip with the loads first (the element-wise form above moved
// 2.4 TB/s); both pointers 16-byte aligned
template <typename T>
__global__ void k_add_inplace_v16(T* __restrict__ dst, const T* __restrict__ src, size_t nvec) {
    constexpr int VE = 8;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        float a[4][VE], b[4][VE];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            VecIO<T, VE>::load(dst, (i + u * stride) * VE, a[u]);
            VecIO<T, VE>::load(src, (i + u * stride) * VE, b[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < VE; ++j) a[u][j] += b[u][j];
            VecIO<T, VE>::store(dst, (i + u * stride) * VE, a[u]);
        }
    }
    for (; i < nvec; i += stride) {
        float a[VE], b[VE];
        VecIO<T, VE>::load(dst, i * VE, a);
        VecIO<T, VE>::load(src, i * VE, b);
#pragma unroll
        for (int j = 0; j < VE; ++j) a[j] += b[j];
        VecIO<T, VE>::store(dst, i * VE, a);
    }
}
template <typename T>
__global__ void k_channel_sum(const T* __restrict__ x, float* __restrict__ out, size_t npix, int C) {
    // block (c-chunk of 64 channels) x pixel slab; lanes along channels for coalescing
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    const int prow = threadIdx.x >> 6;
    float a = 0.f;
    if (c < C)
        for (size_t p = blockIdx.x * 4 + prow; p < npix; p += (size_t)gridDim.x * 4) a += ldf<T>(x, p * C + c);
    __shared__ float sh[256];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (prow == 0 && c < C) atomicAdd(&out[c], sh[threadIdx.x] + sh[threadIdx.x + 64] + sh[threadIdx.x + 128] + sh[threadIdx.x + 192]);
}
// the same sum, 16-byte loads: block = (C / 8 channel vectors) x PL pixel lanes, a chunk of pixels per block
template <typename T>
__global__ void k_channel_sum_v8(const T* __restrict__ x, float* __restrict__ out, size_t npix, int C, int PL, size_t chunk) {
    const int CV = C / 8;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    extern __shared__ float red[];   // [PL][C]
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
    const size_t p0 = blockIdx.x * chunk, p1 = min(npix, p0 + chunk);
    if (pl < PL) {
        size_t p = p0 + pl;
        for (; p + 3 * (size_t)PL < p1; p += 4 * (size_t)PL) {
            float v[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) VecIO<T, 8>::load(x, (p + (size_t)u * PL) * C + (size_t)cv * 8, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] += v[u][j];
        }
        for (; p < p1; p += PL) {
            float v[8];
            VecIO<T, 8>::load(x, p * C + (size_t)cv * 8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += v[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) red[pl * C + cv * 8 + j] = a[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
        float t = 0.f;
        for (int q = 0; q < PL; ++q) t += red[q * C + i];
        atomicAdd(&out[i], t);
    }
}
template <typename TI, typename TO>
__global__ void k_cast(const TI* __restrict__ src, TO* __restrict__ dst, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        stf<TO>(dst, i, ldf<TI>(src, i));
}

template <typename TO>
__global__ void k_posterior_input(const float* __restrict__ x, const uint8_t* __restrict__ s, TO* __restrict__ out,
                                  size_t npix, int nlabels) {
    const int C = 1 + nlabels;
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < npix; p += (size_t)gridDim.x * blockDim.x) {
        stf<TO>(out, p * C, x[p]);
        const int lab = s[p];
        for (int c = 0; c < nlabels; ++c) stf<TO>(out, p * C + 1 + c, (c == lab ? 1.f : 0.f) - 0.5f);
    }
}

// global average pool [B][P][C] -> [B][C] (tiny tensors: one block per (b, c))
__global__ void k_gap_fwd(const float* __restrict__ x, float* __restrict__ y, int P, int C) {
    const int b = blockIdx.x / C, c = blockIdx.x % C;
    float a = 0.f;
    for (int p = threadIdx.x; p < P; p += blockDim.x) a += x[((size_t)b * P + p) * C + c];
    a = wave_sum(a);
    if (threadIdx.x == 0) y[blockIdx.x] = a / (float)P;
}
__global__ void k_gap_bwd(const float* __restrict__ dy, float* __restrict__ dx, int P, int C, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t b = i / ((size_t)P * C);
        dx[i] = dy[b * C + c] / (float)P;
    }
}
template <typename TO>
__global__ void k_bcast_fwd(const float* __restrict__ z, TO* __restrict__ out, int P, int C, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t b = i / ((size_t)P * C);
        stf<TO>(out, i, z[b * C + c]);
    }
}
template <typename T>
__global__ void k_bcast_bwd(const T* __restrict__ dout, float* __restrict__ dz, int P, int C) {
    const int b = blockIdx.x / C, c = blockIdx.x % C;
    float a = 0.f;
    for (int p = threadIdx.x; p < P; p += blockDim.x) a += ldf<T>(dout, ((size_t)b * P + p) * C + c);
    __shared__ float sh[4];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
        dz[blockIdx.x] = t;
    }
}

// =================================================================================================
extern "C" {

int phx_act_bwd(const void* dy, int dy_dt, const void* y, int y_dt, void* dpre, int dpre_dt, size_t n, int act,
                void* stream) {
    PHX_REQUIRE(dy_dt == dpre_dt, PHX_E_INVAL, "act_bwd: dy and dpre dtypes must match");
    PHX_DT_SWITCH(dy_dt, TD, PHX_DT_SWITCH(y_dt, TY, {
        hipLaunchKernelGGL((k_act_bwd<TD, TY, TD>), dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const TD*)dy, (const TY*)y, (TD*)dpre, n, act);
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

#define PHX_SPATIAL_LAUNCH(kern, items_expr, ...)                                                              \
    PHX_DT_SWITCH(dt, T, PHX_VEC_SWITCH(C, V, {                                                                \
        const size_t items = (items_expr) * (size_t)(C / V);                                                   \
        int grid_ = phx_grid_for(items, 256);                                                                  \
        if (grid_ > 8) grid_ = (grid_ + 7) & ~7;          /* whole XCD rounds (xcd_banded_block) */             \
        hipLaunchKernelGGL((kern<T, V>), dim3(grid_), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);         \
    }));                                                                                                       \
    PHX_CHECK_LAUNCH();                                                                                        \
    return PHX_OK;

int phx_avgpool2x2_fwd(const void* x, int dt, void* y, int B, int H, int W, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_avgpool_fwd, (size_t)B * ((H + 1) / 2) * ((W + 1) / 2), (const T*)x, (T*)y, B, H, W, C)
}
int phx_avgpool2x2_bwd(const void* dy, int dt, void* dx, int B, int H, int W, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_avgpool_bwd, (size_t)B * H * W, (const T*)dy, (T*)dx, B, H, W, C, 0)
}
int phx_avgpool2x2_bwd_acc(const void* dy, int dt, void* dx, int B, int H, int W, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_avgpool_bwd, (size_t)B * H * W, (const T*)dy, (T*)dx, B, H, W, C, 1)
}
int phx_bilinear_up2x_fwd(const void* x, int dt, void* y, int B, int h, int w, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_bilinear_up2x_fwd, (size_t)B * h * w, (const T*)x, (T*)y, B, h, w, C)
}
int phx_bilinear_up2x_bwd(const void* dy, int dt, void* dx, int B, int h, int w, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_bilinear_up2x_bwd, (size_t)B * h * w, (const T*)dy, (T*)dx, B, h, w, C, 0)
}
int phx_bilinear_up2x_bwd_acc(const void* dy, int dt, void* dx, int B, int h, int w, int C, void* stream) {
    PHX_SPATIAL_LAUNCH(k_bilinear_up2x_bwd, (size_t)B * h * w, (const T*)dy, (T*)dx, B, h, w, C, 1)
}

int phx_concat2(const void* a, int Ca, const void* b, int Cb, void* out, size_t npix, int dt, void* stream) {
    const int es = dt == PHX_BF16 ? 2 : 4, per16 = 16 / es;
    if (Ca % per16 == 0 && Cb % per16 == 0) {
        const size_t n = npix * (size_t)((Ca + Cb) / per16);
        hipLaunchKernelGGL(k_concat2_v16, dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)a,
                           Ca / per16, (const uint4*)b, Cb / per16, (uint4*)out, npix);
    } else {
        PHX_DT_SWITCH(dt, T, {
            hipLaunchKernelGGL((k_concat2<T>), dim3(phx_grid_for(npix * (Ca + Cb), 256)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)a, Ca, (const T*)b, Cb, (T*)out, npix);
        });
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_split2(const void* in, void* a, int Ca, void* b, int Cb, size_t npix, int dt, void* stream) {
    const int es = dt == PHX_BF16 ? 2 : 4, per16 = 16 / es;
    if (Ca % per16 == 0 && Cb % per16 == 0) {
        const size_t n = npix * (size_t)((Ca + Cb) / per16);
        hipLaunchKernelGGL(k_split2_v16, dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)in,
                           (uint4*)a, Ca / per16, (uint4*)b, Cb / per16, npix);
    } else {
        PHX_DT_SWITCH(dt, T, {
            hipLaunchKernelGGL((k_split2<T>), dim3(phx_grid_for(npix * (Ca + Cb), 256)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)in, (T*)a, Ca, (T*)b, Cb, npix);
        });
    }
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_add_inplace(void* dst, const void* src, size_t n, int dt, void* stream) {
    const size_t ve = 8;
    if (n >= 4096 && n % ve == 0 && ((uintptr_t)dst | (uintptr_t)src) % 16 == 0) {
        const size_t nvec = n / ve;
        size_t blocks = (nvec + 256 * 4 - 1) / (256 * 4);           // four vectors per thread
        if (blocks > 4096) blocks = 4096;
        PHX_DT_SWITCH(dt, T, {
            hipLaunchKernelGGL((k_add_inplace_v16<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (T*)dst,
                               (const T*)src, nvec);
        });
        PHX_CHECK_LAUNCH();
        return PHX_OK;
    }
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_add_inplace<T>), dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (T*)dst,
                           (const T*)src, n);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_channel_sum_accumulate(const void* x, int dt, float* out, size_t npix, int C, void* stream) {
    if (C % 8 == 0 && C / 8 <= 256 && npix >= 64) {
        const int CV = C / 8, PL = 256 / CV, threads = CV * PL;
        size_t rows = (npix + PL - 1) / PL;
        size_t want = (rows + 31) / 32;                   // ~32 pixels per thread, at least 64 and at most 1024 blocks
        if (want < 64) want = rows < 64 ? rows : 64;
        if (want > 1024) want = 1024;
        if (phx_deterministic()) want = 1;
        const size_t chunk = (npix + want - 1) / want;
        const int nchunks = (int)((npix + chunk - 1) / chunk);
        PHX_DT_SWITCH(dt, T, {
            hipLaunchKernelGGL((k_channel_sum_v8<T>), dim3(nchunks), dim3(threads), (size_t)PL * C * sizeof(float), (hipStream_t)stream,
                               (const T*)x, out, npix, C, PL, chunk);
        });
        PHX_CHECK_LAUNCH();
        return PHX_OK;
    }
    int gx = (int)((npix + 63) / 64);
    if (gx > 256) gx = 256;
    if (gx < 1 || phx_deterministic()) gx = 1;
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_channel_sum<T>), dim3(gx, (C + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const T*)x, out,
                           npix, C);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_cast(const void* src, int src_dt, void* dst, int dst_dt, size_t n, void* stream) {
    PHX_DT_SWITCH(src_dt, TI, PHX_DT_SWITCH(dst_dt, TO, {
        hipLaunchKernelGGL((k_cast<TI, TO>), dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const TI*)src, (TO*)dst, n);
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_posterior_input(const float* x, const uint8_t* s, void* out, int out_dt, size_t npix, int nlabels, void* stream) {
    PHX_DT_SWITCH(out_dt, TO, {
        hipLaunchKernelGGL((k_posterior_input<TO>), dim3(phx_grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, x,
                           s, (TO*)out, npix, nlabels);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_global_avgpool_fwd(const float* x, float* y, int B, int P, int C, void* stream) {
    hipLaunchKernelGGL(k_gap_fwd, dim3(B * C), dim3(64), 0, (hipStream_t)stream, x, y, P, C);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_global_avgpool_bwd(const float* dy, float* dx, int B, int P, int C, void* stream) {
    const size_t n = (size_t)B * P * C;
    hipLaunchKernelGGL(k_gap_bwd, dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, P, C, n);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
// out[b * n + k][:] = x[b][:] for k < n: every image's feature map repeated for its n Monte-Carlo samples (16-byte pieces)
__global__ void k_repeat_rows16(const uint4* __restrict__ x, uint4* __restrict__ out, size_t per16, int n, size_t total16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total16; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / per16, e = i - row * per16;
        out[i] = x[(row / n) * per16 + e];
    }
}
int phx_repeat_batch(const void* x, void* out, int B, size_t bytes_per_sample, int n, void* stream) {
    PHX_REQUIRE(bytes_per_sample % 16 == 0 && n >= 1, PHX_E_SHAPE, "repeat_batch: sample size must be a multiple of 16 bytes");
    PHX_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, PHX_E_ALIGN, "repeat_batch: 16-byte alignment");
    const size_t per16 = bytes_per_sample / 16, total16 = per16 * B * n;
    hipLaunchKernelGGL(k_repeat_rows16, dim3(phx_grid_for(total16, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x,
                       (uint4*)out, per16, n, total16);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_broadcast_pixels_fwd(const float* z, void* out, int out_dt, int B, int P, int C, void* stream) {
    const size_t n = (size_t)B * P * C;
    PHX_DT_SWITCH(out_dt, TO, {
        hipLaunchKernelGGL((k_bcast_fwd<TO>), dim3(phx_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, z, (TO*)out,
                           P, C, n);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}
int phx_broadcast_pixels_bwd(const void* dout, int dt, float* dz, int B, int P, int C, void* stream) {
    PHX_DT_SWITCH(dt, T, {
        hipLaunchKernelGGL((k_bcast_bwd<T>), dim3(B * C), dim3(256), 0, (hipStream_t)stream, (const T*)dout, dz, P, C);
    });
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
