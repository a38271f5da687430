// Leaky ReLU as a stream of its own (tfwrapper/activations.py:8-9: tf.maximum(x, alpha * x)); DESIGN.md section 7i.
//   forward   y    = x >= alpha x ? x : alpha x        (one fp32 multiply, one rounding to the storage type)
//   backward  dpre = y >= 0 ? dy : alpha dy            (TF's MaximumGrad: the whole gradient to the first argument on a tie, x == 0)
// Both are HBM-bound: an item is V = 4 (all streams fp32) or 8 (any stream bf16) consecutive elements, one 16-byte access per bf16
// stream and one or two per fp32 stream; a capped grid walks the items with a grid stride.  The first `head` elements and the
// n - head - nvec V last ones are done one by one by the first threads, so neither n nor the pointers need to be multiples of the
// vector: the host picks the head that brings EVERY stream to a 16-byte boundary, and launches the element-by-element form (V = 1)
// when the streams' offsets from a boundary disagree.  A thread writes only the elements it has read, so y == x and dpre == dy are
// safe (no __restrict__ on those); there are no atomics and no cross-thread sums: the same bits in every mode and from run to run.
#include "phx_common.h"

namespace {

constexpr int LR_BLOCK = 256;
constexpr int LR_MAX_BLOCKS = 2048;          // 8 blocks on each of the 256 CUs; the grid stride takes the rest

// V consecutive elements at p[i ..], p + i on a 16-byte boundary
template <typename T, int V> struct LrVec;
template <int V> struct LrVecF32 {
    static __device__ __forceinline__ void load(const float* p, size_t i, float o[V]) {
#pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            const float4 a = reinterpret_cast<const float4*>(p + i)[k];
            o[4 * k] = a.x; o[4 * k + 1] = a.y; o[4 * k + 2] = a.z; o[4 * k + 3] = a.w;
        }
    }
    static __device__ __forceinline__ void store(float* p, size_t i, const float o[V]) {
#pragma unroll
        for (int k = 0; k < V / 4; ++k)
            reinterpret_cast<float4*>(p + i)[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
};
template <> struct LrVec<float, 4> : LrVecF32<4> {};
template <> struct LrVec<float, 8> : LrVecF32<8> {};
template <> struct LrVec<bf16_t, 8> {
    static __device__ __forceinline__ void load(const bf16_t* p, size_t i, float o[8]) {
        const uint4 r = *reinterpret_cast<const uint4*>(p + i);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = __uint_as_float(w[k] << 16);
            o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(bf16_t* p, size_t i, const float o[8]) {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (unsigned)f2bf(o[2 * k]) | ((unsigned)f2bf(o[2 * k + 1]) << 16);   // stf<bf16_t>'s rounding
        *reinterpret_cast<uint4*>(p + i) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};
template <typename T> struct LrVec<T, 1> {
    static __device__ __forceinline__ void load(const T* p, size_t i, float o[1]) { o[0] = ldf<T>(p, i); }
    static __device__ __forceinline__ void store(T* p, size_t i, const float o[1]) { stf<T>(p, i, o[0]); }
};

__device__ __forceinline__ float leaky_fwd(float x, float alpha) {
    const float ax = alpha * x;
    return x >= ax ? x : ax;                 // (a NaN goes through the second arm)
}
__device__ __forceinline__ float leaky_bwd(float dy, float y, float alpha) { return y >= 0.f ? dy : dy * alpha; }

// the scalar edges of a launch: elements [0, head) and [head + nvec V, n), fewer than 2 V in all -> thread t takes edge element t
__device__ __forceinline__ bool lr_edge(size_t t, size_t n, size_t head, size_t body, size_t* i) {
    if (t < head) { *i = t; return true; }
    const size_t e = head + body + (t - head);
    if (e < n) { *i = e; return true; }
    return false;
}

template <typename TX, typename TY, int V>
__global__ void __launch_bounds__(LR_BLOCK) k_leaky_relu_fwd(const TX* x, TY* y, size_t n, size_t head, float alpha) {
    const size_t nvec = (n - head) / V, tid = blockIdx.x * (size_t)LR_BLOCK + threadIdx.x;
    size_t e;
    if (tid < 2 * V && lr_edge(tid, n, head, nvec * V, &e)) stf<TY>(y, e, leaky_fwd(ldf<TX>(x, e), alpha));
    for (size_t it = tid; it < nvec; it += (size_t)gridDim.x * LR_BLOCK) {
        float v[V];
        LrVec<TX, V>::load(x, head + it * V, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = leaky_fwd(v[j], alpha);
        LrVec<TY, V>::store(y, head + it * V, v);
    }
}

template <typename TD, typename TY, int V>
__global__ void __launch_bounds__(LR_BLOCK) k_leaky_relu_bwd(const TD* dy, const TY* y, TD* dpre, size_t n, size_t head, float alpha) {
    const size_t nvec = (n - head) / V, tid = blockIdx.x * (size_t)LR_BLOCK + threadIdx.x;
    size_t e;
    if (tid < 2 * V && lr_edge(tid, n, head, nvec * V, &e)) stf<TD>(dpre, e, leaky_bwd(ldf<TD>(dy, e), ldf<TY>(y, e), alpha));
    for (size_t it = tid; it < nvec; it += (size_t)gridDim.x * LR_BLOCK) {
        float d[V], o[V];
        LrVec<TD, V>::load(dy, head + it * V, d);
        LrVec<TY, V>::load(y, head + it * V, o);
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = leaky_bwd(d[j], o[j], alpha);
        LrVec<TD, V>::store(dpre, head + it * V, d);
    }
}

inline int lr_esize(int dt) { return dt == PHX_BF16 ? 2 : 4; }

// The number of leading elements (< V) after which every stream sits on a 16-byte boundary, or -1 when no such number exists.
inline int lr_head(const void* const* ptrs, const int* dts, int count, int V) {
    for (int h = 0; h < V; ++h) {
        bool ok = true;
        for (int k = 0; k < count; ++k) ok = ok && ((uintptr_t)ptrs[k] + (size_t)h * lr_esize(dts[k])) % 16 == 0;
        if (ok) return h;
    }
    return -1;
}

inline int lr_grid(size_t items) {
    int g = phx_grid_for(items, LR_BLOCK, LR_MAX_BLOCKS);
    if (g > 8) g = (g + 7) & ~7;             // whole rounds over the eight XCDs
    return g;
}

inline bool lr_alpha_ok(float alpha) { return alpha > 0.f && alpha < 1.f; }      // (false for a NaN)

}  // namespace

extern "C" {

int phx_leaky_relu_fwd(const void* x, int x_dt, void* y, int y_dt, size_t n, float alpha, void* stream) {
    PHX_REQUIRE(lr_alpha_ok(alpha), PHX_E_INVAL, "leaky_relu_fwd: alpha must lie in (0, 1)");
    PHX_REQUIRE((x_dt == PHX_F32 || x_dt == PHX_BF16) && (y_dt == PHX_F32 || y_dt == PHX_BF16), PHX_E_INVAL, "leaky_relu_fwd: bad dtype");
    PHX_REQUIRE(n == 0 || (x && y), PHX_E_INVAL, "leaky_relu_fwd: null tensor");
    PHX_REQUIRE((uintptr_t)x % lr_esize(x_dt) == 0 && (uintptr_t)y % lr_esize(y_dt) == 0, PHX_E_INVAL,
                "leaky_relu_fwd: a pointer is not aligned to its element");
    const int V = (x_dt == PHX_F32 && y_dt == PHX_F32) ? 4 : 8;
    const void* ptrs[2] = {x, y};
    const int dts[2] = {x_dt, y_dt};
    const int h = lr_head(ptrs, dts, 2, V);
    PHX_DT_SWITCH(x_dt, TX, PHX_DT_SWITCH(y_dt, TY, {
        constexpr int VV = (sizeof(TX) == 4 && sizeof(TY) == 4) ? 4 : 8;
        if (h >= 0 && n >= (size_t)h + VV) {
            hipLaunchKernelGGL((k_leaky_relu_fwd<TX, TY, VV>), dim3(lr_grid((n - h) / VV)), dim3(LR_BLOCK), 0, (hipStream_t)stream,
                               (const TX*)x, (TY*)y, n, (size_t)h, alpha);
        } else {                             // offsets that no common head aligns, or fewer elements than a head and a vector
            hipLaunchKernelGGL((k_leaky_relu_fwd<TX, TY, 1>), dim3(lr_grid(n)), dim3(LR_BLOCK), 0, (hipStream_t)stream,
                               (const TX*)x, (TY*)y, n, (size_t)0, alpha);
        }
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_leaky_relu_bwd(const void* dy, int dy_dt, const void* y, int y_dt, void* dpre, int dpre_dt, size_t n, float alpha,
                       void* stream) {
    PHX_REQUIRE(lr_alpha_ok(alpha), PHX_E_INVAL, "leaky_relu_bwd: alpha must lie in (0, 1)");
    PHX_REQUIRE(dy_dt == dpre_dt, PHX_E_INVAL, "leaky_relu_bwd: dy and dpre dtypes must match");
    PHX_REQUIRE((dy_dt == PHX_F32 || dy_dt == PHX_BF16) && (y_dt == PHX_F32 || y_dt == PHX_BF16), PHX_E_INVAL, "leaky_relu_bwd: bad dtype");
    PHX_REQUIRE(n == 0 || (dy && y && dpre), PHX_E_INVAL, "leaky_relu_bwd: null tensor");
    PHX_REQUIRE((uintptr_t)dy % lr_esize(dy_dt) == 0 && (uintptr_t)y % lr_esize(y_dt) == 0 && (uintptr_t)dpre % lr_esize(dy_dt) == 0,
                PHX_E_INVAL, "leaky_relu_bwd: a pointer is not aligned to its element");
    const int V = (dy_dt == PHX_F32 && y_dt == PHX_F32) ? 4 : 8;
    const void* ptrs[3] = {dy, y, dpre};
    const int dts[3] = {dy_dt, y_dt, dpre_dt};
    const int h = lr_head(ptrs, dts, 3, V);
    PHX_DT_SWITCH(dy_dt, TD, PHX_DT_SWITCH(y_dt, TY, {
        constexpr int VV = (sizeof(TD) == 4 && sizeof(TY) == 4) ? 4 : 8;
        if (h >= 0 && n >= (size_t)h + VV) {
            hipLaunchKernelGGL((k_leaky_relu_bwd<TD, TY, VV>), dim3(lr_grid((n - h) / VV)), dim3(LR_BLOCK), 0, (hipStream_t)stream,
                               (const TD*)dy, (const TY*)y, (TD*)dpre, n, (size_t)h, alpha);
        } else {
            hipLaunchKernelGGL((k_leaky_relu_bwd<TD, TY, 1>), dim3(lr_grid(n)), dim3(LR_BLOCK), 0, (hipStream_t)stream,
                               (const TD*)dy, (const TY*)y, (TD*)dpre, n, (size_t)0, alpha);
        }
    }));
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
