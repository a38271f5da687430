// 16-byte vector access along the NHWC channel axis, shared by the streaming units (elementwise.hip, norm*.hip).
#pragma once
#include "phx_common.h"

// ---- 8-wide vector access ----------------------------------------------------------------------
template <typename T, int V> struct VecIO;
template <> struct VecIO<float, 8> {
    static __device__ __forceinline__ void load(const float* p, size_t i, float o[8]) {
        const float4* q = reinterpret_cast<const float4*>(p + i);
        float4 a = q[0], b = q[1];
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    }
    static __device__ __forceinline__ void store(float* p, size_t i, const float o[8]) {
        float4* q = reinterpret_cast<float4*>(p + i);
        q[0] = make_float4(o[0], o[1], o[2], o[3]);
        q[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
};
template <> struct VecIO<bf16_t, 8> {
    static __device__ __forceinline__ void load(const bf16_t* p, size_t i, float o[8]) {
        uint4 r = *reinterpret_cast<const uint4*>(p + i);
        unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = __uint_as_float(w[k] << 16);
            o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(bf16_t* p, size_t i, const float o[8]) {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = f2bf_pk(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<uint4*>(p + i) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};
template <typename T> struct VecIO<T, 1> {
    static __device__ __forceinline__ void load(const T* p, size_t i, float o[1]) { o[0] = ldf<T>(p, i); }
    static __device__ __forceinline__ void store(T* p, size_t i, const float o[1]) { stf<T>(p, i, o[0]); }
};

#define PHX_VEC_SWITCH(C, V, ...)                         \
    do {                                                  \
        if ((C) % 8 == 0) { constexpr int V = 8; __VA_ARGS__; } \
        else { constexpr int V = 1; __VA_ARGS__; }        \
    } while (0)

// eight packed bf16 (one 16-byte register quad) -> fp32
__device__ __forceinline__ void bf16x8_unpack(const uint4& r, float o[8]) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[2 * k] = __uint_as_float(w[k] << 16);
        o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}
