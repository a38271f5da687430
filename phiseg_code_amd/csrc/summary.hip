// TensorBoard summaries formed on the device (phiseg_model.py:199-203, 662-818 of the reference): the histograms TensorFlow's CPU
// HistogramSummary op builds from tensors pulled to the host, and put_kernels_on_grid (tfwrapper/utils.py:93-168), beside the buffers.
// Only the bucket counts (12 KB per histogram) and the finished uint8 grids travel to the host.  DESIGN.md section 7b.
#include "phx_common.h"

namespace {

constexpr int SH_NB = PHX_SUMMARY_BUCKETS;     // 1551 buckets = limits
constexpr int SH_NPOS = 775;                   // positive limits: 774 of the geometric ladder + DBL_MAX
constexpr int SH_ZERO = 776;                   // the bucket of +-0.0: first limit above it is limits[776] = 1e-12
constexpr int SH_BLOCK = 256;
constexpr int SH_MAXBX = 512;                  // blocks per segment at most
constexpr size_t SH_MINCHUNK = 16384;          // elements per block at least (64 per thread)

// float -> unsigned key whose unsigned order is the float order (-0.0 below +0.0)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// per-segment raw accumulators (work area); both keys start at 0 and only grow, so one memset initialises them
struct SegAcc {
    unsigned maxkey;        // max of f2key(v)
    unsigned minkey_inv;    // max of ~f2key(v)
    unsigned long long nfinite, nonfinite;
};

// Number of positive limits pos[0 .. 773] that are <= a (strict: < a), a > 0 finite.  The ladder is pos[k] ~ 1e-12 * 1.1^k, so
// k ~ log(a / 1e-12) / log(1.1) to within a unit from a single-precision log2; the answer is then made EXACT by comparing a against
// the neighbouring table entries in double -- the table is the one the host built by repeated multiplication, nothing is recomputed
// here.  pos[774] = DBL_MAX is never reached by a widened float.
template <bool STRICT>
__device__ __forceinline__ int ladder_count(const double* __restrict__ pos, float af, double a) {
    const float t = (__log2f(af) + 39.863137f) * 7.2725409f;       // (log2 a - log2 1e-12) / log2 1.1; a denormal gives -inf
    int j = (int)fminf(fmaxf(t, 0.f), 773.f) + 1;                  // estimate of the count, 1 .. 774
    if (STRICT) {
        while (j < 774 && pos[j] < a) ++j;
        while (j > 0 && !(pos[j - 1] < a)) --j;
    } else {
        while (j < 774 && pos[j] <= a) ++j;
        while (j > 0 && !(pos[j - 1] <= a)) --j;
    }
    return j;
}

// bucket = index of the first limit strictly greater than (double)v = number of limits <= v (std::upper_bound)
__device__ __forceinline__ int bucket_of(const double* __restrict__ pos, float v) {
    if (v == 0.f) return SH_ZERO;
    const float af = fabsf(v);
    const double a = (double)af;
    if (v > 0.f) return SH_ZERO + ladder_count<false>(pos, af, a);           // the 775 negative limits, 0.0, and the ladder up to v
    return SH_NPOS - ladder_count<true>(pos, af, a);                         // -pos[k] <= v  <=>  pos[k] >= a
}

struct Lane {
    unsigned zeros, nonfinite;
    float mn, mx;
    double s, ss;
};

__device__ __forceinline__ void take(Lane& L, unsigned* hist, const double* pos, float v) {
    if (v == 0.f) {                       // the dominant bucket of a post-ReLU tensor: counted in a register, never in LDS
        ++L.zeros;
        L.mn = fminf(L.mn, v);
        L.mx = fmaxf(L.mx, v);
        return;
    }
    if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) {
        ++L.nonfinite;
        return;
    }
    L.mn = fminf(L.mn, v);
    L.mx = fmaxf(L.mx, v);
    const double d = (double)v;
    L.s += d;
    L.ss += d * d;
    atomicAdd(&hist[bucket_of(pos, v)], 1u);
}

__global__ void __launch_bounds__(SH_BLOCK) k_summary_hist(const phx_summary_segment* __restrict__ segs, const double* __restrict__ limits,
                                                           unsigned long long* __restrict__ counts, double* __restrict__ stats,
                                                           SegAcc* __restrict__ acc) {
    __shared__ double pos[SH_NPOS];
    __shared__ unsigned hist[SH_NB];
    __shared__ double red[2][SH_BLOCK / 64];
    __shared__ unsigned redu[4][SH_BLOCK / 64];
    const int seg = blockIdx.y, tid = threadIdx.x;
    const phx_summary_segment sg = segs[seg];
    const size_t n = (size_t)sg.n;
    // this segment's share of the launch: nb blocks of `chunk` elements (a multiple of 1024, so every block starts on a 16-byte
    // boundary of an aligned segment); the remaining blocks of the row leave at once
    size_t nb = (n + SH_MINCHUNK - 1) / SH_MINCHUNK;
    if (nb > gridDim.x) nb = gridDim.x;
    if (blockIdx.x >= nb) return;
    const size_t chunk = ((n + nb - 1) / nb + 1023) / 1024 * 1024;
    const size_t beg = (size_t)blockIdx.x * chunk;
    if (beg >= n) return;
    const size_t end = beg + chunk < n ? beg + chunk : n;

    for (int i = tid; i < SH_NPOS; i += SH_BLOCK) pos[i] = limits[SH_ZERO + i];
    for (int i = tid; i < SH_NB; i += SH_BLOCK) hist[i] = 0u;
    __syncthreads();

    Lane L;
    L.zeros = L.nonfinite = 0u;
    L.mn = INFINITY;
    L.mx = -INFINITY;
    L.s = L.ss = 0.0;
    const bool aligned = (((uintptr_t)sg.ptr) & 15u) == 0;
    if (sg.dtype == PHX_F32) {
        const float* p = (const float*)sg.ptr;
        size_t i = beg;
        if (aligned) {
            const size_t nv = (end - beg) / 4;
            const float4* p4 = (const float4*)(p + beg);
            for (size_t k = tid; k < nv; k += SH_BLOCK) {
                const float4 q = p4[k];
                take(L, hist, pos, q.x);
                take(L, hist, pos, q.y);
                take(L, hist, pos, q.z);
                take(L, hist, pos, q.w);
            }
            i = beg + nv * 4;
        }
        for (size_t k = i + tid; k < end; k += SH_BLOCK) take(L, hist, pos, p[k]);
    } else {
        const unsigned short* p = (const unsigned short*)sg.ptr;
        size_t i = beg;
        if (aligned) {
            const size_t nv = (end - beg) / 8;
            const uint4* p8 = (const uint4*)(p + beg);
            for (size_t k = tid; k < nv; k += SH_BLOCK) {
                const uint4 q = p8[k];
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    take(L, hist, pos, __uint_as_float(w[j] << 16));
                    take(L, hist, pos, __uint_as_float(w[j] & 0xffff0000u));
                }
            }
            i = beg + nv * 8;
        }
        for (size_t k = i + tid; k < end; k += SH_BLOCK) take(L, hist, pos, bf2f(p[k]));
    }

    // wave totals by shuffles, block totals through LDS, then ONE global atomic per statistic and block
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        L.zeros += __shfl_xor(L.zeros, o, 64);
        L.nonfinite += __shfl_xor(L.nonfinite, o, 64);
        L.mn = fminf(L.mn, __shfl_xor(L.mn, o, 64));
        L.mx = fmaxf(L.mx, __shfl_xor(L.mx, o, 64));
        L.s += __shfl_xor(L.s, o, 64);
        L.ss += __shfl_xor(L.ss, o, 64);
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        if (L.zeros) atomicAdd(&hist[SH_ZERO], L.zeros);
        red[0][wave] = L.s;
        red[1][wave] = L.ss;
        redu[0][wave] = L.nonfinite;
        redu[1][wave] = f2key(L.mx);          // (-inf where the wave saw no finite value: below every finite key)
        redu[2][wave] = ~f2key(L.mn);
    }
    __syncthreads();
    unsigned long long nfin = 0;
    for (int i = tid; i < SH_NB; i += SH_BLOCK) {
        const unsigned c = hist[i];
        if (c) {                              // a block of one tensor touches a few dozen neighbouring buckets: flush only those
            atomicAdd(&counts[(size_t)seg * SH_NB + i], (unsigned long long)c);
            nfin += c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nfin += __shfl_xor(nfin, o, 64);
    if ((tid & 63) == 0 && nfin) atomicAdd(&acc[seg].nfinite, nfin);
    if (tid == 0) {
        double s = 0.0, ss = 0.0;
        unsigned nf = 0, kmx = 0, kmn = 0;
        for (int w = 0; w < SH_BLOCK / 64; ++w) {
            s += red[0][w];
            ss += red[1][w];
            nf += redu[0][w];
            kmx = max(kmx, redu[1][w]);
            kmn = max(kmn, redu[2][w]);
        }
        atomicAdd(&stats[(size_t)seg * PHX_SUMMARY_NSTATS + PHX_SUMMARY_SUM], s);
        atomicAdd(&stats[(size_t)seg * PHX_SUMMARY_NSTATS + PHX_SUMMARY_SUM_SQUARES], ss);
        if (nf) atomicAdd(&acc[seg].nonfinite, (unsigned long long)nf);
        atomicMax(&acc[seg].maxkey, kmx);
        atomicMax(&acc[seg].minkey_inv, kmn);
    }
}

__global__ void k_summary_hist_final(const SegAcc* __restrict__ acc, double* __restrict__ stats, int nseg) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const SegAcc a = acc[s];
    double* o = stats + (size_t)s * PHX_SUMMARY_NSTATS;
    const bool any = a.nfinite != 0;
    o[PHX_SUMMARY_MIN] = any ? (double)key2f(~a.minkey_inv) : 0.0;
    o[PHX_SUMMARY_MAX] = any ? (double)key2f(a.maxkey) : 0.0;
    o[PHX_SUMMARY_NUM] = (double)a.nfinite;
    o[PHX_SUMMARY_NONFINITE] = (double)a.nonfinite;
}

// ---- put_kernels_on_grid -------------------------------------------------------------------------------------------------------
// the displayed value of stored pixel `pix`: the arg-max over C (first maximum wins), the label, or the intensity
__device__ __forceinline__ float grid_value(const void* __restrict__ src, int form, size_t pix, int C) {
    if (form == PHX_GRID_LABELS_U8) return (float)((const unsigned char*)src)[pix];
    if (form == PHX_GRID_IMAGE_F32) return ((const float*)src)[pix];
    const float* p = (const float*)src + pix * C;
    int best = 0;
    float bv = p[0];
    for (int c = 1; c < C; ++c) {
        const float v = p[c];
        if (v > bv || (bv != bv && v == v)) {      // np.argmax / tf.argmax: first maximum (a NaN only loses to a number here: deliberate)
            bv = v;
            best = c;
        }
    }
    return (float)best;
}

// (over the pixels of the STORED tensor: a nearest-neighbour view has the same extrema as its expansion)
__global__ void __launch_bounds__(256) k_grid_minmax(const void* __restrict__ src, int form, size_t npix, int C, unsigned* __restrict__ keys) {
    __shared__ unsigned red[2][4];
    float mn = INFINITY, mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const float x = grid_value(src, form, i, C);
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = f2key(mx);
        red[1][threadIdx.x >> 6] = ~f2key(mn);
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

__global__ void __launch_bounds__(256) k_grid_write(const void* __restrict__ src, int form, int H, int W, int C, int sh, int gy_n, int gx_n,
                                                    const unsigned* __restrict__ keys, unsigned char* __restrict__ out) {
    const int Y = H + 2, X = W + 2;
    const size_t rows = (size_t)Y * gy_n, cols = (size_t)X * gx_n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i % cols);
    const int gy = r / Y, y = r % Y, gx = c / X, x = c % X;
    unsigned char o = 0;                                            // the pad of 1 around every tile
    if (y > 0 && y < Y - 1 && x > 0 && x < X - 1) {
        const float mx = key2f(keys[0]), mn = key2f(~keys[1]);
        // `sh`: the buffer is a nearest-neighbour view stored at (H >> sh) x (W >> sh)
        const float v = grid_value(src, form, ((size_t)(gx * gy_n + gy) * (H >> sh) + ((y - 1) >> sh)) * (W >> sh) + ((x - 1) >> sh), C);
        float f = v - mn;                                           // the reference's 'image' branch, step by step in fp32
        f = f / mx;
        f = f * 254.0f;
        o = !(f == f) ? 0 : (f <= 0.f ? 0 : (f >= 255.f ? 255 : (unsigned char)f));     // NaN -> 0, saturate, else truncate
    }
    out[i] = o;
}

}  // namespace

extern "C" {

size_t phx_summary_histograms_ws_bytes(int nseg) { return nseg > 0 ? (size_t)nseg * sizeof(SegAcc) : 0; }

int phx_summary_histograms(const phx_summary_segment* segs, int nseg, uint64_t max_n, const double* limits, unsigned long long* counts,
                           double* stats, void* work, size_t work_bytes, void* stream) {
    static_assert(sizeof(phx_summary_segment) == 24, "phx_summary_segment layout");
    PHX_REQUIRE(nseg > 0 && nseg <= 65535, PHX_E_SHAPE, "summary_histograms: 1 .. 65535 segments");
    PHX_REQUIRE(segs && limits && counts && stats && work, PHX_E_INVAL, "summary_histograms: null pointer");
    PHX_REQUIRE(max_n < ((uint64_t)1 << 40), PHX_E_SHAPE, "summary_histograms: a segment holds fewer than 2^40 elements");
    PHX_REQUIRE(work_bytes >= phx_summary_histograms_ws_bytes(nseg), PHX_E_INVAL, "summary_histograms: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    PHX_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)nseg * SH_NB * sizeof(unsigned long long), st));
    PHX_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)nseg * PHX_SUMMARY_NSTATS * sizeof(double), st));
    PHX_CHECK_HIP(hipMemsetAsync(work, 0, (size_t)nseg * sizeof(SegAcc), st));
    size_t gx = (size_t)((max_n + SH_MINCHUNK - 1) / SH_MINCHUNK);
    gx = gx < 1 ? 1 : (gx > SH_MAXBX ? SH_MAXBX : gx);
    hipLaunchKernelGGL(k_summary_hist, dim3((unsigned)gx, (unsigned)nseg), dim3(SH_BLOCK), 0, st, segs, limits, counts, stats, (SegAcc*)work);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_summary_hist_final, dim3((nseg + 63) / 64), dim3(64), 0, st, (const SegAcc*)work, stats, nseg);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

int phx_summary_grid_u8(const void* src, int form, int B, int H, int W, int C, int shift, int grid_y, int grid_x, unsigned char* out,
                        void* work, void* stream) {
    PHX_REQUIRE(src && out && work, PHX_E_INVAL, "summary_grid_u8: null pointer");
    PHX_REQUIRE(form == PHX_GRID_LOGITS_F32 || form == PHX_GRID_LABELS_U8 || form == PHX_GRID_IMAGE_F32, PHX_E_INVAL, "summary_grid_u8: form");
    PHX_REQUIRE(B > 0 && H > 0 && W > 0 && grid_y > 0 && grid_x > 0 && grid_y * grid_x == B, PHX_E_SHAPE, "summary_grid_u8: grid_y * grid_x == B");
    PHX_REQUIRE(form != PHX_GRID_LOGITS_F32 || (C >= 1 && C <= 256), PHX_E_SHAPE, "summary_grid_u8: 1 <= C <= 256");
    PHX_REQUIRE(shift >= 0 && shift < 16 && ((H >> shift) << shift) == H && ((W >> shift) << shift) == W, PHX_E_SHAPE,
                "summary_grid_u8: H and W are multiples of 2^shift");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)B * (H >> shift) * (W >> shift);
    const size_t nout = (size_t)(H + 2) * grid_y * (size_t)(W + 2) * grid_x;
    PHX_REQUIRE(nout < ((size_t)1 << 40), PHX_E_SHAPE, "summary_grid_u8: grid too large");
    PHX_CHECK_HIP(hipMemsetAsync(work, 0, PHX_SUMMARY_GRID_WS_BYTES, st));
    hipLaunchKernelGGL(k_grid_minmax, dim3(phx_grid_for(npix, 256, 1024)), dim3(256), 0, st, src, form, npix, C, (unsigned*)work);
    PHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_write, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, src, form, H, W, C, shift, grid_y, grid_x,
                       (const unsigned*)work, out);
    PHX_CHECK_LAUNCH();
    return PHX_OK;
}

}  // extern "C"
