// Host-side launch geometry and device-side statistics helpers of the normalisation units (norm.hip, norm_bwd.hip).
#pragma once
#include "vec_io.h"

// A block is CV = C / V channel vectors x PL pixel lanes; the P pixels of a sample group are cut into nchunks chunks of `chunk`
// pixels, one block each: about ppt pixels per thread, but at least fl and at most cap blocks in the whole launch.
static inline int block_geometry(int P, int C, int V, int NS, int ppt, int fl, int cap, int* PL, int* threads, int* chunk, int* nchunks) {
    int CV = C / V;
    if (CV > 256) return -1;
    *PL = 256 / CV;                              // (512 / 1024-thread blocks measured slower: the LDS reduction over PL lanes grows)
    *threads = CV * (*PL);                       // (PL >= 1: CV <= 256)
    const int ns = NS > 0 ? NS : 1;
    int rows = (P + *PL - 1) / (*PL);
    int want = (rows + ppt - 1) / ppt;
    // (the floor counts blocks of the whole launch: with per-sample statistics, NS > 1, every sample gets its share -- a
    // floor per SAMPLE cut the 128 x 128 group-norm layers into thousands of blocks of two pixels per thread: 62 us vs 19)
    const int fl_ns = (fl + ns - 1) / ns;
    int floor_blocks = rows < fl_ns ? rows : fl_ns;
    if (want < floor_blocks) want = floor_blocks;
    cap /= ns;
    if (cap < 1) cap = 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    *chunk = (P + want - 1) / want;
    *nchunks = (P + *chunk - 1) / (*chunk);
    return 0;
}
// Every block of the launch has at least one pixel: the kernels that issue their first loads ahead of the prologue clamp them to the
// block's last pixel, which must exist (nchunks = ceil(P / chunk) gives it; the launchers check it rather than assume it).
static inline bool block_ranges_nonempty(int P, int chunk, int nchunks) {
    return P >= 1 && chunk >= 1 && nchunks >= 1 && (size_t)(nchunks - 1) * (size_t)chunk < (size_t)P;
}
// the statistics pass (nrep == 1) and the backward reduction (nrep > 1)
static inline int norm_geometry(int P, int C, int V, int* PL, int* threads, int* chunk, int* nchunks, int NS, int nrep = 1) {
    // Every block ends in 2C same-address fp32 atomics (~45 ns each, serialised per address): the block count is a trade between
    // streaming parallelism and that tail.  The backward reduction spreads its blocks over nrep accumulator replicas and takes
    // more, shorter blocks (16 pixels per thread, 256..512 blocks); the forward statistics pass has one accumulator set -- 256
    // blocks cost it 11 us of atomics on the H <= 16 levels -- and keeps 8 pixels per thread with a floor of 128 blocks.
    const int ppt_r = 16, fl_r = 256, capv = 512, ppt_s = 8, fl_s = 128;        // (measured: tools/bench_norm.py)
    return nrep > 1 ? block_geometry(P, C, V, NS, ppt_r, fl_r, capv, PL, threads, chunk, nchunks)
                    : block_geometry(P, C, V, NS, ppt_s, fl_s, 2048, PL, threads, chunk, nchunks);
}
// the streaming passes (256 threads per block)
static inline int stream_geometry(int P, int C, int V, int* PL, int* threads, int* chunk, int* nchunks, int NS) {
    // 8 pixels per thread on big maps (two trips of four); on small maps fewer, so that ~1024 blocks exist
    const int ppt_s = 8;                         // pixels per thread (8 / floor 1024 since the prologues are LDS-shared; 32 / 256 before)
    const int fl = 1024;                         // (measured: tools/bench_norm.py)
    return block_geometry(P, C, V, NS, ppt_s, fl, 8192, PL, threads, chunk, nchunks);
}

// Per-channel batch / instance-norm coefficients from the accumulated sums -- ONE definition with floating-point contraction off, used
// by the fused apply kernels AND by k_norm_finalize, so that the stand-alone finalisation and the fused one agree bit for bit (round 5:
// with the compiler free to contract `s2 * invP - d1 * d1` differently in the two kernels the variances differed in the last place --
// a bf16 flip per few thousand activations, and two Adam steps later 30 % of the ELBO of a deliberately ill-conditioned test network).
__device__ __forceinline__ void chan_coeffs(float s1, float s2, float pv, float invP, float eps, float* mu, float* var, float* rs) {
#pragma clang fp contract(off)
    const float d1 = s1 * invP;
    const float m2 = s2 * invP;
    const float dd = d1 * d1;
    *mu = pv + d1;
    *var = fmaxf(m2 - dd, 0.f);
    *rs = rsqrtf(*var + eps);
}
__device__ __forceinline__ void moving_update(float* mm, float* mv, float mu, float var, float m, float momentum) {
#pragma clang fp contract(off)       // TF1 fused-batch-norm moving update (unbiased variance): moving -= (moving - batch) * momentum
    const float ub = var * (m / fmaxf(m - 1.f, 1.f));
    const float dm = (*mm - mu) * momentum, dv = (*mv - ub) * momentum;
    *mm = *mm - dm;
    *mv = *mv - dv;
}
__device__ __forceinline__ void chan_scale_shift(float gamma, float beta, float mu, float rs, float* sc, float* sh) {
#pragma clang fp contract(off)
    const float scv = gamma * rs;
    const float t = mu * scv;
    *sc = scv;
    *sh = beta - t;
}
__device__ __forceinline__ void group_stats(const float* __restrict__ sums, const float* __restrict__ pivot, int ns,
                                            int C, int g, int cg, float invP, float eps, float* mu_out, float* var_out) {
    float mu = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c)
        mu += (pivot ? pivot[(size_t)ns * C + c] : 0.f) + sums[((size_t)ns * C + c) * 2] * invP;
    mu /= (float)cg;
    float var = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
        const float d1 = sums[((size_t)ns * C + c) * 2] * invP;
        float vc = sums[((size_t)ns * C + c) * 2 + 1] * invP - d1 * d1;
        vc = vc > 0.f ? vc : 0.f;
        const float dm = (pivot ? pivot[(size_t)ns * C + c] : 0.f) + d1 - mu;
        var += vc + dm * dm;
    }
    *mu_out = mu;
    *var_out = var / (float)cg;
}
// pixel index in the packed order [B][h][w][(a, b)] -> pixel index of the hi-res map [B][2h][2w]
__device__ __forceinline__ size_t packed_to_hi_pixel(size_t pix, int h, int w) {
    const unsigned q = (unsigned)(pix >> 2), ab = (unsigned)pix & 3u;
    const unsigned t = q / (unsigned)w, j = q - t * (unsigned)w, b = t / (unsigned)h, i = t - b * (unsigned)h;
    return ((size_t)b * 2 * h + 2 * i + (ab >> 1)) * 2 * w + 2 * j + (ab & 1u);
}
