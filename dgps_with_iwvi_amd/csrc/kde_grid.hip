// Log density of a Gaussian kernel-density estimate at G levels per point in ONE launch (iwvi_kde_density_grid): the reference's
// conditional density picture (experiments/demo.py: plot_density and the closing loop) -- per test input S predictive samples, Silverman's
// bandwidth or a fixed one, log p^_n(level) at every level of a grid.
//
//   work    a workgroup of KG_THREADS owns one point and a tile of up to KG_TILE levels.  With Gp = min(KG_TILE, next power of two >= G)
//           thread t holds level t % Gp of the tile in a register and is split t / Gp of nsplit = KG_THREADS / Gp: the splits share a level's
//           samples (at Gp = 64 a split is a wave; at G = 1 all 256 threads split the samples of the one level).
//   stream  the point's samples pass through LDS KG_CHUNK at a time, padded with +inf (|l - inf| = inf never is the nearest sample and
//           exp(-inf) = 0 adds nothing: the inner loops carry no bounds test).  Split q reads the float4 granules q, q + nsplit, .. of the
//           chunk: the lanes of a split read ONE address (a broadcast), neighbouring splits neighbouring granules (no bank is hit twice).
//   passes  A: sum and NaN count on the way into LDS, per level the distance to the nearest sample;  B: sum (x - mean)^2 (the two-pass
//           standard deviation of k_sample_stats);  C: sum_s exp(-e_s^2 / 2 - mx) with mx the exponent of the nearest sample, known from
//           A for any bandwidth -- the largest term is exp(0) = 1, so a level hundreds of standard deviations out keeps its finite value.
//   sums    float64 formed from the float32 values, as k_kde_loglik and k_sample_stats; one division 1 / h per point, then e = (l - x) / h
//           as a product.  A level's per-split partials meet in LDS and are added in split order by one thread: no atomics, and two calls
//           give the same bits.  The result is rounded to float32 once.
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int KG_THREADS = 256;
constexpr int KG_TILE = 64;                      // levels per workgroup (evaluation.KDE_GRID_TILE)
constexpr int KG_CHUNK = 2048;                   // samples staged per pass step (evaluation.KDE_GRID_CHUNK); a multiple of 4 * KG_THREADS
static_assert(KG_CHUNK % (4 * KG_THREADS) == 0, "every split reads whole float4 granules of a chunk");

__device__ __forceinline__ double kg_wsum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }

// sum over the workgroup, left in every thread (fixed order: xor tree in the wave, then the four waves in order)
__device__ __forceinline__ double kg_block_sum(double v, double* red, int tid) {
    v = kg_wsum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < KG_THREADS / 64; ++w) s += red[w];
    __syncthreads();                                              // (red is free again)
    return s;
}

// samples [c0, c0 + KG_CHUNK) of the point -> LDS, +inf behind the last one; SUMS: this thread's values are added to acc, its NaNs counted in nan
template <bool SUMS>
__device__ __forceinline__ void kg_stage(const float* __restrict__ src, long long sstride, int S, int c0, float* x, int tid, double& acc, double& nan) {
#pragma unroll
    for (int k = 0; k < KG_CHUNK / KG_THREADS; ++k) {
        const int i = tid + k * KG_THREADS;
        float v = INFINITY;
        if (i < S - c0) {                                         // (c0 < S, so S - c0 does not overflow)
            v = src[(long long)(c0 + i) * sstride];
            if (SUMS) { acc += (double)v; nan += (v != v) ? 1.0 : 0.0; }
        }
        x[i] = v;
    }
}

__global__ __launch_bounds__(KG_THREADS) void k_kde_grid(const float* __restrict__ samples, long long sstride, long long nstride, int S,
                                                         const float* __restrict__ levels, long long lstride, int G, int Gp, int ntiles,
                                                         double bandwidth, float* __restrict__ out, float* __restrict__ stats,
                                                         float* __restrict__ out_bw) {
    __shared__ __attribute__((aligned(16))) float x[KG_CHUNK];
    __shared__ double red[KG_THREADS];
    const int tid = threadIdx.x;
    const long long n = blockIdx.x / ntiles;
    const int tile = (int)(blockIdx.x - n * ntiles);
    const int nsplit = KG_THREADS / Gp, li = tid & (Gp - 1), q = tid / Gp;      // (Gp: a power of two, 1 .. KG_TILE)
    const int g = tile * KG_TILE + li;
    const bool has_level = g < G;                                 // (a thread without a level runs the same steps on a padding level: the barriers are shared)
    const double lev = has_level ? (double)levels[n * lstride + g] : 0.0;
    const float* src = samples + n * nstride;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int steps = KG_CHUNK / (4 * nsplit);                    // float4 granules of a chunk per split

    // ---- A: sum, NaN count; per level the distance to the nearest sample (needs no bandwidth)
    double sum = 0.0, nan = 0.0, dmin = INFINITY;
    for (int c0 = 0; c0 < S; c0 += KG_CHUNK) {
        kg_stage<true>(src, sstride, S, c0, x, tid, sum, nan);
        __syncthreads();
        for (int j = 0; j < steps; ++j) {
            const float4 v = x4[j * nsplit + q];
            dmin = fmin(dmin, fmin(fmin(fabs(lev - (double)v.x), fabs(lev - (double)v.y)), fmin(fabs(lev - (double)v.z), fabs(lev - (double)v.w))));
        }
        __syncthreads();
    }
    sum = kg_block_sum(sum, red, tid);
    nan = kg_block_sum(nan, red, tid);
    const double mean = sum / S;
    const bool has_nan = nan > 0.0;
    red[tid] = dmin;                                              // the splits of a level: entries li + k Gp
    __syncthreads();
    for (int k = 0; k < nsplit; ++k) dmin = fmin(dmin, red[li + k * Gp]);
    __syncthreads();

    // ---- B: the population standard deviation about that mean, Silverman's bandwidth
    double ssq = 0.0;
    for (int i = tid; i < S; i += KG_THREADS) { const double e = (double)src[(long long)i * sstride] - mean; ssq += e * e; }
    ssq = kg_block_sum(ssq, red, tid);
    const double sd = sqrt(ssq / S);                              // np.std
    const bool silverman = !(bandwidth > 0.0);
    const double bw = silverman ? 1.06 * sd * pow((double)S, -0.2) : bandwidth;
    const double inv_bw = 1.0 / bw;
    double mx;
    { const double e = dmin * inv_bw; mx = -0.5 * e * e; }        // the largest exponent: the sample nearest to the level

    // ---- C: the sum of exponentials relative to it
    double se = 0.0;
    for (int c0 = 0; c0 < S; c0 += KG_CHUNK) {
        if (S > KG_CHUNK) {                                       // (uniform; a single chunk is still in LDS from pass A)
            double unused0 = 0.0, unused1 = 0.0;
            kg_stage<false>(src, sstride, S, c0, x, tid, unused0, unused1);
            __syncthreads();
        }
        for (int j = 0; j < steps; ++j) {
            const float4 v = x4[j * nsplit + q];
            const double e0 = (lev - (double)v.x) * inv_bw, e1 = (lev - (double)v.y) * inv_bw;
            const double e2 = (lev - (double)v.z) * inv_bw, e3 = (lev - (double)v.w) * inv_bw;
            se += exp(-0.5 * e0 * e0 - mx);
            se += exp(-0.5 * e1 * e1 - mx);
            se += exp(-0.5 * e2 * e2 - mx);
            se += exp(-0.5 * e3 * e3 - mx);
        }
        if (S > KG_CHUNK) __syncthreads();
    }
    red[tid] = se;
    __syncthreads();
    const float fnan = __int_as_float(0x7fc00000);
    if (q == 0 && has_level) {
        double tot = red[li];
        for (int k = 1; k < nsplit; ++k) tot += red[li + k * Gp];                // split order: the same bits every call
        float lp = (float)(mx + log(tot) - log((double)S * bw) - 0.9189385332046727);   // - log sqrt(2 pi)
        if (silverman && sd == 0.0) lp = dmin == 0.0 ? INFINITY : -INFINITY;    // all samples equal: a point mass
        if (has_nan || lev != lev) lp = fnan;
        out[n * (long long)G + g] = lp;
    }
    if (tile == 0 && tid == 0) {
        if (stats) { stats[2 * n] = has_nan ? fnan : (float)mean; stats[2 * n + 1] = has_nan ? fnan : (float)sd; }
        if (out_bw) out_bw[n] = has_nan ? fnan : (float)bw;
    }
}

}  // namespace iwvi

extern "C" int iwvi_kde_density_grid(const float* samples, int64_t sample_stride, int64_t point_stride, int64_t N, int64_t S,
                                     const float* levels, int64_t level_point_stride, int G, double bandwidth,
                                     float* out_logdens, float* out_mean_std, float* out_bandwidth, void* stream_) {
    using namespace iwvi;
    const char* fn = "iwvi_kde_density_grid";
    if (!samples) { set_error("%s: null samples", fn); return IWVI_ERR_ARG; }
    if (!levels) { set_error("%s: null levels", fn); return IWVI_ERR_ARG; }
    if (!out_logdens) { set_error("%s: null out_logdens", fn); return IWVI_ERR_ARG; }
    if (sample_stride <= 0 || point_stride <= 0) { set_error("%s: strides %lld / %lld must be positive", fn, (long long)sample_stride, (long long)point_stride); return IWVI_ERR_ARG; }
    if (N < 0) { set_error("%s: N=%lld is negative", fn, (long long)N); return IWVI_ERR_ARG; }
    if (G < 1) { set_error("%s: G=%d must be at least 1", fn, G); return IWVI_ERR_ARG; }
    if (level_point_stride != 0 && level_point_stride < G) { set_error("%s: level_point_stride=%lld must be 0 (shared levels) or >= G=%d", fn, (long long)level_point_stride, G); return IWVI_ERR_ARG; }
    if (!(bandwidth - bandwidth == 0.0)) { set_error("%s: bandwidth=%g is not finite", fn, bandwidth); return IWVI_ERR_ARG; }
    if (S < 1 || S > 0x7fffffffLL - KG_CHUNK) { set_error("%s: S=%lld out of range (1 .. 2^31 - 1 - %d)", fn, (long long)S, KG_CHUNK); return IWVI_ERR_ARG; }
    if (S < 2 && !(bandwidth > 0.0)) { set_error("%s: S=%lld: Silverman's bandwidth (bandwidth <= 0) needs S >= 2", fn, (long long)S); return IWVI_ERR_ARG; }
    const int ntiles = (G + KG_TILE - 1) / KG_TILE;
    if (N * (int64_t)ntiles > 0x7fffffffLL) { set_error("%s: N=%lld x %d level tiles exceeds 2^31 - 1 workgroups", fn, (long long)N, ntiles); return IWVI_ERR_ARG; }
    if (N == 0) return IWVI_OK;
    int Gp = 1;
    while (Gp < G && Gp < KG_TILE) Gp <<= 1;
    hipLaunchKernelGGL(k_kde_grid, dim3((unsigned)(N * ntiles)), dim3(KG_THREADS), 0, (hipStream_t)stream_, samples, (long long)sample_stride,
                       (long long)point_stride, (int)S, levels, (long long)level_point_stride, G, Gp, ntiles, bandwidth, out_logdens,
                       out_mean_std, out_bandwidth);
    return check_launch("k_kde_grid");
}
