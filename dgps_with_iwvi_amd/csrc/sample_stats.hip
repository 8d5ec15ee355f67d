// Per-test-point statistics of S predictive samples in ONE launch (iwvi_sample_stats): the tail of the reference's evaluation loop
// (experiments/run_conditional_density_estimation.py:148-169) -- KDE log density at y with Silverman's bandwidth, squared error of the
// sample mean, Shapiro-Wilk W -- and quantiles, all from one ascending sort of the point's samples held in LDS.
//
//   sort    P = max(64, next power of two >= S) floats per point, padded with +inf; a bitonic network.  A group of TG threads owns a
//           point; element i lives with thread i % TG, so every compare distance j < 64 pairs two lanes of ONE wave: those steps run on
//           registers through __shfl_xor (the first six merge sizes entirely, on the way in from memory; later the last six steps of a
//           merge), the distances j >= 64 go through LDS with one barrier per step.
//   sums    float64 from the float32 values, the arithmetic of k_kde_loglik (csrc/lv_elbo.hip): W = b^2 / sum (x - mean)^2 cancels like
//           1 - W ~ 1e-3..1e-4 at the sizes in use, and the KDE's sum of S exponentials is what the reference's float64 estimate sums.
//   groups  S <= 128: four points per 256-thread workgroup (one wave each); S <= 256: two; above that one point per workgroup, 1024
//           threads from S > 2048.
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int SS_MAX_S = 16384;                 // 64 KiB of sorted floats per workgroup
constexpr int SS_RED = 16 * 3;                  // doubles in front of the samples: 3 partial sums per wave of the workgroup

extern __shared__ __attribute__((aligned(16))) unsigned char ss_smem[];

__device__ __forceinline__ double ss_wsum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ double ss_wmin(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64)); return v; }

// sum (the first NV - NMIN entries) / minimum (the last NMIN) over the group's threads, left in every thread.  nwg = waves per group,
// the same for every group of the workgroup, so the barriers are uniform.
template <int NV, int NMIN>
__device__ __forceinline__ void ss_group_reduce(double (&v)[NV], double* red, int gwave, int nwg, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = k < NV - NMIN ? ss_wsum(v[k]) : ss_wmin(v[k]);
    if (nwg > 1) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) red[gwave * 3 + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = red[k];
            for (int w = 1; w < nwg; ++w) s = k < NV - NMIN ? s + red[w * 3 + k] : fmin(s, red[w * 3 + k]);
            v[k] = s;
        }
        __syncthreads();                                          // (red is free for the next reduction)
    }
}

// one compare-exchange step at distance j < 64 inside a wave: `up` = this element's merge sorts ascending
__device__ __forceinline__ float ss_step(float v, int lane, int j, bool up) {
    const float p = __shfl_xor(v, j, 64);
    return (((lane & j) == 0) == up) ? fminf(v, p) : fmaxf(v, p);
}

__global__ __launch_bounds__(1024) void k_sample_stats(const float* __restrict__ samples, long long sstride, long long nstride,
                                                       const float* __restrict__ y, long long N, int S, int P, int TG,
                                                       const double* __restrict__ coef, const double* __restrict__ probs, int n_probs,
                                                       float* __restrict__ logp, float* __restrict__ sqerr, float* __restrict__ stats,
                                                       float* __restrict__ outW, float* __restrict__ outQ) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = tid / TG, gtid = tid - grp * TG;             // (TG: a power of two, 64 .. blockDim.x)
    const int nwg = TG >> 6, gwave = gtid >> 6;
    const long long n = (long long)blockIdx.x * (blockDim.x / TG) + grp;
    const bool valid = n < N;                                     // (a group without a point runs the same steps on padding: the barriers are shared)
    double* red = reinterpret_cast<double*>(ss_smem) + (size_t)grp * nwg * 3;
    float* x = reinterpret_cast<float*>(ss_smem + SS_RED * sizeof(double)) + (size_t)grp * P;
    const float* src = samples + (valid ? n : 0) * nstride;
    const double yy = (valid && y) ? (double)y[n] : 0.0;

    // ---- in: strided samples -> registers, merge sizes 2 .. 64 on the way (element i and i ^ j, j < 64, are lanes of this wave), -> LDS
    double acc[3] = {0.0, 0.0, INFINITY};                          // sum, NaN count, min |y - x|
    for (int i = gtid; i < P; i += TG) {
        float v = INFINITY;
        if (valid && i < S) {
            v = src[(long long)i * sstride];
            acc[0] += (double)v;
            acc[1] += (v != v) ? 1.0 : 0.0;
            acc[2] = fmin(acc[2], fabs(yy - (double)v));
        }
#pragma unroll
        for (int k2 = 2; k2 <= 64; k2 <<= 1) {
            const bool up = (i & k2) == 0;
#pragma unroll
            for (int j = k2 >> 1; j > 0; j >>= 1) v = ss_step(v, lane, j, up);
        }
        x[i] = v;
    }
    __syncthreads();
    // ---- merge sizes 128 .. P: distances >= 64 through LDS (one barrier each), the last six in registers again
    for (int k2 = 128; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j >= 64; j >>= 1) {
            for (int q = gtid; q < (P >> 1); q += TG) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const float a = x[i], b = x[i + j];
                const bool up = (i & k2) == 0;
                x[i] = up ? fminf(a, b) : fmaxf(a, b);
                x[i + j] = up ? fmaxf(a, b) : fminf(a, b);
            }
            __syncthreads();
        }
        for (int i = gtid; i < P; i += TG) {
            float v = x[i];
            const bool up = (i & k2) == 0;
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) v = ss_step(v, lane, j, up);
            x[i] = v;
        }
        __syncthreads();
    }

    // ---- sums over the sorted samples (float64): mean -> (sum (x - mean)^2, the Shapiro-Wilk numerator) -> the KDE's sum of exponentials
    ss_group_reduce<3, 1>(acc, red, gwave, nwg, lane);
    const double mean = acc[0] / S, dmin = acc[2];
    const bool has_nan = acc[1] > 0.0;
    double acc2[2] = {0.0, 0.0};
    for (int i = gtid; i < S; i += TG) { const double e = (double)x[i] - mean; acc2[0] += e * e; }
    if (coef)
        for (int i = gtid; i < (S >> 1); i += TG) acc2[1] += coef[i] * ((double)x[S - 1 - i] - (double)x[i]);
    ss_group_reduce<2, 0>(acc2, red, gwave, nwg, lane);
    const double ssq = acc2[0], sd = sqrt(ssq / S);               // np.std: population standard deviation
    const double bw = 1.06 * sd * pow((double)S, -0.2);           // Silverman (1986)
    double se[1] = {0.0};
    float mx = 0.f;
    if (logp) {                                                    // (uniform: a kernel argument)
        { const double e = dmin / bw; mx = (float)(-0.5 * e * e); }   // the largest exponent: the sample nearest to y
        for (int i = gtid; i < S; i += TG) { const double e = (yy - (double)x[i]) / bw; se[0] += exp(-0.5 * e * e - (double)mx); }
        ss_group_reduce<1, 0>(se, red, gwave, nwg, lane);
    }
    if (!valid) return;
    const float fnan = __int_as_float(0x7fc00000);
    if (gtid == 0) {
        if (logp) {
            float lp = (float)((double)mx + log(se[0]) - log((double)S * bw) - 0.9189385332046727);   // - log sqrt(2 pi)
            if (sd == 0.0) lp = dmin == 0.0 ? INFINITY : -INFINITY;        // all samples equal: a point mass
            logp[n] = has_nan ? fnan : lp;
        }
        if (sqerr) sqerr[n] = has_nan ? fnan : (float)((mean - yy) * (mean - yy));
        if (stats) { stats[2 * n] = has_nan ? fnan : (float)mean; stats[2 * n + 1] = has_nan ? fnan : (float)sd; }
        if (outW) outW[n] = has_nan ? fnan : (ssq > 0.0 ? (float)(acc2[1] * acc2[1] / ssq) : 1.f);   // all samples equal: W = 1
    }
    // ---- quantiles, NumPy's default rule: position p (S - 1), linear between the two neighbouring sorted values
    for (int q = gtid; q < n_probs; q += TG) {
        const double p = fmin(fmax(probs[q], 0.0), 1.0);       // (float64: 0.975 as a float32 moves the position by 4e-5 at S = 2000)
        const double pos = p * (double)(S - 1);
        int lo = (int)pos;
        lo = lo < S - 1 ? lo : S - 1;
        const int hi = lo + 1 < S ? lo + 1 : S - 1;
        const double a = (double)x[lo], b = (double)x[hi], t = pos - (double)lo;
        outQ[n * n_probs + q] = has_nan ? fnan : (float)(a == b ? a : a + (b - a) * t);
    }
}

}  // namespace iwvi

extern "C" int iwvi_sample_stats(const float* samples, int64_t sample_stride, int64_t point_stride, const float* y, int64_t N, int S,
                                 const double* sw_coef, const double* probs, int n_probs, float* out_logp, float* out_sqerr,
                                 float* out_mean_std, float* out_W, float* out_quantiles, void* stream_) {
    using namespace iwvi;
    if (S < 2 || S > SS_MAX_S) { set_error("iwvi_sample_stats: S=%d out of range (2..%d)", S, SS_MAX_S); return IWVI_ERR_ARG; }
    if (N < 0 || N > 0x7fffffffLL) { set_error("iwvi_sample_stats: N=%lld out of range (0 .. 2^31 - 1)", (long long)N); return IWVI_ERR_ARG; }
    if (!samples) { set_error("iwvi_sample_stats: null samples"); return IWVI_ERR_ARG; }
    if (sample_stride <= 0 || point_stride <= 0) { set_error("iwvi_sample_stats: strides %lld / %lld must be positive", (long long)sample_stride, (long long)point_stride); return IWVI_ERR_ARG; }
    if (n_probs < 0 || (n_probs > 0 && (!probs || !out_quantiles))) { set_error("iwvi_sample_stats: n_probs=%d needs probs and out_quantiles", n_probs); return IWVI_ERR_ARG; }
    if (!y && (out_logp || out_sqerr)) { set_error("iwvi_sample_stats: out_logp / out_sqerr need y"); return IWVI_ERR_ARG; }
    if (out_W && !sw_coef) { set_error("iwvi_sample_stats: out_W needs the %d Shapiro-Wilk coefficients of S=%d", S / 2, S); return IWVI_ERR_ARG; }
    if (N == 0) return IWVI_OK;
    int P = 64;
    while (P < S) P <<= 1;
    const int threads = P >= 4096 ? 1024 : 256;
    int TG = P / 2 < 64 ? 64 : P / 2;
    if (TG > threads) TG = threads;
    const int groups = threads / TG;
    const size_t lds_bytes = SS_RED * sizeof(double) + (size_t)groups * P * sizeof(float);
    static size_t attr_set = 0;
    if (lds_bytes > attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_sample_stats, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute(k_sample_stats, %zu B): %s", lds_bytes, hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
        attr_set = lds_bytes;
    }
    hipLaunchKernelGGL(k_sample_stats, dim3((unsigned)((N + groups - 1) / groups)), dim3(threads), lds_bytes, (hipStream_t)stream_, samples,
                       (long long)sample_stride, (long long)point_stride, y, (long long)N, S, P, TG, out_W ? sw_coef : nullptr, probs, n_probs,
                       out_logp, out_sqerr, out_mean_std, out_W, out_quantiles);
    return check_launch("k_sample_stats");
}
