// Per-test-point statistics of S predictive samples in ONE launch (iwvi_sample_stats): the tail of the reference's evaluation loop
// (experiments/run_conditional_density_estimation.py:148-169) -- KDE log density at y with Silverman's bandwidth, squared error of the
// sample mean, Shapiro-Wilk W -- and quantiles, all from one ascending sort of the point's samples held in LDS.
//
//   sort    the bitonic network of csrc/sample_sort.h, shared with k_sample_scores (csrc/sample_scores.hip): P = max(64, next power of
//           two >= S) floats per point, padded with +inf.
//   sums   float64 from the float32 values, the arithmetic of k_kde_loglik (csrc/lv_elbo.hip): W = b^2 / sum (x - mean)^2 cancels like
//           1 - W ~ 1e-3..1e-4 at the sizes in use, and the KDE's sum of S exponentials is what the reference's float64 estimate sums.
//   groups  ss_shape (csrc/sample_sort.h): four, two or one point per workgroup.
#include <math.h>
#include "iwvi_common.h"
#include "sample_sort.h"

namespace iwvi {

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

    // ---- in: strided samples -> the sort (csrc/sample_sort.h); the sums of the unsorted values are taken on the way
    double acc[3] = {0.0, 0.0, INFINITY};                          // sum, NaN count, min |y - x|
    ss_sort_in(x, P, TG, gtid, lane, [&](int i) {
        float v = INFINITY;
        if (valid && i < S) {
            v = src[(long long)i * sstride];
            acc[0] += (double)v;
            acc[1] += (v != v) ? 1.0 : 0.0;
            acc[2] = fmin(acc[2], fabs(yy - (double)v));
        }
        return v;
    });
    ss_sort_merge(x, P, TG, gtid, lane);

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
    // ---- quantiles, NumPy's default rule (ss_quantile)
    for (int q = gtid; q < n_probs; q += TG) outQ[n * n_probs + q] = has_nan ? fnan : (float)ss_quantile(x, S, probs[q]);
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
    const SsShape sh = ss_shape(S);
    const int P = sh.P, threads = sh.threads, TG = sh.TG, groups = sh.groups;
    const size_t lds_bytes = sh.lds_bytes;
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
