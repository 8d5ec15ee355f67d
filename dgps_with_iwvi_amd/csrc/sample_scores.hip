// Univariate proper scoring rules of S predictive samples per point in ONE launch (iwvi_sample_scores): the ensemble and the fair CRPS,
// the counts a PIT / rank histogram is formed from, quantiles and their pinball loss -- all from the one ascending sort of the point's
// samples in LDS that k_sample_stats does (csrc/sample_sort.h: the same network, grouping rule and quantile arithmetic).
//
//   terms   A = (1/S) sum_s |x_s - y|  and the counts #{x_s < y}, #{x_s == y} from the unsorted values on the way in;
//           G = sum_i (2i - S - 1) x_(i) = 1/2 sum_s sum_t |x_s - x_t| from the sorted ones (i = 1 .. S): S terms instead of S^2.
//   sums    float64 from the float32 values.  (2i - S - 1) x_(i) is exact in float64 (15 + 24 bits); the counts are integers below 2^15.
//           Per-lane partials, then the wave, then the group's waves, in a fixed order: no atomics, the same bits on every call.
#include <math.h>
#include "iwvi_common.h"
#include "sample_sort.h"

namespace iwvi {

__global__ __launch_bounds__(1024) void k_sample_scores(const float* __restrict__ samples, long long sstride, long long nstride,
                                                        const float* __restrict__ y, long long N, int S, int P, int TG,
                                                        const double* __restrict__ probs, int n_probs, float* __restrict__ crps,
                                                        int* __restrict__ counts, float* __restrict__ outQ, float* __restrict__ pinball) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = tid / TG, gtid = tid - grp * TG;             // (TG: a power of two, 64 .. blockDim.x)
    const int nwg = TG >> 6, gwave = gtid >> 6;
    const long long n = (long long)blockIdx.x * (blockDim.x / TG) + grp;
    const bool valid = n < N;                                     // (a group without a point runs the same steps on padding: the barriers are shared)
    double* red = reinterpret_cast<double*>(ss_smem) + (size_t)grp * nwg * 3;
    float* x = reinterpret_cast<float*>(ss_smem + SS_RED * sizeof(double)) + (size_t)grp * P;
    const float* src = samples + (valid ? n : 0) * nstride;
    const float yf = valid ? y[n] : 0.f;
    const double yy = (double)yf;

    double acc[3] = {0.0, 0.0, 0.0};                               // sum |x - y|, NaN count, #{x < y}
    double acc2[2] = {0.0, 0.0};                                   // G, #{x == y}
    ss_sort_in(x, P, TG, gtid, lane, [&](int i) {
        float v = INFINITY;
        if (valid && i < S) {
            v = src[(long long)i * sstride];
            acc[0] += fabs((double)v - yy);
            acc[1] += (v != v) ? 1.0 : 0.0;
            acc[2] += (v < yf) ? 1.0 : 0.0;
            acc2[1] += (v == yf) ? 1.0 : 0.0;
        }
        return v;
    });
    ss_sort_merge(x, P, TG, gtid, lane);

    ss_group_reduce<3, 0>(acc, red, gwave, nwg, lane);
    for (int i = gtid; i < S; i += TG) acc2[0] += (double)(2 * i + 1 - S) * (double)x[i];
    ss_group_reduce<2, 0>(acc2, red, gwave, nwg, lane);
    if (!valid) return;
    const bool has_nan = acc[1] > 0.0 || yf != yf;
    const float fnan = __int_as_float(0x7fc00000);
    if (gtid == 0) {
        const double A = acc[0] / (double)S, G = acc2[0], s = (double)S;
        if (crps) {
            crps[2 * n] = has_nan ? fnan : (float)(A - G / (s * s));
            crps[2 * n + 1] = has_nan ? fnan : (float)(A - G / (s * (s - 1.0)));
        }
        if (counts) {
            counts[2 * n] = has_nan ? -1 : (int)acc[2];
            counts[2 * n + 1] = has_nan ? -1 : (int)acc2[1];
        }
    }
    for (int q = gtid; q < n_probs; q += TG) {
        const double Q = ss_quantile(x, S, probs[q]);
        const double tau = fmin(fmax(probs[q], 0.0), 1.0), d = yy - Q;
        if (outQ) outQ[n * n_probs + q] = has_nan ? fnan : (float)Q;
        if (pinball) pinball[n * n_probs + q] = has_nan ? fnan : (float)fmax(tau * d, (tau - 1.0) * d);
    }
}

}  // namespace iwvi

extern "C" int iwvi_sample_scores(const float* samples, int64_t sample_stride, int64_t point_stride, const float* y, int64_t N, int S,
                                  const double* probs, int n_probs, float* out_crps, int32_t* out_counts, float* out_quantiles,
                                  float* out_pinball, void* stream_) {
    using namespace iwvi;
    if (S < 2 || S > SS_MAX_S) { set_error("iwvi_sample_scores: S=%d out of range (2..%d)", S, SS_MAX_S); return IWVI_ERR_ARG; }
    if (N < 0 || N > 0x7fffffffLL) { set_error("iwvi_sample_scores: N=%lld out of range (0 .. 2^31 - 1)", (long long)N); return IWVI_ERR_ARG; }
    if (!samples) { set_error("iwvi_sample_scores: null samples"); return IWVI_ERR_ARG; }
    if (!y) { set_error("iwvi_sample_scores: null y"); return IWVI_ERR_ARG; }
    if (sample_stride <= 0 || point_stride <= 0) { set_error("iwvi_sample_scores: strides %lld / %lld must be positive", (long long)sample_stride, (long long)point_stride); return IWVI_ERR_ARG; }
    if (n_probs < 0 || (n_probs > 0 && (!probs || (!out_quantiles && !out_pinball)))) { set_error("iwvi_sample_scores: n_probs=%d needs probs and out_quantiles or out_pinball", n_probs); return IWVI_ERR_ARG; }
    if (N == 0) return IWVI_OK;
    const SsShape sh = ss_shape(S);
    static size_t attr_set = 0;
    if (sh.lds_bytes > attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_sample_scores, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.lds_bytes);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute(k_sample_scores, %zu B): %s", sh.lds_bytes, hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
        attr_set = sh.lds_bytes;
    }
    hipLaunchKernelGGL(k_sample_scores, dim3((unsigned)((N + sh.groups - 1) / sh.groups)), dim3(sh.threads), sh.lds_bytes, (hipStream_t)stream_,
                       samples, (long long)sample_stride, (long long)point_stride, y, (long long)N, S, sh.P, sh.TG, probs, n_probs, out_crps,
                       out_counts, out_quantiles, out_pinball);
    return check_launch("k_sample_scores");
}
