// Importance-weight summaries of S draws per point in ONE launch (iwvi_psis_summary): the log-mean weight, Kish's effective sample size,
// the Pareto-k diagnostic and the Pareto-smoothed log-mean weight (Vehtari, Simpson, Gelman, Yao, Gabry: "Pareto smoothed importance
// sampling"; the generalized-Pareto fit of Zhang & Stephens 2009 with the PSIS prior) -- from the one ascending sort of the point's
// log-weights in LDS that k_sample_stats does (csrc/sample_sort.h: the same network and grouping rule).
//
//   in      a draw's log-weight is ASSEMBLED in the sort's load functor, float32: the sum of its term columns, or the Gaussian's predictive
//           density / variational expectation from the final layer's moments, minus the draw's local regularisers (k_bound_logw's order).
//           Nothing per draw reaches memory unless out_logw asks for it.
//   sums    exp(l - max) in float32 (the maximum is the sorted array's last entry), added up in float64: body and tail apart, so that the
//           smoothed estimate replaces the tail's share and nothing else.
//   fit     float64 from the exceedances on, in LDS behind the sorted values: at most 384 exceedances (M = ceil(min(S / 5, 3 sqrt S))) and
//           at most 49 grid points, the grid dealt over the point's waves (a wave per grid point, its lanes over the exceedances); the
//           49-entry softmax and the final k by every wave on its own (the same bits in each: no barrier, no broadcast).
//   order   per-lane partials, then the wave, then the group's waves, in a fixed order: no atomics, the same bits on every call.
// Barriers are workgroup-wide and a workgroup holds up to four points: every loop below whose trip count depends on a point's tail is
// free of barriers, and no thread returns before the last one.
#include <math.h>
#include "iwvi_common.h"
#include "sample_sort.h"

namespace iwvi {

constexpr int PS_MAX_TAIL = 384;                 // 3 sqrt(16384)
constexpr int PS_MAX_GRID = 64;                  // 30 + floor(sqrt(384)) = 49 grid points, one lane each in the softmax
constexpr int PS_FIT = PS_MAX_TAIL + 2 * PS_MAX_GRID;   // doubles per point: exceedances | b_j | L_j
constexpr double PS_LOG_TINY = -87.33654475055310898657;   // log(2^-126)
constexpr double PS_EPS = 2.220446049250313e-16;            // 2^-52

struct PsisArgs {
    const float* terms; int n_terms;
    const float* fmean; const float* fvar; const float* Y; int Dy, var_exp; float lik_var; const float* lik_var_dev;
    const float* kl[IWVI_MAX_KL]; int kl_dims[IWVI_MAX_KL]; int n_kl;
    long long N, stride_n, stride_s; int S, P, TG, M;
    float* out_logw; float* raw; float* ess; float* khat; float* psis;
};

__device__ __forceinline__ double ps_wmax(double v) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64)); return v; }

__global__ __launch_bounds__(1024) void k_psis_summary(PsisArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int TG = a.TG, P = a.P, S = a.S, M = a.M;
    const int grp = tid / TG, gtid = tid - grp * TG;             // (TG: a power of two, 64 .. blockDim.x)
    const int nwg = TG >> 6, gwave = gtid >> 6, groups = blockDim.x / TG;
    const long long n = (long long)blockIdx.x * groups + grp;
    const bool valid = n < a.N;                                   // (a group without a point runs the same steps on padding: the barriers are shared)
    double* red = reinterpret_cast<double*>(ss_smem) + (size_t)grp * nwg * 3;
    float* x = reinterpret_cast<float*>(ss_smem + SS_RED * sizeof(double)) + (size_t)grp * P;
    double* fe = reinterpret_cast<double*>(ss_smem + SS_RED * sizeof(double) + (size_t)groups * P * sizeof(float)) + (size_t)grp * PS_FIT;
    double* fb = fe + PS_MAX_TAIL;
    double* fL = fb + PS_MAX_GRID;

    // ---- in: a draw's log-weight, float32 -> the sort
    const float sv = a.terms ? 1.f : (a.lik_var_dev ? *a.lik_var_dev : a.lik_var);
    const float c0 = -0.5f * logf(6.283185307179586f * sv);
    double acc[3] = {0.0, 0.0, 0.0};                               // NaN / +inf count, body sum, tail sum
    ss_sort_in(x, P, TG, gtid, lane, [&](int i) {
        float v = INFINITY;
        if (valid && i < S) {
            const long long t = n * a.stride_n + (long long)i * a.stride_s;
            float l = 0.f;
            if (a.terms) {
                for (int j = 0; j < a.n_terms; ++j) l += a.terms[t * a.n_terms + j];
            } else {
                for (int d = 0; d < a.Dy; ++d) {
                    const float e = a.Y[n * a.Dy + d] - a.fmean[t * a.Dy + d], fv = a.fvar[t * a.Dy + d];
                    if (a.var_exp) l += c0 - 0.5f * (e * e + fv) / sv;
                    else { const float tv = fv + sv; l += -0.5f * logf(6.283185307179586f * tv) - 0.5f * e * e / tv; }
                }
            }
            for (int q = 0; q < a.n_kl; ++q)
                for (int c = 0; c < a.kl_dims[q]; ++c) l -= a.kl[q][t * a.kl_dims[q] + c];
            v = l;
            acc[0] += (v != v || v == INFINITY) ? 1.0 : 0.0;
            if (a.out_logw) a.out_logw[n * S + i] = v;
        }
        return v;
    });
    ss_sort_merge(x, P, TG, gtid, lane);

    // ---- the tail: the entries strictly above cutoff = max(x_(S-M), log 2^-126), relative to the maximum (uniform in the group)
    const float mf = x[S - 1];
    const double md = (double)mf;
    const bool live = valid && mf > -INFINITY && mf < INFINITY;   // (all draws at -inf: no weights; +inf: counted in acc[0])
    int nt = 0;
    double ec = 0.0;
    if (live && S - M - 1 >= 0) {
        const double cutoff = fmax((double)x[S - M - 1] - md, PS_LOG_TINY);
        int lo = S - M, hi = S;                                    // (x[S - M - 1] is not above the cutoff: at most M entries are)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)x[mid] - md > cutoff) hi = mid; else lo = mid + 1;
        }
        nt = S - lo;
        if (nt <= 4 || nt > PS_MAX_TAIL) nt = 0;                   // too short a tail for a fit: khat = +inf, nothing smoothed
        ec = exp(cutoff);
    }
    const bool fit = nt > 0;

    // ---- sums of the weights (float32 exponentials, float64 sums) and the exceedances (float64), ascending
    double acc2[2] = {0.0, 0.0};                                   // sum w^2, smoothed tail sum
    for (int i = gtid; i < S; i += TG) {
        const float w = live ? __expf(x[i] - mf) : 0.f;
        if (i < S - nt) acc[1] += (double)w; else acc[2] += (double)w;
        acc2[0] += (double)w * (double)w;
    }
    for (int i = gtid; i < nt; i += TG) fe[i] = exp((double)x[S - nt + i] - md) - ec;
    ss_group_reduce<3, 0>(acc, red, gwave, nwg, lane);
    __syncthreads();                                               // (fe is complete: a one-wave group has no barrier in the reduction)

    // ---- the grid: b_j, k_j = mean log1p(-b_j e), L_j = n (log(-b_j / k_j) - k_j - 1); grid point j on wave (j - 1) % nwg
    const double dn = (double)nt;
    const int m = fit ? 30 + (int)floor(sqrt(dn)) : 0;
    if (fit) {
        const double eq = fe[(int)floor(dn / 4.0 + 0.5) - 1], emax = fe[nt - 1];
        for (int j = gwave + 1; j <= m; j += nwg) {
            const double bj = (1.0 - sqrt((double)m / ((double)j - 0.5))) / (3.0 * eq) + 1.0 / emax;
            double ks = 0.0;
            for (int i = lane; i < nt; i += 64) ks += log1p(-bj * fe[i]);
            const double kj = ss_wsum(ks) / dn;
            if (lane == 0) { fb[j - 1] = bj; fL[j - 1] = dn * (log(-bj / kj) - kj - 1.0); }
        }
    }
    __syncthreads();

    // ---- the posterior mean of b over the grid, k and sigma at it (every wave: lane j holds grid point j + 1)
    double khat = INFINITY, sigma = 0.0;
    if (fit) {
        const bool on = lane < m;
        const double Lj = on ? fL[lane] : -INFINITY, bj = on ? fb[lane] : 0.0;
        const double Lmax = ps_wmax(Lj);
        double w = on ? exp(Lj - Lmax) : 0.0;
        w = w / ss_wsum(w);
        w = w < 10.0 * PS_EPS ? 0.0 : w;
        w = w / ss_wsum(w);
        const double bp = ss_wsum(w * bj);
        double ks = 0.0;
        for (int i = lane; i < nt; i += 64) ks += log1p(-bp * fe[i]);
        const double kp = ss_wsum(ks) / dn;
        sigma = -kp / bp;
        khat = (dn * kp + 5.0) / (dn + 10.0);
    }
    const bool smooth = fit && khat - khat == 0.0 && sigma - sigma == 0.0;   // both finite

    // ---- the smoothed tail: the fitted distribution's quantiles at (i - 1/2) / n, capped at the largest weight
    if (smooth) {
        for (int i = gtid; i < nt; i += TG) {
            const double lp = log1p(-((double)i + 0.5) / dn);
            const double q = fabs(khat) < PS_EPS ? -sigma * lp : sigma * expm1(-khat * lp) / khat;
            double v = log(q + ec);
            v = v > 0.0 ? 0.0 : v;
            acc2[1] += exp(v);
        }
    }
    ss_group_reduce<2, 0>(acc2, red, gwave, nwg, lane);
    if (!valid || gtid != 0) return;

    const float fnan = __int_as_float(0x7fc00000);
    float o_raw, o_ess, o_khat, o_psis;
    if (acc[0] > 0.0) {
        o_raw = o_ess = o_khat = o_psis = fnan;
    } else if (!live) {
        o_raw = o_psis = -INFINITY; o_ess = 0.f; o_khat = INFINITY;
    } else {
        const double s1 = acc[1] + acc[2], lS = log((double)S);
        const double r = md + log(s1) - lS;
        o_raw = (float)r;
        o_ess = fminf(fmaxf((float)(s1 * s1 / acc2[0]), 1.f), (float)S);       // (in [1, S] by Cauchy-Schwarz: the clamp only takes rounding off)
        o_khat = (float)khat;
        o_psis = smooth ? (float)(md + log(acc[1] + acc2[1]) - lS) : o_raw;
    }
    if (a.raw) a.raw[n] = o_raw;
    if (a.ess) a.ess[n] = o_ess;
    if (a.khat) a.khat[n] = o_khat;
    if (a.psis) a.psis[n] = o_psis;
}

}  // namespace iwvi

extern "C" int iwvi_psis_summary(const iwvi_psis_desc* d, void* stream_) {
    using namespace iwvi;
    const char* what = "iwvi_psis_summary";
    if (!d) { set_error("%s: null descriptor", what); return IWVI_ERR_ARG; }
    if (d->N < 0 || d->N > 0x7fffffffLL) { set_error("%s: N=%lld out of range (0 .. 2^31 - 1)", what, (long long)d->N); return IWVI_ERR_ARG; }
    if (d->S < 1 || d->S > SS_MAX_S) { set_error("%s: S=%d out of range (1..%d)", what, d->S, SS_MAX_S); return IWVI_ERR_ARG; }
    if (d->stride_n < 0 || d->stride_s < 0) { set_error("%s: strides %lld / %lld must not be negative", what, (long long)d->stride_n, (long long)d->stride_s); return IWVI_ERR_ARG; }
    const bool moments = d->fmean || d->fvar;
    if (!d->terms && !moments) { set_error("%s: neither terms nor moments given", what); return IWVI_ERR_ARG; }
    if (d->terms && moments) { set_error("%s: both terms and moments given", what); return IWVI_ERR_ARG; }
    PsisArgs a{};
    if (d->terms) {
        if (d->n_terms < 1 || d->n_terms > IWVI_MAX_P) { set_error("%s: n_terms=%d outside 1..%d", what, d->n_terms, IWVI_MAX_P); return IWVI_ERR_ARG; }
        a.terms = d->terms; a.n_terms = d->n_terms;
    } else {
        if (!d->fmean || !d->fvar) { set_error("%s: moments need fmean and fvar", what); return IWVI_ERR_ARG; }
        if (d->Dy < 1 || d->Dy > IWVI_MAX_P) { set_error("%s: Dy=%d outside 1..%d", what, d->Dy, IWVI_MAX_P); return IWVI_ERR_ARG; }
        if (!d->Y) { set_error("%s: moments without Y", what); return IWVI_ERR_ARG; }
        if (!(d->lik_variance > 0.f)) { set_error("%s: lik_variance=%g must be positive", what, (double)d->lik_variance); return IWVI_ERR_ARG; }
        a.fmean = d->fmean; a.fvar = d->fvar; a.Y = d->Y; a.Dy = d->Dy; a.var_exp = d->var_exp != 0;
        a.lik_var = d->lik_variance; a.lik_var_dev = d->lik_variance_dev;
    }
    if (d->n_kl < 0 || d->n_kl > IWVI_MAX_KL) { set_error("%s: n_kl=%d outside 0..%d", what, d->n_kl, IWVI_MAX_KL); return IWVI_ERR_ARG; }
    for (int i = 0; i < d->n_kl; ++i) {
        if (!d->kl_local || !d->kl_local[i]) { set_error("%s: null kl_local pointer %d", what, i); return IWVI_ERR_ARG; }
        if (!d->kl_dims || d->kl_dims[i] < 1) { set_error("%s: kl_dims[%d] must be at least 1", what, i); return IWVI_ERR_ARG; }
        a.kl[i] = d->kl_local[i]; a.kl_dims[i] = d->kl_dims[i];
    }
    a.n_kl = d->n_kl;
    if (!d->out_logw && !d->out_raw && !d->out_ess && !d->out_khat && !d->out_psis) { set_error("%s: no output at all", what); return IWVI_ERR_ARG; }
    if (d->N == 0) return IWVI_OK;
    const SsShape sh = ss_shape(d->S);
    a.N = d->N; a.stride_n = d->stride_n; a.stride_s = d->stride_s; a.S = d->S; a.P = sh.P; a.TG = sh.TG;
    a.M = (int)ceil(fmin(0.2 * (double)d->S, 3.0 * sqrt((double)d->S)));
    a.out_logw = d->out_logw; a.raw = d->out_raw; a.ess = d->out_ess; a.khat = d->out_khat; a.psis = d->out_psis;
    const size_t lds_bytes = sh.lds_bytes + (size_t)sh.groups * PS_FIT * sizeof(double);
    static size_t attr_set = 0;
    if (lds_bytes > attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_psis_summary, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute(k_psis_summary, %zu B): %s", lds_bytes, hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
        attr_set = lds_bytes;
    }
    hipLaunchKernelGGL(k_psis_summary, dim3((unsigned)((d->N + sh.groups - 1) / sh.groups)), dim3(sh.threads), lds_bytes, (hipStream_t)stream_, a);
    return check_launch("k_psis_summary");
}
