// What csrc/likelihood_tail.hip, csrc/likelihood_multiclass.hip and csrc/likelihood_explink.hip share: the Gauss-Hermite tables, the
// kernel-argument structs of the iwvi_lik_* entry points and the segment reductions (moved here verbatim from likelihood_tail.hip), the
// point loop of iwvi_lik_predict_mixture for the types whose outputs are independent (mix_points), and the launchers of the multi-class and the exp-link kernels, which the entry points of likelihood_tail.hip call for IWVI_LIK_MULTICLASS and for
// IWVI_LIK_POISSON / _EXPONENTIAL / _GAMMA.
#pragma once
#include "iwvi_common.h"

namespace iwvi {

// numpy.polynomial.hermite.hermgauss(20): the rule is symmetric, x_(19-i) = -x_i with equal weights -- the ten positive nodes, their
// weights w_i / sqrt(pi) and the logarithms of those (log-space sums).  Rounded to float32 the twenty weights sum to 1 - 5e-9.
__device__ __constant__ const float GH_X[10] = {2.453407083e-01f, 7.374737285e-01f, 1.234076215e+00f, 1.738537712e+00f, 2.254974002e+00f,
                                                2.788806058e+00f, 3.347854567e+00f, 3.944764040e+00f, 4.603682450e+00f, 5.387480890e+00f};
__device__ __constant__ const float GH_W[10] = {2.607930634e-01f, 1.617393340e-01f, 6.150637206e-02f, 1.399783745e-02f, 1.830103131e-03f,
                                                1.288262800e-04f, 4.402121090e-06f, 6.127490260e-08f, 2.482062362e-10f, 1.257800672e-13f};
__device__ __constant__ const float GH_LOGW[10] = {-1.344028046e+00f, -1.821769289e+00f, -2.788614499e+00f, -4.268852429e+00f, -6.303382958e+00f,
                                                   -8.957045728e+00f, -1.233342407e+01f, -1.660789550e+01f, -2.211676112e+01f, -2.970424151e+01f};

struct Lik { int type; float p0, p1, lgc; const float* p0_dev; };

constexpr int LIK_MAX_GLOB = 16;
struct LikReduceArgs {
    Lik lik;
    const float* fmean; const float* fvar; const float* Y;
    const float* kl[IWVI_MAX_KL]; int kl_dims[IWVI_MAX_KL]; int n_kl;
    long long B, stride_b, stride_k; int K, Dy, K_total, mode_vi;
    float* ms; float* logp;
    double* elbo; unsigned long long* ticket; double scale;
    const double* klg[LIK_MAX_GLOB]; int klg_n[LIK_MAX_GLOB]; int n_glob;
};

template <int SEG>
__device__ __forceinline__ float lseg_max(float v) {
#pragma unroll
    for (int o = SEG / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
template <int SEG>
__device__ __forceinline__ double lseg_sum(double v) {
#pragma unroll
    for (int o = SEG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int LIK_THREADS = 256;

// One chunk of a segment's running log-sum-exp (k_lik_elbo's own): L is the lane's term, -inf where the lane has none (on = false).  The shift is
// the running float maximum, the sum float64.  A chunk whose every term is -inf adds nothing (no exp(-inf + inf)), and a lane set that calls
// this with no term at all leaves (m, ssum) exactly as they were: nm = m, and exp(m - nm) = exp(0) = 1 exactly.
template <int SEG>
__device__ __forceinline__ void lseg_lse_step(float L, bool on, float& m, double& ssum) {
    const float nm = fmaxf(m, lseg_max<SEG>(L));
    const double cs = lseg_sum<SEG>(on && nm != -INFINITY ? (double)__expf(L - nm) : 0.0);
    ssum = (m == -INFINITY ? 0.0 : ssum * (double)__expf(m - nm)) + cs;
    m = nm;
}

// ---- iwvi_lik_predict_mixture: the Monte Carlo predictive mixture over the S draws of a test point, ONE launch (no workspace, no ticket) ----
struct LikMixArgs {
    Lik lik;
    const float* fmean; const float* fvar; const float* Y;      // Y: NULL exactly when logp is
    long long N, stride_n, stride_s; int S, Dy;
    float* logp; float* mean; float* var;                        // mean and var: both or neither
};
constexpr int MIX_MAX_BLOCKS = 1024;      // four workgroups per CU; beyond that the points are grid-strided

// k_lik_elbo's layout: SEG lanes own a point and stride over its S draws, a workgroup takes LIK_THREADS / SEG points per pass.  OPS gives
// the per-element arithmetic of the elementwise kernels: density(mu, v, y) (without the target's constant), target_const(y) -- HAS_CONST:
// summed once per point and added outside the log-sum-exp, as k_xl_elbo does -- and mean_var(mu, v, e, var).
// The moment sums loop the OUTPUTS outermost: two float64 accumulators per lane whatever Dy is (a per-lane array of Dy of them would be
// indexed dynamically and spill), at the price of walking a point's rows once per output -- they stay in the cache between the walks.
template <int SEG, class OPS>
__device__ __forceinline__ void mix_points(const LikMixArgs& g, const OPS& ops) {
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;           // points per pass
    const int S = g.S, Dy = g.Dy;
    for (long long b0 = (long long)blockIdx.x * PPP; b0 < g.N; b0 += (long long)gridDim.x * PPP) {   // (uniform in the workgroup)
        const long long b = b0 + sg;
        const bool live = b < g.N;                    // uniform within a segment
        if (g.logp) {
            double cb = 0.0;
            if (OPS::HAS_CONST) {
                if (live)
                    for (int d = sl; d < Dy; d += SEG) cb += (double)ops.target_const(g.Y[b * Dy + d]);
                cb = lseg_sum<SEG>(cb);
            }
            float m = -INFINITY;
            double ssum = 0.0;
            for (int s0 = 0; s0 < S; s0 += SEG) {
                const int s = s0 + sl;
                const bool on = live && s < S;
                float L = -INFINITY;
                if (on) {
                    const long long t = (b * g.stride_n + s * g.stride_s) * Dy;
                    double acc = 0.0;                 // (float32 inside an output; the Dy of them are added in float64 and rounded once)
                    for (int d = 0; d < Dy; ++d) acc += (double)ops.density(g.fmean[t + d], g.fvar[t + d], g.Y[b * Dy + d]);
                    L = (float)acc;
                }
                lseg_lse_step<SEG>(L, on, m, ssum);
            }
            // (every draw at -inf: m = -inf, ssum = 0 -> -inf + log 0 = -inf, not NaN)
            if (live && sl == 0) g.logp[b] = (float)((double)m + log(ssum) - log((double)S) + cb);
        }
        if (g.mean) {
            for (int d = 0; d < Dy; ++d) {
                double se = 0.0, se2 = 0.0;              // sum_s E_s, sum_s (Var_s + E_s^2)
                if (live)
                    for (int s = sl; s < S; s += SEG) {
                        const long long t = (b * g.stride_n + s * g.stride_s) * Dy + d;
                        float e, v;
                        ops.mean_var(g.fmean[t], g.fvar[t], e, v);
                        se += (double)e;
                        se2 += (double)v + (double)e * (double)e;
                    }
                se = lseg_sum<SEG>(se);
                se2 = lseg_sum<SEG>(se2);
                if (live && sl == 0) {
                    const double mn = se / (double)S;
                    g.mean[b * Dy + d] = (float)mn;
                    g.var[b * Dy + d] = (float)(se2 / (double)S - mn * mn);      // the subtraction cancels: float64, rounded once
                }
            }
        }
    }
}

inline unsigned mix_blocks(long long N, int seg) {
    const long long ppp = LIK_THREADS / seg, passes = (N + ppp - 1) / ppp;
    return (unsigned)(passes < MIX_MAX_BLOCKS ? passes : MIX_MAX_BLOCKS);
}

struct LikBwdArgs {
    Lik lik;
    const float* fmean; const float* fvar; const float* Y; int Dy;
    const float* kl[IWVI_MAX_KL]; int kl_dims[IWVI_MAX_KL]; int n_kl;
    long long B; int K; double scale; int mode_vi;
    const float* lse_global; int K_total;
    float* w; float* d_mean; float* d_var; double* part;   // part[0..B) = lse - log K, part[B..2B) = d param[0] share
};

// ---- csrc/likelihood_multiclass.hip (IWVI_LIK_MULTICLASS: lik.p0 = epsilon, lik.p1 = Dy = the number of classes, Y one column of labels) ----
int mc_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_mc_elbo<SEG>
int mc_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_mc_elbo_bwd (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp) -> out [T]; 2: predict_mean_and_var -> out, out2 [T, C]
int mc_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int C,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int mc_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_mc_mix<SEG>

// ---- csrc/likelihood_explink.hip (IWVI_LIK_POISSON: lik.p0 = binsize; _EXPONENTIAL: no parameter; _GAMMA: lik.p0 / *lik.p0_dev = shape) ----
inline bool xl_type(int type) { return type >= IWVI_LIK_POISSON && type <= IWVI_LIK_GAMMA; }
int xl_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_xl_elbo<SEG>
int xl_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_xl_elbo_bwd (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp), 2: predict_mean_and_var (out, out2) -- all [T, Dy]
int xl_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int xl_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_xl_mix<SEG>

}  // namespace iwvi
