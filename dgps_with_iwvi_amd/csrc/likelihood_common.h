// What csrc/likelihood_tail.hip, csrc/likelihood_multiclass.hip, csrc/likelihood_explink.hip, csrc/likelihood_bounded.hip and
// csrc/likelihood_hetero.hip (IWVI_LIK_HETERO_GAUSSIAN: HgOps, its launchers at the end of this file) share: the
// Gauss-Hermite tables, the quadrature's variance floor, the probit link's jitter and the float64 digamma of a launch-wide parameter, the
// kernel-argument structs of the iwvi_lik_* entry points and the segment reductions (moved here verbatim from likelihood_tail.hip), the
// point loop of iwvi_lik_predict_mixture for the types whose outputs are independent (mix_points), the bound's reduction and the heads of its
// adjoint for every type (elbo_points, elbo_bwd_point: one core each over a small compile-time policy per family), the SEG and the mode
// dispatch of the launchers, and the launchers of the multi-class, the exp-link and the bounded-target kernels, which the entry points of
// likelihood_tail.hip call for IWVI_LIK_MULTICLASS, for IWVI_LIK_POISSON / _EXPONENTIAL / _GAMMA and for IWVI_LIK_BETA / _ORDINAL.
#pragma once
#include <type_traits>
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

// dE/dv = sum_i w_i g'(f_i) x_i / sqrt(2 v) is 0/0 at v = 0 (the forward clamps a float32 variance that undershot at exactly 0); its limit is
// g''(mu) / 2.  The variance is floored here, for the value and the heads alike (the heads stay the gradient of the value that is
// computed): sqrt(2 v) >= 1.4e-4, which moves E by g'' 5e-9 -- below float32 resolution -- and leaves the quotient finite.
constexpr float LIK_V_FLOOR = 1e-8f;
constexpr float LIK_JIT = 1e-3f;                  // GPflow's inv_probit jitter: p = Phi(f) (1 - 2 jit) + jit

// psi(x), x > 0, float64 -- for a launch-wide parameter (the Gamma's shape, the Beta's scale), once per wave: the recurrence
// psi(x) = psi(x + 1) - 1 / x up to x >= 6 (six steps at the most: the loop is bounded whatever the device scalar holds), then the
// asymptotic series (next term 691 / (32760 x^12) < 1e-11)
__device__ __forceinline__ double digamma_f64(double x) {
    double r = 0.0;
    for (int i = 0; i < 6 && x < 6.0; ++i) { r -= 1.0 / x; x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    return r + log(x) - 0.5 * i - i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0)))));
}

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
template <int SEG, class T>
__device__ __forceinline__ T lseg_sum(T v) {                  // float64 for the sums over samples, float32 for a point's constant
#pragma unroll
    for (int o = SEG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int LIK_THREADS = 256;

// One chunk of a segment's running log-sum-exp: L is the lane's term, -inf where the lane has none (on = false).  The shift is
// the running float maximum, the sum float64.  A chunk whose every term is -inf adds nothing (no exp(-inf + inf)), and a lane set that calls
// this with no term at all leaves (m, ssum) exactly as they were: nm = m, and exp(m - nm) = exp(0) = 1 exactly.
// GUARD = false is the bound's step (elbo_points): bit-equal while any term so far is finite; with every term at -inf it gives NaN, not -inf.
template <int SEG, bool GUARD = true>
__device__ __forceinline__ void lseg_lse_step(float L, bool on, float& m, double& ssum) {
    const float nm = fmaxf(m, lseg_max<SEG>(L));
    const double cs = lseg_sum<SEG>(on && (!GUARD || nm != -INFINITY) ? (double)__expf(L - nm) : 0.0);
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

// the passes of LIK_THREADS / seg points that cover n points
inline long long lik_passes(long long n, int seg) {
    const long long ppp = LIK_THREADS / seg;
    return (n + ppp - 1) / ppp;
}
inline unsigned mix_blocks(long long N, int seg) {
    const long long passes = lik_passes(N, seg);
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

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint, ONE core each for every likelihood.  What differs between the families is a policy OPS
// (LikQuadOps in likelihood_tail.hip, McOps in likelihood_multiclass.hip, XlOps in likelihood_explink.hip, BoOps<TYPE> in
// likelihood_bounded.hip; no runtime branch on the type here):
//   Point point<SEG, GRAD>(Y, b, live, sl)   a data point's state, formed once by the SEG lanes that own it: nothing (Gaussian, Bernoulli,
//                                            Student-t), the clamped label (MultiClass), cb = sum_d c0(y_bd) in float32 (exp link; GRAD: also
//                                            the point's part of d / d shape)
//   HAS_CONST, point_const(pt)               whether the point carries a constant cb that stays OUTSIDE the log-sum-exp over the samples
//   expect(pt, mu, var, Y, b)                one sample's expectation summed over its outputs, float32 (mu, var: the sample's row of moments)
//   heads(pt, mu, var, Y, b, wt, dm, dv, ds) one sample's heads for its weight wt into dm / dv (its rows of d_mean / d_var; NULL: not asked
//                                            for); returns the lane's float64 share ds of d param[0] with the sample's part added
// ------------------------------------------------------------------------------------------
// The last workgroup to arrive adds the published logp up in a fixed order: release / ticket / acquire, the only synchronisation between
// workgroups in the likelihood files.  red: LIK_THREADS doubles of LDS, is_last: one LDS word.
__device__ __forceinline__ void elbo_ticket_sum(const LikReduceArgs& g, double* red, int& is_last) {
    if (!g.elbo) return;
    const int tid = threadIdx.x;
    // ---- publish this workgroup's logp, draw a ticket, the last arriver sums everything ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t = __hip_atomic_fetch_add(g.ticket, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == (unsigned long long)gridDim.x - 1);
        if (last) {
            __hip_atomic_store(g.ticket, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        is_last = last;
    }
    __syncthreads();
    if (!is_last) return;
    double acc = 0.0;
    for (long long b = tid; b < g.B; b += LIK_THREADS) acc += (double)g.logp[b];
    red[tid] = acc;
    __syncthreads();
    for (int s2 = LIK_THREADS / 2; s2 > 0; s2 >>= 1) {
        if (tid < s2) red[tid] += red[tid + s2];
        __syncthreads();
    }
    if (tid == 0) {
        double kl = 0.0;
        for (int i = 0; i < g.n_glob; ++i)
            for (int c = 0; c < g.klg_n[i]; ++c) kl += g.klg[i][c];
        *g.elbo = red[0] * g.scale - kl;                                                              // models.py:150
    }
}

// The reduction (csrc/lv_elbo.hip: k_elbo with the policy's expectation in place of the Gaussian closed form): SEG lanes per data point, one
// lane per sample walking its outputs; float32 inside a sample, the log-sum-exp over K and the sum over the points in float64.  A workgroup
// takes LIK_THREADS / SEG points per pass.  STRIDED: as many passes as the grid leaves it (k_xl_elbo, launched on up to XL_MAX_BLOCKS
// workgroups); otherwise ONE pass, the launcher giving every pass a workgroup of its own (k_lik_elbo, k_mc_elbo).  The one-pass form is not
// the loop run once: with the loop around the quadrature k_lik_elbo compiled to 106 VGPRs for 80 -- four waves on a SIMD for six -- and
// k_mc_elbo to 111 for 108; without it both keep the resource rows they had (the time at configs[2] did not tell the two forms apart).
// The measurements behind the two grids stand above those kernels.
template <int SEG, bool STRIDED, class OPS>
__device__ __forceinline__ void elbo_points(const LikReduceArgs& g, const OPS& ops) {
    __shared__ double red[LIK_THREADS];
    __shared__ int is_last;
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;           // points per pass
    const int K = g.K, Dy = g.Dy;
    auto pass = [&](long long b0) {                   // the PPP points from b0 on (b0: uniform in the workgroup)
        const long long b = b0 + sg;
        const bool live = b < g.B;                    // uniform within a segment
        const auto pt = ops.template point<SEG, false>(g.Y, b, live, sl);
        float m = -INFINITY;
        double ssum = 0.0, lsum = 0.0;
        for (int k0 = 0; k0 < K; k0 += SEG) {
            const int k = k0 + sl;
            const bool on = live && k < K;
            float L = -INFINITY;
            if (on) {
                const long long t = b * g.stride_b + k * g.stride_k;
                float acc = ops.expect(pt, g.fmean + t * Dy, g.fvar + t * Dy, g.Y, b);
                for (int i = 0; i < g.n_kl; ++i)
                    for (int d = 0; d < g.kl_dims[i]; ++d) acc -= g.kl[i][t * g.kl_dims[i] + d];
                L = acc;
            }
            if (g.mode_vi) { lsum += lseg_sum<SEG>(on ? (double)L : 0.0); continue; }
            lseg_lse_step<SEG, false>(L, on, m, ssum);
        }
        if (live && sl == 0) {
            if (g.mode_vi) {
                double lp = lsum / (double)K;                                                         // models.py:84
                if constexpr (OPS::HAS_CONST) lp += (double)ops.point_const(pt);
                if (g.logp) g.logp[b] = (float)lp;
            } else {
                if constexpr (OPS::HAS_CONST) m += ops.point_const(pt);                               // c0 outside the log-sum-exp
                if (g.ms) { g.ms[2 * b] = m; g.ms[2 * b + 1] = (float)ssum; }
                if (g.logp) g.logp[b] = (float)((double)m + log(ssum) - log((double)g.K_total));     // models.py:148
            }
        }
    };
    if constexpr (STRIDED) {
        for (long long b0 = (long long)blockIdx.x * PPP; b0 < g.B; b0 += (long long)gridDim.x * PPP) pass(b0);
    } else {
        pass((long long)blockIdx.x * PPP);
    }
    elbo_ticket_sum(g, red, is_last);
}

// Heads of the bound's adjoint (csrc/backward.hip: k_elbo_bwd with the policy's expectation and heads): one wave per data point, lanes over
// its K samples striding by 64.  Pass 1: L_nk (without the point's constant: it cancels in the weights) and the running (max, sum exp);
// pass 2: the weights and the heads of every sample.
template <class OPS>
__device__ __forceinline__ void elbo_bwd_point(const LikBwdArgs& a, const OPS& ops) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int Dy = a.Dy;
    const auto pt = ops.template point<64, true>(a.Y, b, true, lane);
    auto logw = [&](long long t) {
        float l = ops.expect(pt, a.fmean + t * Dy, a.fvar + t * Dy, a.Y, b);
        for (int i = 0; i < a.n_kl; ++i)
            for (int q = 0; q < a.kl_dims[i]; ++q) l -= a.kl[i][t * a.kl_dims[i] + q];
        return l;
    };
    const bool one = a.K <= 64;                          // every lane holds its only sample's L_nk: no second evaluation
    float Lc = -INFINITY, mx = -INFINITY;
    double se = 0.0;
    if (a.mode_vi) {                                    // models.py:84: mean over the samples -> uniform weights
        for (int k = lane; k < a.K; k += 64) se += (double)logw(b * a.K + k);
        se = lseg_sum<64>(se);
    } else {
        for (int k = lane; k < a.K; k += 64) { Lc = logw(b * a.K + k); mx = fmaxf(mx, Lc); }
        mx = lseg_max<64>(mx);
        if (a.lse_global) {                             // weights against the whole job's normaliser, which carries the constant: exp(L - LSE)
            mx = a.lse_global[b]; se = 1.0;
            if constexpr (OPS::HAS_CONST) mx -= ops.point_const(pt);
        } else {
            for (int k = lane; k < a.K; k += 64) se += (double)__expf((one ? Lc : logw(b * a.K + k)) - mx);
            se = lseg_sum<64>(se);
        }
    }
    double ds = 0.0;
    for (int k = lane; k < a.K; k += 64) {
        const long long t = b * a.K + k;
        float wt;
        if (a.mode_vi) wt = (float)(a.scale / (double)a.K);
        else wt = (float)(a.scale * (double)__expf((one ? Lc : logw(t)) - mx) / se);
        if (a.w) a.w[t] = wt;
        ds = ops.heads(pt, a.fmean + t * Dy, a.fvar + t * Dy, a.Y, b, wt, a.d_mean ? a.d_mean + t * Dy : nullptr,
                       a.d_var ? a.d_var + t * Dy : nullptr, ds);
    }
    ds = lseg_sum<64>(ds);
    if (lane == 0) {
        double lp = a.mode_vi ? se / (double)a.K : (double)mx + log(se) - log((double)(a.lse_global ? a.K_total : a.K));
        if constexpr (OPS::HAS_CONST) lp = (double)ops.point_const(pt) + lp;
        a.part[b] = lp;
        a.part[a.B + b] = ds;
    }
}

// K (the reductions) or S (the mixtures) -> the narrowest segment that gives every sample a lane: f(integral_constant<int, SEG>)
template <class F>
inline int seg_dispatch(int n, F&& f) {
    if (n <= 4) return f(std::integral_constant<int, 4>{});
    if (n <= 8) return f(std::integral_constant<int, 8>{});
    if (n <= 16) return f(std::integral_constant<int, 16>{});
    if (n <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

// the elementwise kernels' grid: n elements, 256 a workgroup, grid-strided beyond 4096 workgroups
inline int elem_blocks(long long n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

// the elementwise kernels' launch where the mode is a runtime value (the launchers of the multi-class and the exp-link files; lik_elementwise
// of likelihood_tail.hip knows its MODE at compile time and launches directly): launch(integral_constant<int, MODE>, blocks)
template <class F>
inline int launch_elem_mode(const char* what, int mode, long long n, F&& launch) {
    const int blocks = elem_blocks(n);
    if (mode == 0) launch(std::integral_constant<int, 0>{}, blocks);
    else if (mode == 1) launch(std::integral_constant<int, 1>{}, blocks);
    else launch(std::integral_constant<int, 2>{}, blocks);
    return check_launch(what);
}

// ---- csrc/likelihood_tail.hip: the descriptor checks every iwvi_lik_* entry point shares (csrc/likelihood_sample.hip calls them too) ----
int take_lik(const iwvi_lik_desc* d, Lik& L, const char* what, bool need_df2 = false);
int mc_check_classes(const Lik& L, int Dy, const char* what);

// ---- csrc/likelihood_multiclass.hip (IWVI_LIK_MULTICLASS: lik.p0 = epsilon, lik.p1 = Dy = the number of classes, Y one column of labels) ----
int mc_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_mc_elbo<SEG>
int mc_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_mc_elbo_bwd (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp) -> out [T]; 2: predict_mean_and_var -> out, out2 [T, C]
int mc_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int C,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int mc_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_mc_mix<SEG>

// ---- csrc/likelihood_hetero.hip (IWVI_LIK_HETERO_GAUSSIAN: no parameter; Dy = 2 Dt moments per row -- Dt means, then Dt log noise variances --,
//      Y and every elementwise / mixture output Dt columns).  Every exponent is clipped to [-60, 60] before exp, and the heads are the gradient
//      of the value AS COMPUTED: zero through an active clip, MultiClass's rule ----
int hg_check_dim(int Dy, const char* what);                                       // Dy even, in 2..IWVI_MAX_P (the limit in the text)
int hg_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_hg_elbo<SEG>
int hg_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_hg_elbo_bwd (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp), 2: predict_mean_and_var (out, out2) -- all [T, Dy / 2]
int hg_launch_elem(const char* what, int mode, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int hg_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_hg_mix<SEG>

// ---- csrc/likelihood_explink.hip (IWVI_LIK_POISSON: lik.p0 = binsize; _EXPONENTIAL: no parameter; _GAMMA: lik.p0 / *lik.p0_dev = shape) ----
inline bool xl_type(int type) { return type >= IWVI_LIK_POISSON && type <= IWVI_LIK_GAMMA; }
int xl_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_xl_elbo<SEG>
int xl_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_xl_elbo_bwd (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp), 2: predict_mean_and_var (out, out2) -- all [T, Dy]
int xl_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int xl_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_xl_mix<SEG>

// ---- csrc/likelihood_bounded.hip (IWVI_LIK_BETA: lik.p0 / *lik.p0_dev = scale; _ORDINAL: lik.p0_dev = [sigma, e_0 .. e_(n-1)], lik.p1 = n) ----
inline bool bo_type(int type) { return type == IWVI_LIK_BETA || type == IWVI_LIK_ORDINAL; }
int bo_launch_elbo(const LikReduceArgs& g, hipStream_t stream);                   // k_bo_elbo<TYPE, SEG>
int bo_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream);                  // k_bo_elbo_bwd<TYPE> (the caller launches k_lik_finish behind it)
// mode 0: variational_expectations, 1: predict_density (Fvar == NULL: logp), 2: predict_mean_and_var (out, out2) -- all [T, Dy]
int bo_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream);
int bo_launch_mix(const LikMixArgs& g, hipStream_t stream);                       // k_bo_mix<TYPE, SEG>

}  // namespace iwvi
