// Heteroskedastic Gaussian: a second latent GP on the log noise variance (include/iwvi_hip.h: IWVI_LIK_HETERO_GAUSSIAN), behind the
// iwvi_lik_* entry points of csrc/likelihood_tail.hip.  The final layer has Dy = 2 Dt outputs for Dt target columns: columns 0 .. Dt-1 are
// the mean function f, columns Dt .. 2 Dt-1 are g, the LOG NOISE VARIANCE of the same target column -- like the MultiClass, the expectation
// couples outputs of one sample (d with Dt + d), and the targets are narrower than the moments (Y has Dt columns):
//   logp(f, g, y) = -1/2 log 2 pi - g / 2 - (y - f)^2 exp(-g) / 2.
// Under N(f; m_f, v_f) N(g; m_g, v_g) the variational expectation is a CLOSED FORM, as for the exp-link family:
//   E = -1/2 log 2 pi - m_g / 2 - q r / 2,     q = (y - m_f)^2 + v_f,   r = exp(a),   a = -m_g + v_g / 2
//   dE/dm_f = (y - m_f) r,   dE/dv_f = -r / 2,   dE/dm_g = -1/2 + q r / 2,   dE/dv_g = -q r / 4
// -- one exp per (point, sample, target column), no quadrature, no division by sqrt(v) and hence no variance floor in the training path.
// THE CLIP: every exponent (a; -g in logp; m_g + v_g / 2 in predict_mean_and_var; the nodes' g_i in predict_density; g / 2 in the sampler)
// is clipped to [-60, 60] before exp, so float32 cannot overflow (exp(60) = 1.1e26, and q r stays finite for q < 3e12).  The heads are the
// gradient of the value AS COMPUTED: through an active clip (|a| > 60) the derivative is zero, as tf.clip_by_value gives -- the m_g / v_g
// parts through r vanish there and dE/dm_g is the -1/2 of the linear term alone; the m_f / v_f heads keep the clipped r.  (MultiClass's rule.)
// predict_density = log int N(y; m_f, v_f + exp(g)) N(g; m_g, v_g) dg by the 20-point rule of likelihood_common.h over g IN LOG SPACE (the
// largest term first, then the sum), v_g floored at LIK_V_FLOOR as the other quadratures; predict_mean_and_var = (m_f, v_f + exp(m_g + v_g / 2)),
// the exact moments.  There is no parameter and nothing is trained: part[B..2B) = 0.
#include "likelihood_common.h"

namespace iwvi {

constexpr float HG_CLIP = 60.f;
constexpr float HG_HALF_LOG_2PI = 0.91893853320467274f;

// the clipped exponent (a NaN stays a NaN); in: the clip is not active, so the derivative passes (the ends themselves pass, as tf.clip_by_value)
__device__ __forceinline__ float hg_clip(float a, bool& in) {
    in = a >= -HG_CLIP && a <= HG_CLIP;
    const float c = fminf(fmaxf(a, -HG_CLIP), HG_CLIP);
    return a != a ? a : c;
}
__device__ __forceinline__ float hg_clip(float a) { bool in; return hg_clip(a, in); }

// the closed-form expectation of one target column; e = y - m_f, q, r and whether the derivative passes through r are left for the heads
__device__ __forceinline__ float hg_ve(float y, float mf, float vf, float mg, float vg, float& e, float& q, float& r, bool& in) {
    e = y - mf;
    q = fmaf(e, e, vf);
    r = expf(hg_clip(fmaf(0.5f, vg, -mg), in));
    return fmaf(-0.5f * q, r, fmaf(-0.5f, mg, -HG_HALF_LOG_2PI));
}
// logp(f, g, y)
__device__ __forceinline__ float hg_logp(float y, float f, float g) {
    const float e = y - f;
    return fmaf(-0.5f * e * e, expf(hg_clip(-g)), fmaf(-0.5f, g, -HG_HALF_LOG_2PI));
}
// predict_mean_and_var of one target column
__device__ __forceinline__ void hg_mean_var(float mf, float vf, float mg, float vg, float& em, float& ev) {
    em = mf;
    ev = vf + expf(hg_clip(fmaf(0.5f, vg, mg)));
}
// log N(y; m_f, s) + log w at one node, s = max(v_f, 0) + exp(clip(g_i)) > 0
__device__ __forceinline__ float hg_node(float e2, float vf, float gi, float logw) {
    const float s = vf + expf(hg_clip(gi));
    return logw - HG_HALF_LOG_2PI - 0.5f * logf(s) - 0.5f * e2 / s;
}
// predict_density of one target column: log sum_i exp(log N(y; m_f, v_f + exp(g_i)) + log w_i), g_i = m_g +- sqrt(2 v_g) x_j -- the largest
// term first, then the sum (a node is evaluated twice; nothing is kept in scratch).  Every term at -inf (e^2 / s overflowed): -inf, not NaN.
__device__ __forceinline__ float hg_density(float y, float mf, float vf, float mg, float vg) {
    const float e = y - mf, e2 = e * e;
    vf = fmaxf(vf, 0.f);
    const float a = sqrtf(2.f * fmaxf(vg, LIK_V_FLOOR));
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        mx = fmaxf(mx, fmaxf(hg_node(e2, vf, mg + xa, GH_LOGW[j]), hg_node(e2, vf, mg - xa, GH_LOGW[j])));
    }
    if (mx == -INFINITY) return mx;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        s += expf(hg_node(e2, vf, mg + xa, GH_LOGW[j]) - mx) + expf(hg_node(e2, vf, mg - xa, GH_LOGW[j]) - mx);
    }
    return mx + logf(s);
}

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint: the cores of likelihood_common.h over the closed form.  A point has no state of its
// own and no constant outside the log-sum-exp; a sample's row of moments is [f_0 .. f_(Dt-1), g_0 .. g_(Dt-1)] and Y's row has Dt columns.
// A sample has 2 Dy heads (d_mean and d_var of both halves of its row); nothing is trained: ds passes through unchanged.
// ------------------------------------------------------------------------------------------
struct HgOps {
    static constexpr bool HAS_CONST = false;
    struct Point {};
    int Dt;
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float*, long long, bool, int) const { return {}; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float* var, const float* Y, long long b) const {
        float acc = 0.f, e, q, r;
        bool in;
        for (int d = 0; d < Dt; ++d) acc += hg_ve(Y[b * Dt + d], mu[d], var[d], mu[Dt + d], var[Dt + d], e, q, r, in);
        return acc;
    }
    __device__ __forceinline__ double heads(const Point&, const float* mu, const float* var, const float* Y, long long b, float wt,
                                            float* dm, float* dv, double ds) const {
        for (int d = 0; d < Dt; ++d) {
            float e, q, r;
            bool in;
            hg_ve(Y[b * Dt + d], mu[d], var[d], mu[Dt + d], var[Dt + d], e, q, r, in);
            const float qr = in ? q * r : 0.f;               // d (q r) / d a: zero through an active clip
            if (dm) { dm[d] = wt * (e * r); dm[Dt + d] = wt * fmaf(0.5f, qr, -0.5f); }
            if (dv) { dv[d] = wt * (-0.5f * r); dv[Dt + d] = wt * (-0.25f * qr); }
        }
        return ds;
    }
};

// THE GRID: k_xl_elbo's strided one (up to HG_MAX_BLOCKS workgroups, each taking as many passes of LIK_THREADS / SEG points as the grid leaves
// it -- ONE pass each at B = 1024), not the one-pass grid of the quadrature kernels.  A sample costs a handful of FMAs and one exp per target
// column, as the exp-link family's: the one-pass form exists because the loop around a QUADRATURE cost k_lik_elbo a wave of occupancy, which
// a closed form has not got to lose, and the strided grid bounds the number of workgroups whatever B is.
constexpr int HG_MAX_BLOCKS = 1024;     // four workgroups per CU

template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_hg_elbo(LikReduceArgs g) {
    const HgOps ops{g.Dy / 2};
    elbo_points<SEG, true>(g, ops);
}

__global__ __launch_bounds__(256) void k_hg_elbo_bwd(LikBwdArgs a) {
    const HgOps ops{a.Dy / 2};
    elbo_bwd_point(a, ops);
}

// ------------------------------------------------------------------------------------------
// Elementwise callables on ROWS: one lane per (row t, target column d), reading columns d and Dt + d of the row's 2 Dt moments; n = T Dt
// elements and every output is [T, Dt].  MODE 0: variational_expectations (the closed form); 1: predict_density (Fvar == NULL: logp);
// 2: predict_mean_and_var.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_hg_elem(const float* __restrict__ Fmu, const float* __restrict__ Fvar, const float* __restrict__ Y,
                                                 long long n, int Dt, long long row_div, long long row_mod,
                                                 float* __restrict__ out, float* __restrict__ out2) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const long long t = idx / Dt;
        const int d = (int)(idx - t * Dt);
        const long long jf = t * 2 * Dt + d, jg = jf + Dt;
        if (MODE == 2) {
            float em, ev;
            hg_mean_var(Fmu[jf], Fvar[jf], Fmu[jg], Fvar[jg], em, ev);
            out[idx] = em; out2[idx] = ev;
            continue;
        }
        const float y = Y[((t / row_div) % row_mod) * Dt + d];
        if (MODE == 0) {
            float e, q, r;
            bool in;
            out[idx] = hg_ve(y, Fmu[jf], Fvar[jf], Fmu[jg], Fvar[jg], e, q, r, in);
            continue;
        }
        if (!Fvar) { out[idx] = hg_logp(y, Fmu[jf], Fmu[jg]); continue; }
        out[idx] = hg_density(y, Fmu[jf], Fvar[jf], Fmu[jg], Fvar[jg]);
    }
}

// ------------------------------------------------------------------------------------------
// iwvi_lik_predict_mixture: mix_points' layout (SEG lanes per point striding over its S draws, LIK_THREADS / SEG points per pass, grid-strided
// beyond MIX_MAX_BLOCKS workgroups) with a point loop of its own, since a target column reads TWO columns of a draw's row.  One launch, no
// workspace.  A draw's density is the sum over its Dt target columns (float32 inside a column, added in float64 and rounded once); the
// log-sum-exp over the draws and the moment sums are float64.  The moment sums loop the target columns outermost: two accumulators per lane
// whatever Dt is.  out_mean / out_var are [N, Dt].
// ------------------------------------------------------------------------------------------
template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_hg_mix(LikMixArgs g) {
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;
    const int S = g.S, Dy = g.Dy, Dt = g.Dy / 2;
    for (long long b0 = (long long)blockIdx.x * PPP; b0 < g.N; b0 += (long long)gridDim.x * PPP) {   // (uniform in the workgroup)
        const long long b = b0 + sg;
        const bool live = b < g.N;                    // uniform within a segment
        if (g.logp) {
            float m = -INFINITY;
            double ssum = 0.0;
            for (int s0 = 0; s0 < S; s0 += SEG) {
                const int s = s0 + sl;
                const bool on = live && s < S;
                float L = -INFINITY;
                if (on) {
                    const long long t = (b * g.stride_n + s * g.stride_s) * Dy;
                    double acc = 0.0;
                    for (int d = 0; d < Dt; ++d)
                        acc += (double)hg_density(g.Y[b * Dt + d], g.fmean[t + d], g.fvar[t + d], g.fmean[t + Dt + d], g.fvar[t + Dt + d]);
                    L = (float)acc;
                }
                lseg_lse_step<SEG>(L, on, m, ssum);
            }
            // (every draw at -inf: m = -inf, ssum = 0 -> -inf + log 0 = -inf, not NaN)
            if (live && sl == 0) g.logp[b] = (float)((double)m + log(ssum) - log((double)S));
        }
        if (g.mean) {
            for (int d = 0; d < Dt; ++d) {
                double se = 0.0, se2 = 0.0;              // sum_s E_s, sum_s (Var_s + E_s^2)
                if (live)
                    for (int s = sl; s < S; s += SEG) {
                        const long long t = (b * g.stride_n + s * g.stride_s) * Dy + d;
                        float e, v;
                        hg_mean_var(g.fmean[t], g.fvar[t], g.fmean[t + Dt], g.fvar[t + Dt], e, v);
                        se += (double)e;
                        se2 += (double)v + (double)e * (double)e;
                    }
                se = lseg_sum<SEG>(se);
                se2 = lseg_sum<SEG>(se2);
                if (live && sl == 0) {
                    const double mn = se / (double)S;
                    g.mean[b * Dt + d] = (float)mn;
                    g.var[b * Dt + d] = (float)(se2 / (double)S - mn * mn);      // the subtraction cancels: float64, rounded once
                }
            }
        }
    }
}

int hg_check_dim(int Dy, const char* what) {
    if (Dy < 2 || (Dy & 1) || Dy > IWVI_MAX_P) {
        set_error("%s: the heteroskedastic Gaussian needs an even Dy = 2 x (target columns) in 2..%d -- mean columns, then log noise "
                  "variance columns --, got %d", what, IWVI_MAX_P, Dy);
        return IWVI_ERR_ARG;
    }
    return IWVI_OK;
}

int hg_launch_elbo(const LikReduceArgs& g, hipStream_t stream) {
    return seg_dispatch(g.K, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        const long long passes = lik_passes(g.B, SEG);
        hipLaunchKernelGGL(k_hg_elbo<SEG>, dim3((unsigned)(passes < HG_MAX_BLOCKS ? passes : HG_MAX_BLOCKS)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_hg_elbo");
    });
}

int hg_launch_mix(const LikMixArgs& g, hipStream_t stream) {
    return seg_dispatch(g.S, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_hg_mix<SEG>, dim3(mix_blocks(g.N, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_hg_mix");
    });
}

int hg_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_hg_elbo_bwd, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
    return check_launch("k_hg_elbo_bwd");
}

int hg_launch_elem(const char* what, int mode, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream) {
    const int Dt = Dy / 2;
    const long long n = T * Dt;
    return launch_elem_mode(what, mode, n, [&](auto m, int blocks) {
        hipLaunchKernelGGL(k_hg_elem<decltype(m)::value>, dim3(blocks), dim3(256), 0, stream, Fmu, Fvar, Y, n, Dt, row_div, row_mod, out, out2);
    });
}

}  // namespace iwvi
