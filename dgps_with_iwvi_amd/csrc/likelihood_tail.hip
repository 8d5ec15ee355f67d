// The bound's tail and the heads of its adjoint for likelihoods other than the Gaussian (include/iwvi_hip.h: iwvi_lik_*), and the
// likelihood's methods as elementwise callables.  The reference passes any GPflow-1.x likelihood to its models (models.py:66,105,134);
// the non-conjugate ones -- Bernoulli with the probit link, Student-t -- integrate by GPflow's ndiagquad: Gauss-Hermite, 20 points.
// The entry points at the end of this file serve every type of include/iwvi_hip.h: Gaussian, Bernoulli and Student-t by the kernels here,
// MultiClass by csrc/likelihood_multiclass.hip, the heteroskedastic Gaussian by csrc/likelihood_hetero.hip, Poisson / Exponential / Gamma (exp link, closed-form expectations) by csrc/likelihood_explink.hip,
// Beta / Ordinal (probit link, quadrature) by csrc/likelihood_bounded.hip.
// The layer stack is untouched: these kernels read the final layer's moments (and the local regularisers) the layer launch left in HBM.
#include "likelihood_common.h"   // the node tables GH_X / GH_W / GH_LOGW, LIK_V_FLOOR, LIK_JIT, Lik, the argument structs, lseg_*

namespace iwvi {

// g(f) = logp(f, y);  GRAD: also g'(f) and d g / d param[0]
template <bool GRAD>
__device__ __forceinline__ float lik_eval(const Lik& L, float p0, float f, float y, float& gp, float& gpar) {
    if (L.type == IWVI_LIK_BERNOULLI_PROBIT) {
        // Phi(f) = erfc(-f / sqrt 2) / 2 and 1 - Phi(f) = erfc(f / sqrt 2) / 2: neither tail cancels; 1 - p = (1 - Phi)(1 - 2 jit) + jit
        const float u = f * 0.70710678118654752f;
        const float p = 0.5f * erfcf(-u) * (1.f - 2.f * LIK_JIT) + LIK_JIT;
        const float q = 0.5f * erfcf(u) * (1.f - 2.f * LIK_JIT) + LIK_JIT;
        const bool one = (y == 1.f);
        if (GRAD) {
            const float dp = (1.f - 2.f * LIK_JIT) * 0.3989422804014327f * __expf(-0.5f * f * f);
            gp = one ? dp / p : -dp / q;
            gpar = 0.f;
        }
        return logf(one ? p : q);
    }
    const float e = y - f;
    if (L.type == IWVI_LIK_STUDENT_T) {
        const float s = p0, nu = L.p1, s2nu = s * s * nu;
        if (GRAD) {
            const float den = s2nu + e * e;
            gp = (nu + 1.f) * e / den;
            gpar = -1.f / s + (nu + 1.f) * e * e / (s * den);
        }
        return L.lgc - logf(s) - 0.5f * logf(nu * 3.14159265358979324f) - 0.5f * (nu + 1.f) * log1pf(e * e / s2nu);
    }
    if (GRAD) {
        gp = e / p0;
        gpar = -0.5f / p0 + 0.5f * e * e / (p0 * p0);
    }
    return -0.5f * logf(6.283185307179586f * p0) - 0.5f * e * e / p0;
}

// E_{N(f; mu, v)} g(f) by the rule; GRAD: dE/dmu, dE/dv, dE/dparam[0] by its reparameterised form (first derivatives only)
template <bool GRAD>
__device__ __forceinline__ float lik_quad(const Lik& L, float p0, float mu, float v, float y, float& dmu, float& dv, float& dpar) {
    const float a = sqrtf(2.f * fmaxf(v, LIK_V_FLOOR));
    float E = 0.f, s1 = 0.f, s2 = 0.f, sp = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        float gpa = 0.f, gpb = 0.f, qa = 0.f, qb = 0.f;
        const float ga = lik_eval<GRAD>(L, p0, mu + xa, y, gpa, qa);
        const float gb = lik_eval<GRAD>(L, p0, mu - xa, y, gpb, qb);
        E = fmaf(GH_W[j], ga + gb, E);
        if (GRAD) {
            s1 = fmaf(GH_W[j], gpa + gpb, s1);
            s2 = fmaf(GH_W[j] * GH_X[j], gpa - gpb, s2);
            sp = fmaf(GH_W[j], qa + qb, sp);
        }
    }
    if (GRAD) { dmu = s1; dv = s2 / a; dpar = sp; }
    return E;
}

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint: the cores of likelihood_common.h (elbo_points, elbo_bwd_point) over the quadrature,
// one output at a time (the reduction; the heads kernel keeps a body of its own, below).  A point has no state of its own.
// ------------------------------------------------------------------------------------------
struct LikQuadOps {
    static constexpr bool HAS_CONST = false;
    struct Point {};
    const Lik& L; float p0; int Dy;
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float*, long long, bool, int) const { return {}; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float* var, const float* Y, long long b) const {
        float acc = 0.f, d0, d1, d2;
        for (int d = 0; d < Dy; ++d) acc += lik_quad<false>(L, p0, mu[d], var[d], Y[b * Dy + d], d0, d1, d2);
        return acc;
    }
};

// A workgroup takes ONE pass of LIK_THREADS / SEG points (k_elbo takes 64 points in several passes: its per-sample work is a handful of
// FMAs; here a sample costs 20 x Dy evaluations of erfc / log, and 64 points per workgroup left configs[2] -- B = 1024 -- on 16 of the
// chip's 256 CUs: a Bernoulli evaluation took 101.6 us against 66.0 with the points spread -- profiles/likelihood_tail_time.json)
template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_lik_elbo(LikReduceArgs g) {
    const LikQuadOps ops{g.lik, g.lik.p0_dev ? *g.lik.p0_dev : g.lik.p0, g.Dy};
    elbo_points<SEG, false>(g, ops);
}

// Heads of the bound's adjoint: elbo_bwd_point's layout and steps (likelihood_common.h) in a body of its own.  Through the shared core this
// kernel compiled to 101 VGPRs for 115 and was SLOWER: a Bernoulli value + gradient on ten columns at configs[2] took 703.6-705.6 us against
// 697.3-703.0 with this body, three alternating pairs in one session (profiles/likcore_time.json) -- so it keeps the body, and a change to the
// core's lse_global branch, weight or part[] stores has to be made here as well.
__global__ __launch_bounds__(256) void k_lik_elbo_bwd(LikBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const float p0 = a.lik.p0_dev ? *a.lik.p0_dev : a.lik.p0;
    auto logw = [&](long long t) {
        float l = 0.f, d0, d1, d2;
        for (int j = 0; j < a.Dy; ++j)
            l += lik_quad<false>(a.lik, p0, a.fmean[t * a.Dy + j], a.fvar[t * a.Dy + j], a.Y[b * a.Dy + j], d0, d1, d2);
        for (int i = 0; i < a.n_kl; ++i)
            for (int q = 0; q < a.kl_dims[i]; ++q) l -= a.kl[i][t * a.kl_dims[i] + q];
        return l;
    };
    const bool one = a.K <= 64;                          // every lane holds its only sample's L_nk: no second evaluation
    float Lc = -INFINITY, mx = -INFINITY;
    double se = 0.0;
    if (a.mode_vi) {                                    // models.py:84: mean over the samples -> uniform weights
        for (int k = lane; k < a.K; k += 64) se += (double)logw(b * a.K + k);
        for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
    } else {
        for (int k = lane; k < a.K; k += 64) { Lc = logw(b * a.K + k); mx = fmaxf(mx, Lc); }
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if (a.lse_global) {                             // weights against the whole job's normaliser: exp(L - LSE)
            mx = a.lse_global[b]; se = 1.0;
        } else {
            for (int k = lane; k < a.K; k += 64) se += (double)__expf((one ? Lc : logw(b * a.K + k)) - mx);
            for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
        }
    }
    double ds = 0.0;
    for (int k = lane; k < a.K; k += 64) {
        const long long t = b * a.K + k;
        float wt;
        if (a.mode_vi) wt = (float)(a.scale / (double)a.K);
        else wt = (float)(a.scale * (double)__expf((one ? Lc : logw(t)) - mx) / se);
        if (a.w) a.w[t] = wt;
        for (int j = 0; j < a.Dy; ++j) {
            float dmu, dv, dp;
            lik_quad<true>(a.lik, p0, a.fmean[t * a.Dy + j], a.fvar[t * a.Dy + j], a.Y[b * a.Dy + j], dmu, dv, dp);
            if (a.d_mean) a.d_mean[t * a.Dy + j] = wt * dmu;
            if (a.d_var) a.d_var[t * a.Dy + j] = wt * dv;
            ds += (double)wt * (double)dp;
        }
    }
    for (int o = 32; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
    if (lane == 0) {
        a.part[b] = a.mode_vi ? se / (double)a.K : (double)mx + log(se) - log((double)(a.lse_global ? a.K_total : a.K));
        a.part[a.B + b] = ds;
    }
}
// out[0] = sum part[0..n), out[1] = sum part[n..2n), out[2] = scale * out[0] - sum of the global KL shares (the bound)
struct LikFinishArgs { const double* part; long long n; double scale; const double* klg[IWVI_MAX_LAYERS]; int kln[IWVI_MAX_LAYERS]; int n_glob; double* out; };
__global__ __launch_bounds__(256) void k_lik_finish(LikFinishArgs a) {
    __shared__ double red[256];
    double tot[2];
    for (int i = 0; i < 2; ++i) {
        const double* p = a.part + (size_t)i * a.n;
        double s = 0.0;
        for (long long k = threadIdx.x; k < a.n; k += 256) s += p[k];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        tot[i] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double kl = 0.0;
        for (int i = 0; i < a.n_glob; ++i) for (int q = 0; q < a.kln[i]; ++q) kl += a.klg[i][q];
        a.out[0] = tot[0]; a.out[1] = tot[1]; a.out[2] = a.scale * tot[0] - kl;
    }
}

// ------------------------------------------------------------------------------------------
// Elementwise callables.  MODE 0: variational_expectations; 1: predict_density (Fvar == NULL: logp); 2: predict_mean_and_var
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float inv_probit(float x) { return 0.5f * erfcf(-x * 0.70710678118654752f) * (1.f - 2.f * LIK_JIT) + LIK_JIT; }

// predict_mean_and_var of one element (MODE 2 of k_lik_elem, and the moments of k_lik_mix)
__device__ __forceinline__ void lik_mean_var(const Lik& L, float p0, float mu, float v, float& em, float& ev) {
    if (L.type == IWVI_LIK_BERNOULLI_PROBIT) {
        const float p = inv_probit(mu * rsqrtf(1.f + v));
        em = p; ev = p - p * p;
    } else if (L.type == IWVI_LIK_STUDENT_T) {
        // m = E[F] = mu (the nodes are symmetric); E[s^2 nu / (nu - 2) + F^2] - m^2 by the rule in its centred form: f_i^2 - mu^2 =
        // (a x_i)(2 mu + a x_i), and the node pair +-x_i adds 2 (a x_i)^2 -- mu^2 never enters, so nothing cancels
        const float a = sqrtf(2.f * fmaxf(v, 0.f)), c = p0 * p0 * L.p1 / (L.p1 - 2.f);
        float m2 = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
            m2 = fmaf(GH_W[j], 2.f * xa * xa, m2);
        }
        em = mu; ev = c + m2;
    } else {
        em = mu; ev = v + p0;
    }
}

// predict_density of one element (MODE 1 of k_lik_elem with a variance, and the densities of k_lik_mix)
__device__ __forceinline__ float lik_density(const Lik& L, float p0, float mu, float v, float y) {
    float d0, d1;
    if (L.type == IWVI_LIK_BERNOULLI_PROBIT) {
        const float x = mu * rsqrtf(1.f + v);
        return logf(y == 1.f ? inv_probit(x) : 0.5f * erfcf(x * 0.70710678118654752f) * (1.f - 2.f * LIK_JIT) + LIK_JIT);
    }
    if (L.type == IWVI_LIK_STUDENT_T) {
        // log sum_i exp(g(f_i) + log w_i): the largest term first, then the sum (g is evaluated twice; nothing is kept in scratch)
        const float a = sqrtf(2.f * fmaxf(v, 0.f));
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
            mx = fmaxf(mx, GH_LOGW[j] + fmaxf(lik_eval<false>(L, p0, mu + xa, y, d0, d1), lik_eval<false>(L, p0, mu - xa, y, d0, d1)));
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
            s += __expf(GH_LOGW[j] + lik_eval<false>(L, p0, mu + xa, y, d0, d1) - mx) + __expf(GH_LOGW[j] + lik_eval<false>(L, p0, mu - xa, y, d0, d1) - mx);
        }
        return mx + logf(s);
    }
    const float e = y - mu, s = v + p0;
    return -0.5f * logf(6.283185307179586f * s) - 0.5f * e * e / s;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_lik_elem(Lik L, const float* __restrict__ Fmu, const float* __restrict__ Fvar,
                                                  const float* __restrict__ Y, long long n, int Dy, long long row_div, long long row_mod,
                                                  float* __restrict__ out, float* __restrict__ out2) {
    const float p0 = L.p0_dev ? *L.p0_dev : L.p0;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const float mu = Fmu[idx];
        float d0, d1, d2;
        if (MODE == 2) {
            float em, ev;
            lik_mean_var(L, p0, mu, Fvar[idx], em, ev);
            out[idx] = em; out2[idx] = ev;
            continue;
        }
        const long long t = idx / Dy;
        const int d = (int)(idx - t * Dy);
        const float y = Y[((t / row_div) % row_mod) * Dy + d];
        if (MODE == 0) { out[idx] = lik_quad<false>(L, p0, mu, Fvar[idx], y, d0, d1, d2); continue; }
        if (!Fvar) { out[idx] = lik_eval<false>(L, p0, mu, y, d0, d1); continue; }
        out[idx] = lik_density(L, p0, mu, Fvar[idx], y);
    }
}

// ------------------------------------------------------------------------------------------
// iwvi_lik_predict_mixture for the Gaussian, the Bernoulli and the Student-t: the point loop of likelihood_common.h over the two functions above.
// ------------------------------------------------------------------------------------------
struct LikMixOps {
    static constexpr bool HAS_CONST = false;
    const Lik& L; float p0;
    __device__ __forceinline__ float density(float mu, float v, float y) const { return lik_density(L, p0, mu, v, y); }
    __device__ __forceinline__ float target_const(float) const { return 0.f; }
    __device__ __forceinline__ void mean_var(float mu, float v, float& em, float& ev) const { lik_mean_var(L, p0, mu, v, em, ev); }
};
template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_lik_mix(LikMixArgs g) {
    const LikMixOps ops{g.lik, g.lik.p0_dev ? *g.lik.p0_dev : g.lik.p0};
    mix_points<SEG>(g, ops);
}

// descriptor -> kernel argument; what: the entry point's name for the error text; need_df2: predict_mean_and_var of the Student-t
// IWVI_LIK_MULTICLASS: the moments have one column per class (Dy = param[1]) while Y has ONE column of labels
int mc_check_classes(const Lik& L, int Dy, const char* what) {
    if (Dy != (int)L.p1) { set_error("%s: MultiClass with %d classes needs Dy = %d, got %d", what, (int)L.p1, (int)L.p1, Dy); return IWVI_ERR_ARG; }
    return IWVI_OK;
}

int take_lik(const iwvi_lik_desc* d, Lik& L, const char* what, bool need_df2) {
    if (!d) { set_error("%s: null likelihood descriptor", what); return IWVI_ERR_ARG; }
    L.type = d->type; L.p0 = d->param[0]; L.p1 = d->param[1]; L.lgc = d->lgc; L.p0_dev = d->param0_dev;
    switch (d->type) {
        case IWVI_LIK_GAUSSIAN:
            if (!(d->param[0] > 0.f)) { set_error("%s: Gaussian variance must be positive", what); return IWVI_ERR_ARG; }
            return IWVI_OK;
        case IWVI_LIK_BERNOULLI_PROBIT:
            L.p0 = 1.f; L.p0_dev = nullptr;
            return IWVI_OK;
        case IWVI_LIK_STUDENT_T:
            if (!(d->param[0] > 0.f)) { set_error("%s: Student-t scale must be positive", what); return IWVI_ERR_ARG; }
            if (!(d->param[1] > 0.f)) { set_error("%s: Student-t df must be positive", what); return IWVI_ERR_ARG; }
            if (need_df2 && !(d->param[1] > 2.f)) { set_error("%s: the Student-t variance needs df > 2 (got %g)", what, (double)d->param[1]); return IWVI_ERR_ARG; }
            return IWVI_OK;
        case IWVI_LIK_MULTICLASS: {
            // (type 3 was refused as unknown before this extension: the text says so to a caller whose 3 means something else)
            const float eps = d->param[0], C = d->param[1];
            if (!(eps > 0.f && eps < 1.f)) {
                set_error("%s: MultiClass epsilon (param[0]) must lie in (0, 1), got %g -- a descriptor of an unknown likelihood type? "
                          "Type %d is MultiClass: param[0] = epsilon, param[1] = the number of classes", what, (double)eps, d->type);
                return IWVI_ERR_ARG;
            }
            if (!(C >= 2.f && C <= (float)IWVI_MAX_P) || C != (float)(int)C) {
                set_error("%s: MultiClass needs an integral number of classes (param[1]) in 2..%d, got %g", what, IWVI_MAX_P, (double)C);
                return IWVI_ERR_ARG;
            }
            L.p0_dev = nullptr;
            return IWVI_OK;
        }
        case IWVI_LIK_POISSON:
            if (!(d->param[0] > 0.f)) { set_error("%s: Poisson binsize (param[0]) must be positive, got %g", what, (double)d->param[0]); return IWVI_ERR_ARG; }
            L.p0_dev = nullptr;                              // binsize is a fixed host parameter
            return IWVI_OK;
        case IWVI_LIK_EXPONENTIAL:
            L.p0 = 1.f; L.p0_dev = nullptr;
            return IWVI_OK;
        case IWVI_LIK_GAMMA:
            if (!(d->param[0] > 0.f)) { set_error("%s: Gamma shape (param[0]) must be positive, got %g", what, (double)d->param[0]); return IWVI_ERR_ARG; }
            return IWVI_OK;
        case IWVI_LIK_BETA:
            if (!(d->param[0] > 0.f)) { set_error("%s: Beta scale (param[0]) must be positive, got %g", what, (double)d->param[0]); return IWVI_ERR_ARG; }
            return IWVI_OK;
        case IWVI_LIK_ORDINAL: {
            const float n = d->param[1];
            if (!(n >= 1.f && n <= (float)(IWVI_MAX_P - 1)) || n != (float)(int)n) {
                set_error("%s: Ordinal needs an integral number of bin edges (param[1]) in 1..%d, got %g", what, IWVI_MAX_P - 1, (double)n);
                return IWVI_ERR_ARG;
            }
            if (!d->param0_dev) {
                set_error("%s: Ordinal needs param0_dev: %d device floats [sigma, e_0 .. e_%d]", what, 1 + (int)n, (int)n - 1);
                return IWVI_ERR_ARG;
            }
            if (!(d->param[0] > 0.f)) { set_error("%s: Ordinal sigma (param[0]) must be positive, got %g", what, (double)d->param[0]); return IWVI_ERR_ARG; }
            return IWVI_OK;
        }
        case IWVI_LIK_HETERO_GAUSSIAN:                       // no parameter: param[], lgc and param0_dev are ignored
            L.p0 = 1.f; L.p1 = 0.f; L.p0_dev = nullptr;
            return IWVI_OK;
        default:                                             // (7 and 10 are unassigned: include/iwvi_hip.h)
            set_error("%s: unknown likelihood type %d", what, d->type); return IWVI_ERR_ARG;
    }
}

}  // namespace iwvi

using namespace iwvi;

extern "C" int iwvi_lik_elbo_reduce(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y,
                                    int64_t B, int K, int Dy, int64_t stride_b, int64_t stride_k,
                                    const float* const* kl_local, const int32_t* kl_dims, int n_kl,
                                    const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                                    double scale, int K_total, int mode_vi,
                                    float* out_ms, float* out_logp, double* out_elbo, uint64_t* ticket, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LikReduceArgs g{};
    int rc;
    if ((rc = take_lik(lik, g.lik, "iwvi_lik_elbo_reduce")) != IWVI_OK) return rc;
    if (g.lik.type == IWVI_LIK_HETERO_GAUSSIAN && (rc = hg_check_dim(Dy, "iwvi_lik_elbo_reduce")) != IWVI_OK) return rc;
    if (!fmean || !fvar || !Y) { set_error("iwvi_lik_elbo_reduce: null input"); return IWVI_ERR_ARG; }
    if (B <= 0) { set_error("iwvi_lik_elbo_reduce: empty minibatch"); return IWVI_ERR_ARG; }
    if (K <= 0 || Dy <= 0) { set_error("iwvi_lik_elbo_reduce: bad K=%d or Dy=%d", K, Dy); return IWVI_ERR_ARG; }
    if (n_kl < 0 || n_kl > IWVI_MAX_KL) { set_error("iwvi_lik_elbo_reduce: %d local regularisers (max %d)", n_kl, IWVI_MAX_KL); return IWVI_ERR_ARG; }
    if (!out_ms && !out_logp && !out_elbo) { set_error("iwvi_lik_elbo_reduce: no output asked for"); return IWVI_ERR_ARG; }
    if (out_elbo && (!out_logp || !ticket)) { set_error("iwvi_lik_elbo_reduce: out_elbo needs out_logp (scratch) and a zero-initialised ticket word"); return IWVI_ERR_ARG; }
    g.fmean = fmean; g.fvar = fvar; g.Y = Y; g.n_kl = n_kl;
    for (int i = 0; i < n_kl; ++i) {
        if (!kl_local || !kl_local[i] || !kl_dims || kl_dims[i] <= 0) { set_error("iwvi_lik_elbo_reduce: bad local regulariser %d", i); return IWVI_ERR_ARG; }
        g.kl[i] = kl_local[i]; g.kl_dims[i] = kl_dims[i];
    }
    g.stride_b = stride_b; g.stride_k = stride_k;
    g.B = B; g.K = K; g.Dy = Dy; g.K_total = K_total > 0 ? K_total : K; g.mode_vi = mode_vi;
    g.ms = out_ms; g.logp = out_logp; g.elbo = out_elbo; g.ticket = (unsigned long long*)ticket; g.scale = scale;
    if (out_elbo) {
        if (n_glob < 0 || n_glob > LIK_MAX_GLOB) { set_error("iwvi_lik_elbo_reduce: too many global KL terms (%d > %d)", n_glob, LIK_MAX_GLOB); return IWVI_ERR_ARG; }
        for (int i = 0; i < n_glob; ++i) {
            if (!kl_global || !kl_global[i]) { set_error("iwvi_lik_elbo_reduce: null global KL pointer %d", i); return IWVI_ERR_ARG; }
            g.klg[i] = kl_global[i];
            g.klg_n[i] = kl_global_counts ? kl_global_counts[i] : 1;
            if (g.klg_n[i] <= 0 || g.klg_n[i] > IWVI_MAX_R) { set_error("iwvi_lik_elbo_reduce: bad global KL count %d", g.klg_n[i]); return IWVI_ERR_ARG; }
        }
        g.n_glob = n_glob;
    }
    if (g.lik.type == IWVI_LIK_MULTICLASS) {
        if ((rc = mc_check_classes(g.lik, Dy, "iwvi_lik_elbo_reduce")) != IWVI_OK) return rc;
        return mc_launch_elbo(g, stream);
    }
    if (g.lik.type == IWVI_LIK_HETERO_GAUSSIAN) return hg_launch_elbo(g, stream);
    if (xl_type(g.lik.type)) return xl_launch_elbo(g, stream);
    if (bo_type(g.lik.type)) return bo_launch_elbo(g, stream);
    return seg_dispatch(K, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_lik_elbo<SEG>, dim3((unsigned)lik_passes(B, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_lik_elbo");
    });
}

extern "C" int iwvi_lik_elbo_backward(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y, int Dy,
                                      const float* const* kl_local, const int32_t* kl_dims, int n_local,
                                      int64_t B, int K, double scale, int mode_vi,
                                      float* out_w, float* d_mean, float* d_var,
                                      const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                                      const float* lse_global, int K_total, double* out_sums, double* ws, void* stream_) {
    LikBwdArgs a{};
    int rc;
    if ((rc = take_lik(lik, a.lik, "iwvi_lik_elbo_backward")) != IWVI_OK) return rc;
    if (a.lik.type == IWVI_LIK_HETERO_GAUSSIAN && (rc = hg_check_dim(Dy, "iwvi_lik_elbo_backward")) != IWVI_OK) return rc;
    if (!fmean || !fvar || !Y || !out_sums || !ws || Dy <= 0 || B <= 0 || K <= 0 || n_local < 0 || n_local > IWVI_MAX_KL ||
        n_glob < 0 || n_glob > IWVI_MAX_LAYERS) {
        set_error("iwvi_lik_elbo_backward: bad argument"); return IWVI_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream_;
    a.fmean = fmean; a.fvar = fvar; a.Y = Y; a.Dy = Dy; a.n_kl = n_local;
    for (int i = 0; i < n_local; ++i) {
        if (!kl_local || !kl_local[i] || !kl_dims || kl_dims[i] <= 0) { set_error("iwvi_lik_elbo_backward: bad local regulariser %d", i); return IWVI_ERR_ARG; }
        a.kl[i] = kl_local[i]; a.kl_dims[i] = kl_dims[i];
    }
    if (lse_global && (mode_vi || K_total < K)) { set_error("iwvi_lik_elbo_backward: lse_global needs the IW bound and K_total >= K"); return IWVI_ERR_ARG; }
    LikFinishArgs fa{};
    fa.part = ws; fa.n = B; fa.scale = scale; fa.n_glob = n_glob; fa.out = out_sums;
    for (int i = 0; i < n_glob; ++i) {
        if (!kl_global || !kl_global[i] || !kl_global_counts || kl_global_counts[i] <= 0) { set_error("iwvi_lik_elbo_backward: bad global KL %d", i); return IWVI_ERR_ARG; }
        fa.klg[i] = kl_global[i]; fa.kln[i] = kl_global_counts[i];
    }
    a.B = B; a.K = K; a.scale = scale; a.mode_vi = mode_vi; a.lse_global = lse_global; a.K_total = K_total;
    a.w = out_w; a.d_mean = d_mean; a.d_var = d_var; a.part = ws;
    if (a.lik.type == IWVI_LIK_MULTICLASS) {
        if ((rc = mc_check_classes(a.lik, Dy, "iwvi_lik_elbo_backward")) != IWVI_OK) return rc;
        if ((rc = mc_launch_elbo_bwd(a, st)) != IWVI_OK) return rc;
    } else if (a.lik.type == IWVI_LIK_HETERO_GAUSSIAN) {
        if ((rc = hg_launch_elbo_bwd(a, st)) != IWVI_OK) return rc;
    } else if (xl_type(a.lik.type)) {
        if ((rc = xl_launch_elbo_bwd(a, st)) != IWVI_OK) return rc;
    } else if (bo_type(a.lik.type)) {
        if ((rc = bo_launch_elbo_bwd(a, st)) != IWVI_OK) return rc;
    } else {
        hipLaunchKernelGGL(k_lik_elbo_bwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_lik_finish, dim3(1), dim3(256), 0, st, fa);
    return check_launch("k_lik_elbo_bwd");
}

template <int MODE>
static int lik_elementwise(const char* what, const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, const float* Y, int64_t T, int Dy,
                           int64_t row_div, int64_t row_mod, float* out, float* out2, void* stream_) {
    Lik L{};
    int rc;
    if ((rc = take_lik(lik, L, what, MODE == 2)) != IWVI_OK) return rc;
    if (L.type == IWVI_LIK_HETERO_GAUSSIAN && (rc = hg_check_dim(Dy, what)) != IWVI_OK) return rc;
    if (T < 0 || Dy <= 0 || row_div <= 0 || row_mod <= 0) { set_error("%s: bad size", what); return IWVI_ERR_ARG; }
    if (L.type == IWVI_LIK_MULTICLASS && (rc = mc_check_classes(L, Dy, what)) != IWVI_OK) return rc;
    if (T == 0) return IWVI_OK;
    if (!Fmu || !out || (MODE != 1 && !Fvar) || (MODE != 2 && !Y) || (MODE == 2 && !out2)) { set_error("%s: null pointer", what); return IWVI_ERR_ARG; }
    if (L.type == IWVI_LIK_MULTICLASS)
        return mc_launch_elem(what, MODE, L, Fmu, Fvar, Y, (long long)T, Dy, (long long)row_div, (long long)row_mod, out, out2, (hipStream_t)stream_);
    if (L.type == IWVI_LIK_HETERO_GAUSSIAN)
        return hg_launch_elem(what, MODE, Fmu, Fvar, Y, (long long)T, Dy, (long long)row_div, (long long)row_mod, out, out2, (hipStream_t)stream_);
    if (xl_type(L.type))
        return xl_launch_elem(what, MODE, L, Fmu, Fvar, Y, (long long)T, Dy, (long long)row_div, (long long)row_mod, out, out2, (hipStream_t)stream_);
    if (bo_type(L.type))
        return bo_launch_elem(what, MODE, L, Fmu, Fvar, Y, (long long)T, Dy, (long long)row_div, (long long)row_mod, out, out2, (hipStream_t)stream_);
    const long long n = (long long)T * Dy;
    hipLaunchKernelGGL(k_lik_elem<MODE>, dim3(elem_blocks(n)), dim3(256), 0, (hipStream_t)stream_, L, Fmu, Fvar, Y, n, Dy,
                       (long long)row_div, (long long)row_mod, out, out2);
    return check_launch(what);
}

extern "C" int iwvi_lik_var_exp(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, const float* Y,
                                int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream_) {
    return lik_elementwise<0>("iwvi_lik_var_exp", lik, Fmu, Fvar, Y, T, Dy, row_div, row_mod, out, nullptr, stream_);
}

extern "C" int iwvi_lik_predict_density(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, const float* Y,
                                        int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream_) {
    return lik_elementwise<1>("iwvi_lik_predict_density", lik, Fmu, Fvar, Y, T, Dy, row_div, row_mod, out, nullptr, stream_);
}

extern "C" int iwvi_lik_predict_mean_and_var(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, int64_t n,
                                             float* out_mean, float* out_var, void* stream_) {
    if (lik && lik->type == IWVI_LIK_MULTICLASS) {             // n = T C elements: rows of C = param[1] classes
        Lik L{};
        int rc;
        if ((rc = take_lik(lik, L, "iwvi_lik_predict_mean_and_var")) != IWVI_OK) return rc;
        const int C = (int)L.p1;
        if (n < 0 || n % C != 0) { set_error("iwvi_lik_predict_mean_and_var: MultiClass takes n = T x %d elements, got %lld", C, (long long)n); return IWVI_ERR_ARG; }
        return lik_elementwise<2>("iwvi_lik_predict_mean_and_var", lik, Fmu, Fvar, nullptr, n / C, C, 1, 1, out_mean, out_var, stream_);
    }
    if (lik && lik->type == IWVI_LIK_HETERO_GAUSSIAN) {       // n = T Dy elements of moments: rows of Dy = param[1] columns, outputs [T, Dy / 2]
        const char* what = "iwvi_lik_predict_mean_and_var";
        const float w = lik->param[1];
        int rc;
        if (!(w >= 2.f && w <= (float)IWVI_MAX_P) || w != (float)(int)w) {
            set_error("%s: the heteroskedastic Gaussian takes the row width Dy (even, 2..%d) in param[1] here -- this entry has no Dy argument --, got %g",
                      what, IWVI_MAX_P, (double)w);
            return IWVI_ERR_ARG;
        }
        const int Dy = (int)w;
        if ((rc = hg_check_dim(Dy, what)) != IWVI_OK) return rc;
        if (n < 0 || n % Dy != 0) { set_error("%s: the heteroskedastic Gaussian takes n = T x %d elements, got %lld", what, Dy, (long long)n); return IWVI_ERR_ARG; }
        return lik_elementwise<2>(what, lik, Fmu, Fvar, nullptr, n / Dy, Dy, 1, 1, out_mean, out_var, stream_);
    }
    return lik_elementwise<2>("iwvi_lik_predict_mean_and_var", lik, Fmu, Fvar, nullptr, n, 1, 1, 1, out_mean, out_var, stream_);
}

extern "C" int iwvi_lik_predict_mixture(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y,
                                        int64_t N, int S, int Dy, int64_t stride_n, int64_t stride_s,
                                        float* out_logp, float* out_mean, float* out_var, void* stream_) {
    const char* what = "iwvi_lik_predict_mixture";
    hipStream_t stream = (hipStream_t)stream_;
    LikMixArgs g{};
    int rc;
    if ((rc = take_lik(lik, g.lik, what, out_mean != nullptr)) != IWVI_OK) return rc;
    if (N < 0) { set_error("%s: N = %lld", what, (long long)N); return IWVI_ERR_ARG; }
    if (S < 1) { set_error("%s: S = %d draws (at least 1)", what, S); return IWVI_ERR_ARG; }
    if (g.lik.type == IWVI_LIK_HETERO_GAUSSIAN && (rc = hg_check_dim(Dy, what)) != IWVI_OK) return rc;
    if (Dy < 1 || Dy > IWVI_MAX_P) { set_error("%s: Dy = %d outside 1..%d", what, Dy, IWVI_MAX_P); return IWVI_ERR_ARG; }
    if (g.lik.type == IWVI_LIK_MULTICLASS && (rc = mc_check_classes(g.lik, Dy, what)) != IWVI_OK) return rc;
    if (stride_n < 0 || stride_s < 0) { set_error("%s: negative stride", what); return IWVI_ERR_ARG; }
    if (!out_logp && !out_mean && !out_var) { set_error("%s: no output asked for", what); return IWVI_ERR_ARG; }
    if ((out_mean == nullptr) != (out_var == nullptr)) { set_error("%s: out_mean and out_var go together", what); return IWVI_ERR_ARG; }
    if ((out_logp == nullptr) != (Y == nullptr)) { set_error("%s: out_logp needs Y, and Y is read for out_logp alone: both or neither", what); return IWVI_ERR_ARG; }
    if (N == 0) return IWVI_OK;
    if (!fmean || !fvar) { set_error("%s: null moments", what); return IWVI_ERR_ARG; }
    g.fmean = fmean; g.fvar = fvar; g.Y = Y;
    g.N = N; g.S = S; g.Dy = Dy; g.stride_n = stride_n; g.stride_s = stride_s;
    g.logp = out_logp; g.mean = out_mean; g.var = out_var;
    if (g.lik.type == IWVI_LIK_MULTICLASS) return mc_launch_mix(g, stream);
    if (g.lik.type == IWVI_LIK_HETERO_GAUSSIAN) return hg_launch_mix(g, stream);
    if (xl_type(g.lik.type)) return xl_launch_mix(g, stream);
    if (bo_type(g.lik.type)) return bo_launch_mix(g, stream);
    return seg_dispatch(S, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_lik_mix<SEG>, dim3(mix_blocks(N, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_lik_mix");
    });
}
