// GPflow 1.x Poisson(binsize), Exponential() and Gamma(shape) with their default exp link, lambda = exp(F) (include/iwvi_hip.h:
// IWVI_LIK_POISSON / _EXPONENTIAL / _GAMMA), behind the iwvi_lik_* entry points of csrc/likelihood_tail.hip.  All three log-densities have
// ONE shape,
//   logp(f, y) = cm f - ce exp(sg f) + c0(y)
//                  cm      ce      sg    c0(y)
//     Poisson      y       beta    +1    y log beta - lgamma(y + 1)               beta = binsize = param[0] (fixed, host)
//     Exponential  -1      y       -1    0
//     Gamma        -a      y       -1    (a - 1) log y - lgamma(a)                a = shape = param[0] / *param0_dev (trained)
// so the variational expectation under N(f; mu, v) is a closed form -- GPflow's own branch for the exp link --
//   E = cm mu - ce exp(sg mu + v / 2) + c0(y),      dE/dmu = cm - sg ce e,   dE/dv = -ce e / 2,   dE/da = -mu - psi(a) + log y   (Gamma)
// with e = exp(sg mu + v / 2): one exp per (point, sample, output) against the 40 erfc / log of the quadrature tail, no division by
// sqrt(v) and hence no variance floor.  c0 depends on the target alone: it is formed once per (point, output), summed per point and added
// OUTSIDE the log-sum-exp over the samples (the running maximum carries it, so ms[:, 0] + log ms[:, 1] - log K is still log p).
// predict_density and predict_mean_and_var are GPflow's base-class defaults: the 20-point rule of likelihood_common.h over logp (in log
// space, the largest term first) and over the conditional mean / variance (beta l, beta l | l, l^2 | a l, a l^2 with l = exp(f)).
// lgamma(a) and psi(a) are evaluated here, in float64, from the value the launch reads -- the shape may be a device scalar that an
// optimiser moves between two replays of a captured graph --; they are wave-uniform, so every wave evaluates them once.
// NO CLAMP: where exp overflows float32 (|sg mu + v / 2| above about 88) the formulas give +-inf or NaN, as GPflow's do in float64 at 709.
#include "likelihood_common.h"

namespace iwvi {

// the launch's view of the descriptor (wave-uniform)
struct XlPar {
    int type;
    float sg;                  // the exponential's argument is sg f (+ v / 2)
    float beta, logbeta;       // Poisson
    float cmu;                 // what multiplies f where the target does not: -1 (Exponential), -a (Gamma)
    float am1, lga;            // Gamma: a - 1, lgamma(a)
    double psi;                // Gamma, PSI only: psi(a)
};
template <bool LGA, bool PSI>
__device__ __forceinline__ XlPar xl_par(const Lik& L) {
    XlPar P{};
    P.type = L.type;
    P.sg = L.type == IWVI_LIK_POISSON ? 1.f : -1.f;
    P.beta = L.p0; P.cmu = -1.f;
    if (L.type == IWVI_LIK_POISSON) P.logbeta = logf(L.p0);
    if (L.type == IWVI_LIK_GAMMA) {
        const float a = L.p0_dev ? *L.p0_dev : L.p0;
        P.cmu = -a; P.am1 = a - 1.f;
        if (LGA) P.lga = (float)lgamma((double)a);
        if (PSI) P.psi = digamma_f64((double)a);
    }
    return P;
}

// cm f - ce exp(sg f + hv): logp without c0 at hv = 0, the closed-form expectation without c0 at hv = v / 2; e: the exponential
__device__ __forceinline__ float xl_g(const XlPar& P, float y, float f, float hv, float& e) {
    const bool pois = P.type == IWVI_LIK_POISSON;
    e = expf(fmaf(P.sg, f, hv));
    return fmaf(pois ? y : P.cmu, f, -(pois ? P.beta : y) * e);
}
// c0(y); logy: log y where c0 needs it (Gamma), else 0
__device__ __forceinline__ float xl_c0(const XlPar& P, float y, float& logy) {
    logy = 0.f;
    if (P.type == IWVI_LIK_POISSON) return fmaf(y, P.logbeta, -lgammaf(y + 1.f));
    if (P.type == IWVI_LIK_GAMMA) { logy = logf(y); return fmaf(P.am1, logy, -P.lga); }
    return 0.f;
}

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint: the cores of likelihood_common.h over the closed forms.  A point's state is its
// constant cb = sum_d c0(y_bd), formed once by the lanes that own the point (over its outputs, float32) and added outside the log-sum-exp;
// for the heads also sum_d (log y_d - psi(a)), the point's part of d / d shape.  With lse_global the core takes the constant off the job's
// normaliser (the local L_nk do not carry it) and adds it back in part[b].
// part[B..2B): the share of d / d shape (Gamma), sum_k w_k sum_d (-mu_kd - psi(a) + log y_d); 0 for the other two.
// ------------------------------------------------------------------------------------------
struct XlOps {
    static constexpr bool HAS_CONST = true;
    struct Point { float cb; double dpar0; };
    const XlPar& P; int Dy;
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float* Y, long long b, bool live, int sl) const {
        float cb = 0.f, lyb = 0.f;
        if (live && P.type != IWVI_LIK_EXPONENTIAL)
            for (int d = sl; d < Dy; d += SEG) { float ly; cb += xl_c0(P, Y[b * Dy + d], ly); lyb += ly; }
        cb = lseg_sum<SEG>(cb);
        if (!GRAD) return {cb, 0.0};
        lyb = lseg_sum<SEG>(lyb);
        return {cb, (double)lyb - (double)Dy * P.psi};          // sum_d (log y_d - psi(a))
    }
    __device__ __forceinline__ float point_const(const Point& pt) const { return pt.cb; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float* var, const float* Y, long long b) const {
        float acc = 0.f, e;
        for (int d = 0; d < Dy; ++d) acc += xl_g(P, Y[b * Dy + d], mu[d], 0.5f * var[d], e);
        return acc;
    }
    __device__ __forceinline__ double heads(const Point& pt, const float* mu, const float* var, const float* Y, long long b, float wt,
                                            float* dm, float* dv, double ds) const {
        const bool pois = P.type == IWVI_LIK_POISSON;
        double smu = 0.0;
        for (int j = 0; j < Dy; ++j) {
            const float y = Y[b * Dy + j];
            float e;
            xl_g(P, y, mu[j], 0.5f * var[j], e);
            const float ce = (pois ? P.beta : y) * e;
            if (dm) dm[j] = wt * fmaf(-P.sg, ce, pois ? y : P.cmu);
            if (dv) dv[j] = wt * (-0.5f * ce);
            smu += (double)mu[j];
        }
        return P.type == IWVI_LIK_GAMMA ? ds + (double)wt * (pt.dpar0 - smu) : ds;
    }
};

// A workgroup takes as many passes as the grid leaves it: the launcher spreads the points over up to XL_MAX_BLOCKS workgroups, ONE pass each
// at B = 1024.  (k_elbo's 64 points per workgroup -- csrc/lv_elbo.hip -- were tried first, a sample being a handful
// of FMAs and one exp: 16 workgroups at configs[2], and an evaluation took 74.5-79.0 us against the Student-t's 68.3 in the same session.  The
// per-sample work is small, but a pass is a chain of dependent loads and cross-lane reductions, and eight of them in a row on 16 of 256 CUs
// is what the time went into -- the finding of DESIGN.md section 6 for k_lik_elbo, again.)
constexpr int XL_MAX_BLOCKS = 1024;     // four workgroups per CU

template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_xl_elbo(LikReduceArgs g) {
    const XlPar P = xl_par<true, false>(g.lik);
    const XlOps ops{P, g.Dy};
    elbo_points<SEG, true>(g, ops);
}

__global__ __launch_bounds__(256) void k_xl_elbo_bwd(LikBwdArgs a) {
    const XlPar P = xl_par<true, true>(a.lik);
    const XlOps ops{P, a.Dy};
    elbo_bwd_point(a, ops);
}

// ------------------------------------------------------------------------------------------
// Elementwise callables.  MODE 0: variational_expectations (the closed form); 1: predict_density (Fvar == NULL: logp); 2: predict_mean_and_var.
// Modes 1 and 2 are the 20-point rule, f_i = mu +- a x_j with a = sqrt(2 v): the rule defines the result, not exp(mu + v / 2).
// ------------------------------------------------------------------------------------------
// predict_mean_and_var of one element (MODE 2 of k_xl_elem; k_xl_mix)
__device__ __forceinline__ void xl_mean_var(const XlPar& P, float mu, float v, float& ey, float& ev) {
    // M1 = sum_i w_i exp(f_i), M2 = sum_i w_i exp(2 f_i);  E_y = sum w mean(f_i), E_y2 = sum w (var(f_i) + mean(f_i)^2), var = E_y2 - E_y^2
    const float a = sqrtf(2.f * fmaxf(v, 0.f));
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        const float ea = expf(mu + xa), eb = expf(mu - xa);
        m1 = fmaf(GH_W[j], ea + eb, m1);
        m2 = fmaf(GH_W[j], fmaf(ea, ea, eb * eb), m2);
    }
    float ey2;
    if (P.type == IWVI_LIK_POISSON) { ey = P.beta * m1; ey2 = fmaf(P.beta * P.beta, m2, ey); }
    else if (P.type == IWVI_LIK_EXPONENTIAL) { ey = m1; ey2 = 2.f * m2; }
    else { const float sh = -P.cmu; ey = sh * m1; ey2 = fmaf(sh, sh, sh) * m2; }
    ev = fmaf(-ey, ey, ey2);
}

// predict_density of one element WITHOUT c0(y) (MODE 1 of k_xl_elem with a variance, which adds c0; k_xl_mix, which adds a point's c0 once):
// log sum_i exp(g(f_i) + log w_i), the largest term first, then the sum (g is evaluated twice; nothing is kept in scratch)
__device__ __forceinline__ float xl_density(const XlPar& P, float mu, float v, float y) {
    float e;
    const float a = sqrtf(2.f * fmaxf(v, 0.f));
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        mx = fmaxf(mx, GH_LOGW[j] + fmaxf(xl_g(P, y, mu + xa, 0.f, e), xl_g(P, y, mu - xa, 0.f, e)));
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        s += expf(GH_LOGW[j] + xl_g(P, y, mu + xa, 0.f, e) - mx) + expf(GH_LOGW[j] + xl_g(P, y, mu - xa, 0.f, e) - mx);
    }
    return mx + logf(s);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_xl_elem(Lik L, const float* __restrict__ Fmu, const float* __restrict__ Fvar,
                                                 const float* __restrict__ Y, long long n, int Dy, long long row_div, long long row_mod,
                                                 float* __restrict__ out, float* __restrict__ out2) {
    const XlPar P = xl_par<MODE != 2, false>(L);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const float mu = Fmu[idx];
        float e;
        if (MODE == 2) {
            float ey, ev;
            xl_mean_var(P, mu, Fvar[idx], ey, ev);
            out[idx] = ey; out2[idx] = ev;
            continue;
        }
        const long long t = idx / Dy;
        const int d = (int)(idx - t * Dy);
        const float y = Y[((t / row_div) % row_mod) * Dy + d];
        float logy;
        const float c0 = xl_c0(P, y, logy);
        if (MODE == 0) { out[idx] = xl_g(P, y, mu, 0.5f * Fvar[idx], e) + c0; continue; }
        if (!Fvar) { out[idx] = xl_g(P, y, mu, 0.f, e) + c0; continue; }
        out[idx] = xl_density(P, mu, Fvar[idx], y) + c0;
    }
}

// ------------------------------------------------------------------------------------------
// iwvi_lik_predict_mixture for the three exp-link types: the point loop of likelihood_common.h over the two functions above; a point's
// sum_d c0(y_d) is formed once and added outside the log-sum-exp over its draws, as k_xl_elbo does.
// ------------------------------------------------------------------------------------------
struct XlMixOps {
    static constexpr bool HAS_CONST = true;
    const XlPar& P;
    __device__ __forceinline__ float density(float mu, float v, float y) const { return xl_density(P, mu, v, y); }
    __device__ __forceinline__ float target_const(float y) const { float ly; return xl_c0(P, y, ly); }
    __device__ __forceinline__ void mean_var(float mu, float v, float& ey, float& ev) const { xl_mean_var(P, mu, v, ey, ev); }
};
template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_xl_mix(LikMixArgs g) {
    const XlPar P = xl_par<true, false>(g.lik);
    const XlMixOps ops{P};
    mix_points<SEG>(g, ops);
}

int xl_launch_elbo(const LikReduceArgs& g, hipStream_t stream) {
    return seg_dispatch(g.K, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        const long long passes = lik_passes(g.B, SEG);
        hipLaunchKernelGGL(k_xl_elbo<SEG>, dim3((unsigned)(passes < XL_MAX_BLOCKS ? passes : XL_MAX_BLOCKS)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_xl_elbo");
    });
}

int xl_launch_mix(const LikMixArgs& g, hipStream_t stream) {
    return seg_dispatch(g.S, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_xl_mix<SEG>, dim3(mix_blocks(g.N, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_xl_mix");
    });
}

int xl_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_xl_elbo_bwd, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
    return check_launch("k_xl_elbo_bwd");
}

int xl_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream) {
    const long long n = T * Dy;
    return launch_elem_mode(what, mode, n, [&](auto m, int blocks) {
        hipLaunchKernelGGL(k_xl_elem<decltype(m)::value>, dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, Dy, row_div, row_mod, out, out2);
    });
}

}  // namespace iwvi
