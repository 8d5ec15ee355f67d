// GPflow 1.x Beta(invlink=inv_probit, scale) and Ordinal(bin_edges) (include/iwvi_hip.h: IWVI_LIK_BETA / IWVI_LIK_ORDINAL), behind the
// iwvi_lik_* entry points of csrc/likelihood_tail.hip.  Both squash the latent through the probit link with GPflow's jitter,
//   ip(x) = Phi(x) (1 - 2 jit) + jit,   jit = LIK_JIT,
// and neither has a closed-form expectation: variational_expectations, predict_density (in log space, the largest term first) and
// predict_mean_and_var are GPflow's base-class defaults by the 20-point rule of likelihood_common.h; the heads are the reparameterised
// first-derivative form of csrc/likelihood_tail.hip (lik_quad), the variance floored at LIK_V_FLOOR.
//   Beta      m = ip(f), alpha = m s, beta = s - alpha = (1 - m) s, yc = clip(y, 1e-6, 1 - 1e-6)
//             logp = (alpha - 1) log yc + (beta - 1) log(1 - yc) + lgamma(s) - lgamma(alpha) - lgamma(beta)
//             s = scale = param[0] / *param0_dev (trained): lgamma(s) and psi(s) are evaluated here, in float64, once per wave from the
//             value the launch reads (as the Gamma's shape is, csrc/likelihood_explink.hip); they are constants of the rule and are added
//             behind it.  psi(alpha) and psi(beta) are per node, float32 (bo_digammaf).
//   Ordinal   P_y(f) = ip((e_y - f) / sigma) - ip((e_(y-1) - f) / sigma),  e_(-1) = -inf, e_n = +inf;  logp = log(P_y + 1e-6)
//             *param0_dev = [sigma, e_0 .. e_(n-1)] (sigma trained, the edges fixed), n = param[1].  The jitter cancels in the difference,
//             P = (1 - 2 jit) (Phi(a) - Phi(b)), and the difference is never formed from two values near 1 or near 0 (bo_phi_diff).
// The node evaluation is templated on the type (BoFam<TYPE>): no runtime branch on it anywhere below the launchers.
// The node loops are NOT unrolled (#pragma unroll 1): a Beta node is two erfc, two lgamma and, for the heads, two digamma and an exp --
// forty copies of that per element would be instruction-cache misses, not speed; the node tables are read with a uniform index.
#include "likelihood_common.h"

namespace iwvi {

constexpr float BO_C = 1.f - 2.f * LIK_JIT;          // what the jitter leaves of Phi
constexpr float BO_RSQRT2 = 0.70710678118654752f;
constexpr float BO_RSQRT2PI = 0.3989422804014327f;
constexpr float BO_Y_EPS = 1e-6f;                    // the Beta's clip of its targets, the Ordinal's floor inside the log
constexpr float BO_LOG_EPS = -13.815510557964274f;   // log(1e-6)
constexpr float BO_LOG1M_EPS = -1.0000005000003334e-6f;   // log(1 - 1e-6)

// psi(x), x > 0, float32: psi(x) = psi(x + 6) - sum_{k < 6} 1 / (x + k), then the asymptotic series at X = x + 6 >= 6 (next term
// 1 / (240 X^8) < 2.5e-9).  No branch and no loop over the data: every lane takes the six steps.  The largest reciprocal comes first.
__device__ __forceinline__ float bo_digammaf(float x) {
    float r = __builtin_amdgcn_rcpf(x);
#pragma unroll
    for (int k = 1; k < 6; ++k) r += __builtin_amdgcn_rcpf(x + (float)k);
    const float X = x + 6.f, i = __builtin_amdgcn_rcpf(X), i2 = i * i;
    return logf(X) - 0.5f * i - i2 * (1.f / 12.f - i2 * (1.f / 120.f - i2 * (1.f / 252.f))) - r;
}

// Phi(a sqrt 2) - Phi(b sqrt 2) for a >= b (the arguments already divided by sqrt 2; a = +inf, b = -inf allowed), at float32 RELATIVE
// accuracy: on one side of 0 both terms come from erfc there -- two small numbers, not two numbers near 1 --, across 0 from erf, where
// both terms are positive.
__device__ __forceinline__ float bo_phi_diff(float a, float b) {
    if (b >= 0.f) return 0.5f * (erfcf(b) - erfcf(a));
    if (a <= 0.f) return 0.5f * (erfcf(-a) - erfcf(-b));
    return 0.5f * (erff(a) + erff(-b));
}

// ---- the two families: Par (the launch's view of the descriptor, wave-uniform), Tgt (what a target contributes, formed once per
// (sample, output) outside the node loop), eval<GRAD> (g(f) = logp without the constants of the rule; GRAD: g'(f), d g / d param[0]),
// E0 / DP0 (those constants: added once behind the rule), cond_moments (sum_i w_i mean(f_i), sum_i w_i (var(f_i) + mean(f_i)^2)) ----
template <int TYPE> struct BoFam;

template <> struct BoFam<IWVI_LIK_BETA> {
    struct Par { float s, lgs, psis, rs1; };          // scale, lgamma(s), psi(s), 1 / (s + 1)
    struct Tgt { float ly, l1y; };                    // log yc, log(1 - yc)
    template <bool LGS, bool PSI>
    static __device__ __forceinline__ Par par(const Lik& L) {
        Par P{};
        P.s = L.p0_dev ? *L.p0_dev : L.p0;
        if (LGS) P.lgs = (float)lgamma((double)P.s);
        if (PSI) P.psis = (float)digamma_f64((double)P.s);
        P.rs1 = 1.f / (P.s + 1.f);
        return P;
    }
    // the clip decides in the target's own precision what the float64 clip of that float32 value decides: 0.999999f is the float just
    // below 1 - 1e-6, and 1 - y is exact in float32 for y in [1/2, 1]
    static __device__ __forceinline__ Tgt tgt(const Par&, float y) {
        if (y <= BO_Y_EPS) return {BO_LOG_EPS, BO_LOG1M_EPS};
        if (y > 0.999999f) return {BO_LOG1M_EPS, BO_LOG_EPS};
        return {logf(y), log1pf(-y)};
    }
    static __device__ __forceinline__ float E0(const Par& P) { return P.lgs; }
    static __device__ __forceinline__ float DP0(const Par& P) { return P.psis; }
    template <bool GRAD>
    static __device__ __forceinline__ float eval(const Par& P, const Tgt& T, float f, float& gp, float& gpar) {
        // m and 1 - m from erfc on their own sides (neither tail cancels, as the Bernoulli's p and q): m + q = 1 up to rounding
        const float u = f * BO_RSQRT2;
        const float m = 0.5f * erfcf(-u) * BO_C + LIK_JIT;
        const float q = 0.5f * erfcf(u) * BO_C + LIK_JIT;
        const float al = P.s * m, be = P.s * q;
        if (GRAD) {
            const float psa = bo_digammaf(al), psb = bo_digammaf(be);
            const float dm = BO_C * BO_RSQRT2PI * __expf(-0.5f * f * f);
            gp = P.s * dm * ((T.ly - T.l1y) - (psa - psb));
            gpar = fmaf(m, T.ly - psa, q * (T.l1y - psb));
        }
        return fmaf(al - 1.f, T.ly, (be - 1.f) * T.l1y) - lgammaf(al) - lgammaf(be);
    }
    static __device__ __forceinline__ void cond_moments(const Par& P, float mu, float a, float& ey, float& ey2) {
        // mean = m, var + mean^2 = m q / (s + 1) + m^2
        float s1 = 0.f, s2 = 0.f;
#pragma unroll 1
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float u = (h ? mu - xa : mu + xa) * BO_RSQRT2;
                const float m = 0.5f * erfcf(-u) * BO_C + LIK_JIT, q = 0.5f * erfcf(u) * BO_C + LIK_JIT;
                s1 = fmaf(GH_W[j], m, s1);
                s2 = fmaf(GH_W[j], fmaf(m * q, P.rs1, m * m), s2);
            }
        }
        ey = s1; ey2 = s2;
    }
};

template <> struct BoFam<IWVI_LIK_ORDINAL> {
    struct Par { float k, rsig; const float* edges; int n; };   // 1 / (sigma sqrt 2), 1 / sigma, e_0 .. e_(n-1), n
    struct Tgt { float ehi, elo; bool hi, lo; };                 // the label's own edges; hi / lo: whether it has one on that side
    template <bool, bool>
    static __device__ __forceinline__ Par par(const Lik& L) {
        const float rsig = 1.f / L.p0_dev[0];
        return {BO_RSQRT2 * rsig, rsig, L.p0_dev + 1, (int)L.p1};
    }
    // a label outside 0 .. n is read as the nearest bin (the edge array is never indexed out of bounds; the host checks the targets)
    static __device__ __forceinline__ Tgt tgt(const Par& P, float y) {
        const int yi = min(max((int)y, 0), P.n);
        Tgt T;
        T.hi = yi < P.n; T.lo = yi > 0;
        T.ehi = T.hi ? P.edges[yi] : INFINITY;
        T.elo = T.lo ? P.edges[yi - 1] : -INFINITY;
        return T;
    }
    static __device__ __forceinline__ float E0(const Par&) { return 0.f; }
    static __device__ __forceinline__ float DP0(const Par&) { return 0.f; }
    template <bool GRAD>
    static __device__ __forceinline__ float eval(const Par& P, const Tgt& T, float f, float& gp, float& gpar) {
        const float a = (T.ehi - f) * P.k, b = (T.elo - f) * P.k;           // (e - f) / (sigma sqrt 2); +-inf on an open side
        const float den = fmaf(BO_C, bo_phi_diff(a, b), BO_Y_EPS);
        if (GRAD) {
            // d Phi(x) = phi(x) dx with x = (e - f) / sigma: dx/df = -1 / sigma, dx/dsigma = -x / sigma; an open side contributes nothing
            // (inf * 0 is never formed)
            const float pa = T.hi ? __expf(-a * a) : 0.f, pb = T.lo ? __expf(-b * b) : 0.f;
            const float xa = T.hi ? a * pa : 0.f, xb = T.lo ? b * pb : 0.f;
            const float c = BO_C * BO_RSQRT2PI * P.rsig / den;
            gp = c * (pb - pa);
            gpar = c * 1.41421356237309505f * (xb - xa);
        }
        return logf(den);
    }
    static __device__ __forceinline__ void cond_moments(const Par& P, float mu, float a, float& ey, float& ey2) {
        // sum_j j P_j = C sum_{j < n} Q_j and sum_j j^2 P_j = C sum_{j < n} (2 j + 1) Q_j, Q_j = 1 - Phi((e_j - f) / sigma) (summation by
        // parts: Phi_n = 1): positive terms only.  The edges are the outer loop, the rule the inner one.
        float s1 = 0.f, s2 = 0.f;
        for (int e = 0; e < P.n; ++e) {
            const float c = (P.edges[e] - mu) * P.k, d = a * P.k;
            float qe = 0.f;
#pragma unroll 1
            for (int j = 0; j < 10; ++j) {
                const float xd = d * GH_X[j];
                qe = fmaf(GH_W[j], 0.5f * (erfcf(c - xd) + erfcf(c + xd)), qe);
            }
            s1 += qe;
            s2 = fmaf((float)(2 * e + 1), qe, s2);
        }
        ey = BO_C * s1; ey2 = BO_C * s2;
    }
};

// E_{N(f; mu, v)} logp(f, y) by the rule; GRAD: dE/dmu, dE/dv, dE/dparam[0] by its reparameterised form (lik_quad of likelihood_tail.hip)
template <int TYPE, bool GRAD>
__device__ __forceinline__ float bo_quad(const typename BoFam<TYPE>::Par& P, float mu, float v, float y, float& dmu, float& dv, float& dpar) {
    using F = BoFam<TYPE>;
    const typename F::Tgt T = F::tgt(P, y);
    const float a = sqrtf(2.f * fmaxf(v, LIK_V_FLOOR));
    float E = 0.f, s1 = 0.f, s2 = 0.f, sp = 0.f;
#pragma unroll 1
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        float gpa = 0.f, gpb = 0.f, qa = 0.f, qb = 0.f;
        const float ga = F::template eval<GRAD>(P, T, mu + xa, gpa, qa);
        const float gb = F::template eval<GRAD>(P, T, mu - xa, gpb, qb);
        E = fmaf(GH_W[j], ga + gb, E);
        if (GRAD) {
            s1 = fmaf(GH_W[j], gpa + gpb, s1);
            s2 = fmaf(GH_W[j] * GH_X[j], gpa - gpb, s2);
            sp = fmaf(GH_W[j], qa + qb, sp);
        }
    }
    if (GRAD) { dmu = s1; dv = s2 / a; dpar = sp + F::DP0(P); }
    return E + F::E0(P);
}

// predict_density of one element: log sum_i exp(g(f_i) + log w_i), the largest term first, then the sum (g is evaluated twice; nothing is
// kept in scratch)
template <int TYPE>
__device__ __forceinline__ float bo_density(const typename BoFam<TYPE>::Par& P, float mu, float v, float y) {
    using F = BoFam<TYPE>;
    const typename F::Tgt T = F::tgt(P, y);
    const float a = sqrtf(2.f * fmaxf(v, 0.f));
    float d0, d1, mx = -INFINITY;
#pragma unroll 1
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        mx = fmaxf(mx, GH_LOGW[j] + fmaxf(F::template eval<false>(P, T, mu + xa, d0, d1), F::template eval<false>(P, T, mu - xa, d0, d1)));
    }
    float s = 0.f;
#pragma unroll 1
    for (int j = 0; j < 10; ++j) {
        const float xa = a * GH_X[j];
        s += __expf(GH_LOGW[j] + F::template eval<false>(P, T, mu + xa, d0, d1) - mx) + __expf(GH_LOGW[j] + F::template eval<false>(P, T, mu - xa, d0, d1) - mx);
    }
    return mx + logf(s) + F::E0(P);
}

// predict_mean_and_var of one element: (E_y, E_y2 - E_y^2)
template <int TYPE>
__device__ __forceinline__ void bo_mean_var(const typename BoFam<TYPE>::Par& P, float mu, float v, float& ey, float& ev) {
    float ey2;
    BoFam<TYPE>::cond_moments(P, mu, sqrtf(2.f * fmaxf(v, 0.f)), ey, ey2);
    ev = fmaf(-ey, ey, ey2);
}

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint: the cores of likelihood_common.h over the quadrature, one output at a time.  A point
// has no state of its own.  part[B..2B): the share of d / d scale (Beta) or d / d sigma (Ordinal).
// ------------------------------------------------------------------------------------------
template <int TYPE>
struct BoOps {
    static constexpr bool HAS_CONST = false;
    struct Point {};
    const typename BoFam<TYPE>::Par& P; int Dy;
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float*, long long, bool, int) const { return {}; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float* var, const float* Y, long long b) const {
        float acc = 0.f, d0, d1, d2;
        for (int d = 0; d < Dy; ++d) acc += bo_quad<TYPE, false>(P, mu[d], var[d], Y[b * Dy + d], d0, d1, d2);
        return acc;
    }
    __device__ __forceinline__ double heads(const Point&, const float* mu, const float* var, const float* Y, long long b, float wt,
                                            float* dm, float* dv, double ds) const {
        for (int j = 0; j < Dy; ++j) {
            float dmu, dvv, dp;
            bo_quad<TYPE, true>(P, mu[j], var[j], Y[b * Dy + j], dmu, dvv, dp);
            if (dm) dm[j] = wt * dmu;
            if (dv) dv[j] = wt * dvv;
            ds += (double)wt * (double)dp;
        }
        return ds;
    }
};

// A workgroup takes ONE pass of LIK_THREADS / SEG points, as k_lik_elbo does and for its reason: a sample costs 20 x Dy node evaluations.
template <int TYPE, int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_bo_elbo(LikReduceArgs g) {
    const auto P = BoFam<TYPE>::template par<true, false>(g.lik);
    const BoOps<TYPE> ops{P, g.Dy};
    elbo_points<SEG, false>(g, ops);
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_bo_elbo_bwd(LikBwdArgs a) {
    const auto P = BoFam<TYPE>::template par<true, true>(a.lik);
    const BoOps<TYPE> ops{P, a.Dy};
    elbo_bwd_point(a, ops);
}

// ------------------------------------------------------------------------------------------
// Elementwise callables.  MODE 0: variational_expectations; 1: predict_density (Fvar == NULL: logp); 2: predict_mean_and_var
// ------------------------------------------------------------------------------------------
template <int TYPE, int MODE>
__global__ __launch_bounds__(256) void k_bo_elem(Lik L, const float* __restrict__ Fmu, const float* __restrict__ Fvar,
                                                 const float* __restrict__ Y, long long n, int Dy, long long row_div, long long row_mod,
                                                 float* __restrict__ out, float* __restrict__ out2) {
    using F = BoFam<TYPE>;
    const auto P = F::template par<MODE != 2, false>(L);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const float mu = Fmu[idx];
        float d0, d1, d2;
        if (MODE == 2) {
            float ey, ev;
            bo_mean_var<TYPE>(P, mu, Fvar[idx], ey, ev);
            out[idx] = ey; out2[idx] = ev;
            continue;
        }
        const long long t = idx / Dy;
        const int d = (int)(idx - t * Dy);
        const float y = Y[((t / row_div) % row_mod) * Dy + d];
        if (MODE == 0) { out[idx] = bo_quad<TYPE, false>(P, mu, Fvar[idx], y, d0, d1, d2); continue; }
        if (!Fvar) { out[idx] = F::template eval<false>(P, F::tgt(P, y), mu, d0, d1) + F::E0(P); continue; }
        out[idx] = bo_density<TYPE>(P, mu, Fvar[idx], y);
    }
}

// ------------------------------------------------------------------------------------------
// iwvi_lik_predict_mixture for the two types: the point loop of likelihood_common.h over the two functions above.
// ------------------------------------------------------------------------------------------
template <int TYPE>
struct BoMixOps {
    static constexpr bool HAS_CONST = false;
    const typename BoFam<TYPE>::Par& P;
    __device__ __forceinline__ float density(float mu, float v, float y) const { return bo_density<TYPE>(P, mu, v, y); }
    __device__ __forceinline__ float target_const(float) const { return 0.f; }
    __device__ __forceinline__ void mean_var(float mu, float v, float& ey, float& ev) const { bo_mean_var<TYPE>(P, mu, v, ey, ev); }
};
template <int TYPE, int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_bo_mix(LikMixArgs g) {
    const auto P = BoFam<TYPE>::template par<true, false>(g.lik);
    const BoMixOps<TYPE> ops{P};
    mix_points<SEG>(g, ops);
}

// the type is a template argument of every kernel: f(integral_constant<int, TYPE>)
template <class F>
static inline int bo_type_dispatch(int type, F&& f) {
    if (type == IWVI_LIK_BETA) return f(std::integral_constant<int, IWVI_LIK_BETA>{});
    return f(std::integral_constant<int, IWVI_LIK_ORDINAL>{});
}

int bo_launch_elbo(const LikReduceArgs& g, hipStream_t stream) {
    return bo_type_dispatch(g.lik.type, [&](auto ty) {
        return seg_dispatch(g.K, [&](auto seg) {
            constexpr int SEG = decltype(seg)::value;
            hipLaunchKernelGGL((k_bo_elbo<decltype(ty)::value, SEG>), dim3((unsigned)lik_passes(g.B, SEG)), dim3(LIK_THREADS), 0, stream, g);
            return check_launch("k_bo_elbo");
        });
    });
}

int bo_launch_mix(const LikMixArgs& g, hipStream_t stream) {
    return bo_type_dispatch(g.lik.type, [&](auto ty) {
        return seg_dispatch(g.S, [&](auto seg) {
            constexpr int SEG = decltype(seg)::value;
            hipLaunchKernelGGL((k_bo_mix<decltype(ty)::value, SEG>), dim3(mix_blocks(g.N, SEG)), dim3(LIK_THREADS), 0, stream, g);
            return check_launch("k_bo_mix");
        });
    });
}

int bo_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream) {
    return bo_type_dispatch(a.lik.type, [&](auto ty) {
        hipLaunchKernelGGL(k_bo_elbo_bwd<decltype(ty)::value>, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
        return check_launch("k_bo_elbo_bwd");
    });
}

int bo_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream) {
    const long long n = T * Dy;
    return bo_type_dispatch(L.type, [&](auto ty) {
        return launch_elem_mode(what, mode, n, [&](auto m, int blocks) {
            hipLaunchKernelGGL((k_bo_elem<decltype(ty)::value, decltype(m)::value>), dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, Dy,
                               row_div, row_mod, out, out2);
        });
    });
}

}  // namespace iwvi
