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

// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6 (six steps at the most: the loop is bounded whatever the device
// scalar holds), then the asymptotic series (next term 691 / (32760 x^12) < 1e-11)
__device__ __forceinline__ double xl_digamma(double x) {
    double r = 0.0;
    for (int i = 0; i < 6 && x < 6.0; ++i) { r -= 1.0 / x; x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    return r + log(x) - 0.5 * i - i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0)))));
}

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
        if (PSI) P.psi = xl_digamma((double)a);
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

template <int SEG>
__device__ __forceinline__ float xl_seg_sum(float v) {
#pragma unroll
    for (int o = SEG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------
// The reduction: k_lik_elbo's contracts (ms / logp / elbo, the release / ticket / acquire epilogue).  SEG lanes per data point, one lane per
// sample walking its Dy outputs; float32 inside a sample, the log-sum-exp over K and the sum over the points in float64.  A workgroup takes
// LIK_THREADS / SEG points per pass and as many passes as the grid leaves it: the launcher spreads the points over up to XL_MAX_BLOCKS
// workgroups, ONE pass each at B = 1024.  (k_elbo's 64 points per workgroup -- csrc/lv_elbo.hip -- were tried first, a sample being a handful
// of FMAs and one exp: 16 workgroups at configs[2], and an evaluation took 74.5-79.0 us against the Student-t's 68.3 in the same session.  The
// per-sample work is small, but a pass is a chain of dependent loads and cross-lane reductions, and eight of them in a row on 16 of 256 CUs
// is what the time went into -- the finding of DESIGN.md section 6 for k_lik_elbo, again.)
// ------------------------------------------------------------------------------------------
constexpr int XL_MAX_BLOCKS = 1024;     // four workgroups per CU

template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_xl_elbo(LikReduceArgs g) {
    __shared__ double red[LIK_THREADS];
    __shared__ int is_last;
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;           // points per pass
    const int K = g.K, Dy = g.Dy;
    const XlPar P = xl_par<true, false>(g.lik);
    for (long long b0 = (long long)blockIdx.x * PPP; b0 < g.B; b0 += (long long)gridDim.x * PPP) {   // (uniform in the workgroup)
        const long long b = b0 + sg;
        const bool live = b < g.B;                    // uniform within a segment
        // sum_d c0(y_bd): once per point, the segment's lanes over the outputs
        float cb = 0.f;
        if (live && P.type != IWVI_LIK_EXPONENTIAL)
            for (int d = sl; d < Dy; d += SEG) { float ly; cb += xl_c0(P, g.Y[b * Dy + d], ly); }
        cb = xl_seg_sum<SEG>(cb);
        float m = -INFINITY;
        double ssum = 0.0, lsum = 0.0;
        for (int k0 = 0; k0 < K; k0 += SEG) {
            const int k = k0 + sl;
            const bool on = live && k < K;
            float L = -INFINITY;
            if (on) {
                const long long t = b * g.stride_b + k * g.stride_k;
                float acc = 0.f, e;
                for (int d = 0; d < Dy; ++d)
                    acc += xl_g(P, g.Y[b * Dy + d], g.fmean[t * Dy + d], 0.5f * g.fvar[t * Dy + d], e);
                for (int i = 0; i < g.n_kl; ++i)
                    for (int d = 0; d < g.kl_dims[i]; ++d) acc -= g.kl[i][t * g.kl_dims[i] + d];
                L = acc;
            }
            if (g.mode_vi) { lsum += lseg_sum<SEG>(on ? (double)L : 0.0); continue; }
            const float nm = fmaxf(m, lseg_max<SEG>(L));
            const double cs = lseg_sum<SEG>(on ? (double)__expf(L - nm) : 0.0);
            ssum = (m == -INFINITY ? 0.0 : ssum * (double)__expf(m - nm)) + cs;
            m = nm;
        }
        if (live && sl == 0) {
            if (g.mode_vi) {
                if (g.logp) g.logp[b] = (float)(lsum / (double)K + (double)cb);                      // models.py:84
            } else {
                m += cb;                                                                              // c0 outside the log-sum-exp
                if (g.ms) { g.ms[2 * b] = m; g.ms[2 * b + 1] = (float)ssum; }
                if (g.logp) g.logp[b] = (float)((double)m + log(ssum) - log((double)g.K_total));     // models.py:148
            }
        }
    }
    if (!g.elbo) return;
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

// ------------------------------------------------------------------------------------------
// Heads of the bound's adjoint: k_lik_elbo_bwd with the closed forms.  One wave per data point, lanes over its K samples striding by 64.
// Pass 1: L_nk (without the point's constant: it cancels in the weights) and the running (max, sum exp); pass 2: the weights and the heads.
// part[B..2B): the share of d / d shape (Gamma), sum_k w_k sum_d (-mu_kd - psi(a) + log y_d); 0 for the other two.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_xl_elbo_bwd(LikBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const XlPar P = xl_par<true, true>(a.lik);
    const bool gam = P.type == IWVI_LIK_GAMMA;
    // once per point: sum_d c0(y_d) and (Gamma) sum_d log y_d, the lanes over the outputs
    float cb = 0.f, lyb = 0.f;
    if (P.type != IWVI_LIK_EXPONENTIAL)
        for (int j = lane; j < a.Dy; j += 64) { float ly; cb += xl_c0(P, a.Y[b * a.Dy + j], ly); lyb += ly; }
    for (int o = 32; o > 0; o >>= 1) { cb += __shfl_xor(cb, o, 64); lyb += __shfl_xor(lyb, o, 64); }
    auto logw = [&](long long t) {
        float l = 0.f, e;
        for (int j = 0; j < a.Dy; ++j)
            l += xl_g(P, a.Y[b * a.Dy + j], a.fmean[t * a.Dy + j], 0.5f * a.fvar[t * a.Dy + j], e);
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
        if (a.lse_global) {                             // weights against the whole job's normaliser, which carries the constant
            mx = a.lse_global[b] - cb; se = 1.0;
        } else {
            for (int k = lane; k < a.K; k += 64) se += (double)__expf((one ? Lc : logw(b * a.K + k)) - mx);
            for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
        }
    }
    const double dpar0 = (double)lyb - (double)a.Dy * P.psi;     // sum_d (log y_d - psi(a))
    double ds = 0.0;
    for (int k = lane; k < a.K; k += 64) {
        const long long t = b * a.K + k;
        float wt;
        if (a.mode_vi) wt = (float)(a.scale / (double)a.K);
        else wt = (float)(a.scale * (double)__expf((one ? Lc : logw(t)) - mx) / se);
        if (a.w) a.w[t] = wt;
        double smu = 0.0;
        for (int j = 0; j < a.Dy; ++j) {
            const float y = a.Y[b * a.Dy + j], mu = a.fmean[t * a.Dy + j];
            float e;
            xl_g(P, y, mu, 0.5f * a.fvar[t * a.Dy + j], e);
            const bool pois = P.type == IWVI_LIK_POISSON;
            const float ce = (pois ? P.beta : y) * e;
            if (a.d_mean) a.d_mean[t * a.Dy + j] = wt * fmaf(-P.sg, ce, pois ? y : P.cmu);
            if (a.d_var) a.d_var[t * a.Dy + j] = wt * (-0.5f * ce);
            smu += (double)mu;
        }
        if (gam) ds += (double)wt * (dpar0 - smu);
    }
    for (int o = 32; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
    if (lane == 0) {
        a.part[b] = (double)cb + (a.mode_vi ? se / (double)a.K : (double)mx + log(se) - log((double)(a.lse_global ? a.K_total : a.K)));
        a.part[a.B + b] = ds;
    }
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

template <int SEG>
static int launch_xl_elbo(const LikReduceArgs& g, hipStream_t stream) {
    constexpr int PPP = LIK_THREADS / SEG;
    const long long passes = (g.B + PPP - 1) / PPP;
    const long long blocks = passes < XL_MAX_BLOCKS ? passes : XL_MAX_BLOCKS;
    hipLaunchKernelGGL(k_xl_elbo<SEG>, dim3((unsigned)blocks), dim3(LIK_THREADS), 0, stream, g);
    return check_launch("k_xl_elbo");
}

int xl_launch_elbo(const LikReduceArgs& g, hipStream_t stream) {
    if (g.K <= 4) return launch_xl_elbo<4>(g, stream);
    if (g.K <= 8) return launch_xl_elbo<8>(g, stream);
    if (g.K <= 16) return launch_xl_elbo<16>(g, stream);
    if (g.K <= 32) return launch_xl_elbo<32>(g, stream);
    return launch_xl_elbo<64>(g, stream);
}

template <int SEG>
static int launch_xl_mix(const LikMixArgs& g, hipStream_t stream) {
    hipLaunchKernelGGL(k_xl_mix<SEG>, dim3(mix_blocks(g.N, SEG)), dim3(LIK_THREADS), 0, stream, g);
    return check_launch("k_xl_mix");
}

int xl_launch_mix(const LikMixArgs& g, hipStream_t stream) {
    if (g.S <= 4) return launch_xl_mix<4>(g, stream);
    if (g.S <= 8) return launch_xl_mix<8>(g, stream);
    if (g.S <= 16) return launch_xl_mix<16>(g, stream);
    if (g.S <= 32) return launch_xl_mix<32>(g, stream);
    return launch_xl_mix<64>(g, stream);
}

int xl_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_xl_elbo_bwd, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
    return check_launch("k_xl_elbo_bwd");
}

int xl_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int Dy,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream) {
    const long long n = T * Dy;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    if (mode == 0) hipLaunchKernelGGL(k_xl_elem<0>, dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, Dy, row_div, row_mod, out, out2);
    else if (mode == 1) hipLaunchKernelGGL(k_xl_elem<1>, dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, Dy, row_div, row_mod, out, out2);
    else hipLaunchKernelGGL(k_xl_elem<2>, dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, Dy, row_div, row_mod, out, out2);
    return check_launch(what);
}

}  // namespace iwvi
