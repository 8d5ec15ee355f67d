// The bound family between the K-sample ELBO and the importance-weighted bound (Rainforth et al. 2018; Li & Turner 2016): MIWAE, CIWAE and the
// tempered (VR-alpha) log-sum-exp as ONE triple (groups G, tau, beta) -- include/iwvi_hip.h: iwvi_bound_desc.  Per data point n, K_g = K / G:
//   bound_n = beta (1/K) sum_k L_nk + (1 - beta) (1/G) sum_g (1/tau) [ logsumexp_{k in g}(tau L_nk) - log K_g ]
//   w_nk    = beta / K + (1 - beta) / G softmax_{k' in group(k)}(tau L_nk')_k
// Two cores over the policy interface of likelihood_common.h (point / expect / heads / HAS_CONST), in the layouts of the kernels they stand
// beside: bound_points (k_elbo's: SEG lanes per point) and bound_bwd_point (k_elbo_bwd's: one wave per point, lanes striding K by 64).
// Both walk a point's samples in chunks of SEG (64) and see a group as a run of neighbouring lanes of a chunk: group_chunk below.
#include "likelihood_common.h"

namespace iwvi {

struct BoundPar { int G, Kg; float tau, beta; };

// x = tau L, ROUNDED: the product is never fused into the subtraction of the group's maximum that follows it (x - m would become
// fma(tau, L, -m) in some places and not in others, and a sample's term would differ from its share of the group's sum by the rounding of x)
__device__ __forceinline__ float tempered_term(float tau, float L) {
#pragma clang fp contract(off)
    return tau * L;
}

// One chunk (samples k0 .. k0 + SEG - 1, lane sl holds k = k0 + sl) of a point's groups.  x: the lane's tau L_nk, -inf where it has no sample
// (on = false).  term(k) -> tau L_nk of ANY sample of the point (the lanes of a segment call it with different k).
// A group lies in the chunk as a run of lanes [rs, re].  A run that IS its group (contained) is reduced by a segmented scan: a lane only
// ever takes values from lanes of its own run, so no term of a neighbouring group is read.  A group that goes on beyond the chunk -- there
// is at most one: the group of the chunk's last sample -- is reduced over its whole range [gts, gte) by all SEG lanes the first time a chunk
// meets it, and carried (cm, cs) for the chunks that follow: the group that reaches into a chunk from below is always the one carried.
// -> (gm, gsum): max and sum exp(x - max) of the lane's group; acc: the lane's float64 share of sum_g [gm + log gsum - log K_g] (every group is
// added exactly once, by the last lane of its run or, for a carried group, by lane 0 of the chunk that formed it).
template <int SEG, class TERM>
__device__ __forceinline__ void group_chunk(int k0, int sl, int K, int Kg, bool live, float x, TERM&& term, float& cm, double& cs,
                                            double& acc, float& gm, double& gsum) {
    const int k = k0 + sl;
    const bool on = live && k < K;
    const int g = k / Kg, gs = g * Kg, ge = gs + Kg;
    const int rs = gs > k0 ? gs - k0 : 0;                       // the run of this lane's group inside the chunk
    const int re = ge - 1 - k0 < SEG - 1 ? ge - 1 - k0 : SEG - 1;
    float mx = x;
#pragma unroll
    for (int o = 1; o < SEG; o <<= 1) {
        const float t = __shfl_up(mx, o, SEG);
        if (sl - o >= rs) mx = fmaxf(mx, t);
    }
    mx = __shfl(mx, re, SEG);                                    // the run's maximum, in every lane of the run
    double sm = (on && mx != -INFINITY) ? (double)__expf(x - mx) : 0.0;
#pragma unroll
    for (int o = 1; o < SEG; o <<= 1) {
        const double t = __shfl_up(sm, o, SEG);
        if (sl - o >= rs) sm += t;
    }
    sm = __shfl(sm, re, SEG);
    const bool contained = gs >= k0 && ge <= k0 + SEG;
    if (contained && on && sl == re) acc += (double)mx + log(sm) - log((double)Kg);
    // ---- the group of the chunk's last sample, when it goes on beyond the chunk (uniform in the segment: k0, K, Kg only) ----
    const int kt = k0 + SEG - 1;
    float nm = cm;
    double ns = cs;
    if (kt < K) {
        const int gts = (kt / Kg) * Kg, gte = gts + Kg;
        if (gte > k0 + SEG && gts >= k0) {                       // met for the first time: its whole range, by all SEG lanes
            float m = -INFINITY;
            for (int kk = gts + sl; kk < gte; kk += SEG) m = fmaxf(m, live ? term(kk) : -INFINITY);
            m = lseg_max<SEG>(m);
            double s = 0.0;
            for (int kk = gts + sl; kk < gte; kk += SEG) s += (live && m != -INFINITY) ? (double)__expf(term(kk) - m) : 0.0;
            s = lseg_sum<SEG>(s);
            nm = m; ns = s;
            if (live && sl == 0) acc += (double)m + log(s) - log((double)Kg);
        }
    }
    if (contained) { gm = mx; gsum = sm; }
    else if (gs < k0) { gm = cm; gsum = cs; }                    // reaches in from below: carried
    else { gm = nm; gsum = ns; }                                 // goes on beyond the chunk: just formed
    cm = nm; cs = ns;
}

// ---- the reduction ----
struct BoundReduceArgs {
    const float* fmean; const float* fvar; const float* Y;
    const float* kl[IWVI_MAX_KL]; int kl_dims[IWVI_MAX_KL]; int n_kl;
    long long B, stride_b, stride_k; int K, Dy;
    BoundPar bp;
    float* logp; float* ess;
    double* elbo; unsigned long long* ticket; double scale;
    const double* klg[LIK_MAX_GLOB]; int klg_n[LIK_MAX_GLOB]; int n_glob;
};
constexpr int BOUND_PTS = 64;             // points per workgroup, as k_elbo

// precomputed log-weights as a policy: the "moments" of a sample are its one log-weight
struct LogwOps {
    static constexpr bool HAS_CONST = false;
    struct Point {};
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float*, long long, bool, int) const { return {}; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float*, const float*, long long) const { return mu[0]; }
};

// the Gaussian's closed-form expectation and heads (csrc/backward.hip: k_elbo_bwd's arithmetic, term by term)
struct GaussOps {
    static constexpr bool HAS_CONST = false;
    struct Point {};
    float s, c0; int Dy;
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float*, long long, bool, int) const { return {}; }
    __device__ __forceinline__ float expect(const Point&, const float* mu, const float* var, const float* Y, long long b) const {
        float l = 0.f;
        for (int j = 0; j < Dy; ++j) {
            const float e = Y[b * Dy + j] - mu[j];
            l += c0 - 0.5f * (e * e + var[j]) / s;
        }
        return l;
    }
    __device__ __forceinline__ double heads(const Point&, const float* mu, const float* var, const float* Y, long long b, float wt,
                                            float* dm, float* dv, double ds) const {
        for (int j = 0; j < Dy; ++j) {
            const float e = Y[b * Dy + j] - mu[j], v = var[j];
            if (dm) dm[j] = wt * e / s;
            if (dv) dv[j] = -0.5f * wt / s;
            ds += (double)wt * (-0.5 / (double)s + 0.5 * ((double)e * e + (double)v) / ((double)s * s));
        }
        return ds;
    }
};

// SEG lanes per data point, BOUND_PTS points per workgroup in passes of 256 / SEG; float32 inside a sample, the groups' log-sum-exps, the sum
// over the groups, Kish's effective sample size and the sum over the points in float64.  The last workgroup to arrive adds the published
// logp up in a fixed order (the ticket protocol of k_elbo), so two calls give the same bits.
template <int SEG, class OPS>
__device__ __forceinline__ void bound_points(const BoundReduceArgs& g, const OPS& ops) {
    __shared__ double red[LIK_THREADS];
    __shared__ int is_last;
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;
    const int K = g.K, Dy = g.Dy, Kg = g.bp.Kg;
    const float tau = g.bp.tau;
    for (int pp = 0; pp < BOUND_PTS; pp += PPP) {
        const long long b = (long long)blockIdx.x * BOUND_PTS + pp + sg;
        const bool live = b < g.B;                    // uniform within a segment
        const auto pt = ops.template point<SEG, false>(g.Y, b, live, sl);
        auto logw = [&](int k) {
            const long long t = b * g.stride_b + (long long)k * g.stride_k;
            float a = ops.expect(pt, g.fmean + t * Dy, g.fvar + t * Dy, g.Y, b);
            for (int i = 0; i < g.n_kl; ++i)
                for (int d = 0; d < g.kl_dims[i]; ++d) a -= g.kl[i][t * g.kl_dims[i] + d];
            return a;
        };
        auto term = [&](int k) { return tempered_term(tau, logw(k)); };
        float m = -INFINITY, cm = -INFINITY, gm;
        double s1 = 0.0, s2 = 0.0, lsum = 0.0, cs = 0.0, acc = 0.0, gsum;
        for (int k0 = 0; k0 < K; k0 += SEG) {
            const bool on = live && k0 + sl < K;
            const float L = on ? logw(k0 + sl) : -INFINITY;
            lsum += on ? (double)L : 0.0;
            // all K samples: running maximum, sum exp(L - m) and sum exp(2 (L - m)) for the effective sample size
            const float nm = fmaxf(m, lseg_max<SEG>(L));
            const float d = L - nm;
            const double c1 = lseg_sum<SEG>(on && nm != -INFINITY ? (double)__expf(d) : 0.0);
            const double c2 = lseg_sum<SEG>(on && nm != -INFINITY ? (double)__expf(2.f * d) : 0.0);
            const float r = m - nm;
            s1 = (m == -INFINITY ? 0.0 : s1 * (double)__expf(r)) + c1;
            s2 = (m == -INFINITY ? 0.0 : s2 * (double)__expf(2.f * r)) + c2;
            m = nm;
            group_chunk<SEG>(k0, sl, K, Kg, live, on ? tempered_term(tau, L) : -INFINITY, term, cm, cs, acc, gm, gsum);
        }
        lsum = lseg_sum<SEG>(lsum);
        acc = lseg_sum<SEG>(acc);
        if (live && sl == 0) {
            double lp = (double)g.bp.beta * (lsum / (double)K) + (1.0 - (double)g.bp.beta) * (acc / ((double)tau * (double)g.bp.G));
            if constexpr (OPS::HAS_CONST) lp += (double)ops.point_const(pt);
            if (g.logp) g.logp[b] = (float)lp;
            if (g.ess) g.ess[b] = fminf(fmaxf((float)(s1 * s1 / s2), 1.f), (float)K);       // (in [1, K] by Cauchy-Schwarz: the clamp only takes rounding off)
        }
    }
    if (!g.elbo) return;
    // ---- publish this workgroup's logp, draw a ticket, the last arriver sums everything (csrc/lv_elbo.hip: k_elbo) ----
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
    double sum = 0.0;
    for (long long b = tid; b < g.B; b += LIK_THREADS) sum += (double)g.logp[b];
    red[tid] = sum;
    __syncthreads();
    for (int s = LIK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        double kl = 0.0;
        for (int i = 0; i < g.n_glob; ++i)
            for (int c = 0; c < g.klg_n[i]; ++c) kl += g.klg[i][c];
        *g.elbo = red[0] * g.scale - kl;
    }
}

template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_bound_logw(BoundReduceArgs g) {
    bound_points<SEG>(g, LogwOps{});
}

// ---- the heads of the adjoint ----
struct BoundBwdArgs {
    const float* fmean; const float* fvar; const float* Y; int Dy;
    const float* kl[IWVI_MAX_KL]; int kl_dims[IWVI_MAX_KL]; int n_kl;
    long long B; int K; float lik_var; const float* lik_var_dev; double scale;
    BoundPar bp;
    float* w; float* d_mean; float* d_var; double* part;   // part[0..B) = bound_n, part[B..2B) = d param[0] share
};

// One wave per data point, lanes over its K samples striding by 64.  A chunk of 64 samples is evaluated once (every lane keeps its L_nk);
// only a group that crosses a chunk boundary has its samples evaluated a second time, when group_chunk forms its total.
template <class OPS>
__device__ __forceinline__ void bound_bwd_point(const BoundBwdArgs& a, const OPS& ops) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int Dy = a.Dy, K = a.K;
    const float tau = a.bp.tau;
    const auto pt = ops.template point<64, true>(a.Y, b, true, lane);
    auto logw = [&](int k) {
        const long long t = b * K + k;
        float l = ops.expect(pt, a.fmean + t * Dy, a.fvar + t * Dy, a.Y, b);
        for (int i = 0; i < a.n_kl; ++i)
            for (int q = 0; q < a.kl_dims[i]; ++q) l -= a.kl[i][t * a.kl_dims[i] + q];
        return l;
    };
    auto term = [&](int k) { return tempered_term(tau, logw(k)); };
    const double wu = (double)a.bp.beta / (double)K, wg = (1.0 - (double)a.bp.beta) / (double)a.bp.G;
    float cm = -INFINITY, gm;
    double cs = 0.0, acc = 0.0, lsum = 0.0, ds = 0.0, gsum;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const bool on = k < K;
        const float L = on ? logw(k) : -INFINITY;
        const float x = on ? tempered_term(tau, L) : -INFINITY;
        lsum += on ? (double)L : 0.0;
        group_chunk<64>(k0, lane, K, a.bp.Kg, true, x, term, cm, cs, acc, gm, gsum);
        if (on) {
            const long long t = b * K + k;
            const float wt = (float)(a.scale * (wu + wg * (double)__expf(x - gm) / gsum));
            if (a.w) a.w[t] = wt;
            ds = ops.heads(pt, a.fmean + t * Dy, a.fvar + t * Dy, a.Y, b, wt, a.d_mean ? a.d_mean + t * Dy : nullptr,
                           a.d_var ? a.d_var + t * Dy : nullptr, ds);
        }
    }
    ds = lseg_sum<64>(ds);
    lsum = lseg_sum<64>(lsum);
    acc = lseg_sum<64>(acc);
    if (lane == 0) {
        double lp = (double)a.bp.beta * (lsum / (double)K) + (1.0 - (double)a.bp.beta) * (acc / ((double)tau * (double)a.bp.G));
        if constexpr (OPS::HAS_CONST) lp += (double)ops.point_const(pt);
        a.part[b] = lp;
        a.part[a.B + b] = ds;
    }
}

__global__ __launch_bounds__(256) void k_bound_bwd(BoundBwdArgs a) {
    const float s = a.lik_var_dev ? *a.lik_var_dev : a.lik_var;
    bound_bwd_point(a, GaussOps{s, -0.5f * logf(6.283185307179586f * s), a.Dy});
}

// out[0] = sum part[0..n), out[1] = sum part[n..2n), out[2] = scale * out[0] - sum of the global KL shares (the bound); fixed order
struct BoundFinishArgs { const double* part; long long n; double scale; const double* klg[IWVI_MAX_LAYERS]; int kln[IWVI_MAX_LAYERS]; int n_glob; double* out; };
__global__ __launch_bounds__(256) void k_bound_finish(BoundFinishArgs a) {
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

// the descriptor checks both entries share -> IWVI_OK and the kernel's form of the triple
static int take_bound(const iwvi_bound_desc* d, int K, BoundPar& bp, const char* what) {
    if (!d) { set_error("%s: null bound descriptor", what); return IWVI_ERR_ARG; }
    if (d->groups < 1 || K % d->groups != 0) { set_error("%s: groups=%d must be >= 1 and divide K=%d", what, d->groups, K); return IWVI_ERR_ARG; }
    if (!(d->tau > 0.f && d->tau <= 1.f)) { set_error("%s: tau=%g outside (0, 1]", what, (double)d->tau); return IWVI_ERR_ARG; }
    if (!(d->beta >= 0.f && d->beta <= 1.f)) { set_error("%s: beta=%g outside [0, 1]", what, (double)d->beta); return IWVI_ERR_ARG; }
    bp.G = d->groups; bp.Kg = K / d->groups; bp.tau = d->tau; bp.beta = d->beta;
    return IWVI_OK;
}

}  // namespace iwvi

using namespace iwvi;

extern "C" int iwvi_bound_logw_reduce(const iwvi_bound_desc* bound, const float* logw, int64_t B, int K, int64_t stride_b, int64_t stride_k,
                                      const double* const* kl_global, const int32_t* kl_global_counts, int n_glob, double scale,
                                      float* out_logp, float* out_ess, double* out_elbo, uint64_t* ticket, void* stream_) {
    const char* what = "iwvi_bound_logw_reduce";
    if (!logw) { set_error("%s: null input", what); return IWVI_ERR_ARG; }
    if (B <= 0 || K <= 0) { set_error("%s: empty minibatch or K=%d", what, K); return IWVI_ERR_ARG; }
    if (out_elbo && (!out_logp || !ticket)) { set_error("%s: out_elbo needs out_logp (scratch) and a zero-initialised ticket word", what); return IWVI_ERR_ARG; }
    BoundReduceArgs g{};
    int rc;
    if ((rc = take_bound(bound, K, g.bp, what)) != IWVI_OK) return rc;
    g.fmean = logw; g.fvar = logw; g.stride_b = stride_b; g.stride_k = stride_k;
    g.B = B; g.K = K; g.Dy = 1;
    g.logp = out_logp; g.ess = out_ess; g.elbo = out_elbo; g.ticket = (unsigned long long*)ticket; g.scale = scale;
    if (out_elbo) {
        if (n_glob < 0 || n_glob > LIK_MAX_GLOB) { set_error("%s: too many global KL terms (%d > %d)", what, n_glob, LIK_MAX_GLOB); return IWVI_ERR_ARG; }
        for (int i = 0; i < n_glob; ++i) {
            if (!kl_global || !kl_global[i]) { set_error("%s: null global KL pointer %d", what, i); return IWVI_ERR_ARG; }
            g.klg[i] = kl_global[i];
            g.klg_n[i] = kl_global_counts ? kl_global_counts[i] : 1;
            if (g.klg_n[i] <= 0 || g.klg_n[i] > IWVI_MAX_R) { set_error("%s: bad global KL count %d", what, g.klg_n[i]); return IWVI_ERR_ARG; }
        }
        g.n_glob = n_glob;
    }
    if (!out_logp && !out_ess) return IWVI_OK;                   // nothing asked for
    const unsigned blocks = (unsigned)((B + BOUND_PTS - 1) / BOUND_PTS);
    hipStream_t stream = (hipStream_t)stream_;
    return seg_dispatch(K, [&](auto seg) {
        hipLaunchKernelGGL(k_bound_logw<decltype(seg)::value>, dim3(blocks), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_bound_logw");
    });
}

extern "C" int iwvi_bound_elbo_backward(const iwvi_bound_desc* bound, const float* fmean, const float* fvar, const float* Y, int Dy,
                                        const float* const* kl_local, const int32_t* kl_dims, int n_local,
                                        int64_t B, int K, float lik_variance, const float* lik_variance_dev, double scale,
                                        float* out_w, float* d_mean, float* d_var,
                                        const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                                        double* out_sums, double* ws, void* stream_) {
    const char* what = "iwvi_bound_elbo_backward";
    if (!fmean || !fvar || !Y || !out_sums || !ws || Dy <= 0 || B <= 0 || K <= 0 || n_local < 0 || n_local > IWVI_MAX_KL || !(lik_variance > 0.f) ||
        n_glob < 0 || n_glob > IWVI_MAX_LAYERS) {
        set_error("%s: bad argument", what); return IWVI_ERR_ARG;
    }
    BoundBwdArgs a{};
    int rc;
    if ((rc = take_bound(bound, K, a.bp, what)) != IWVI_OK) return rc;
    a.fmean = fmean; a.fvar = fvar; a.Y = Y; a.Dy = Dy; a.n_kl = n_local;
    for (int i = 0; i < n_local; ++i) {
        if (!kl_local || !kl_local[i] || !kl_dims || kl_dims[i] <= 0) { set_error("%s: bad local regulariser %d", what, i); return IWVI_ERR_ARG; }
        a.kl[i] = kl_local[i]; a.kl_dims[i] = kl_dims[i];
    }
    BoundFinishArgs fa{};
    fa.part = ws; fa.n = B; fa.scale = scale; fa.n_glob = n_glob; fa.out = out_sums;
    for (int i = 0; i < n_glob; ++i) {
        if (!kl_global || !kl_global[i] || !kl_global_counts || kl_global_counts[i] <= 0) { set_error("%s: bad global KL %d", what, i); return IWVI_ERR_ARG; }
        fa.klg[i] = kl_global[i]; fa.kln[i] = kl_global_counts[i];
    }
    a.B = B; a.K = K; a.lik_var = lik_variance; a.lik_var_dev = lik_variance_dev; a.scale = scale;
    a.w = out_w; a.d_mean = d_mean; a.d_var = d_var; a.part = ws;
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_bound_bwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_bound_finish, dim3(1), dim3(256), 0, st, fa);
    return check_launch("k_bound_bwd");
}
