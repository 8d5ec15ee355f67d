// GPflow 1.x MultiClass(num_classes) with the RobustMax link (include/iwvi_hip.h: IWVI_LIK_MULTICLASS), behind the iwvi_lik_* entry
// points of csrc/likelihood_tail.hip.  Unlike the likelihoods there, the expectation couples all C outputs of a sample, and the targets
// are ONE column of class labels:
//   p = prob_is_largest(y; mu, v) = sum_i w_i prod_{c != y} Phi~((X_i - mu_c) / sqrt(max(v_c, 1e-10))),  X_i = mu_y + x_i sqrt(max(2 v_y, 1e-10)),
//   Phi~(d) = Phi(d) (1 - 2e-4) + 1e-4      -- the 20-point rule of likelihood_common.h; clips and jitter are GPflow's, part of the definition
//   variational_expectations = p log(1 - eps) + (1 - p) log(eps / (C - 1)).
// C is a runtime value: the class loop is OUTSIDE and the (unrolled) node loop inside, so the twenty running products live in registers
// and per class mu_c and 1 / sigma_c are loaded once -- a per-class array would be indexed dynamically and land in scratch.
#include "likelihood_common.h"

namespace iwvi {

constexpr float MC_CLIP = 1e-10f;                // tf.clip_by_value(., 1e-10, inf) on 2 v_y and on v_c
constexpr float MC_JIT = 1e-4f;                  // the cdf jitter of prob_is_largest

// Phi(d) = erfc(-d / sqrt 2) / 2: neither tail cancels
__device__ __forceinline__ float mc_cdf(float d) { return 0.5f * erfcf(-d * 0.70710678118654752f) * (1.f - 2.f * MC_JIT) + MC_JIT; }

// a label as the kernels index with it: kept inside [0, C) whatever the float holds (the Python side refuses other targets on the host)
__device__ __forceinline__ int mc_label(float y, int C) { return min(max((int)y, 0), C - 1); }

// p for label y of one sample (mu, var: its C moments); pa[j] / pb[j]: the products at the nodes +x_j / -x_j, a = sqrt(max(2 v_y, clip))
__device__ __forceinline__ float mc_prob(const float* __restrict__ mu, const float* __restrict__ var, int C, int y,
                                         float (&pa)[10], float (&pb)[10], float& a) {
    const float mu_y = mu[y];
    a = sqrtf(fmaxf(2.f * var[y], MC_CLIP));
#pragma unroll
    for (int j = 0; j < 10; ++j) pa[j] = pb[j] = 1.f;
    for (int c = 0; c < C; ++c) {
        if (c == y) continue;
        const float dm = mu_y - mu[c], rs = 1.f / sqrtf(fmaxf(var[c], MC_CLIP));
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
            pa[j] *= mc_cdf((dm + xa) * rs);
            pb[j] *= mc_cdf((dm - xa) * rs);
        }
    }
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) p = fmaf(GH_W[j], pa[j] + pb[j], p);
    return p;
}

// l0 = log eps_1, l1 = log(1 - eps).  The expectation is formed as p l1 + (1 - p) l0, not l0 + p (l1 - l0): near p = 1 the result is ~ -eps and
// the second form would carry the rounding of |l0| ~ 9; its derivative with respect to p is l1 - l0 either way.
__device__ __forceinline__ void mc_logs(const Lik& L, int C, float& l0, float& l1) {
    l0 = logf(L.p0 / (float)(C - 1));
    l1 = log1pf(-L.p0);
}
__device__ __forceinline__ float mc_ve(float p, float l0, float l1) { return fmaf(p, l1, (1.f - p) * l0); }

// gs * dp/dmu_c -> dmean[c], gs * dp/dv_c -> dvar[c] for all C classes: a second pass over the classes that recomputes d_ci and Phi~_ci and
// divides the full product P_i by it (Phi~ >= 1e-4).  Through an active clip the derivative is zero, as tf.clip_by_value gives.
__device__ __forceinline__ void mc_heads(const float* __restrict__ mu, const float* __restrict__ var, int C, int y, float gs,
                                         float* __restrict__ dmean, float* __restrict__ dvar) {
    float pa[10], pb[10], a;
    mc_prob(mu, var, C, y, pa, pb, a);
#pragma unroll
    for (int j = 0; j < 10; ++j) {                 // w_i P_i (1 - 2 jit) / sqrt(2 pi)
        const float w = GH_W[j] * (1.f - 2.f * MC_JIT) * 0.3989422804014327f;
        pa[j] *= w; pb[j] *= w;
    }
    const float mu_y = mu[y];
    float gmy = 0.f, gvy = 0.f;
    for (int c = 0; c < C; ++c) {
        if (c == y) continue;
        const float vc = var[c];
        const float dm = mu_y - mu[c], rs = 1.f / sqrtf(fmaxf(vc, MC_CLIP));
        float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const float xa = a * GH_X[j];
            const float da = (dm + xa) * rs, db = (dm - xa) * rs;
            const float ra = pa[j] * __expf(-0.5f * da * da) / mc_cdf(da);
            const float rb = pb[j] * __expf(-0.5f * db * db) / mc_cdf(db);
            s1 += ra + rb;
            s2 = fmaf(ra, da, fmaf(rb, db, s2));
            s3 = fmaf(GH_X[j], ra - rb, s3);
        }
        if (dmean) dmean[c] = -gs * s1 * rs;
        if (dvar) dvar[c] = vc >= MC_CLIP ? -gs * s2 * 0.5f * rs * rs : 0.f;
        gmy = fmaf(s1, rs, gmy);
        gvy = fmaf(s3, rs, gvy);
    }
    if (dmean) dmean[y] = gs * gmy;
    if (dvar) dvar[y] = 2.f * var[y] >= MC_CLIP ? gs * gvy / a : 0.f;
}

// ------------------------------------------------------------------------------------------
// The bound's reduction and the heads of its adjoint: the cores of likelihood_common.h over the coupled expectation.  A point's state is its
// clamped label; a sample has 2 C heads, skipped when neither array is asked for.  There is no trained parameter: part[B..2B) = 0.
// ------------------------------------------------------------------------------------------
struct McOps {
    static constexpr bool HAS_CONST = false;
    struct Point { int y; };
    int C; float l0, l1;
    __device__ __forceinline__ McOps(const Lik& L, int C_) : C(C_) { mc_logs(L, C, l0, l1); }
    template <int SEG, bool GRAD>
    __device__ __forceinline__ Point point(const float* Y, long long b, bool live, int) const { return {live ? mc_label(Y[b], C) : 0}; }
    __device__ __forceinline__ float expect(const Point& pt, const float* mu, const float* var, const float*, long long) const {
        float pa[10], pb[10], a;
        return mc_ve(mc_prob(mu, var, C, pt.y, pa, pb, a), l0, l1);
    }
    __device__ __forceinline__ double heads(const Point& pt, const float* mu, const float* var, const float*, long long, float wt,
                                            float* dm, float* dv, double ds) const {
        if (dm || dv) mc_heads(mu, var, C, pt.y, wt * (l1 - l0), dm, dv);
        return ds;
    }
};

template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_mc_elbo(LikReduceArgs g) {
    const McOps ops(g.lik, g.Dy);
    elbo_points<SEG, false>(g, ops);
}

__global__ __launch_bounds__(256) void k_mc_elbo_bwd(LikBwdArgs a) {
    const McOps ops(a.lik, a.Dy);
    elbo_bwd_point(a, ops);
}

// ------------------------------------------------------------------------------------------
// Elementwise callables.  MODE 0: variational_expectations, 1: predict_density (Fvar == NULL: logp) -- n = T rows, out [T];
// MODE 2: predict_mean_and_var -- n = T C elements, the rule once per candidate class, out / out2 [T, C].
// ------------------------------------------------------------------------------------------
// P_k, the predictive probability of class k of one sample (MODE 2 of k_mc_elem; its logarithm at k = the label is MODE 1; k_mc_mix)
__device__ __forceinline__ float mc_class_prob(const float* __restrict__ mu, const float* __restrict__ var, int C, int k, float eps, float eps1) {
    float pa[10], pb[10], a;
    const float p = mc_prob(mu, var, C, k, pa, pb, a);
    return fmaf(p, 1.f - eps - eps1, eps1);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_mc_elem(Lik L, const float* __restrict__ Fmu, const float* __restrict__ Fvar,
                                                 const float* __restrict__ Y, long long n, int C, long long row_div, long long row_mod,
                                                 float* __restrict__ out, float* __restrict__ out2) {
    const float eps = L.p0, eps1 = eps / (float)(C - 1);
    float l0, l1;
    mc_logs(L, C, l0, l1);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        float pa[10], pb[10], a;
        if (MODE == 2) {
            const long long t = idx / C;
            const float P = mc_class_prob(Fmu + t * C, Fvar + t * C, C, (int)(idx - t * C), eps, eps1);
            out[idx] = P; out2[idx] = P - P * P;
            continue;
        }
        const int y = mc_label(Y[(idx / row_div) % row_mod], C);
        const float* mu = Fmu + idx * C;
        if (MODE == 1 && !Fvar) {                       // logp: the FIRST maximum wins, as tf.argmax
            int best = 0;
            float fb = mu[0];
            for (int c = 1; c < C; ++c) { const float f = mu[c]; if (f > fb) { fb = f; best = c; } }
            out[idx] = best == y ? l1 : l0;
            continue;
        }
        if (MODE == 1) { out[idx] = logf(mc_class_prob(mu, Fvar + idx * C, C, y, eps, eps1)); continue; }
        out[idx] = mc_ve(mc_prob(mu, Fvar + idx * C, C, y, pa, pb, a), l0, l1);
    }
}

// ------------------------------------------------------------------------------------------
// iwvi_lik_predict_mixture: k_mc_elbo's layout (SEG lanes per point striding over its S draws, LIK_THREADS / SEG points per pass, grid-strided
// beyond MIX_MAX_BLOCKS workgroups).  The CLASSES are the outer loop: class k of every draw costs one rule, its P_k enters the two float64
// moment sums of that class, and at k = the point's label log P_k IS the draw's density -- the C probabilities of a draw are evaluated once.
// With the density alone asked for, only k = the label runs.  The log-sum-exp step is taken by every segment in every class pass (the cross-lane
// reductions stay outside divergent control flow); for a segment whose label is another class it is the exact no-op lseg_lse_step documents.
// ------------------------------------------------------------------------------------------
template <int SEG>
__global__ __launch_bounds__(LIK_THREADS) void k_mc_mix(LikMixArgs g) {
    const int tid = threadIdx.x, sl = tid % SEG, sg = tid / SEG;
    constexpr int PPP = LIK_THREADS / SEG;
    const int S = g.S, C = g.Dy;
    const float eps = g.lik.p0, eps1 = eps / (float)(C - 1);
    const int passes = g.mean ? C : 1;
    for (long long b0 = (long long)blockIdx.x * PPP; b0 < g.N; b0 += (long long)gridDim.x * PPP) {   // (uniform in the workgroup)
        const long long b = b0 + sg;
        const bool live = b < g.N;                    // uniform within a segment
        const int y = (live && g.logp) ? mc_label(g.Y[b], C) : 0;
        float m = -INFINITY;
        double ssum = 0.0;
        for (int ci = 0; ci < passes; ++ci) {
            const int k = g.mean ? ci : y;
            const bool hit = g.logp && k == y;
            double se = 0.0, se2 = 0.0;                  // sum_s P_k, sum_s ((P_k - P_k^2) + P_k^2)
            for (int s0 = 0; s0 < S; s0 += SEG) {
                const int s = s0 + sl;
                const bool on = live && s < S;
                float L = -INFINITY;
                if (on) {
                    const long long t = (b * g.stride_n + s * g.stride_s) * C;
                    const float P = mc_class_prob(g.fmean + t, g.fvar + t, C, k, eps, eps1);
                    const float V = P - P * P;
                    se += (double)P;
                    se2 += (double)V + (double)P * (double)P;
                    if (hit) L = logf(P);
                }
                if (g.logp) lseg_lse_step<SEG>(L, on && hit, m, ssum);
            }
            if (g.mean) {
                se = lseg_sum<SEG>(se);
                se2 = lseg_sum<SEG>(se2);
                if (live && sl == 0) {
                    const double mn = se / (double)S;
                    g.mean[b * C + k] = (float)mn;
                    g.var[b * C + k] = (float)(se2 / (double)S - mn * mn);
                }
            }
        }
        if (g.logp && live && sl == 0) g.logp[b] = (float)((double)m + log(ssum) - log((double)S));
    }
}

int mc_launch_elbo(const LikReduceArgs& g, hipStream_t stream) {
    return seg_dispatch(g.K, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_mc_elbo<SEG>, dim3((unsigned)lik_passes(g.B, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_mc_elbo");
    });
}

int mc_launch_mix(const LikMixArgs& g, hipStream_t stream) {
    return seg_dispatch(g.S, [&](auto seg) {
        constexpr int SEG = decltype(seg)::value;
        hipLaunchKernelGGL(k_mc_mix<SEG>, dim3(mix_blocks(g.N, SEG)), dim3(LIK_THREADS), 0, stream, g);
        return check_launch("k_mc_mix");
    });
}

int mc_launch_elbo_bwd(const LikBwdArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_mc_elbo_bwd, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
    return check_launch("k_mc_elbo_bwd");
}

int mc_launch_elem(const char* what, int mode, const Lik& L, const float* Fmu, const float* Fvar, const float* Y, long long T, int C,
                   long long row_div, long long row_mod, float* out, float* out2, hipStream_t stream) {
    const long long n = mode == 2 ? T * C : T;
    return launch_elem_mode(what, mode, n, [&](auto m, int blocks) {
        hipLaunchKernelGGL(k_mc_elem<decltype(m)::value>, dim3(blocks), dim3(256), 0, stream, L, Fmu, Fvar, Y, n, C, row_div, row_mod, out, out2);
    });
}

}  // namespace iwvi
