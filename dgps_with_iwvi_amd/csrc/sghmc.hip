// The SGHMC inference mode (reference experiments/sghmc.py, adapted there from cambridge-mlg/sghmc_dgp): the sampler's update of every
// sampled tensor in ONE launch, and the negative log prior of a whitened q_mu that replaces KL[q(u) || p(u)] for a layer without q_sqrt
// (dgps_with_iwvi/temp_workaround.py:167-184).  Public ABI: include/iwvi_hip.h (iwvi_sghmc_step, iwvi_neg_log_prior).
#include "iwvi_common.h"
#include <math.h>

namespace iwvi {

constexpr int SGHMC_MAX = IWVI_SGHMC_MAX_TENSORS;
struct SghmcTensor {
    float* theta; const float* grad; double* xi; double* g; double* g2; double* p; double* master;
    const float* noise; float* noise_out; long long n; unsigned long long ctr_off;     // ctr_off: Philox counters the drawing tensors in front of this one take
};
struct SghmcArgs {
    SghmcTensor t[SGHMC_MAX];
    double eps2, mdecay, nscale;                                 // epsilon^2 | mdecay | 2 (epsilon / sqrt(num_data))^2 mdecay
    unsigned long long seed; unsigned long long* state; unsigned long long nq_drawn;
    int burn_in;
};

// One thread per group of four consecutive elements (one Philox counter: the layout of k_fill_normal, csrc/lv_elbo.hip), grid.y = tensor.
// Every right-hand side reads the values from before the step (sghmc.py:33-48); float64 throughout, without contraction, so that each line is
// the rounding of the operation it names; theta is stored as the float32 rounding of its float64 master.
__global__ __launch_bounds__(256) void k_sghmc_step(SghmcArgs a) {
#pragma clang fp contract(off)
    const SghmcTensor& T = a.t[blockIdx.y];
    const bool draw = T.noise == nullptr;
    unsigned long long base = 0;
    if (a.state) base = a.state[0];                              // every block reads the counter before it takes its ticket (as k_fill_normal does)
    const long long nq = (T.n + 3) / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (draw) {
            const uint64_t ctr = base + T.ctr_off + (uint64_t)q;
            uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
            philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            box_muller4(c, nz);
        }
        for (int e = 0; e < 4; ++e) {
            const long long i = 4 * q + e;
            if (i >= T.n) break;
            if (!draw) nz[e] = T.noise[i];
            if (T.noise_out) T.noise_out[i] = nz[e];
            const double grad = -(double)T.grad[i];              // `grad` holds d bound / d theta; the sampler descends nll = -bound
            const double xi = T.xi[i], g = T.g[i], g2 = T.g2[i], p = T.p[i];
            const double Minv = 1.0 / (sqrt(g2 + 1e-16) + 1e-16);
            const double sigma = sqrt(fmax(a.nscale * Minv, 1e-16));
            const double p1 = p - a.eps2 * Minv * grad - a.mdecay * p + sigma * (double)nz[e];
            const double th = T.master[i] + p1;
            if (a.burn_in) {
                const double r = 1.0 / (xi + 1.0);
                T.g[i] = (1.0 - r) * g + r * grad;
                T.g2[i] = (1.0 - r) * g2 + r * (grad * grad);
                T.xi[i] = 1.0 + xi * (1.0 - g * g / (g2 + 1e-16));
            }
            T.p[i] = p1;
            T.master[i] = th;
            T.theta[i] = (float)th;
        }
    }
    if (a.state) {
        // the last block of the whole grid to arrive re-zeroes the ticket and advances the counter by what this launch drew
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
            const unsigned long long t = __hip_atomic_fetch_add(&a.state[1], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == total - 1) {
                __hip_atomic_store(&a.state[1], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&a.state[0], a.nq_drawn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// -log N(q_mu; 0, I) summed over all M R entries (temp_workaround.py:177-184 with q_sqrt None, whitened): 1/2 |q_mu|_F^2 + 1/2 M R log 2 pi
__global__ __launch_bounds__(256) void k_neg_log_prior(const float* q_mu, long long n, double* out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) { const double v = (double)q_mu[i]; s += v * v; }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = 0.5 * red[0] + 0.5 * (double)n * 1.8378770664093453;   // log 2 pi
}

}  // namespace iwvi

using namespace iwvi;

extern "C" int iwvi_sghmc_step(const iwvi_sghmc_tensor* tensors, int n_tensors, double epsilon, double mdecay, double num_data,
                               int burn_in, uint64_t seed, uint64_t* rng_state, void* stream_) {
    if (!tensors || n_tensors <= 0 || n_tensors > SGHMC_MAX) { set_error("iwvi_sghmc_step: bad argument (1 to %d tensors)", SGHMC_MAX); return IWVI_ERR_ARG; }
    if (!(epsilon > 0.0) || !(mdecay >= 0.0) || !(num_data > 0.0) || !isfinite(epsilon) || !isfinite(mdecay) || !isfinite(num_data)) {
        set_error("iwvi_sghmc_step: epsilon > 0, mdecay >= 0 and num_data > 0 (finite) expected, got %g, %g, %g", epsilon, mdecay, num_data);
        return IWVI_ERR_ARG;
    }
    SghmcArgs a{};
    long long nqmax = 1;
    unsigned long long drawn = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const iwvi_sghmc_tensor& s = tensors[i];
        if (!s.theta || !s.grad || !s.xi || !s.g || !s.g2 || !s.p || !s.theta64 || s.n <= 0) { set_error("iwvi_sghmc_step: bad tensor %d", i); return IWVI_ERR_ARG; }
        const long long nq = ((long long)s.n + 3) / 4;
        a.t[i] = SghmcTensor{s.theta, s.grad, s.xi, s.g, s.g2, s.p, s.theta64, s.noise, s.noise_out, (long long)s.n, drawn};
        if (!s.noise) drawn += (unsigned long long)nq;
        if (nq > nqmax) nqmax = nq;
    }
    if (drawn && !rng_state) { set_error("iwvi_sghmc_step: a tensor without injected noise needs rng_state"); return IWVI_ERR_ARG; }
    const double eps_s = epsilon / sqrt(num_data);
    a.eps2 = epsilon * epsilon; a.mdecay = mdecay; a.nscale = 2.0 * (eps_s * eps_s) * mdecay;
    a.seed = seed; a.state = drawn ? (unsigned long long*)rng_state : nullptr; a.nq_drawn = drawn; a.burn_in = burn_in ? 1 : 0;
    long long blocks = (nqmax + 255) / 256; if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_sghmc_step, dim3((unsigned)blocks, n_tensors), dim3(256), 0, (hipStream_t)stream_, a);
    return check_launch("k_sghmc_step");
}

extern "C" int iwvi_neg_log_prior(const float* q_mu, int M, int R, double* out, void* stream_) {
    if (!q_mu || !out || M <= 0 || R <= 0 || M > IWVI_MAX_M || R > IWVI_MAX_R) { set_error("iwvi_neg_log_prior: bad argument (q_mu [M <= %d, R <= %d], out)", IWVI_MAX_M, IWVI_MAX_R); return IWVI_ERR_ARG; }
    hipLaunchKernelGGL(k_neg_log_prior, dim3(1), dim3(256), 0, (hipStream_t)stream_, q_mu, (long long)M * R, out);
    return check_launch("k_neg_log_prior");
}
