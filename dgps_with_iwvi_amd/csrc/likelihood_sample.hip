// iwvi_lik_sample_y: exact draws y ~ p(y | f), f ~ N(fmean, fvar), for every likelihood of include/iwvi_hip.h -- the producer of the
// sample sets that iwvi_sample_stats and iwvi_kde_density_grid consume.  ONE launch, elementwise over the [T, Dy] moments (MULTICLASS: one
// lane per row of C classes; HETERO_GAUSSIAN: one lane per (row, target column) of a row of 2 Dt moments), no workspace, no host synchronisation.  Definitions, loop caps and the stream: include/iwvi_hip.h, DESIGN.md section 6.
//
// Every loop has a fixed iteration cap (SMP_ROUNDS rounds per rejection sampler, SMP_INV_CAP steps of the Poisson inversion, n edges of the
// Ordinal, C classes): a lane whose rounds run out takes the conditional mean, so a wave never spins whatever the moments hold.
// Lanes of a wave leave a rejection loop at different rounds; the loop body is one Philox call, one Box-Muller pair and the test.
#include "likelihood_common.h"

namespace iwvi {

constexpr int SMP_ROUNDS = 32;                 // Marsaglia-Tsang accepts >= 95 %, PTRS >= 86 % of its rounds: exhaustion below 0.14^32 = 5e-28
constexpr float SMP_PTRS_MIN = 10.f;           // Hoermann's PTRS is derived for rates >= 10; sequential inversion below
constexpr int SMP_INV_CAP = 64;                // P(Poisson(10) > 64) < 1e-29: the inversion search never needs more steps below the switch rate
constexpr float SMP_POIS_NORMAL = 16777216.f;  // 2^24: float32 no longer holds the integers, round(rate + sqrt(rate) n) from there on
constexpr float SMP_RSQRT2 = 0.70710678118654752f;

struct LikSampleArgs {
    Lik lik;
    const float* fmean; const float* fvar; const float* z_f;
    long long T; int Dy;
    unsigned long long seed, serial; unsigned long long* serial_dev;
    float* out_y; float* out_f;
};

// the sub-stream of one element: counter = (element low, element high, round, serial low), key = (seed low, seed high ^ serial high)
struct SmpStream { uint32_t e0, e1, ser, k0, k1; };
__device__ __forceinline__ SmpStream smp_stream(long long e, unsigned long long seed, unsigned long long serial) {
    return {(uint32_t)e, (uint32_t)((unsigned long long)e >> 32), (uint32_t)serial, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(serial >> 32)};
}
__device__ __forceinline__ void smp_words(const SmpStream& s, uint32_t round, uint32_t w[4]) {
    w[0] = s.e0; w[1] = s.e1; w[2] = round; w[3] = s.ser;
    philox4x32_10(w, s.k0, s.k1);
}
// uniform on the 2^23 midpoints of (0, 1): (k + 1/2) 2^-23 is exact in float32, never 0 and never 1
__device__ __forceinline__ float smp_u23(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }
// uniform in (0, 1] with float32's own resolution towards 0: for -log u and u^(1/a)
__device__ __forceinline__ float smp_u32(uint32_t w) { return fminf(((float)w + 0.5f) * 2.3283064365386963e-10f, 1.f); }
// the two normals of words (0, 1): box_muller4's first pair
__device__ __forceinline__ void smp_normal2(const uint32_t w[4], float& n0, float& n1) {
    float u1 = ((float)w[0] + 0.5f) * 2.3283064365386963e-10f;
    const float u2 = ((float)w[1] + 0.5f) * 2.3283064365386963e-10f;
    u1 = fminf(fmaxf(u1, 1.1754944e-38f), 0.99999994f);
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    n0 = rad * __builtin_amdgcn_cosf(u2); n1 = rad * __builtin_amdgcn_sinf(u2);
}
__device__ __forceinline__ float smp_inv_probit(float f) { return 0.5f * erfcf(-f * SMP_RSQRT2) * (1.f - 2.f * LIK_JIT) + LIK_JIT; }

// G ~ Gamma(a, 1) for a >= 1 by Marsaglia-Tsang (2000), rounds round0 .. round0 + SMP_ROUNDS - 1 of the element's stream: words (0, 1) the
// normal, word 2 the uniform.  false: the rounds ran out (or a is NaN: no comparison holds) and g is untouched.
__device__ __forceinline__ bool smp_gamma_mt(const SmpStream& st, uint32_t round0, float a, float& g) {
    const float d = a - 0.33333333333f, c = 1.f / sqrtf(9.f * d);
    bool ok = false;
#pragma unroll 1
    for (int r = 0; r < SMP_ROUNDS; ++r) {
        uint32_t w[4];
        smp_words(st, round0 + (uint32_t)r, w);
        float x, unused;
        smp_normal2(w, x, unused);
        float v = fmaf(c, x, 1.f);
        v = v * v * v;
        const float u = smp_u32(w[2]), x2 = x * x;
        if (v > 0.f && (u < 1.f - 0.0331f * x2 * x2 || logf(u) < 0.5f * x2 + d * (1.f - v + logf(v)))) { g = d * v; ok = true; break; }
    }
    return ok;
}
// log G, G ~ Gamma(a, 1), any a > 0: a < 1 draws Gamma(a + 1) and adds log(u) / a (the u^(1/a) boost, in log space: nothing underflows);
// u: the boost's uniform in (0, 1]
__device__ __forceinline__ bool smp_log_gamma(const SmpStream& st, uint32_t round0, float a, float u, float& lg) {
    const bool boost = a < 1.f;
    float g = 1.f;
    const bool ok = smp_gamma_mt(st, round0, boost ? a + 1.f : a, g);
    lg = logf(g) + (boost ? logf(u) / a : 0.f);
    return ok;
}

// log k!, float64, k an integer >= 0: a table below 8, Stirling's series at x = k + 1 >= 9 above (next term 1 / (1680 x^7) < 2e-10).  The
// library's float64 lgamma took the Poisson kernel to 165 VGPRs; with this it compiles to 69.
__device__ __constant__ const double SMP_LOG_FACT[8] = {0.0, 0.0, 0.69314718055994531, 1.7917594692280550, 3.1780538303479456,
                                                        4.7874917427820460, 6.5792512120101010, 8.5251613610654143};
__device__ __forceinline__ double smp_log_factorial(double k) {
    if (k < 8.0) return SMP_LOG_FACT[(int)k];
    const double x = k + 1.0, i = 1.0 / x, i2 = i * i;
    return (x - 0.5) * log(x) - x + 0.91893853320467274 + i * (1.0 / 12.0 - i2 * (1.0 / 360.0 - i2 * (1.0 / 1260.0)));
}

// k ~ Poisson(lam), 0 <= lam < 2^24.  lam < SMP_PTRS_MIN: sequential inversion of u (at most SMP_INV_CAP steps; the search also ends where
// the terms have vanished, p < 1e-12 beyond the mode, should float32's running sum stay below u).  Above: Hoermann's PTRS (1993), rounds
// 1 .. SMP_ROUNDS: words 0, 1 the uniforms U, V; k is formed in float64 (lam + 0.43 is not exact in float32 above 2^23) and the one log-space
// test of a round that neither squeeze decides is float64 as well (k log lam and log k! are ~1e6 at lam = 1e5 and cancel).
__device__ __forceinline__ float smp_poisson(const SmpStream& st, float lam, float u) {
    if (lam < SMP_PTRS_MIN) {
        float p = expf(-lam), s = p;
        int k = 0;
#pragma unroll 1
        for (int i = 0; i < SMP_INV_CAP; ++i) {
            if (u <= s || (p < 1e-12f && (float)k > lam)) break;
            ++k;
            p *= lam / (float)k;
            s += p;
        }
        return (float)k;
    }
    const float slam = sqrtf(lam);
    const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
    const float inva = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.f);
    const double dlam = (double)lam, loglam = log(dlam);
    float y = rintf(lam);                                  // the conditional mean, rounded: what is left if the rounds run out
#pragma unroll 1
    for (int r = 1; r <= SMP_ROUNDS; ++r) {
        uint32_t w[4];
        smp_words(st, (uint32_t)r, w);
        const float U = smp_u23(w[0]) - 0.5f, V = smp_u32(w[1]);
        const float us = 0.5f - fabsf(U);                  // >= 2^-24: U is a midpoint of the 2^-23 grid
        const double kd = floor((double)((2.f * a / us + b) * U) + dlam + 0.43);
        if (us >= 0.07f && V <= vr) { y = (float)kd; break; }
        if (kd < 0.0 || (us < 0.013f && V > us)) continue;
        if (log((double)V * (double)inva / ((double)a / ((double)us * (double)us) + (double)b)) <= kd * loglam - dlam - smp_log_factorial(kd)) { y = (float)kd; break; }
    }
    return y;
}

// One element (t, d) of every type but MULTICLASS.  p0: the launch's trained scalar (variance, scale, shape), read once per lane.
template <int TYPE>
__device__ __forceinline__ void smp_element(const LikSampleArgs& g, long long e, unsigned long long serial, float p0) {
    const SmpStream st = smp_stream(e, g.seed, serial);
    uint32_t w[4];
    smp_words(st, 0u, w);                                  // round 0: words (0, 1) -> z, n; words 2, 3 -> two uniforms
    float z, n;
    smp_normal2(w, z, n);
    const float m = g.fmean[e];
    float f = m;
    if (g.fvar) f = fmaf(sqrtf(fmaxf(g.fvar[e], 0.f)), g.z_f ? g.z_f[e] : z, m);
    if (g.out_f) g.out_f[e] = f;
    float y;
    if constexpr (TYPE == IWVI_LIK_GAUSSIAN) {
        y = fmaf(sqrtf(p0), n, f);
    } else if constexpr (TYPE == IWVI_LIK_BERNOULLI_PROBIT) {
        y = smp_u23(w[2]) < smp_inv_probit(f) ? 1.f : 0.f;
    } else if constexpr (TYPE == IWVI_LIK_STUDENT_T) {
        const float h = 0.5f * g.lik.p1;                   // nu / 2
        float lg;
        y = smp_log_gamma(st, 1u, h, smp_u32(w[2]), lg) ? fmaf(p0 * n, expf(0.5f * (logf(h) - lg)), f) : f;
    } else if constexpr (TYPE == IWVI_LIK_POISSON) {
        const float lam = g.lik.p0 * expf(f);
        if (!(lam < INFINITY)) y = lam;                    // +inf stays +inf (and NaN NaN)
        else if (lam >= SMP_POIS_NORMAL) y = rintf(fmaf(sqrtf(lam), n, lam));
        else y = smp_poisson(st, lam, smp_u23(w[2]));
    } else if constexpr (TYPE == IWVI_LIK_EXPONENTIAL) {
        y = -expf(f) * logf(smp_u32(w[2]));
    } else if constexpr (TYPE == IWVI_LIK_GAMMA) {
        float lg;
        y = smp_log_gamma(st, 1u, p0, smp_u32(w[2]), lg) ? expf(f + lg) : p0 * expf(f);
    } else if constexpr (TYPE == IWVI_LIK_BETA) {
        const float mu = smp_inv_probit(f), al = mu * p0, be = p0 - al;
        float la, lb;
        const bool oka = smp_log_gamma(st, 1u, al, smp_u32(w[2]), la), okb = smp_log_gamma(st, 1u + SMP_ROUNDS, be, smp_u32(w[3]), lb);
        y = oka && okb ? 1.f / (1.f + expf(lb - la)) : mu;       // G_a / (G_a + G_b)
    } else {                                               // ORDINAL: inverse CDF over the n + 1 bins, Phi((e_j - f) / sigma) the CDF at bin j
        const float k = SMP_RSQRT2 / g.lik.p0_dev[0], u = smp_u23(w[2]);
        const int ne = (int)g.lik.p1;
        int j = 0;
        for (int i = 0; i < ne; ++i) j += 0.5f * erfcf((f - g.lik.p0_dev[1 + i]) * k) < u ? 1 : 0;
        y = (float)j;
    }
    g.out_y[e] = f != f ? f : y;                           // a NaN moment gives a NaN y
}

// MULTICLASS: one lane per row.  Class c draws its f from the sub-stream of element t C + c; the hit / miss uniforms are words 2, 3 of
// class 0's round.  The first maximum is the hit (strict >), a miss is one of the other C - 1 classes, uniformly.
__device__ __forceinline__ void smp_row_multiclass(const LikSampleArgs& g, long long t, unsigned long long serial) {
    const int C = g.Dy;
    float best = -INFINITY, u1 = 0.f, u2 = 0.f;
    int arg = 0;
    bool nan = false;
    for (int c = 0; c < C; ++c) {
        const long long e = t * C + c;
        uint32_t w[4];
        smp_words(smp_stream(e, g.seed, serial), 0u, w);
        float z, unused;
        smp_normal2(w, z, unused);
        if (c == 0) { u1 = smp_u23(w[2]); u2 = smp_u23(w[3]); }
        const float m = g.fmean[e];
        float f = m;
        if (g.fvar) f = fmaf(sqrtf(fmaxf(g.fvar[e], 0.f)), g.z_f ? g.z_f[e] : z, m);
        if (g.out_f) g.out_f[e] = f;
        nan |= f != f;
        if (f > best) { best = f; arg = c; }
    }
    int y = arg;
    if (u1 < g.lik.p0) {
        const int o = 1 + min((int)(u2 * (float)(C - 1)), C - 2);
        y = arg + o; y = y >= C ? y - C : y;
    }
    g.out_y[t] = nan ? NAN : (float)y;
}

// HETERO_GAUSSIAN: one lane per (row t, target column d), e = t Dt + d its element and sub-stream.  Round 0: words (0, 1) -> z_1 (the mean's
// normal) and eps (the target's noise), words (2, 3) -> z_2 (the log noise variance's normal).  f and g are columns d and Dt + d of the row.
__device__ __forceinline__ void smp_row_hetero(const LikSampleArgs& g, long long e, unsigned long long serial) {
    const int Dt = g.Dy / 2;
    const long long t = e / Dt;
    const int d = (int)(e - t * Dt);
    const long long jf = t * g.Dy + d, jg = jf + Dt;
    uint32_t w[4];
    smp_words(smp_stream(e, g.seed, serial), 0u, w);
    float z1, eps, z2, unused;
    smp_normal2(w, z1, eps);
    smp_normal2(w + 2, z2, unused);
    float f = g.fmean[jf], lv = g.fmean[jg];
    if (g.fvar) {
        f = fmaf(sqrtf(fmaxf(g.fvar[jf], 0.f)), g.z_f ? g.z_f[jf] : z1, f);
        lv = fmaf(sqrtf(fmaxf(g.fvar[jg], 0.f)), g.z_f ? g.z_f[jg] : z2, lv);
    }
    if (g.out_f) { g.out_f[jf] = f; g.out_f[jg] = lv; }
    const float h = fminf(fmaxf(0.5f * lv, -60.f), 60.f);    // the exponent's clip of csrc/likelihood_hetero.hip
    const float y = fmaf(expf(h), eps, f);
    g.out_y[e] = (f != f || lv != lv) ? NAN : y;            // a NaN moment gives a NaN y
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_lik_sample(LikSampleArgs g) {
    // serial_dev: the low half is the serial, the high half this launch's arrival count.  Every workgroup reads the serial before it takes
    // its ticket, so before the last one advances it.
    unsigned long long serial = g.serial;
    if (g.serial_dev) serial = __hip_atomic_load(g.serial_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xffffffffULL;
    const long long n = TYPE == IWVI_LIK_MULTICLASS ? g.T : TYPE == IWVI_LIK_HETERO_GAUSSIAN ? g.T * (g.Dy / 2) : g.T * g.Dy;
    float p0 = g.lik.p0;
    if (TYPE != IWVI_LIK_ORDINAL && g.lik.p0_dev) p0 = *g.lik.p0_dev;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        if constexpr (TYPE == IWVI_LIK_MULTICLASS) smp_row_multiclass(g, e, serial);
        else if constexpr (TYPE == IWVI_LIK_HETERO_GAUSSIAN) smp_row_hetero(g, e, serial);
        else smp_element<TYPE>(g, e, serial, p0);
    }
    if (g.serial_dev) {
        // the last workgroup of THIS launch to get here (k_fill_normal's ticket, kept in the word's high half) clears the count and adds one
        // to the serial in a single atomic: a replayed graph draws fresh values
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long t = __hip_atomic_fetch_add(g.serial_dev, 1ULL << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((t >> 32) == (unsigned long long)gridDim.x - 1)
                __hip_atomic_fetch_add(g.serial_dev, 1ULL - ((unsigned long long)gridDim.x << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int TYPE>
static int smp_launch(const LikSampleArgs& g, long long n, hipStream_t stream) {
    hipLaunchKernelGGL(k_lik_sample<TYPE>, dim3(elem_blocks(n)), dim3(256), 0, stream, g);
    return check_launch("k_lik_sample");
}

}  // namespace iwvi

using namespace iwvi;

extern "C" int iwvi_lik_sample_y(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, int64_t T, int Dy, const float* z_f,
                                 uint64_t seed, uint64_t serial, uint64_t* serial_dev, float* out_y, float* out_f, void* stream_) {
    const char* what = "iwvi_lik_sample_y";
    hipStream_t stream = (hipStream_t)stream_;
    LikSampleArgs g{};
    int rc;
    if ((rc = take_lik(lik, g.lik, what)) != IWVI_OK) return rc;
    if (T < 0) { set_error("%s: T = %lld", what, (long long)T); return IWVI_ERR_ARG; }
    if (g.lik.type == IWVI_LIK_HETERO_GAUSSIAN && (rc = hg_check_dim(Dy, what)) != IWVI_OK) return rc;
    if (Dy < 1 || Dy > IWVI_MAX_P) { set_error("%s: Dy = %d outside 1..%d", what, Dy, IWVI_MAX_P); return IWVI_ERR_ARG; }
    if (g.lik.type == IWVI_LIK_MULTICLASS && (rc = mc_check_classes(g.lik, Dy, what)) != IWVI_OK) return rc;
    if (!out_y) { set_error("%s: null out_y", what); return IWVI_ERR_ARG; }
    if (T == 0) return IWVI_OK;
    if (!fmean) { set_error("%s: null fmean", what); return IWVI_ERR_ARG; }
    g.fmean = fmean; g.fvar = fvar; g.z_f = z_f; g.T = T; g.Dy = Dy;
    g.seed = seed; g.serial = serial; g.serial_dev = (unsigned long long*)serial_dev;
    g.out_y = out_y; g.out_f = out_f;
    const long long n = (long long)T * Dy;
    switch (g.lik.type) {
        case IWVI_LIK_GAUSSIAN: return smp_launch<IWVI_LIK_GAUSSIAN>(g, n, stream);
        case IWVI_LIK_BERNOULLI_PROBIT: return smp_launch<IWVI_LIK_BERNOULLI_PROBIT>(g, n, stream);
        case IWVI_LIK_STUDENT_T: return smp_launch<IWVI_LIK_STUDENT_T>(g, n, stream);
        case IWVI_LIK_MULTICLASS: return smp_launch<IWVI_LIK_MULTICLASS>(g, (long long)T, stream);
        case IWVI_LIK_POISSON: return smp_launch<IWVI_LIK_POISSON>(g, n, stream);
        case IWVI_LIK_EXPONENTIAL: return smp_launch<IWVI_LIK_EXPONENTIAL>(g, n, stream);
        case IWVI_LIK_GAMMA: return smp_launch<IWVI_LIK_GAMMA>(g, n, stream);
        case IWVI_LIK_BETA: return smp_launch<IWVI_LIK_BETA>(g, n, stream);
        case IWVI_LIK_HETERO_GAUSSIAN: return smp_launch<IWVI_LIK_HETERO_GAUSSIAN>(g, (long long)T * (Dy / 2), stream);
        default: return smp_launch<IWVI_LIK_ORDINAL>(g, n, stream);      // (take_lik has refused every other value)
    }
}
