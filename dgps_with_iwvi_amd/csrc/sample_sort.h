// One ascending sort of a point's S samples in LDS, shared by k_sample_stats (csrc/sample_stats.hip) and k_sample_scores
// (csrc/sample_scores.hip): the bitonic network, the float64 group reductions, the grouping rule and NumPy's quantile rule.
//
//   sort    P = max(64, next power of two >= S) floats per point, padded with +inf; a bitonic network.  A group of TG threads owns a
//           point; element i lives with thread i % TG, so every compare distance j < 64 pairs two lanes of ONE wave: those steps run on
//           registers through __shfl_xor (the first six merge sizes entirely, on the way in from memory; later the last six steps of a
//           merge), the distances j >= 64 go through LDS with one barrier per step.
//   groups  S <= 128: four points per 256-thread workgroup (one wave each); S <= 256: two; above that one point per workgroup, 1024
//           threads from S > 2048.
#pragma once
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int SS_MAX_S = 16384;                 // 64 KiB of sorted floats per workgroup
constexpr int SS_RED = 16 * 3;                  // doubles in front of the samples: 3 partial sums per wave of the workgroup

extern __shared__ __attribute__((aligned(16))) unsigned char ss_smem[];

__device__ __forceinline__ double ss_wsum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ double ss_wmin(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64)); return v; }

// sum (the first NV - NMIN entries) / minimum (the last NMIN) over the group's threads, left in every thread.  nwg = waves per group,
// the same for every group of the workgroup, so the barriers are uniform.  NV <= 3 (SS_RED).
template <int NV, int NMIN>
__device__ __forceinline__ void ss_group_reduce(double (&v)[NV], double* red, int gwave, int nwg, int lane) {
    static_assert(NV <= 3, "SS_RED holds three partial sums per wave");
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = k < NV - NMIN ? ss_wsum(v[k]) : ss_wmin(v[k]);
    if (nwg > 1) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) red[gwave * 3 + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = red[k];
            for (int w = 1; w < nwg; ++w) s = k < NV - NMIN ? s + red[w * 3 + k] : fmin(s, red[w * 3 + k]);
            v[k] = s;
        }
        __syncthreads();                                          // (red is free for the next reduction)
    }
}

// one compare-exchange step at distance j < 64 inside a wave: `up` = this element's merge sorts ascending
__device__ __forceinline__ float ss_step(float v, int lane, int j, bool up) {
    const float p = __shfl_xor(v, j, 64);
    return (((lane & j) == 0) == up) ? fminf(v, p) : fmaxf(v, p);
}

// ---- in: element i = load(i) (i < P; the caller pads with +inf and accumulates what it needs from the unsorted values) -> registers,
// merge sizes 2 .. 64 on the way (element i and i ^ j, j < 64, are lanes of this wave), -> LDS
template <class Load>
__device__ __forceinline__ void ss_sort_in(float* x, int P, int TG, int gtid, int lane, Load load) {
    for (int i = gtid; i < P; i += TG) {
        float v = load(i);
#pragma unroll
        for (int k2 = 2; k2 <= 64; k2 <<= 1) {
            const bool up = (i & k2) == 0;
#pragma unroll
            for (int j = k2 >> 1; j > 0; j >>= 1) v = ss_step(v, lane, j, up);
        }
        x[i] = v;
    }
    __syncthreads();
}

// ---- merge sizes 128 .. P: distances >= 64 through LDS (one barrier each), the last six in registers again
__device__ __forceinline__ void ss_sort_merge(float* x, int P, int TG, int gtid, int lane) {
    for (int k2 = 128; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j >= 64; j >>= 1) {
            for (int q = gtid; q < (P >> 1); q += TG) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const float a = x[i], b = x[i + j];
                const bool up = (i & k2) == 0;
                x[i] = up ? fminf(a, b) : fmaxf(a, b);
                x[i + j] = up ? fmaxf(a, b) : fminf(a, b);
            }
            __syncthreads();
        }
        for (int i = gtid; i < P; i += TG) {
            float v = x[i];
            const bool up = (i & k2) == 0;
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) v = ss_step(v, lane, j, up);
            x[i] = v;
        }
        __syncthreads();
    }
}

// quantile of the sorted x[0 .. S), NumPy's default rule: position p (S - 1), linear between the two neighbouring sorted values
// (p float64: 0.975 as a float32 moves the position by 4e-5 at S = 2000; values outside [0, 1] are clamped)
__device__ __forceinline__ double ss_quantile(const float* x, int S, double prob) {
    const double p = fmin(fmax(prob, 0.0), 1.0);
    const double pos = p * (double)(S - 1);
    int lo = (int)pos;
    lo = lo < S - 1 ? lo : S - 1;
    const int hi = lo + 1 < S ? lo + 1 : S - 1;
    const double a = (double)x[lo], b = (double)x[hi], t = pos - (double)lo;
    return a == b ? a : a + (b - a) * t;
}

// the launch shape of a one-sort-per-point kernel (host)
struct SsShape { int P, threads, TG, groups; size_t lds_bytes; };
static inline SsShape ss_shape(int S) {
    SsShape s;
    s.P = 64;
    while (s.P < S) s.P <<= 1;
    s.threads = s.P >= 4096 ? 1024 : 256;
    s.TG = s.P / 2 < 64 ? 64 : s.P / 2;
    if (s.TG > s.threads) s.TG = s.threads;
    s.groups = s.threads / s.TG;
    s.lds_bytes = SS_RED * sizeof(double) + (size_t)s.groups * s.P * sizeof(float);
    return s;
}

}  // namespace iwvi
