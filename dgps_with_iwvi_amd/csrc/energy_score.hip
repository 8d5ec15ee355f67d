// The energy score (the multivariate CRPS) of S predictive samples in D dimensions per point, one launch (iwvi_energy_score):
//   A = (1/S) sum_s |x_s - y|,   B = sum_{s<t} |x_s - x_t|,   out = A - B / S^2 (ensemble),  A - B / (S (S - 1)) (fair).
//
//   pairs     One workgroup per point walks the upper triangle s < t in tiles of T x T samples, T = blockDim.x = min(256, S rounded up to a
//             wave).  A tile of T samples x DP coordinates (DP = D rounded up to a power of two, the padding zero) is staged in LDS --
//             S D floats do not fit at S = 2000, D = 32 --; thread r keeps sample i0 + r of the row tile in DP registers (read from the
//             diagonal tile) and every lane reads column sample j from the same LDS address (a broadcast, no bank conflict).  In a
//             diagonal tile wave w starts at column 64 w + 1: everything to the left is below the diagonal for all of its rows.
//   distance  from the differences, sum_d (x_sd - x_td)^2 in float32 (one fused multiply-add per coordinate) and one correctly rounded
//             square root: NOT |x_s|^2 + |x_t|^2 - 2 x_s . x_t, which would run on the matrix cores but keeps no digit of the near pairs
//             that dominate B when the samples are tight against their offset (1e3 + 1e-3 z: the Gram form's error is ~1e6 ulp(1) ~ 0.1
//             on distances of 1e-3).
//   sums      float64 per lane over its pairs in tile order, then the wave (xor tree), then the workgroup's waves in order: fixed, no atomics.
//   NaN       a NaN coordinate is in S - 1 >= 1 distances and in A, a NaN target in A: the point's two outputs are NaN by arithmetic.
// Every loop bound is a kernel argument or the block size.
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int ES_MAX_S = 16384;
constexpr int ES_TILE = 256;                    // most samples per tile = most threads per workgroup

template <int DP>
__global__ __launch_bounds__(ES_TILE) void k_energy_score(const float* __restrict__ samples, long long sstride, long long nstride,
                                                          long long dstride, const float* __restrict__ Y, int S, int D,
                                                          float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[ES_TILE * DP];
    __shared__ __attribute__((aligned(16))) float ys[DP];
    __shared__ double red[2 * (ES_TILE / 64)];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const long long n = blockIdx.x;
    const float* src = samples + n * nstride;

    if (tid < DP) ys[tid] = tid < D ? Y[n * D + tid] : 0.f;
    double accA = 0.0, accB = 0.0;
    for (int i0 = 0; i0 < S; i0 += T) {
        const int i = i0 + tid;
        const bool row = i < S;
        float xr[DP];
        for (int j0 = i0; j0 < S; j0 += T) {
            __syncthreads();                                          // (the previous tile has been read by every wave)
            for (int e = tid; e < T * DP; e += T) {
                const int jj = e / DP, d = e % DP;                    // (DP: a power of two)
                tile[e] = (d < D && j0 + jj < S) ? src[(long long)(j0 + jj) * sstride + (long long)d * dstride] : 0.f;
            }
            __syncthreads();
            int jbeg = 0;
            if (j0 == i0) {                                           // the diagonal tile: this thread's row sample, its distance to y
                float d2 = 0.f;
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    xr[d] = tile[tid * DP + d];
                    const float df = xr[d] - ys[d];
                    d2 = fmaf(df, df, d2);
                }
                if (row) accA += (double)sqrtf(d2);
                jbeg = wave * 64 + 1;
            }
            const int jend = S - j0 < T ? S - j0 : T;
            for (int jj = jbeg; jj < jend; ++jj) {
                const float* c = tile + jj * DP;
                float d2 = 0.f;
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    const float df = xr[d] - c[d];
                    d2 = fmaf(df, df, d2);
                }
                if (row && j0 + jj > i) accB += (double)sqrtf(d2);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { accA += __shfl_xor(accA, o, 64); accB += __shfl_xor(accB, o, 64); }
    if (lane == 0) { red[2 * wave] = accA; red[2 * wave + 1] = accB; }
    __syncthreads();
    if (tid == 0) {
        double A = red[0], B = red[1];
        for (int w = 1; w < (T >> 6); ++w) { A += red[2 * w]; B += red[2 * w + 1]; }
        const double s = (double)S;
        A /= s;
        out[2 * n] = (float)(A - B / (s * s));
        out[2 * n + 1] = (float)(A - B / (s * (s - 1.0)));
    }
}

template <int DP>
static void es_launch(const float* samples, long long ss, long long ns, long long ds, const float* Y, long long N, int S, int D, float* out,
                      hipStream_t st) {
    int T = (S + 63) / 64 * 64;
    if (T > ES_TILE) T = ES_TILE;
    hipLaunchKernelGGL(k_energy_score<DP>, dim3((unsigned)N), dim3(T), 0, st, samples, ss, ns, ds, Y, S, D, out);
}

}  // namespace iwvi

extern "C" int iwvi_energy_score(const float* samples, int64_t sample_stride, int64_t point_stride, int64_t dim_stride, const float* Y,
                                 int64_t N, int S, int D, float* out, void* stream_) {
    using namespace iwvi;
    if (S < 2 || S > ES_MAX_S) { set_error("iwvi_energy_score: S=%d out of range (2..%d)", S, ES_MAX_S); return IWVI_ERR_ARG; }
    if (D < 1 || D > IWVI_MAX_P) { set_error("iwvi_energy_score: D=%d out of range (1..%d)", D, IWVI_MAX_P); return IWVI_ERR_ARG; }
    if (N < 0 || N > 0x7fffffffLL) { set_error("iwvi_energy_score: N=%lld out of range (0 .. 2^31 - 1)", (long long)N); return IWVI_ERR_ARG; }
    if (!samples || !Y || !out) { set_error("iwvi_energy_score: null samples, Y or out"); return IWVI_ERR_ARG; }
    if (sample_stride <= 0 || point_stride <= 0 || dim_stride <= 0) {
        set_error("iwvi_energy_score: strides %lld / %lld / %lld must be positive", (long long)sample_stride, (long long)point_stride, (long long)dim_stride);
        return IWVI_ERR_ARG;
    }
    if (N == 0) return IWVI_OK;
    hipStream_t st = (hipStream_t)stream_;
    const long long ss = sample_stride, ns = point_stride, ds = dim_stride;
    if (D <= 1) es_launch<1>(samples, ss, ns, ds, Y, N, S, D, out, st);
    else if (D <= 2) es_launch<2>(samples, ss, ns, ds, Y, N, S, D, out, st);
    else if (D <= 4) es_launch<4>(samples, ss, ns, ds, Y, N, S, D, out, st);
    else if (D <= 8) es_launch<8>(samples, ss, ns, ds, Y, N, S, D, out, st);
    else if (D <= 16) es_launch<16>(samples, ss, ns, ds, Y, N, S, D, out, st);
    else es_launch<32>(samples, ss, ns, ds, Y, N, S, D, out, st);
    return check_launch("k_energy_score");
}
