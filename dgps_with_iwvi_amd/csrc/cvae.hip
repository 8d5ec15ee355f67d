// The CVAE baseline (reference experiments/build_models.py:29-142): an MLP encoder and an MLP decoder in float32 without skip connections, a
// clipped log-variance head, a decoder fed [z, x], a Gaussian log density and an analytic KL.  Public ABI: include/iwvi_hip.h (iwvi_cvae_*).
//
// k_cvae_rows   eight rows per workgroup: encoder -> clip -> sample -> decoder -> per-row log p and KL -> (GRAD) the deltas of every map.  The
//               activations of a tile live in LDS; a map's weights are staged in LDS once per use (transposed for the backward, so that both
//               directions read them without bank conflicts), the next map's weights travelling in registers meanwhile.
// k_cvae_wgrad  dW = A^T Delta and db of every map, one 8 x 8 tile per workgroup, four row segments summed in a fixed order; its last
//               workgroup adds the per-tile (log p, KL, d variance) partials in float64 in a fixed order and advances the noise counter.
// k_cvae_finish that last workgroup alone (the value entry).
// k_cvae_sample 16 (point, sample) rows per wave through the decoder on the exact-f32 matrix cores, activations in registers; one launch.
// No float atomics anywhere: the same inputs give the same bits.
#include "iwvi_common.h"
#include <math.h>

namespace iwvi {

constexpr int CV_MAPS = IWVI_CVAE_MAX_MAPS, CV_W = IWVI_CVAE_MAX_WIDTH;
constexpr int CV_TR = 8, CV_NT = 512, CV_RPT = CV_TR / (CV_NT / CV_W);      // row launch: rows per workgroup, threads, rows per thread
constexpr int CV_SNT = 256, CV_STR = 16 * (CV_SNT / 64);                     // sampler: four waves of 16 rows per pass
constexpr int CV_WBUF = CV_W * (CV_W + 1);                                  // a map's weights, transposed with an odd row stride
constexpr int CV_SLAB = CV_W * CV_TR;                                       // one activation slab of the row launch: [width][row]
constexpr int CV_ROWS_LDS = (CV_WBUF + 10 * CV_SLAB + 2 * IWVI_CVAE_MAX_L * CV_TR + 5 * 8 * CV_TR) * (int)sizeof(float);
constexpr int CV_SAMPLE_LDS_MAX = 152 * 1024;                               // the sampler's weights stay resident in LDS up to this
#define CV_CLIP_LO (-27.631021115928547f)   /* ln 1e-12 */
#define CV_CLIP_HI 23.025850929940457f      /* ln 1e10  */

struct CvNet { const float* W[CV_MAPS]; const float* b[CV_MAPS]; int dims[CV_MAPS + 1]; };
struct CvRowArgs {
    CvNet enc, dec;
    int n, Dx, Dy, L, act;
    float variance; const float* variance_dev;
    const float* X; const float* Y; long long B;
    const float* eps; float* eps_out; unsigned long long seed; const unsigned long long* state;
    float* A[2 * CV_MAPS]; float* D[2 * CV_MAPS];     // workspace, per map (encoder 0 .. n-1, decoder n .. 2n-1): inputs [B, in], deltas [B, out]
    double* part;                                      // [tiles, 3] = (sum log p, sum KL, d elbo / d variance) of a tile
};
struct CvGradArgs {
    const float* A[2 * CV_MAPS]; const float* D[2 * CV_MAPS]; float* dW[2 * CV_MAPS]; float* db[2 * CV_MAPS];
    int in[2 * CV_MAPS], out[2 * CV_MAPS], tile0[2 * CV_MAPS + 1];
    int nl; long long B;
    const double* part; long long nparts; double* out3; double* dvar;
    unsigned long long* state; unsigned long long advance;
};
struct CvSampleArgs {
    CvNet dec;
    int n, Dx, Dy, L, act, resident, no_y_noise;
    int woff[CV_MAPS]; long long ntiles;
    float variance; const float* variance_dev;
    const float* X; long long T, S;
    const float* z; const float* zy; unsigned long long seed; unsigned long long* state; unsigned long long nqz, nqy;
    float* out;
};

// element e of the stream iwvi_fill_normal(out, n, seed, ctr0) writes
__device__ __forceinline__ float cv_draw(unsigned long long seed, unsigned long long ctr0, unsigned long long e) {
    const uint64_t ctr = ctr0 + (e >> 2);
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float v[4];
    box_muller4(c, v);
    const int s = (int)(e & 3);
    return s == 0 ? v[0] : s == 1 ? v[1] : s == 2 ? v[2] : v[3];
}

// ---- a map's weights: global -> registers -> LDS (W is [in, out] row-major, n = in * out <= 128 * 128) ----
template <int NT>
__device__ __forceinline__ void w_load(float (&pre)[CV_W * CV_W / NT], const float* W, int n) {
#pragma unroll
    for (int m = 0; m < CV_W * CV_W / NT; ++m) {
        const int i = (int)threadIdx.x + NT * m;
        pre[m] = i < n ? W[i] : 0.f;
    }
}
// TRANS = false: buf[k * out + j] (the forward: lanes over j);  true: buf[j * (in | 1) + k] (the backward: lanes over k; the odd stride keeps
// these stores, whose lanes run over j, off one bank)
template <int NT, bool TRANS>
__device__ __forceinline__ void w_store(const float (&pre)[CV_W * CV_W / NT], float* buf, int in, int out) {
    const int n = in * out;
    if (!TRANS) {
#pragma unroll
        for (int m = 0; m < CV_W * CV_W / NT; ++m) {
            const int i = (int)threadIdx.x + NT * m;
            if (i < n) buf[i] = pre[m];
        }
    } else {
        const int ldt = in | 1, q = NT / out, r = NT % out;
        int k = (int)threadIdx.x / out, j = (int)threadIdx.x % out;
#pragma unroll
        for (int m = 0; m < CV_W * CV_W / NT; ++m) {
            const int i = (int)threadIdx.x + NT * m;
            if (i < n) buf[j * ldt + k] = pre[m];
            k += q; j += r;
            if (j >= out) { j -= out; ++k; }
        }
    }
}

// aout[j][r] = f(b[j] + sum_k ain[k][r] W[k][j]) for the TR = RPT * NT / 128 rows of a tile; slabs are [width][TR].  Thread (j = tid & 127,
// tid >> 7) owns RPT = 2 consecutive rows of column j.  gout (optional): the same values as rows of a [B, out] array, rows row0 .. < B.
template <int NT, int RPT>
__device__ __forceinline__ void fwd_compute(const float* wbuf, const float* bias, const float* ain, float* aout, int in, int out, int act,
                                            bool last, float* gout, long long row0, long long B) {
    constexpr int TR = RPT * (NT / CV_W);
    static_assert(RPT == 2, "two rows per thread");
    const int j = threadIdx.x & (CV_W - 1), r0 = ((int)threadIdx.x >> 7) * RPT;
    if (j >= out) return;
    float acc[RPT];
    const float bj = bias[j];
#pragma unroll
    for (int r = 0; r < RPT; ++r) acc[r] = bj;
#pragma unroll 4
    for (int k = 0; k < in; ++k) {
        const float w = wbuf[k * out + j];
        const float2 v = *(const float2*)(ain + k * TR + r0);
        acc[0] = fmaf(v.x, w, acc[0]); acc[1] = fmaf(v.y, w, acc[1]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const float v = last ? acc[r] : enc_act(acc[r], act);
        aout[j * TR + r0 + r] = v;
        if (gout && row0 + r0 + r < B) gout[(row0 + r0 + r) * out + j] = v;
    }
}

// din[k][r] = (sum_j dout[j][r] W[k][j]) act'(ain[k][r]) for k < kmax, from the transposed weights; ain = the post-activation values the map
// read (NULL: the map read raw inputs, no activation in front).  gout (optional): rows of the [B, in] delta array of the map below.
template <int NT, int RPT>
__device__ __forceinline__ void bwd_compute(const float* wt, const float* dout, const float* ain, float* din, int in, int out, int kmax,
                                            int act, float* gout, long long row0, long long B) {
    constexpr int TR = RPT * (NT / CV_W);
    static_assert(RPT == 2, "the backward runs in the row launch only");
    const int k = threadIdx.x & (CV_W - 1), r0 = ((int)threadIdx.x >> 7) * RPT;
    if (k >= kmax) return;
    const int ldt = in | 1;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
    for (int j = 0; j < out; ++j) {
        const float w = wt[j * ldt + k];
        const float2 v = *(const float2*)(dout + j * TR + r0);
        a0 = fmaf(v.x, w, a0); a1 = fmaf(v.y, w, a1);
    }
    if (ain) { a0 *= enc_act_grad(ain[k * TR + r0], act); a1 *= enc_act_grad(ain[k * TR + r0 + 1], act); }
    din[k * TR + r0] = a0; din[k * TR + r0 + 1] = a1;
    if (gout) {
        if (row0 + r0 < B) gout[(row0 + r0) * in + k] = a0;
        if (row0 + r0 + 1 < B) gout[(row0 + r0 + 1) * in + k] = a1;
    }
}

template <bool GRAD>
__global__ __launch_bounds__(CV_NT) void k_cvae_rows(CvRowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cvsm[];
    constexpr int TR = CV_TR, NT = CV_NT, RPT = CV_RPT, SL = CV_SLAB, LM = IWVI_CVAE_MAX_L;
    float* wbuf = cvsm;
    float* xy = wbuf + CV_WBUF;          // encoder input [x, y]
    float* eh = xy + SL;                 // encoder hidden activations, 3 slabs
    float* zx = eh + 3 * SL;             // decoder input [z, x]
    float* dh = zx + SL;                 // decoder hidden activations, 3 slabs
    float* dc = dh + 3 * SL;             // delta ping-pong
    float* dn = dc + SL;
    float* eo = dn + SL;                 // encoder output (means | raw) [2 L][TR]
    float* epss = eo + 2 * LM * TR;      // [L][TR] the draws, then sigma, KL per entry, ...
    float* sigs = epss + 8 * TR;
    float* klv = sigs + 8 * TR;
    float* lpv = klv + 8 * TR;           // [Dy][TR]
    float* dvv = lpv + 8 * TR;
    float* yo = dc;                      // decoder output [Dy][TR]: read by the loss head only, which then writes the first delta over it

    const int tid = threadIdx.x, n = a.n, L = a.L, Dx = a.Dx, Dy = a.Dy, act = a.act;
    const long long row0 = (long long)blockIdx.x * TR, B = a.B;
    const int in0 = a.enc.dims[0], dz0 = a.dec.dims[0];
    float pre[CV_W * CV_W / NT];
    w_load<NT>(pre, a.enc.W[0], in0 * a.enc.dims[1]);

    // inputs: [x, y] for the encoder, the x part of [z, x] for the decoder, the draws
    for (int idx = tid; idx < TR * in0; idx += NT) {
        const int r = idx / in0, k = idx - r * in0;
        const long long row = row0 + r;
        float v = 0.f;
        if (row < B) v = k < Dx ? a.X[row * Dx + k] : a.Y[row * Dy + (k - Dx)];
        xy[k * TR + r] = v;
        if (k < Dx) zx[(L + k) * TR + r] = v;
        if (GRAD && row < B) a.A[0][row * in0 + k] = v;
    }
    if (tid < TR * L) {
        const int r = tid / L, j = tid - r * L;
        const long long row = row0 + r;
        float v = 0.f;
        if (row < B) {
            const unsigned long long e = (unsigned long long)row * L + j;
            v = a.eps ? a.eps[e] : cv_draw(a.seed, a.state[0], e);
            if (a.eps_out) a.eps_out[e] = v;
        }
        epss[j * TR + r] = v;
    }

    // encoder
    for (int l = 0; l < n; ++l) {
        const int in = a.enc.dims[l], out = a.enc.dims[l + 1];
        w_store<NT, false>(pre, wbuf, in, out);
        __syncthreads();
        if (l + 1 < n) w_load<NT>(pre, a.enc.W[l + 1], out * a.enc.dims[l + 2]);
        else w_load<NT>(pre, a.dec.W[0], dz0 * a.dec.dims[1]);
        const bool last = l == n - 1;
        fwd_compute<NT, RPT>(wbuf, a.enc.b[l], l == 0 ? xy : eh + (l - 1) * SL, last ? eo : eh + l * SL, in, out, act, last,
                             GRAD && !last ? a.A[l + 1] : nullptr, row0, B);
        __syncthreads();
    }
    // clip, sample, KL
    if (tid < TR * L) {
        const int r = tid / L, j = tid - r * L;
        const float mu = eo[j * TR + r], raw = eo[(L + j) * TR + r];
        const float rc = fminf(fmaxf(raw, CV_CLIP_LO), CV_CLIP_HI);
        const float sg = expf(0.5f * rc);
        const bool live = row0 + r < B;
        zx[j * TR + r] = live ? fmaf(epss[j * TR + r], sg, mu) : 0.f;
        sigs[j * TR + r] = sg;
        klv[j * TR + r] = live ? 0.5f * (sg * sg + mu * mu - 1.f - rc) : 0.f;
    }
    __syncthreads();
    if (GRAD) {
        for (int idx = tid; idx < TR * dz0; idx += NT) {
            const int r = idx / dz0, k = idx - r * dz0;
            if (row0 + r < B) a.A[n][(row0 + r) * dz0 + k] = zx[k * TR + r];
        }
    }
    // decoder
    for (int l = 0; l < n; ++l) {
        const int in = a.dec.dims[l], out = a.dec.dims[l + 1];
        w_store<NT, false>(pre, wbuf, in, out);
        __syncthreads();
        if (l + 1 < n) w_load<NT>(pre, a.dec.W[l + 1], out * a.dec.dims[l + 2]);
        else if (GRAD) w_load<NT>(pre, a.dec.W[n - 1], in * out);
        const bool last = l == n - 1;
        fwd_compute<NT, RPT>(wbuf, a.dec.b[l], l == 0 ? zx : dh + (l - 1) * SL, last ? yo : dh + l * SL, in, out, act, last,
                             GRAD && !last ? a.A[n + l + 1] : nullptr, row0, B);
        __syncthreads();
    }
    // log density and its head
    const float var = a.variance_dev ? a.variance_dev[0] : a.variance;
    if (tid < TR * Dy) {
        const int r = tid / Dy, d = tid - r * Dy;
        const long long row = row0 + r;
        float lp = 0.f, dl = 0.f, dv = 0.f;
        if (row < B) {
            const float e = a.Y[row * Dy + d] - yo[d * TR + r];
            const float iv = 1.f / var;
            lp = -0.9189385332046727f - 0.5f * logf(var) - 0.5f * e * e * iv;
            dl = e * iv;
            dv = 0.5f * iv * (e * e * iv - 1.f);
            if (GRAD) a.D[2 * n - 1][row * Dy + d] = dl;
        }
        lpv[d * TR + r] = lp; dvv[d * TR + r] = dv;
        dc[d * TR + r] = dl;             // over yo: this thread was the only reader of that entry
    }
    __syncthreads();
    if (tid == 0) {                      // fixed order, float64
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < Dy * TR; ++i) { s0 += (double)lpv[i]; s2 += (double)dvv[i]; }
        for (int i = 0; i < L * TR; ++i) s1 += (double)klv[i];
        a.part[3 * (long long)blockIdx.x] = s0; a.part[3 * (long long)blockIdx.x + 1] = s1; a.part[3 * (long long)blockIdx.x + 2] = s2;
    }
    if (!GRAD) return;

    // decoder backward
    for (int l = n - 1; l >= 0; --l) {
        const int in = a.dec.dims[l], out = a.dec.dims[l + 1];
        w_store<NT, true>(pre, wbuf, in, out);
        __syncthreads();
        if (l > 0) w_load<NT>(pre, a.dec.W[l - 1], a.dec.dims[l - 1] * in);
        else if (n > 1) w_load<NT>(pre, a.enc.W[n - 1], a.enc.dims[n - 1] * a.enc.dims[n]);
        bwd_compute<NT, RPT>(wbuf, dc, l > 0 ? dh + (l - 1) * SL : nullptr, dn, in, out, l > 0 ? in : L, act,
                             l > 0 ? a.D[n + l - 1] : nullptr, row0, B);
        __syncthreads();
        float* t = dc; dc = dn; dn = t;
    }
    // latent backward: dc holds d elbo / d z through the decoder
    if (tid < TR * L) {
        const int r = tid / L, j = tid - r * L;
        const long long row = row0 + r;
        float dmu = 0.f, draw = 0.f;
        if (row < B) {
            const float dz = dc[j * TR + r], mu = eo[j * TR + r], raw = eo[(L + j) * TR + r], sg = sigs[j * TR + r];
            dmu = dz - mu;
            if (raw >= CV_CLIP_LO && raw <= CV_CLIP_HI) draw = 0.5f * (dz * epss[j * TR + r] * sg - (sg * sg - 1.f));
            a.D[n - 1][row * 2 * L + j] = dmu;
            a.D[n - 1][row * 2 * L + L + j] = draw;
        }
        dn[j * TR + r] = dmu; dn[(L + j) * TR + r] = draw;
    }
    __syncthreads();
    { float* t = dc; dc = dn; dn = t; }
    // encoder backward (the first map needs no input delta)
    for (int l = n - 1; l >= 1; --l) {
        const int in = a.enc.dims[l], out = a.enc.dims[l + 1];
        w_store<NT, true>(pre, wbuf, in, out);
        __syncthreads();
        if (l > 1) w_load<NT>(pre, a.enc.W[l - 1], a.enc.dims[l - 1] * in);
        bwd_compute<NT, RPT>(wbuf, dc, eh + (l - 1) * SL, dn, in, out, in, act, a.D[l - 1], row0, B);
        __syncthreads();
        float* t = dc; dc = dn; dn = t;
    }
}

// the per-tile partials in a fixed order (256 threads), float64; then the noise counter
__device__ __forceinline__ void cv_finish(const double* part, long long nparts, double* out3, double* dvar, unsigned long long* state,
                                          unsigned long long advance, double (*red)[256]) {
    const int t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long i = t; i < nparts; i += 256) { s0 += part[3 * i]; s1 += part[3 * i + 1]; s2 += part[3 * i + 2]; }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        out3[0] = red[0][0] - red[1][0]; out3[1] = red[0][0]; out3[2] = red[1][0];
        if (dvar) dvar[0] = red[2][0];
        if (state && advance) __hip_atomic_fetch_add(&state[0], advance, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_cvae_finish(const double* part, long long nparts, double* out3, unsigned long long* state,
                                                     unsigned long long advance) {
    __shared__ double red[3][256];
    cv_finish(part, nparts, out3, nullptr, state, advance, red);
}

// dW[k][j] = sum_r A[r][k] Delta[r][j], db[j] = sum_r Delta[r][j] (the row k == in of the tiling).  256 threads = 8 x 8 entries x 4 row segments.
__global__ __launch_bounds__(256) void k_cvae_wgrad(CvGradArgs a) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    if (blk >= a.tile0[a.nl]) { cv_finish(a.part, a.nparts, a.out3, a.dvar, a.state, a.advance, red); return; }
    int l = 0;
    while (l + 1 < a.nl && blk >= a.tile0[l + 1]) ++l;
    const int in = a.in[l], out = a.out[l], tt = blk - a.tile0[l];
    const int tj = (out + 7) / 8;
    const int k = (tt / tj) * 8 + ((tid & 63) >> 3), j = (tt % tj) * 8 + (tid & 7), seg = tid >> 6;
    const long long rps = (a.B + 3) / 4;
    const long long rlo = seg * rps, rhi = rlo + rps < a.B ? rlo + rps : a.B;
    const bool live = k <= in && j < out;
    float acc = 0.f;
    if (live) {
        const float* D = a.D[l] + j;
        if (k < in) {
            const float* A = a.A[l] + k;
#pragma unroll 8
            for (long long r = rlo; r < rhi; ++r) acc = fmaf(A[r * in], D[r * out], acc);
        } else {
#pragma unroll 8
            for (long long r = rlo; r < rhi; ++r) acc += D[r * out];
        }
    }
    float* redf = (float*)&red[0][0];
    redf[tid] = acc;
    __syncthreads();
    if (seg == 0 && live) {
        const float s = (redf[tid] + redf[tid + 64]) + (redf[tid + 128] + redf[tid + 192]);
        if (k < in) a.dW[l][k * out + j] = s; else a.db[l][j] = s;
    }
}

// 64 rows t = n S + s per workgroup pass, 16 per wave, through the decoder on the exact-f32 matrix cores; out[t, d] = decoder(z_t, x_n)_d +
// sqrt(variance) z_y[t, d].  A hidden map is computed TRANSPOSED, out^T [out, 16] = W^T [out, in] act^T [in, 16], with v_mfma_f32_16x16x4_f32:
// the A operand of lane (g = lane >> 4, j = lane & 15) is W[k][16 jb + j], the B operand of lane (g, i) is act[k][sample i], and the result
// tile jb leaves lane (g, i) holding out columns 16 jb + 4 g + r (r = 0 .. 3) of sample i.  With MFMA step s of chunk c contracting
// k = 16 c + 4 g + s, register s of result tile c IS the next map's B operand: a wave's activations never leave its registers.  The last
// map (Dy <= 8 columns) is plain FMAs over the lane's own k and two cross-lane adds.  Weights sit in LDS, zero-padded to multiples of 16
// with a row stride = 4 (mod 16) words (the four g groups of an A-operand read then fall on four different bank quarters); all maps stay
// resident while a workgroup strides over its tiles when they fit, else each map is staged per tile.
typedef float cv_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void cv_stage(float* dst, const float* W, int in, int out) {
    const int inp = round_up(in, 16), outp = round_up(out, 16), ld = outp + 4;
    for (int idx = threadIdx.x; idx < inp * outp; idx += CV_SNT) {
        const int k = idx / outp, j = idx - k * outp;
        dst[k * ld + j] = (k < in && j < out) ? W[k * out + j] : 0.f;
    }
}

__global__ __launch_bounds__(CV_SNT, 2) void k_cvae_sample(CvSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cvss[];
    constexpr int NT8 = CV_W / 16;
    float* bbuf = cvss;                       // [map][128] biases, zero beyond the width
    float* wb = cvss + CV_MAPS * CV_W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int n = a.n, L = a.L, Dx = a.Dx, Dy = a.Dy, w0 = a.dec.dims[0];
    const long long T = a.T;
    const unsigned long long ctr = a.state ? a.state[0] : 0ULL;   // every block reads the counter before it takes its ticket
    for (int idx = tid; idx < n * CV_W; idx += CV_SNT) {
        const int l = idx >> 7, j = idx & (CV_W - 1);
        bbuf[idx] = j < a.dec.dims[l + 1] ? a.dec.b[l][j] : 0.f;
    }
    if (a.resident)
        for (int l = 0; l < n; ++l) cv_stage(wb + a.woff[l], a.dec.W[l], a.dec.dims[l], a.dec.dims[l + 1]);
    __syncthreads();
    const float sd = sqrtf(a.variance_dev ? a.variance_dev[0] : a.variance);
    for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long long t = tile * CV_STR + wave * 16 + i;
        const bool live = t < T;
        const float* xrow = a.X + (live ? t / a.S : 0) * Dx;
        cv_f4 cur[NT8], nxt[NT8];
#pragma unroll
        for (int c = 0; c < NT8; ++c) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * c + 4 * g + s;
                float v = 0.f;
                if (live && k < w0) {
                    if (c == 0 && k < L) {                       // L <= 8: the draws sit in the first chunk
                        const unsigned long long e = (unsigned long long)t * L + k;
                        v = a.z ? a.z[e] : cv_draw(a.seed, ctr, e);
                    } else {
                        v = xrow[k - L];
                    }
                }
                cur[c][s] = v;
            }
        }
        for (int l = 0; l < n - 1; ++l) {         // hidden maps
            const int in = a.dec.dims[l], out = a.dec.dims[l + 1];
            const int nc = (in + 15) >> 4, nj = (out + 15) >> 4, ld = round_up(out, 16) + 4;
            const float* wl = a.resident ? wb + a.woff[l] : wb;
            if (!a.resident) {
                __syncthreads();
                cv_stage(wb, a.dec.W[l], in, out);
                __syncthreads();
            }
#pragma unroll
            for (int jb = 0; jb < NT8; ++jb) {
                nxt[jb] = cv_f4{0.f, 0.f, 0.f, 0.f};
                if (jb < nj) nxt[jb] = *(const cv_f4*)(bbuf + l * CV_W + 16 * jb + 4 * g);
            }
#pragma unroll
            for (int c = 0; c < NT8; ++c) {
                if (c < nc) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float bv = cur[c][s];
                        const float* wr = wl + (16 * c + 4 * g + s) * ld + i;
#pragma unroll
                        for (int jb = 0; jb < NT8; ++jb)
                            if (jb < nj) nxt[jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * jb], bv, nxt[jb], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);       // one step's eight operand reads in flight, not all 256 of the unrolled map
                    }
                }
            }
#pragma unroll
            for (int jb = 0; jb < NT8; ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r) cur[jb][r] = jb < nj ? enc_act(nxt[jb][r], a.act) : 0.f;
        }
        {   // the last map: Dy <= 8 columns, this lane's k's, then the four g groups of a sample are added
            const int l = n - 1, in = a.dec.dims[l], out = Dy;
            const int nc = (in + 15) >> 4, ld = round_up(out, 16) + 4;
            const float* wl = a.resident ? wb + a.woff[l] : wb;
            if (!a.resident) {
                __syncthreads();
                cv_stage(wb, a.dec.W[l], in, out);
                __syncthreads();
            }
            float y[IWVI_CVAE_MAX_DY];
#pragma unroll
            for (int d = 0; d < IWVI_CVAE_MAX_DY; ++d) y[d] = 0.f;
#pragma unroll
            for (int c = 0; c < NT8; ++c) {
                if (c < nc) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float* wr = wl + (16 * c + 4 * g + s) * ld;
                        const cv_f4 w0v = *(const cv_f4*)wr, w1v = *(const cv_f4*)(wr + 4);
#pragma unroll
                        for (int d = 0; d < 4; ++d) { y[d] = fmaf(cur[c][s], w0v[d], y[d]); y[4 + d] = fmaf(cur[c][s], w1v[d], y[4 + d]); }
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < IWVI_CVAE_MAX_DY; ++d) {
                y[d] += __shfl_xor(y[d], 16, 64);
                y[d] += __shfl_xor(y[d], 32, 64);
            }
            if (live && g == 0) {
#pragma unroll
                for (int d = 0; d < IWVI_CVAE_MAX_DY; ++d) {
                    if (d < Dy) {
                        float v = y[d] + bbuf[l * CV_W + d];
                        if (!a.no_y_noise) {
                            const unsigned long long e = (unsigned long long)t * Dy + d;
                            v = fmaf(sd, a.zy ? a.zy[e] : cv_draw(a.seed, ctr + a.nqz, e), v);
                        }
                        a.out[t * Dy + d] = v;
                    }
                }
            }
        }
    }
    if (a.state) {
        // the last block to arrive re-zeroes the ticket and advances the counter (as k_fill_normal)
        __syncthreads();
        if (tid == 0) {
            const unsigned long long tk = __hip_atomic_fetch_add(&a.state[1], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tk == (unsigned long long)gridDim.x - 1) {
                __hip_atomic_store(&a.state[1], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&a.state[0], a.nqz + a.nqy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
static bool cv_validate(const iwvi_cvae_desc* d, const char* who) {
    if (!d) { set_error("%s: null descriptor", who); return false; }
    if (!d->enc_W || !d->enc_b || !d->dec_W || !d->dec_b || !d->enc_dims || !d->dec_dims) { set_error("%s: null pointer in the descriptor", who); return false; }
    const int n = d->n_maps;
    if (n < 1 || n > CV_MAPS) { set_error("%s: %d linear maps per net (1 .. %d)", who, n, CV_MAPS); return false; }
    if (d->L < 1 || d->L > IWVI_CVAE_MAX_L) { set_error("%s: L = %d outside 1 .. %d", who, d->L, IWVI_CVAE_MAX_L); return false; }
    if (d->Dy < 1 || d->Dy > IWVI_CVAE_MAX_DY) { set_error("%s: Dy = %d outside 1 .. %d", who, d->Dy, IWVI_CVAE_MAX_DY); return false; }
    if (d->Dx < 1) { set_error("%s: Dx = %d", who, d->Dx); return false; }
    if (d->act < IWVI_ACT_TANH || d->act > IWVI_ACT_IDENTITY) { set_error("%s: unknown activation %d", who, d->act); return false; }
    for (int i = 0; i <= n; ++i) {
        if (d->enc_dims[i] < 1 || d->enc_dims[i] > CV_W || d->dec_dims[i] < 1 || d->dec_dims[i] > CV_W) {
            set_error("%s: width %d / %d of map %d outside 1 .. %d", who, d->enc_dims[i], d->dec_dims[i], i, CV_W); return false;
        }
        if (i > 0 && i < n && d->enc_dims[i] != d->dec_dims[i]) {
            set_error("%s: hidden width %d differs between the nets (%d, %d)", who, i, d->enc_dims[i], d->dec_dims[i]); return false;
        }
    }
    if (d->enc_dims[0] != d->Dx + d->Dy) { set_error("%s: enc_dims[0] = %d, expected Dx + Dy = %d", who, d->enc_dims[0], d->Dx + d->Dy); return false; }
    if (d->dec_dims[0] != d->L + d->Dx) { set_error("%s: dec_dims[0] = %d, expected L + Dx = %d", who, d->dec_dims[0], d->L + d->Dx); return false; }
    if (d->enc_dims[n] != 2 * d->L) { set_error("%s: enc_dims[last] = %d, expected 2 L = %d", who, d->enc_dims[n], 2 * d->L); return false; }
    if (d->dec_dims[n] != d->Dy) { set_error("%s: dec_dims[last] = %d, expected Dy = %d", who, d->dec_dims[n], d->Dy); return false; }
    for (int i = 0; i < n; ++i)
        if (!d->enc_W[i] || !d->enc_b[i] || !d->dec_W[i] || !d->dec_b[i]) { set_error("%s: null weight or bias of map %d", who, i); return false; }
    if (!d->variance_dev && !(d->variance > 0.f)) { set_error("%s: variance %g", who, (double)d->variance); return false; }
    return true;
}

static void cv_net(CvNet& o, const float* const* W, const float* const* b, const int32_t* dims, int n) {
    for (int i = 0; i < CV_MAPS; ++i) { o.W[i] = i < n ? W[i] : nullptr; o.b[i] = i < n ? b[i] : nullptr; }
    for (int i = 0; i <= CV_MAPS; ++i) o.dims[i] = i <= n ? dims[i] : 0;
}

struct CvWs { size_t off_A[2 * CV_MAPS], off_D[2 * CV_MAPS], bytes; long long tiles; };
static CvWs cv_ws_layout(const iwvi_cvae_desc* d, long long B) {
    CvWs w{};
    w.tiles = (B + CV_TR - 1) / CV_TR;
    size_t o = align256(sizeof(double) * 3 * (size_t)w.tiles);
    const int n = d->n_maps;
    for (int l = 0; l < 2 * n; ++l) {
        const int32_t* dims = l < n ? d->enc_dims : d->dec_dims;
        const int i = l < n ? l : l - n;
        w.off_A[l] = o; o = align256(o + sizeof(float) * (size_t)B * dims[i]);
        w.off_D[l] = o; o = align256(o + sizeof(float) * (size_t)B * dims[i + 1]);
    }
    w.bytes = o;
    return w;
}

static int cv_train_entry(const char* who, const iwvi_cvae_desc* d, const float* X, const float* Y, int64_t B, const float* eps,
                          uint64_t seed, uint64_t* rng_state, float* eps_out, double* out, const iwvi_cvae_grads* g, bool grad, void* ws,
                          hipStream_t st) {
    if (!cv_validate(d, who)) return IWVI_ERR_ARG;
    if (!X || !Y || !out) { set_error("%s: null X, Y or out", who); return IWVI_ERR_ARG; }
    if (B <= 0 || B > (int64_t)1 << 40) { set_error("%s: B = %lld", who, (long long)B); return IWVI_ERR_ARG; }
    if (!ws || ((uintptr_t)ws & 7)) { set_error("%s: the workspace is missing (iwvi_cvae_ws_bytes) or misaligned", who); return IWVI_ERR_ARG; }
    if (!eps && !rng_state) { set_error("%s: drawing the noise needs rng_state", who); return IWVI_ERR_ARG; }
    const int n = d->n_maps;
    if (grad) {
        if (!g || !g->enc_dW || !g->enc_db || !g->dec_dW || !g->dec_db || !g->dvariance) { set_error("%s: null pointer in grads", who); return IWVI_ERR_ARG; }
        for (int i = 0; i < n; ++i)
            if (!g->enc_dW[i] || !g->enc_db[i] || !g->dec_dW[i] || !g->dec_db[i]) { set_error("%s: null gradient of map %d", who, i); return IWVI_ERR_ARG; }
    }
    const CvWs w = cv_ws_layout(d, B);
    if (w.tiles > 0x7fffffffLL) { set_error("%s: B = %lld too large", who, (long long)B); return IWVI_ERR_ARG; }
    {   // once per process: the row launch's LDS (hipFuncSetAttribute is not a stream operation)
        static bool done = false;
        if (!done) {
            hipError_t e = hipFuncSetAttribute((const void*)k_cvae_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CV_ROWS_LDS);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_cvae_rows<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CV_ROWS_LDS);
            if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute(%d B LDS): %s", who, CV_ROWS_LDS, hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
            done = true;
        }
    }
    char* base = (char*)ws;
    CvRowArgs a{};
    cv_net(a.enc, d->enc_W, d->enc_b, d->enc_dims, n);
    cv_net(a.dec, d->dec_W, d->dec_b, d->dec_dims, n);
    a.n = n; a.Dx = d->Dx; a.Dy = d->Dy; a.L = d->L; a.act = d->act;
    a.variance = d->variance; a.variance_dev = d->variance_dev;
    a.X = X; a.Y = Y; a.B = B; a.eps = eps; a.eps_out = eps_out; a.seed = seed; a.state = eps ? nullptr : (const unsigned long long*)rng_state;
    for (int l = 0; l < 2 * n; ++l) { a.A[l] = (float*)(base + w.off_A[l]); a.D[l] = (float*)(base + w.off_D[l]); }
    a.part = (double*)base;
    const unsigned long long advance = eps ? 0ULL : (unsigned long long)(((long long)B * d->L + 3) / 4);
    unsigned long long* state = eps ? nullptr : (unsigned long long*)rng_state;
    if (!grad) {
        hipLaunchKernelGGL(k_cvae_rows<false>, dim3((unsigned)w.tiles), dim3(CV_NT), CV_ROWS_LDS, st, a);
        int rc = check_launch("k_cvae_rows");
        if (rc) return rc;
        hipLaunchKernelGGL(k_cvae_finish, dim3(1), dim3(256), 0, st, (const double*)a.part, w.tiles, out, state, advance);
        return check_launch("k_cvae_finish");
    }
    hipLaunchKernelGGL(k_cvae_rows<true>, dim3((unsigned)w.tiles), dim3(CV_NT), CV_ROWS_LDS, st, a);
    int rc = check_launch("k_cvae_rows");
    if (rc) return rc;
    CvGradArgs ga{};
    ga.nl = 2 * n; ga.B = B;
    int tiles = 0;
    for (int l = 0; l < 2 * n; ++l) {
        const int32_t* dims = l < n ? d->enc_dims : d->dec_dims;
        const int i = l < n ? l : l - n;
        ga.A[l] = a.A[l]; ga.D[l] = a.D[l];
        ga.dW[l] = l < n ? g->enc_dW[i] : g->dec_dW[i];
        ga.db[l] = l < n ? g->enc_db[i] : g->dec_db[i];
        ga.in[l] = dims[i]; ga.out[l] = dims[i + 1];
        ga.tile0[l] = tiles;
        tiles += ((dims[i] + 1 + 7) / 8) * ((dims[i + 1] + 7) / 8);
    }
    ga.tile0[2 * n] = tiles;
    ga.part = a.part; ga.nparts = w.tiles; ga.out3 = out; ga.dvar = g->dvariance; ga.state = state; ga.advance = advance;
    hipLaunchKernelGGL(k_cvae_wgrad, dim3((unsigned)tiles + 1), dim3(256), 0, st, ga);
    return check_launch("k_cvae_wgrad");
}

}  // namespace iwvi

using namespace iwvi;

extern "C" size_t iwvi_cvae_ws_bytes(const iwvi_cvae_desc* desc, int64_t B) {
    if (B <= 0 || B > (int64_t)1 << 40 || !cv_validate(desc, "iwvi_cvae_ws_bytes")) return 0;
    return cv_ws_layout(desc, B).bytes;
}

extern "C" int iwvi_cvae_elbo(const iwvi_cvae_desc* desc, const float* X, const float* Y, int64_t B, const float* eps, uint64_t seed,
                              uint64_t* rng_state, float* eps_out, double* out, void* ws, void* stream_) {
    return cv_train_entry("iwvi_cvae_elbo", desc, X, Y, B, eps, seed, rng_state, eps_out, out, nullptr, false, ws, (hipStream_t)stream_);
}

extern "C" int iwvi_cvae_elbo_and_grad(const iwvi_cvae_desc* desc, const float* X, const float* Y, int64_t B, const float* eps, uint64_t seed,
                                       uint64_t* rng_state, float* eps_out, double* out, const iwvi_cvae_grads* grads, void* ws,
                                       void* stream_) {
    return cv_train_entry("iwvi_cvae_elbo_and_grad", desc, X, Y, B, eps, seed, rng_state, eps_out, out, grads, true, ws, (hipStream_t)stream_);
}

extern "C" int iwvi_cvae_predict_samples(const iwvi_cvae_desc* desc, const float* X, int64_t N, int64_t S, const float* z, const float* z_y,
                                         int flags, uint64_t seed, uint64_t* rng_state, float* out_y, void* stream_) {
    const char* who = "iwvi_cvae_predict_samples";
    if (!cv_validate(desc, who)) return IWVI_ERR_ARG;
    if (!X || !out_y) { set_error("%s: null X or out_y", who); return IWVI_ERR_ARG; }
    if (N <= 0 || S <= 0) { set_error("%s: N = %lld, S = %lld", who, (long long)N, (long long)S); return IWVI_ERR_ARG; }
    if (N >= 2147479552LL || S >= 2147479552LL || N * S >= 2147479552LL) { set_error("%s: N x S = %lld x %lld must stay below 2^31 - 4096", who, (long long)N, (long long)S); return IWVI_ERR_ARG; }
    if (flags & ~IWVI_CVAE_NO_Y_NOISE) { set_error("%s: unknown flags %d", who, flags); return IWVI_ERR_ARG; }
    const bool no_y = (flags & IWVI_CVAE_NO_Y_NOISE) != 0;
    const bool draws = !z || (!no_y && !z_y);
    if (draws && !rng_state) { set_error("%s: drawing the noise needs rng_state", who); return IWVI_ERR_ARG; }
    const int n = desc->n_maps;
    CvSampleArgs a{};
    cv_net(a.dec, desc->dec_W, desc->dec_b, desc->dec_dims, n);
    a.n = n; a.Dx = desc->Dx; a.Dy = desc->Dy; a.L = desc->L; a.act = desc->act; a.no_y_noise = no_y ? 1 : 0;
    size_t total = 0, largest = 0;                                // floats of the zero-padded weight images
    for (int l = 0; l < n; ++l) {
        const size_t w = (size_t)round_up(desc->dec_dims[l], 16) * (round_up(desc->dec_dims[l + 1], 16) + 4);
        a.woff[l] = (int)total; total += w;
        if (w > largest) largest = w;
    }
    const size_t bias = sizeof(float) * CV_MAPS * CV_W;
    a.resident = bias + sizeof(float) * total <= (size_t)CV_SAMPLE_LDS_MAX ? 1 : 0;
    a.variance = desc->variance; a.variance_dev = desc->variance_dev;
    a.X = X; a.T = N * S; a.S = S; a.z = z; a.zy = z_y; a.seed = seed;
    a.state = draws ? (unsigned long long*)rng_state : nullptr;
    a.nqz = (unsigned long long)((a.T * desc->L + 3) / 4); a.nqy = (unsigned long long)((a.T * desc->Dy + 3) / 4);
    a.out = out_y;
    const size_t lds = bias + sizeof(float) * (a.resident ? total : largest);
    {
        static bool done = false;
        if (!done) {
            hipError_t e = hipFuncSetAttribute((const void*)k_cvae_sample, hipFuncAttributeMaxDynamicSharedMemorySize, CV_SAMPLE_LDS_MAX);
            if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute(%d B LDS): %s", who, CV_SAMPLE_LDS_MAX, hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
            done = true;
        }
    }
    a.ntiles = (a.T + CV_STR - 1) / CV_STR;
    const long long blocks = a.ntiles < 1024 ? a.ntiles : 1024;   // a workgroup strides over its tiles with the weights staged once
    hipLaunchKernelGGL(k_cvae_sample, dim3((unsigned)blocks), dim3(CV_SNT), lds, (hipStream_t)stream_, a);
    return check_launch("k_cvae_sample");
}
