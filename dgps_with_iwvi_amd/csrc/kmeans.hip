// Lloyd's k-means with the semantics of scipy.cluster.vq.kmeans2's loop (iwvi_kmeans): the first-layer inducing inputs of every model the
// reference builds (experiments/build_models.py:179-180), ten rounds of an N x M distance table and M segmented means.
//
//   launches  k_km_init (Z_init -> the float64 running centroids C in the workspace), then per iteration k_km_step and k_km_update.
//             Nothing returns to the host in between.
//   step      a grid of G = min(chunks, KM_MAX_WG) workgroups (times S cluster ranges, below); workgroup g walks ITS contiguous run of
//             chunks of 256 P points in order.  A lane owns P points, their coordinates float64 in registers, padded with zeros to the
//             template ceiling DC (8 / 16 / 32: (0 - 0)^2 adds an exact zero, the D loop is unrolled without a bound).  The centroids stand
//             in LDS as [tile][DC] float64 (zero padded alike): a row is read at one address by the whole wave, a broadcast; P = 2 (below
//             DC = 32, beyond KM_P1_POINTS points) halves those reads per distance.  d = sum_d (x_d - c_d)^2 in dimension order, best = the lowest index of the
//             smallest d (strict <, from best = 0 and d = +inf: the index is a centroid's whatever the data holds).  M DC 8 B of centroids
//             beyond KM_CEN_BYTES are walked in tiles, restaged per chunk.
//   sums      labels and coordinates of the chunk pass through LDS.  Cluster m belongs to the group of DC threads q = m % groups, thread
//             (dimension d, group q) owns the LDS accumulator (m, d).  A lane marks its point in the bitmap of the group that owns the
//             point's cluster (an integer OR in LDS: the words do not depend on who came first); each group then walks ITS set bits in
//             ascending order -- its points in order -- and adds x_d: one owner per (m, d), one order of addition, no floating-point
//             atomics.  M DC 8 B of accumulators beyond KM_ACC_BYTES: S workgroups per run of chunks, each owning a range of clusters
//             (all of them repeat the assignment; the first one writes labels and inertia).  A point with a non-finite coordinate gets label
//             -1, which is in no range: it enters no sum, no count, no inertia; a label is tested against the workgroup's range before it
//             is an offset.  The workgroup leaves [M, D] float64 sums, [M] counts and its inertia in the workspace.
//   update    workgroup m adds the G partials of cluster m: thread (d, slice) a contiguous run of workgroups in order, the slices in order.
//             mean = sum / count, an empty cluster keeps its row.  The last iteration writes the outputs.
//   Every sum has one fixed order for given (N, M, D): two calls give the same bits.
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int KM_THREADS = 256;
constexpr int KM_MAX_WG = 512;                   // workgroups per step launch (two per CU): the workspace holds one [M, D] partial for each
constexpr int KM_P1_POINTS = 256 * KM_MAX_WG;    // up to this N a lane owns ONE point (P = 1): a workgroup per 256 points, a short chunk each
constexpr int KM_CEN_BYTES = 48 * 1024;          // centroid tile in LDS
constexpr int KM_ACC_BYTES = 64 * 1024;          // cluster-sum accumulators in LDS
// LDS of a step workgroup: centroid tile | accumulators | 8 doubles | coordinates of a chunk (256 P DC floats <= 32 KiB) | labels | counts |
// the owner groups' bitmaps (<= 2 KiB)

struct KmArgs {
    const float* X; long long N; int D, M;
    double* C;                                   // [M, D] running centroids
    double* part; double* pin; int* pcnt;        // [G, M, D] sums, [G] inertia, [G, M] counts
    int* labels;                                 // written when non-null (the last iteration)
    int G, S, TM, Mh, nchunks;                   // workgroups, cluster ranges, centroids per tile, clusters per range, chunks of 256 P points
    float* out_Z; double* out_Z64; int* out_counts; double* out_inertia;
};

__device__ __forceinline__ double km_wsum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }

__global__ void k_km_init(const float* __restrict__ Z, double* __restrict__ C, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) C[i] = (double)Z[i];
}

// a centroid's row [DC] from LDS (one address for the whole wave) into registers
template <int DC>
__device__ __forceinline__ void km_load_row(double2 (&r)[DC / 2], const double* row) {
#pragma unroll
    for (int k = 0; k < DC / 2; ++k) r[k] = reinterpret_cast<const double2*>(row)[k];
}

// squared distance of the lane's P points to the centroid in r, summed in dimension order; the nearest so far is kept (strict <)
template <int DC, int P>
__device__ __forceinline__ void km_nearest(const double (&x)[P][DC], const double2 (&r)[DC / 2], int m, double (&bd)[P], int (&bi)[P]) {
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DC / 2; ++k) {
            const double t0 = x[q][2 * k] - r[k].x, t1 = x[q][2 * k + 1] - r[k].y;
            s = fma(t0, t0, s);
            s = fma(t1, t1, s);
        }
        if (s < bd[q]) { bd[q] = s; bi[q] = m; }
    }
}

template <int DC, int P>
__global__ __launch_bounds__(KM_THREADS) void k_km_step(KmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    constexpr int CH = KM_THREADS * P;
    double* cen = reinterpret_cast<double*>(km_lds);              // [TM][DC]
    double* acc = cen + (size_t)a.TM * DC;                        // [Mh][DC]
    double* red = acc + (size_t)a.Mh * DC;                        // [8]
    float* xs = reinterpret_cast<float*>(red + 8);                // [CH][DC]
    int* lab = reinterpret_cast<int*>(xs + CH * DC);              // [CH]
    int* cnt = lab + CH;                                          // [Mh]
    constexpr int NG = KM_THREADS / DC, BW = CH / 32;             // owner groups; words of a group's bitmap over the chunk's points
    unsigned* bmap = reinterpret_cast<unsigned*>(cnt + a.Mh);     // [NG][BW]
    const int tid = threadIdx.x, g = blockIdx.x, h = blockIdx.y;
    const int D = a.D, M = a.M, TM = a.TM;
    const int m_lo = h * a.Mh, mh = min(a.Mh, M - m_lo);          // this workgroup's clusters (S Mh >= M and (S - 1) Mh < M: mh >= 1)
    const int d_own = tid & (DC - 1), grp = tid / DC;
    for (int i = tid; i < mh * DC; i += KM_THREADS) acc[i] = 0.0;
    for (int i = tid; i < mh; i += KM_THREADS) cnt[i] = 0;
    for (int i = tid; i < NG * BW; i += KM_THREADS) bmap[i] = 0u;
    const int c_lo = (int)((long long)g * a.nchunks / a.G), c_hi = (int)((long long)(g + 1) * a.nchunks / a.G);
    const bool one_tile = TM >= M;
    double inertia = 0.0;
    for (int c = c_lo; c < c_hi; ++c) {
        const long long p0 = (long long)c * CH;
        double x[P][DC], bd[P];
        int bi[P];
        bool fin[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const long long p = p0 + q * KM_THREADS + tid;
            const bool live = p < a.N;
            const float* row = a.X + (size_t)(live ? p : 0) * D;
            float v[DC];
#pragma unroll
            for (int d = 0; d < DC; ++d) v[d] = row[min(d, D - 1)];      // every load is issued, none waits for another: the address is clamped,
            fin[q] = live;                                        // the value chosen afterwards
#pragma unroll
            for (int d = 0; d < DC; ++d) {
                const float u = (d < D && live) ? v[d] : 0.f;
                fin[q] = fin[q] && (u - u == 0.f);
                x[q][d] = (double)u;
            }
            bd[q] = INFINITY; bi[q] = 0;
        }
        for (int m0 = 0; m0 < M; m0 += TM) {
            const int tm = min(TM, M - m0);
            if (!one_tile || c == c_lo) {                         // (uniform) a single tile is staged once
                __syncthreads();                                  // the tile's previous readers are done
                for (int i = tid; i < tm * DC; i += KM_THREADS) {
                    const int mm = i / DC, d = i & (DC - 1);
                    cen[i] = d < D ? a.C[(size_t)(m0 + mm) * D + d] : 0.0;
                }
                __syncthreads();
            }
            // the row of centroid m + 1 is on its way from LDS to registers while row m is used: one wave per SIMD hides no LDS latency,
            // and left to itself the compiler waits for every 16 bytes where it needs them
            // (two register rows used in turn: no copies)
            double2 ra[DC / 2], rb[DC / 2];
            km_load_row<DC>(ra, cen);
            for (int m = 0; m < tm; m += 2) {
                km_load_row<DC>(rb, cen + min(m + 1, tm - 1) * DC);
                __builtin_amdgcn_sched_barrier(0);                // (the loads stay ahead of the arithmetic)
                km_nearest<DC, P>(x, ra, m0 + m, bd, bi);
                __builtin_amdgcn_sched_barrier(0);
                km_load_row<DC>(ra, cen + min(m + 2, tm - 1) * DC);
                __builtin_amdgcn_sched_barrier(0);
                if (m + 1 < tm) km_nearest<DC, P>(x, rb, m0 + m + 1, bd, bi);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const int idx = q * KM_THREADS + tid;
            const long long p = p0 + idx;
            const int l = fin[q] ? bi[q] : -1;
            lab[idx] = l;                                         // (every entry of the chunk is written: -1 behind the last point)
#pragma unroll
            for (int d = 0; d < DC; ++d) xs[idx * DC + d] = (float)x[q][d];
            if (fin[q]) inertia += bd[q];
            if (a.labels && h == 0 && p < a.N) a.labels[p] = l;
            // a point of this workgroup's clusters: its bit in the bitmap of the group that owns the cluster (an integer OR: the words do
            // not depend on the order of arrival).  The label is tested against the range before it is an index
            const int m = l - m_lo;
            if ((unsigned)m < (unsigned)mh) atomicOr(&bmap[(m & (NG - 1)) * BW + (idx >> 5)], 1u << (idx & 31));
        }
        __syncthreads();
        {   // thread (d_own, grp) walks the set bits of its group in ascending order -- the points in order -- and clears the words
            unsigned bits[BW];
#pragma unroll
            for (int w = 0; w < BW; ++w) bits[w] = bmap[grp * BW + w];
#pragma unroll
            for (int w = 0; w < BW; ++w) {
                unsigned b = bits[w];
                while (b) {
                    const int pt = w * 32 + __ffs(b) - 1;
                    b &= b - 1;
                    const int m = lab[pt] - m_lo;
                    if ((unsigned)m < (unsigned)mh) {
                        acc[m * DC + d_own] += (double)xs[pt * DC + d_own];
                        if (d_own == 0) cnt[m] += 1;
                    }
                }
                if (bits[w]) bmap[grp * BW + w] = 0u;             // (every lane of the group stores the same zero)
            }
        }
        __syncthreads();                                          // labels, coordinates and bitmaps are free for the next chunk
    }
    __syncthreads();
    for (int i = tid; i < mh * D; i += KM_THREADS) {
        const int mm = i / D, d = i - mm * D;
        a.part[((size_t)g * M + m_lo + mm) * D + d] = acc[mm * DC + d];
    }
    for (int i = tid; i < mh; i += KM_THREADS) a.pcnt[(size_t)g * M + m_lo + i] = cnt[i];
    inertia = km_wsum(inertia);                                   // fixed order: xor tree in the wave, then the four waves in order
    if ((tid & 63) == 0) red[tid >> 6] = inertia;
    __syncthreads();
    if (tid == 0 && h == 0) a.pin[g] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <int DC>
__global__ __launch_bounds__(KM_THREADS) void k_km_update(KmArgs a, int last) {
    constexpr int NS = KM_THREADS / DC;
    __shared__ double red[KM_THREADS];
    __shared__ int cred[NS];
    const int tid = threadIdx.x, m = blockIdx.x, d = tid & (DC - 1), s = tid / DC;
    const int D = a.D, M = a.M, G = a.G;
    const int g_lo = s * G / NS, g_hi = (s + 1) * G / NS;
    double v = 0.0;
    int n = 0;
    if (d < D) for (int g = g_lo; g < g_hi; ++g) v += a.part[((size_t)g * M + m) * D + d];
    if (d == 0) for (int g = g_lo; g < g_hi; ++g) n += a.pcnt[(size_t)g * M + m];
    red[tid] = v;
    if (d == 0) cred[s] = n;
    __syncthreads();
    if (s == 0 && d < D) {
        double tot = red[d];
        int cnt = cred[0];
        for (int k = 1; k < NS; ++k) { tot += red[k * DC + d]; cnt += cred[k]; }
        const size_t e = (size_t)m * D + d;
        const double c = cnt > 0 ? tot / (double)cnt : a.C[e];    // an empty cluster keeps its row
        a.C[e] = c;
        if (last) {
            if (a.out_Z64) a.out_Z64[e] = c;
            a.out_Z[e] = (float)c;
            if (d == 0 && a.out_counts) a.out_counts[m] = cnt;
        }
    }
    if (last && m == 0 && tid == 0 && a.out_inertia) {
        double t = 0.0;
        for (int g = 0; g < G; ++g) t += a.pin[g];
        *a.out_inertia = t;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
struct KmPlan { int DC, P, G, S, TM, Mh, nchunks; size_t lds, off_part, off_pin, off_pcnt, bytes; };

static bool km_args_ok(int64_t N, int M, int D) { return N >= 1 && N <= 0x7fffffffLL && D >= 1 && D <= IWVI_MAX_D && M >= 1 && M <= IWVI_MAX_M; }

// max_wg: KM_MAX_WG, or the development switch IWVI_KM_MAX_WG below it (a smaller grid: the tests reach a workgroup's walk over several
// chunks at small N with it; the workspace is sized for KM_MAX_WG)
static KmPlan km_plan(int64_t N, int M, int D, int max_wg = KM_MAX_WG) {
    KmPlan p{};
    p.DC = D <= 8 ? 8 : D <= 16 ? 16 : 32;
    p.P = (p.DC == 32 || N <= KM_P1_POINTS) ? 1 : 2;
    const int ch = KM_THREADS * p.P;
    p.nchunks = (int)((N + ch - 1) / ch);
    p.G = p.nchunks < max_wg ? p.nchunks : max_wg;
    const int tm_max = KM_CEN_BYTES / (8 * p.DC), mh_max = KM_ACC_BYTES / (8 * p.DC);
    p.TM = M < tm_max ? M : tm_max;
    p.S = (M + mh_max - 1) / mh_max;
    p.Mh = (M + p.S - 1) / p.S;
    p.lds = sizeof(double) * ((size_t)p.TM * p.DC + (size_t)p.Mh * p.DC + 8) + sizeof(float) * (size_t)ch * p.DC + sizeof(int) * ((size_t)ch + p.Mh + (size_t)(KM_THREADS / p.DC) * (ch / 32));
    size_t o = align256(sizeof(double) * (size_t)M * D);
    p.off_part = o; o = align256(o + sizeof(double) * (size_t)p.G * M * D);
    p.off_pin = o;  o = align256(o + sizeof(double) * (size_t)p.G);
    p.off_pcnt = o; o = align256(o + sizeof(int) * (size_t)p.G * M);
    p.bytes = o;
    return p;
}

template <int DC, int P>
static int km_run(const KmArgs& a0, const KmPlan& p, int iters, int* labels, hipStream_t st) {
    static bool attr_set = false;                                 // once per process and instantiation (not a stream operation)
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_km_step<DC, P>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("iwvi_kmeans: hipFuncSetAttribute: %s", hipGetErrorString(e)); return IWVI_ERR_LAUNCH; }
        attr_set = true;
    }
    for (int it = 0; it < iters; ++it) {
        const int last = it == iters - 1;
        KmArgs a = a0;
        a.labels = last ? labels : nullptr;
        hipLaunchKernelGGL((k_km_step<DC, P>), dim3(p.G, p.S), dim3(KM_THREADS), p.lds, st, a);
        if (int rc = check_launch("k_km_step")) return rc;
        hipLaunchKernelGGL((k_km_update<DC>), dim3(a.M), dim3(KM_THREADS), 0, st, a, last);
        if (int rc = check_launch("k_km_update")) return rc;
    }
    return IWVI_OK;
}

}  // namespace iwvi

extern "C" size_t iwvi_kmeans_ws_bytes(int64_t N, int M, int D) {
    using namespace iwvi;
    return km_args_ok(N, M, D) ? km_plan(N, M, D).bytes : 0;
}

extern "C" int iwvi_kmeans(const float* X, int64_t N, int D, const float* Z_init, int M, int iters,
                           float* out_Z, double* out_Z64, int32_t* out_labels, int32_t* out_counts, double* out_inertia,
                           void* ws, void* stream_) {
    using namespace iwvi;
    const char* fn = "iwvi_kmeans";
    if (!X) { set_error("%s: null X", fn); return IWVI_ERR_ARG; }
    if (!Z_init) { set_error("%s: null Z_init", fn); return IWVI_ERR_ARG; }
    if (!out_Z) { set_error("%s: null out_Z", fn); return IWVI_ERR_ARG; }
    if (!ws) { set_error("%s: null ws", fn); return IWVI_ERR_ARG; }
    if (N < 1 || N > 0x7fffffffLL) { set_error("%s: N=%lld out of range (1 .. 2^31 - 1)", fn, (long long)N); return IWVI_ERR_ARG; }
    if (D < 1 || D > IWVI_MAX_D) { set_error("%s: D=%d out of range (1 .. %d)", fn, D, IWVI_MAX_D); return IWVI_ERR_ARG; }
    if (M < 1 || M > IWVI_MAX_M) { set_error("%s: M=%d out of range (1 .. %d)", fn, M, IWVI_MAX_M); return IWVI_ERR_ARG; }
    if (iters < 1) { set_error("%s: iters=%d must be at least 1", fn, iters); return IWVI_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream_;
    const int cap = dbg_opt("IWVI_KM_MAX_WG");
    const KmPlan p = km_plan(N, M, D, cap >= 1 && cap < KM_MAX_WG ? cap : KM_MAX_WG);
    char* w = static_cast<char*>(ws);
    KmArgs a{};
    a.X = X; a.N = N; a.D = D; a.M = M;
    a.C = reinterpret_cast<double*>(w);
    a.part = reinterpret_cast<double*>(w + p.off_part);
    a.pin = reinterpret_cast<double*>(w + p.off_pin);
    a.pcnt = reinterpret_cast<int*>(w + p.off_pcnt);
    a.G = p.G; a.S = p.S; a.TM = p.TM; a.Mh = p.Mh; a.nchunks = p.nchunks;
    a.out_Z = out_Z; a.out_Z64 = out_Z64; a.out_counts = out_counts; a.out_inertia = out_inertia;
    hipLaunchKernelGGL(k_km_init, dim3((M * D + KM_THREADS - 1) / KM_THREADS), dim3(KM_THREADS), 0, st, Z_init, a.C, M * D);   // (before out_Z is written: it may be Z_init)
    if (int rc = check_launch("k_km_init")) return rc;
    if (p.DC == 8) return p.P == 2 ? km_run<8, 2>(a, p, iters, out_labels, st) : km_run<8, 1>(a, p, iters, out_labels, st);
    if (p.DC == 16) return p.P == 2 ? km_run<16, 2>(a, p, iters, out_labels, st) : km_run<16, 1>(a, p, iters, out_labels, st);
    return km_run<32, 1>(a, p, iters, out_labels, st);
}
