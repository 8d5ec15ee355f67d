// Running mean and sum of squared deviations of a set of float32 tensors, in float64 (iwvi_moments_update): the instrument behind
// backward.gradient_moments / snr_summary -- the gradient of every parameter over repeated noise draws, accumulated on the device.
//
//   launches  k_moments (grid = (blocks, tensors), like k_adam: one table by value, one launch for all of them), then k_moments_count (one
//             thread) which stores the new count.  Every thread of k_moments reads the OLD count, so the two launches are ordered by the
//             stream alone and a captured pair replays as it is: nothing the host knows enters the kernels but pointers.
//   update    Welford's: c = count + 1, d = x - mean, mean += d / c, m2 += d (x - mean).  One thread owns an element: no reduction, no
//             atomics, two calls on the same data give the same bits.  At c = 1 mean = x exactly (d / 1) and m2 = d (x - x) = 0 exactly.
#include <math.h>
#include "iwvi_common.h"

namespace iwvi {

constexpr int MOM_MAX = 48;                      // tensors per call (iwvi_adam_step's table size: the same parameter lists arrive here)
struct MomTensor { const float* x; double* mean; double* m2; long long n; };
struct MomArgs { MomTensor t[MOM_MAX]; const long long* count; };

__global__ __launch_bounds__(256) void k_moments(MomArgs a) {
    const MomTensor& T = a.t[blockIdx.y];
    const double c = (double)(*a.count + 1);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < T.n; i += (long long)gridDim.x * blockDim.x) {
        const double x = (double)T.x[i];
        double mean = T.mean[i];
        const double d = x - mean;
        mean += d / c;
        T.mean[i] = mean;
        T.m2[i] += d * (x - mean);
    }
}
__global__ void k_moments_count(long long* p) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += 1; }

}  // namespace iwvi

using namespace iwvi;

extern "C" int iwvi_moments_update(const iwvi_moments_tensor* tensors, int n_tensors, int64_t* count_dev, void* stream_) {
    if (!tensors || n_tensors <= 0 || n_tensors > MOM_MAX || !count_dev) { set_error("iwvi_moments_update: bad argument (1..%d tensors, a device count)", MOM_MAX); return IWVI_ERR_ARG; }
    MomArgs a{};
    long long nmax = 1;
    for (int i = 0; i < n_tensors; ++i) {
        const iwvi_moments_tensor& s = tensors[i];
        if (!s.x || !s.mean || !s.m2 || s.n < 0) { set_error("iwvi_moments_update: bad tensor %d", i); return IWVI_ERR_ARG; }
        a.t[i] = MomTensor{s.x, s.mean, s.m2, (long long)s.n};
        if (s.n > nmax) nmax = s.n;
    }
    a.count = (const long long*)count_dev;
    long long blocks = (nmax + 255) / 256; if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_moments, dim3((unsigned)blocks, n_tensors), dim3(256), 0, (hipStream_t)stream_, a);
    hipLaunchKernelGGL(k_moments_count, dim3(1), dim3(64), 0, (hipStream_t)stream_, (long long*)count_dev);
    return check_launch("k_moments");
}
