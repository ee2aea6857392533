// swf_devutil.h — device functions that more than one operator's kernel uses unchanged: the sampling hash and the iteration bound of
// the two RANSAC kernels (k_pnp_frame, k_track_reject) and the finiteness test.  The NumPy referees of the tests mirror these
// definitions operation by operation; what differs between the kernels (sampling loops, inlier tests, scans) stays with them.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

__device__ __forceinline__ unsigned long long swf_mix(unsigned long long x) {     // splitmix64's output at state x + 0x9E37..
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ bool swf_finite(double v) { return fabs(v) < __builtin_inf(); }          // false for a NaN

// OpenCV's RANSACUpdateNumIters with ep = (n - count) / n; the power is m - 1 products
__device__ __forceinline__ int swf_update_iters(double conf, int count, int n, int m, int n_iters) {
    const double p = fmin(fmax(conf, 0.0), 1.0);
    const double ep = fmin(fmax((double)(n - count) / (double)n, 0.0), 1.0);
    const double num = fmax(1.0 - p, DBL_MIN), w = 1.0 - ep;
    double wm = w;
    for (int i = 1; i < m; i++) wm *= w;
    const double d = 1.0 - wm;
    if (d < DBL_MIN) return 0;
    const double ln = log(num), ld = log(d);
    if (ld >= 0.0 || -ln >= (double)n_iters * -ld) return n_iters;
    return (int)rint(ln / ld);
}
