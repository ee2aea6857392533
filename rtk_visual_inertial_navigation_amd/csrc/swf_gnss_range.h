// swf_gnss_range.h — distance() of the reference (R/gnss/src/common_function.cpp:126-134): the geometric range with the Sagnac
// term, and the unit line-of-sight vector.  One restatement for every translation unit that evaluates a GNSS range: the scalar
// factors of the solve path (swf_kernels.h) and the pre-fit carrier-phase screen (swf_phasescreen.hip).
#pragma once
#include <hip/hip_runtime.h>

#define CLIGHT_D 299792458.0
#define OMGE_D 7.2921151467E-5

__device__ __forceinline__ double gnss_distance(const double* rr, const double* rs, double* e) {
    e[0] = rr[0] - rs[0]; e[1] = rr[1] - rs[1]; e[2] = rr[2] - rs[2];
    double r = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    e[0] /= r; e[1] /= r; e[2] /= r;
    return r + OMGE_D * (rs[0] * rr[1] - rs[1] * rr[0]) / CLIGHT_D;
}
