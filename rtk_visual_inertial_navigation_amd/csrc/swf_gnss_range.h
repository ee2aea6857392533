// swf_gnss_range.h — distance() of the reference (R/gnss/src/common_function.cpp:126-134): the geometric range with the Sagnac
// term, and the unit line-of-sight vector.  One restatement for every translation unit that evaluates a GNSS range: the scalar
// factors of the solve path (swf_kernels.h), the pre-fit carrier-phase screen (swf_phasescreen.hip) and the single-epoch solve
// (swf_gnssepoch.hip).  gnss_range_rate is velecitydistance() (R/gnss/src/common_function.cpp:411-421) with the statements of
// d_eval_scalar's Doppler branch: the range rate with its Sagnac term, the unit line of sight e, ev = vel - satvel, the plain
// distance rr and ee = ev . e (what the position Jacobian (ev - ee e) / rr needs).
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

__device__ __forceinline__ double gnss_range_rate(const double* xg, const double* vel, const double* rs, const double* vs, double* e,
                                                  double* ev, double* rr, double* ee) {
    e[0] = xg[0] - rs[0]; e[1] = xg[1] - rs[1]; e[2] = xg[2] - rs[2];
    *rr = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    for (int k = 0; k < 3; k++) { e[k] /= *rr; ev[k] = vel[k] - vs[k]; }
    *ee = ev[0] * e[0] + ev[1] * e[1] + ev[2] * e[2];
    return *ee + OMGE_D / CLIGHT_D * (vs[1] * xg[0] + rs[1] * vel[0] - vs[0] * xg[1] - rs[0] * vel[1]);
}
