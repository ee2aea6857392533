// swf_trk_lift.h — the two device functions of k_track_reject that the resident tracker's finishing kernel (swf_tracker.hip) must
// evaluate to the same bits: PinholeFullCamera::liftProjective and the quotient of ptsVelocity.  One definition, included by both.
#pragma once
#include <hip/hip_runtime.h>
#include "swf_trackreject.h"

// PinholeFullCamera::liftProjective (:535-607): nine fixed-point steps in the reference's operation order.  Contraction is off, so
// every operation rounds once and a float64 evaluation of the same expressions gives the same bits.
__device__ __forceinline__ void trk_lift(const double cam[12], double px, double py, double& xo, double& yo) {
#pragma clang fp contract(off)
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7];
    const double k3 = cam[8], k4 = cam[9], k5 = cam[10], k6 = cam[11];
    const double x0 = px / fx - cx / fx, y0 = py / fy - cy / fy;
    double x = x0, y = y0;
    for (int j = 0; j < TRK_LIFT_STEPS; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double deltaX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double deltaY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    xo = x; yo = y;
}

// ptsVelocity (:361-363): with the flag the difference is a float's, the quotient a double's, the result a float's
__device__ __forceinline__ double trk_velocity(double c, double p, double dt, bool as_float) {
#pragma clang fp contract(off)
    if (as_float) return (double)(float)((double)((float)c - (float)p) / dt);
    return (c - p) / dt;
}
