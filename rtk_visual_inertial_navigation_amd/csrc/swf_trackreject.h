// swf_trackreject.h — the geometric gate between tracked pixels and the estimator: FeatureTracker::rejectWithF with undistortedPts and
// ptsVelocity (R/feature/feature_tracker.cpp:265-294, :334-376) for a batch of frame pairs, one workgroup each.  The
// reference's numerical content is PinholeFullCamera::liftProjective and cv::findFundamentalMat(FM_RANSAC); what is kept of the
// latter and what is specified anew is listed at swf_track_reject_batch in include/swf_solver.h.
// Per pair:
//   lift       thread t lifts points t, t + 256, ..: nine fixed-point steps, no contraction (the float64 referee's bits); un_cur,
//              un_prev, velocity are written, the virtual-camera pixels (u1 v1 of cur, u2 v2 of prev) go to LDS
//   chunk c    lane t owns hypothesis k = 256 c + t: sample of 8 (splitmix64, as k_pnp_frame), Hartley normalisation, the null vector
//              of the 8 x 9 design matrix by eight Householder reflections in registers, rank 2 by a one-sided Jacobi SVD of the
//              3 x 3, denormalisation; then the count against every point (LDS broadcast reads)
//   scan       one lane continues the sequential scan over the chunk's counts (OpenCV's RANSACUpdateNumIters, 8 model points); the
//              chunk loop ends at the first chunk that starts at or beyond n_iters
//   mask       status from the winning F with the scoring loop's own test; keep_idx by a prefix sum over the workgroup
//   exports    only for a pair with a model: a second pass over every chunk recomputes the hypotheses and writes samples, hyp, count
// No atomics: a pair's result depends on nothing but the pair, and a rerun gives the same bits.
#ifndef SWF_TRACKREJECT_H
#define SWF_TRACKREJECT_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { TRK_NMAX = SWF_TRK_NMAX, TRK_HMAX = SWF_TRK_HMAX, TRK_THREADS = 256, TRK_DRAWS = 64, TRK_LIFT_STEPS = 9, TRK_SWEEPS = 6 };

struct TrkArgs {
    int n_pairs;
    const int* first; const double* cur_px; const double* prev_px; const double* dt;     // [n_pairs + 1], [..][2], [..][2], [n_pairs]
    double cam[12];                                                                     // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
    double focal, half_col, half_row;
    int iterations, flags;
    double thr2, confidence;
    unsigned long long seed;
    unsigned char* status; int* keep_idx; int* n_inliers; int* best; int* n_iters; int* info;      // all but info may be null
    double* F; double* un_cur; double* un_prev; double* velocity;
    int* samples; double* hyp; int* count;                                              // stage exports, may be null
};

// enqueue k_track_reject for A.n_pairs pairs on stream st (swf_trackreject.hip)
int swf_internal_trk_launch(const TrkArgs& A, hipStream_t st);

#endif
