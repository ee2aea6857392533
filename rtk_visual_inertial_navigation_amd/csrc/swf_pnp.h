// swf_pnp.h — the pose of a new image frame from the landmarks it observes: FeatureManager::initFramePoseByPnP with solvePoseByPnP
// (R/feature/feature_manager.cpp:164-243) for a batch of frames, one workgroup each.  The reference's numerical content is
// cv::solvePnPRansac; what is kept of it and what is specified anew is listed at swf_pnp_frame_batch in include/swf_solver.h.
// Per frame:
//   stage      the frame's points (X Y Z u v), rounded through float with flag bit 0, in LDS; Ps / Rs of the previous frame -> cam_T_w
//   sample     lane k draws the 5 indices of hypothesis k: x = splitmix64(seed + 64 k + j), index ((x >> 32) n) >> 32, repeats skipped
//   solve      lane k: PNP_K_MIN Gauss-Newton steps from the guess over its sample, 21 + 6 sums, R and t in registers
//   score      lane k against every point (LDS broadcast reads): inlier iff z > 0 and |r|^2 <= thr^2; integer counts
//   scan       one lane: the best hypothesis and the adaptive iteration count, OpenCV's RANSACUpdateNumIters
//   refine     PNP_K_REF steps over the best hypothesis's inliers: thread t adds points t, t + 128, .. in ascending order, the 27 sums
//              are combined by a halving tree in LDS, nine at a time; every thread then solves the same 6 x 6 system
//   convert    cam_T_w -> Ps, Rs of the IMU frame
// No atomics: a frame's result depends on nothing but the frame, and a rerun gives the same bits.
#ifndef SWF_PNP_H
#define SWF_PNP_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { PNP_NMAX = SWF_PNP_NMAX, PNP_HMAX = SWF_PNP_HMAX, PNP_THREADS = 128, PNP_K_MIN = 6, PNP_K_REF = 10, PNP_DRAWS = 64 };

struct PnpArgs {
    int n_frames;
    const int* first; const double* pts_w; const double* pts_uv;      // [n_frames + 1], [..][3], [..][2]
    const double* Ps_prev; const double* Rs_prev;                     // [n_frames][3], [n_frames][9]
    double tic[3], ric[9], pbg[3];
    int iterations, flags;
    double thr2, confidence;
    unsigned long long seed;
    double* Ps_out; double* Rs_out; int* n_inliers; unsigned char* inlier; int* best; int* n_iters; int* info;
    int* samples; double* hyp; int* count;                            // stage exports, may be null
};

// enqueue k_pnp_frame for A.n_frames frames on stream st (swf_pnp.hip)
int swf_internal_pnp_launch(const PnpArgs& A, hipStream_t st);

#endif
