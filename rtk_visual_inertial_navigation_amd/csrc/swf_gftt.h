// swf_gftt.h — the stage that produces the points to track: setMask, cv::goodFeaturesToTrack and addPoints of
// FeatureTracker::trackImage (R/feature/feature_tracker.cpp:148-165) for a batch of frames.  The specification is at
// swf_gftt_detect_batch in include/swf_solver.h.
//   k_gftt_old     one workgroup per frame, stage A: the tracked points ranked by counting (track_cnt descending, index ascending),
//                  then one wave walks the ranked points in chunks of 64: every lane tests its point against the kept centres in LDS,
//                  a ballot loop keeps the first surviving lane and clears the lanes inside its disc — the sequential greedy walk
//                  exactly.  The kept centres and indices go to the workspace; the frame's state and candidate counter are reset.
//   k_gftt_eig     the whole-image pass, one workgroup per 64 x 16 tile: tile + halo 2 as bytes in LDS, Sobel on tile + 1 as int16,
//                  the 3 x 3 sums of products in int32, D in int64, one double expression.  No derivative image, no float, no
//                  scratch.  free() is tested against the kept centres whose disc's bounding box meets the tile (collected in LDS
//                  once per workgroup); one partial maximum over the tile's free pixels per workgroup.
//   k_gftt_max     one workgroup per frame: the maximum of the partial maxima.  A launch of its own instead of a re-reduction in
//                  every workgroup of k_gftt_cand: at 8192 x 8192 there are 65536 tiles, and 65536 workgroups reading 65536 doubles
//                  each would cost more than the whole-image pass.
//   k_gftt_cand    per tile: eig of tile + 1 in LDS, the threshold, the 3 x 3 test, free(); the tile's candidates take their places
//                  through a counter in LDS, the workgroup takes its range from the frame's counter with one atomic add and appends
//                  (bits of t, linear index).  The counter counts every candidate, stored or not, so n_cand and TOO_MANY do not
//                  depend on the order of arrival; the total order of stage D makes the order of the list irrelevant.
//   k_gftt_select  one workgroup of 1024 threads per frame, stage D without a full sort: a radix select over the 96-bit key (t, index)
//                  finds the GFTT_K-th largest key below the last round's, those keys are gathered into LDS (48 KB), sorted by a
//                  bitonic network and walked: 1024 candidates at a time are tested by all threads against the new points kept
//                  before, then one wave runs the chunk-of-64 ballot walk over the survivors.  Further rounds only while the budget
//                  is not met and candidates remain.  Writes new_px, n_new, n_cand, max_eig, info.  The scans of the kept lists
//                  read four entries per LDS access and the passes over the candidates keep four keys in flight per thread: both
//                  are chains of dependent reads otherwise.
//   k_gftt_pack    one workgroup per frame: its offset (the sum of the totals in front of it), pack_first, pack_px, pack_src.
// Six launches on the caller's stream, whatever the arguments.  The one atomic is the candidate counter; nothing read back depends
// on the order in which it is taken, so a frame's result depends on nothing but the frame and a rerun gives the same bits.
#ifndef SWF_GFTT_H
#define SWF_GFTT_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { GFTT_NMAX = SWF_GFTT_NMAX, GFTT_RMAX = 64, GFTT_TW = 64, GFTT_TH = 16, GFTT_THREADS = 256, GFTT_SEL_THREADS = 1024, GFTT_K = 4096,
       GFTT_HEAD = 64,                                                       // bytes of the per-frame header below
       GFTT_GO = 0, GFTT_SKIP = 1, GFTT_FAILED = 2 };                        // state: detect, budget <= 0 (stage A only), writes info only

// the header of a frame's workspace, behind eig
struct GfttHead {
    int state, n_old, n_new, n_cand, total, pad;
    double m;                                                                // max of eig over the free pixels; -1: no free pixel
};

// the layout of one frame's workspace; depends on rows, cols and cand_cap alone
struct GfttLayout {
    size_t head, kept_c, kept_i, new_c, why, pmax, cand_t, cand_i, bytes;    // eig is at 0
    int tiles_x, tiles_y;
};

struct GfttArgs {
    int n_frames, rows, cols, max_cnt, r, cand_cap, flags;
    double quality;
    const unsigned char* img; const unsigned char* mask;                    // [n_frames][rows][cols]; mask or null
    const int* first; const double* px; const int* track_cnt;               // [n_frames + 1], [..][2], [..]
    const int* user_hw;                                                      // [r + 1] or null
    short hw[GFTT_RMAX + 1];                                                 // floor(sqrt(r^2 - d^2))
    int* order; int* why; int* n_old; double* new_px; int* n_new; int* n_cand; double* max_eig;
    int* pack_first; double* pack_px; int* pack_src; int* info;
    unsigned char* work;                                                     // [n_frames][L.bytes]
    GfttLayout L;
};

GfttLayout gftt_layout(int rows, int cols, int cand_cap);
// enqueue the six kernels for A.n_frames frames on stream st (swf_gftt.hip)
int swf_internal_gftt_launch(const GfttArgs& A, hipStream_t st);

#endif
