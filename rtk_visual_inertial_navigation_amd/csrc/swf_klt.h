// swf_klt.h — the stage that produces the tracked pixel pairs: the sparse optical flow of FeatureTracker::trackImage
// (R/feature/feature_tracker.cpp:98-141) for a batch of image pairs.  The reference's numerical content is
// cv::calcOpticalFlowPyrLK forward, once more in reverse from the previous positions, the 0.5 px forward-backward gate and inBorder;
// the specification is at swf_klt_track_batch in include/swf_solver.h.
//   k_klt_pyrdown  one launch per level for both images of every pair: the 5 x 5 binomial stencil on bytes, reflect-101 by index
//                  arithmetic, four neighbouring outputs per thread (55 reads instead of 100), integers only
//   k_klt_track    one wavefront per point, four per workgroup, no workgroup barrier: a wave owns its LDS slice.  Per level the wave
//                  stages the (win + 3)^2 template footprint, forms Scharr on the (win + 1)^2 grid of bilinear corners in LDS (no
//                  derivative image exists anywhere), interpolates the win^2 template into registers (element e = lane + 64 t, seven
//                  per lane at win 21) and reduces A over the wave.  Each iteration stages the (win + 1)^2 search footprint over the
//                  template's bytes, interpolates, reduces b1 and b2 and takes the 2 x 2 step in every lane alike.  The sums are sums
//                  of integers (per lane in int32, across lanes in double, below 2^35): exact in any order.  The forward and the
//                  reverse pass run in the same wave.
//   k_klt_compact  one workgroup per pair: info, and status -> keep_idx, n_keep by a prefix sum (as k_track_reject)
// max_level + 2 launches (max(max_level, back_level) + 2 where back_level is the larger).  No atomics: a pair's result depends on
// nothing but the pair, and a rerun gives the same bits.
#ifndef SWF_KLT_H
#define SWF_KLT_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { KLT_WMAX = SWF_KLT_WMAX, KLT_LMAX = SWF_KLT_LMAX, KLT_NMAX = SWF_KLT_NMAX, KLT_THREADS = 256, KLT_WAVES = 4,
       KLT_PER_LANE = (KLT_WMAX * KLT_WMAX + 63) / 64,                      // template elements per lane: 7
       KLT_GRID_PER_LANE = ((KLT_WMAX + 1) * (KLT_WMAX + 1) + 63) / 64,     // corner-grid elements per lane: 8
       KLT_FOOT = (KLT_WMAX + 3) * (KLT_WMAX + 3),                          // 576 bytes: template footprint, then search footprint
       KLT_GRID = (KLT_WMAX + 1) * (KLT_WMAX + 1),                          // 484 shorts each for Ix and Iy
       KLT_LDS_WAVE = KLT_FOOT + 4 * KLT_GRID,                              // 2512 bytes per wave
       KLT_BLOCKS_DEVICE = 64 };                                           // workgroups per pair when the point counts are device memory

struct KltArgs {
    int n_pairs, rows, cols, win, top_build, top_f, top_b, max_count, flags, blocks_per_pair;
    double eps2, min_eig, back_dist;
    const unsigned char* prev_img; const unsigned char* cur_img;            // [n_pairs][rows][cols]
    const int* first; const double* prev_px; const double* guess_px;        // [n_pairs + 1], [..][2], [..][2] or null
    double* cur_px; double* back_px; unsigned char* status; int* why; int* keep_idx; int* n_keep; int* info;
    int* trace_iters; double* trace_px;
    unsigned char* pyr;                                                     // [n_pairs][pair_bytes]
    int lw[KLT_LMAX + 1], lh[KLT_LMAX + 1];                                 // level sizes, level 0 the image
    size_t loff[KLT_LMAX + 1];                                              // offset of level l >= 1 in one image's half of a pair
    size_t half_bytes;                                                      // one image's levels 1 ..: pair_bytes / 2
};

// enqueue the pyramid, track and compact kernels for A.n_pairs pairs on stream st (swf_klt.hip)
int swf_internal_klt_launch(const KltArgs& A, hipStream_t st);

#endif
