// swf_ftable.h — the resident feature table: FeatureManager (R/feature/feature_manager.cpp) as ImagePreprocess, ImagePostprocess,
// SlideWindowOld and SlideWindowNew drive it (R/swf/swf_image.cpp), for n_streams windows whose track table stays on the device
// (DESIGN 3v).  The specification is at swf_ftable_add_frame in include/swf_solver.h.  One workgroup of 256 threads per stream in
// every kernel; a stream's features live in feat_cap slots, in the reference's list order, in one of two state sets.  A kernel that
// erases features gathers the survivors from one set into the other (as k_tracker_gather does), so no move races with a read:
//   k_ftable_add        addFeatureCheckParallax + removeOut: the frame's ids rank-sorted in LDS with their source index, every table
//                       feature finds itself by binary search, appends and marks the hit; survivors of removeOut are gathered by a
//                       block scan, then the unmarked ids, ascending already, are appended behind them            (1 launch)
//   k_ftable_pnp        the gather of initFramePoseByPnP; pass 0 counts, pass 1 packs behind the streams in front  (2 launches)
//   k_ftable_tri_gather / swf_triangulate_batch's kernel / k_ftable_tri_scatter                                    (3 launches)
//   k_ftable_list       AddFeature2Problem as data; pass 0 counts landmarks and projections, pass 1 packs          (2 launches)
//   k_ftable_set_solved the landmark tail of Double2Vector and the verdict of OutliersRejection, in place          (1 launch)
//   k_ftable_remove     removeFailures; pass 0 counts, pass 1 gathers the survivors and packs the erased ids      (2 launches)
//   k_ftable_parallax   CheckParallax: the terms in parallel into a scratch row, their sum by one lane in list order (1 launch)
//   k_ftable_slide      removeBack / removeFront + removeOut2's world-point effect, gathered into the other set   (1 launch)
// Packed outputs find their offset as tracker_offset does, by summing the counts of the streams in front: no atomics, no fences, no
// scan kernel.  The launch counts above depend on nothing but the operation.
//
// Floating point, all under `#pragma clang fp contract(off)`, every operation rounding once, in this order:
//   depth in a frame   d_k = world_k - P_k;  a_r = (R[0][r] d_0 + R[1][r] d_1) + R[2][r] d_2;  b_r = (a_r + pbg_r) - tic_r;
//                      z = (ric[0][2] b_0 + ric[1][2] b_1) + ric[2][2] b_2;  idepth = 1 / z
//   parallax term      u = x_i / z_i;  v = y_i / z_i;  du = u - x_j;  dv = v - y_j;  term = sqrt(du du + dv dv)
//   parallax           sum = ((0 + term_0) + term_1) + ..;  mean = sum / num;  last_average_parallax = mean * focal;  mean >= min_parallax
//   keyframe (add)     (double) new_feature_num > new_ratio * (double) last_track_num
//   triangulate        idepth = 1 / depth, depth and world being swf_triangulate_batch's
#ifndef SWF_FTABLE_H
#define SWF_FTABLE_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { FTABLE_THREADS = 256, FTABLE_FRAME_MAX = SWF_PNP_NMAX };

// one set of the state; a stream's slot i is s * feat_cap + i, its observation k is slot * window + k
struct FtableState {
    int* n_frames; int* n_feat; int* n_listed;                              // [n_streams]
    int* id; int* start; int* n_obs; int* valid; int* flag;                 // [n_streams][feat_cap]
    double* idepth; double* world;                                          // [..], [..][3]
    double* obs; int* in_problem;                                           // [..][window][7], [..][window]
};

struct FtableArgs {
    int n_streams, window, feat_cap, frame_cap, feature_continue, min_track, min_long, long_len, pass;
    double new_ratio, min_parallax, focal;
    FtableState S, D;
    int* counts; double* parallax;                                          // [n_streams][SWF_FTABLE_NCOUNT], [n_streams]
    int* cnt_a; int* cnt_b;                                                 // pass 0 -> pass 1: [n_streams] each
    const int* f_first; const int* f_ids; const double* f_obs;              // add_frame: the frame
    int* pnp_first; double* pnp_w; double* pnp_uv;                          // pnp_points
    int* tri_start; double* tri_pt0; double* tri_pt1; double* tri_depth; double* tri_world;   // triangulate, [n_streams * feat_cap] slots
    int* lm_first; int* proj_first; int* lm_id; double* lm_world; int* lm_start; int* lm_nobs; int* lm_valid;   // list
    int* proj_frame; int* proj_lm; double* proj_uv; int* proj_new;
    const int* in_first; const double* in_world; const unsigned char* in_flags;   // set_solved
    const double* Ps; const double* Rs;                                     // [n_streams][window][3], [..][9]: set_solved
    const double* P1; const double* R1;                                     // [n_streams][3], [..][9]: slide
    const int* mode;                                                        // [n_streams]: slide
    int* rm_first; int* rm_ids;                                             // remove_failures
    double* terms;                                                          // [n_streams][feat_cap]: check_parallax
    double tic[3], ric[9], pbg[3];
};

#endif
