// swf_features.h — the post-solve feature check (SWFOptimization::OutliersRejection + the depth-sign test of Double2Vector,
// R/swf/swf_image.cpp:255-308, R/swf/swf.cpp:214-229) as a read-only operator over the device state: what the engine
// (swf_engine.hip) and the kernels' translation unit (swf_features.hip) share.
//
// The check owns its observation table: it is built from the flat window alone (every projection factor and every inverse-depth
// factor, whichever solve path they took), features in the caller's order, a feature's observations in the caller's factor order.
#ifndef SWF_FEATURES_H
#define SWF_FEATURES_H

#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/swf_solver.h"
// FeatWinSrc, the window's visual factors as the caller gave them, is declared in swf_plan.h: the symbolic phase fills it (HostWin::feat)
// and that file must stay free of HIP, which this header is not; swf_internal_feature_tables below is its only reader
#include "swf_plan.h"

enum { FEAT_BLK = 256 };      // observations per workgroup (whole features; a longer track has a workgroup of its own)

// host form of the tables (concatenated over the windows of a batch)
struct FeatTables {
    std::vector<int4> o_a;            // per observation: state index of pose j (-1: identity), of the camera extrinsic, of the feature block, of the anchor pose (-1: none)
    std::vector<int2> o_b;            // per observation: state index of the extrinsic the anchor point is lifted through (inverse depth; -1 for a world point), its feature
    std::vector<double2> o_uv;        // per observation: image point
    std::vector<int> f_obs0;          // [n_feat + 1] first observation of a feature
    std::vector<double> f_pi;         // [n_feat][3] anchor point pts_i of an inverse-depth feature (0 for a world point)
    std::vector<int4> blk;            // per workgroup: window, first feature, one past its last feature, 0
    std::vector<int> w_feat0;         // [n_win + 1] first feature of a window
    std::vector<double> w_cst;        // [n_win][4] pbg, proj_sqrt_info
};

struct FeatArgs {
    const double* x;                  // the batch state (what swf_batch_download_state copies)
    const int4* o_a; const int2* o_b; const double2* o_uv;
    const int* f_obs0; const double* f_pi; const int4* blk; const int* w_feat0; const double* w_cst;
    double* mean_err; double* depth; int* n_obs; unsigned char* flags;      // [n_feat]
    int* rejected; int* n_rejected;                                         // [n_feat] (a window's run starts at its first feature), [n_win]
    int n_blk, n_win; double thr;
};

// SWF_E_INVALID (message set) when the factors of one inverse depth disagree on (pose_i, pts_i)
int swf_internal_feature_tables(const std::vector<FeatWinSrc>& src, FeatTables& T);
int swf_internal_feature_launch(const FeatArgs& A, hipStream_t st);

#endif
