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

enum { FEAT_BLK = 256 };      // observations per workgroup (whole features; a longer track has a workgroup of its own)

// what the symbolic phase keeps of one window (copied at swf_batch_create: the caller's arrays are read during that call only)
struct FeatWinSrc {
    int x_base = 0, n_pose = 0, n_sb = 0, n_lm = 0, n_sc = 0;
    std::vector<int> proj_idx; std::vector<double> proj_uv;                             // [n_proj][3], [n_proj][2]
    std::vector<int> idp_kind, idp_idx; std::vector<double> idp_pts;                    // [n_idp], [n_idp][5], [n_idp][6]
    double pbg[3] = { 0, 0, 0 }; double sqrt_info = 0;
};

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
