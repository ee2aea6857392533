// swf_tracker.h — the resident feature tracker: FeatureTracker::trackImage (R/feature/feature_tracker.cpp:88-263) and removeOutliers
// for n_streams image sequences whose state stays on the device.  The specification is at swf_tracker_track in
// include/swf_solver.h.  The numeric stages are the three operators' launchers, unchanged; this file's kernels are the bookkeeping
// between them, one workgroup of 256 threads per stream each:
//   k_tracker_after_klt   gathers prev_px, cur_px, ids, track_cnt (+ 1: the reference's n++) and the lineage by the KLT's keep_idx
//   k_tracker_after_f     gathers cur_px, ids, track_cnt and the lineage by the gate's keep_idx (all points where the gate did not run
//                         or found no model)
//   k_tracker_finish      walks the detector's pack_px / pack_src: a kept point takes its id, count and lineage, a new one
//                         id = n_id + j, count 1, lineage -1; the lift, the velocity against the previous frame's observation at the
//                         lineage index, the 7-vector; writes the frame and the rolled state, n_id += n_new, counts and info
//   k_tracker_mark        removeOutliers: the stream's id list in LDS, every point tested against it, the survivors' indices by wave64
//                         ballots and an LDS scan over the four waves
//   k_tracker_gather      the state gathered by k_tracker_mark's indices into the other state buffer
// Every array is packed stream after stream behind a `first` of n_streams + 1 offsets, as the operators want it.  A workgroup finds
// its offset by summing the counts of the streams in front of it (as k_gftt_pack does), so there is no scan kernel and stream order
// is the only dependency: no atomics, no fences.  A stream keeps at most max_cnt points, so n_streams * max_cnt slots hold any frame.
// The lineage of a point is its index in the previous frame's observation array (-1: new); it replaces the reference's id maps.
#ifndef SWF_TRACKER_H
#define SWF_TRACKER_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"
#include "swf_gftt.h"

enum { TRACKER_THREADS = 256 };

// one set of the state that lives from frame to frame; removeOutliers gathers from one set into the other
struct TrackerState {
    int* first; double* px; int* ids; int* tc; int* lin;                    // [n_streams + 1], [..][2], [..], [..], [..]
};

struct TrackerArgs {
    int n_streams, max_cnt, have_klt;
    TrackerState S;                                                         // the state the frame starts from and rolls into
    TrackerState D;                                                         // k_tracker_gather: the destination
    int* n_id;                                                              // [n_streams]
    const double* dt;                                                       // [n_streams]
    double* cur1; int* k1; int* nk1; int* kinfo;                            // the KLT's outputs on S
    int* first1; double* pxp1; double* pxc1; int* ids1; int* tc1; int* lin1;   // after the KLT
    int* k2; int* ni2; int* tinfo;                                          // the gate's outputs
    int* first2; double* px2; int* ids2; int* tc2; int* lin2;               // after the gate
    int* pf3; double* ppx3; int* psrc3; int* nold3; int* nnew3; int* ncand3; int* ginfo;   // the detector's outputs
    const unsigned char* work; GfttLayout L;                                // its workspace: a TOO_MANY frame's kept list is read there
    int* ffirst; int* fids; int* ftc; double* fpx; double* obs; const double* obs_prev;    // the frame
    int* counts; int* info;                                                 // [n_streams][SWF_TRACKER_NCOUNT], [n_streams]
    const int* rm_first; const int* rm_ids; int* krm; int* nkrm;            // removeOutliers
    double cam[12];
};

#endif
