// swf_ddselect.h — the choice of the double-difference pairs of the integer ambiguity search on the device: the reference election
// of FindReferenceSatellites (R/swf/swf_lambda.cpp:8-53) and the loop of SWFOptimization::LambdaSearch that builds D3 (:118-188).
// Per window, to the letter of the reference:
//   epochs     newest first; the `use` marks of the ambiguities carry over from an epoch to the older ones (:118-126)
//   election   per class = sys * 2 + f: the candidates are the epoch's observations of the class whose ambiguity is not used, in
//              observation order; cost_j = sum_i |s - round(s)|, s = y_i - y_j, added left to right, the i == j term included (:27-35);
//              the reference is the LAST candidate whose cost equals the minimum (:41-46: every equal entry overwrites)
//   pairs      every other unused observation of a class with a reference is marked used BEFORE the gate (:146), then paired with
//              the reference iff |d - round(d)| < gate, d = y_k - y_ref (:163); a reference is never marked
//   go         tail >= 6, last_count + last_ref_count >= 6, last_count >= 4, at least 4 pairs (:96, :178, :184)
// round is C round (halves away from zero), written out as trunc and a compare so that every instance rounds alike.
// All arithmetic is subtraction, round, fabs, addition and comparison; floating-point contraction is off in swf_ddselect.hip.
//
// Layout: one wavefront (= one workgroup) per window; the window's epochs run one after the other in that wavefront because the
// used marks carry over.  Per epoch the records (class, t, y, candidate) are staged in LDS; lane j accumulates cost_j with a
// sequential loop over the epoch's records in order (LDS broadcast reads), lanes striding over j for epochs beyond 64 records;
// the election is a wave reduction on (cost ascending, index descending) per class; the pairs are appended in observation order,
// 64 records at a time, with a ballot and a popcount prefix.  The used marks are a bitmap of DDS_TMAX bits in LDS.  No atomics
// on global memory: a window's result cannot depend on the other windows of the call.
//
// BATCH = true is swf_batch_select_ambiguity_pairs: y is read from the device state through a host-built state index per
// observation, and the pairs are also written as the (ta, tb, xa, xb) records of k_lambda<true> into the window's 64-slot range
// of the search's pair table, with the pair count the selected search reads.
#ifndef SWF_DDSELECT_H
#define SWF_DDSELECT_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { DDS_NMAX = SWF_DDSEL_NMAX };          // observations per epoch
enum { DDS_TMAX = SWF_DDSEL_TMAX };          // tail coordinates per window (the used bitmap: 64 words of LDS)
enum { DDS_CLASSES = 6 };

struct DdSelectArgs {
    int n_windows;
    const int* epoch_first; const int* obs_first; const int* obs;     // [n_windows + 1], [n_epochs + 1], [n_obs][2] = class, t
    const int* y_first; const double* y;                              // stand-alone: [n_windows + 1], the tails' float values
    const double* gate;                                               // [n_windows]
    int* pairs; int* counts; int* refs; double* cost; unsigned char* role;   // outputs, any of which may be null (see swf_solver.h)
    // BATCH only
    const int* tail; const int* xidx; const double* x;                // tail dimension [n_windows], state index [n_obs], the device state
    int4* am_pairs; int* am_first; int* pair_count;                   // [n_windows][64], [n_windows + 1] = 64 w, [n_windows] (0 unless SWF_DDSEL_OK)
};

// enqueue k_dd_select<batch> for A.n_windows windows on stream st (swf_ddselect.hip)
int swf_internal_dd_select_launch(const DdSelectArgs& A, bool batch, hipStream_t st);
// the rejections of host-resident inputs (tail[w] = the tail dimension of window w); SWF_OK or the code with the message set
int swf_internal_dd_select_check(const char* who, int n_windows, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs,
                                 const int32_t* tail, const double* gate);

#endif
