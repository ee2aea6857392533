// swf_phasescreen.h — the pre-fit carrier-phase screen: the numeric core of the first half of SWFOptimization::GnssPreprocess
// (R/swf/swf_gnss.cpp:337-499) for a batch of epochs on the device.  Per epoch, to the letter of the reference:
//   masking    el < AZELMIN zeroes the phase (:351-353); the record still takes part in the median (:354-362)
//   residual   the un-weighted RTKCarrierPhaseFactor (R/factor/gnss_factor.cpp:105-138, use_istd = false) at the predicted pose,
//              r = distance(pos + base, sat) - N lam - L_lam + dt (:354-379), with the distance() of swf_gnss_range.h
//   median     per (kind, group = sys * 2 + f) over the continuing ambiguities, sorted[size / 2] (:381-394)
//   decisions  |r - median| > lam / 2 (RTK, :406-414) or > lam (rover-only phase, :425), code minus phase beyond
//              10 m / sin^2(el) (:419), and which ambiguities are created anew (:432-472)
// The PBtype bookkeeping itself (:434-444, :455-465, :474-495) stays with the caller: it is list surgery on host objects.
//
// Layout: one wavefront per epoch, SCR_WPB epochs per workgroup; record i of the epoch in lane i % 64, slot i / 64, in registers.
// Loads by dependency level: `first`, then the epoch's records, pos, base and mode.  The median is found by counting: per
// (kind, group) the members' lanes come from __ballot, every member's residual is broadcast with readlane, and each member
// counts the members that sort before it (ties by record index, NaN last); the member of rank cnt / 2 publishes the median.
// The reset list is compacted in the same wavefront: ballot, then a popcount prefix, 64 flags at a time.  No LDS, no barrier,
// no atomics: a wavefront's result cannot depend on its neighbours in the workgroup or on the other epochs of the call.
//
// Two instances: SLOTS = 1 (epochs of <= 64 records) and SLOTS = 4 (<= SWF_SCR_NMAX = 256); the arithmetic of a record is one
// inlined function in both and floating-point contraction is off in swf_phasescreen.hip, so an epoch's results are bit-identical
// whichever runs it.
#ifndef SWF_PHASESCREEN_H
#define SWF_PHASESCREEN_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { SCR_WPB = 4 };                 // wavefronts (= epochs) per workgroup
enum { SCR_SETS = 2 * SWF_SCR_GROUPS };       // median sets per epoch: kind * SWF_SCR_GROUPS + group

struct PhaseScreenArgs {
    int n_epochs;
    const int* first;                 // [n_epochs + 1]
    const double* pos; const double* base; const int* mode;      // [n_epochs][3], [n_epochs][3], [n_epochs]
    double el_min;
    const double* dat; const int* rec;                           // [n][SWF_SCR_DOUBLES], [n][4] = kind, group, state, partner
    double* r; unsigned char* flags;                             // [n]
    double* med; int* cnt;                                       // [n_epochs][2][SWF_SCR_GROUPS]
    int* reset; int* n_reset;                                    // [n] (an epoch's run starts at first[e]; -1 beyond n_reset[e]), [n_epochs]
};

// enqueue k_phase_screen<slots> (slots = 1: every epoch has <= 64 records; 4: <= SWF_SCR_NMAX) on stream st
int swf_internal_phase_screen_launch(const PhaseScreenArgs& A, int slots, hipStream_t st);

#endif
