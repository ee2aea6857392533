// swf_gnssepoch.h — the single-epoch GNSS solve for a batch of epochs on the device: the seed mini-solve of
// SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:534-575) and the first fix of GnssProcess (:203-215) as one operator.  The
// definition is in include/swf_solver.h (swf_gnss_epoch_solve_batch).  Every raw GNSS factor is a scalar row on the position, the
// velocity, one clock and at most one ambiguity (R/factor/gnss_factor.cpp), so the Gauss-Newton system is an arrowhead:
//   a free ambiguity is seen by one row only: its Schur complement is zero, the row drops out and the ambiguity absorbs the
//     residual after the last iteration;
//   the clocks are diagonal among themselves and are eliminated as scalars;
//   what remains is [pos, vel], 6 x 6 at most, factored by Cholesky; with both constant every clock step is a weighted mean.
//
// Layout: one wavefront per epoch, GES_WPB epochs per workgroup; record i of a 64-record chunk in lane i % 64.  Loads by
// dependency level: `first`, then the records and the epoch's state.  Per chunk and iteration the lanes' contributions to the
// normal equations are summed by a reduce-scatter (ges_reduce): at every halving step a lane keeps half of its quantities and hands
// the other half to its partner, so K quantities cost K shuffles instead of 6 K and quantity k ends in lane k * 64 / K.  Five such
// sums per chunk with [pos, vel] free (27 entries of the [pos, vel] block; 8 per clock, four clocks to a sum; the thirteenth clock),
// one with both constant (the 13 clock diagonals and gradients).  Chunks are added in ascending order.  The elimination, the 6 x 6
// Cholesky and the back-substitution run on wave-uniform values read with readlane.  No LDS, no barrier, no atomics: a wavefront's
// result cannot depend on its neighbours in the workgroup or on the other epochs of the call, and every sum runs in a fixed order.
//
// Two instances: RES = true keeps the (<= 64) records of the epoch in registers across the iterations, RES = false re-reads each
// chunk from L2 in every pass (<= SWF_GES_NMAX records).  Both run the same chunk loop over the same inlined functions and
// floating-point contraction is off in swf_gnssepoch.hip, so an epoch's results are bit-identical whichever runs it.
#ifndef SWF_GNSSEPOCH_H
#define SWF_GNSSEPOCH_H

#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

enum { GES_WPB = 4 };                 // wavefronts (= epochs) per workgroup

struct GnssEpochArgs {
    int n_epochs;
    const int* first;                                                        // [n_epochs + 1]
    const double* pos; const double* vel; const double* base;                // [n_epochs][3]
    const double* clock;                                                     // [n_epochs][SWF_GES_CLOCKS]
    const int* mode; const int* clk_const;                                   // [n_epochs]
    const double* dat; const int* rec;                                       // [n][SWF_GES_DOUBLES], [n][4] = kind, clock slot, state, 0
    int max_iter; double step_tol, eps_rank;
    double* pos_out; double* vel_out; double* clock_out;                     // [n_epochs][3], [3], [SWF_GES_CLOCKS]
    double* N_out; double* r_out;                                            // [n]
    double* cost; int* iters; int* status;                                   // [n_epochs]
    int* clk_rows; double* info;                                             // [n_epochs][SWF_GES_CLOCKS], [n_epochs][36]
};

// enqueue k_gnss_epoch<resident> on stream st (resident: every epoch has <= 64 records)
int swf_internal_gnss_epoch_launch(const GnssEpochArgs& A, bool resident, hipStream_t st);

#endif
