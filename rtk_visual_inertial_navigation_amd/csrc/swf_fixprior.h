// swf_fixprior.h — fix and hold on the device: the accepted integers of an ambiguity search folded into a linear prior, the second half
// of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:249-355): a MarginalizationInfo over the current prior plus one
// FixedIntegerFactor(round(F), istd) per double difference and one FixedIntegerFactor(0, istd) per reference ambiguity, each attached
// to a hidden offset tf per (system, frequency), the tf eliminated by marginalize(false, true).
//
// The operator.  Prior r(x) = r0 + J dx(x, x0), J n x n row-major; constraint rows (c_i, g_i, v_i): c = the prior-local
// coordinate of a one-dimensional kept block, g = its group (rows of one group share one tf), v = its value.  With r the prior's
// residual at the new linearisation point:
//   A0 = J^T J, b0 = J^T r;   per group with members c_1 .. c_k:  A'[c_a, c_b] = A0[c_a, c_b] + istd^2 (delta_ab - 1 / k),
//                                                                 b'[c_a]      = b0[c_a]      - istd^2 (v_a - mean(v))
// which IS the Schur elimination of the tf (they are mutually independent: their block is diag(k_g istd^2)); then (J', r0') = the
// square root of (A', b') in the two forms of swf_batch_marginalize, and x0' = the new point.
//
// k_fix_prior: one 1024-thread workgroup per problem, n <= MG_MAXN = 140, everything fp64, every sum in a fixed order, no atomics on
// data.  Phases: [BATCH: rows from the search's device buffers, dx and r = r0 + J dx from the device state] -> J to LDS -> Gram in
// 4 x 4 register tiles over the lower triangle -> group update -> root: SWF_PRIOR_CHOLESKY a right-looking Cholesky in LDS,
// SWF_PRIOR_EIGEN the pivoted Cholesky + one-sided Jacobi of the marginalisation consumer (swf_rootdev.h: d_pivoted_chol,
// d_jacobi_sweeps, d_eigen_root_out — the same device functions, not copies).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"
#include "swf_dev.h"

#define FXP_MAXN 140                      // = MG_MAXN: the largest matrix the eigen root keeps in LDS

// per window of swf_batch_fix_prior (host-built at the call)
struct FixWin {
    int gf;                               // generic-factor id of the prior to update
    int col0;                             // first entry of the window's tail-coordinate -> prior-column table in FixPriorArgs::tailcol
    int n_use;                            // pairs of the search to take (the first n_use)
    int enable;
};

struct FixPriorArgs {
    int n_prob, form;
    double istd, eps;
    // stand-alone: problems concatenated (dim^2 / dim doubles each, in order)
    const int* dim; const double* J; const double* r;
    const int* row_first; const int* rows; const double* vals;      // rows [.][2] = coordinate, group
    // outputs.  Stand-alone: concatenated like the inputs.  BATCH: slabs of ldn^2 / ldn / ldx doubles per window.
    double* A; double* b; double* Jn; double* r0; double* eig; int* rank;
    // BATCH only
    const FixWin* fw; const int* tailcol;
    const int* pair_first; const int4* pairs; const double* rec; int rec_ld;      // the search's device buffers (swf_lambda.h)
    int ignore_ratio, scalars_at_zero, ldn, ldx;
    double* x0n; int* applied;
};

// enqueue k_fix_prior<batch> on stream st (swf_fixprior.hip); B is read on the batch path only
int swf_internal_fix_prior_launch(const FixPriorArgs& P, const DevBatch& B, bool batch, hipStream_t st);
// enqueue k_fix_install: (J', r0', x0') of the applied windows into the batch's own prior records and what derives from them
int swf_internal_fix_install_launch(const FixPriorArgs& P, const DevBatch& B, hipStream_t st);
// the checks of the operator's definition on host-resident rows ([.][2] = coordinate, group) of one problem of dimension n: 0 or a
// negative SWF_E_* (message set); `who` names the entry point in the message
int swf_internal_fix_rows_check(int n, int nrows, const int32_t* rows, const char* who);
