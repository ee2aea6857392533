/*
 * swf_solver.h — C-ABI of the MI355X-native sliding-window Gauss-Newton solver.
 *
 * This is the drop-in boundary for the reference's L4<->L2 line: what
 * SWFOptimization does through ceres::Problem / ceres::Solver / the modified-Ceres
 * private globals, it does here through opaque handles and plain pointers.  No C++ or
 * torch types cross the boundary.  All functions return 0 on success, a negative
 * SWF_E_* code otherwise; the library never falls back to a CPU path: if no HIP device
 * is usable, every compute entry point returns SWF_E_NODEVICE.
 *
 * Two layers:
 *   (1) swf_batch_*   — the engine: a batch of flat windows (include/swf_types.h) resident
 *                       in HBM, solved together.  The batch-throughput path (BASELINE cfg4)
 *                       and what bench.py times.
 *   (2) swf_problem_* — the pointer-keyed, ceres::Problem-shaped surface for one window
 *                       (the single-window latency path).  It flattens to (1) with B = 1.
 *
 * R/ = /root/reference/rtk_visual_inertial_src/rtk_visual_inertial/src/
 */
#ifndef SWF_SOLVER_H
#define SWF_SOLVER_H

#include <stddef.h>
#include <stdint.h>
#include "swf_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SWF_OK = 0,
    SWF_E_NODEVICE = -1,      /* no usable HIP device / HIP runtime error */
    SWF_E_INVALID = -2,       /* bad argument / malformed window */
    SWF_E_UNSUPPORTED = -3,   /* structure outside what the kernels cover */
    SWF_E_NOTFOUND = -4,      /* unknown parameter block / factor id */
    SWF_E_STATE = -5          /* call order violated (e.g. export before solve) */
};

/* library / device info */
/* 100 + the number of ABI revisions.  104 (round 4): swf_timing grew by lm_schur_flops_sym / lm_schur_mfma (swf_batch_timing writes
 * sizeof(swf_timing) bytes: a caller compiled against an older header must be rebuilt); swf_composite_assemble / _add_mid_prior stride
 * HpN / HNN by N_cap; after an optimising solve swf_get_reduced / swf_batch_export_reduced return L zero outside the parameter_head tail
 * block (the whole factor only after step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY); swf_prior_reset_linearization_point added.
 * 105 (round 5): no layout change; a composite IMU-GNSS factor may touch one block of elimination group 0 (MyOrdering's own order), which
 * 104 refused with SWF_E_UNSUPPORTED; SWF_PRIOR_EIGEN keeps every direction of information above eps on healthy windows.
 * 106 (round 6): swf_options::reserved became swf_options::composite_root (same offset and size; 0 = the previous behaviour); the
 * environment variable SWF_COMP_EIGEN_ROOT is gone, as are the A/B kernels behind SWF_CHOL_RR2 / RR3 / V1, SWF_ASM_OLD, SWF_POST_*.
 * Structural limits of a group-0 clique (a non-landmark block of elimination group 0 with the factors touching it): at most 9 eliminated
 * dimensions d_e, at most 768 columns d = d_e + d_f, and — for cliques beyond one wavefront's 64 x 64 / 96 x 64, which take the
 * workgroup kernel — d_e * d <= 1536 (d <= 170 at d_e = 9, 256 at d_e = 6, 512 at d_e = 3): SWF_E_UNSUPPORTED beyond.
 * 107: no layout change; the LAMBDA integer ambiguity search on the device: swf_lambda_batch (stand-alone, RTKLIB's lambda() for a batch
 * of problems) and swf_batch_ambiguity_search / swf_batch_get_ambiguity_fix (LambdaSearch's numeric core after
 * swf_batch_tail_covariance, ratio test included).
 * 108: no layout change; the post-solve feature check on the device: swf_batch_check_features / swf_batch_get_feature_check
 * (OutliersRejection's mean reprojection error and Double2Vector's depth sign per feature, the rejected list compacted on the
 * device), swf_problem_check_features / swf_problem_get_feature_check / swf_problem_rejected_features by parameter-block key.
 * Round 8 (still 108, no ABI change): the final linearisation of an optimising solve forms the gradient alone (no group-0 inverses; the
 * reduced system of that pass was never solved or exported).  Test aids read once at swf_batch_create, next to SWF_NO_SPEC_EVAL and the
 * other launch-shape knobs: SWF_FULL_FINAL_ELIM=1 restores the complete elimination in that pass (bit-identical results);
 * SWF_LS_GRAD_QPB=1|2|4|8|16 sets the landmark parts per workgroup of its landmark kernel (a measuring aid, as SWF_LS_QPB is).
 * 109: no layout change; fix and hold on the device: swf_prior_fix_batch (stand-alone: a linear prior plus fixed-integer constraints whose
 * hidden offsets are eliminated in closed form, re-rooted), swf_batch_fix_prior / swf_batch_get_fixed_prior / swf_batch_install_fixed_prior
 * (the second half of LambdaSearch behind swf_batch_ambiguity_search, the new prior written into the resident batch without a rebuild),
 * swf_problem_fix_prior by parameter-block key.  A linear prior may keep blocks of the parameter_head tail.
 * 110: no layout change; the pre-fit carrier-phase screen on the device: swf_phase_screen_batch (stand-alone: GnssPreprocess's residuals at
 * the predicted pose, their medians per constellation and frequency, the slip flags and the compacted list of ambiguities to re-create).
 * 111: no layout change; the single-epoch GNSS solve on the device: swf_gnss_epoch_solve_batch (stand-alone: the seed mini-solve of
 * GnssPreprocess and the first fix of GnssProcess for a batch of epochs, one wavefront each).
 * 112: no layout change; the double-difference pairs of the ambiguity search chosen on the device: swf_dd_select_batch (stand-alone:
 * FindReferenceSatellites and LambdaSearch's D3 loop for a batch of windows, one wavefront each), swf_batch_select_ambiguity_pairs /
 * swf_batch_ambiguity_search_selected / swf_batch_get_ambiguity_pairs (solve, tail covariance, pair selection, LAMBDA and ratio test as
 * one enqueue).  swf_batch_ambiguity_search with host pairs is unchanged.
 * 113: no layout change; swf_batch_export_step, the debug / parity export of the last proposed step (next to swf_batch_export_vectors).
 * swf_abi_sizes reports sizeof(swf_options), sizeof(swf_summary), sizeof(swf_timing), sizeof(swf_flat_window), sizeof(swf_iteration) so a binding can check its own. */
int swf_version(void);
int swf_abi_sizes(int32_t out[5]);
int swf_device_count(int32_t* n);                 /* hipGetDeviceCount */
int swf_set_device(int32_t device);               /* hipSetDevice: the device of the batches / problems created next on this thread */
void swf_default_options(swf_options* opt);       /* Solver::Options as the reference sets them for the window solves (R/swf/swf.cpp:25-30: DENSE_SCHUR, DOGLEG,
                                                      8 iterations, jacobi_scaling = false) + the public Ceres 2.x defaults of SURVEY.md App. C */
const char* swf_last_error(void);                 /* thread-local message for the last failure */

/* =====================================================================================
 * (1) batch engine
 * ===================================================================================== */
typedef struct swf_batch swf_batch;

/* Build the static (symbolic) structure for n windows and upload structure + state to the
 * current device.  The windows' arrays are read during this call only; their pose/sb/lm/sc
 * pointers are remembered for swf_batch_download_state().  `stream` is a hipStream_t (or
 * NULL for the default stream) on which every later operation of this batch is enqueued. */
int swf_batch_create(const swf_flat_window* const* windows, int32_t n, void* stream, swf_batch** out);

/* ---- several GPUs of one node from ONE process (SURVEY.md 8b "batch API swf_solve_batch(handles[], n, device_mask)", 8e "one host
 * thread + one HIP stream per GPU").  Windows are independent units: they are dealt to the devices in contiguous blocks, there is no
 * data-path collective, and because swf_batch_solve only enqueues, one host thread drives every device.  A batch remembers its device;
 * every swf_batch_* call switches to it for its duration (and back), so batches of different devices may be used from the same thread.
 *   swf_batch_create_on       swf_batch_create on the given device (the caller's current device is left as it was).
 *   swf_batch_create_sharded  windows [0, n) in near-equal contiguous blocks over the devices of device_mask (bit d = device d, 0 = all
 *                             visible devices); out_batches / out_first / out_count need room for one entry per selected device.
 *   swf_solve_batches         swf_batch_solve on every batch, then swf_batch_sync on every batch: the node-level Solve.
 *   swf_batch_device          the device a batch lives on.
 *   swf_shard_partition       the block partition swf_batch_create_sharded applies (and the multi-process harness, shard.py).
 * This replaces the reference's single CPU solve loop (R/swf/swf_image.cpp:198-251) only for the batch-throughput path; the single-window
 * latency path stays on one GPU. */
int swf_batch_create_on(int32_t device, const swf_flat_window* const* windows, int32_t n, void* stream, swf_batch** out);
int swf_batch_create_sharded(const swf_flat_window* const* windows, int32_t n, uint32_t device_mask,
                             swf_batch** out_batches, int32_t* out_first, int32_t* out_count, int32_t* n_batches);
int swf_solve_batches(swf_batch* const* batches, int32_t n, const swf_options* opt);
int swf_batch_device(swf_batch* b, int32_t* device);
int swf_shard_partition(int32_t n, int32_t G, int32_t k, int32_t* first, int32_t* count);   /* shard k of G: the first n % G shards take one more (host only) */
int swf_batch_destroy(swf_batch* b);

/* Re-upload the parameter blocks from the windows' host arrays (new epoch, same structure):
 * the analogue of Vector2Double() before ceres::Solve (R/swf/swf.cpp:140, swf_image.cpp:202). */
int swf_batch_upload_state(swf_batch* b);
/* Device-side restore of the state uploaded last (so a benchmark can re-solve the same
 * windows with inputs resident in HBM). */
int swf_batch_reset_state(swf_batch* b);

/* Enqueue one full solve of every window (= ceres::Solve, R/swf/swf_image.cpp:219):
 * options.step_mode selects OPTIMIZE or ASSEMBLE_ELIMINATE_ONLY (= is_optimize=false,
 * R/swf/swf_image.cpp:404-416).  Asynchronous on the batch stream; no host round-trip
 * happens inside (accept/reject, trust-region radius and convergence live on the device). */
int swf_batch_solve(swf_batch* b, const swf_options* opt);
/* Block until the stream has drained. */
int swf_batch_sync(swf_batch* b);

/* Copy parameter blocks back into the windows' host arrays (Double2Vector, R/swf/swf.cpp:188). */
int swf_batch_download_state(swf_batch* b);
/* Per-window summaries incl. iteration trace; out[n]. */
int swf_batch_summaries(swf_batch* b, swf_summary* out);

/* Export of the reduced system of window w from the LAST linearisation, the analogue of
 * ceres::internal::{lhs_out, rhs_out, lhs_out2, hs_row} (R/swf/swf_gnss.cpp:25-94):
 *   S   hs_row x hs_row row-major, full symmetric (damping included as solved)
 *   rhs hs_row
 *   L   hs_row x hs_row row-major lower Cholesky factor, S = L L^T, in elimination order;
 *       its trailing tail_dim x tail_dim block L_nn gives L_nn L_nn^T = marginal information
 *       of the parameter_head states (R/swf/swf_gnss.cpp:85-87).
 *       After a solve with step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY (UpdateSchur's and the marginalisation's mode) L is the
 *       whole factor.  After an optimising solve of a system of up to 256 dimensions (240 up to library version 104) only the block the reference reads then
 *       (UpdateSchurHessianOnly, R/swf/swf_gnss.cpp:65-94) is kept: rows and columns from the 16-aligned index at or before the
 *       parameter_head tail; the rest is returned as zero (the factor lives in registers and is not written to HBM on solve
 *       paths).
 * Any pointer may be NULL.  hs_row is summary.reduced_dim. */
int swf_batch_export_reduced(swf_batch* b, int32_t w, double* S, double* rhs, double* L);
/* Debug/parity export of local-space vectors of window w (n_loc doubles each, ordering
 * order): gradient J^T r, squared column norms, and y = (J^T J + D)^-1 J^T r. */
int swf_batch_export_vectors(swf_batch* b, int32_t w, double* grad, double* diag, double* y);
/* Debug/parity export of the step of window w (n_loc doubles, ordering order, as swf_batch_export_vectors): the local-space
 * increment of the candidate the LAST trust-region iteration proposed, x_candidate = Plus(x, step) — the dogleg step (Gauss-Newton,
 * clipped Cauchy or interpolated) or Levenberg-Marquardt's -y, exactly as the step kernel stored it.  For a vector block x_new - x
 * recovers it only to half an ulp of x (nothing, for an ambiguity of 1e7 cycles moved by 1e-6): this is what the entrywise step
 * tests read.  A stream synchronisation and one copy; not on any solve path.  SWF_E_STATE unless the last solve was an optimising
 * one (step_mode = SWF_OPTIMIZE); zero for a window whose solve proposed no step. */
int swf_batch_export_step(swf_batch* b, int32_t w, double* step);
int swf_batch_dims(swf_batch* b, int32_t w, int32_t* n_loc, int32_t* n_e, int32_t* n_red);
/* Debug/parity export of the LAST linearisation of window w, factor by factor: the residual vector r [n_res] and the dense
 * Jacobian J [n_res][n_loc] (row-major; columns = local coordinates in elimination order, as swf_batch_export_vectors) exactly
 * as the device holds them — loss-corrected (CauchyLoss corrector, R/factor/marginalization_factor.cpp:23-45), whitened.
 * Rows: the window's projection factors in the caller's order (2 rows each), then imu (15 each), cp, pr, dop, sp, spr, scp,
 * fix (1 each), idp (2 each), the linear priors (dim each), the composite factors (30 + N each, as rewritten by their last
 * re-elimination).  Columns of constant blocks do not exist.  r / J may be NULL (then only the sizes are returned).  A solve
 * with step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY leaves the linearisation at the uploaded state.  Not on any solve path: this is
 * what the parity tests compare with numpy factor code and finite differences, and what their dense normal equations are
 * assembled from. */
int swf_batch_export_jacobian(swf_batch* b, int32_t w, double* r, double* J, int32_t* n_res, int32_t* n_loc);

/* Marginalisation consumer: what the reference does with the export of an is_optimize = false solve —
 * SWFOptimization::UpdateSchur (R/swf/swf_gnss.cpp:25-61) followed by MarginalizationInfo::setmarginalizeinfo(..., Sqrt =
 * true) (R/factor/marginalization_factor.cpp:449-488).  Valid after a solve with step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY.
 * For every window, with n = the local dimension of its parameter_head tail:
 *   A  n x n   marginal information of the tail  (= S_nn - S_nm S_mm^-1 S_mn = L_nn L_nn^T)
 *   bv n       its right-hand side               (= b_n  - S_nm S_mm^-1 b_m), sign convention b = J^T r
 *   J  n x n, r0 n : the new linear prior r = r0 + J dx with J^T J = A, J^T r0 = bv:
 *     SWF_PRIOR_EIGEN     J = sqrt(Lambda+) V^T (rows by ascending eigenvalue), r0 = Lambda+^-1/2 V^T bv, eigenvalues <= eps
 *                         dropped — the reference's form; rank = number kept.  Eigenvector signs are not defined.
 *     SWF_PRIOR_CHOLESKY  J = L_nn^T, r0 = L_nn^T y_n: the same quadratic without an eigen-decomposition (rank = n).
 * The reference pseudo-inverts S_mm through an eigen-decomposition with threshold 1e-8; this library uses the Cholesky
 * factor of the solve, which is the same thing whenever S_mm is positive definite.  A marginal that is SINGULAR on the kept
 * states (an unobservable extrinsic, a direction nobody measured) is normal in the reference — its eigen square root drops
 * the null directions — while the factorisation of the whole S breaks down in the tail of such a window (the solve reports
 * SWF_LINEAR_SOLVER_FAILURE): SWF_PRIOR_EIGEN then re-factors the first m columns only and takes a rank-revealing factor of
 * A (rank < n is reported, the prior is valid); SWF_PRIOR_CHOLESKY has no such variant and reports rank -1.  A breakdown
 * inside S_mm itself is a failure in both forms (rank -1, no silent fallback).  Both forms: n <= SWF_MAX_TAIL_DIM = 640, the limit
 * of the tiled factorisation of the reduced system itself (SWF_PRIOR_EIGEN: the Jacobi iteration keeps its matrix in LDS up to n = 140; above
 * that it is a block Jacobi over many workgroups on an HBM scratch, 8-column blocks up to 576 dimensions, 4-column blocks to 640).  A
 * healthy window's eigen form keeps every direction whose information exceeds eps (the pivoted Cholesky that preconditions the sweeps
 * runs down to pivots of eps / (16 n), whatever the largest diagonal entry).  Asynchronous on the batch stream up to tails of 140 dimensions; SWF_PRIOR_EIGEN above that (the block-Jacobi
 * schedule over many workgroups) is SYNCHRONOUS: the host reads the rotation counters back every few sweeps to stop enqueueing, so the
 * call blocks the calling thread until the priors exist. */
enum { SWF_PRIOR_EIGEN = 0, SWF_PRIOR_CHOLESKY = 1 };
#define SWF_MAX_TAIL_DIM 640
#define SWF_MAX_COMPOSITE_AMBIGUITIES 64
int swf_batch_marginalize(swf_batch* b, double eps, int32_t form);
/* Results of the last swf_batch_marginalize for window w (synchronises).  Any pointer may be NULL; eig receives the n
 * eigenvalues (ascending; for SWF_PRIOR_CHOLESKY the squared diagonal of L_nn). */
int swf_batch_get_prior(swf_batch* b, int32_t w, double* A, double* bv, double* J, double* r0, double* eig, int32_t* n, int32_t* rank);

/* Ambiguity covariance hand-off, for every window of the batch, after ANY solve:
 *   A  = L_nn L_nn^T   information of the parameter_head states — what SWFOptimization::UpdateSchurHessianOnly forms from
 *                      lhs_out2 (R/swf/swf_gnss.cpp:65-94);
 *   Qy = A^-1          their covariance — what SWFOptimization::LambdaSearch computes next (R/swf/swf_lambda.cpp:94-99) and feeds,
 *                      with the float ambiguities, to the LAMBDA search.  The search runs on the device too:
 *                      swf_batch_ambiguity_search below takes Qy from here without a host round trip.
 * L is the Cholesky factor of the last linear solve of each window (it includes the dogleg's mu * diag regularisation, as the
 * exported lhs_out2 does).  n_red <= 512.  swf_batch_tail_covariance is asynchronous; the getter synchronises; both matrices
 * are n x n row-major, n = tail dimension; *n = -1 and SWF_E_STATE for a window without a valid factor. */
int swf_batch_tail_covariance(swf_batch* b);
int swf_batch_get_tail_covariance(swf_batch* b, int32_t w, double* A, double* Qy, int32_t* n);

/* Integer ambiguity resolution: the numeric core of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:82-365) for every window,
 * on the device (swf_lambda_batch's kernel with a gather prologue and a ratio-test epilogue).  Needs a swf_batch_tail_covariance
 * issued after the last solve (SWF_E_STATE otherwise).
 *   pair_first [n_windows + 1], pairs [pair_first[n_windows]][2]   host arrays: window w owns pairs pair_first[w] ..
 *             pair_first[w+1]-1; a pair is (tail coordinate of an ambiguity, tail coordinate of its reference ambiguity) — one row
 *             of the reference's D (:164-166).  An index outside the tail, a == b, or a coordinate of a tail block whose size is not
 *             1: SWF_E_INVALID; more than SWF_LAMBDA_NMAX pairs in a window: SWF_E_UNSUPPORTED.
 * Then, asynchronously on the batch stream, per window with n_b pairs:
 *   Qb = D Qy D^T (n_b x n_b, from the tail covariance), bf = D y (y = the device state of the tail blocks at call time),
 *   the LAMBDA search with m = 2 (F, s, info as swf_lambda_batch), and the ratio test (:208-253):
 *     S = {i : |F1_i - F2_i| < 1e-2}, same_cost = e_S^T Qb_SS^-1 e_S with e = F1 - bf, s1' = s[1] - same_cost,
 *     s0' = s[0] - same_cost (1e-3 when |s0'| < 1e-3), ratio = {s[1] / s[0], s1' / s0'},
 *     fixed = s[0] <= 0 || ratio[0] >= ratio_threshold || ratio[1] >= ratio_threshold   (the reference's threshold is 2).
 *   A window without pairs or without a valid tail covariance reports SWF_LAMBDA_NO_INPUT.
 * The getter synchronises; its first call after a search copies every window's results to the host in one transfer, later calls
 * read that copy.  Every pointer may be NULL.  F [2][n_b] (candidate j at F[j * n_b + i]), s [2], ratio [2], fixed [1],
 * Qb [n_b][n_b] row-major and bf [n_b] (the search's own inputs, so that a caller can replay them), n_b, info (SWF_LAMBDA_*).
 * ratio / fixed are 0 unless info == SWF_LAMBDA_OK.  The search results are invalidated by the next swf_batch_solve
 * (SWF_E_STATE).  Stays with the caller of THIS entry point: the choice of the reference satellites and the fractional-part gating of
 * D's rows (:163), the early returns on too few rows (:178, :184) — swf_batch_select_ambiguity_pairs below makes them on the device —
 * and the fix counter.  The new prior of FixedIntegerFactors (:250-355) is swf_batch_fix_prior below. */
int swf_batch_ambiguity_search(swf_batch* b, const int32_t* pair_first, const int32_t* pairs, double ratio_threshold);
int swf_batch_get_ambiguity_fix(swf_batch* b, int32_t w, double* F, double* s, double* ratio, int32_t* fixed,
                                double* Qb, double* bf, int32_t* n_b, int32_t* info);

/* The pairs of the search chosen on the device (the operator of swf_dd_select_batch, which see, on the batch's own state): with it
 * solve -> tail covariance -> pair selection -> LAMBDA -> ratio test is one uninterrupted enqueue.
 * swf_batch_select_ambiguity_pairs needs a solve (SWF_E_STATE otherwise) and is asynchronous on the batch stream; epoch_first, obs_first,
 * obs and gate are host arrays as for swf_dd_select_batch, t being a coordinate of the window's parameter_head tail, and y the device
 * state at that moment, as in the search.  Refused with SWF_E_INVALID before anything is enqueued: what swf_dd_select_batch refuses, and
 * a t on a tail block whose size is not 1; more than SWF_DDSEL_NMAX observations in an epoch or a tail beyond SWF_DDSEL_TMAX:
 * SWF_E_UNSUPPORTED.  The pairs go into window w's 64-slot range of the search's own device pair table, with a device pair count that is
 * 0 unless the window's info == SWF_DDSEL_OK (the reference's early returns).  A selection replaces the pair table: results of an
 * earlier search or fix_prior are invalidated (SWF_E_STATE from their getters).
 * swf_batch_ambiguity_search_selected needs a selection after the last solve and a tail covariance (SWF_E_STATE otherwise) and runs the
 * search of swf_batch_ambiguity_search on the selected pairs: every field swf_batch_get_ambiguity_fix returns equals, bit for bit, what
 * swf_batch_ambiguity_search returns for the same pairs passed from the host.  A window whose count is 0 reports SWF_LAMBDA_NO_INPUT.
 * swf_batch_get_ambiguity_pairs synchronises; its first call after a selection copies every window's selection in one transfer per
 * array.  pairs [64][2], counts [4], refs [epochs of w][6], cost / role [observations of w], as swf_dd_select_batch; any may be NULL.
 * swf_batch_fix_prior after a selected search reads the selection back in the same way (n_use: the reference takes counts[1] =
 * last_count).  The reference's host reads `fixed` for its fix counter at that point anyway: this is the one synchronisation of the chain.
 * A new solve, a state upload, a state reset or a swf_batch_ambiguity_search with host pairs invalidates the selection (SWF_E_STATE). */
int swf_batch_select_ambiguity_pairs(swf_batch* b, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs, const double* gate);
int swf_batch_ambiguity_search_selected(swf_batch* b, double ratio_threshold);
int swf_batch_get_ambiguity_pairs(swf_batch* b, int32_t w, int32_t* pairs, int32_t* counts, int32_t* refs, double* cost, uint8_t* role);

/* Fix and hold: the second half of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:249-355) for every window, on the device.  The
 * reference builds a MarginalizationInfo from the window prior, adds FixedIntegerFactor(ROUND(F), 1/0.03) per double difference and
 * FixedIntegerFactor(0, 1/0.03) per reference ambiguity, both on a hidden offset tf per (system, frequency), eliminates the tf with
 * marginalize(false, true) and makes the result the window prior.  Here (the operator of swf_prior_fix_batch, which see): needs a
 * swf_batch_ambiguity_search after the last solve (SWF_E_STATE otherwise); asynchronous on the batch stream.
 *   prior_sel [n_windows]  which LINEAR prior of the window to update (index among swf_flat_window::n_prior; NULL = prior 0).  A window
 *                          has no such prior (a composite factor's record is none): SWF_E_INVALID; its dimension > 140: SWF_E_UNSUPPORTED.
 *   n_use [n_windows]      take the first n_use[w] pairs of the search (NULL = all; the reference takes the newest epoch's, last_count)
 *   enable [n_windows]     0 = leave the window alone (NULL = all enabled; the host's fix counter stays with the caller)
 * Rows of window w, from the search's own device buffers: pair i < n_use[w] = (a, b) gives (coordinate of a, group b, v = ROUND(F1[i]));
 * every distinct b gives (coordinate of b, group b, v = 0).  A tail coordinate whose block the prior does not keep, or rows the operator
 * rejects (one coordinate twice): SWF_E_INVALID at the call, before anything is enqueued.  A window is APPLIED iff it is enabled with
 * n_use > 0, the search's info == SWF_LAMBDA_OK, and (ignore_ratio || fixed) — fixed is read on the device.  The prior's residual is
 * evaluated at the state swf_batch_download_state would return at that moment; scalars_at_zero != 0 evaluates every one-dimensional kept
 * block at 0 and returns 0 as its new linearisation point (PhaseBiasSaveAndReset / PhaseBiasRestore around the reference's call); with
 * scalars_at_zero == 0 the rows' values are taken relative to the scalars' current values (the prior and the constraints are linear in
 * scalars, so both settings describe the same quadratic).  Read-only until installed: a solve, export, marginalisation or
 * search issued afterwards is bit-identical with and without the call.
 * swf_batch_get_fixed_prior synchronises; its first call copies every window's results in one transfer per array.  A / J n x n row-major,
 * bv / r0 / eig n, x0 = the new linearisation point (global sizes concatenated in kept-block order), n = the prior's dimension, rank as
 * swf_batch_marginalize reports it (SWF_PRIOR_CHOLESKY on a singular A': -1 and not applied), applied 0 / 1.  Arrays of a window that was
 * not applied are not written.  Any pointer may be NULL.  Results are invalidated by the next swf_batch_solve or search (SWF_E_STATE).
 * swf_batch_install_fixed_prior writes (J', r0', x0') of every applied window into the batch's own record of that prior and everything
 * derived from it (the transposed record, the static prior clique's C = J^T J and its diagonal, accumulated in swf_batch_create's order:
 * the batch equals one freshly created with the new prior bit for bit); windows that were not applied keep their prior bit for bit.  The
 * next swf_batch_solve runs with the fix-and-hold prior, without a rebuild.  An install is a change of the batch's STRUCTURE data, not of
 * its state: swf_batch_upload_state and swf_batch_reset_state do not undo it (the windows' own prior_J / prior_r0 / prior_x0 arrays are
 * not touched either: fetch the new prior with the getter if the host keeps a copy). */
int swf_batch_fix_prior(swf_batch* b, const int32_t* prior_sel, const int32_t* n_use, const uint8_t* enable, int32_t ignore_ratio,
                        int32_t scalars_at_zero, double istd, double eps, int32_t form);
int swf_batch_get_fixed_prior(swf_batch* b, int32_t w, double* A, double* bv, double* J, double* r0, double* x0, double* eig,
                              int32_t* n, int32_t* rank, int32_t* applied);
int swf_batch_install_fixed_prior(swf_batch* b);

/* Post-solve feature check: what the reference does to every feature after every window solve — the depth-sign test of
 * SWFOptimization::Double2Vector (R/swf/swf.cpp:214-229) and the mean reprojection error of OutliersRejection
 * (R/swf/swf_image.cpp:255-308) — for every window, on the device, without moving the state to the host.  Read-only: it reads the
 * state swf_batch_download_state would return at that moment (after a solve the accepted point; after swf_batch_upload_state /
 * swf_batch_reset_state the uploaded one) and writes nothing a solve, an export, a marginalisation or an ambiguity search reads.
 * Features of window w, in this order: its n_lm world-point landmarks in pool order, then its inverse-depth features = the distinct
 * scalar-pool blocks idp_idx[][4] names, ascending.  Per feature, with P_j = p_j - R_j pbg and R from the normalised quaternion:
 *   world point X       for each of its projection factors k (frame j, extrinsic e, image point uv) in the caller's factor order:
 *                       pc = R_e^T (R_j^T (X - P_j) - t_e), err_k = |pc.xy / pc.z - uv|; mean_err = (sum err_k) / n_obs, summed left
 *                       to right; depth = pc.z of its first factor.
 *   inverse depth lam   anchor pose i and anchor point pts_i from its factors: X = R_i (R_ex (pts_i / lam) + t_ex - pbg) + p_i, then
 *                       the same error for every factor with its pts_j (kinds 1 / 2 in the second camera; kind 2 in the anchor frame),
 *                       preceded by one term for the anchor's own observation (X back in the anchor's first camera against pts_i:
 *                       the reference's loop starts at start_frame); n_obs = factors + 1; depth = 1 / lam.  A lam that only kind-2
 *                       factors name has no pose: it is evaluated in the anchor's body frame.  Factors of one lam that disagree on
 *                       (pose_i, pts_i): SWF_E_INVALID from swf_batch_check_features.
 *   flags               SWF_FEAT_OUTLIER iff mean_err * proj_sqrt_info > max_mean_error (the reference: 2, strict);
 *                       SWF_FEAT_NEG_DEPTH iff depth < 0 (world point) / lam < 0 (inverse depth); SWF_FEAT_UNOBSERVED for a landmark
 *                       no projection factor names (mean_err = depth = 0, never rejected).  A NaN mean sets neither bit.
 * Constant landmarks, landmarks outside elimination group 0 and factors with a variable extrinsic are covered like any other.
 * swf_batch_check_features is asynchronous on the batch stream (the first call builds the check's observation table).  The getter
 * synchronises; its first call after a check copies every window's results to the host once, later calls read that copy.  Arrays
 * are [n_feat]; rejected [<= n_feat] = the indices of the features with OUTLIER | NEG_DEPTH, ascending (compacted on the device).
 * Any pointer may be NULL.  Results are invalidated by the next swf_batch_solve / _upload_state / _reset_state (SWF_E_STATE, as is
 * a getter before any check); w out of range, max_mean_error not finite or < 0: SWF_E_INVALID.  Removing the rejected blocks
 * (FeatureManager::removeFailures) stays with the caller. */
enum { SWF_FEAT_OUTLIER = 1, SWF_FEAT_NEG_DEPTH = 2, SWF_FEAT_UNOBSERVED = 4 };
int swf_batch_check_features(swf_batch* b, double max_mean_error);
int swf_batch_get_feature_check(swf_batch* b, int32_t w, double* mean_err, double* depth, int32_t* n_obs, uint8_t* flags,
                                int32_t* rejected, int32_t* n_rejected, int32_t* n_feat);

/* Timing of the last swf_batch_solve, measured with HIP events recorded on the batch stream
 * around individual kernel launches (valid after swf_batch_sync).  `mask` selects which
 * kernels get an event pair per launch (bit k = SWF_K_*); bit 0 brackets the whole solve.
 * ms[k] = summed duration, calls[k] = number of launches bracketed.
 * One id per distinct kernel.  Mutually independent small kernels run as segments of one fused grid:
 *   LM_SCHUR    = k_lm_schur        landmark elimination + reduced-camera product (cells stay in LDS)
 *   EVAL_PS     = k_eval_ps<true>   projection + scalar-factor residuals and Jacobians (round 6, dogleg: at the candidate; one window: k_step_eval,
 *                                   which carries k_dogleg at its head — no DOGLEG bracket then; SWF_K_FRAME_SUMS is never recorded any more)
 *   POST_CHOL   = k_post_chol       back-substitution + |J D^-2 g|^2 of the Cauchy point
 *   POST_DOGLEG = k_post_dogleg     cost-only candidate residuals (Levenberg-Marquardt, windows with composite factors; one window: k_step_eval<., false>)
 *   DECIDE      = k_decide          (one window, dogleg: inside k_decide_lm_clique, recorded under LM_SCHUR)
 *   CAND_EVAL   = k_eval_imu<false> + k_eval_prior<false> (candidate residuals)
 *   CLIQUE_ELIM = the (up to three) size classes of k_clique_elim
 *   ASSEMBLE    = k_assemble_flat   the reduced system and its vectors from the static assembly program */
enum { SWF_K_TOTAL = 0, SWF_K_EVAL_PS = 1, SWF_K_EVAL_IMU = 2, SWF_K_FRAME_SUMS = 3, SWF_K_EVAL_PRIOR = 4,
       SWF_K_LM_SCHUR = 5, SWF_K_CLIQUE_ELIM = 6, SWF_K_LM_ELIM = 7, SWF_K_ASSEMBLE = 8, SWF_K_CHOL = 9,
       SWF_K_POST_CHOL = 10, SWF_K_POST_DOGLEG = 11, SWF_K_DOGLEG = 12, SWF_K_CAND_EVAL = 13, SWF_K_DECIDE = 14,
       SWF_K_COUNT = 16 };
typedef struct swf_timing {
    double ms[SWF_K_COUNT];
    int32_t calls[SWF_K_COUNT];
    int64_t jacobian_bytes;  /* algorithmic bytes of ONE Jacobian evaluation of the batch */
    int64_t proj_bytes;      /* the projection-factor share of it (312 B per observation) */
    int64_t chol_flops;      /* sum over windows of n_red^3 / 3 flops = n_red^3 / 6 multiply-adds (one factorisation of the batch) */
    int64_t lm_schur_flops;  /* landmark Schur product: sum over landmarks of 216 k^2 + 108 k flops */
    int64_t n_obs;           /* projection observations in the batch */
    int32_t n_linearizations;/* Jacobian evaluations enqueued per window in the last solve */
    int32_t reserved;
    int64_t lm_schur_flops_sym;  /* the same product counted over the lower triangle only: sum over landmarks of 108 k (k - 1) + 162 k flops */
    int64_t lm_schur_mfma;       /* v_mfma_f64_16x16x4_f64 instructions one product launch executes over the batch (2048 flops each) */
} swf_timing;
int swf_batch_enable_timing(swf_batch* b, int32_t mask);
int swf_batch_timing(swf_batch* b, swf_timing* out);

/* =====================================================================================
 * Input producer: batched IMU pre-integration
 *
 * IntegrationBase ctor / push_back / propagate / midPointIntegration / get_sqrtinfo
 * (R/factor/integration_base.cpp:5-142) for n_intervals keyframe intervals, one wavefront each.
 *   samples  [first[n_intervals]][7]  dt, acc(3), gyr(3).  The first sample of an interval seeds acc_0 / gyr_0 (its dt
 *            is ignored, as the reference's constructor takes no dt); every further sample is one push_back(dt, acc, gyr).
 *   first    [n_intervals + 1]        sample offsets (interval i owns samples first[i] .. first[i+1]-1)
 *   bias     [n_intervals][6]         linearisation biases ba, bg
 *   noise    ACC_N, GYR_N, ACC_W, GYR_W (yaml; R/parameter/parameters.cpp)
 *   pre      [n_intervals][SWF_PRE_DOUBLES] records, the layout swf_add_imu / swf_flat_window::imu_pre take.
 *            A covariance without full rank (an interval with no push_back or with one: rank 12; all-zero noise densities) leaves
 *            sqrt_info zero: a pivot of its factorisation at or below 2^-20 of its own diagonal entry refuses it.
 * on_device = 0: all pointers are host memory; the call copies in, runs, copies out and synchronises.
 * on_device = 1: all pointers are device memory; the kernel is enqueued on `stream` and the call returns.
 * ===================================================================================== */
int swf_preintegrate_batch(const double* samples, const int32_t* first, int32_t n_intervals, const double* bias,
                           const double noise[4], double* pre, int32_t on_device, void* stream);

/* The same pre-integration over a gather list: interval i is the runs run_first[i] .. run_first[i+1]-1 of `runs`, each an
 * (offset, count) pair of rows of samples[n_samples][7].  The first row of the interval's first non-empty run seeds acc_0 / gyr_0,
 * every further row of every run is one push_back; the record is bit-identical to swf_preintegrate_batch on the concatenated rows.
 * The merged interval of SlideWindowFrame (R/swf/swf.cpp:241-247) is "the rows of interval k, then the rows of interval k+1 without
 * its seed row": two runs, nothing is copied.
 *   runs       [run_first[n_intervals]][2]   offset, count (count 0 is allowed)
 *   run_first  [n_intervals + 1]
 * Host memory: a negative offset or count, a run beyond n_samples, or decreasing run_first: SWF_E_INVALID.  Device memory: such a
 * run counts as empty.  on_device as for swf_preintegrate_batch. */
int swf_preintegrate_runs_batch(const double* samples, int32_t n_samples, const int32_t* runs, const int32_t* run_first,
                                int32_t n_intervals, const double* bias, const double noise[4], double* pre,
                                int32_t on_device, void* stream);

/* The IMU front of a frame: SWFOptimization::ImuIntegrate and IMUProcess (R/swf/swf_imu.cpp:117-213) for n_frames independent
 * frames in one launch: the time-stamped samples are cut to (t0, t1] with the last one blended onto t1, the frame's Ps / Rs / Vs are
 * propagated with the mid-point rule, and the effective samples are pre-integrated.
 *   raw        [first[n_frames]][7]  t, acc(3), gyr(3): what GetImuInterval (:82-106) hands over: every sample with t0 < t < t1, then
 *              the first with t >= t1.  A sample beyond t1 is the last one used; rows after it are ignored.
 *   first      [n_frames + 1]        sample offsets
 *   t01        [n_frames][2]         t0 = the previous frame's time (the reference's static current_time on entry), t1 = cur_time
 *   seed       [n_frames][6]         acc_0, gyr_0 on entry: the last effective sample of the previous frame
 *   state      [n_frames][21]        the new frame's slot on entry: P(3), R(9, row-major), V(3), ba(3), bg(3)
 *   gyrj_prev  [n_frames][3]         pre_integrations[j-1]->gyrj
 *   flags      [n_frames]            bit 0: apply the velocity lever-arm terms (frame index > 5, :124, :173)
 *   pbg, g_w, noise                  host scalars: the antenna lever arm, Rwgw * G, and ACC_N, GYR_N, ACC_W, GYR_W
 *   cut        [first[n_frames] + n_frames][7]  frame f owns rows first[f] + f ..: the seed with dt 0, then one (dt, acc, gyr) row per
 *              IMUProcess call: the layout swf_preintegrate_batch and swf_preintegrate_runs_batch read
 *   pre        [n_frames][SWF_PRE_DOUBLES]      bit-identical to swf_preintegrate_batch on those rows with the bias of `state`
 *   pred       [n_frames][15]        P, R, V after the loop and the lever-arm restore
 *   info       [n_frames]            SWF_IMUF_*, where the reference asserts; a failed frame writes its info and nothing else
 * dt_i = t_i - t_(i-1) with t_(-1) = t0.  The sample beyond t1 becomes dt_1 = t1 - t_prev with acc / gyr = w1 * previous raw sample +
 * w2 * this one, w1 = dt_2 / (dt_1 + dt_2), w2 = dt_1 / (dt_1 + dt_2), dt_2 = t - t1.  The rotation update multiplies by what the
 * reference forms: Eigen's toRotationMatrix of the unnormalised quaternion (1, theta / 2) of Utility::deltaQ: R does not stay
 * orthonormal, and that is kept.  The reference neither pushes nor propagates for frame index 0 (:196): callers do not pass that frame.
 * Null pointers or (host memory) decreasing `first`: SWF_E_INVALID.  With host memory the per-frame failures are found before the
 * device is touched (a call whose frames all fail needs none).  A frame's result does not depend on the other frames of the call.
 * on_device as for swf_preintegrate_batch. */
enum { SWF_IMUF_OK = 0, SWF_IMUF_EMPTY = 1, SWF_IMUF_NO_INNER = 2, SWF_IMUF_TIME_ORDER = 3 };
int swf_imu_frame_batch(const double* raw, const int32_t* first, int32_t n_frames, const double* t01, const double* seed,
                        const double* state, const double* gyrj_prev, const int32_t* flags, const double pbg[3],
                        const double g_w[3], const double noise[4], double* cut, double* pre, double* pred, int32_t* info,
                        int32_t on_device, void* stream);

/* Integer least squares: RTKLIB's lambda(n, m, a, Q, F, s) (R/gnss/src/lambda.cpp:58-235) for a batch of problems, one wavefront
 * each: LtDL factorisation, LAMBDA reduction, MLAMBDA search for the m best integer vectors, with the reference's discrete decisions
 * (ROUND = floor(x + 0.5), the 1e-6 permutation margin, LOOPMAX = 10000 search iterations).  The reduction, unbounded in the
 * reference, gives up after 100000 permutations; both limits report SWF_LAMBDA_LOOP_LIMIT.  F = Z^-T E is formed from Z^-1 carried
 * through the reduction as integer row updates: exactly integer-valued.
 *   n  [n_problems]                 unknowns per problem, 1 <= n <= ld
 *   a  [n_problems][ld]             float solutions
 *   Q  [n_problems][ld][ld]         their covariances, column-major (only the lower triangle is read)
 *   m                               candidates, 1 or 2 (the reference takes 2)
 *   F  [n_problems][m][ld]          candidate j of problem p at F[(p * m + j) * ld + i] (0 beyond n and on failure)
 *   s  [n_problems][m]              their squared distances (a - F)^T Q^-1 (a - F), ascending
 *   info [n_problems]               SWF_LAMBDA_* per problem
 * ld > 64, m out of range, or (host memory) some n > 64 or n > ld: SWF_E_UNSUPPORTED; null pointers: SWF_E_INVALID.  A problem's
 * result does not depend on the other problems of the call.  on_device as for swf_preintegrate_batch. */
#define SWF_LAMBDA_NMAX 64
enum { SWF_LAMBDA_OK = 0, SWF_LAMBDA_NOT_PD = 1, SWF_LAMBDA_LOOP_LIMIT = 2, SWF_LAMBDA_NO_INPUT = 3 };
int swf_lambda_batch(int32_t n_problems, int32_t ld, const int32_t* n, const double* a, const double* Q,
                     int32_t m, double* F, double* s, int32_t* info, int32_t on_device, void* stream);

/* Fix and hold as a stand-alone operator: n linear priors, each with a list of fixed-integer constraint rows whose hidden per-group
 * offsets are eliminated (FixedIntegerFactor + marginalize(false, true), R/swf/swf_lambda.cpp:254-343), re-rooted.  One workgroup per
 * problem, fp64, every sum in a fixed order: a problem's result does not depend on the other problems of the call.
 *   dim [n]                 dimension of each prior, 1..SWF_FIX_PRIOR_MAXN (= 140: the largest matrix the root keeps in LDS; beyond: SWF_E_UNSUPPORTED)
 *   J, r                    the priors' Jacobians (dim x dim row-major) and their residuals r = r0 + J dx(x, x0) at the NEW linearisation point,
 *                           evaluated by the caller; concatenated over the problems (dim^2 / dim doubles each), as are all outputs
 *   row_first [n + 1], rows [row_first[n]][2], vals [row_first[n]]   problem p owns rows row_first[p] .. row_first[p+1]-1; a row is
 *                           (coordinate c of a one-dimensional kept block, group g) with value v: 0 for the group's reference ambiguity,
 *                           the fixed integer for the others — both RELATIVE to the point the scalar is linearised at (the reference zeroes
 *                           the ambiguities first, PhaseBiasSaveAndReset: there the values are the integers themselves).  Rows of one group
 *                           share one hidden offset: a row is the residual istd ((x_c - tf_g) - v) of FixedIntegerFactor.
 *   istd                    the weight of a row (the reference: 1 / 0.03);  eps, form: as swf_batch_marginalize
 * With A0 = J^T J, b0 = J^T r, per group with members c_1 .. c_k:  A'[c_a, c_b] = A0[c_a, c_b] + istd^2 (delta_ab - 1 / k),
 * b'[c_a] = b0[c_a] - istd^2 (v_a - mean(v)) — the Schur elimination of the offsets in closed form (they are mutually independent).
 *   A, b                    A', b' (sign convention b = J^T r)
 *   Jn, r0, eig, rank       the square root of (A', b'): SWF_PRIOR_EIGEN rows by ascending eigenvalue, eigenvalues <= eps dropped, rank = number
 *                           kept, eigenvector signs not defined; SWF_PRIOR_CHOLESKY Jn = L^T upper triangular, r0 = L^-1 b', eig = diag(L)^2,
 *                           rank = dim, or -1 (zeros) where A' is not positive definite
 * Rejected (host memory: before the device is touched): a coordinate outside the prior, two rows of one problem on one coordinate, a group
 * with a single row: SWF_E_INVALID.  on_device as for swf_lambda_batch; device-resident inputs cannot be checked by the host: a problem
 * with a bad dimension or bad rows reports rank -1 and writes nothing else.  Only a problem whose dim is outside 1..140 counts as empty
 * in the concatenation; one with bad rows still occupies its dim^2 / dim doubles.  Host memory: any output pointer may be NULL. */
#define SWF_FIX_PRIOR_MAXN 140
int swf_prior_fix_batch(int32_t n, const int32_t* dim, const double* J, const double* r, const int32_t* row_first, const int32_t* rows,
                        const double* vals, double istd, double eps, int32_t form, double* A, double* b, double* Jn, double* r0,
                        double* eig, int32_t* rank, int32_t on_device, void* stream);

/* Pre-fit carrier-phase screen: the numeric core of the first half of SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:337-499)
 * for a batch of epochs, one wavefront each.  A record is one carrier-phase observation of the new epoch: RTK (base-rover single
 * difference) or SPP (rover-only phase).
 *   first [n_epochs + 1]        epoch e owns records first[e] .. first[e+1]-1; an epoch without records is legal
 *   pos, base [n_epochs][3]     the predicted position of the epoch's frame (para_pose[g2f[ir]][0..2]); the base-station position
 *   mode [n_epochs]             SWF_SCR_GATE_RTK = USE_IMU && USE_RTK && solver_flag == NonLinear && rover_count > 1 (:407),
 *                               SWF_SCR_GATE_SPP = the same with USE_SPP_PHASE (:417), SWF_SCR_RESET_ALL = not_fix_count > Phase_ALL_RESET_COUNT (:433)
 *   el_min                      AZELMIN (the reference: 25 degrees, in radians)
 *   dat [n][SWF_SCR_DOUBLES]    sat[3]; L_lam = the phase in metres; lam; el; P = the pseudorange of the code-minus-phase test (SPP only);
 *                               N = the ambiguity's value; dt = the receiver clock (para_gnss_dt[0][sys*2+f] for RTK, [6+sys*2] for SPP)
 *   rec [n][4]                  kind (SWF_SCR_RTK / _SPP); group sys * 2 + f in 0..5; state bits: SWF_SCR_HAS_AMB = the Npoint exists,
 *                               SWF_SCR_CONTINUING = its SLIP_COUNT equals the observation's; partner = the index within the epoch of the
 *                               RTK record of the same satellite and frequency, or -1 (read for SPP records only)
 * Per epoch:
 *   1. a record is MASKED iff el < el_min (:351-353); its L_lam is then taken as 0.
 *   2. r = distance(pos + base, sat) - N lam - L_lam + dt, added left to right, for a record with HAS_AMB (:354-379: the un-weighted
 *      RTKCarrierPhaseFactor, distance() with the Sagnac term); r = 0 without, and N, dt are then not used.
 *   3. the median set of (kind, group) is the records with HAS_AMB && CONTINUING — masked ones included, as the reference pushes their
 *      residual with the phase zeroed (:351-362).  cnt = its size; med = the element of rank cnt / 2 in ascending order (the upper median,
 *      sorted[size / 2], :385), ties by record index, a NaN last; cnt = 0, med = NaN for an empty set.
 *   4. un-masked records only (:402-472).  RTK: SLIP_RESIDUAL (the reference's condition3) iff GATE_RTK && HAS_AMB && CONTINUING &&
 *      |r - med| > lam / 2;  NEW_AMB iff !HAS_AMB || !CONTINUING || SLIP_RESIDUAL || RESET_ALL.  SPP, under GATE_SPP && HAS_AMB && CONTINUING:
 *      SLIP_CODE iff |(L_lam + N lam) - P| sin(el)^2 > 10, SLIP_RESIDUAL iff |r - med| > lam;  NEW_AMB iff !HAS_AMB || !CONTINUING ||
 *      the partner's SLIP_RESIDUAL || SLIP_CODE || SLIP_RESIDUAL (RESET_ALL does not reach SPP records, :454).  A masked record carries
 *      MASKED and nothing else; a comparison with a NaN sets no bit.
 * Outputs: r [n], flags [n] (SWF_SCR_* output flags); med, cnt [n_epochs][2][SWF_SCR_GROUPS] indexed kind, then group; reset [n]: the
 * within-epoch indices of the records with NEW_AMB, ascending, compacted on the device into reset[first[e] ..] (-1 behind them up to the
 * epoch's end); n_reset [n_epochs].  An epoch's result does not depend on the other epochs of the call; every count runs in a fixed order.
 * Rejected (host memory: before the device is touched): first[0] != 0 or a decreasing first, a kind, group or state bit out of range, a
 * partner that is out of range, is the record itself or is not an RTK record, lam or el_min not finite, lam <= 0, null input pointers:
 * SWF_E_INVALID; an epoch with more than SWF_SCR_NMAX records: SWF_E_UNSUPPORTED.  on_device as for swf_lambda_batch; device-resident
 * inputs cannot be checked by the host: an epoch whose records the kernel finds invalid reports n_reset = -1 and writes nothing else.
 * Any output pointer may be NULL.
 * Stays with the caller: creating the PBtype entries the NEW_AMB flags ask for, continue_count, last_update_time and the 10 s staleness
 * rule (:300-330, :434-495); the pseudorange-correction variables (:474-491).  The seed mini-solve that follows (:534-575) is
 * swf_gnss_epoch_solve_batch below.  For a single epoch the host loop is faster than a launch: the operator is for batched epoch pipelines whose
 * inputs and consumers (swf_batch_marginal_priors) are on the device. */
#define SWF_SCR_NMAX 256           /* MAXOBS (64) x NFREQ (2) x {RTK, SPP} records per epoch */
enum { SWF_SCR_RTK = 0, SWF_SCR_SPP = 1 };                                   /* kind */
enum { SWF_SCR_HAS_AMB = 1, SWF_SCR_CONTINUING = 2 };                        /* record state bits */
enum { SWF_SCR_GATE_RTK = 1, SWF_SCR_GATE_SPP = 2, SWF_SCR_RESET_ALL = 4 };  /* epoch mode bits */
enum { SWF_SCR_MASKED = 1, SWF_SCR_SLIP_RESIDUAL = 2, SWF_SCR_SLIP_CODE = 4, SWF_SCR_NEW_AMB = 8 }; /* output flags */
int swf_phase_screen_batch(int32_t n_epochs, const int32_t* first,
                           const double* pos, const double* base, const int32_t* mode, double el_min,
                           const double* dat, const int32_t* rec,
                           double* r, uint8_t* flags, double* med, int32_t* cnt, int32_t* reset, int32_t* n_reset,
                           int32_t on_device, void* stream);

/* Single-epoch GNSS solve: the seed mini-solve of SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:534-575: pose and speed-bias
 * constant, ambiguities older than ten epochs constant, the receiver clocks and the new ambiguities fitted in two iterations) and the
 * first fix of GnssProcess (:203-215: one epoch's raw factors, position, velocity and clocks free, 20 iterations) as one operator for
 * a batch of epochs, one wavefront each.  All five raw GNSS factor classes are scalar rows on the position of the pose, the velocity
 * of the speed-bias, one of 13 clock scalars and at most one ambiguity (R/factor/gnss_factor.cpp).
 * Records.  A record is one scalar factor of the epoch.
 *   dat [n][SWF_GES_DOUBLES]    sat[3] satvel[3] obs w lam N: w = the square-root information the factor would use (1 / sqrt(varerr2) or
 *                               istd; the operator does not compute varerr2); satvel is read by Doppler rows, lam and N by phase rows
 *   rec [n][4]                  kind; clock slot 0..12; state bits (SWF_GES_AMB_FREE: the row's ambiguity is an unknown); 0
 * With xg = pos + base, rho = distance(xg, sat) (the Sagnac term included), clk = clock[slot], sums left to right as written:
 *   SWF_GES_RTK_PHASE   RTKCarrierPhaseFactor   r = w (rho - N lam - obs + clk)
 *   SWF_GES_RTK_CODE    RTKPseudorangeFactor    r = w (rho - obs + clk)
 *   SWF_GES_SPP_CODE    SppPseudorangeFactor    r = w (rho + clk - obs)
 *   SWF_GES_SPP_PHASE   SppCarrierPhaseFactor (also the pseudorange-correction rows of R/swf/swf_core.cpp:174-186)
 *                                               r = w (rho + clk - N lam - obs)
 *   SWF_GES_DOPPLER     SppDopplerFactor        r = w (rate + clk + obs), rate = velecitydistance(): with e = (xg - sat) / |xg - sat| and
 *                                               ev = vel - satvel, rate = ev . e + OMGE / CLIGHT (satvel[1] xg[0] + sat[1] vel[0] -
 *                                               satvel[0] xg[1] - sat[0] vel[1])
 * Jacobians are the factors' own: position w e for range rows (the Sagnac term is not differentiated, as in the reference) and
 * w (ev - (ev . e) e) / |xg - sat| for Doppler rows; velocity w e for Doppler rows; clock w; ambiguity -w lam.
 * Inputs per epoch: first [n_epochs + 1] (an epoch without records is legal); pos, vel, base [n_epochs][3]; clock [n_epochs][13];
 * mode [n_epochs] (SWF_GES_FREE_POS | SWF_GES_FREE_VEL); clk_const [n_epochs]: bit s set = clock s is held constant.
 * Inputs per call: max_iter, step_tol, eps_rank.
 * One iteration:
 *   1. every record is evaluated at the current state.
 *   2. the reduced system is formed from the rows without AMB_FREE (a free ambiguity is seen by its row alone: its Schur complement is
 *      zero and the row drops out).  Unknowns: the free part of [pos, vel], and the clocks that are not constant and have at least one
 *      such row with w > 0.  The normal equations are formed, the clocks eliminated as scalars, and what is left (dimension 0, 3 or 6)
 *      is factored by Cholesky.
 *   3. a pivot <= eps_rank x its reduced diagonal entry ends the epoch with SWF_GES_RANK_DEFICIENT, and so does a reduced diagonal
 *      entry <= eps_rank x that entry before the clocks were eliminated (one that the elimination cancelled to rounding noise).  The
 *      state outputs of such an epoch are the inputs.
 *   4. otherwise the clocks are back-substituted and the step is added.
 *   5. the epoch stops when every entry of the step is <= step_tol in magnitude (SWF_GES_CONVERGED) or after max_iter iterations
 *      (SWF_GES_MAX_ITER).  A clock without a determining row keeps its value.
 * After the last iteration every AMB_FREE phase row gets the N that makes its residual zero at the final state: (rho - obs + clk) / lam
 * (RTK), (rho + clk - obs) / lam (SPP); other rows echo their N.
 * Outputs, any of which may be NULL: pos_out, vel_out [n_epochs][3]; clock_out [n_epochs][13]; N_out [n]; r_out [n]: the weighted
 * post-fit residuals, 0 for absorbed rows; cost [n_epochs] = 1/2 sum r^2; iters (iterations run, the deficient one included); status;
 * clk_rows [n_epochs][13]: the rows without AMB_FREE and with w > 0 per clock; info [n_epochs][36]: the reduced 6 x 6 information matrix
 * of [pos, vel] at the last linearisation, row-major, with zero rows and columns for the constant part.
 * An epoch's result does not depend on the other epochs of the call; every sum runs in a fixed order; there are no atomics.
 * Rejected (host memory: before the device is touched): first[0] != 0 or a decreasing first, a kind, slot, state, mode or clk_const bit
 * out of range, a non-zero fourth record integer, AMB_FREE on a row that is not a phase row, a non-finite value (records, pos, vel, base,
 * clock, step_tol, eps_rank), w < 0, lam <= 0 on a phase row, max_iter < 1, null input pointers: SWF_E_INVALID; an epoch with more
 * than SWF_GES_NMAX records: SWF_E_UNSUPPORTED.  on_device as for swf_lambda_batch; device-resident inputs cannot be checked by the
 * host: the kernel makes the same checks and an epoch it finds invalid reports status = -1 and writes nothing else.
 * Stays with the caller: creating the PBtype entries and continue_count (which rows carry AMB_FREE), update_azel (elevation enters
 * through w), gating on the post-fit residuals, and the dummy anchor InitialBlackFactor, which shares no row with the rest. */
#define SWF_GES_NMAX 512           /* MAXOBS (64) x 8 rows per satellite */
enum { SWF_GES_RTK_PHASE = 0, SWF_GES_RTK_CODE = 1, SWF_GES_SPP_CODE = 2, SWF_GES_SPP_PHASE = 3, SWF_GES_DOPPLER = 4 };  /* kind */
enum { SWF_GES_AMB_FREE = 1 };                                                /* record state bits */
enum { SWF_GES_FREE_POS = 1, SWF_GES_FREE_VEL = 2 };                          /* epoch mode bits */
enum { SWF_GES_CONVERGED = 0, SWF_GES_MAX_ITER = 1, SWF_GES_RANK_DEFICIENT = 2 };  /* status (-1: an invalid device-resident epoch) */
int swf_gnss_epoch_solve_batch(int32_t n_epochs, const int32_t* first,
                               const double* pos, const double* vel, const double* base, const double* clock,
                               const int32_t* mode, const int32_t* clk_const, const double* dat, const int32_t* rec,
                               int32_t max_iter, double step_tol, double eps_rank,
                               double* pos_out, double* vel_out, double* clock_out, double* N_out, double* r_out, double* cost,
                               int32_t* iters, int32_t* status, int32_t* clk_rows, double* info,
                               int32_t on_device, void* stream);

/* The double-difference pairs of the integer ambiguity search: FindReferenceSatellites (R/swf/swf_lambda.cpp:8-53) and the loop of
 * SWFOptimization::LambdaSearch that builds D3 (:118-188) for a batch of windows, one wavefront each.
 *   epoch_first [n_windows + 1]   window w owns epochs epoch_first[w] .. epoch_first[w+1]-1, in the reference's processing order:
 *                                 NEWEST FIRST (ir = rover_count-1 .. 0); a window without epochs is legal
 *   obs_first [n_epochs + 1]      epoch e owns observations obs_first[e] .. obs_first[e+1]-1, in the reference's iteration order
 *                                 (observation index ascending, frequency ascending); an epoch without observations is legal
 *   obs [n_obs][2]                class = sys * 2 + f in 0..5; t = the tail coordinate of the observation's ambiguity
 *   y_first [n_windows + 1], y    window w's tail has y_first[w+1] - y_first[w] coordinates, y[y_first[w] + t] the float value of t
 *   gate [n_windows]              the reference: 0.2 after a fix, 1.4 otherwise (:163)
 * Observations whose ambiguity is absent or not in the tail are left out by the caller: they can never be candidates (:14-18) nor
 * produce a pair (:150-154), their `use` marks are only ever read for themselves, and the :141-144 fallback that names one as a
 * reference can only lead to the a < 0 || b < 0 exit.  The reference reads a block at index 0 of parameter_block_idx as absent
 * (:16, :150); which observations are passed is the caller's decision.
 * Per window (round = C round(), halves away from zero; every sum left to right; no product anywhere):
 *   used = {}; for each epoch, newest first:
 *     for each class c: the candidates are the epoch's observations of class c with t not in used, in order; without one the class
 *       has no reference in this epoch; cost_j = sum over the candidates i of |s - round(s)|, s = y[t_i] - y[t_j] (i == j included);
 *       the reference is the LAST candidate whose cost equals the minimum.  A reference is never marked used.
 *     for each observation k in order: its class has no reference: role 4.  Else t_k in used: role 0.  Else k is the reference:
 *       role 1.  Else t_k is marked used (before the gate: a gated-out ambiguity is not reconsidered in an older epoch) and, with
 *       d = y[t_k] - y[t_ref], |d - round(d)| < gate appends the pair (t_k, t_ref): role 2; otherwise role 3.
 *   last_count = the pairs of the newest epoch, last_ref_count = its classes with a reference;
 *   go = tail >= 6 && last_count + last_ref_count >= 6 && last_count >= 4 && n_pairs >= 4  (:96, :178, :184).
 * Outputs, any of which may be NULL: pairs [n_windows][64][2] in the order they were appended, -1 behind them; counts [n_windows][4]
 * = n_pairs, last_count, last_ref_count, info; refs [n_epochs][6] = the reference's observation index within the epoch, or -1;
 * cost [n_obs], -1 where the observation was no candidate; role [n_obs] (SWF_DDSEL_SKIPPED ..).
 *   info  SWF_DDSEL_OK         go
 *         SWF_DDSEL_TOO_FEW    the reference's early returns; pairs and counts are still reported
 *         SWF_DDSEL_OVERFLOW   more than SWF_LAMBDA_NMAX pairs: n_pairs = 0 and no pair is reported; the other outputs are
 *         SWF_DDSEL_NONFINITE  some y the window's observations name is not finite (every ambiguity is a candidate where it first
 *                              appears, and the reference sorts the costs, which is undefined with a NaN): counts = 0, refs = -1,
 *                              cost = -1, role = 0, no pair
 * A window's result does not depend on the other windows of the call and is a function of its inputs alone, bit for bit.
 * Rejected (host memory: before the device is touched, no output written): first[0] != 0 or a decreasing prefix array, a class outside
 * 0..5, a t outside the tail, one t twice within an epoch, a gate that is not finite and positive, null input pointers: SWF_E_INVALID;
 * an epoch with more than SWF_DDSEL_NMAX observations or a tail of more than SWF_DDSEL_TMAX coordinates: SWF_E_UNSUPPORTED.
 * on_device as for swf_preintegrate_batch: every pointer is device memory, the call is asynchronous on `stream`, and the kernel makes
 * the checks itself (one t twice within an epoch excepted): a window it finds invalid reports info = -1 and writes nothing else.
 * Stays with the caller: the fix counter, the gnss_last_updatetime reset, and which ambiguities are in the tail
 * (UpdateNParameterHead's eligibility rules).  For a single window the host loop is faster than a launch: the operator is for batches
 * whose state and whose consumer (swf_batch_ambiguity_search_selected) are on the device. */
#define SWF_DDSEL_NMAX 256          /* MAXOBS (64) x NFREQ (2), with room: observations per epoch */
#define SWF_DDSEL_TMAX 2048         /* tail coordinates per window */
enum { SWF_DDSEL_OK = 0, SWF_DDSEL_TOO_FEW = 1, SWF_DDSEL_OVERFLOW = 2, SWF_DDSEL_NONFINITE = 3 };             /* info */
enum { SWF_DDSEL_SKIPPED = 0, SWF_DDSEL_REFERENCE = 1, SWF_DDSEL_PAIRED = 2, SWF_DDSEL_GATED_OUT = 3, SWF_DDSEL_NO_REFERENCE = 4 };  /* role */
int swf_dd_select_batch(int32_t n_windows, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs,
                        const int32_t* y_first, const double* y, const double* gate,
                        int32_t* pairs, int32_t* counts, int32_t* refs, double* cost, uint8_t* role,
                        int32_t on_device, void* stream);

/* Input producer: the pose of a new image frame from the landmarks it observes — FeatureManager::initFramePoseByPnP with
 * solvePoseByPnP (R/feature/feature_manager.cpp:164-243) for n_frames independent frames in one launch, one workgroup per frame.
 * The reference's numerical content is cv::solvePnPRansac(pts3D, pts2D, I, -, rvec, t, true, 100, 8.0 / FOCAL_LENGTH, 0.99).  Kept of
 * it: the 5-point model (4 points for a frame of exactly 4), the previous frame's pose as the guess, the threshold on the squared
 * reprojection error, the confidence and the adaptive iteration count (RANSACUpdateNumIters), the inlier set of the winning hypothesis,
 * a refinement on the inliers, the pose conversions and the float rounding of the points.  Specified anew, because they are OpenCV
 * internals:
 *   sampler    draw j of hypothesis k is x = splitmix64(seed + 64 k + j) (the generator's output function at state x + 0x9E3779B97F4A7C15,
 *              modulo 2^64), index ((x >> 32) n) >> 32; a draw equal to an earlier index of the sample is skipped; a sample that is
 *              not complete after 64 draws is an invalid hypothesis.  The frame index is not mixed in.  n == 4: one hypothesis, 0 1 2 3.
 *   minimal    6 Gauss-Newton steps from the guess over the sample's residuals r = (x/z - u, y/z - v), p_c = R p_w + t, J = [-J_p [R p_w]_x | J_p],
 *              unpivoted Cholesky of J^T J, R <- Exp(dtheta) R, t <- t + dt.  Invalid on a pivot <= 0, |z| < 1e-12 or a non-finite value:
 *              count 0, exported rows NaN.  (OpenCV: EPnP, which needs no guess.)
 *   inliers    z > 0 and |r|^2 <= threshold^2.  (cv::projectPoints has no test on z.)
 *   scan       k = 0, 1, .. while k < n_iters (iterations at first): a count > max(best count, m - 1) becomes the best and n_iters is
 *              updated with ep = (n - count) / n; the quotient of the logarithms is rounded to nearest, halves to even.
 *   refinement 10 Gauss-Newton steps of the same form from the best hypothesis over its inliers, every sum in a fixed order.
 * Arrays:
 *   first      [n_frames + 1]             point offsets
 *   pts_w      [first[n_frames]][3]       the landmarks' world points (ptsInW, :214-218);  pts_uv [..][2] their normalised observations
 *   Ps_prev    [n_frames][3], Rs_prev [n_frames][9] row-major   Ps / Rs[frameCnt - 1] as the reference passes them
 *   tic, ric (row-major), pbg             camera extrinsic and the IMU->antenna lever arm
 *   iterations, threshold, confidence     100, 8.0 / FOCAL_LENGTH, 0.99 in the reference;  1 <= iterations <= SWF_PNP_HMAX
 *   flags      bit 0: round pts_w, pts_uv through float first, as cv::Point3f / Point2f do
 *   Ps_out     [n_frames][3], Rs_out [n_frames][9]   the new frame's pose, in the layout swf_triangulate_batch reads
 *   n_inliers, best, n_iters, info [n_frames];  inlier [first[n_frames]]   the winning hypothesis's index, count and mask
 *   samples    [n_frames][iterations][5], hyp [n_frames][iterations][12] (R row-major, then t, of cam_T_w), count [n_frames][iterations]:
 *              stage exports, null when not wanted; a frame of 4 points writes row 0 only
 * info: SWF_PNP_TOO_FEW (n < 4), SWF_PNP_BAD_INPUT (a non-finite point or previous pose), SWF_PNP_NO_MODEL (no hypothesis with at
 * least m inliers): the frame writes its info and nothing else, as the reference leaves the pose alone.  SWF_PNP_UNREFINED: the
 * refinement met a pivot <= 0, |z| < 1e-12 or a non-finite value; the unrefined hypothesis is written.  Without a usable guess the
 * operator reports SWF_PNP_NO_MODEL where EPnP might have found a pose.
 * iterations outside 1 .. SWF_PNP_HMAX or (host memory) a frame above SWF_PNP_NMAX points: SWF_E_UNSUPPORTED; null required pointers,
 * (host memory) a negative or decreasing `first`, a threshold that is not finite and positive, non-finite confidence or extrinsics: SWF_E_INVALID.
 * With host memory the TOO_FEW / BAD_INPUT frames are found before the device is touched (a call whose frames all fail so needs none).
 * Device memory: a frame whose offsets are negative, decreasing or above SWF_PNP_NMAX reports info = -1 and writes nothing else.
 * A frame's result does not depend on the other frames of the call, and a rerun gives the same bits.  on_device as for
 * swf_preintegrate_batch. */
enum { SWF_PNP_OK = 0, SWF_PNP_TOO_FEW = 1, SWF_PNP_NO_MODEL = 2, SWF_PNP_UNREFINED = 3, SWF_PNP_BAD_INPUT = 4 };
#define SWF_PNP_NMAX 1024      /* points per frame */
#define SWF_PNP_HMAX 128       /* hypotheses */
int swf_pnp_frame_batch(int32_t n_frames, const int32_t* first, const double* pts_w, const double* pts_uv,
                        const double* Ps_prev, const double* Rs_prev, const double tic[3], const double ric[9], const double pbg[3],
                        int32_t iterations, double threshold, double confidence, uint64_t seed, int32_t flags,
                        double* Ps_out, double* Rs_out, int32_t* n_inliers, uint8_t* inlier, int32_t* best, int32_t* n_iters,
                        int32_t* info, int32_t* samples, double* hyp, int32_t* count, int32_t on_device, void* stream);

/* Input producer: the geometric gate between tracked pixels and the estimator — FeatureTracker::rejectWithF with undistortedPts and
 * ptsVelocity (R/feature/feature_tracker.cpp:265-294, :334-376) for n_pairs independent frame pairs in one launch, one workgroup per
 * pair.  The reference's numerical content is PinholeFullCamera::liftProjective (C/src/camera_models/PinholeFullCamera.cc:535-607) and
 * cv::findFundamentalMat(un_cur, un_prev, FM_RANSAC, F_THRESHOLD, 0.99, status).  Kept of the latter: the virtual-camera pixels, the
 * symmetric epipolar distance against the squared threshold, the confidence and the adaptive iteration count (RANSACUpdateNumIters),
 * the status of the winning hypothesis, no refit.  Specified anew:
 *   lift       x0 = p.x / fx - cx / fx (y alike), then exactly nine fixed-point steps in the order of :574-581: r2, icdist =
 *              (1 + ((k6 r2 + k5) r2 + k4) r2) / (1 + ((k3 r2 + k2) r2 + k1) r2), deltaX, deltaY, x = (x0 - deltaX) icdist, y alike
 *              (the reference's loop ends only by its counter).  Every operation rounds once.  u = focal x + col / 2, v = focal y + row / 2.
 *   sampler    that of swf_pnp_frame_batch with 8 indices: draw j of hypothesis k is x = splitmix64(seed + 64 k + j), index
 *              ((x >> 32) n) >> 32, repeats skipped, invalid when incomplete after 64 draws.  n == 8: one hypothesis, 0 .. 7.
 *   minimal    the 8-point algorithm (OpenCV's run8Point; FM_RANSAC itself draws 7 points and solves a cubic): each image's sample is
 *              translated to its centroid and scaled by sqrt(2) / mean distance (invalid below a mean distance of 2^-23); rows
 *              [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], m1 = cur, m2 = prev; F0 the unit right null vector (Householder QR of
 *              the transposed design matrix); the smallest singular value of the 3 x 3 set to 0 (one-sided Jacobi, six sweeps);
 *              F = T2^T F0 T1, row-major.  A non-finite value makes the hypothesis invalid: count 0, exported row NaN.
 *   inliers    d2 = (m2^T F m1)^2 / (a^2 + b^2), (a, b, .) = F m1; d1 alike through F^T m2; inlier iff d1 <= thr^2 and d2 <= thr^2.
 *   scan       k = 0, 1, .. while k < n_iters (iterations at first): a count > max(best count, 7) becomes the best and n_iters is
 *              updated with 8 model points; the quotient of the logarithms is rounded to nearest, halves to even.
 * Arrays:
 *   first      [n_pairs + 1]              point offsets
 *   cur_px, prev_px [first[n_pairs]][2]   pixel positions of the same tracks in the current and the previous frame
 *   cam        [12]                       fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 (PINHOLE_FULL);  col, row, focal: 752, 480, FOCAL_LENGTH = 1000
 *   dt         [n_pairs]                  cur_time - prev_time
 *   iterations, threshold, confidence     1 <= iterations <= SWF_TRK_HMAX (OpenCV: 1000), F_THRESHOLD = 1.0 px, 0.99
 *   flags      bit 0: round through float wherever the reference holds a cv::Point2f: the pixel inputs, the virtual-camera pixels, the
 *              normalised outputs, and the velocity (difference formed in float, divided by dt in double, stored as float)
 *   status     [first[n_pairs]]           1 = keep;  keep_idx [first[n_pairs]]: the kept indices of a pair (counted from the pair's first
 *              point) in ascending order from first[k], -1 behind them (reduceVector)
 *   n_inliers, best, n_iters, info [n_pairs];  F [n_pairs][9] the winning hypothesis
 *   un_cur, un_prev [..][2]               undistortedPts;  velocity [..][2] = (un_cur - un_prev) / dt (ptsVelocity for an aligned pair)
 *   samples    [n_pairs][iterations][8], hyp [n_pairs][iterations][9], count [n_pairs][iterations]: stage exports of every hypothesis,
 *              whatever the scan used; a pair of 8 points writes row 0 only
 * Every output but info may be null.
 * info: SWF_TRK_BAD_INPUT (a non-finite pixel or dt, dt <= 0; tested first): the pair writes its info only.  SWF_TRK_TOO_FEW (n < 8,
 * the reference skips the gate) and SWF_TRK_NO_MODEL (no hypothesis with 8 inliers): un_cur, un_prev and velocity are written, nothing
 * else.  iterations outside 1 .. SWF_TRK_HMAX or (host memory) a pair above SWF_TRK_NMAX points: SWF_E_UNSUPPORTED; null required
 * pointers, (host memory) a negative or decreasing `first`, a threshold or focal that is not finite and positive, a non-finite
 * confidence or cam, fx or fy of 0: SWF_E_INVALID.  With host memory the BAD_INPUT pairs are found before the device is touched.
 * Device memory: a pair whose offsets are negative, decreasing or above SWF_TRK_NMAX reports info = -1 and writes nothing else.
 * A pair's result does not depend on the other pairs of the call, and a rerun gives the same bits.  on_device as for
 * swf_preintegrate_batch. */
enum { SWF_TRK_OK = 0, SWF_TRK_TOO_FEW = 1, SWF_TRK_NO_MODEL = 2, SWF_TRK_BAD_INPUT = 3 };
#define SWF_TRK_NMAX 1024      /* points per pair */
#define SWF_TRK_HMAX 1024      /* hypotheses */
int swf_track_reject_batch(int32_t n_pairs, const int32_t* first, const double* cur_px, const double* prev_px, const double cam[12],
                           int32_t col, int32_t row, double focal, const double* dt, int32_t iterations, double threshold,
                           double confidence, uint64_t seed, int32_t flags, uint8_t* status, int32_t* keep_idx, int32_t* n_inliers,
                           int32_t* best, int32_t* n_iters, int32_t* info, double* F, double* un_cur, double* un_prev,
                           double* velocity, int32_t* samples, double* hyp, int32_t* count, int32_t on_device, void* stream);

/* Input producer: the tracked pixel pairs themselves — the sparse optical flow of FeatureTracker::trackImage
 * (R/feature/feature_tracker.cpp:98-141) for n_pairs independent image pairs, one wavefront per point: a forward pyramidal
 * Lucas-Kanade pass (cv::calcOpticalFlowPyrLK, 21 x 21, 3 levels), a reverse pass with 1 level started from the previous positions
 * (FLOW_BACK), the 0.5 px forward-backward gate, inBorder and reduceVector.  It is OpenCV's LKTrackerInvoker restated, with one
 * declared difference: OpenCV accumulates A and b in float in SIMD order; here they are exact integer sums converted once to double,
 * so the float64 referee of the tests is met bit for bit.  Not here: the n++ of track_cnt, setPrediction, the stereo branch (setMask,
 * goodFeaturesToTrack and addPoints: swf_gftt_detect_batch below).  The specification; positions are (x, y), floor is towards -inf, rint to nearest even,
 * descale(v, n) = (v + 2^(n-1)) >> n arithmetically, r101(i, n) = |i|, and 2 (n - 1) - i above n - 1:
 *   pyramid    level l + 1 has size ((w + 1) / 2, (h + 1) / 2); dst(x, y) = (sum_ij k_i k_j src(r101(2x + i - 2, w), r101(2y + j - 2, h))
 *              + 128) >> 8, k = 1 4 6 4 1.  Building stops before a level whose width or height would be <= win; the level count
 *              used is min(max_level, that), for the reverse pass min(back_level, that).
 *   Scharr     inside the image Ix(x, y) = 3 (P(x+1, y-1) - P(x-1, y-1)) + 10 (P(x+1, y) - P(x-1, y)) + 3 (P(x+1, y+1) - P(x-1, y+1)), P
 *              through r101, Iy the transposed stencil; both 0 outside the image.  Intensities outside are read through r101.
 *   weights    at p: ip = floor(p), a = p.x - ip.x, b = p.y - ip.y, w00 = rint((1-a)(1-b) 16384), w01 = rint(a (1-b) 16384),
 *              w10 = rint((1-a) b 16384), w11 = 16384 - w00 - w01 - w10 (each product rounded once, left to right); for a source S
 *              and the win^2 offsets (i, j): v = S(ip+(i,j)) w00 + S(ip+(i+1,j)) w01 + S(ip+(i,j+1)) w10 + S(ip+(i+1,j+1)) w11.
 *              p is outside its level when ip.x < -win or ip.x >= cols_l, or the same in y.
 *   per point  for l = top .. 0, half = (win - 1) / 2, template image I, search image J:
 *              1. p = prev 2^-l; q = (l == top) ? (bit 1 ? guess : prev) 2^-l : 2 q; p -= half; p outside: LOST at level 0, else the
 *                 next level with q kept.
 *              2. It = descale(v_I, 9), Itx = descale(v_Ix, 14), Ity alike; A11 = (sum Itx^2) 2^-20, A12 = (sum Itx Ity) 2^-20,
 *                 A22 = (sum Ity^2) 2^-20; D = A11 A22 - A12 A12; minEig = (A22 + A11 - sqrt((A11 - A22)(A11 - A22) + 4 A12 A12)) /
 *                 (2 win^2); minEig < min_eig or D < 2^-23: FLAT at level 0, else the next level; D = 1 / D.
 *              3. q -= half; for j = 0 .. max_count - 1: q outside: LOST at level 0, break; d = descale(v_J at q, 9) - It;
 *                 b1 = (sum d Itx) 2^-20, b2 alike; delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D); q += delta, the iteration
 *                 counts; |delta|^2 <= eps^2: break; j > 0 and |delta + previous delta| < 0.01 in x and in y: q -= 0.5 delta, break.
 *                 Then q += half.
 *              4. cur = q of level 0.  The reverse pass: the same with the images swapped, prev := cur, the initial flow the original
 *                 prev_px, over the reverse level count; it gives back.  BACK_FAR: sqrt(dx^2 + dy^2) > back_dist, (dx, dy) = prev - back.
 *                 BORDER: !(1 <= rint(cur.x) < cols - 1 and 1 <= rint(cur.y) < rows - 1).  The reverse pass runs for every point,
 *                 whatever the forward pass found (as in the reference).
 *   exactness  |It| <= 8160, |Itx| <= 4080: every sum over 441 terms is an integer below 2^35, exact in any order; everything else
 *              is a fixed sequence of double operations, each rounded once (no contraction, correctly rounded sqrt and division).
 * Arrays:
 *   prev_img, cur_img [n_pairs][rows][cols]  8-bit grey, dense rows
 *   first      [n_pairs + 1]                 point offsets
 *   prev_px, guess_px, cur_px, back_px [first[n_pairs]][2];  guess_px goes with flag bit 1 and only with it (else null)
 *   win, max_level, back_level, max_count, eps, min_eig, back_dist: the reference's 21, 3, 1, 30, 0.01, 1e-4, 0.5;  max_count 1 .. 1000
 *   flags      bit 0: round prev_px / guess_px on entry and cur_px / back_px at the end of each pass through float, where the reference
 *              holds a cv::Point2f (everything between is double);  bit 1: guess_px is the initial flow of the forward pass
 *              (hasPrediction);  bit 2: run the reverse pass and its gate (FLOW_BACK).  The reference: 5.
 *   status     [..] 1 = keep;  why [..] the first of the point codes that applies, in the order of the enum (without bit 2 the BACK codes
 *              do not occur and back_px is not written)
 *   keep_idx   [..], n_keep [n_pairs]        as in swf_track_reject_batch: ascending indices from first[k], -1 behind them
 *   trace_iters [..][2][SWF_KLT_LMAX + 1]    iterations run per pass (0 forward, 1 reverse) and level; -1: level not visited, the
 *              template window outside the level, or the level flat
 *   trace_px   [..][2][SWF_KLT_LMAX + 1][2]  q after that level in that level's pixels (as set in step 1 where the level was left
 *              early; 0 for a level not visited)
 *   pyr        [n_pairs][swf_klt_pyramid_bytes(rows, cols, max(max_level, back_level))]  the workspace and a stage export: per pair
 *              the levels 1 .. of prev, then (from half of the pair's bytes) of cur, dense; the layout depends on the image size alone,
 *              levels that are not built (see pyramid) are not written.  Host memory: may be null (staged internally).  Device
 *              memory: required, and written for every pair.
 * Every output but info may be null; in device memory n_keep needs one of status, why and keep_idx, which carries the flags
 * between the kernels (SWF_E_INVALID otherwise).
 * info: SWF_KLT_BAD_INPUT (a non-finite point or guess, tested on what is staged): the pair writes its info only.  rows or cols <= win
 * or > 8192, an even win or one outside 3 .. 21, a level outside 0 .. 4, max_count outside 1 .. 1000, unknown flag bits, more than 2^20
 * pairs, (host memory) a pair above SWF_KLT_NMAX points: SWF_E_UNSUPPORTED; null required pointers, guess_px without bit 1 or bit 1
 * without it, (host memory) a negative or decreasing `first`, eps, min_eig or back_dist not finite and positive: SWF_E_INVALID.  With host
 * memory the BAD_INPUT pairs are found before the device is touched, and a call none of whose pairs has a point to track does not
 * touch it at all.  Device memory: a pair whose offsets are negative, decreasing or above SWF_KLT_NMAX reports info = -1 and writes
 * nothing else.  A pair's result does not depend on the other pairs of the call, and a rerun gives the same bits.  on_device as for
 * swf_preintegrate_batch.  max(max_level, back_level) + 2 launches on the caller's stream. */
enum { SWF_KLT_OK = 0, SWF_KLT_BAD_INPUT = 1 };                      /* per pair */
enum { SWF_KLT_TRACKED = 0, SWF_KLT_FWD_LOST = 1, SWF_KLT_FWD_FLAT = 2, SWF_KLT_BACK_LOST = 3, SWF_KLT_BACK_FLAT = 4,
       SWF_KLT_BACK_FAR = 5, SWF_KLT_BORDER = 6 };                  /* per point: why */
#define SWF_KLT_WMAX 21     /* window side, odd, 3 .. 21 */
#define SWF_KLT_LMAX 4      /* max_level, back_level: 0 .. 4 */
#define SWF_KLT_NMAX 4096   /* points per pair */
size_t swf_klt_pyramid_bytes(int32_t rows, int32_t cols, int32_t max_level);      /* host only: workspace per PAIR (both images, levels 1 ..) */
int swf_klt_track_batch(int32_t n_pairs, int32_t rows, int32_t cols, const uint8_t* prev_img, const uint8_t* cur_img,
                        const int32_t* first, const double* prev_px, const double* guess_px,
                        int32_t win, int32_t max_level, int32_t back_level, int32_t max_count, double eps, double min_eig,
                        double back_dist, int32_t flags,
                        double* cur_px, double* back_px, uint8_t* status, int32_t* why, int32_t* keep_idx, int32_t* n_keep,
                        int32_t* info, int32_t* trace_iters, double* trace_px, uint8_t* pyr, int32_t on_device, void* stream);

/* Input producer: the points to track — setMask, cv::goodFeaturesToTrack(cur_img, n_pts, MAX_CNT - cur_pts.size(), 0.01, MIN_DIST, mask)
 * and addPoints of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:148-165, :44-79) for n_frames independent frames.  It is
 * OpenCV's goodFeaturesToTrack (blockSize 3, Sobel aperture 3, useHarris false) behind the reference's setMask, restated with the
 * declared differences below.  The specification; positions are (x, y), rint and r101(i, n) as for swf_klt_track_batch,
 * r = min_dist:
 *   A setMask  per frame, c_i = (rint(x_i), rint(y_i)); the tracked points are walked by track_cnt descending, then index ascending.
 *              c_i outside [0, cols) x [0, rows): why = OUTSIDE, dropped.  c_i not free: why = CROWDED, dropped.  Otherwise KEPT, and
 *              disc(c_i) is blocked from then on.  free(p): the caller's mask byte at p is non-zero (when a mask is given) and p lies in
 *              no disc of a kept point.  disc(c) = { (x, y) : |y - c.y| <= r, |x - c.x| <= hw[|y - c.y|] }; with disc_halfwidth null
 *              hw[d] = floor(sqrt(r^2 - d^2)), an exact integer square root.  No mask image is rasterised on the device.
 *   B eig      every pixel, P read through r101: Ix = (P(x+1,y-1) - P(x-1,y-1)) + 2 (P(x+1,y) - P(x-1,y)) + (P(x+1,y+1) - P(x-1,y+1)),
 *              Iy the transposed stencil; A = sum Ix^2, B = sum Ix Iy, C = sum Iy^2 over the 3 x 3 neighbourhood, its positions
 *              through r101 (the products are reflected, as cv::boxFilter does); D = (A - C)^2 + 4 B^2;
 *              eig = ((double)(A + C) - sqrt((double)D)) / 18727200.0  (OpenCV's scale 1 / (255 * 4 * 3) squared, the halves folded in).
 *   exactness  |Ix| <= 1020, A <= 9 363 600 < 2^24, D < 2^49: everything up to D is an exact integer; then one subtraction, one
 *              correctly rounded square root and one division, each rounded once, no contraction.  D <= (A + C)^2, so eig >= 0.
 *   C cand     m = max of eig over the free pixels of the whole image; no free pixel or m = 0: no candidates.  t(p) = eig(p) if
 *              eig(p) > quality * m (one double product), else 0.  p is a candidate iff 1 <= x <= cols - 2 and 1 <= y <= rows - 2,
 *              t(p) != 0, t(p) >= t of its eight neighbours (blocked neighbours count: OpenCV's dilation does not look at the
 *              mask), and free(p).
 *   D select   the candidates are walked by t descending, then by linear index y * cols + x descending (OpenCV's greaterThanPtr); a
 *              candidate is kept iff every new point kept before it has dx^2 + dy^2 >= r^2; the walk ends at budget = max_cnt - n_old.
 *              A budget <= 0 skips B to D (n_new = n_cand = 0, max_eig = 0, eig not written).  New points are kept away from old
 *              ones through free() only, as in the reference.
 * Declared differences from OpenCV and the reference: (1) OpenCV forms the derivatives, products, box sums and the eigenvalue in float;
 * here they are exact integers and one double expression, so the operator is not OpenCV bit for bit — it is its own float64 referee
 * (tests/np_gftt.py) bit for bit.  (2) cv::circle's filled raster is replaced by the half-width table; the default is the Euclidean
 * disc, and a caller who wants OpenCV's midpoint raster passes its row half-widths (the values are used as they are: a negative one
 * blocks nothing in its rows).  (3) The reference's std::sort leaves equal track_cnt in unspecified order; here ties go by index.
 * (4) The reference reads mask.at out of range for a point outside the image; here the point is dropped.
 * Arrays:
 *   img        [n_frames][rows][cols]      8-bit grey, dense rows;  mask alike or null: the caller's own mask, 0 = blocked
 *   first      [n_frames + 1]              offsets of the tracked points;  px [..][2], track_cnt [..] after the caller's n++
 *   max_cnt, min_dist, quality             the reference's 350, 30, 0.01;  disc_halfwidth [min_dist + 1] or null
 *   cand_cap                               candidates a frame's workspace can hold
 *   flags      bit 0: px is rounded through float first, where the reference holds a cv::Point2f
 *   order      [..]  the kept indices of a frame (counted from its first point) in kept order from first[k], -1 behind them
 *   why        [..]  SWF_GFTT_KEPT, _OUTSIDE, _CROWDED;  n_old [n_frames]
 *   new_px     [n_frames][max_cnt][2]      integer-valued, in selection order; entries behind n_new are not written;  n_new [n_frames]
 *   n_cand, max_eig [n_frames]             the candidates of stage C;  m (0 where there is no free pixel)
 *   pack_first [n_frames + 1], pack_px [..][2], pack_src [..]: per frame the kept old points' px as given (float-rounded under bit 0)
 *              in kept order, then the new points; pack_src the index from first[k], -1 for a new point.  pack_first[0] = 0; a frame
 *              that writes its info only owns an empty range.  Sized for first[n_frames] - first[0] + n_frames * max_cnt points: the
 *              next call's first / prev_px without a host copy.
 *   work       [n_frames][swf_gftt_workspace_bytes(rows, cols, cand_cap)], 8-byte aligned: the workspace; a frame's first
 *              rows * cols doubles are eig, a stage export.  Device memory: required.  Host memory: may be null (staged
 *              internally); where given, the eig of every SWF_GFTT_OK frame with a budget > 0 is copied back and nothing else.
 * Every output but info may be null.
 * info: SWF_GFTT_BAD_INPUT (a non-finite coordinate, tested on what is staged, or a negative track_cnt): the frame writes its info
 * only.  SWF_GFTT_TOO_MANY (more than cand_cap candidates): the frame writes info and the true n_cand only, so the caller can size the
 * next call.  rows or cols outside 8 .. 8192, max_cnt outside 1 .. 1024, min_dist outside 1 .. 64, cand_cap above 2^24, unknown flag
 * bits, more than 65535 frames, (host memory) a frame above SWF_GFTT_NMAX tracked points: SWF_E_UNSUPPORTED; null required pointers
 * (img, first, px, track_cnt, info; work in device memory), quality outside (0, 1], cand_cap below 64, (host memory) a negative or
 * decreasing `first`: SWF_E_INVALID; all before any launch.  With host memory the BAD_INPUT frames are found before the device is
 * touched, and a call all of whose frames are BAD_INPUT does not touch it.  Device memory: a frame whose offsets are negative,
 * decreasing or above SWF_GFTT_NMAX reports info = -1 and writes nothing else.  A frame's result does not depend on the other frames of
 * the call (pack_first alone counts the frames in front), and a rerun gives the same bits.  on_device as for swf_preintegrate_batch.
 * Six launches on the caller's stream, whatever the arguments. */
enum { SWF_GFTT_OK = 0, SWF_GFTT_BAD_INPUT = 1, SWF_GFTT_TOO_MANY = 2 };   /* per frame */
enum { SWF_GFTT_KEPT = 0, SWF_GFTT_OUTSIDE = 1, SWF_GFTT_CROWDED = 2 };    /* per tracked point: why */
#define SWF_GFTT_NMAX 1024  /* tracked points per frame, and max_cnt */
size_t swf_gftt_workspace_bytes(int32_t rows, int32_t cols, int32_t cand_cap);    /* host only: workspace per FRAME; 0 outside the limits */
int swf_gftt_detect_batch(int32_t n_frames, int32_t rows, int32_t cols, const uint8_t* img, const uint8_t* mask,
                          const int32_t* first, const double* px, const int32_t* track_cnt,
                          int32_t max_cnt, int32_t min_dist, double quality, const int32_t* disc_halfwidth, int32_t cand_cap, int32_t flags,
                          int32_t* order, int32_t* why, int32_t* n_old, double* new_px, int32_t* n_new, int32_t* n_cand, double* max_eig,
                          int32_t* pack_first, double* pack_px, int32_t* pack_src, int32_t* info, uint8_t* work,
                          int32_t on_device, void* stream);

/* The resident feature tracker: FeatureTracker::trackImage (R/feature/feature_tracker.cpp:88-263) and removeOutliers for n_streams
 * independent image sequences whose state (prev_img, prev_pts, ids, track_cnt, n_id, the previous normalised points, prev_time) stays
 * on the device.  swf_tracker_track enqueues one frame of every stream on the tracker's stream: the three operators above
 * through their launchers, unchanged, with the reference's flags (KLT 5, or 1 without flow_back; float rounding bit 0 everywhere),
 * and between them the bookkeeping kernels of swf_tracker.hip.  It does not synchronise, allocate or copy from the device.
 * Per stream, in the reference's order:
 *   1 KLT prev_img -> img from prev_px (not on the tracker's first call: no stream has points); prev_px, cur_px, ids, track_cnt and the
 *     lineage are gathered by keep_idx, a new `first` is the prefix of n_keep
 *   2 track_cnt += 1
 *   3 rejectWithF on the survivors, dt = times[s] - prev_time[s] (1 on a stream's first frame, which has no points), the call's seed;
 *     gathered by its keep_idx.  SWF_TRK_TOO_FEW keeps all, as the reference.  SWF_TRK_NO_MODEL keeps all and sets SWF_TRACKER_NO_MODEL
 *     in info: a declared difference (OpenCV leaves status unwritten there and the reference reads it out of range).
 *   4 setMask, goodFeaturesToTrack, addPoints on img: a kept point carries its id and track_cnt, the j-th new point of the stream gets
 *     id = n_id + j and track_cnt = 1 in selection order, then n_id += n_new.  SWF_GFTT_TOO_MANY: the stream keeps what setMask kept,
 *     adds none, sets SWF_TRACKER_TOO_MANY in info and reports the true n_cand in counts.
 *   5 un = the PINHOLE_FULL lift of the final pixels: swf_track_reject_batch's un_cur for the same pixels, bit for bit
 *   6 velocity = ptsVelocity: for a point of the previous frame's final list the difference in float, the quotient by dt in double,
 *     stored as float; (0, 0) for a new point and on a stream's first frame.  The reference's id maps are replaced by a lineage index
 *     carried through the gathers; ids are unique, so the two agree.
 *   7 obs = (un.x, un.y, 1, px.x, px.y, v.x, v.y), the float values widened to double
 *   8 the state rolls; the two image buffers swap as pointers.
 * counts [n_streams][SWF_TRACKER_NCOUNT]: points in, after KLT, after the F gate, kept by setMask, new, n_cand, final, then the info
 * words of the KLT (0 where it did not run), track-reject and detection stages.  info [n_streams]: the SWF_TRACKER_* bits;
 * SWF_TRACKER_STAGE_FAILED marks a stage info no valid state can produce (BAD_INPUT, -1): that stage then keeps every point.
 * A stream's result does not depend on the other streams, a rerun from the same state gives the same bits, and the number of launches
 * depends on the options and on whether it is the first call, never on the data: 3 bookkeeping kernels, 6 of the detector, 1 of the
 * gate and, from the second call on, max(max_level, back_level) + 2 of the KLT.
 * swf_tracker_create allocates everything (two image buffers, the mask, the KLT pyramids, the detector workspace, max_cnt slots of
 * state per stream, the inter-stage arrays).  Refused before the device is touched, as by the operators it wraps: null cam, opt or
 * out, non-finite or non-positive eps, min_eig, back_dist, f_threshold, focal, non-finite f_confidence or cam, fx or fy of 0, quality
 * outside (0, 1], cand_cap below 64: SWF_E_INVALID; n_streams outside 1 .. 65535, win even or outside 3 .. 21, rows or cols <= win,
 * below 8 or above 8192, levels outside 0 .. 4, max_count outside 1 .. 1000, max_cnt outside 1 .. SWF_GFTT_NMAX, min_dist outside
 * 1 .. 64, cand_cap above 2^24, f_iterations outside 1 .. SWF_TRK_HMAX, negative virt_col or virt_row: SWF_E_UNSUPPORTED.
 * swf_tracker_track: times is host memory; img is [n_streams][rows][cols] in host memory, or device memory with img_on_device (then
 * mask too); a host image is copied in with hipMemcpyAsync on the tracker's stream.  Null t, times or img, a non-finite time or one
 * not strictly above the stream's previous time: SWF_E_INVALID before any launch, the state untouched.
 * swf_tracker_remove_ids is removeOutliers: the ids[first[s] .. first[s + 1]) leave stream s's prev_px, ids and track_cnt, order
 * preserved; an id that is not there is ignored; the previous normalised points stay.  More than max_cnt ids for a stream:
 * SWF_E_UNSUPPORTED; a negative or decreasing first, null pointers: SWF_E_INVALID.  Two launches, no synchronisation.
 * swf_tracker_download synchronises and copies the frame the last swf_tracker_track produced (a later remove_ids shows in the next
 * frame): n [n_streams], and ids, track_cnt, obs [..][7] packed stream after stream (at most n_streams * max_cnt points); any pointer
 * may be null.  SWF_E_STATE before the first track.  swf_tracker_device_frame gives the device pointers of the same frame: first
 * [n_streams + 1], ids, track_cnt, px [..][2], obs [..][7]; first and px are the first / prev_px of swf_klt_track_batch.
 * Not covered: setPrediction / hasPrediction (never called in the reference), the stereo branch (USE_STEREO 0 in every shipped
 * configuration), drawTrack, and streams that skip a frame (every call carries a frame for every stream). */
typedef struct swf_tracker swf_tracker;
typedef struct swf_tracker_options {   /* swf_tracker_default_options fills the reference's values */
    int32_t max_cnt, min_dist;          /* MAX_CNT 350 (<= SWF_GFTT_NMAX), MIN_DIST 30 */
    double  quality;                    /* 0.01 */
    int32_t cand_cap;                   /* 1 << 15 */
    int32_t win, max_level, back_level, max_count;   /* 21, 3, 1, 30 */
    double  eps, min_eig, back_dist;    /* 0.01, 1e-4, 0.5 */
    int32_t flow_back;                  /* FLOW_BACK: 1 */
    int32_t f_iterations; double f_threshold, f_confidence, focal;   /* 1000, F_THRESHOLD 1.0, 0.99, FOCAL_LENGTH 1000 */
    int32_t virt_col, virt_row;         /* the col / row of rejectWithF's virtual camera: 0 = the image's */
} swf_tracker_options;
enum { SWF_TRACKER_NO_MODEL = 1, SWF_TRACKER_TOO_MANY = 2, SWF_TRACKER_STAGE_FAILED = 4 };   /* info bits */
enum { SWF_TRACKER_C_IN = 0, SWF_TRACKER_C_KLT = 1, SWF_TRACKER_C_F = 2, SWF_TRACKER_C_MASK = 3, SWF_TRACKER_C_NEW = 4, SWF_TRACKER_C_CAND = 5,
       SWF_TRACKER_C_FINAL = 6, SWF_TRACKER_C_KLT_INFO = 7, SWF_TRACKER_C_TRK_INFO = 8, SWF_TRACKER_C_GFTT_INFO = 9 };
#define SWF_TRACKER_NCOUNT 10
void swf_tracker_default_options(swf_tracker_options*);
int swf_tracker_create(int32_t n_streams, int32_t rows, int32_t cols, const double cam[12], const swf_tracker_options* opt,
                       void* stream, swf_tracker** out);
int swf_tracker_track(swf_tracker* t, const double* times /* host, [n_streams] */, const uint8_t* img /* [n_streams][rows][cols] */,
                      const uint8_t* mask /* or null */, uint64_t seed, int32_t img_on_device);
int swf_tracker_remove_ids(swf_tracker* t, const int32_t* first /* host, [n_streams + 1] */, const int32_t* ids /* host */);
int swf_tracker_download(swf_tracker* t, int32_t* n /* [n_streams] */, int32_t* ids, int32_t* track_cnt, double* obs /* [..][7] */,
                         int32_t* counts /* [n_streams][SWF_TRACKER_NCOUNT] */, int32_t* info /* [n_streams] */);
int swf_tracker_device_frame(swf_tracker* t, const int32_t** first, const int32_t** ids, const int32_t** track_cnt,
                             const double** px, const double** obs);   /* device pointers of the current frame, for chaining */
int swf_tracker_sync(swf_tracker* t);
int swf_tracker_destroy(swf_tracker* t);

/* The resident feature table: FeatureManager (R/feature/feature_manager.cpp) as ImagePreprocess, ImagePostprocess, SlideWindowOld and
 * SlideWindowNew drive it (R/swf/swf_image.cpp:27-62, 115-127, 313-320), for n_streams independent windows whose track table stays on
 * the device.  It consumes swf_tracker_device_frame and produces the inputs of swf_pnp_frame_batch, swf_triangulate_batch
 * and the flat window's lm / proj_idx / proj_uv.  Scope: the reference's compiled default, USE_INVERSE_DEPTH 0, USE_STEREO 0,
 * FEATURE_CONTINUE 2.  Every operation is asynchronous on the table's stream, handles all streams in one call with one workgroup per
 * stream, and does not synchronise, allocate or copy from the device; the number of launches depends on the operation alone (given
 * with each).  Arrays are host memory, or device memory with on_device; tic, ric (row-major), pbg and mode are always host memory.
 * State per stream: n_frames (the reference's image_count) and a list of at most feat_cap features IN THE REFERENCE'S LIST ORDER
 * (insertion order, every erase a stable compaction; not sorted by id).  Per feature: id, start_frame, n_obs, valid, solve_flag,
 * idepth, world[3] and up to `window` observations, each the tracker's 7-vector x y z u v vx vy with an in_problem bit.
 * endFrame = start_frame + n_obs - 1.
 *
 * 1 swf_ftable_add_frame — addFeatureCheckParallax (:40-77), then removeOut (:418-425).  first [n_streams + 1], ids, obs [..][7] are
 *   what swf_tracker_device_frame returns.  image_index = n_frames.  The frame's points are taken in ascending id (the reference
 *   iterates a std::map; the tracker's frame is not sorted).  A found id appends its observation (in_problem clear), counts in
 *   last_track_num and, when n_obs >= long_len after the append, in long_track_num.  An id not found is appended at the end of the
 *   list with start_frame = image_index, valid = 0, solve_flag = 0, idepth = 0, world = 0 and counts in new_feature_num.
 *   keyframe = image_index < 2 || last_track_num < min_track || long_track_num < min_long || new_feature_num > new_ratio * last_track_num.
 *   Then n_frames += 1, then every feature with endFrame != n_frames - 1 && n_obs < feature_continue is erased.  counts: KEYFRAME,
 *   LAST_TRACK, LONG_TRACK, NEW, ERASED, INFO.  Info bits: SWF_FTABLE_WINDOW_FULL (n_frames == window already) and SWF_FTABLE_BAD_FRAME
 *   (an id twice in the frame, more than frame_cap points, offsets that are negative or decreasing, a non-finite observation): the
 *   stream is left exactly as it was, n_frames included, its counters 0.  SWF_FTABLE_TABLE_FULL: the j-th new id, ascending, is taken
 *   while (features before the call) + j < feat_cap; the others are dropped and not counted — a declared difference.   1 launch.
 * 2 swf_ftable_pnp_points — the gather of initFramePoseByPnP (:207-228, world-point branch) with frameCnt = n_frames - 1: the valid
 *   features with n_obs >= frameCnt - start_frame + 1, in list order, give world and x, y of the observation at frameCnt - start_frame.
 *   The three out-pointers receive device arrays in swf_pnp_frame_batch's first / pts_w / pts_uv layout.  n_frames < 2: an empty
 *   range.   2 launches.
 * 3 swf_ftable_triangulate — triangulate (:245-316), the branch every feature with !valid && n_obs > 1 takes.  Ps [n_streams][window][3],
 *   Rs [..][9] row-major by image frame.  A gather kernel writes start (s * window + start_frame, or -1 for a slot that is not to be
 *   triangulated), pt0, pt1 for all n_streams * feat_cap slots, swf_triangulate_batch runs over them on device memory, a scatter
 *   kernel takes the rows whose depth is not the -1 sentinel: idepth = 1 / depth, world, valid = 1.  Bit-identical to
 *   swf_triangulate_batch on the same inputs.  The stereo branch and the N-view SVD (unreachable for feature_continue >= 2) are not
 *   covered.   3 launches.
 * 4 swf_ftable_list — AddFeature2Problem (R/swf/swf_image.cpp:65-114, world-point branch) as data: the features with
 *   n_obs >= feature_continue in list order, their observations in frame order from start_frame.  Packed per stream behind lm_first /
 *   proj_first [n_streams + 1]: lm_id, lm_world [..][3], lm_start, lm_nobs, lm_valid; proj_frame, proj_lm (an index into the stream's
 *   listed landmarks), proj_uv [..][2] (x, y), proj_new (1 when in_problem was clear).  The call sets in_problem on everything it
 *   lists and remembers the stream's landmark count.  counts: N_LISTED, N_PROJ.   2 launches.
 * 5 swf_ftable_set_solved — the landmark tail of Double2Vector (R/swf/swf.cpp:214-228) and the verdict of OutliersRejection.
 *   lm_world [..][3] behind lm_first, in the order of the last listing, is written to world; pts_cj = ric^T (Rs[start]^T (world - Ps[start])
 *   + pbg - tic), idepth = 1 / pts_cj.z, solve_flag = idepth < 0 ? 2 : 1.  A non-null flags [..] (what swf_batch_get_feature_check
 *   returns) with SWF_FEAT_OUTLIER or SWF_FEAT_NEG_DEPTH set makes solve_flag 2.  A stream whose features with n_obs >= feature_continue,
 *   or whose lm_first range, do not number what its last listing did sets SWF_FTABLE_STALE_LIST and is left untouched.   1 launch.
 * 6 swf_ftable_remove_failures — removeFailures (:122-139): the features with solve_flag == 2 are erased; the out-pointers receive
 *   device first [n_streams + 1] / ids of the erased, packed, in list order.  swf_ftable_removed downloads them for
 *   swf_tracker_remove_ids.  counts: ERASED.   2 launches.
 * 7 swf_ftable_check_parallax — CheckParallax(n_frames - 1) with compensatedParallax2 (:81-101, 469-498), idx = n_frames - 1: over the
 *   features with start_frame <= idx - 2 && endFrame >= idx - 1, sequentially in list order, term = sqrt(du du + dv dv),
 *   du = x_i / z_i - x_j, dv = y_i / z_i - y_j, i and j the observations of frames idx - 2 and idx - 1.  counts: PARALLAX_NUM,
 *   KEYFRAME = num == 0 || sum / num >= min_parallax; parallax [n_streams] = sum / num * focal (0 for num == 0).   1 launch.
 * 8 swf_ftable_slide — mode [n_streams]: 0 leaves the stream alone.  1 is removeBack (:362-391): start_frame != 0 decrements it;
 *   otherwise pts_cj = ric^T (R1^T (world - P1) + pbg - tic), idepth = 1 / pts_cj.z and observation 0 is erased.  2 is
 *   removeFront(n_frames - 1) (:393-416), literally: start_frame == n_frames - 1 decrements it, otherwise a feature with
 *   endFrame >= n_frames - 2 loses observation j = n_frames - 2 - start_frame (j == 0 included).  A feature left with no observation is
 *   erased (the reference asserts there: a declared difference, the release build's behaviour).  Both then set n_frames -= 1 and clear
 *   in_problem on every observation of a feature with n_obs < feature_continue (removeOut2's world-point effect, :427-447).  P1 [n_streams][3],
 *   R1 [..][9]; P0, R0 are the reference's arguments, unread in world-point mode, and may be null.  Mode 1 or 2 with n_frames < 2,
 *   or another mode: SWF_FTABLE_BAD_SLIDE, nothing done.  counts: ERASED, INFO.   1 launch.
 * 9 swf_ftable_create allocates everything.  swf_ftable_download synchronises and copies the whole state in capacity layout:
 *   n_frames, n_feat [n_streams]; id, start_frame, n_obs, valid, solve_flag, idepth [n_streams][feat_cap]; world [..][3];
 *   obs [..][window][7]; in_problem [..][window]; any pointer may be null.  swf_ftable_counts synchronises and copies counts
 *   [n_streams][SWF_FTABLE_NCOUNT] and parallax [n_streams]; every operation overwrites the words named with it, INFO included.
 *   swf_ftable_clear is ClearState with n_frames = 0.
 * Refused before the device is touched: null pointers, non-finite options: SWF_E_INVALID; n_streams outside 1 .. 65535, window outside
 * 3 .. 32, feat_cap outside 1 .. 65536, frame_cap outside 1 .. SWF_PNP_NMAX, feature_continue outside 2 .. window: SWF_E_UNSUPPORTED; a
 * host-memory first that is negative or decreasing: SWF_E_INVALID.
 * A stream's result does not depend on the other streams, and a rerun from the same state gives the same bits.  Declared differences:
 * TABLE_FULL, the erase where the reference asserts, world-point mode only. */
typedef struct swf_ftable swf_ftable;
typedef struct swf_ftable_options {    /* swf_ftable_default_options fills the reference's values */
    int32_t window, feat_cap, frame_cap;            /* FEATURE_WINDOW_SIZE + 1 = 11, 4096, the tracker's max_cnt 350 */
    int32_t feature_continue, min_track, min_long, long_len;   /* 2, 20, 40, 4 */
    double  new_ratio, min_parallax, focal, init_depth;        /* 0.5, keyframe_parallax / FOCAL_LENGTH = 10 / 1000, 1000, 5.0 */
} swf_ftable_options;
typedef struct swf_ftable_listing {    /* device pointers, valid until the next swf_ftable_list */
    const int32_t* lm_first; const int32_t* proj_first;
    const int32_t* lm_id; const double* lm_world; const int32_t* lm_start; const int32_t* lm_nobs; const int32_t* lm_valid;
    const int32_t* proj_frame; const int32_t* proj_lm; const double* proj_uv; const int32_t* proj_new;
} swf_ftable_listing;
enum { SWF_FTABLE_WINDOW_FULL = 1, SWF_FTABLE_TABLE_FULL = 2, SWF_FTABLE_BAD_FRAME = 4, SWF_FTABLE_STALE_LIST = 8, SWF_FTABLE_BAD_SLIDE = 16 };
enum { SWF_FTABLE_C_KEYFRAME = 0, SWF_FTABLE_C_LAST_TRACK = 1, SWF_FTABLE_C_LONG_TRACK = 2, SWF_FTABLE_C_NEW = 3, SWF_FTABLE_C_ERASED = 4,
       SWF_FTABLE_C_INFO = 5, SWF_FTABLE_C_PARALLAX_NUM = 6, SWF_FTABLE_C_N_LISTED = 7, SWF_FTABLE_C_N_PROJ = 8, SWF_FTABLE_C_N_PNP = 9 };
#define SWF_FTABLE_NCOUNT 10
void swf_ftable_default_options(swf_ftable_options*);
int swf_ftable_create(int32_t n_streams, const swf_ftable_options* opt, void* stream, swf_ftable** out);
int swf_ftable_add_frame(swf_ftable* t, const int32_t* first, const int32_t* ids, const double* obs, int32_t on_device);
int swf_ftable_pnp_points(swf_ftable* t, const int32_t** first_out, const double** pts_w, const double** pts_uv);
int swf_ftable_triangulate(swf_ftable* t, const double* Ps, const double* Rs, const double tic[3], const double ric[9], const double pbg[3],
                           int32_t on_device);
int swf_ftable_list(swf_ftable* t, swf_ftable_listing* out);
int swf_ftable_set_solved(swf_ftable* t, const int32_t* lm_first, const double* lm_world, const uint8_t* flags /* or null */,
                          const double* Ps, const double* Rs, const double tic[3], const double ric[9], const double pbg[3], int32_t on_device);
int swf_ftable_remove_failures(swf_ftable* t, const int32_t** first_out, const int32_t** ids_out);
int swf_ftable_removed(swf_ftable* t, int32_t* first /* host, [n_streams + 1] */, int32_t* ids /* host, up to n_streams * feat_cap */);
int swf_ftable_check_parallax(swf_ftable* t);
int swf_ftable_slide(swf_ftable* t, const int32_t* mode /* host */, const double* P0, const double* R0, const double* P1, const double* R1,
                     const double tic[3], const double ric[9], const double pbg[3], int32_t on_device);
int swf_ftable_download(swf_ftable* t, int32_t* n_frames, int32_t* n_feat, int32_t* id, int32_t* start_frame, int32_t* n_obs, int32_t* valid,
                        int32_t* solve_flag, double* idepth, double* world, double* obs, int32_t* in_problem);
int swf_ftable_counts(swf_ftable* t, int32_t* counts /* [n_streams][SWF_FTABLE_NCOUNT] */, double* parallax /* [n_streams] */);
int swf_ftable_fetch(swf_ftable* t, void* dst, const void* device_src, uint64_t bytes);   /* synchronise, then copy a device array out */
int swf_ftable_sync(swf_ftable* t);
int swf_ftable_clear(swf_ftable* t);
int swf_ftable_destroy(swf_ftable* t);

/* Input producer: two-view landmark triangulation for a batch of features — FeatureManager::triangulate, the branch every
 * feature with >= 2 observations takes (R/feature/feature_manager.cpp:285-316), with triangulatePoint (:148-161).
 *   Ps [n_frames][3], Rs [n_frames][9] (row-major)  frame positions / rotations as the reference passes them
 *   tic, ric (row-major), pbg                        camera extrinsic and the IMU->antenna lever arm
 *   start_frame [n]                                  first observing frame i of each feature (the second view is i + 1);
 *                                                    concatenate the frames of many windows and use absolute indices
 *   pt0, pt1 [n][2]                                  normalised image coordinates in frames i and i + 1
 *   depth [n]                                        depth in camera i; init_depth (INIT_DEPTH, R/parameter/parameters.h:29) when the
 *                                                    triangulated depth is not positive; -1 for an out-of-range start_frame
 *   pts_world [n][3]                                 Rs[i] (ric (pt0 depth) + tic - pbg) + Ps[i], the landmark block's initial value
 * on_device as for swf_preintegrate_batch. */
int swf_triangulate_batch(const double* Ps, const double* Rs, int32_t n_frames, const double tic[3], const double ric[9],
                          const double pbg[3], const int32_t* start_frame, const double* pt0, const double* pt1, int32_t n,
                          double init_depth, double* depth, double* pts_world, int32_t on_device, void* stream);

/* Inverse-depth projection factors for a batch, one lane per factor — the stand-alone evaluator (parity
 * against the oracle).  Inside the solver the same factors are a factor type of the loop: swf_flat_window::idp_* /
 * swf_add_projection_inverse_depth, the inverse depth being a scalar block of elimination group 0.
 *   kind [n]      0 ProjectionTwoFrameOneCamFactor (R/factor/projection_factor.cpp:179-256): pose_i, pose_j, ex, lambda
 *                 1 ProjectionTwoFrameTwoCamFactor (:77-166): pose_i, pose_j, ex, ex2, lambda
 *                 2 ProjectionOneFrameTwoCamFactor (:269-329): ex, ex2, lambda
 *   idx  [n][5]   pose_i, pose_j, ex, ex2 (rows of poses [n_pose][7]; ignored where the kind has none), lambda (row of lambda [n_lambda])
 *   pts  [n][6]   pts_i (3), pts_j (3): the normalised observations in the anchor and in the second view
 *   r    [n][2];  J [n][50] = d r / d pose_i (2x6, local) | pose_j | ex | ex2 | lambda (2); blocks a kind does not have are zero */
int swf_eval_inverse_depth_batch(const int32_t* kind, const int32_t* idx, int32_t n, const double* poses, int32_t n_pose,
                                 const double* lambda, int32_t n_lambda, const double* pts, double sqrt_info, const double pbg[3],
                                 double* r, double* J, int32_t on_device, void* stream);

/* =====================================================================================
 * Composite IMU-GNSS factors as a batched, stateful device operator
 *
 * IMUGNSSBase / IMUGNSSFactor (R/factor/gnss_imu_factor.cpp): n factors, each hiding M[f] GNSS-epoch states between two
 * visual frames behind N[f] <= 24 ambiguities.  Arrays are concatenated over the factors in order:
 *   pose, sb            [sum M][7], [sum M][9]   hidden epochs (gnss_poses / gnss_speed_bias), copied: the handle owns them
 *   pose_lin, sb_lin    linearisation points of the per-epoch GNSS priors
 *   Hpp [sum M][225], HpN [sum 15 M N], rhs_p [sum M][15], HNN [sum N N], rhsN [sum N]   the blocks AddMargInfo :245-352 keeps
 *   pre                 [sum M + n][SWF_PRE_DOUBLES]: factor f owns M[f] + 1 records: frame_i -> e_0, ..., e_M-1 -> frame_j
 * swf_composite_evaluate = IMUGNSSBase::Evaluate (:678-799) for all factors at once:
 *   outer [n][32] = pose_i(7) sb_i(9) pose_j(7) sb_j(9), Nv [sum N] = the ambiguity values
 *   want_jac != 0: back-substitute the hidden epochs from the outer increment, re-eliminate, return the (30+N)-vector
 *                  residual and the (30+N)^2 Jacobian (row-major, columns = local [pose_i sb_i | pose_j sb_j | N]) of each factor;
 *   want_jac == 0: the linear model r_lin - J INC of the last linearisation (the first call linearises).
 * The Jacobian is the Cholesky square root L^T of the remaining system (the reference takes the eigen square root: same
 * J^T J and J^T r whenever the remainder is positive definite; status[f] = -1 reports a factor where it was not).
 * Hd / rd (optional) receive the remaining system itself ((30+N)^2, 30+N per factor).  Host pointers; synchronous.
 * ===================================================================================== */
typedef struct swf_composite swf_composite;
int swf_composite_create(int32_t n, const int32_t* M, const int32_t* N, const double* pose, const double* sb,
                         const double* pose_lin, const double* sb_lin, const double* Hpp, const double* HpN,
                         const double* rhs_p, const double* HNN, const double* rhsN, const double* pre,
                         const double pbg[3], const double gw[3], void* stream, swf_composite** out);
int swf_composite_evaluate(swf_composite* c, const double* outer, const double* Nv, int32_t want_jac,
                           double* residual, double* jac, double* Hd, double* rd, int32_t* status);
int swf_composite_hidden(swf_composite* c, double* pose, double* sb);
/* The middle-marginalisation branch (AddMidMargInfo :121-240, Evaluate :738-759): mid[f] = k in 1..M[f]-1 replaces the IMU factor of
 * the link e_k-1 -> e_k by the cross block H12[f] (15 x 15 row-major, rows = e_k-1, columns = e_k) of a marginalised stretch of
 * epochs; 0 = none.  Call before the first evaluation. */
int swf_composite_set_mid_links(swf_composite* c, const int32_t* mid, const double* H12);
/* Which square root of the remaining system the factor exposes.  SWF_ROOT_PIVOTED_CHOLESKY (default): rows v_r of a diagonally pivoted
 * outer-product Cholesky.  SWF_ROOT_EIGEN: the reference's own (UpdateSchurComponent :454-488): J = sqrt(lam+) V^T, r = lam+^-1/2 V^T rhs,
 * eigenvalues <= 1e-8 dropped, rows in ascending eigenvalue order — the reference's residual vector up to the sign of each eigenvector.
 * Both give the same J^T J and J^T r (to rounding; the pivoted root stops at pivots the eigen root's absolute 1e-8 cut may keep, and
 * the directions kept by one and dropped by the other are rounding noise of a matrix with entries ~1e8: their r_k = v_k^T rhs / sqrt(lam_k)
 * are O(1), so |r|^2 — the factor's contribution to the COST — differs by a constant of that size, the gradient and the step do not).
 * Inside a solve (swf_flat_window::comp_*) swf_options::composite_root selects the form for every composite factor of the solve
 * (enum in swf_types.h). */
int swf_composite_set_root(swf_composite* c, int32_t form);
int swf_composite_destroy(swf_composite* c);

/* =====================================================================================
 * The construction side of the composite factor: per-epoch GNSS pre-elimination and AddMargInfo
 *
 * swf_batch_marginal_priors: MarginalizationInfo::marginalize (R/factor/marginalization_factor.cpp:260-377) for n small problems
 * at once — what GnssPreprocess runs for every GNSS epoch (R/swf/swf_gnss.cpp:504-532: the epoch's raw factors, receiver clocks
 * dropped, {pose, speed-bias, ambiguities, dummy} kept).  Each problem is a flat window whose KEPT blocks are its parameter_head
 * tail (n_tail) and whose dropped blocks are ordered before it (independent ones, the clocks, in group 0); one batch through the
 * engine with step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY, then swf_batch_marginalize(eps, form).  Outputs, concatenated over the
 * problems in order: dims[i] = dimension of prior i (sum of the kept blocks' local sizes, in tail order), ranks[i], A (dims^2,
 * row-major), b, J, r0 (see swf_batch_marginalize).  A / b / J / r0 / ranks may be NULL (dims only: a sizing call).  Host
 * pointers; synchronous.  The priors are linearised at the windows' current values (the reference zeroes the ambiguities
 * first, PhaseBiasSaveAndReset, R/swf/swf_gnss.cpp:516: do the same in the windows you pass).
 *
 * swf_composite_assemble: IMUGNSSBase::AddMargInfo (R/factor/gnss_imu_factor.cpp:245-352) for a chain of M epochs — pure host
 * bookkeeping.  Epoch e keeps n_kept[e] blocks; kept_size (7 / 9 / 1) and kept_key (the block's address; only the scalars' are
 * looked at) are concatenated over the epochs in prior order, as are A (dim_e^2) and b (dim_e).  The scalar blocks become the
 * factor's ambiguities in first-seen order: *N_out of them, their keys in N_keys.  Hpp [M][225], HpN [M][15][N_cap], rhs_p [M][15],
 * HNN [N_cap][N_cap], rhsN [N_cap] receive what swf_add_imu_gnss / swf_flat_window::comp_* expect (pose rows 0..5, speed-bias rows
 * 6..14 of an epoch's 15-block; the N x N block and its right-hand side accumulate over the epochs).  Passing Hpp = NULL only counts
 * (*N_out).  N_cap = the N the caller sized HpN / HNN / rhsN / N_keys for — and the STRIDE of their ambiguity dimension, here and in
 * swf_composite_add_mid_prior alike (so the two calls chain on the same buffers; compact to *N_out / *N_io before handing the arrays
 * to swf_add_imu_gnss if N_cap was larger).  swf_batch_marginal_priors reports a window whose marginal could not be formed with
 * ranks[i] = -1 (and zeros in its slots): check the ranks before filing the priors into a composite factor.
 * ===================================================================================== */
int swf_batch_marginal_priors(const swf_flat_window* const* windows, int32_t n, double eps, int32_t form,
                              int32_t* dims, int32_t* ranks, double* A, double* b, double* J, double* r0, void* stream);
int swf_composite_assemble(int32_t M, const int32_t* n_kept, const int32_t* kept_size, double* const* kept_key,
                           const double* A, const double* b, int32_t N_cap, double** N_keys, int32_t* N_out,
                           double* Hpp, double* HpN, double* rhs_p, double* HNN, double* rhsN);
/* swf_prior_reset_linearization_point: MarginalizationInfo::ResetLinearizationPoint (R/factor/marginalization_factor.cpp:232-258;
 * called on the two priors bounding a middle marginalisation, R/swf/swf_core.cpp:636-637) — host bookkeeping on the prior's own arrays.
 * kept_size[n_kept] = global sizes of the kept blocks in kept order (7 = pose), x_new[k] = the block's current values, dim = sum of the
 * local sizes.  dx_k = x_new - x0 (pose: [p - p0 ; +-2 vec(q0^-1 q)], sign of the scalar part, as MarginalizationFactor::Evaluate);
 * r0 += J dx (linearized_residuals, J dim x dim row-major), b += A dx (either pair may be NULL), x0 (concatenated global sizes) <- x_new.
 * (The reference asserts that scalar blocks hold 0 at the call — PhaseBiasSaveAndReset zeroes them first; not enforced here.) */
int swf_prior_reset_linearization_point(int32_t n_kept, const int32_t* kept_size, const double* const* x_new, int32_t dim,
                                        const double* J, const double* A, double* r0, double* b, double* x0);
/* swf_composite_add_mid_prior: IMUGNSSBase::AddMidMargInfo (R/factor/gnss_imu_factor.cpp:121-240) — host bookkeeping.  The prior
 * (A, b) of a marginalised stretch of GNSS epochs (MargGNSSFrames, R/swf/swf_core.cpp:570-641) keeps n_kept blocks: the pose (7) and
 * speed-bias (9) of the two epochs either side of the stretch — kept_epoch[q] = k-1 or k for those blocks (ignored for scalars) — and
 * ambiguities (1, identified by kept_key).  Its diagonal / ambiguity blocks are ADDED into the factor's arrays (laid out for N_cap
 * ambiguities per row: HpN [M][15][N_cap], HNN [N_cap][N_cap], rhsN [N_cap]; N_keys holds *N_io keys on entry), ambiguities it
 * sees first are appended (*N_io grows; SWF_E_INVALID beyond N_cap), and the cross block between the two epochs is returned in
 * H12 (15 x 15 row-major, rows = e_k-1): pass k and H12 on as comp_mid / comp_H12 (swf_set_imu_gnss_mid_link,
 * swf_composite_set_mid_links).  Compact HpN / HNN to stride *N_io afterwards if N_cap was larger. */
int swf_composite_add_mid_prior(int32_t M, int32_t k, int32_t n_kept, const int32_t* kept_size, const int32_t* kept_epoch,
                                double* const* kept_key, const double* A, const double* b, int32_t N_cap, double** N_keys,
                                int32_t* N_io, double* Hpp, double* HpN, double* rhs_p, double* HNN, double* rhsN, double* H12);

/* =====================================================================================
 * (2) ceres::Problem-shaped single-window surface
 *
 * Parameter blocks are identified BY ADDRESS like in Ceres; values are read through the
 * pointer at swf_problem_solve() and written back before it returns.
 * ===================================================================================== */
typedef struct swf_problem swf_problem;
/* Factor ids are SLOT numbers: stable while the factor lives; the slot of a removed factor is handed out again (LIFO) to a later
 * swf_add_*, so an id held across its own swf_remove_factor / a cascading swf_remove_parameter_block may name a DIFFERENT live factor
 * afterwards (it does not become SWF_E_NOTFOUND) — drop ids when you remove, as with ceres::ResidualBlockId.  The flat window is built
 * in slot order, so a long-lived problem and a freshly built one with the same factors may sum in a different factor order (results
 * agree to rounding, not bit for bit). */
typedef int32_t swf_factor_id;

enum { SWF_MANIFOLD_NONE = 0, SWF_MANIFOLD_POSE = 1 };   /* PoseLocalParameterization, 7 -> 6 */

int swf_problem_create(swf_problem** out);                      /* ceres::Problem()            */
int swf_problem_destroy(swf_problem* p);

/* ceres::Problem::AddParameterBlock(ptr, size, LocalParameterization*).  size in {7,9,3,1}.  The manifold is fixed by the
 * size — a 7-block is a pose on PoseLocalParameterization whether or not `manifold` says so, everything else is Euclidean —
 * so calling it on an existing block to (re)attach the parameterization (R/swf/swf_core.cpp:53-56) is accepted and changes
 * nothing. */
int swf_add_parameter_block(swf_problem* p, double* key, int32_t size, int32_t manifold);
int swf_has_parameter_block(swf_problem* p, const double* key);           /* 1 / 0             */
int swf_remove_parameter_block(swf_problem* p, double* key);    /* cascades to its factors     */
int swf_set_parameter_block_constant(swf_problem* p, double* key);
int swf_set_parameter_block_variable(swf_problem* p, double* key);
int swf_is_parameter_block_constant(swf_problem* p, const double* key);   /* 1 / 0             */
int swf_parameter_block_size(swf_problem* p, const double* key);
int swf_num_parameter_blocks(swf_problem* p);
int swf_num_residual_blocks(swf_problem* p);

/* Typed AddResidualBlock()s.  Each returns the factor id (>= 0) or a negative error.
 * Unknown parameter blocks are added implicitly, as ceres does. */
/* projection_factor(pts) + CauchyLoss(loss_a) (R/swf/swf_image.cpp:98-100); loss_a<=0: no loss */
swf_factor_id swf_add_projection(swf_problem* p, double* pose, double* ex_pose, double* point,
                                 const double uv[2], double sqrt_info, double loss_a);
/* IMUFactor(pre_integration) (R/swf/swf_imu.cpp:185-193); pre = SWF_PRE_DOUBLES record */
swf_factor_id swf_add_imu(swf_problem* p, double* pose_i, double* sb_i, double* pose_j, double* sb_j,
                          const double* pre);
/* RTKCarrierPhaseFactor (R/swf/swf_core.cpp:113-117); dat = SWF_CP_DOUBLES record */
swf_factor_id swf_add_rtk_carrier_phase(swf_problem* p, double* pose, double* ambiguity, double* clock,
                                        const double* dat);
/* RTKPseudorangeFactor (R/swf/swf_core.cpp:130-133); dat = SWF_PR_DOUBLES record */
swf_factor_id swf_add_rtk_pseudorange(swf_problem* p, double* pose, double* clock, const double* dat);
/* SppDopplerFactor (R/swf/swf_core.cpp:197-201); dat = SWF_DOP_DOUBLES record */
swf_factor_id swf_add_doppler(swf_problem* p, double* speed_bias, double* clock_drift, double* pose,
                              const double* dat);
/* SppPseudorangeFactor (R/swf/swf_core.cpp:157-163); dat = SWF_SPR_DOUBLES record (sat[3] P1 istd) */
swf_factor_id swf_add_spp_pseudorange(swf_problem* p, double* pose, double* clock, const double* dat);
/* SppCarrierPhaseFactor (R/swf/swf_core.cpp:170-190); block order pose, clock, ambiguity as in the reference;
 * dat = SWF_SCP_DOUBLES record (sat[3] L1_lam istd lam) */
swf_factor_id swf_add_spp_carrier_phase(swf_problem* p, double* pose, double* clock, double* ambiguity,
                                        const double* dat);
/* FixedIntegerFactor(N21, istd) (R/swf/swf_lambda.cpp:318-330): r = istd ((*n_b - *n_a) - N21) */
swf_factor_id swf_add_fixed_integer(swf_problem* p, double* n_a, double* n_b, double N21, double istd);
/* ProjectionTwoFrameOneCamFactor (kind 0) / ProjectionTwoFrameTwoCamFactor (1) / ProjectionOneFrameTwoCamFactor (2)
 * (R/factor/projection_factor.h:33-66, USE_INVERSE_DEPTH builds) + CauchyLoss(loss_a): inv_depth is a one-dimensional block (the
 * feature's inverse depth along pts_i in the anchor frame), normally ordered into group 0 like the world-point landmarks.
 * Blocks a kind does not have are ignored.  sqrt_info / loss_a must equal those of the other projection factors. */
swf_factor_id swf_add_projection_inverse_depth(swf_problem* p, int32_t kind, double* pose_i, double* pose_j, double* ex, double* ex2,
                                               double* inv_depth, const double pts_i[3], const double pts_j[3], double sqrt_info, double loss_a);
/* IMUGNSSFactor(IMUGNSS_info) (R/swf/swf.cpp:713-730, R/factor/gnss_imu_factor.cpp:99-119): the composite factor over
 * (pose_i, sb_i, pose_j, sb_j, N ambiguities) hiding M GNSS epochs.  hidden_pose [M][7] / hidden_sb [M][9] are the epochs'
 * parameter memory (gnss_poses / gnss_speed_bias): read at every solve, updated in place by it.  The other arrays (copied)
 * are laid out as in swf_composite_create for one factor; pre holds M + 1 records.  Its blocks must be variable; at most ONE of them
 * may be in elimination group 0 (MyOrdering puts every other speed-bias block there, R/swf/swf_gnss.cpp:683-691: pass the ordering as it
 * is — the factor's rows then join that block's clique); N <= 64 (SWF_MAX_COMPOSITE_AMBIGUITIES). */
swf_factor_id swf_add_imu_gnss(swf_problem* p, double* pose_i, double* sb_i, double* pose_j, double* sb_j, double* const* ambiguities,
                               int32_t N, int32_t M, double* hidden_pose, double* hidden_sb, const double* pose_lin, const double* sb_lin,
                               const double* Hpp, const double* HpN, const double* rhs_p, const double* HNN, const double* rhsN, const double* pre);
/* the factor's middle-marginalisation link (IMUGNSSBase::AddMidMargInfo): see swf_flat_window::comp_mid / comp_H12.  k = 0 clears it. */
int swf_set_imu_gnss_mid_link(swf_problem* p, swf_factor_id id, int32_t k, const double* H12);
/* InitialBlackFactor(w) (R/swf/swf_core.cpp:553-556) */
swf_factor_id swf_add_scalar_prior(swf_problem* p, double* scalar, double w);
/* MarginalizationFactor(info) (R/swf/swf_core.cpp:551-552): kept blocks `keys` (sizes from the
 * problem), J dim x dim row-major, r0[dim], x0 = concatenated linearisation points. */
swf_factor_id swf_add_linear_prior(swf_problem* p, double* const* keys, int32_t n_keys,
                                   const double* J, const double* r0, const double* x0);
/* Fix and hold by key (the second half of LambdaSearch, R/swf/swf_lambda.cpp:254-343, for one window): prior_id = a swf_add_linear_prior
 * factor; double difference i fixes *amb[i] - *ref[i] to N21[i] (the caller passes ROUND(F), as the reference does): one row (amb[i],
 * group = ref[i], N21[i]) each and one row (ref, its group, 0) per distinct reference, through swf_prior_fix_batch with one problem.  The
 * prior's residual is taken at the blocks' CURRENT values (read through the keys); scalars_at_zero != 0: one-dimensional kept blocks at 0
 * (PhaseBiasSaveAndReset).  amb / ref must be one-dimensional blocks the prior keeps (SWF_E_INVALID); the operator's own rejections
 * apply.  J [dim][dim], r0 [dim], x0 (global sizes, kept-block order): solver-owned, valid until the next swf_problem_fix_prior or
 * destroy; any out pointer may be NULL.  The caller then does what the reference does at :344-354: swf_remove_factor(prior_id) and
 * swf_add_linear_prior with the prior's own keys. */
int swf_problem_fix_prior(swf_problem* p, swf_factor_id prior_id, double* const* amb, double* const* ref, const double* N21, int32_t n,
                          int32_t scalars_at_zero, double istd, double eps, int32_t form, const double** J, const double** r0,
                          const double** x0, int32_t* dim, int32_t* rank);
int swf_remove_factor(swf_problem* p, swf_factor_id id);                  /* RemoveResidualBlock */
int swf_factor_set_enabled(swf_problem* p, swf_factor_id id, int32_t on); /* ResidualBlock::is_use */
int swf_factor_is_enabled(swf_problem* p, swf_factor_id id);              /* 1 / 0; SWF_E_NOTFOUND */

/* The query surface of ceres::Problem the estimator walks when it marginalises through the solver (GlobalMarge,
 * R/swf/swf_image.cpp:350-367), re-attaches landmark blocks (R/swf/swf.cpp:413-422, R/feature/feature_manager.cpp:456-461)
 * and finds the dummy anchor's block (R/swf/swf_gnss.cpp:651).  Each getter writes the total count to *n and fills at most
 * `cap` entries (call with cap = 0 to size the buffer).  Residual blocks are reported in creation order, parameter blocks in
 * insertion order, the blocks of a residual block in the order of its AddResidualBlock call.
 *   Problem::GetResidualBlocks / GetResidualBlocksForParameterBlock / GetParameterBlocks / GetParameterBlocksForResidualBlock */
int swf_get_residual_blocks(swf_problem* p, swf_factor_id* ids, int32_t cap, int32_t* n);
int swf_get_residual_blocks_for_parameter_block(swf_problem* p, const double* key, swf_factor_id* ids, int32_t cap, int32_t* n);
int swf_get_parameter_blocks(swf_problem* p, double** keys, int32_t cap, int32_t* n);
int swf_get_parameter_blocks_for_residual_block(swf_problem* p, swf_factor_id id, double** keys, int32_t cap, int32_t* n);

/* window constants the factors read from globals in the reference (Pbg, Rwgw*G, base_xyz) */
int swf_set_constants(swf_problem* p, const double pbg[3], const double gw[3], const double base[3]);

/* options.linear_solver_ordering: ParameterBlockOrdering::AddElementToGroup() per entry
 * (R/swf/swf_gnss.cpp:629-783).  Replaces any previous ordering; setting the ordering it already has is free (no structure
 * change).  n = 0 (= a null linear_solver_ordering, the default Solver::Options of R/swf/swf_gnss.cpp:200-216, 562-572) asks
 * for an automatic ordering: every landmark and a greedy independent set of scalars in group 0, one group per remaining
 * variable block in insertion order, the export tail last. */
int swf_set_ordering(swf_problem* p, double* const* keys, const int32_t* groups, int32_t n);
/* ceres::internal::parameter_head: blocks ordered last and exported (R/swf/swf_gnss.cpp:116) */
int swf_set_export_tail(swf_problem* p, double* const* keys, int32_t n);

/* ceres::Solve(options, &problem, &summary) */
int swf_problem_solve(swf_problem* p, const swf_options* opt, swf_summary* summary);
/* UpdateSchur + setmarginalizeinfo(Sqrt = true) on the problem's export tail (R/swf/swf_image.cpp:404-418: is_optimize =
 * false, Solve, UpdateSchur, setmarginalizeinfo): valid after swf_problem_solve with step_mode =
 * SWF_ASSEMBLE_ELIMINATE_ONLY.  See swf_batch_marginalize for the outputs; buffers are solver-owned (n x n row-major / n),
 * valid until the next solve, marginalize or destroy.  Any out pointer may be NULL. */
int swf_problem_marginalize(swf_problem* p, double eps, int32_t form, const double** J, const double** r0,
                            const double** A, const double** bv, int32_t* n, int32_t* rank);
/* lhs_out / rhs_out / lhs_out2 / hs_row of the last solve; buffers solver-owned, valid until the
 * next solve or destroy. */
/* UpdateSchurHessianOnly + the covariance LambdaSearch takes from it (see swf_batch_tail_covariance); pointers are owned by
 * the problem and valid until the next call / solve. */
int swf_problem_tail_covariance(swf_problem* p, const double** A, const double** Qy, int32_t* n);
int swf_get_reduced(swf_problem* p, const double** S, const double** rhs, const double** L, int32_t* hs_row);
/* The feature check (see swf_batch_check_features) on the problem's cached batch, valid after swf_problem_solve (SWF_E_STATE
 * otherwise): features are the size-3 blocks and the inverse depths of swf_add_projection_inverse_depth, addressed by key
 * (SWF_E_NOTFOUND for a key that is no feature of the last solve).  swf_problem_rejected_features writes up to cap keys of the
 * features with OUTLIER | NEG_DEPTH, in feature order, and their full count to *n.  Any out pointer may be NULL. */
int swf_problem_check_features(swf_problem* p, double max_mean_error);
int swf_problem_get_feature_check(swf_problem* p, const double* key, double* mean_err, double* depth, int32_t* n_obs, int32_t* flags);
int swf_problem_rejected_features(swf_problem* p, double** keys, int32_t cap, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* SWF_SOLVER_H */
