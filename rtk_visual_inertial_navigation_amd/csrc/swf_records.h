// swf_records.h — what the host's symbolic phase (swf_plan.cpp) and the device code share: the plain records of the batch's index
// tables and the limits both sides must agree on.  No HIP here: this header compiles with a plain C++ compiler.  swf_dev.h includes
// it, so every kernel header sees these names.
#pragma once
#include <stdint.h>
#include "../../include/swf_types.h"

// ---- per-window static record -----------------------------------------------------------
struct WinRec {
    int x_base, x_n;             // ambient state range
    int blk_base, n_blk;         // block table range
    int loc_base, n_loc, n_e, n_red;   // local vector: [eliminated dims | reduced dims]
    long long S_base;            // offset of this window's n_red x n_red reduced matrix S
    long long Lt_base;           // offset of the (n_red+1)^2 transposed Cholesky factor (+ rhs row)
    int proj0, proj1;            // projection observations (sorted by landmark, then frame)
    int lm0, lm1;                // landmark records
    int fr_base, nF;             // observing frames (pose blocks that carry observations)
    long long P_base;            // (6 nF)^2 landmark Schur product
    int gf0, gf1;                // generic (non-projection) factors
    int cl0, cl1;                // cliques
    int pair0, pair1;            // reduced block pairs
    int fsb0, fsb1;              // frame-sum blocks of this window
    int tail_dim;                // dimensions of the parameter_head tail (last rows of the reduced system): the block of L its consumers read
    int n_pose_blk;              // the window's first n_pose_blk blocks are its pose blocks (7 -> 6, PoseLocalParameterization)
    int lmb0, lmb1;              // landmark back-substitution blocks of this window (DevBatch::lmb_rec)
    int pch0, pch1;              // row chunks of this window's priors (DevBatch::pch_q / pch_r0)
    double proj_sqrt_info, proj_loss_a;
    double pbg[3], gw[3], base[3];
};

// ---- per-window mutable solver state (lives on the device for the whole solve) ----------
struct WinState {
    double radius, mu, x_cost, x_norm, alpha, dogleg_step_norm, step_norm, gmax;
    double jg_sq, initial_cost;
    double lm_dec;               // LevenbergMarquardtStrategy::decrease_factor_ (SWF_LEVENBERG_MARQUARDT only)
    double model_cost_change;    // of the step k_dogleg proposed (from vectors alone, see k_dogleg)
    int status, iter, need_lin, reuse, eval_cand, lin_fail, invalid_run, nsucc, nunsucc;
    int chol_fail;               // lin_fail came from the dense factorisation (S itself is valid): the marginalisation consumer can still work
};

// ---- generic factor (everything except projection) --------------------------------------
enum { GF_IMU = 1, GF_CP = 2, GF_PR = 3, GF_DOP = 4, GF_SP = 5, GF_PRIOR = 6, GF_SPR = 7, GF_SCP = 8, GF_FIX = 9, GF_IDP = 10,
       GF_PROJX = 11 };      // GF_PROJX: a world-point projection factor on the generic clique path (variable extrinsic, or a landmark outside group 0)
struct GFac {
    int type, win, nres, nslot;
    int slot0;                   // into slot arrays
    int roff;                    // into g_r
    int data;                    // index into the type's data array (record index)
    int clique;                  // owning clique
    int jld;                     // column stride of this factor's Jacobian blocks in g_J (= rows of the clique's dense column-major matrix)
    int pad;                     // GF_PROJX: the caller's projection-factor index (row order of the Jacobian export)
};

// flat record of a scalar or an IMU factor for the J v products (jt_row_dot, swf_kernels.h): what sc_gf / imu_gf -> gf -> the slot arrays
// hold about the factor, in one 96-byte load.  JT_MAXSLOT: the most parameter blocks a typed adder gives such a factor (an
// inverse-depth projection between two cameras: two poses, two extrinsics, the inverse depth; an IMU factor has four).
#define JT_MAXSLOT 5
struct alignas(16) JtRec {
    int win, nres, jld, nslot;
    int roff, f, pad0, pad1;      // f: the factor's index in gf (g_aux)
    int joff[JT_MAXSLOT];         // g_J offset of the slot's block, -1 where the slot has none (constant block, static clique)
    int loc[JT_MAXSLOT];          // first local coordinate of the slot's block
    int ls[JT_MAXSLOT];           // local size of the slot's block
    int pad2;
};
static_assert(sizeof(JtRec) == 96, "JtRec: six 16-byte loads");

// flat record of an IMU factor for its evaluation (d_eval_imu, swf_kernels.h), one per entry of imu_gf: what imu_gf -> gf -> s_x /
// s_joff hold about the factor, in four 16-byte loads.  Slots: pose i, speed-bias i, pose j, speed-bias j.
struct alignas(16) ImuRec {
    int win, f, roff, data;       // window; index in gf (g_cost); first residual row in g_r; record in imu_pre
    int jld, pad0, pad1, pad2;    // column stride of the factor's Jacobian blocks in g_J
    int xo[4];                    // state offset of each slot's block (7, 9, 7, 9 doubles)
    int joff[4];                  // g_J offset of each slot's block (6, 9, 6, 9 columns of 15 rows), -1 where the slot has none
};
static_assert(sizeof(ImuRec) == 64, "ImuRec: four 16-byte loads");

// ---- clique: a group-0 block (or none) + the factors touching it + its reduced neighbours
struct Clique {
    int win;
    int e_loc, d_e;              // local offset / size of the eliminated block (d_e = 0: none)
    int d_f;                     // sum of member local sizes
    int fac0, fac1;              // into clique factor list (generic factor ids)
    int mem0, mem1;              // into member arrays (loc offset, size, column)
    long long C_off;             // d_f x d_f Schur'd block (static for priors)
    int v_off;                   // d_f vectors: graw, dgraw, cs
    int e_off;                   // d_e*d_e Einv + d_e*d_f strip + d_e g_e   (offset into e-buffer)
    int is_static;               // 1: prior clique, C/dgraw precomputed; only graw changes
    int n_rows;                  // total residual rows of the clique's factors
    int j_off, r_off;            // the clique's dense column-major Jacobian [d_e + d_f][n_rows] in g_J, and its residual rows in g_r
    int pad0, pad1;
};

// ---- reduced block pair (a >= b in elimination order): one wave assembles S[a,b] --------
struct Pair {
    int win;
    int ra, rb, la, lb;          // reduced offsets and sizes
    int fa, fb;                  // frame slots (>= 0 if pose carries observations) else -1
    int c0, c1;                  // contribution list range
    int is_diag;
    int loc_a;                   // local offset of block a (for g/diag/rhs of diagonal pairs)
    int fsb0, fsb1;              // the window's frame-sum blocks (diagonal pairs of observing poses)
    int n, m;                    // the window's n_red and 6 * nF, and its S / P slabs: the record is self-contained,
    long long S_base, P_base;    // no load of the pair's data depends on a second record
    long long q_base;            // the window's landmark rhs partials in DevBatch::lmq (GEMM_SPLIT vectors of m doubles)
};

// ---- assembly program of a window (k_assemble_flat): one thread per entry of the reduced system that receives anything, one
// per reduced dimension for the vectors.  The tables hold window-RELATIVE offsets, so windows of identical structure (a batch
// of one configuration) share one copy, which then lives in L2.
struct AsmWin {
    int se0, ne;                 // S-entry range in the shared tables
    int ve0, nv;                 // vector-entry range
    int n_red, m;                // reduced dimension; 6 nF
    int loc_base;                // first local dimension of the window's REDUCED part (g / diag / vc / rhs / jsc)
    int fs_base;                 // first frame-sum row of the window (fs_part rows of 27 doubles)
    int v_base;                  // first clique-vector slot of the window (cv_graw / cv_dgraw / cv_cs)
    int win;
    long long C_base, S_base, P_base, q_base;
};
#define AS_NC(c) ((c) & 4095u)
#define AS_NP(c) (((c) >> 12) & 31u)
#define AS_NH(c) (((c) >> 17) & 4095u)
#define AS_DIAG(c) (((c) >> 29) & 1u)
#define AS_SOLD(c) (((c) >> 30) & 1u)

struct DevBatch {
    int n_win;
    int n_x, n_loc_total;
    int max_iter_trace;
    // state
    double* x; double* xc; double* x0;
    // local-space vectors
    double* g; double* diag; double* rhs; double* y; double* step;
    double* vc;                                // D^-2 g = g / clamp(diag): written next to g / diag by their producers (Cauchy direction)
    // reduced matrices
    double* S; double* L;
    double* Wk;                                // working copy of the trailing matrix for k_chol_col (latency path, max n_red > 240), laid out like L
    double* Linv;                              // inverse diagonal tiles of k_chol_big: [window][32][16][16] (allocated when max n_red > 240)
    // tables
    const WinRec* win; WinState* ws; swf_iteration* trace;
    const int* blk_xoff; const int* blk_loc; const int* blk_gs;
    const int* loc2x;                          // per local dimension: its ambient coordinate (absolute), -1 for the dimensions of a pose block
    const unsigned char* x_var;                // per ambient coordinate: 1 if its block is variable
    // projection observations (SoA outputs, stride n_proj)
    int n_proj;
    const int* p_win; const int* p_xpose; const int* p_xex; const int* p_xlm;
    const int* p_lpose; const int* p_llm; const int* p_fr; const int* p_lm;
    const double* p_uv;
    double* p_r; double* p_Jp; double* p_Jl;
    // block partial sums (round 6): the cost of a frame-sum block's observations (written by every projection evaluation, one value per
    // block) and |J D^-2 g|^2 of a landmark back-substitution block's observations (k_post_chol).  The per-window control kernels add
    // a dozen block values in block order instead of reading 16 B per observation; per-observation costs are not stored any more.
    double* p_cpart; double* p_apart;
    // two-level per-frame sums: blocks of <= 256 observations of one window
    int n_fsb; const int* fsb_rec; const int* fsb_perm; const int* fsb_foff;   // fsb_rec: 8 ints per block (ProjBlk, swf_kernels.h)
    double* fs_part;
    double* jsc;                 // [n_loc_total] Jacobi scaling of the solve's first linearisation, (1 + sqrt(diag))^2 (Solver::Options::jacobi_scaling)
    // landmarks
    int n_lm;
    const int* lm_win; const int* lm_obs0; const int* lm_loc; const int* lm_col;
    double* lm_Einv; double* lm_g;             // SoA stride n_lm: 6 / 3
    double* P;                                 // landmark Schur product, GEMM_SPLIT partials per window
    double* lmq;                               // landmark part of the reduced rhs, sum_l Y_l g_l per pose row: GEMM_SPLIT partial vectors of 6 nF per window (at 6 fr_base GEMM_SPLIT)
    const int* lmb_rec; int n_lmb;             // landmark back-substitution blocks: {first observation, observations (<= 256), first landmark, landmarks}, whole landmarks of one window
    const int* sch_c0; const int* sch_rec;     // k_lm_schur chunk table: chunks of block (window, split); 8-int record per (chunk, group)
    const int* sch_km;                         // k_lm_schur tile masks: word (chunk, launch, consumer wave) = 3 TW bits per tile slot of the wave, bit 3 g + j = k-step j of wave task g is needed
    const unsigned long long* lm_fmask;        // frames (slots < 64) each landmark is observed in
    // frames
    int n_fr;
    const int* fr_obs0; const int* fr_obs;     // CSR of observations per frame
    const int* fr_red;                         // per frame slot: offset of its pose block in the reduced system
    // generic factors
    int n_gf;
    const GFac* gf;
    const int* s_x; const int* s_loc; const int* s_ls; const int* s_joff; const int* s_ccol;   // per slot: Jacobian block offset in g_J (column stride: GFac.jld)
    double* g_r; double* g_J; double* g_cost; double* g_aux;
    const double* imu_pre; const double* cp_dat; const double* pr_dat; const double* dop_dat; const double* sp_w;
    const double* gx_dat;            // records of the rover-only / fixed-integer scalar factors (GFac.data = offset in doubles)
    int n_imu; const int* imu_gf;              // generic-factor ids by kernel
    int n_idp; const int* idp_gf;              // two-row projection factors of the generic path: inverse-depth (GF_IDP) and world-point (GF_PROJX) ones (also members of sc_gf for the J v products)
    int n_sc;  const int* sc_gf;
    const JtRec* sc_jt; const JtRec* imu_jt;    // flat J v records, one per entry of sc_gf / imu_gf
    const ImuRec* imu_rec;                     // flat evaluation records, one per entry of imu_gf
    int n_prior; const int* prior_gf;
    // priors.  A prior of more than PRIOR_SPLIT_DIM rows is evaluated by one workgroup per chunk of PRIOR_CHUNK rows (its n x n record is
    // n^2 doubles through ONE compute unit otherwise: 553 KB, 19 us per pass, for the 263-dimension marginalisation prior of BASELINE
    // config 5); smaller ones are one chunk.  pch_q / pch_r0: prior and first row of every chunk; pr_cpart / pr_apart: the chunk's cost and
    // its share of |J D^-2 g|^2, which the per-window control kernels add in chunk order (a prior's generic cost slot stays zero).
    int n_pch; const int* pch_q; const int* pch_r0; const int* prior_nch;
    double* pr_cpart; double* pr_apart;
    const int* prior_dim; const long long* prior_Joff; const int* prior_roff; const int* prior_x0off;
    const double* prior_J; const double* prior_r0; const double* prior_x0;
    const double* prior_Jt;          // the same records transposed (element (k, c) at c * n + k): the J v products read these, lanes over rows
    const int* prior_colloc;         // per prior column (at prior_roff + c): reduced-local index of the column's variable, -1 if constant
    const int* prior_colcc;          // likewise: the column's position in the prior clique's vectors, -1 if constant
    const int* s_pcol; const int* s_pxo;   // prior slots only: first column of the block / its offset in the record's x0
    // cliques
    int n_cl;
    const Clique* cl;
    const int* cl_fac; const int* cl_frow;     // factor ids and their first row in the clique Jacobian
    const int* cm_loc; const int* cm_ls; const int* cm_col;
    double* C; double* cv_graw; double* cv_dgraw; double* cv_cs; double* cE;
    const int* cv_loc;                         // per clique vector slot (v_off + c): local index of the variable behind column c of the clique's reduced part
    int n_clc[5]; const Clique* clc_rec[5];    // non-static cliques by size class (copies of the records: no index indirection); 3 = k_clique_big, 4 = k_clique_tall
    int n_cle; const Clique* cle_rec;          // cliques with an eliminated block (back-substitution), likewise
    // pairs
    int n_pair;
    const long long* pc_coff; const int* pc_cld; const int* pc_voff;
    int n_pd, n_po; const Pair* pair_d; const Pair* pair_o;   // diagonal / off-diagonal pair records (the latter sorted by size)
    // assembly programs (k_assemble_flat)
    const AsmWin* asw; int as_max_ne, as_max_nv;
    const int* as_dst; const unsigned* as_cnt; const int* as_src0; const int* as_aux; const int* as_src;
    const int* av_loc; const int* av_red; const unsigned* av_cnt; const int* av_src0; const int* av_i; const int* av_src;
    const unsigned* s_tnz;                     // per window, 4 words: bit I (I - 1) / 2 + J = some block pair reaches tile (I, J), I > J, of the reduced matrix (k_chol_rr4 loads only those; n_red <= 256)
    int spec;                    // this launch evaluates Jacobians at the CANDIDATE of the windows with a proposed step (swf_kernels.h: eval_gate / eval_src); 0 in the batch the engine keeps
    int rr_nmax;                 // reduced systems up to this size take the register-resident Cholesky (256: k_chol_rr4); the streamed kernels take the rest
};

// ------------------------------------------------------------------ limits the symbolic phase builds its tables to
// (only those the plan reads; a kernel's other constants stay with the kernel)
// k_lm_schur (swf_lmschur.h)
#define GEMM_SPLIT 16                         // fixed landmark split: partial products P_0..P_15, summed in order (by k_lm_schur
                                              // itself when one block covers them all, else by k_assemble)
#define LS_GRAD_QPB 4                         // landmark parts per workgroup of the gradient-only pass (GRAD in swf_lmschur.h) in batches
#define LS_NB 4                               // ring buffers = producer teams
#define LS_MAXF 64                            // observing frames per window (64-bit frame masks)
// a block of NCW consumer waves with TPW tile slots each has the registers for the folded product (k_lm_schur: CAN_FOLD); the size
// classes 0 and 1 (<8, 2, ..> and <8, 5, ..>) are those blocks, and the plan's ls_folded says so with the same predicate
constexpr bool ls_can_fold(int NCW, int TPW) { return TPW <= 5 && NCW == 8; }
// prior evaluation (swf_kernels.h)
#define PRIOR_SPLIT_DIM 96              // priors beyond this dimension are evaluated in row chunks, a workgroup each
#define PRIOR_CHUNK 32
// clique elimination (swf_kernels.h): the one-wavefront kernels, the tall class (k_clique_tall), the workgroup kernel (k_clique_big)
#define CLQ_MAXD 64
#define CLQ_MAXR 64
#define CLQ_TALLR 96
#define CB_MAXD 768                           // columns of a big clique (d_e + d_f)
#define CB_MAXED 1536                         // d_e x (d_e + d_f) of a big clique: the rows of M that belong to e, and T = Einv M_ef, live in LDS
// frame sums (swf_kernels.h): observations per block, doubles per (block, frame) = lower(Jp^T Jp)(21) | Jp^T r (6)
#define FS_BLK 256
#define FS_VAL 27
// dense factorisation (swf_kernels2.h)
#define CB_NMAX 640                     // largest reduced system of the tiled kernels (hs_row reaches ~620 in a live window)
#define CC_NMAX 512                     // k_chol_col keeps two panels in LDS: up to 512 dimensions
// threads of the per-window control kernels k_dogleg / k_decide (swf_kernels2.h): a thread per pose block bounds a window's pose blocks
#define CTL_NT 256
// composite IMU-GNSS factors (swf_kernels4.h)
#define CO_MAXN 64                         // ambiguities per composite factor (the reference's data model: 3 constellations x NFREQ 2 on up to MAXOBS 64
                                           // satellites, R/gnss/include/common_function.h:24-37; 30..48 per gap is a normal open-sky epoch)
