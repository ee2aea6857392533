// swf_plan.h — the symbolic phase of the batch engine as a host-only plan: flat windows -> every index table, count, buffer size
// and launch-shape decision a batch is created from (swf_batch_create uploads a Plan; it computes none of this itself).
// No HIP here or in swf_plan.cpp: the densest index arithmetic of the project builds and runs where there is no GPU.
#pragma once
#include <string>
#include <vector>
#include "../../include/swf_solver.h"
#include "swf_records.h"

// what the symbolic phase keeps of one window's visual factors (copied at swf_batch_create: the caller's arrays are read during that
// call only); the post-solve feature check (swf_features.h) builds its table from them
struct FeatWinSrc {
    int x_base = 0, n_pose = 0, n_sb = 0, n_lm = 0, n_sc = 0;
    std::vector<int> proj_idx; std::vector<double> proj_uv;                             // [n_proj][3], [n_proj][2]
    std::vector<int> idp_kind, idp_idx; std::vector<double> idp_pts;                    // [n_idp], [n_idp][5], [n_idp][6]
    double pbg[3] = { 0, 0, 0 }; double sqrt_info = 0;
};

struct HostWin {       // what the host keeps per window for state transfer / export
    double *pose, *sb, *lm, *sc;
    int n_pose, n_sb, n_lm, n_sc;
    int tail_dim;
    double *comp_pose = nullptr, *comp_sb = nullptr;    // hidden epochs of the window's composite factors (caller memory)
    int comp_e0 = 0, comp_ne = 0;                       // their range in the batch-wide hidden-epoch arrays
    std::vector<int> p_orig;                            // device observation (proj0 + q) -> the caller's projection factor index
    int n_proj_all = 0;                                 // the caller's projection factors, fast path + generic path (GF_PROJX)
    std::vector<int> tail_x;                            // per tail coordinate: its state index if its block has size 1, else -1
    FeatWinSrc feat;                                    // the window's visual factors as the caller gave them (swf_batch_check_features builds its table from them)
    // the window's linear priors (not the records of composite factors), in the caller's order, for swf_batch_fix_prior
    struct LinPrior { int gf, dim, gsum; std::vector<int> col_x; };      // col_x: per prior column, the state index of its block if the block has size 1, else -1
    std::vector<LinPrior> lin_prior;
};

// what the plan depends on besides the windows: the chip's compute units and the launch-shape knobs (test aids, each exercised by
// the GPU tier; 0 / false = not forced)
struct PlanShape {
    int n_cu = 256;
    bool no_lat_fuse = false;         // SWF_NO_LAT_FUSE
    int ls_variant = 0;               // SWF_LS_VARIANT: the smallest k_lm_schur size class allowed
    int ls_qpb = 0;                   // SWF_LS_QPB: landmark parts per workgroup of k_lm_schur (a power of two <= GEMM_SPLIT)
    int ls_grad_qpb = 0;              // SWF_LS_GRAD_QPB: the same for the gradient-only pass
    bool no_chol_col = false;         // SWF_NO_CHOL_COL
};
PlanShape plan_shape_from_env(int n_cu);

struct Plan {
    // concatenated host arrays
    std::vector<WinRec> win;
    std::vector<HostWin> hw;
    std::vector<int> blk_xoff, blk_loc, blk_gs, loc2x;
    std::vector<unsigned char> x_var;
    std::vector<int> p_win, p_xpose, p_xex, p_xlm, p_lpose, p_llm, p_fr, p_lm;
    std::vector<double> p_uv;
    std::vector<int> lm_win, lm_obs0, lm_loc, lm_col;
    std::vector<unsigned long long> lm_fmask;
    std::vector<int> fsb_win, fsb_obs0, fsb_perm, fsb_foff, fsb_foff0, fsb_out0;
    long long fs_tot = 0;
    std::vector<int> fr_obs0, fr_obs, fr_red;
    std::vector<GFac> gf;
    std::vector<int> s_x, s_loc, s_ls, s_joff, s_ccol;
    std::vector<double> imu_pre, cp_dat, pr_dat, dop_dat, sp_w, gx_dat;
    std::vector<int> imu_gf, sc_gf, prior_gf, idp_gf;
    std::vector<int> prior_dim, prior_roff, prior_x0off;
    std::vector<long long> prior_Joff;
    std::vector<double> prior_J, prior_r0, prior_x0;
    std::vector<Clique> cl;
    std::vector<int> cl_fac, cl_frow, cm_loc, cm_ls, cm_col;
    std::vector<double> C_init, dgraw_init;      // static parts (prior cliques)
    // composite factors (concatenated over the batch)
    std::vector<int> co_M, co_N, co_gf, co_win, co_xo, co_xo_off{ 0 };
    std::vector<double> co_pose, co_sb, co_pose_lin, co_sb_lin, co_Hpp, co_HpN, co_rhs_p, co_HNN, co_rhsN, co_pre, co_pbgw, co_H12;
    std::vector<int> co_mid;
    std::vector<Pair> pair;
    std::vector<long long> pc_coff;
    std::vector<int> pc_cld, pc_voff;
    // sizes of the mutable buffers
    long long n_x = 0, n_loc = 0, S_tot = 0, Lt_tot = 0, P_tot = 0, C_tot = 0;
    int v_tot = 0, e_tot = 0, r_tot = 0, j_tot = 0, n_fr = 0;
    int max_tiles = 0, max_prior_dim = 0;
    // tables derived from the arrays above, under their DevBatch names
    std::vector<int> lmb_rec, pch_q, pch_r0, prior_nch;
    std::vector<int> sch_c0, sch_rec, sch_km;
    std::vector<int> fsb_rec;
    std::vector<JtRec> sc_jt, imu_jt;
    std::vector<ImuRec> imu_rec;
    std::vector<double> prior_Jt;
    std::vector<int> prior_colloc, prior_colcc, s_pcol, s_pxo, cv_loc;
    std::vector<Pair> pair_d, pair_o;
    std::vector<Clique> clc_rec[5], cle_rec;
    std::vector<AsmWin> asw;
    std::vector<unsigned> s_tnz;
    std::vector<int> as_dst, as_src0, as_aux, as_src, av_loc, av_red, av_src0, av_i, av_src;
    std::vector<unsigned> as_cnt, av_cnt;
    // composite factors: offsets into the operator's arrays (per factor, + 1 for the running ones), where each factor's prior record
    // and clique live, the (factor, link) list of its IMU links
    std::vector<int> co_eo, co_no, co_roff, co_x0off, co_voff, co_iq_f, co_iq_k;
    std::vector<long long> co_pno, co_nno, co_go, co_g2o, co_Joff, co_Coff;
    // counts (DevBatch::n_*): the entries in use, before the tables are padded to a non-empty upload
    int n_win = 0, n_proj = 0, n_lm = 0, n_lmb = 0, n_pch = 0, n_fsb = 0, n_pd = 0, n_po = 0, n_cle = 0, n_clc[5] = { 0, 0, 0, 0, 0 };
    int as_max_ne = 0, as_max_nv = 0;
    // launch shape, fixed at creation (swf_batch holds the same names)
    int n_cu = 256, rr_nmax = 256, max_red = 0, min_red = 1 << 30;
    int ls_qpb = 1, ls_var = 0, ls_kms = 8, ls_gqpb = 4; bool ls_folded = false, s_direct = false;
    bool lat_fuse = false, want_aux = false, want_Linv = false, want_Wk = false;
    bool clc_imu[5] = { false, false, false, false, false };
    int clp_rows = 1, clp_ld = 3;      // class 0 (k_clique_pack): the largest n_rows, and (largest d + 2) | 1, of the batch's class-0 cliques — the kernel's LDS is sized by them
    int n_pch_split = 0; bool rr4_has15 = false, rr4_has16 = false;
    int n_comp = 0, comp_nmax = 0, comp_nmin = 1 << 30; long long comp_ne = 0;
    int asm_programs = 0;
    // flop and byte counters
    int64_t jac_bytes = 0, proj_bytes = 0, chol_flops = 0, lm_schur_flops = 0, lm_schur_flops_sym = 0, lm_schur_mfma = 0;
};

// Builds the plan of a batch.  A window the engine cannot take is refused with the code and the message swf_batch_create reports
// (SWF_E_INVALID / SWF_E_UNSUPPORTED, err); nothing of the device is touched.
int plan_build(const swf_flat_window* const* windows, int n, const PlanShape& shape, Plan& plan, std::string& err);

// Recomputes from the plan's primary data what every kernel trusts without checking — index ranges, partitions, the k_lm_schur task
// table and its tile masks, the assembly programs, the s_tnz bits, the clique classes — and names the first table that disagrees.
// Not on the creation path (a rebuild is latency-sensitive): reached through swf_debug_plan_check.
int plan_validate(const Plan& plan, std::string& err);
