// swf_plan.cpp — the symbolic phase: flat windows -> the index arrays every kernel trusts (Plan, swf_plan.h), once per structure.
// Host-only: a plain C++17 translation unit, no HIP.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "swf_plan.h"

namespace {
int refuse(std::string& err, int code, const std::string& msg) { err = msg; return code; }
// k_lm_schur's size classes 0..3 = <NCW, TPW, TW, LDR> <8, 2, 2, 80>, <8, 5, 2, 144>, <12, 6, 1, 272>, <12, 6, 1, 400> (swf_lmschur.h)
int ls_ncw(int var) { return var <= 1 ? 8 : 12; }
int ls_tpw(int var) { return var == 0 ? 2 : var == 1 ? 5 : 6; }

// one window: block layout and ordering, observations in k_lm_schur's landmark order, frame-sum blocks, generic factors, cliques, block pairs
int plan_window(Plan& B, const swf_flat_window* w, int wi, HostWin& hw, std::string& err) {
    WinRec R{};
    const int nP = w->n_pose, nS = w->n_sb, nL = w->n_lm, nC = w->n_sc;
    const int nb = nP + nS + nL + nC;
    if (nb <= 0) return refuse(err, SWF_E_INVALID, "empty window");
    hw = HostWin{ w->pose, w->sb, w->lm, w->sc, nP, nS, nL, nC, 0 };
    R.x_base = (int)B.n_x; R.blk_base = (int)B.blk_xoff.size(); R.n_blk = nb;
    R.loc_base = (int)B.n_loc;
    std::vector<int> gs(nb), ls(nb), xo(nb), loc(nb, -1), grp(nb, -1);
    int xoff = 0;
    for (int b = 0; b < nb; b++) {
        int g = b < nP ? 7 : b < nP + nS ? 9 : b < nP + nS + nL ? 3 : 1;
        gs[b] = g; ls[b] = g == 7 ? 6 : g; xo[b] = xoff; xoff += g;
    }
    R.x_n = xoff;
    int lo = 0, ne = 0, prevg = 0;
    for (int i = 0; i < w->n_order; i++) {
        int b = w->order_block[i], g = w->order_group[i];
        if (b < 0 || b >= nb) return refuse(err, SWF_E_INVALID, "ordering: block id out of range");
        if (w->is_const[b]) return refuse(err, SWF_E_INVALID, "ordering: constant block in ordering");
        if (loc[b] >= 0) return refuse(err, SWF_E_INVALID, "ordering: block listed twice");
        if (g < prevg) return refuse(err, SWF_E_INVALID, "ordering: groups must ascend");
        prevg = g;
        loc[b] = lo; grp[b] = g; lo += ls[b];
        if (g == 0) ne += ls[b];
    }
    for (int b = 0; b < nb; b++) if (!w->is_const[b] && loc[b] < 0) return refuse(err, SWF_E_INVALID, "ordering: variable block missing from ordering");
    R.n_loc = lo; R.n_e = ne; R.n_red = lo - ne;
    if (R.n_red + 1 > 1024) return refuse(err, SWF_E_UNSUPPORTED, "reduced system larger than 1023");
    R.S_base = B.S_tot; B.S_tot += (long long)(R.n_red + 1) * R.n_red;      // n x n (lower used) + the reduced rhs as row n
    R.Lt_base = B.Lt_tot; B.Lt_tot += (long long)(R.n_red + 1) * (R.n_red + 1);
    {
        int td = 0;
        hw.tail_x.clear();
        for (int i = w->n_order - w->n_tail; i < w->n_order; i++) if (i >= 0) {
            const int b = w->order_block[i];
            td += ls[b];
            for (int k = 0; k < ls[b]; k++) hw.tail_x.push_back(gs[b] == 1 ? R.x_base + xo[b] : -1);
        }
        hw.tail_dim = td; R.tail_dim = td;
    }
    if (nP > CTL_NT) return refuse(err, SWF_E_UNSUPPORTED, "more than 256 pose blocks in a window");      // k_dogleg: a thread per pose block
    R.n_pose_blk = nP;
    B.loc2x.resize((size_t)R.loc_base + (size_t)R.n_loc, -1); B.x_var.resize((size_t)R.x_base + (size_t)R.x_n, 0);
    for (int b = 0; b < nb; b++) {
        B.blk_xoff.push_back(R.x_base + xo[b]);
        B.blk_loc.push_back(loc[b] >= 0 ? R.loc_base + loc[b] : -1);
        B.blk_gs.push_back(gs[b]);
        if (loc[b] < 0) continue;
        for (int k = 0; k < gs[b]; k++) B.x_var[(size_t)R.x_base + xo[b] + k] = 1;
        if (gs[b] != 7) for (int k = 0; k < gs[b]; k++) B.loc2x[(size_t)R.loc_base + loc[b] + k] = R.x_base + xo[b] + k;
    }
    auto bidP = [&](int i) { return i; };
    auto bidS = [&](int i) { return nP + i; };
    auto bidL = [&](int i) { return nP + nS + i; };
    auto bidC = [&](int i) { return nP + nS + nL + i; };
    auto is_e = [&](int b) { return grp[b] == 0; };
    auto gloc = [&](int b) { return loc[b] >= 0 ? R.loc_base + loc[b] : -1; };
    auto gx = [&](int b) { return R.x_base + xo[b]; };

    // ---- which landmarks leave the fast path (k_lm_schur: world point in group 0, constant extrinsic, one factor per frame)
    // for the generic one (GF_PROJX factors in cliques): a variable extrinsic on any of its factors — the reference's
    // marginalisation solves un-freeze para_ex_Pose (R/swf/swf_image.cpp:384-389) — or a variable landmark outside group 0
    std::vector<char> lm_generic(nL, 0);
    for (int i = 0; i < w->n_proj; i++) {
        int p = w->proj_idx[i * 3], ex = w->proj_idx[i * 3 + 1], l = w->proj_idx[i * 3 + 2];
        if (p < 0 || p >= nP || ex < 0 || ex >= nP || l < 0 || l >= nL) return refuse(err, SWF_E_INVALID, "projection factor: index out of range");
        if (loc[bidP(ex)] >= 0 || (loc[bidL(l)] >= 0 && !is_e(bidL(l)))) lm_generic[l] = 1;
    }
    hw.n_proj_all = w->n_proj;
    {
        FeatWinSrc& fs = hw.feat;
        fs.x_base = R.x_base; fs.n_pose = nP; fs.n_sb = nS; fs.n_lm = nL; fs.n_sc = nC;
        if (w->n_proj > 0) { fs.proj_idx.assign(w->proj_idx, w->proj_idx + (size_t)3 * w->n_proj); fs.proj_uv.assign(w->proj_uv, w->proj_uv + (size_t)2 * w->n_proj); }
        if (w->n_idp > 0) {
            fs.idp_kind.assign(w->idp_kind, w->idp_kind + w->n_idp); fs.idp_idx.assign(w->idp_idx, w->idp_idx + (size_t)5 * w->n_idp);
            fs.idp_pts.assign(w->idp_pts, w->idp_pts + (size_t)6 * w->n_idp);
        }
        for (int k = 0; k < 3; k++) fs.pbg[k] = w->pbg[k];
        fs.sqrt_info = w->proj_sqrt_info;
    }
    // ---- projection observations of the fast path sorted by (landmark, pose)
    std::vector<int> ord;
    for (int i = 0; i < w->n_proj; i++) if (!lm_generic[w->proj_idx[i * 3 + 2]]) ord.push_back(i);
    const int n_fast = (int)ord.size();
    // (sorted below, once the landmark records have their order)
    // frames: variable, non-eliminated poses that carry observations, in pose order
    std::vector<int> frame_of(nP, -1);
    {
        std::vector<char> seen(nP, 0);
        for (int i : ord) seen[w->proj_idx[i * 3]] = 1;
        int nf = 0;
        for (int p = 0; p < nP; p++) if (seen[p] && loc[bidP(p)] >= 0) {
            if (is_e(bidP(p))) return refuse(err, SWF_E_UNSUPPORTED, "pose block in elimination group 0");
            frame_of[p] = nf++;
            B.fr_red.push_back(loc[bidP(p)] - ne);
        }
        R.nF = nf; R.fr_base = B.n_fr;
    }
    // Landmark records — and with them the observations — are laid out in the order k_lm_schur packs them into wave tasks: by the
    // footprint of the track in the 16-row tiles of the reduced camera matrix (last tile, first tile), ties in the caller's order.
    // A wave task's four landmarks then read four adjacent runs of every Jacobian array.  (Internal order only: the elimination
    // order is that of the blocks, and hw.p_orig maps the observations back to the caller's factors.)
    std::vector<int> lm_rank(nL), lm_perm(nL);
    {
        std::vector<unsigned> trs(nL, 0u);
        for (int i : ord) {
            int f = frame_of[w->proj_idx[i * 3]];
            if (f >= 0 && f < 64) { trs[w->proj_idx[i * 3 + 2]] |= 1u << ((6 * f) / 16); trs[w->proj_idx[i * 3 + 2]] |= 1u << ((6 * f + 5) / 16); }
        }
        auto key = [&](int l) { unsigned t = trs[l]; return t ? (31 - __builtin_clz(t)) * 64 + __builtin_ctz(t) : (lm_generic[l] ? 1 << 20 : 0); };
        for (int l = 0; l < nL; l++) lm_perm[l] = l;
        std::stable_sort(lm_perm.begin(), lm_perm.end(), [&](int a, int b) { return key(a) < key(b); });
        for (int r = 0; r < nL; r++) lm_rank[lm_perm[r]] = r;
    }
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
        int la = lm_rank[w->proj_idx[a * 3 + 2]], lb = lm_rank[w->proj_idx[b * 3 + 2]];
        if (la != lb) return la < lb;
        return w->proj_idx[a * 3] < w->proj_idx[b * 3];
    });
    R.proj0 = (int)B.p_win.size();
    R.lm0 = (int)B.lm_win.size();
    hw.p_orig = ord;
    {
        std::vector<std::vector<int>> fobs(R.nF);
        std::vector<int> lm_first(nL + 1, 0);
        for (int q = 0; q < n_fast; q++) {
            int i = ord[q];
            int p = w->proj_idx[i * 3], ex = w->proj_idx[i * 3 + 1], l = w->proj_idx[i * 3 + 2];
            if (q > 0 && w->proj_idx[ord[q - 1] * 3 + 2] == l && w->proj_idx[ord[q - 1] * 3] == p && frame_of[p] >= 0)
                return refuse(err, SWF_E_UNSUPPORTED, "two projection factors of one landmark in the same frame");
            int gi = (int)B.p_win.size();
            B.p_win.push_back(wi);
            B.p_xpose.push_back(gx(bidP(p))); B.p_xex.push_back(gx(bidP(ex))); B.p_xlm.push_back(gx(bidL(l)));
            B.p_lpose.push_back(gloc(bidP(p))); B.p_llm.push_back(gloc(bidL(l)));
            B.p_fr.push_back(frame_of[p]); B.p_lm.push_back(R.lm0 + lm_rank[l]);
            B.p_uv.push_back(w->proj_uv[i * 2]); B.p_uv.push_back(w->proj_uv[i * 2 + 1]);
            if (frame_of[p] >= 0) fobs[frame_of[p]].push_back(gi);
            lm_first[lm_rank[l] + 1]++;
        }
        for (int l = 0; l < nL; l++) lm_first[l + 1] += lm_first[l];
        for (int rk = 0; rk < nL; rk++) {
            const int l = lm_perm[rk];
            int b = bidL(l);
            B.lm_win.push_back(wi);
            B.lm_obs0.push_back(R.proj0 + lm_first[rk]);
            B.lm_loc.push_back(lm_generic[l] ? -1 : gloc(b));        // a generic-path landmark has no observations here: an inactive record
            B.lm_col.push_back(3 * l);
            B.lm_fmask.push_back(0ULL);
        }
        for (int q = R.proj0; q < (int)B.p_win.size(); q++) {
            int f = B.p_fr[q];
            if (f >= 0) B.lm_fmask[B.p_lm[q]] |= (f < 64) ? (1ULL << f) : ~0ULL;
        }
        if (R.nF > 64) for (int l = 0; l < nL; l++) B.lm_fmask[R.lm0 + l] = ~0ULL;   // no skipping beyond 64 frames
        for (int f = 0; f < R.nF; f++) {
            B.fr_obs0.push_back((int)B.fr_obs.size());
            for (int o : fobs[f]) B.fr_obs.push_back(o);
        }
        B.n_fr += R.nF;
    }
    R.proj1 = (int)B.p_win.size();
    R.lm1 = (int)B.lm_win.size();
    // frame-sum blocks: <= FS_BLK consecutive observations, frame-sorted permutation per block
    R.fsb0 = (int)B.fsb_win.size();
    for (int o0 = R.proj0; o0 < R.proj1; o0 += FS_BLK) {
        int cnt = std::min(FS_BLK, R.proj1 - o0);
        B.fsb_win.push_back(wi); B.fsb_obs0.push_back(o0);
        B.fsb_foff0.push_back((int)B.fsb_foff.size());
        B.fsb_out0.push_back((int)B.fs_tot); B.fs_tot += R.nF;
        std::vector<std::vector<int>> byf(R.nF);
        for (int t = 0; t < cnt; t++) { int f = B.p_fr[o0 + t]; if (f >= 0) byf[f].push_back(t); }
        // fsb_perm[o] = rank of observation o in the block's frame-sorted order (observations of constant poses go last)
        int pos = 0;
        B.fsb_perm.resize((size_t)o0 + cnt, -1);
        for (int f = 0; f < R.nF; f++) {
            B.fsb_foff.push_back(pos);
            for (int t : byf[f]) B.fsb_perm[(size_t)o0 + t] = pos++;
        }
        B.fsb_foff.push_back(pos);
        for (int t = 0; t < cnt; t++) if (B.fsb_perm[(size_t)o0 + t] < 0) B.fsb_perm[(size_t)o0 + t] = pos++;
    }
    R.fsb1 = (int)B.fsb_win.size();
    R.P_base = B.P_tot; B.P_tot += (long long)36 * R.nF * R.nF;       // x GEMM_SPLIT partial products at allocation
    {
        int m = 6 * R.nF, nt = (m + 15) / 16;
        B.max_tiles = std::max(B.max_tiles, nt * (nt + 1) / 2);
        if (R.nF > LS_MAXF) return refuse(err, SWF_E_UNSUPPORTED, "more than 64 observing frames in one window");
    }

    // ---- generic factors
    R.gf0 = (int)B.gf.size();
    struct TmpF { std::vector<int> blk; };
    std::vector<TmpF> tf;
    auto add_gf = [&](int type, int nres, int data, const std::vector<int>& blks) {
        GFac G{};
        G.type = type; G.win = wi; G.nres = nres; G.nslot = (int)blks.size();
        G.slot0 = (int)B.s_x.size(); G.roff = -1; G.data = data; G.clique = -1;
        for (int b : blks) {
            B.s_x.push_back(gx(b)); B.s_loc.push_back(gloc(b)); B.s_ls.push_back(ls[b]);
            // Jacobian block placement (s_joff, s_jld) and the residual offset are assigned with the cliques below
            B.s_joff.push_back((loc[b] >= 0 && type != GF_PRIOR) ? 0 : -1);
            B.s_ccol.push_back(-1);
        }
        B.gf.push_back(G);
        tf.push_back(TmpF{ blks });
        return (int)B.gf.size() - 1;
    };
#define CHK(i, n, what) if ((i) < 0 || (i) >= (n)) return refuse(err, SWF_E_INVALID, what ": index out of range");
    for (int i = 0; i < w->n_imu; i++) {
        const int* ix = w->imu_idx + i * 4;
        CHK(ix[0], nP, "imu") CHK(ix[1], nS, "imu") CHK(ix[2], nP, "imu") CHK(ix[3], nS, "imu")
        int data = (int)(B.imu_pre.size() / SWF_PRE_DOUBLES);
        B.imu_pre.insert(B.imu_pre.end(), w->imu_pre + (size_t)i * SWF_PRE_DOUBLES, w->imu_pre + (size_t)(i + 1) * SWF_PRE_DOUBLES);
        B.imu_gf.push_back(add_gf(GF_IMU, 15, data, { bidP(ix[0]), bidS(ix[1]), bidP(ix[2]), bidS(ix[3]) }));
    }
    for (int i = 0; i < w->n_cp; i++) {
        const int* ix = w->cp_idx + i * 3;
        CHK(ix[0], nP, "carrier phase") CHK(ix[1], nC, "carrier phase") CHK(ix[2], nC, "carrier phase")
        int data = (int)(B.cp_dat.size() / SWF_CP_DOUBLES);
        B.cp_dat.insert(B.cp_dat.end(), w->cp_dat + i * SWF_CP_DOUBLES, w->cp_dat + (i + 1) * SWF_CP_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_CP, 1, data, { bidP(ix[0]), bidC(ix[1]), bidC(ix[2]) }));
    }
    for (int i = 0; i < w->n_pr; i++) {
        const int* ix = w->pr_idx + i * 2;
        CHK(ix[0], nP, "pseudorange") CHK(ix[1], nC, "pseudorange")
        int data = (int)(B.pr_dat.size() / SWF_PR_DOUBLES);
        B.pr_dat.insert(B.pr_dat.end(), w->pr_dat + i * SWF_PR_DOUBLES, w->pr_dat + (i + 1) * SWF_PR_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_PR, 1, data, { bidP(ix[0]), bidC(ix[1]) }));
    }
    for (int i = 0; i < w->n_dop; i++) {
        const int* ix = w->dop_idx + i * 3;
        CHK(ix[0], nS, "doppler") CHK(ix[1], nC, "doppler") CHK(ix[2], nP, "doppler")
        int data = (int)(B.dop_dat.size() / SWF_DOP_DOUBLES);
        B.dop_dat.insert(B.dop_dat.end(), w->dop_dat + i * SWF_DOP_DOUBLES, w->dop_dat + (i + 1) * SWF_DOP_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_DOP, 1, data, { bidS(ix[0]), bidC(ix[1]), bidP(ix[2]) }));
    }
    for (int i = 0; i < w->n_sp; i++) {
        CHK(w->sp_idx[i], nC, "scalar prior")
        int data = (int)B.sp_w.size();
        B.sp_w.push_back(w->sp_w[i]);
        B.sc_gf.push_back(add_gf(GF_SP, 1, data, { bidC(w->sp_idx[i]) }));
    }
    // rover-only pseudorange / carrier phase and fixed-integer factors share one record pool (GFac.data = offset in doubles)
    for (int i = 0; i < w->n_spr; i++) {
        const int* ix = w->spr_idx + i * 2;
        CHK(ix[0], nP, "spp pseudorange") CHK(ix[1], nC, "spp pseudorange")
        int data = (int)B.gx_dat.size();
        B.gx_dat.insert(B.gx_dat.end(), w->spr_dat + i * SWF_SPR_DOUBLES, w->spr_dat + (i + 1) * SWF_SPR_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_SPR, 1, data, { bidP(ix[0]), bidC(ix[1]) }));
    }
    for (int i = 0; i < w->n_scp; i++) {
        const int* ix = w->scp_idx + i * 3;
        CHK(ix[0], nP, "spp carrier phase") CHK(ix[1], nC, "spp carrier phase") CHK(ix[2], nC, "spp carrier phase")
        int data = (int)B.gx_dat.size();
        B.gx_dat.insert(B.gx_dat.end(), w->scp_dat + i * SWF_SCP_DOUBLES, w->scp_dat + (i + 1) * SWF_SCP_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_SCP, 1, data, { bidP(ix[0]), bidC(ix[1]), bidC(ix[2]) }));
    }
    for (int i = 0; i < w->n_fix; i++) {
        const int* ix = w->fix_idx + i * 2;
        CHK(ix[0], nC, "fixed integer") CHK(ix[1], nC, "fixed integer")
        if (ix[0] == ix[1]) return refuse(err, SWF_E_INVALID, "fixed integer: both blocks are the same scalar");
        int data = (int)B.gx_dat.size();
        B.gx_dat.insert(B.gx_dat.end(), w->fix_dat + i * SWF_FIX_DOUBLES, w->fix_dat + (i + 1) * SWF_FIX_DOUBLES);
        B.sc_gf.push_back(add_gf(GF_FIX, 1, data, { bidC(ix[0]), bidC(ix[1]) }));
    }
    // inverse-depth projection factors: two residual rows, evaluated one lane each with the scalar factors; record = kind | pts (6)
    for (int i = 0; i < w->n_idp; i++) {
        const int* ix = w->idp_idx + i * 5; const int kd = w->idp_kind[i];
        if (kd < 0 || kd > 2) return refuse(err, SWF_E_INVALID, "inverse-depth projection: kind must be 0, 1 or 2");
        std::vector<int> blks;
        if (kd != 2) { CHK(ix[0], nP, "inverse-depth projection") CHK(ix[1], nP, "inverse-depth projection") blks.push_back(bidP(ix[0])); blks.push_back(bidP(ix[1])); }
        CHK(ix[2], nP, "inverse-depth projection") blks.push_back(bidP(ix[2]));
        if (kd != 0) { CHK(ix[3], nP, "inverse-depth projection") blks.push_back(bidP(ix[3])); }
        CHK(ix[4], nC, "inverse-depth projection") blks.push_back(bidC(ix[4]));
        for (size_t a = 0; a < blks.size(); a++) for (size_t c2 = 0; c2 < a; c2++)
            if (blks[a] == blks[c2]) return refuse(err, SWF_E_INVALID, "inverse-depth projection: repeated parameter block");
        int data = (int)B.gx_dat.size();
        B.gx_dat.push_back((double)kd);
        B.gx_dat.insert(B.gx_dat.end(), w->idp_pts + (size_t)i * 6, w->idp_pts + (size_t)(i + 1) * 6);
        { int g = add_gf(GF_IDP, 2, data, blks); B.sc_gf.push_back(g); B.idp_gf.push_back(g); }
    }
    // world-point projection factors of the generic path (GF_PROJX): record = uv; GFac.pad = the caller's factor index
    for (int i = 0; i < w->n_proj; i++) {
        const int* ix = w->proj_idx + i * 3;
        if (!lm_generic[ix[2]]) continue;
        int data = (int)B.gx_dat.size();
        B.gx_dat.push_back(w->proj_uv[i * 2]); B.gx_dat.push_back(w->proj_uv[i * 2 + 1]);
        int g = add_gf(GF_PROJX, 2, data, { bidP(ix[0]), bidP(ix[1]), bidL(ix[2]) });
        B.gf[g].pad = i;
        B.sc_gf.push_back(g); B.idp_gf.push_back(g);
    }
    std::vector<int> prior_first_gf;
    {
        int bo = 0; long long jo = 0; int ro = 0, x0o = 0;
        for (int k = 0; k < w->n_prior; k++) {
            int nbk = w->prior_nblk[k], dim = w->prior_dim[k];
            std::vector<int> blks(w->prior_blk + bo, w->prior_blk + bo + nbk);
            int dsum = 0, gsum = 0;
            for (int b : blks) { CHK(b, nb, "prior") dsum += ls[b]; gsum += gs[b]; }
            if (dsum != dim) return refuse(err, SWF_E_INVALID, "prior: dim != sum of local block sizes");
            int data = (int)B.prior_dim.size();
            B.prior_dim.push_back(dim);
            B.prior_Joff.push_back((long long)B.prior_J.size());
            B.prior_roff.push_back((int)B.prior_r0.size());
            B.prior_x0off.push_back((int)B.prior_x0.size());
            B.prior_J.insert(B.prior_J.end(), w->prior_J + jo, w->prior_J + jo + (long long)dim * dim);
            B.prior_r0.insert(B.prior_r0.end(), w->prior_r0 + ro, w->prior_r0 + ro + dim);
            B.prior_x0.insert(B.prior_x0.end(), w->prior_x0 + x0o, w->prior_x0 + x0o + gsum);
            int g = add_gf(GF_PRIOR, dim, data, blks);
            B.prior_gf.push_back(g);
            prior_first_gf.push_back(g);
            {
                HostWin::LinPrior lp{ g, dim, gsum, {} };
                for (int b : blks) for (int q = 0; q < ls[b]; q++) lp.col_x.push_back(gs[b] == 1 ? gx(b) : -1);
                hw.lin_prior.push_back(std::move(lp));
            }
            B.max_prior_dim = std::max(B.max_prior_dim, dim);
            bo += nbk; jo += (long long)dim * dim; ro += dim; x0o += gsum;
        }
    }
    // composite IMU-GNSS factors: carried as prior-type factors whose record k_comp_scatter rewrites at every linearisation
    hw.comp_pose = w->comp_pose; hw.comp_sb = w->comp_sb; hw.comp_e0 = (int)(B.co_pose.size() / 7);
    {
        int io = 0; long long pn = 0, nn = 0; int no = 0, e0 = 0;
        for (int k = 0; k < w->n_comp; k++) {
            const int M = w->comp_M[k], N = w->comp_N[k], G = 30 + N;
            if (M < 1) return refuse(err, SWF_E_INVALID, "composite factor without hidden epochs");
            if (N < 0 || N > CO_MAXN) return refuse(err, SWF_E_UNSUPPORTED, "composite factor with more than 64 ambiguities");
            const int* ix = w->comp_idx + io;
            CHK(ix[0], nP, "composite") CHK(ix[1], nS, "composite") CHK(ix[2], nP, "composite") CHK(ix[3], nS, "composite")
            std::vector<int> blks = { bidP(ix[0]), bidS(ix[1]), bidP(ix[2]), bidS(ix[3]) };
            for (int q = 0; q < N; q++) { CHK(ix[4 + q], nC, "composite") blks.push_back(bidC(ix[4 + q])); }
            for (size_t a = 0; a < blks.size(); a++) {
                if (loc[blks[a]] < 0) return refuse(err, SWF_E_UNSUPPORTED, "composite factor on a constant parameter block");
                for (size_t c2 = 0; c2 < a; c2++) if (blks[c2] == blks[a]) return refuse(err, SWF_E_INVALID, "composite factor: repeated parameter block");
            }
            int data = (int)B.prior_dim.size();
            B.prior_dim.push_back(G);
            B.prior_Joff.push_back((long long)B.prior_J.size()); B.prior_roff.push_back((int)B.prior_r0.size()); B.prior_x0off.push_back((int)B.prior_x0.size());
            B.prior_J.resize(B.prior_J.size() + (size_t)G * G, 0.0); B.prior_r0.resize(B.prior_r0.size() + G, 0.0);
            {   // a valid linearisation point until the first k_comp_scatter: the blocks' current values
                const double* src[4] = { w->pose + 7 * ix[0], w->sb + 9 * ix[1], w->pose + 7 * ix[2], w->sb + 9 * ix[3] };
                const int gsz[4] = { 7, 9, 7, 9 };
                for (int a = 0; a < 4; a++) B.prior_x0.insert(B.prior_x0.end(), src[a], src[a] + gsz[a]);
                for (int q = 0; q < N; q++) B.prior_x0.push_back(w->sc[ix[4 + q]]);
            }
            int g = add_gf(GF_PRIOR, G, data, blks);
            B.prior_gf.push_back(g);
            B.max_prior_dim = std::max(B.max_prior_dim, G);
            B.co_M.push_back(M); B.co_N.push_back(N); B.co_gf.push_back(g); B.co_win.push_back(wi);
            for (int b : blks) B.co_xo.push_back(gx(b));
            B.co_xo_off.push_back((int)B.co_xo.size());
            B.co_pose.insert(B.co_pose.end(), w->comp_pose + (size_t)e0 * 7, w->comp_pose + (size_t)(e0 + M) * 7);
            B.co_sb.insert(B.co_sb.end(), w->comp_sb + (size_t)e0 * 9, w->comp_sb + (size_t)(e0 + M) * 9);
            B.co_pose_lin.insert(B.co_pose_lin.end(), w->comp_pose_lin + (size_t)e0 * 7, w->comp_pose_lin + (size_t)(e0 + M) * 7);
            B.co_sb_lin.insert(B.co_sb_lin.end(), w->comp_sb_lin + (size_t)e0 * 9, w->comp_sb_lin + (size_t)(e0 + M) * 9);
            B.co_Hpp.insert(B.co_Hpp.end(), w->comp_Hpp + (size_t)e0 * 225, w->comp_Hpp + (size_t)(e0 + M) * 225);
            B.co_HpN.insert(B.co_HpN.end(), w->comp_HpN + pn, w->comp_HpN + pn + 15LL * M * N);
            B.co_rhs_p.insert(B.co_rhs_p.end(), w->comp_rhs_p + (size_t)e0 * 15, w->comp_rhs_p + (size_t)(e0 + M) * 15);
            B.co_HNN.insert(B.co_HNN.end(), w->comp_HNN + nn, w->comp_HNN + nn + (long long)N * N);
            B.co_rhsN.insert(B.co_rhsN.end(), w->comp_rhsN + no, w->comp_rhsN + no + N);
            B.co_pre.insert(B.co_pre.end(), w->comp_pre + (size_t)(e0 + k) * SWF_PRE_DOUBLES, w->comp_pre + (size_t)(e0 + k + M + 1) * SWF_PRE_DOUBLES);
            {   // middle-marginalisation link (AddMidMargInfo): optional
                int mid = w->comp_mid ? w->comp_mid[k] : 0;
                if (mid != 0 && (mid < 1 || mid > M - 1 || !w->comp_H12)) return refuse(err, SWF_E_INVALID, "composite factor: comp_mid must be 0 or a link between two hidden epochs (1..M-1), with comp_H12 given");
                B.co_mid.push_back(mid);
                if (mid) B.co_H12.insert(B.co_H12.end(), w->comp_H12 + (size_t)k * 225, w->comp_H12 + (size_t)(k + 1) * 225);
                else B.co_H12.resize(B.co_H12.size() + 225, 0.0);
            }
            for (int q = 0; q < 3; q++) B.co_pbgw.push_back(w->pbg[q]);
            for (int q = 0; q < 3; q++) B.co_pbgw.push_back(w->gw[q]);
            io += 4 + N; pn += 15LL * M * N; nn += (long long)N * N; no += N; e0 += M;
        }
        hw.comp_ne = e0;
    }
#undef CHK
    R.gf1 = (int)B.gf.size();

    // ---- cliques
    R.cl0 = (int)B.cl.size();
    std::map<int, int> e_clique;            // window block id -> clique
    std::map<int, int> free_clique;         // first variable block -> clique (free factors)
    struct TmpC { int e; std::vector<int> facs; std::vector<int> mem; bool is_static; };
    std::vector<TmpC> tc;
    // group-0 non-landmark blocks, in ordering order, always get a clique
    for (int i = 0; i < w->n_order; i++) {
        int b = w->order_block[i];
        if (w->order_group[i] != 0) break;
        if (b >= nP + nS && b < nP + nS + nL && !lm_generic[b - nP - nS]) continue;      // fast-path landmarks: k_lm_schur
        e_clique[b] = (int)tc.size();
        tc.push_back(TmpC{ b, {}, {}, false });
    }
    for (int f = R.gf0; f < R.gf1; f++) {
        const TmpF& t = tf[f - R.gf0];
        int e = -1, first_var = -1;
        for (int b : t.blk) {
            if (loc[b] < 0) continue;
            if (first_var < 0) first_var = b;
            if (is_e(b)) {
                if (b >= nP + nS && b < nP + nS + nL && !lm_generic[b - nP - nS]) return refuse(err, SWF_E_UNSUPPORTED, "non-projection factor on a landmark");
                if (e >= 0 && e != b) return refuse(err, SWF_E_INVALID, "elimination group 0 is not an independent set");
                e = b;
            }
        }
        int c;
        if (e >= 0) c = e_clique[e];
        else if (B.gf[f].type == GF_PRIOR) { c = (int)tc.size(); tc.push_back(TmpC{ -1, {}, {}, true }); }
        else if (first_var < 0) continue;    // all-constant factor: contributes only to the cost
        else {
            auto it = free_clique.find(first_var);
            if (it == free_clique.end()) { c = (int)tc.size(); free_clique[first_var] = c; tc.push_back(TmpC{ -1, {}, {}, false }); }
            else c = it->second;
        }
        tc[c].facs.push_back(f);
        for (int b : t.blk) {
            if (loc[b] < 0 || b == e) continue;
            if (std::find(tc[c].mem.begin(), tc[c].mem.end(), b) == tc[c].mem.end()) tc[c].mem.push_back(b);
        }
    }
    // reduced offsets
    auto red = [&](int b) { return loc[b] - ne; };
    std::map<std::pair<int, int>, std::vector<std::array<long long, 3>>> pmap;   // (a,b) -> (coff, cld, voff)
    for (size_t ci = 0; ci < tc.size(); ci++) {
        TmpC& t = tc[ci];
        Clique C{};
        C.win = wi;
        C.d_e = t.e >= 0 ? ls[t.e] : 0;
        C.e_loc = t.e >= 0 ? gloc(t.e) : -1;
        C.fac0 = (int)B.cl_fac.size();
        int nrows = 0;
        for (int f : t.facs) { B.cl_fac.push_back(f); B.cl_frow.push_back(nrows); nrows += B.gf[f].nres; B.gf[f].clique = (int)B.cl.size(); }
        C.fac1 = (int)B.cl_fac.size();
        C.n_rows = nrows;

        C.mem0 = (int)B.cm_loc.size();
        int df = 0;
        std::map<int, int> colof;
        for (int b : t.mem) {
            B.cm_loc.push_back(gloc(b)); B.cm_ls.push_back(ls[b]); B.cm_col.push_back(df);
            colof[b] = df; df += ls[b];
        }
        C.mem1 = (int)B.cm_loc.size();
        C.d_f = df;
        if (!t.is_static && C.d_e + df > CB_MAXD) return refuse(err, SWF_E_UNSUPPORTED, "clique with more than 768 columns");
        if (!t.is_static && C.d_e > 9) return refuse(err, SWF_E_UNSUPPORTED, "group-0 block larger than 9 dimensions");
        // (k_clique_big keeps the e-rows of M and T = Einv M_ef in LDS: only the cliques that take it — beyond 64 x 64 / 96 x 64 — are bound by that)
        if (!t.is_static && (nrows > CLQ_TALLR || C.d_e + df > 64) && (long long)C.d_e * (C.d_e + df) > CB_MAXED)
            return refuse(err, SWF_E_UNSUPPORTED, "clique beyond one wavefront with d_e (d_e + d_f) > 1536 (swf_solver.h: limits of a group-0 clique)");
        C.C_off = B.C_tot; B.C_tot += (long long)df * df;
        C.v_off = B.v_tot; B.v_tot += df;
        C.e_off = B.e_tot; B.e_tot += C.d_e * C.d_e + C.d_e * df + C.d_e;
        C.is_static = t.is_static ? 1 : 0;
        // slot -> clique column
        for (int f : t.facs) {
            const TmpF& tff = tf[f - R.gf0];
            for (size_t sl = 0; sl < tff.blk.size(); sl++) {
                int b = tff.blk[sl];
                int cc = -1;
                if (loc[b] >= 0) cc = (b == t.e) ? 0 : C.d_e + colof[b];
                B.s_ccol[B.gf[f].slot0 + sl] = cc;
            }
        }
        // storage: a non-static clique owns a dense column-major Jacobian [d][n_rows] in g_J (each factor's blocks sit at
        // their (row, column) position, column stride n_rows) and contiguous residual rows in g_r; factors of static cliques
        // only need residual rows
        C.r_off = B.r_tot; B.r_tot += nrows;
        C.j_off = B.j_tot;
        {
            int dcl = C.d_e + df, frow = 0;
            for (int f : t.facs) {
                GFac& G = B.gf[f];
                G.roff = C.r_off + frow; G.jld = nrows;
                for (int sl = 0; sl < G.nslot; sl++) {
                    int cc = B.s_ccol[G.slot0 + sl];
                    // a prior-type record inside the clique of a group-0 block (a composite factor on an eliminated speed-bias block, as
                    // MyOrdering produces them, R/swf/swf_gnss.cpp:683-691): its rows join the clique's dense Jacobian like any factor's —
                    // the prior evaluation copies the record's columns there at every linearisation
                    if (G.type == GF_PRIOR && !t.is_static && cc >= 0) B.s_joff[G.slot0 + sl] = 0;
                    if (B.s_joff[G.slot0 + sl] < 0) continue;
                    if (t.is_static || cc < 0) { B.s_joff[G.slot0 + sl] = -1; continue; }
                    B.s_joff[G.slot0 + sl] = C.j_off + cc * nrows + frow;
                }
                frow += G.nres;
            }
            if (!t.is_static) B.j_tot += nrows * dcl;
        }
        // static prior clique: C = J^T J over member columns, dgraw = diag
        B.C_init.resize((size_t)B.C_tot, 0.0);
        B.dgraw_init.resize((size_t)B.v_tot, 0.0);
        if (t.is_static) {
            const GFac& G = B.gf[t.facs[0]];
            int dim = G.nres;
            const double* J = B.prior_J.data() + B.prior_Joff[G.data];
            // prior column -> member column (or -1)
            std::vector<int> pcol(dim, -1);
            {
                int col = 0;
                const TmpF& tff = tf[t.facs[0] - R.gf0];
                for (int b : tff.blk) { if (loc[b] >= 0) for (int j = 0; j < ls[b]; j++) pcol[col + j] = colof[b] + j; col += ls[b]; }
            }
            double* Cm = B.C_init.data() + C.C_off;
            for (int a = 0; a < dim; a++) {
                if (pcol[a] < 0) continue;
                for (int b2 = 0; b2 < dim; b2++) {
                    if (pcol[b2] < 0) continue;
                    double sacc = 0;
                    for (int r = 0; r < dim; r++) sacc += J[(size_t)r * dim + a] * J[(size_t)r * dim + b2];
                    Cm[(size_t)pcol[a] * df + pcol[b2]] = sacc;
                }
                B.dgraw_init[C.v_off + pcol[a]] = Cm[(size_t)pcol[a] * df + pcol[a]];
            }
        }
        // pair contributions
        for (int a : t.mem) for (int b2 : t.mem) {
            if (red(a) < red(b2)) continue;
            pmap[{ a, b2 }].push_back({ C.C_off + (long long)colof[a] * df + colof[b2], df, C.v_off + colof[a] });
        }
        B.cl.push_back(C);
    }
    R.cl1 = (int)B.cl.size();
    // factors outside every clique (all blocks constant) still own residual rows (cost only)
    for (int f = R.gf0; f < R.gf1; f++) if (B.gf[f].roff < 0) { B.gf[f].roff = B.r_tot; B.r_tot += B.gf[f].nres; }

    // ---- pairs: clique pairs, all frame pairs, a diagonal pair for every reduced block
    for (int p = 0; p < nP; p++) if (frame_of[p] >= 0)
        for (int q = 0; q < nP; q++) if (frame_of[q] >= 0 && red(bidP(p)) >= red(bidP(q))) pmap[{ bidP(p), bidP(q) }];
    for (int i = 0; i < w->n_order; i++) { int b = w->order_block[i]; if (!is_e(b)) pmap[{ b, b }]; }
    R.pair0 = (int)B.pair.size();
    for (auto& kv : pmap) {
        int a = kv.first.first, b2 = kv.first.second;
        Pair P{};
        P.win = wi; P.ra = red(a); P.rb = red(b2); P.la = ls[a]; P.lb = ls[b2];
        P.fa = a < nP ? frame_of[a] : -1; P.fb = b2 < nP ? frame_of[b2] : -1;
        P.c0 = (int)B.pc_coff.size();
        for (auto& c : kv.second) { B.pc_coff.push_back(c[0]); B.pc_cld.push_back((int)c[1]); B.pc_voff.push_back((int)c[2]); }
        P.c1 = (int)B.pc_coff.size();
        P.is_diag = (a == b2) ? 1 : 0;
        P.loc_a = gloc(a);
        B.pair.push_back(P);
    }
    R.pair1 = (int)B.pair.size();

    R.proj_sqrt_info = w->proj_sqrt_info; R.proj_loss_a = w->proj_loss_a;
    for (int k = 0; k < 3; k++) { R.pbg[k] = w->pbg[k]; R.gw[k] = w->gw[k]; R.base[k] = w->base[k]; }
    B.n_x += R.x_n; B.n_loc += R.n_loc;
    // algorithmic Jacobian bytes of one evaluation (SURVEY.md §8d formula)
    {
        int64_t pb = 0;
        for (int k = 0; k < w->n_prior; k++) { int64_t n = w->prior_dim[k]; pb += 8 * (n * n + 4 * n); }
        B.jac_bytes += (int64_t)312 * w->n_proj + (int64_t)5480 * w->n_imu + (int64_t)176 * w->n_cp + (int64_t)152 * w->n_pr + (int64_t)208 * w->n_dop
                     + (int64_t)136 * w->n_spr + (int64_t)160 * w->n_scp + (int64_t)56 * w->n_fix + (int64_t)584 * w->n_idp + pb;
    }
    B.win.push_back(R);
    return SWF_OK;
}

// flop and byte counters of the batch; the reduced systems' size range and which instances of k_chol_rr4 it needs
void plan_counters(Plan& B) {
    B.proj_bytes = (int64_t)312 * (int64_t)B.p_win.size();
    for (size_t l = 0; l + 1 < B.lm_obs0.size() + 1 && l < B.lm_win.size(); l++) {
        int64_t k = (l + 1 < B.lm_obs0.size() ? B.lm_obs0[l + 1] : (int)B.p_win.size()) - B.lm_obs0[l];
        B.lm_schur_flops += 216 * k * k + 108 * k;
        B.lm_schur_flops_sym += 108 * k * (k - 1) + 162 * k;
    }
    for (auto& W : B.win) { B.chol_flops += (int64_t)W.n_red * W.n_red * W.n_red / 3; B.max_red = std::max(B.max_red, W.n_red); B.min_red = std::min(B.min_red, W.n_red); if (W.n_red > 224 && W.n_red <= 240) B.rr4_has15 = true; if (W.n_red > 240 && W.n_red <= 256) B.rr4_has16 = true; }
}

// (the steps below run once per batch, in this order: plan_build)
int plan_lm_blocks(Plan& B, std::string& err) {
    // landmark back-substitution blocks: consecutive landmarks of one window with at most 256 observations together
    // (built before the window records are uploaded: a window knows its block range, WinRec::lmb0 / lmb1)
    std::vector<int>& lr = B.lmb_rec;
    std::vector<int> obs0 = B.lm_obs0; obs0.push_back((int)B.p_win.size());
    for (WinRec& Wr : B.win) {
        Wr.lmb0 = (int)(lr.size() / 4);
        int l = Wr.lm0;
        while (l < Wr.lm1) {
            const int o0 = obs0[(size_t)l]; int l1 = l, cnt = 0;
            while (l1 < Wr.lm1 && l1 - l < 256 && cnt + (obs0[(size_t)l1 + 1] - obs0[(size_t)l1]) <= 256) { cnt += obs0[(size_t)l1 + 1] - obs0[(size_t)l1]; l1++; }
            if (l1 == l) return refuse(err, SWF_E_UNSUPPORTED, "landmark with more than 256 observations");
            lr.push_back(o0); lr.push_back(cnt); lr.push_back(l); lr.push_back(l1 - l);
            l = l1;
        }
        Wr.lmb1 = (int)(lr.size() / 4);
    }
    B.n_lmb = (int)(lr.size() / 4);
    if (lr.empty()) lr.resize(4, 0);
    return SWF_OK;
}

void plan_prior_chunks(Plan& B) {
    std::vector<int>&pch_q = B.pch_q, &pch_r0 = B.pch_r0, &prior_nch = B.prior_nch;
    // row chunks of the priors (swf_records.h): a prior beyond PRIOR_SPLIT_DIM rows is evaluated by one workgroup per PRIOR_CHUNK rows;
    // a window's priors (the composite factors' records among them) are contiguous in prior_gf, and so are their chunks
    for (WinRec& Wr : B.win) { Wr.pch0 = 0; Wr.pch1 = 0; }
    int cur_w = -1;
    for (size_t q = 0; q < B.prior_gf.size(); q++) {
        const GFac& G = B.gf[(size_t)B.prior_gf[q]];
        const int n = G.nres, nch = n > PRIOR_SPLIT_DIM ? (n + PRIOR_CHUNK - 1) / PRIOR_CHUNK : 1;
        if (G.win != cur_w) { cur_w = G.win; B.win[(size_t)cur_w].pch0 = (int)pch_q.size(); }
        prior_nch.push_back(nch);
        for (int c = 0; c < nch; c++) { pch_q.push_back((int)q); pch_r0.push_back(nch > 1 ? c * PRIOR_CHUNK : 0); }
        B.win[(size_t)cur_w].pch1 = (int)pch_q.size();
        if (nch > 1 && G.clique >= 0 && B.cl[(size_t)G.clique].is_static) B.n_pch_split += nch;
    }
    B.n_pch = (int)pch_q.size();
    if (pch_q.empty()) { pch_q.push_back(0); pch_r0.push_back(0); }
    if (prior_nch.empty()) prior_nch.push_back(1);
}

void plan_schur_shape(Plan& B, const PlanShape& sh) {
    // k_lm_schur's launch shape: the row class of the panel by the batch's largest window (<= 10 / 21 / 42 / 64 observing frames) and
    // the landmark parts per block — as many as still leave >= 2 blocks per CU.  SWF_LS_VARIANT / SWF_LS_QPB: test / debugging aids.
    // A block that covers all parts folds them in registers (ls_folded) and, in that case, writes -P straight into S (s_direct); the
    // off-diagonal frame pairs without any other contribution then leave the assembly's list.
    const int n = B.n_win, force = sh.ls_variant, force_qpb = sh.ls_qpb;
    int qpb = 1;
    while (qpb < GEMM_SPLIT && (long long)n * GEMM_SPLIT / (2 * qpb) >= 2LL * B.n_cu) qpb *= 2;
    // from half a chip of windows on, one block per window: the folded product and the direct-to-S write-out are worth more than the
    // second round of blocks
    if (2LL * n >= B.n_cu) qpb = GEMM_SPLIT;
    if (force_qpb >= 1 && force_qpb <= GEMM_SPLIT && (force_qpb & (force_qpb - 1)) == 0) qpb = force_qpb;
    B.ls_qpb = qpb;
    B.ls_var = (B.max_tiles <= 10 && force < 1) ? 0 : (B.max_tiles <= 36 && force < 2) ? 1 : (B.max_tiles <= 136 && force < 3) ? 2 : 3;
    B.ls_folded = qpb == GEMM_SPLIT && ls_can_fold(ls_ncw(B.ls_var), ls_tpw(B.ls_var));      // the predicate k_lm_schur folds by
    B.s_direct = B.ls_folded;
    // the gradient-only pass of the final linearisation: never more parts per workgroup than the product kernel takes (the latency path
    // keeps its spread of a window over the chip).  SWF_LS_GRAD_QPB: test / measuring aid.
    const int force_gqpb = sh.ls_grad_qpb;
    B.ls_gqpb = std::min(qpb, LS_GRAD_QPB);
    if (force_gqpb >= 1 && force_gqpb <= GEMM_SPLIT && (force_gqpb & (force_gqpb - 1)) == 0) B.ls_gqpb = force_gqpb;
}

int plan_schur_tasks(Plan& B, std::string& err) {
    // k_lm_schur task table.  A wave task = the four 16-lane groups of one producer wave = four landmarks, one group and three of the
    // task's twelve panel columns each (a track of more than 16 observations takes further rounds of its group's lanes).  Record of
    // (task, group): L (-1 = empty), loc, first / end observation of the landmark, first column within the task (0, 3, 6, 9).  The window's landmarks
    // enter in the order of their tile footprint (last, first 16-row tile of the reduced camera matrix they touch), so the landmarks of a
    // task mostly share theirs; bit g of the tile mask of (chunk, tile) — some landmark of the chunk's wave task g is seen from the tile's
    // row frames and from its column frames, per k-step of the task since round 4 (three bits per task: a tile skips the k-steps none of
    // whose landmarks touch it) — is what the consumer waves walk (a chunk = TW tasks, by size class; the packing into tasks
    // and the parts, which end on even task numbers, are the same in every class: so is every sum).  Tile list of a window: the nt
    // diagonal tiles, then (tr > tc) row by row.
    const int TW = B.ls_var <= 1 ? 2 : 1;
    const int NCW = ls_ncw(B.ls_var), TPW = ls_tpw(B.ls_var);
    const int n_launch = std::max(1, (B.max_tiles + NCW * TPW - 1) / (NCW * TPW));
    B.ls_kms = n_launch * NCW;                                  // mask words per chunk
    std::vector<int>&c0 = B.sch_c0, &rec = B.sch_rec, &km = B.sch_km;
    std::vector<std::vector<unsigned>> task_tiles;               // per task of the current window: tile-list entries it touches
    for (auto& W : B.win) {
        const int m = 6 * W.nF, nt = (m + 15) / 16, ntl = nt * (nt + 1) / 2;
        auto tile_rows = [&](unsigned long long fm) {          // 16-row tiles the frames of fm touch
            unsigned t = 0;
            for (int f = 0; f < W.nF && f < 64; f++) if ((fm >> f) & 1ULL) { t |= 1u << ((6 * f) / 16); t |= 1u << ((6 * f + 5) / 16); }
            return t;
        };
        std::vector<int> ord; std::vector<unsigned> trs((size_t)(W.lm1 - W.lm0), 0u);
        for (int l = W.lm0; l < W.lm1; l++) {
            if (B.lm_loc[l] < 0) continue;                     // constant landmark: nothing to eliminate
            int k = B.lm_obs0[l + 1] - B.lm_obs0[l];
            if (k > 64) return refuse(err, SWF_E_UNSUPPORTED, "landmark with more than 64 observations");
            trs[(size_t)(l - W.lm0)] = tile_rows(B.lm_fmask[l]);
            ord.push_back(l);
        }
        auto key = [&](int l) { unsigned t = trs[(size_t)(l - W.lm0)]; int lo = t ? __builtin_ctz(t) : 0, hi = t ? 31 - __builtin_clz(t) : 0; return hi * 64 + lo; };
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return key(x) < key(y); });
        const int first_task = (int)(rec.size() / 32);
        task_tiles.clear();
        size_t at = 0; int lw = 4;                             // force a new task at the first landmark
        auto new_task = [&]() { at = rec.size(); rec.resize(at + 32, 0); for (int g = 0; g < 4; g++) rec[at + g * 8] = -1; task_tiles.emplace_back((size_t)ntl, 0u); lw = 0; };
        for (int l : ord) {
            int o0 = B.lm_obs0[l], k = B.lm_obs0[l + 1] - o0;
            if (lw >= 4) new_task();
            int* r = &rec[at + (size_t)lw * 8];                 // group lw of the task = this landmark, whatever its track length
            r[0] = l; r[1] = B.lm_loc[l]; r[2] = o0; r[3] = o0 + k; r[4] = 3 * lw; r[5] = 0; r[6] = 0; r[7] = 0;
            // tile-list entries this landmark touches, as the k-steps of the task that carry its three columns (columns 3 lw .. 3 lw + 2 of
            // the task's twelve; a k-step = four columns): group 0 -> k-step 0, group 1 -> 0 and 1, group 2 -> 1 and 2, group 3 -> 2
            unsigned t = trs[(size_t)(l - W.lm0)];
            const unsigned ks = lw == 0 ? 1u : lw == 1 ? 3u : lw == 2 ? 6u : 4u;
            std::vector<unsigned>& tt = task_tiles.back();
            for (int tr = 0; tr < nt; tr++) {
                if (!((t >> tr) & 1u)) continue;
                tt[(size_t)tr] |= ks;
                for (int tc = 0; tc < tr; tc++) if ((t >> tc) & 1u) tt[(size_t)(nt + tr * (tr - 1) / 2 + tc)] |= ks;
            }
            lw++;
        }
        if (task_tiles.size() & 1) new_task();                 // an even number of tasks per window
        const int ntask = (int)task_tiles.size();
        // masks: chunk c of this window = tasks [c TW, (c + 1) TW)
        for (int c = 0; c < ntask / TW; c++) {
            size_t kw = km.size(); km.resize(kw + (size_t)B.ls_kms, 0);
            for (int g = 0; g < TW; g++) {
                const std::vector<unsigned>& tt = task_tiles[(size_t)(c * TW + g)];
                for (int e = 0; e < ntl; e++) if (tt[(size_t)e]) {
                    B.lm_schur_mfma += __builtin_popcount(tt[(size_t)e]);
                    int lp = e / (NCW * TPW), r = e % (NCW * TPW), sl = r / NCW, cw = r % NCW;
                    km[kw + (size_t)(lp * NCW + cw)] |= (tt[(size_t)e] << (3 * g)) << (3 * TW * sl);
                }
            }
        }
        // part sp = task pairs [sp np / 16, (sp + 1) np / 16): the parts differ by at most one pair, so any grouping of consecutive parts
        // into workgroups (qpb = 1 .. 16, by batch size) is balanced
        const int np = ntask / 2;
        for (int sp = 0; sp < GEMM_SPLIT; sp++) c0.push_back(first_task + 2 * (int)((long long)sp * np / GEMM_SPLIT));
    }
    c0.push_back((int)(rec.size() / 32));
    rec.resize(rec.size() + (size_t)32 * 4 * LS_NB, 0);           // slack behind the table
    km.resize(km.size() + (size_t)B.ls_kms * 2, 0);
    return SWF_OK;
}

// the closing entries of the frame / frame-sum CSR arrays, and the frame-sum block records
void plan_frame_sums(Plan& B) {
    B.fr_obs0.push_back((int)B.fr_obs.size());
    B.fsb_obs0.push_back(B.n_proj); B.fsb_perm.resize((size_t)B.n_proj + 1, 0);
    // one 32-byte record per frame-sum block (layout: ProjBlk, swf_kernels.h): everything the block's evaluation needs to address its loads comes with ONE load
    std::vector<int>& rec = B.fsb_rec;
    rec.assign((size_t)8 * std::max(B.n_fsb, 1), 0);
    for (int k = 0; k < B.n_fsb; k++) {
        int* r = rec.data() + (size_t)8 * k;
        r[0] = B.fsb_win[(size_t)k]; r[1] = B.fsb_obs0[(size_t)k]; r[2] = B.fsb_obs0[(size_t)k + 1] - B.fsb_obs0[(size_t)k];
        r[3] = B.fsb_foff0[(size_t)k]; r[4] = B.fsb_out0[(size_t)k]; r[5] = B.win[(size_t)r[0]].nF;
    }
}

int plan_jt_records(Plan& B, std::string& err) {
    // flat J v records of the scalar and the IMU factors (JtRec, swf_records.h): the factor and its slots as the tables above hold them
    bool fits = true;
    auto jt_recs = [&](const std::vector<int>& list) {
        std::vector<JtRec> out(list.size());
        for (size_t q = 0; q < list.size(); q++) {
            const GFac& G = B.gf[(size_t)list[q]];
            JtRec& r = out[q];
            r = JtRec{};
            r.win = G.win; r.nres = G.nres; r.jld = G.jld; r.nslot = G.nslot; r.roff = G.roff; r.f = list[q];
            if (G.nslot > JT_MAXSLOT) { fits = false; continue; }
            for (int t = 0; t < JT_MAXSLOT; t++) {
                const bool has = t < G.nslot;
                r.joff[t] = has ? B.s_joff[(size_t)G.slot0 + t] : -1; r.loc[t] = has ? B.s_loc[(size_t)G.slot0 + t] : 0; r.ls[t] = has ? B.s_ls[(size_t)G.slot0 + t] : 0;
            }
        }
        return out;
    };
    B.sc_jt = jt_recs(B.sc_gf); B.imu_jt = jt_recs(B.imu_gf);
    if (!fits) return refuse(err, SWF_E_UNSUPPORTED, "scalar / IMU factor with more than JT_MAXSLOT parameter blocks");
    // flat evaluation records of the IMU factors (ImuRec, swf_records.h): an IMU factor has its four slots, pose i, speed-bias i, pose j, speed-bias j
    B.imu_rec.assign(B.imu_gf.size(), ImuRec{});
    for (size_t q = 0; q < B.imu_gf.size(); q++) {
        const GFac& G = B.gf[(size_t)B.imu_gf[q]];
        ImuRec& r = B.imu_rec[q];
        r.win = G.win; r.f = B.imu_gf[q]; r.roff = G.roff; r.data = G.data; r.jld = G.jld;
        for (int t = 0; t < 4; t++) { const bool has = t < G.nslot; r.xo[t] = has ? B.s_x[(size_t)G.slot0 + t] : 0; r.joff[t] = has ? B.s_joff[(size_t)G.slot0 + t] : -1; }
    }
    return SWF_OK;
}

void plan_prior_maps(Plan& B) {
    // transposed copies of the prior records for the J v products
    std::vector<double>& Jt = B.prior_Jt;
    Jt.assign(B.prior_J.size(), 0.0);
    for (size_t k = 0; k < B.prior_dim.size(); k++) {
        const size_t n = (size_t)B.prior_dim[k]; const double* J = B.prior_J.data() + B.prior_Joff[k]; double* T = Jt.data() + B.prior_Joff[k];
        for (size_t r = 0; r < n; r++) for (size_t c = 0; c < n; c++) T[c * n + r] = J[r * n + c];
    }
    // column -> local index of every prior record (the J v products walk the columns flat, eight at a time)
    std::vector<int>&cl = B.prior_colloc, &cc = B.prior_colcc, &pcol = B.s_pcol, &pxo = B.s_pxo;
    cl.assign(B.prior_r0.size(), -1); cc.assign(B.prior_r0.size(), -1); pcol.assign(B.s_ls.size(), 0); pxo.assign(B.s_ls.size(), 0);
    for (const GFac& G : B.gf) {
        if (G.type != GF_PRIOR) continue;
        int col = 0, xo = 0;
        for (int t = 0; t < G.nslot; t++) {
            int l = B.s_ls[G.slot0 + t], lo = B.s_loc[G.slot0 + t], mc = B.s_ccol[G.slot0 + t];
            pcol[G.slot0 + t] = col; pxo[G.slot0 + t] = xo;
            for (int q = 0; q < l; q++) {
                cl[(size_t)B.prior_roff[G.data] + col + q] = lo >= 0 ? lo + q : -1;
                cc[(size_t)B.prior_roff[G.data] + col + q] = mc >= 0 ? mc + q : -1;
            }
            col += l; xo += (l == 6 ? 7 : l);
        }
    }
    // per clique vector slot: the local index of the variable behind it
    std::vector<int>& cvl = B.cv_loc;
    cvl.assign((size_t)std::max(B.v_tot, 1), 0);
    for (const Clique& c : B.cl)
        for (int m = c.mem0; m < c.mem1; m++)
            for (int q = 0; q < B.cm_ls[(size_t)m]; q++) cvl[(size_t)c.v_off + (size_t)B.cm_col[(size_t)m] + (size_t)q] = B.cm_loc[(size_t)m] + q;
}

// the pairs the assembly visits (pd / po: indices into B.pair) as self-contained records, and the cliques by size class
void plan_pair_clique_classes(Plan& B, std::vector<int>& pd, std::vector<int>& po) {
    std::vector<int> clc[5], cle;
    for (size_t i = 0; i < B.pair.size(); i++) {
        Pair& Pq = B.pair[i]; const WinRec& Rw = B.win[Pq.win];      // self-contained records (see Pair)
        Pq.fsb0 = Rw.fsb0; Pq.fsb1 = Rw.fsb1; Pq.n = Rw.n_red; Pq.m = 6 * Rw.nF; Pq.S_base = Rw.S_base; Pq.P_base = Rw.P_base; Pq.q_base = (long long)6 * Rw.fr_base * GEMM_SPLIT;
        if (B.s_direct && !Pq.is_diag && Pq.fa >= 0 && Pq.fb >= 0 && Pq.c0 == Pq.c1) continue;       // -P is already in S, nothing to add
        (Pq.is_diag ? pd : po).push_back((int)i);
    }
    // off-diagonal pairs by descending entry rounds (16 entries per round): the round-2 pair-walking assembly's waves (four pairs each) become
    // homogeneous and skip the rounds none of their pairs has; every pair is still written once, by the same arithmetic
    std::stable_sort(po.begin(), po.end(), [&](int a, int c) {
        return (B.pair[a].la * B.pair[a].lb + 15) / 16 > (B.pair[c].la * B.pair[c].lb + 15) / 16; });
    for (size_t i = 0; i < B.cl.size(); i++) {
        const Clique& c = B.cl[i];
        if (c.d_e > 0) cle.push_back((int)i);
        if (c.is_static) continue;
        int d = c.d_e + c.d_f;
        // one wavefront per clique up to 64 x 64 (three size classes); anything larger takes the workgroup kernel (class 3)
        int cls = (c.d_e <= 1 && d <= 32 && c.n_rows <= 48) ? 0 : (c.n_rows <= 32 && d <= 48) ? 1 : (c.n_rows <= CLQ_MAXR && d <= CLQ_MAXD) ? 2 : (c.n_rows <= CLQ_TALLR && d <= 64) ? 4 : 3;
        // latency path: every one-wavefront clique in ONE launch (the 64 x 64 instantiation; the classes differ in loop bounds and zero
        // padding only, the sums and their order are the same: bit-identical results)
        if (B.lat_fuse && cls < 2) cls = 2;
        clc[cls].push_back((int)i);
        for (int q = c.fac0; q < c.fac1; q++) if (B.gf[B.cl_fac[q]].type == GF_IMU) B.clc_imu[cls] = true;
    }
    B.n_pd = (int)pd.size(); B.n_po = (int)po.size(); B.n_cle = (int)cle.size();
    std::vector<Pair>&vd = B.pair_d, &vo = B.pair_o;
    for (int i : pd) vd.push_back(B.pair[i]);
    for (int i : po) vo.push_back(B.pair[i]);
    for (int i : cle) B.cle_rec.push_back(B.cl[i]);
    for (int k = 0; k < 5; k++) {
        for (int i : clc[k]) B.clc_rec[k].push_back(B.cl[i]);
        B.n_clc[k] = (int)clc[k].size();
    }
    // class 0 runs two cliques per wavefront out of dynamic LDS (k_clique_pack): rows x leading dimension of the largest one (odd, two pad columns)
    B.clp_rows = 1; B.clp_ld = 3;
    for (const Clique& c : B.clc_rec[0]) { B.clp_rows = std::max(B.clp_rows, c.n_rows); B.clp_ld = std::max(B.clp_ld, (c.d_e + c.d_f + 2) | 1); }
}

int plan_asm_programs(Plan& B, const std::vector<int>& pd, const std::vector<int>& po, std::string& err) {
    // ---- assembly programs (k_assemble_flat): every pair of the two lists above, flattened into per-entry source lists with
    // window-relative offsets; windows whose programs come out identical share one copy.  Entry order inside a window: the
    // window's pairs in pair order, (i, j) row-major — any order would do, every entry is written by exactly one thread.
    const int n_part = B.s_direct ? 0 : B.ls_folded ? 1 : GEMM_SPLIT, n_qpart = B.ls_folded ? 1 : GEMM_SPLIT;
    const int n = B.n_win;
    struct Prog { std::vector<int> dst, src0, aux, src, vloc, vred, vsrc0, vi, vsrc; std::vector<unsigned> cnt, vcnt; };
    std::vector<AsmWin>& asw = B.asw;
    asw.assign((size_t)n, AsmWin{});
    std::vector<int>&t_dst = B.as_dst, &t_src0 = B.as_src0, &t_aux = B.as_aux, &t_src = B.as_src, &tv_loc = B.av_loc, &tv_red = B.av_red, &tv_src0 = B.av_src0, &tv_i = B.av_i, &tv_src = B.av_src;
    std::vector<unsigned>&t_cnt = B.as_cnt, &tv_cnt = B.av_cnt;
    std::map<std::vector<int>, std::array<int, 4>> seen;           // serialised program -> (se0, ne, ve0, nv)
    std::vector<std::vector<int>> wpairs((size_t)n);
    for (int i : pd) wpairs[(size_t)B.pair[i].win].push_back(i);
    for (int i : po) wpairs[(size_t)B.pair[i].win].push_back(i);
    bool overflow = false;
    // the 16 x 16 tiles of S some block pair reaches, strictly below the tile diagonal (the diagonal tiles are always loaded): from
    // EVERY pair of the window — the frame pairs whose only contribution is the -P that k_lm_schur writes straight into S have
    // left the assembly's lists above, but their tiles are not zero
    std::vector<unsigned>& tnz = B.s_tnz;
    tnz.assign((size_t)n * 4, 0u);
    for (const Pair& Pq : B.pair) {
        if (B.win[(size_t)Pq.win].n_red > 256) continue;
        for (int I = Pq.ra / 16; I <= (Pq.ra + Pq.la - 1) / 16; I++)
            for (int J = Pq.rb / 16; J <= (Pq.rb + Pq.lb - 1) / 16 && J < I; J++) { const int t = I * (I - 1) / 2 + J; tnz[(size_t)Pq.win * 4 + (t >> 5)] |= 1u << (t & 31); }
    }
    for (int w = 0; w < n; w++) {
        const WinRec& Rw = B.win[w];
        AsmWin& A = asw[(size_t)w];
        A.win = w; A.n_red = Rw.n_red; A.m = 6 * Rw.nF; A.loc_base = Rw.loc_base; A.S_base = Rw.S_base;
        A.P_base = Rw.P_base * GEMM_SPLIT; A.q_base = (long long)6 * Rw.fr_base * GEMM_SPLIT;
        A.fs_base = Rw.fsb1 > Rw.fsb0 ? B.fsb_out0[(size_t)Rw.fsb0] : 0;
        long long Cb = -1; int vb = -1;
        for (int c = Rw.cl0; c < Rw.cl1; c++) { if (Cb < 0 || B.cl[c].C_off < Cb) Cb = B.cl[c].C_off; if (vb < 0 || B.cl[c].v_off < vb) vb = B.cl[c].v_off; }
        A.C_base = Cb < 0 ? 0 : Cb; A.v_base = vb < 0 ? 0 : vb;
        Prog Pg;
        const int nfsb = Rw.fsb1 - Rw.fsb0, mm = A.m;
        for (int pi_ : wpairs[(size_t)w]) {
            const Pair& Pq = B.pair[(size_t)pi_];
            const bool frame_pair = Pq.fa >= 0 && Pq.fb >= 0, obs = Pq.is_diag && Pq.fa >= 0;
            const int ncon = Pq.c1 - Pq.c0;
            for (int i = 0; i < Pq.la; i++) for (int j = 0; j < Pq.lb; j++) {
                if (Pq.is_diag && j > i) continue;                  // lower half only; the mirror is the host's job at export
                const bool dg = Pq.is_diag && i == j;
                const int nP = frame_pair ? n_part : 0, nH = obs ? nfsb : 0;
                if (ncon > 4095 || nH > 4095) overflow = true;
                Pg.dst.push_back((Pq.ra + i) * Pq.n + Pq.rb + j);
                Pg.cnt.push_back((unsigned)ncon | ((unsigned)nP << 12) | ((unsigned)nH << 17) | ((dg ? 1u : 0u) << 29) | ((frame_pair && B.s_direct ? 1u : 0u) << 30));
                Pg.src0.push_back((int)Pg.src.size());
                Pg.aux.push_back(dg ? (Pq.loc_a - Rw.loc_base) + i : 0);
                for (int c = Pq.c0; c < Pq.c1; c++) Pg.src.push_back((int)(B.pc_coff[(size_t)c] + (long long)i * B.pc_cld[(size_t)c] + j - A.C_base));
                if (nP) {
                    const int pr = 6 * Pq.fa + i, pc = 6 * Pq.fb + j;
                    const long long pel = pr >= pc ? (long long)pr * mm + pc : (long long)pc * mm + pr;
                    for (int q = 0; q < nP; q++) Pg.src.push_back((int)((long long)q * mm * mm + pel));
                }
                if (nH) {
                    const int hi = i > j ? i : j, lo = i > j ? j : i;
                    for (int k2 = Rw.fsb0; k2 < Rw.fsb1; k2++) Pg.src.push_back((B.fsb_out0[(size_t)k2] - A.fs_base + Pq.fa) * FS_VAL + hi * (hi + 1) / 2 + lo);
                }
                if (dg) for (int c = Pq.c0; c < Pq.c1; c++) Pg.src.push_back(B.pc_voff[(size_t)c] + i - A.v_base);
            }
            if (!Pq.is_diag) continue;
            for (int i = 0; i < Pq.la; i++) {
                const int nH = obs ? nfsb : 0, nQ = obs ? n_qpart : 0;
                Pg.vloc.push_back(Pq.loc_a - Rw.loc_base + i); Pg.vred.push_back(Pq.ra + i); Pg.vi.push_back(obs ? i : 0);
                Pg.vcnt.push_back((unsigned)ncon | ((unsigned)nQ << 12) | ((unsigned)nH << 17));
                Pg.vsrc0.push_back((int)Pg.vsrc.size());
                if (nH) for (int k2 = Rw.fsb0; k2 < Rw.fsb1; k2++) Pg.vsrc.push_back((B.fsb_out0[(size_t)k2] - A.fs_base + Pq.fa) * FS_VAL);
                for (int c = Pq.c0; c < Pq.c1; c++) Pg.vsrc.push_back(B.pc_voff[(size_t)c] + i - A.v_base);
                for (int q = 0; q < nQ; q++) Pg.vsrc.push_back(q * mm + 6 * Pq.fa + i);
            }
        }
        // serialise and look up
        std::vector<int> key;
        key.reserve(Pg.dst.size() * 4 + Pg.src.size() + Pg.vloc.size() * 5 + Pg.vsrc.size() + 8);
        key.push_back((int)Pg.dst.size()); key.push_back((int)Pg.vloc.size());
        key.insert(key.end(), Pg.dst.begin(), Pg.dst.end()); for (unsigned c : Pg.cnt) key.push_back((int)c);
        key.insert(key.end(), Pg.src0.begin(), Pg.src0.end()); key.insert(key.end(), Pg.aux.begin(), Pg.aux.end()); key.insert(key.end(), Pg.src.begin(), Pg.src.end());
        key.insert(key.end(), Pg.vloc.begin(), Pg.vloc.end()); key.insert(key.end(), Pg.vred.begin(), Pg.vred.end()); for (unsigned c : Pg.vcnt) key.push_back((int)c);
        key.insert(key.end(), Pg.vsrc0.begin(), Pg.vsrc0.end()); key.insert(key.end(), Pg.vi.begin(), Pg.vi.end()); key.insert(key.end(), Pg.vsrc.begin(), Pg.vsrc.end());
        auto it = seen.find(key);
        if (it == seen.end()) {
            const int se0 = (int)t_dst.size(), ve0 = (int)tv_loc.size(), so = (int)t_src.size(), vo = (int)tv_src.size();
            t_dst.insert(t_dst.end(), Pg.dst.begin(), Pg.dst.end()); t_cnt.insert(t_cnt.end(), Pg.cnt.begin(), Pg.cnt.end()); t_aux.insert(t_aux.end(), Pg.aux.begin(), Pg.aux.end());
            for (int x : Pg.src0) t_src0.push_back(x + so);
            t_src.insert(t_src.end(), Pg.src.begin(), Pg.src.end());
            tv_loc.insert(tv_loc.end(), Pg.vloc.begin(), Pg.vloc.end()); tv_red.insert(tv_red.end(), Pg.vred.begin(), Pg.vred.end()); tv_cnt.insert(tv_cnt.end(), Pg.vcnt.begin(), Pg.vcnt.end());
            tv_i.insert(tv_i.end(), Pg.vi.begin(), Pg.vi.end());
            for (int x : Pg.vsrc0) tv_src0.push_back(x + vo);
            tv_src.insert(tv_src.end(), Pg.vsrc.begin(), Pg.vsrc.end());
            it = seen.emplace(std::move(key), std::array<int, 4>{ se0, (int)Pg.dst.size(), ve0, (int)Pg.vloc.size() }).first;
        }
        A.se0 = it->second[0]; A.ne = it->second[1]; A.ve0 = it->second[2]; A.nv = it->second[3];
        B.as_max_ne = std::max(B.as_max_ne, A.ne); B.as_max_nv = std::max(B.as_max_nv, A.nv);
    }
    if (overflow) return refuse(err, SWF_E_UNSUPPORTED, "assembly program: more than 4095 contributions to one entry of the reduced system");
    B.asm_programs = (int)seen.size();
    auto nonempty_i = [](std::vector<int>& v) { if (v.empty()) v.push_back(0); };
    auto nonempty_u = [](std::vector<unsigned>& v) { if (v.empty()) v.push_back(0u); };
    nonempty_i(t_dst); nonempty_u(t_cnt); nonempty_i(t_src0); nonempty_i(t_aux); nonempty_i(t_src);
    nonempty_i(tv_loc); nonempty_i(tv_red); nonempty_u(tv_cnt); nonempty_i(tv_src0); nonempty_i(tv_i); nonempty_i(tv_src);
    return SWF_OK;
}

int plan_composite(Plan& B, std::string& err) {
    B.n_comp = (int)B.co_M.size();
    // composite IMU-GNSS factors: offsets of the operator's arguments over the whole batch + where each factor's prior record and clique live
    if (B.n_comp) {
        const int nc = B.n_comp;
        std::vector<int>&eo = B.co_eo, &no = B.co_no, &roff = B.co_roff, &x0off = B.co_x0off, &voff = B.co_voff;
        std::vector<long long>&pno = B.co_pno, &nno = B.co_nno, &go = B.co_go, &g2o = B.co_g2o, &Joff = B.co_Joff, &Coff = B.co_Coff;
        eo.assign(nc + 1, 0); no.assign(nc + 1, 0); roff.assign(nc, 0); x0off.assign(nc, 0); voff.assign(nc, 0);
        pno.assign(nc + 1, 0); nno.assign(nc + 1, 0); go.assign(nc + 1, 0); g2o.assign(nc + 1, 0); Joff.assign(nc, 0); Coff.assign(nc, 0);
        for (int f = 0; f < nc; f++) {
            const int M = B.co_M[f], N = B.co_N[f], G = 30 + N;
            B.comp_nmax = std::max(B.comp_nmax, N); B.comp_nmin = std::min(B.comp_nmin, N);
            eo[f + 1] = eo[f] + M; no[f + 1] = no[f] + N; pno[f + 1] = pno[f] + 15LL * M * N; nno[f + 1] = nno[f] + (long long)N * N;
            go[f + 1] = go[f] + G; g2o[f + 1] = g2o[f] + (long long)G * G;
            const GFac& Gf = B.gf[B.co_gf[f]];
            const Clique& Cq = B.cl[Gf.clique];
            // either its own static clique (every block outside group 0: k_comp_scatter writes C = H and the diagonal there), or a member of
            // the clique of the ONE group-0 block it touches (its rows reach the elimination through the clique's Jacobian: Coff = -1)
            if (Cq.is_static ? (Cq.d_f != G || Cq.d_e != 0) : (Cq.d_e <= 0)) return refuse(err, SWF_E_UNSUPPORTED, "composite factor: its blocks must all be variable");
            Joff[f] = B.prior_Joff[Gf.data]; roff[f] = B.prior_roff[Gf.data]; x0off[f] = B.prior_x0off[Gf.data];
            Coff[f] = Cq.is_static ? Cq.C_off : -1; voff[f] = Cq.is_static ? Cq.v_off : -1;
        }
        B.comp_ne = eo[nc];
        std::vector<int>&qf = B.co_iq_f, &qk = B.co_iq_k;
        for (int f = 0; f < nc; f++) for (int k = 0; k <= B.co_M[f]; k++) { qf.push_back(f); qk.push_back(k); }
    }
    return SWF_OK;
}
}  // namespace

PlanShape plan_shape_from_env(int n_cu) {
    auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; };
    PlanShape sh;
    sh.n_cu = n_cu;
    sh.no_lat_fuse = getenv("SWF_NO_LAT_FUSE") != nullptr; sh.no_chol_col = getenv("SWF_NO_CHOL_COL") != nullptr;
    sh.ls_variant = num("SWF_LS_VARIANT"); sh.ls_qpb = num("SWF_LS_QPB"); sh.ls_grad_qpb = num("SWF_LS_GRAD_QPB");
    return sh;
}

int plan_build(const swf_flat_window* const* windows, int n, const PlanShape& sh, Plan& B, std::string& err) {
    int rc;
    B.hw.resize((size_t)n);
    for (int i = 0; i < n; i++) if ((rc = plan_window(B, windows[i], i, B.hw[(size_t)i], err)) != SWF_OK) return rc;
    if (B.n_x > 0x7fffffffLL || B.n_loc > 0x7fffffffLL) return refuse(err, SWF_E_UNSUPPORTED, "batch too large for 32-bit offsets");
    B.n_win = n; B.n_cu = sh.n_cu;
    B.n_proj = (int)B.p_win.size(); B.n_lm = (int)B.lm_win.size(); B.n_fsb = (int)B.fsb_win.size();
    // latency path (up to n_CU / 8 windows): independent kernels of an iteration ride in ONE grid (the IMU factors with the projection /
    // scalar factors, every clique size class in one launch) on ONE stream.  Round 3 ran the IMU / clique branch of such batches on the
    // auxiliary stream instead; the kernel trace shows what that buys: every cross-queue edge (event record -> stream wait) costs 6-13 us
    // of dependency resolution, as much as the overlap saves (one window: 1.432 ms with the auxiliary stream, 1.443 without).
    B.lat_fuse = n * 8 <= B.n_cu && !sh.no_lat_fuse;
    // auxiliary stream: the latency path (<= n_CU / 16 windows), and batches of half a chip to a chip of windows, where the IMU / clique branch
    // fills what one-block-per-window kernels leave idle (measured: 256 windows 5.52 -> 5.22 ms, 128 windows 3.73 -> 3.49 ms per solve; 64 and
    // 512 windows: no gain)
    B.want_aux = (n * 16 <= B.n_cu && !B.lat_fuse) || (2 * n >= B.n_cu && n <= B.n_cu);            // fork / join inside a linearisation
    plan_counters(B);
    if ((rc = plan_lm_blocks(B, err)) != SWF_OK) return rc;
    plan_prior_chunks(B);
    if (B.loc2x.empty()) B.loc2x.push_back(-1);
    B.lm_obs0.push_back(B.n_proj);
    plan_schur_shape(B, sh);
    if ((rc = plan_schur_tasks(B, err)) != SWF_OK) return rc;
    plan_frame_sums(B);
    if ((rc = plan_jt_records(B, err)) != SWF_OK) return rc;
    plan_prior_maps(B);
    std::vector<int> pd, po;                              // the pairs the assembly visits: indices into B.pair
    plan_pair_clique_classes(B, pd, po);
    if ((rc = plan_asm_programs(B, pd, po, err)) != SWF_OK) return rc;
    B.C_init.resize((size_t)B.C_tot, 0.0); B.dgraw_init.resize((size_t)B.v_tot, 0.0);
    if ((rc = plan_composite(B, err)) != SWF_OK) return rc;
    B.want_Linv = B.max_red > B.rr_nmax && B.max_red <= CB_NMAX;
    // few windows, one of them on the streamed Cholesky: the factorisation is spread over the chip, two tile columns per launch (k_chol_col)
    B.want_Wk = B.max_red > B.rr_nmax && B.max_red <= CC_NMAX && n * 4 <= B.n_cu && !sh.no_chol_col;      // >= 4 workgroups per window
    return SWF_OK;
}

// ------------------------------------------------------------------ validation
// Every check recomputes from the plan's primary data (the window records, the landmark / observation / clique / pair arrays) what a
// derived table must say.  NEED(condition, table, index): the first table that disagrees, and where.
int plan_validate(const Plan& B, std::string& err) {
#define NEED(cond, table, i) do { if (!(cond)) { err = std::string("plan_validate: ") + (table) + " [" + std::to_string((long long)(i)) + "]: " #cond; return SWF_E_INVALID; } } while (0)
    auto in = [](long long v, long long lo, long long hi) { return v >= lo && v < hi; };      // lo <= v < hi
    const int n = B.n_win;
    const long long n_gf = (long long)B.gf.size(), n_cl = (long long)B.cl.size(), n_slot = (long long)B.s_x.size();
    NEED((int)B.win.size() == n && (int)B.asw.size() == n && (int)B.s_tnz.size() == 4 * n, "win", n);
    NEED((int)B.lm_obs0.size() == B.n_lm + 1 && (int)B.lm_fmask.size() == B.n_lm && (int)B.fr_obs0.size() == B.n_fr + 1, "lm_obs0", B.n_lm);
    NEED((int)B.sch_c0.size() == n * GEMM_SPLIT + 1, "sch_c0", B.sch_c0.size());
    // ---- observations, landmarks, frames, frame-sum blocks
    for (int q = 0; q < B.n_proj; q++) {
        NEED(in(B.p_win[q], 0, n), "p_win", q);
        const WinRec& W = B.win[B.p_win[q]];
        NEED(in(q, W.proj0, W.proj1) && in(B.p_xpose[q], 0, B.n_x) && in(B.p_xex[q], 0, B.n_x) && in(B.p_xlm[q], 0, B.n_x), "p_x*", q);
        NEED(in(B.p_lpose[q], -1, B.n_loc) && in(B.p_llm[q], -1, B.n_loc) && in(B.p_fr[q], -1, W.nF) && in(B.p_lm[q], W.lm0, W.lm1), "p_l*", q);
        NEED(in(q, B.lm_obs0[B.p_lm[q]], B.lm_obs0[B.p_lm[q] + 1]), "lm_obs0", B.p_lm[q]);
    }
    for (int l = 0; l < B.n_lm; l++) NEED(B.lm_obs0[l] <= B.lm_obs0[l + 1] && in(B.lm_obs0[l], 0, B.n_proj + 1) && in(B.lm_loc[l], -1, B.n_loc) && in(B.lm_win[l], 0, n), "lm_obs0", l);
    for (int f = 0; f < B.n_fr; f++) for (int o = B.fr_obs0[f]; o < B.fr_obs0[f + 1]; o++) NEED(in(o, 0, (long long)B.fr_obs.size()) && in(B.fr_obs[o], 0, B.n_proj), "fr_obs", o);
    for (int k = 0; k < B.n_fsb; k++) {
        const int* r = &B.fsb_rec[(size_t)8 * k];
        NEED(in(r[0], 0, n), "fsb_rec", k);
        const WinRec& W = B.win[r[0]];
        NEED(in(k, W.fsb0, W.fsb1) && r[1] >= W.proj0 && r[2] >= 1 && r[2] <= FS_BLK && r[1] + r[2] <= W.proj1 && r[5] == W.nF, "fsb_rec", k);
        NEED(r[3] >= 0 && r[3] + W.nF + 1 <= (long long)B.fsb_foff.size() && r[4] >= 0 && r[4] + W.nF <= B.fs_tot, "fsb_rec", k);
        std::vector<char> hit((size_t)r[2], 0);
        for (int t = 0; t < r[2]; t++) { const int p = B.fsb_perm[(size_t)r[1] + t]; NEED(in(p, 0, r[2]) && !hit[p], "fsb_perm", r[1] + t); hit[p] = 1; }
        for (int f = 0; f <= W.nF; f++) NEED(in(B.fsb_foff[(size_t)r[3] + f], 0, r[2] + 1), "fsb_foff", r[3] + f);
    }
    // ---- generic factors, J v records, priors and their chunks
    for (long long f = 0; f < n_gf; f++) {
        const GFac& G = B.gf[f];
        NEED(in(G.win, 0, n) && G.nslot >= 0 && G.slot0 >= 0 && G.slot0 + G.nslot <= n_slot && G.roff >= 0 && G.roff + G.nres <= B.r_tot && in(G.clique, -1, n_cl), "gf", f);
        for (int t = G.slot0; t < G.slot0 + G.nslot; t++) {
            NEED(in(B.s_x[t], 0, B.n_x) && in(B.s_loc[t], -1, B.n_loc) && B.s_loc[t] + B.s_ls[t] <= B.n_loc, "s_loc", t);
            NEED(B.s_joff[t] == -1 || (B.s_joff[t] >= 0 && B.s_joff[t] + (long long)(B.s_ls[t] - 1) * G.jld + G.nres <= B.j_tot), "s_joff", t);
        }
    }
    for (int pass = 0; pass < 2; pass++) {
        const std::vector<JtRec>& jt = pass ? B.imu_jt : B.sc_jt; const std::vector<int>& list = pass ? B.imu_gf : B.sc_gf;
        NEED(jt.size() == list.size(), pass ? "imu_jt" : "sc_jt", jt.size());
        for (size_t q = 0; q < jt.size(); q++) {
            const JtRec& r = jt[q];
            NEED(in(r.f, 0, n_gf) && r.f == list[q] && in(r.win, 0, n) && r.roff >= 0 && r.roff + r.nres <= B.r_tot && in(r.nslot, 0, JT_MAXSLOT + 1), pass ? "imu_jt" : "sc_jt", q);
            for (int t = 0; t < JT_MAXSLOT; t++)
                NEED(r.loc[t] >= -1 && r.loc[t] + r.ls[t] <= B.n_loc && (r.joff[t] == -1 || (r.loc[t] >= 0 && r.joff[t] >= 0 && r.joff[t] + (long long)(r.ls[t] - 1) * r.jld + r.nres <= B.j_tot)) && (t < r.nslot || r.joff[t] == -1), pass ? "imu_jt" : "sc_jt", q);
        }
    }
    // the IMU evaluation records: every field against the factor it copies, and against its array with the FULL extent a lane of
    // d_eval_imu touches whether the window's gate is open or not (15 residual rows, the whole pre-integration record, 7 / 9 state
    // values per slot, 6 / 9 Jacobian columns of 15 rows per slot)
    NEED(B.imu_rec.size() == B.imu_gf.size() && B.imu_pre.size() % SWF_PRE_DOUBLES == 0, "imu_rec", B.imu_rec.size());
    for (size_t q = 0; q < B.imu_rec.size(); q++) {
        const ImuRec& r = B.imu_rec[q];
        NEED(in(r.f, 0, n_gf) && r.f == B.imu_gf[q], "imu_rec", q);
        const GFac& G = B.gf[r.f];
        NEED(G.type == GF_IMU && G.nslot == 4 && G.nres == 15 && r.win == G.win && in(r.win, 0, n) && r.roff == G.roff && r.roff >= 0 && (long long)r.roff + 15 <= B.r_tot, "imu_rec", q);
        NEED(r.data == G.data && r.data >= 0 && ((long long)r.data + 1) * SWF_PRE_DOUBLES <= (long long)B.imu_pre.size() && r.jld == G.jld && r.jld >= 0, "imu_rec", q);
        for (int t = 0; t < 4; t++) {
            const long long gs = (t & 1) ? 9 : 7, ls = (t & 1) ? 9 : 6;
            NEED(r.xo[t] == B.s_x[(size_t)G.slot0 + t] && r.xo[t] >= 0 && r.xo[t] + gs <= B.n_x, "imu_rec", q);
            NEED(r.joff[t] == B.s_joff[(size_t)G.slot0 + t] && (r.joff[t] == -1 || (r.joff[t] >= 0 && r.joff[t] + (ls - 1) * r.jld + 15 <= B.j_tot)), "imu_rec", q);
        }
    }
    {
        int ch = 0;                                           // the chunks partition each prior's rows, prior after prior
        std::vector<int> w_first(n, -1), w_end(n, 0);
        for (size_t q = 0; q < B.prior_gf.size(); q++) {
            NEED(in(B.prior_gf[q], 0, n_gf), "prior_gf", q);
            const GFac& G = B.gf[B.prior_gf[q]];
            NEED(G.type == GF_PRIOR && in(G.data, 0, (long long)B.prior_dim.size()) && B.prior_dim[G.data] == G.nres, "prior_gf", q);
            const long long dim = G.nres;
            NEED(B.prior_Joff[G.data] >= 0 && B.prior_Joff[G.data] + dim * dim <= (long long)B.prior_J.size() && B.prior_Jt.size() == B.prior_J.size(), "prior_Joff", G.data);
            NEED(B.prior_roff[G.data] >= 0 && B.prior_roff[G.data] + dim <= (long long)B.prior_r0.size() && B.prior_x0off[G.data] >= 0, "prior_roff", G.data);
            const int nch = B.prior_nch[q];
            NEED(nch >= 1 && (dim > PRIOR_SPLIT_DIM ? (long long)nch * PRIOR_CHUNK >= dim && (long long)(nch - 1) * PRIOR_CHUNK < dim : nch == 1), "prior_nch", q);
            for (int c = 0; c < nch; c++, ch++) NEED(ch < B.n_pch && B.pch_q[ch] == (int)q && B.pch_r0[ch] == (nch > 1 ? c * PRIOR_CHUNK : 0), "pch_q", ch);
            if (w_first[G.win] < 0) w_first[G.win] = ch - nch;
            w_end[G.win] = ch;
        }
        NEED(ch == B.n_pch, "pch_q", ch);
        for (int w = 0; w < n; w++) NEED(w_first[w] < 0 ? B.win[w].pch0 == B.win[w].pch1 : (B.win[w].pch0 == w_first[w] && B.win[w].pch1 == w_end[w]), "win.pch", w);
    }
    // ---- parameter blocks: blk_* against the window's ranges, loc2x / x_var recomputed from them; lm_col a permutation of the window's landmarks
    NEED((long long)B.loc2x.size() >= std::max<long long>(B.n_loc, 1) && (long long)B.x_var.size() == B.n_x && B.blk_xoff.size() == B.blk_loc.size() && B.blk_xoff.size() == B.blk_gs.size(), "loc2x", B.loc2x.size());
    for (int w = 0; w < n; w++) {
        const WinRec& W = B.win[w];
        NEED(W.blk_base >= 0 && W.n_blk >= 0 && W.blk_base + W.n_blk <= (long long)B.blk_xoff.size() && W.x_base >= 0 && W.x_base + W.x_n <= B.n_x && W.loc_base >= 0 && W.loc_base + W.n_loc <= B.n_loc, "win.blk", w);
        int xo = W.x_base; long long nvar = 0;
        for (int b = W.blk_base; b < W.blk_base + W.n_blk; b++) {
            const int gs = B.blk_gs[b], ls = gs == 7 ? 6 : gs, lo = B.blk_loc[b];
            NEED((gs == 7 || gs == 9 || gs == 3 || gs == 1) && B.blk_xoff[b] == xo && xo + gs <= W.x_base + W.x_n, "blk_xoff", b);
            NEED(lo == -1 || (lo >= W.loc_base && lo + ls <= W.loc_base + W.n_loc), "blk_loc", b);
            for (int k = 0; k < gs; k++) NEED(B.x_var[(size_t)xo + k] == (lo >= 0 ? 1 : 0), "x_var", xo + k);
            if (lo >= 0) { nvar += ls; for (int k = 0; k < ls; k++) NEED(B.loc2x[(size_t)lo + k] == (gs == 7 ? -1 : xo + k), "loc2x", lo + k); }
            xo += gs;
        }
        NEED(xo == W.x_base + W.x_n && nvar == W.n_loc, "blk_gs: the blocks do not fill the window", w);
        std::vector<char> hit((size_t)(W.lm1 - W.lm0), 0);
        for (int l = W.lm0; l < W.lm1; l++) { const int c = B.lm_col[l]; NEED(c >= 0 && c % 3 == 0 && c / 3 < W.lm1 - W.lm0 && !hit[c / 3], "lm_col", l); hit[c / 3] = 1; }
    }
    // ---- factor slots: the clique column of every slot; the prior records' column maps recomputed from their slots
    NEED(B.prior_colloc.size() == B.prior_r0.size() && B.prior_colcc.size() == B.prior_r0.size() && (long long)B.s_pcol.size() == n_slot && (long long)B.s_pxo.size() == n_slot && (long long)B.s_ccol.size() == n_slot, "prior_colloc", B.prior_colloc.size());
    for (long long f = 0; f < n_gf; f++) {
        const GFac& G = B.gf[f];
        const long long d = G.clique >= 0 ? B.cl[G.clique].d_e + B.cl[G.clique].d_f : 0;
        for (int t = G.slot0; t < G.slot0 + G.nslot; t++) NEED(B.s_ccol[t] == -1 || (B.s_ccol[t] >= 0 && B.s_ccol[t] + B.s_ls[t] <= d), "s_ccol", t);
        if (G.type != GF_PRIOR) continue;
        NEED(in(G.data, 0, (long long)B.prior_dim.size()), "gf.data", f);
        const long long roff = B.prior_roff[G.data], x0o = B.prior_x0off[G.data];
        const long long gsum = ((size_t)G.data + 1 < B.prior_x0off.size() ? B.prior_x0off[G.data + 1] : (long long)B.prior_x0.size()) - x0o;
        int col = 0, xo = 0;
        for (int t = G.slot0; t < G.slot0 + G.nslot; t++) {
            const int l = B.s_ls[t];
            NEED(B.s_pcol[t] == col && col + l <= G.nres && B.s_pxo[t] == xo && xo + (l == 6 ? 7 : l) <= gsum, "s_pcol", t);
            for (int q = 0; q < l; q++) {
                NEED(B.prior_colloc[(size_t)roff + col + q] == (B.s_loc[t] >= 0 ? B.s_loc[t] + q : -1), "prior_colloc", roff + col + q);
                NEED(B.prior_colcc[(size_t)roff + col + q] == (B.s_ccol[t] >= 0 ? B.s_ccol[t] + q : -1), "prior_colcc", roff + col + q);
            }
            col += l; xo += l == 6 ? 7 : l;
        }
        NEED(col == G.nres && xo == gsum, "s_pcol: the slots do not fill the prior", f);
    }
    {   // ---- cle_rec: the cliques with an eliminated block, copied in clique order
        size_t k = 0;
        for (const Clique& C : B.cl) if (C.d_e > 0) { NEED(k < B.cle_rec.size() && !memcmp(&B.cle_rec[k], &C, sizeof(Clique)), "cle_rec", k); k++; }
        NEED((int)k == B.n_cle && k == B.cle_rec.size(), "cle_rec", k);
    }
    // ---- composite factors: every offset table against the array it addresses
    if (const int nc = B.n_comp) {
        NEED((int)B.co_M.size() == nc && (int)B.co_N.size() == nc && (int)B.co_gf.size() == nc && (int)B.co_win.size() == nc && (int)B.co_mid.size() == nc && (int)B.co_xo_off.size() == nc + 1, "co_M", nc);
        NEED((int)B.co_eo.size() == nc + 1 && (int)B.co_no.size() == nc + 1 && (int)B.co_pno.size() == nc + 1 && (int)B.co_nno.size() == nc + 1 && (int)B.co_go.size() == nc + 1 && (int)B.co_g2o.size() == nc + 1, "co_eo", nc);
        NEED((int)B.co_Joff.size() == nc && (int)B.co_roff.size() == nc && (int)B.co_x0off.size() == nc && (int)B.co_Coff.size() == nc && (int)B.co_voff.size() == nc, "co_Joff", nc);
        NEED(B.co_eo[0] == 0 && B.co_no[0] == 0 && B.co_pno[0] == 0 && B.co_nno[0] == 0 && B.co_go[0] == 0 && B.co_g2o[0] == 0 && B.co_xo_off[0] == 0, "co_eo", 0);
        size_t iq = 0;
        for (int f = 0; f < nc; f++) {
            const long long M = B.co_M[f], N = B.co_N[f], G = 30 + N;
            NEED(M >= 1 && N >= 0 && N <= CO_MAXN && in(B.co_win[f], 0, n) && in(B.co_mid[f], 0, M) && in(B.co_gf[f], 0, n_gf) && B.gf[B.co_gf[f]].type == GF_PRIOR && B.gf[B.co_gf[f]].nres == G, "co_M", f);
            NEED(B.co_eo[f + 1] == B.co_eo[f] + M && B.co_no[f + 1] == B.co_no[f] + N && B.co_pno[f + 1] == B.co_pno[f] + 15 * M * N && B.co_nno[f + 1] == B.co_nno[f] + N * N, "co_eo", f + 1);
            NEED(B.co_go[f + 1] == B.co_go[f] + G && B.co_g2o[f + 1] == B.co_g2o[f] + G * G && B.co_xo_off[f + 1] == B.co_xo_off[f] + 4 + N && B.co_xo_off[f + 1] <= (long long)B.co_xo.size(), "co_go", f + 1);
            for (int q = B.co_xo_off[f]; q < B.co_xo_off[f + 1]; q++) NEED(in(B.co_xo[q], B.win[B.co_win[f]].x_base, (long long)B.win[B.co_win[f]].x_base + B.win[B.co_win[f]].x_n), "co_xo", q);
            NEED(B.co_Joff[f] >= 0 && B.co_Joff[f] + G * G <= (long long)B.prior_J.size() && B.co_roff[f] >= 0 && B.co_roff[f] + G <= (long long)B.prior_r0.size() && B.co_x0off[f] >= 0 && B.co_x0off[f] + 32 + N <= (long long)B.prior_x0.size(), "co_Joff", f);
            NEED((B.co_Coff[f] == -1 && B.co_voff[f] == -1) || (B.co_Coff[f] >= 0 && B.co_Coff[f] + G * G <= B.C_tot && B.co_voff[f] >= 0 && B.co_voff[f] + G <= B.v_tot), "co_Coff", f);
            for (int k = 0; k <= M; k++, iq++) NEED(iq < B.co_iq_f.size() && iq < B.co_iq_k.size() && B.co_iq_f[iq] == f && B.co_iq_k[iq] == k, "co_iq_f", iq);
        }
        const size_t ne = (size_t)B.co_eo[nc];
        NEED(iq == B.co_iq_f.size() && (long long)ne == B.comp_ne && B.co_pose.size() == ne * 7 && B.co_sb.size() == ne * 9 && B.co_pose_lin.size() == ne * 7 && B.co_sb_lin.size() == ne * 9, "co_pose", ne);
        NEED(B.co_Hpp.size() == ne * 225 && B.co_rhs_p.size() == ne * 15 && (long long)B.co_HpN.size() == B.co_pno[nc] && (long long)B.co_HNN.size() == B.co_nno[nc] && (long long)B.co_rhsN.size() == B.co_no[nc], "co_Hpp", ne);
        NEED(B.co_pre.size() == (ne + nc) * SWF_PRE_DOUBLES && B.co_H12.size() == (size_t)nc * 225 && B.co_pbgw.size() == (size_t)nc * 6 && (int)B.co_xo.size() == B.co_xo_off[nc], "co_pre", ne);
    }
    // ---- cliques: ranges, and every non-static one in exactly one class whose kernel instance holds it
    std::map<std::array<long long, 3>, int> cl_seen;                // (fac0, mem0, e_off) names a clique
    for (long long c = 0; c < n_cl; c++) {
        const Clique& C = B.cl[c]; const long long d = C.d_e + C.d_f;
        NEED(in(C.win, 0, n) && in(c, B.win[C.win].cl0, B.win[C.win].cl1) && C.fac0 >= 0 && C.fac0 <= C.fac1 && C.fac1 <= (long long)B.cl_fac.size() && C.mem0 >= 0 && C.mem0 <= C.mem1 && C.mem1 <= (long long)B.cm_loc.size(), "cl", c);
        NEED(in(C.e_loc, -1, B.n_loc) && C.C_off >= 0 && C.C_off + (long long)C.d_f * C.d_f <= B.C_tot && C.v_off >= 0 && C.v_off + C.d_f <= B.v_tot && C.e_off >= 0 && C.e_off + C.d_e * d + C.d_e <= B.e_tot, "cl", c);
        NEED(C.r_off >= 0 && C.r_off + C.n_rows <= B.r_tot && (C.is_static || (C.j_off >= 0 && C.j_off + C.n_rows * d <= B.j_tot)), "cl", c);
        for (int q = C.fac0; q < C.fac1; q++) NEED(in(B.cl_fac[q], 0, n_gf) && in(B.cl_frow[q], 0, C.n_rows + 1), "cl_fac", q);
        for (int m = C.mem0; m < C.mem1; m++) {
            NEED(B.cm_loc[m] >= 0 && B.cm_loc[m] + B.cm_ls[m] <= B.n_loc && B.cm_col[m] >= 0 && B.cm_col[m] + B.cm_ls[m] <= C.d_f, "cm_loc", m);
            for (int q = 0; q < B.cm_ls[m]; q++) NEED(B.cv_loc[(size_t)C.v_off + B.cm_col[m] + q] == B.cm_loc[m] + q, "cv_loc", C.v_off + B.cm_col[m] + q);
        }
        if (!C.is_static) cl_seen[{ C.fac0, C.mem0, C.e_off }] = 0;
    }
    for (int k = 0; k < 5; k++) {
        NEED((int)B.clc_rec[k].size() == B.n_clc[k], "clc_rec", k);
        for (const Clique& C : B.clc_rec[k]) {
            const long long d = C.d_e + C.d_f; const int R = C.n_rows;
            auto it = cl_seen.find({ C.fac0, C.mem0, C.e_off });
            NEED(it != cl_seen.end() && it->second++ == 0, "clc_rec", k);
            // the instance class k launches: d_clique_elim<rows, columns> of 48 x 32, 32 x 48, 64 x 64, (4) 96 x 64; (3) k_clique_big
            NEED(k == 0 ? (C.d_e <= 1 && d <= 32 && R <= 48) : k == 1 ? (R <= 32 && d <= 48) : k == 2 ? (R <= CLQ_MAXR && d <= CLQ_MAXD) : k == 4 ? (R <= CLQ_TALLR && d <= 64)
                        : (d <= CB_MAXD && C.d_e <= 9 && (long long)C.d_e * d <= CB_MAXED), "clc_rec", k);
        }
    }
    for (auto& kv : cl_seen) NEED(kv.second == 1, "clc_rec: a clique in no class, fac0", kv.first[0]);
    // k_clique_pack's LDS: every class-0 clique inside clp_rows x clp_ld (two pad columns behind its d), the leading dimension odd, the envelope not exceeded
    NEED(B.clp_rows >= 1 && B.clp_rows <= 48 && B.clp_ld >= 3 && B.clp_ld <= 35 && (B.clp_ld & 1) == 1, "clp_rows", B.clp_rows);
    {
        int mr = 1, ml = 3;
        for (const Clique& C : B.clc_rec[0]) {
            NEED(C.n_rows <= B.clp_rows && C.d_e + C.d_f + 2 <= B.clp_ld, "clp_ld", &C - B.clc_rec[0].data());
            mr = std::max(mr, C.n_rows); ml = std::max(ml, (C.d_e + C.d_f + 2) | 1);
        }
        NEED(mr == B.clp_rows && ml == B.clp_ld, "clp_rows: not the largest class-0 clique", mr);
    }
    // ---- per window: back-substitution blocks, the k_lm_schur task table and its masks, pairs, the assembly program, s_tnz
    const int TW = B.ls_var <= 1 ? 2 : 1, NCW = ls_ncw(B.ls_var), TPW = ls_tpw(B.ls_var);
    NEED((long long)B.sch_rec.size() >= ((long long)B.sch_c0.back() + 4 * LS_NB) * 32 && (long long)B.sch_km.size() >= ((long long)B.sch_c0.back() / TW + 2) * B.ls_kms, "sch_rec", B.sch_rec.size());
    std::vector<std::vector<const Pair*>> wpair((size_t)n);
    // every field of a pair record the kernels read, against the pair's window: the batch's pairs and the two uploaded lists alike
    auto pair_ok = [&](const Pair& P) {
        if (!in(P.win, 0, n)) return false;
        const WinRec& W = B.win[P.win];
        return P.ra >= 0 && P.la >= 1 && P.ra + P.la <= W.n_red && P.rb >= 0 && P.lb >= 1 && P.rb + P.lb <= W.n_red && P.rb <= P.ra && in(P.fa, -1, W.nF) && in(P.fb, -1, W.nF)
            && P.c0 >= 0 && P.c0 <= P.c1 && P.c1 <= (long long)B.pc_coff.size() && (P.is_diag ? (P.ra == P.rb && P.la == P.lb) : P.ra != P.rb) && P.loc_a == W.loc_base + W.n_e + P.ra
            && P.fsb0 == W.fsb0 && P.fsb1 == W.fsb1 && P.n == W.n_red && P.m == 6 * W.nF && P.S_base == W.S_base && P.P_base == W.P_base && P.q_base == 6LL * W.fr_base * GEMM_SPLIT;
    };
    NEED((int)B.pair_d.size() == B.n_pd && (int)B.pair_o.size() == B.n_po, "pair_d", B.pair_d.size());
    for (const Pair& P : B.pair) NEED(pair_ok(P), "pair", &P - B.pair.data());
    for (const Pair& P : B.pair_d) { NEED(pair_ok(P) && P.is_diag, "pair_d", &P - B.pair_d.data()); wpair[P.win].push_back(&P); }
    for (const Pair& P : B.pair_o) { NEED(pair_ok(P) && !P.is_diag, "pair_o", &P - B.pair_o.data()); wpair[P.win].push_back(&P); }
    std::map<std::array<int, 4>, std::vector<int>> programs;        // (se0, ne, ve0, nv) -> its serialised content
    for (int w = 0; w < n; w++) {
        const WinRec& W = B.win[w];
        NEED(W.n_e + W.n_red == W.n_loc && W.loc_base >= 0 && W.loc_base + W.n_loc <= B.n_loc && W.x_base >= 0 && W.x_base + W.x_n <= B.n_x, "win", w);
        NEED(W.S_base >= 0 && W.S_base + (long long)(W.n_red + 1) * W.n_red <= B.S_tot && W.Lt_base + (long long)(W.n_red + 1) * (W.n_red + 1) <= B.Lt_tot && W.P_base + 36LL * W.nF * W.nF <= B.P_tot, "win", w);
        NEED(W.fr_base >= 0 && W.fr_base + W.nF <= B.n_fr && W.nF <= LS_MAXF && W.lm0 <= W.lm1 && W.lm1 <= B.n_lm, "win", w);
        for (int f = 0; f < W.nF; f++) NEED(B.fr_red[W.fr_base + f] >= 0 && B.fr_red[W.fr_base + f] + 6 <= W.n_red, "fr_red", W.fr_base + f);
        {   // the blocks partition the window's landmarks and observations
            int l = W.lm0;
            for (int k = W.lmb0; k < W.lmb1; k++) {
                const int* r = &B.lmb_rec[(size_t)4 * k];
                NEED(k < B.n_lmb && r[2] == l && r[3] >= 1 && r[3] <= 256 && l + r[3] <= W.lm1 && r[0] == B.lm_obs0[l] && r[1] == B.lm_obs0[l + r[3]] - r[0] && r[1] <= 256, "lmb_rec", k);
                l += r[3];
            }
            NEED(l == W.lm1, "lmb_rec", W.lmb1);
        }
        {   // tasks: the parts ascend and start on even tasks; every variable fast-path landmark in exactly one (task, group)
            const int* c0 = &B.sch_c0[(size_t)w * GEMM_SPLIT];
            const int t0 = c0[0], t1 = c0[GEMM_SPLIT], m = 6 * W.nF, nt = (m + 15) / 16;
            for (int sp = 0; sp < GEMM_SPLIT; sp++) NEED(c0[sp] >= 0 && c0[sp] <= c0[sp + 1] && (c0[sp] & 1) == 0, "sch_c0", w * GEMM_SPLIT + sp);
            NEED(((t1 - t0) & 1) == 0 && (w > 0 || t0 == 0), "sch_c0", w * GEMM_SPLIT);
            std::vector<int> times((size_t)(W.lm1 - W.lm0), 0);
            for (int t = t0; t < t1; t++) for (int g = 0; g < 4; g++) {
                const int* r = &B.sch_rec[((size_t)t * 4 + g) * 8]; const int L = r[0];
                if (L == -1) continue;
                NEED(in(L, W.lm0, W.lm1) && B.lm_loc[L] >= 0 && r[1] == B.lm_loc[L] && r[2] == B.lm_obs0[L] && r[3] == B.lm_obs0[L + 1] && r[3] - r[2] <= 64 && r[4] == 3 * g, "sch_rec", ((size_t)t * 4 + g) * 8);
                times[L - W.lm0]++;
                // the k-steps that carry the landmark's columns, at every tile its frames touch (from lm_fmask)
                unsigned rows = 0;
                for (int f = 0; f < W.nF && f < 64; f++) if ((B.lm_fmask[L] >> f) & 1ULL) { rows |= 1u << ((6 * f) / 16); rows |= 1u << ((6 * f + 5) / 16); }
                const unsigned ks = g == 0 ? 1u : g == 1 ? 3u : g == 2 ? 6u : 4u;
                for (int tr = 0; tr < nt; tr++) for (int tc = 0; tc <= tr; tc++) {
                    if (!((rows >> tr) & 1u) || !((rows >> tc) & 1u)) continue;
                    const int e = tr == tc ? tr : nt + tr * (tr - 1) / 2 + tc, lp = e / (NCW * TPW), rr = e % (NCW * TPW), sl = rr / NCW, cw = rr % NCW;
                    const size_t word = (size_t)(t / TW) * B.ls_kms + (size_t)(lp * NCW + cw);
                    NEED(lp * NCW + cw < B.ls_kms && (((unsigned)B.sch_km[word] >> (3 * TW * sl + 3 * (t % TW))) & ks) == ks, "sch_km", word);
                }
            }
            for (int l = W.lm0; l < W.lm1; l++) NEED(times[l - W.lm0] == (B.lm_loc[l] >= 0 ? 1 : 0), "sch_rec: landmark", l);
        }
        // pairs of the assembly's lists; s_tnz holds the tiles of EVERY pair (those s_direct dropped too)
        for (int p = W.pair0; p < W.pair1; p++) {
            const Pair& P = B.pair[p];
            NEED(P.win == w, "pair", p);
            for (int c = P.c0; c < P.c1; c++) NEED(B.pc_coff[c] >= 0 && B.pc_coff[c] + (long long)(P.la - 1) * B.pc_cld[c] + P.lb <= B.C_tot && B.pc_voff[c] >= 0 && B.pc_voff[c] + P.la <= B.v_tot, "pc_coff", c);
            if (W.n_red > 256) continue;
            for (int I = P.ra / 16; I <= (P.ra + P.la - 1) / 16; I++) for (int J = P.rb / 16; J <= (P.rb + P.lb - 1) / 16 && J < I; J++) {
                const int t = I * (I - 1) / 2 + J;
                NEED((B.s_tnz[(size_t)w * 4 + (t >> 5)] >> (t & 31)) & 1u, "s_tnz", w * 4 + (t >> 5));
            }
        }
        // the assembly program: every source inside its array, no entry of S written twice, every pair of the lists present
        const AsmWin& A = B.asw[w];
        const long long nS = (long long)B.as_dst.size(), nV = (long long)B.av_loc.size(), mm = A.m;
        NEED(A.win == w && A.n_red == W.n_red && A.m == 6 * W.nF && A.se0 >= 0 && A.se0 + A.ne <= nS && A.ve0 >= 0 && A.ve0 + A.nv <= nV && A.ne <= B.as_max_ne && A.nv <= B.as_max_nv, "asw", w);
        NEED(A.S_base == W.S_base && A.C_base >= 0 && A.v_base >= 0 && A.fs_base >= 0 && A.P_base == W.P_base * GEMM_SPLIT && A.q_base == 6LL * W.fr_base * GEMM_SPLIT && A.loc_base == W.loc_base, "asw", w);
        const long long fs_n = (B.fs_tot - A.fs_base) * FS_VAL, P_n = B.P_tot * GEMM_SPLIT - A.P_base, q_n = (long long)std::max(1, 6 * B.n_fr) * GEMM_SPLIT - A.q_base;
        std::vector<char> written((size_t)W.n_red * W.n_red, 0);
        for (int k = A.se0; k < A.se0 + A.ne; k++) {
            const unsigned cnt = B.as_cnt[k]; const int nC = AS_NC(cnt), nP = AS_NP(cnt), nH = AS_NH(cnt), s0 = B.as_src0[k], dst = B.as_dst[k];
            NEED(in(dst, 0, (long long)W.n_red * W.n_red) && dst % W.n_red <= dst / W.n_red && !written[dst], "as_dst", k);
            written[dst] = 1;
            NEED(s0 >= 0 && s0 + nC + nP + nH + (AS_DIAG(cnt) ? nC : 0) <= (long long)B.as_src.size() && in(B.as_aux[k], 0, W.n_loc) && (!AS_SOLD(cnt) || B.s_direct), "as_src0", k);
            const int* s = &B.as_src[s0];
            for (int c = 0; c < nC; c++) NEED(in(A.C_base + s[c], 0, B.C_tot), "as_src", s0 + c);
            for (int c = nC; c < nC + nP; c++) NEED(in(s[c], 0, P_n) && s[c] < GEMM_SPLIT * mm * mm, "as_src", s0 + c);
            for (int c = nC + nP; c < nC + nP + nH; c++) NEED(in(s[c], 0, fs_n), "as_src", s0 + c);
            if (AS_DIAG(cnt)) for (int c = nC + nP + nH; c < 2 * nC + nP + nH; c++) NEED(in(A.v_base + s[c], 0, B.v_tot), "as_src", s0 + c);
        }
        for (int k = A.ve0; k < A.ve0 + A.nv; k++) {
            const unsigned cnt = B.av_cnt[k]; const int nC = AS_NC(cnt), nQ = AS_NP(cnt), nH = AS_NH(cnt), s0 = B.av_src0[k];
            NEED(in(B.av_loc[k], 0, W.n_loc) && in(B.av_red[k], 0, W.n_red) && in(B.av_i[k], 0, 6) && s0 >= 0 && s0 + nH + nC + nQ <= (long long)B.av_src.size(), "av_src0", k);
            const int* s = &B.av_src[s0];
            for (int c = 0; c < nH; c++) NEED(s[c] >= 0 && s[c] + FS_VAL <= fs_n, "av_src", s0 + c);
            for (int c = nH; c < nH + nC; c++) NEED(in(A.v_base + s[c], 0, B.v_tot), "av_src", s0 + c);
            for (int c = nH + nC; c < nH + nC + nQ; c++) NEED(in(s[c], 0, q_n), "av_src", s0 + c);
        }
        for (const Pair* P : wpair[w]) for (int i = 0; i < P->la; i++) for (int j = 0; j < (P->is_diag ? i + 1 : P->lb); j++)
            NEED(P->ra + i < W.n_red && P->rb + j < W.n_red && written[(size_t)(P->ra + i) * W.n_red + P->rb + j], "as_dst: an entry of pair_d / pair_o is missing, window", w);
        // programs are shared exactly when they are equal: windows of one structure have one
        std::vector<int>& key = programs[{ A.se0, A.ne, A.ve0, A.nv }];
        if (key.empty()) {
            key.push_back(A.ne);
            for (int k = A.se0; k < A.se0 + A.ne; k++) {
                const unsigned cnt = B.as_cnt[k]; const int len = AS_NC(cnt) * (AS_DIAG(cnt) ? 2 : 1) + AS_NP(cnt) + AS_NH(cnt);
                key.push_back(B.as_dst[k]); key.push_back((int)cnt); key.push_back(B.as_aux[k]);
                key.insert(key.end(), &B.as_src[B.as_src0[k]], &B.as_src[B.as_src0[k]] + len);
            }
            for (int k = A.ve0; k < A.ve0 + A.nv; k++) {
                const unsigned cnt = B.av_cnt[k]; const int len = AS_NC(cnt) + AS_NP(cnt) + AS_NH(cnt);
                key.push_back(B.av_loc[k]); key.push_back(B.av_red[k]); key.push_back((int)cnt); key.push_back(B.av_i[k]);
                key.insert(key.end(), &B.av_src[B.av_src0[k]], &B.av_src[B.av_src0[k]] + len);
            }
        }
    }
    NEED((int)programs.size() == B.asm_programs, "asw: programs", programs.size());
    for (auto a = programs.begin(); a != programs.end(); ++a) for (auto b = std::next(a); b != programs.end(); ++b)
        NEED(a->second != b->second, "asw: two copies of one program, se0", b->first[0]);
    return SWF_OK;
#undef NEED
}
