// =========================================================================================
// Speed-bias cliques (class 1) of the batch path with J^T J and the C update on the matrix cores.
//
// k_clique_mm<32, 48, 9> is k_clique_elim<32, 48, 9, 1> (full form, one wavefront per clique, the same records and outputs) with its
// two products taken off the VALU:
//   M = Jc^T Jc      lower triangle in up to six 16x16 accumulator tiles, one v_mfma_f64_16x16x4_f64 per tile and group of four rows;
//                    diag(M), M_e* (tile column 0) and M_ff all come out of these tiles
//   C = M_ff - M_fe T   three more k-steps on the same accumulators with A = -M_fe, B = T (K = MAXE padded to 12 with zero rows)
// g_c = J_c^T r, the Gauss-Jordan inverse, T, Eg, the cE record and cv_cs are the code of d_clique_elim.
//
// BITS.  d_clique_elim forms every element of M as a k-ascending chain m = fma(x_k, y_k, m) from +0 and applies the correction as
// m = fma(-f_a, t_a, m), a ascending.  v_mfma_f64_16x16x4_f64 forms, per output element, fma(a3, b3, fma(a2, b2, fma(a1, b1,
// fma(a0, b0, c)))) over its four k-slots in slot order (measured: tests/test_clique_mfma_gpu.py), so with row
// k0 + kk of Jc in slot kk the accumulator runs through the same chain.  The zero rows that pad n_rows to a multiple of four and MAXE to
// twelve add fma(0, 0, m) = m: m starts at +0 and a round-to-nearest sum chain from +0 never reaches -0, so the padding leaves the
// bits alone.  SWF_NO_CLIQUE_MFMA=1 keeps k_clique_elim<32, 48, 9, 1>; the two give the same bytes (tests/test_clique_mfma_gpu.py).
// =========================================================================================
#pragma once

// slot kk of an MFMA k-step holds row k0 + CMM_SLOT_ROW[kk]: the hardware accumulates its slots in ascending order
__device__ constexpr int CMM_SLOT_ROW[4] = { 0, 1, 2, 3 };

// one v_mfma_f64_16x16x4_f64 on host-given operands (swf_debug_mfma_f64): A 16 x 4, B 4 x 16, C / D 16 x 16, all row-major
__global__ void __launch_bounds__(64) k_debug_mfma_f64(const double* A, const double* Bm, const double* Cm, double* Dm) {
    const int lane = threadIdx.x, i = lane & 15, k = lane >> 4;
    double4_t c;
#pragma unroll
    for (int r = 0; r < 4; r++) c[r] = Cm[(k + 4 * r) * 16 + i];
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(A[i * 4 + k], Bm[k * 16 + i], c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) Dm[(k + 4 * r) * 16 + i] = c[r];
}

template <int MAXR, int MAXD, int MAXE>
__global__ void __launch_bounds__(64) k_clique_mm(DevBatch B, DevOpt O) {
    static_assert(MAXR % 4 == 0 && MAXD == 48 && MAXE <= 16, "k_clique_mm: whole k-steps, three 16-column tiles, the eliminated block inside tile column 0");
    constexpr int LD = MAXD + 1, CLS = 1, PF = 24, KE = (MAXE + 3) / 4;
    // the dense clique Jacobian (rows up to the next multiple of 4 and columns up to MAXD zeroed) is dead once M and g are formed: M_e*,
    // T, Einv and Eg take its place, so a clique holds 12 800 B of LDS (twelve per CU) where k_clique_elim<32,48,9,1> holds 20 440 B (eight)
    __shared__ double lds[MAXR * LD + MAXR];
    static_assert((2 * MAXD + MAXE + 1) * MAXE <= MAXR * LD, "k_clique_mm: Me | T | Ei | Eg inside the Jacobian's storage");
    double (*Jc)[LD] = reinterpret_cast<double (*)[LD]>(lds);
    double* rv = lds + MAXR * LD;
    double (*Me)[MAXD] = reinterpret_cast<double (*)[MAXD]>(lds);                                   // M_e* = J_e^T J
    double (*T)[MAXD] = reinterpret_cast<double (*)[MAXD]>(lds + MAXE * MAXD);                      // Einv M_ef (row 0 stages diag(M) before T exists)
    double (*Ei)[MAXE] = reinterpret_cast<double (*)[MAXE]>(lds + 2 * MAXE * MAXD);                 // Einv
    double* Eg = lds + 2 * MAXE * MAXD + MAXE * MAXE;
    const int cidx_ = (int)blockIdx.x;
#ifdef SWF_PROFILE_CLQ
    unsigned long long tq_ = __builtin_amdgcn_s_memtime();
    if (cidx_ == SWF_PROFILE_CLQ_IDX && threadIdx.x == 0) for (int i = 0; i < 16; i++) g_clq_stamps[i] = 0;
#endif
    if (cidx_ >= B.n_clc[CLS]) return;
    const Clique& C = B.clc_rec[CLS][cidx_];
    WinState& s = B.ws[C.win];
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int de = C.d_e, df = C.d_f, d = de + df, nrow = C.n_rows, nr4 = (nrow + 3) & ~3;
    const int nt = (d + 15) >> 4;                   // tile rows / columns in use (wave-uniform)
    // Gate last (round 11): the window's flags, the residual rows and the first PF values per lane of the Jacobian are requested in one
    // level behind the record; need_lin is tested with them in flight.  Every address is the record's own: row lane < n_rows of g_r at
    // r_off and element e < n_rows * d of g_J at j_off belong to the clique whether its window runs or not (plan_validate, "cl").
    const double* gJ = B.g_J + C.j_off;
    const int tot = nrow * d;
    const int need = s.need_lin;
    const double s_mu = s.mu; const bool s_it0 = s.iter == 0;
    double rl = lane < nrow ? B.g_r[C.r_off + lane] : 0.0;
    double v0[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) { int e = u * 64 + lane; v0[u] = e < tot ? gJ[e] : 0.0; }
    rl = pinned_d(rl);                              // (held in front of the gate: the compiler would sink the loads behind it)
#pragma unroll
    for (int u = 0; u < PF; u++) v0[u] = pinned_d(v0[u]);
    if (!need) return;
    QST(0);
    {
        float rd = 1.0f / (float)nrow;
        if (lane < nrow) rv[lane] = rl;
        // zero rows n_rows .. nr4 - 1 and zero columns d .. MAXD - 1: what the k-steps and the tiles read beyond the clique
        for (int e = lane; e < (nr4 - nrow) * MAXD; e += 64) Jc[nrow + e / MAXD][e % MAXD] = 0.0;
        for (int e = lane; e < nrow * (MAXD - d); e += 64) Jc[e % nrow][d + e / nrow] = 0.0;
        // flat, fully coalesced loads, all issued before the first use (one exposed round trip per PF values)
        for (int base = 0; base < tot; base += PF * 64) {
            double v[PF];
#pragma unroll
            for (int u = 0; u < PF; u++) { int e = base + u * 64 + lane; v[u] = base == 0 ? v0[u] : e < tot ? gJ[e] : 0.0; }      // (the first round came with the flag)
#pragma unroll
            for (int u = 0; u < PF; u++) {
                int e = base + u * 64 + lane;
                int col = (int)((e + 0.5f) * rd);                                    // exact floor(e / nrow) for e < 4096, nrow <= 64
                col += (e - col * nrow >= nrow) ? 1 : 0; col -= (e - col * nrow < 0) ? 1 : 0;   // (belt and braces)
                if (e < tot) Jc[e - col * nrow][col] = v[u];
            }
        }
    }
    __syncthreads();
    QST(1);
    // M = Jc^T Jc, lower triangle of tiles: acc[ti (ti + 1) / 2 + tj] holds rows 16 ti .. and columns 16 tj ..; element
    // (row (lane >> 4) + 4 reg, column lane & 15).  One operand per tile column and k-step serves as A (Jc^T) and as B (Jc).
    double4_t acc[6];
#pragma unroll
    for (int t = 0; t < 6; t++) acc[t] = double4_t{ 0, 0, 0, 0 };
    for (int k0 = 0; k0 < nr4; k0 += 4) {
        const int k = k0 + CMM_SLOT_ROW[lk];
        double x[3];
#pragma unroll
        for (int t = 0; t < 3; t++) x[t] = t < nt ? Jc[k][16 * t + li] : 0.0;
#pragma unroll
        for (int ti = 0; ti < 3; ti++)
#pragma unroll
            for (int tj = 0; tj <= ti; tj++)
                if (ti < nt) acc[ti * (ti + 1) / 2 + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ti], x[tj], acc[ti * (ti + 1) / 2 + tj], 0, 0, 0);
    }
    // lane c < d: gradient entry g_c, k-ascending
    double gc = 0;
    {
        const int c = lane < d ? lane : 0;
#pragma unroll 4
        for (int k = 0; k < nrow; k++) gc += Jc[k][c] * rv[k];
    }
    __syncthreads();                                // (the last reads of Jc are behind: Me and T overwrite it)
    // diag(M) from the diagonal tiles (staged in T's first row), M_e* from tile column 0 (rows >= d_e of Me are kept at zero)
#pragma unroll
    for (int ti = 0; ti < 3; ti++) {
        if (ti < nt) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = lk + 4 * r;
                if (row == li) T[0][16 * ti + li] = acc[ti * (ti + 1) / 2 + ti][r];
                if (li < MAXE) Me[li][16 * ti + row] = li < de ? acc[ti * (ti + 1) / 2][r] : 0.0;
            }
        }
    }
    __syncthreads();
    if (lane < d) {
        const double mcc = T[0][lane];
        if (lane < de) { B.g[C.e_loc + lane] = gc; B.diag[C.e_loc + lane] = mcc; B.vc[C.e_loc + lane] = gc / clampd(mcc, O.min_diag, O.max_diag); }
        else { B.cv_graw[C.v_off + lane - de] = gc; B.cv_dgraw[C.v_off + lane - de] = mcc; }
    }
    __syncthreads();
    QST(2);
    if (de > 0) {
        {
            // [M_ee + mu D | I] -> [I | Einv] by Gauss-Jordan (SPD: no pivoting).  Lane r < d_e keeps row r in registers;
            // step k broadcasts the pivot row through SGPRs (v_readlane), so there is no LDS traffic and no barrier.
            double row[2 * MAXE];
#pragma unroll
            for (int j = 0; j < MAXE; j++) {
                double v = (lane < de && j < de) ? Me[lane][j] : 0.0;
                if (j == lane) v += s_mu * (lane < de ? damp_diag(O, v, B.jsc + C.e_loc + lane, s_it0) : clampd(v, O.min_diag, O.max_diag));
                row[j] = v; row[MAXE + j] = (j == lane) ? 1.0 : 0.0;
            }
            bool bad = false;
#pragma unroll
            for (int k = 0; k < MAXE; k++) {
                if (k < de) {
                    double piv = readlane_d(row[k], k);
                    if (!(piv > 0.0)) bad = true;
                    // reciprocal by v_rcp_f64 + 2 Newton steps instead of the IEEE division expansion
                    double ip = __builtin_amdgcn_rcp(piv);
                    ip = ip * (2.0 - piv * ip); ip = ip * (2.0 - piv * ip);
                    double aik = row[k];
#pragma unroll
                    for (int j = 0; j < 2 * MAXE; j++) {
                        double akj = readlane_d(row[j], k) * ip;
                        row[j] = (lane == k) ? akj : row[j] - aik * akj;
                    }
                }
            }
            if (bad) { if (lane == 0) s.lin_fail = 1; return; }
            if (lane < MAXE) {
#pragma unroll
                for (int j = 0; j < MAXE; j++) Ei[lane][j] = (lane < de && j < de) ? row[MAXE + j] : 0.0;
            }
        }
        __syncthreads();
        QST(3);
        // lane j < d_f: column j of T = Einv M_ef; lanes < d_e: Eg = Einv g_e
        {
            double gE = 0;
            // g_e entries sit in lanes < d_e (gc): broadcast them
            int j = lane < df ? lane : 0;
            // (the column of M_ef and g_e once in registers, a row of Einv at a time: the accumulator tiles stay live across this phase)
            double mcol[MAXE], gb[MAXE];
#pragma unroll
            for (int b2 = 0; b2 < MAXE; b2++) { mcol[b2] = Me[b2][de + j]; gb[b2] = readlane_d(gc, b2); }
#pragma unroll 1
            for (int a2 = 0; a2 < MAXE; a2++) {
                double sv = 0, sg = 0;
#pragma unroll
                for (int b2 = 0; b2 < MAXE; b2++) { double ev = Ei[a2][b2]; sv += ev * mcol[b2]; sg += ev * gb[b2]; }
                if (lane < df) T[a2][lane] = sv;
                if (lane == a2) gE = sg;
            }
            if (lane < de) Eg[lane] = gE;
        }
        __syncthreads();
        QST(4);
        double* E = B.cE + C.e_off;
        {
            for (int e = lane; e < de * de; e += 64) E[e] = Ei[e / de][e % de];
            if (lane < df) {
#pragma unroll
                for (int a2 = 0; a2 < MAXE; a2++) if (a2 < de) E[de * de + a2 * df + lane] = Me[a2][de + lane];
            }
            if (lane < de) E[de * de + de * df + lane] = gc;
            // cs_j = -(M_fe Eg)_j
            if (lane < df) {
                double v = 0;
#pragma unroll
                for (int a2 = 0; a2 < MAXE; a2++) v -= Me[a2][de + lane] * (a2 < de ? Eg[a2] : 0.0);
                B.cv_cs[C.v_off + lane] = v;
            }
        }
        // C = M_ff - M_fe T on the accumulators: A = -M_fe (row 16 ti + i of the tile is column 16 ti + i of Me), B = T shifted by d_e,
        // a2 ascending, rows a2 >= MAXE zero.  (Columns of Me beyond d are zeros of the product above; rows >= d_e of Me and T are zero.)
#pragma unroll
        for (int ks = 0; ks < KE; ks++) {
            const int a2 = 4 * ks + CMM_SLOT_ROW[lk], a2c = a2 < MAXE ? a2 : 0;
            double fa[3], tb[3];
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const int cc = 16 * t + li - de;
                const bool on = t < nt && a2 < MAXE;
                fa[t] = on ? -Me[a2c][16 * t + li] : 0.0;
                tb[t] = on && cc >= 0 && cc < df ? T[a2c][cc] : 0.0;
            }
#pragma unroll
            for (int ti = 0; ti < 3; ti++)
#pragma unroll
                for (int tj = 0; tj <= ti; tj++)
                    if (ti < nt) acc[ti * (ti + 1) / 2 + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ti], tb[tj], acc[ti * (ti + 1) / 2 + tj], 0, 0, 0);
        }
    } else {
        if (lane < df) B.cv_cs[C.v_off + lane] = 0.0;      // (no eliminated block: C = M_ff)
    }
    // both triangles of C from the lower triangle of the tiles
    double* Cm = B.C + C.C_off;
#pragma unroll
    for (int ti = 0; ti < 3; ti++)
#pragma unroll
        for (int tj = 0; tj <= ti; tj++) {
            if (ti < nt) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int R = 16 * ti + lk + 4 * r, Cc = 16 * tj + li;
                    if (R >= Cc && Cc >= de && R < d) {
                        const int i = R - de, j = Cc - de;
                        const double v = acc[ti * (ti + 1) / 2 + tj][r];
                        Cm[i * df + j] = v; Cm[j * df + i] = v;
                    }
                }
            }
        }
    QST(5);
}
