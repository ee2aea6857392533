// swf_rootdev.h — the device functions of the eigen square root, shared by the marginalisation consumer (swf_kernels3.h) and the
// fix-and-hold operator (swf_fixprior.hip): d_pivoted_chol, d_jacobi_sweeps, d_eigen_root_out, with the limits they are built for.
// Each is run by one 1024-thread workgroup; the algorithms are described where their first user is (swf_kernels3.h).
#pragma once
#include "swf_dev.h"

#define MG_MAXN 140                       // largest tail whose M is LDS-resident (153 KB)
#define MG_BIGN 640                       // largest tail of the eigen form (= the largest reduced system, CB_NMAX): above MG_MAXN, M lives in a per-window HBM / L2 scratch
#define MG_NT 1024                        // 64 sixteen-lane groups = 64 column pairs per step
#define MG_LDS_DOUBLES 19600              // 153 KB: M for n <= 140, M and V together for n <= 98
#define Mc(c, r) Mm[(c) * n + (r)]
#define RS_NB 16
// Diagonally pivoted Cholesky of the n x n matrix A (full symmetric, ld = n; read only), 16 pivots at a time, by one 1024-thread
// workgroup: rows v_r of V (ld = n) with sum_r v_r v_r^T = A up to the pivots it drops (the stopping rules: drop_abs below;
// the remaining rows are zero).  LEFT-LOOKING by blocks: a block starts from a POOL of candidates, the (up to) 24 largest entries of
// the running diagonal; their rows of the Schur complement, A[p, :] - sum_r v_r[:] v_r[p] over all rows so far, are formed in LDS in one
// pass over V; the block's (up to) 16 pivots are then taken from the pool in the order the running diagonal dictates (it is kept up to
// date pivot by pivot: that is all the choice needs), each pivot row = its pool row minus the block's earlier rows — LDS work behind
// ONE barrier, no trip to L2 per pivot, no trailing matrix to update (round 3: a rank-one update of the trailing matrix per pivot;
// an earlier form of this round: a lazily updated trailing matrix, one L2 round trip per pivot + 0.5 MB streamed per block).  With 24
// candidates for 16 places the pivots are those of full diagonal pivoting on the cfg5 prior (same rotation counts in the sweeps).
//   !INPLACE: V in global memory (rows) with VT its transpose (the pool pass reads v_r[p] for 24 fixed p and all r: contiguous in VT),
//             Rb = LDS pool rows (24 x n), stg = LDS staging of the pool's VT rows (24 x rc doubles, rc = rows of V per pass)
//   INPLACE:  V itself is LDS (the small tails): pool rows and pivot rows are built in its rows, everything is read from there
// dg = n doubles of LDS: the running diagonal, -1e300 for an eliminated (or dropped) index.
// Two callers: the rank-deficient tails (k_marg_rescue), and the PRECONDITIONER of the Jacobi sweeps (k_marg_pchol, k_marginalize):
// the one-sided Jacobi on the columns of a pivoted Cholesky factor (Veselic / Hari) converges in about half the sweeps the columns of
// the unpivoted L_nn need (cfg5's 263-dimension prior: 8 against 16).
#define RS_POOL 24                        // candidate rows held per block (16 of them at most become pivots)
#define RS_GONE (-1e300)
template <bool INPLACE>
// drop_abs: the stopping rule.  The rank-deficient tails pass 0: the rank-revealing rule, which is SCALE-INVARIANT — an index is
// numerically null once its running diagonal is at most 1e-14 of ITS OWN original A_ii (never a pivot, dropped with its pool), and the
// factorisation ends when no index is left.  (Until this rule the cut was 1e-14 of the LARGEST diagonal entry: with a state of information
// 1e10 in the tail it sat at 1e-4, and decoupled states of information 9e-6 .. 9e-8, which the reference's absolute eigenvalue threshold
// of 1e-8 keeps, came out of k_marg_rescue with a null row — tests/test_eigroot_componentwise.py, rescue_weak.)  What it leaves out is a
// positive semi-definite remainder with diagonal <= 1e-14 A_ii, so |remainder_ij| <= 1e-14 sqrt(A_ii A_jj).
// The preconditioner of a HEALTHY window (its Cholesky went through: A is numerically definite) passes eps / (16 n), eps = the caller's
// eigenvalue threshold (the reference's 1e-8, R/factor/marginalization_factor.cpp:463-470): there the relative cut alone would drop
// whole directions the reference keeps — with diag(A) ~ 1e10 it sits at 1e-4, far above eps — whereas a factorisation that ends at a
// pivot p leaves a remainder of trace <= (n - r) p, i.e. below eps / 16 in every direction: nothing the eps test would have kept is lost.
__device__ __forceinline__ void d_pivoted_chol(const double* A, double* V, double* VT, double* Rb, double* dg, double* stg, const int rc, const int n, const double drop_abs = 0.0) {
    __shared__ int cid[RS_POOL];                          // the block's candidates (indices)
    __shared__ double cdg[RS_POOL];                       // their running diagonal entries; -2 once taken, -1 for an empty slot
    __shared__ double cthr[RS_POOL];                      // drop_abs == 0: 1e-14 of their own original diagonal entries (at or below it: numerically null)
    __shared__ int ncand_s;
    __shared__ double d0_s;
    const int tid = threadIdx.x;
    __syncthreads();
    for (int e = tid; e < n * n; e += 1024) V[e] = 0.0;
    for (int i = tid; i < n; i += 1024) dg[i] = A[(size_t)i * n + i];
    if (tid == 0) d0_s = -1.0;
    __syncthreads();
    // thread (g, i): group 0 owns index i = tid (n <= 640) through the pivot steps; up to three groups share the passes over j (ranks)
    // and over the rows of V (pool rows), a third of the rows each, their partial sums added in group order (deterministic)
    const int ng = min(3, 1024 / n), g = tid / n, i = tid - g * n;
    const bool act = g == 0, gact = g < ng;
#ifdef SWF_PROFILE_CHOL
    unsigned long long pc_t[6] = {0, 0, 0, 0, 0, 0}, pc_l = __builtin_amdgcn_s_memtime();
#define PCACC(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); pc_t[k] += t_ - pc_l; pc_l = t_; } while (0)
#else
#define PCACC(k)
#endif
    int r0 = 0;                                             // rows of V written
    bool stop = false;
    while (r0 < n && !stop) {
        double* R = INPLACE ? V + (size_t)r0 * n : Rb;        // (a compile-time choice: the pointer keeps its address space, LDS either way)
        // ---- the block's candidate pool: the largest entries of the running diagonal, by rank (ties: the smaller index first)
        if (tid < RS_POOL) { cid[tid] = -1; cdg[tid] = -1.0; cthr[tid] = 0.0; }
        if (tid == 0) ncand_s = 0;
        __syncthreads();
        int myslot = -1;
        const int pool = INPLACE ? min(RS_POOL, n - r0) : RS_POOL;
        int* rk = INPLACE ? (int*)R : (int*)stg;            // n integers of LDS that are free right now
        if (act) rk[i] = 0;
        __syncthreads();
        if (gact && dg[i] > 0.5 * RS_GONE) {
            const double ki = dg[i];
            int rank = 0;
            const int j0 = g * n / ng, j1 = (g + 1) * n / ng;
#pragma unroll 8
            for (int j = j0; j < j1; j++) { const double kj = dg[j]; rank += (kj > ki) || (kj == ki && j < i); }
            atomicAdd(&rk[i], rank);
        }
        __syncthreads();
        if (act && dg[i] > 0.5 * RS_GONE) {
            const int rank = rk[i];
            if (rank < pool) { myslot = rank; cid[rank] = i; cdg[rank] = dg[i]; if (!(drop_abs > 0.0)) cthr[rank] = fmax(0.0, 1e-14 * A[(size_t)i * n + i]); atomicAdd(&ncand_s, 1); }
        }
        __syncthreads();
        if (INPLACE && act && 2 * i < n + 1) R[i] = 0.0;      // (the rank counters sat in a row of V)
        PCACC(0);
        const int ncand = ncand_s;                          // (ranks 0 .. ncand - 1 are all present)
        if (ncand == 0) break;
        if (d0_s < 0.0) { __syncthreads(); if (tid == 0) d0_s = cdg[0]; __syncthreads(); }
        const double d0 = d0_s;
        const double thr = drop_abs > 0.0 ? fmin(1e-14 * d0, drop_abs) : 1e-14 * d0;
        // ---- the pool's rows of the Schur complement: thread (g, i) forms entry i of all of them over every ng-th row of V
        {
            double acc[RS_POOL];
#pragma unroll
            for (int c = 0; c < RS_POOL; c++) acc[c] = 0.0;
            if (INPLACE) {
                int pc[RS_POOL];
#pragma unroll
                for (int c = 0; c < RS_POOL; c++) pc[c] = c < ncand ? cid[c] : 0;
                if (gact) for (int r = g; r < r0; r += ng) {
                    const double* row = V + (size_t)r * n;
                    const double vi = row[i];
#pragma unroll
                    for (int c = 0; c < RS_POOL; c++) acc[c] -= vi * row[pc[c]];
                }
            } else {
                for (int rb = 0; rb < r0; rb += rc) {
                    const int nr_ = min(rc, r0 - rb);
                    // stg[rr][c] = v_(rb + rr)[cid[c]], read along the rows of VT
                    __syncthreads();
                    for (int e = tid; e < RS_POOL * nr_; e += 1024) { const int c = e / nr_, rr = e - c * nr_; stg[rr * RS_POOL + c] = c < ncand ? __hip_atomic_load(VT + (size_t)cid[c] * n + rb + rr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0; }      // (past this CU's L1: the lines of a row of VT fill up block by block, written by other waves)
                    __syncthreads();
                    if (gact) {
                        // (eight rows of V on their way at a time: a row is one L2 round trip)
#pragma unroll 8
                        for (int rr = g; rr < nr_; rr += ng) {
                            const double vi = V[(size_t)(rb + rr) * n + i];
                            const double* sp = stg + rr * RS_POOL;
#pragma unroll
                            for (int c = 0; c < RS_POOL; c++) acc[c] -= vi * sp[c];
                        }
                    }
                }
            }
            for (int gg = 0; gg < ng; gg++) {
                if (g == gg) {
#pragma unroll
                    for (int c = 0; c < RS_POOL; c++) if (c < ncand) R[(size_t)c * n + i] = (gg == 0 ? A[(size_t)cid[c] * n + i] : R[(size_t)c * n + i]) + acc[c];      // (A is symmetric: row p = column p, read along the row)
                }
                if (gg + 1 < ng) __syncthreads();
            }
        }
        __syncthreads();
        PCACC(1);
        unsigned long long o_lo = 0, o_hi = 0;              // slot taken at each step, a byte each (uniform)
        auto slot_of = [&](int t) { return (int)(((t < 8 ? o_lo : o_hi) >> (8 * (t & 7))) & 255ull); };
        int nbk = 0;
        for (int sblk = 0; sblk < RS_NB && sblk < ncand; sblk++) {
            // the largest running diagonal entry among the candidates not taken yet (every thread, redundantly: no broadcast step)
            // (every wave, redundantly — no broadcast step — but lane-parallel: most of the 16 waves have no index to work on, and what
            // they issue here competes with the waves that do.  Lane c holds candidate c; the first lane holding the maximum wins.)
            const int ln = tid & 63;
            // (a candidate at or below its cut is never a pivot.  With the one cut of drop_abs > 0 that is the test of the largest one)
            const double cv = ln < RS_POOL && cdg[ln] > (drop_abs > 0.0 ? thr : cthr[ln]) ? cdg[ln] : -3.0;
            const double m16 = grp16_max(cv);
            const double bv = fmax(rows_lane(m16, 0), rows_lane(m16, 16));
            const unsigned long long hit = __builtin_amdgcn_ballot_w64(cv == bv);
            int bc = hit ? __builtin_ctzll(hit) : -1;
            const int ok = (int)(bc >= 0 && bv > 0.0);      // uniform
            // no candidate left above its cut.  drop_abs > 0: the largest of all is numerically zero, rank reached.  drop_abs == 0: the
            // pool holds null indices only; they are dropped below and the next pool may hold smaller indices that are not null on their own scale
            if (!ok) { if (sblk == 0 && drop_abs > 0.0) stop = true; break; }
            const int p = __builtin_amdgcn_readfirstlane(cid[bc]); const double isq = rsqrt_nr(bv);
            // row of the pivot: its pool row minus the block's earlier rows (all requests before the first use); zero at eliminated indices
            if (act) {
                double v = R[(size_t)bc * n + i];
                double xi[RS_NB], xp[RS_NB];
#pragma unroll
                for (int t = 0; t < RS_NB; t++) { const double* row = R + (size_t)(t < sblk ? slot_of(t) : bc) * n; xi[t] = row[i]; xp[t] = row[p]; }
#pragma unroll
                for (int t = 0; t < RS_NB; t++) v -= t < sblk ? xi[t] * xp[t] : 0.0;
                const double di = dg[i];
                const bool gone = !(di > 0.5 * RS_GONE);
                v = gone ? 0.0 : v * isq;
                R[(size_t)bc * n + i] = v;
                const double d = di - v * v;
                if (i == p) { dg[i] = RS_GONE; cdg[bc] = -2.0; }
                else if (!gone) { dg[i] = d; if (myslot >= 0) cdg[myslot] = d; }
            }
            if (sblk < 8) o_lo |= (unsigned long long)bc << (8 * sblk); else o_hi |= (unsigned long long)bc << (8 * (sblk - 8));
            nbk = sblk + 1;
            __syncthreads();
        }
        PCACC(2);
        // pool members that are numerically null by now (a running diagonal only shrinks) are dropped for good
        if (act && myslot >= 0) { const double di = dg[i]; if (di > 0.5 * RS_GONE && !(di > (drop_abs > 0.0 ? thr : cthr[myslot]))) dg[i] = RS_GONE; }
        if (INPLACE) {
            // the block's rows to the front of the pool's slots, in pivot order (row swaps inside LDS: thread i moves column i)
            for (int t = 0; t < nbk; t++) {
                const int sl = slot_of(t);                      // uniform
                if (sl != t) {
                    if (act) { const double x = R[(size_t)t * n + i]; R[(size_t)t * n + i] = R[(size_t)sl * n + i]; R[(size_t)sl * n + i] = x; }
                    // whatever pivot row sat in slot t now sits in slot sl
                    for (int u = t + 1; u < nbk; u++) if (slot_of(u) == t) {
                        if (u < 8) o_lo = (o_lo & ~(255ull << (8 * u))) | ((unsigned long long)sl << (8 * u));
                        else o_hi = (o_hi & ~(255ull << (8 * (u - 8)))) | ((unsigned long long)sl << (8 * (u - 8)));
                    }
                    if (t < 8) o_lo = (o_lo & ~(255ull << (8 * t))) | ((unsigned long long)t << (8 * t));
                    else o_hi = (o_hi & ~(255ull << (8 * (t - 8)))) | ((unsigned long long)t << (8 * (t - 8)));
                }
            }
            __syncthreads();
            for (int e = tid; e < (ncand - nbk) * n; e += 1024) R[(size_t)nbk * n + e] = 0.0;      // the other slots back to zero
        } else if (act) {
            // the block's rows to V and, transposed, to VT (thread i: 16 consecutive entries of its row of VT)
            for (int t = 0; t < nbk; t++) { const double v = R[(size_t)slot_of(t) * n + i]; V[(size_t)(r0 + t) * n + i] = v; VT[(size_t)i * n + r0 + t] = v; }
        }
        r0 += nbk;
        if (nbk == 0 && drop_abs > 0.0) stop = true;      // (drop_abs == 0: every member of the pool was dropped above, the loop ends at an empty pool)
        __threadfence_block();
        __syncthreads();
        PCACC(3);
    }
    __syncthreads();
#ifdef SWF_PROFILE_CHOL
    if (tid == 0 && blockIdx.x == 0) for (int k = 0; k < 5; k++) g_chol_stamps[40 + k] = pc_t[k];
#endif
}

// The two halves of the eigen square root that k_marginalize and the fix-and-hold operator (swf_fixprior.h) share, for a 1024-thread
// workgroup with G in Mm (n x n, column c contiguous; LDS or a global scratch).  d_jacobi_sweeps: the one-sided Jacobi described in
// k_marginalize, at most max_sweeps sweeps; nrot / crit_sh are the caller's __shared__ counters; returns the sweeps run.
__device__ __forceinline__ int d_jacobi_sweeps(double* Mm, const int n, int& nrot, unsigned long long* crit_sh, const int max_sweeps) {
    const int tid = threadIdx.x;
    int grp = tid >> 4, sub = tid & 15;
    int ne = (n + 1) & ~1;                            // even number of players in the round-robin (a bye if n is odd)
    int sweeps_done = 0;
    for (int sweep = 0; sweep < max_sweeps; sweep++) {
        sweeps_done = sweep + 1;
        if (tid == 0) { nrot = 0; crit_sh[0] = 0; crit_sh[1] = 0; }
        double mc2 = 0.0, ms2 = 0.0;
        __syncthreads();
        for (int st = 0; st < ne - 1; st++) {
            // circle method: player ne-1 is fixed, the others rotate; group k plays pair k (and k + 64) of this step
            for (int pr = grp; pr < ne / 2; pr += MG_NT / 16) {
                int p, q;
                if (pr == 0) { p = ne - 1; q = st; }
                else { p = st + pr; if (p >= ne - 1) p -= ne - 1; q = st - pr; if (q < 0) q += ne - 1; }
                if (p > q) { int t = p; p = q; q = t; }
                if (q >= n) continue;                 // the bye (odd n)
                double al = 0, be = 0, ga = 0;
                for (int r = sub; r < n; r += 16) { double a = Mc(p, r), b2 = Mc(q, r); al += a * a; be += b2 * b2; ga += a * b2; }
                al = grp16_sum(al); be = grp16_sum(be); ga = grp16_sum(ga);
                // (the second test keeps zeta^2 finite when a column is numerically null — rank-deficient tails, k_marg_rescue)
                if (ga * ga > 1e-30 * (al * be) && fabs(ga) > 1e-140 * (al + be)) {
                    // rotation from v_rcp / v_rsq + Newton steps: this scalar chain is the critical path of a step
                    double zeta = (be - al) * (0.5 * rcp_nr(ga));
                    double hz = 1.0 + zeta * zeta;
                    double t = (zeta >= 0 ? 1.0 : -1.0) * rcp_nr(fabs(zeta) + hz * rsqrt_nr(hz));
                    double c = rsqrt_nr(1.0 + t * t), sn = c * t;
                    mc2 = fmax(mc2, ga * ga * __builtin_amdgcn_rcp(al * be)); ms2 = fmax(ms2, sn * sn);
                    for (int r = sub; r < n; r += 16) { double a = Mc(p, r), b2 = Mc(q, r); Mc(p, r) = c * a - sn * b2; Mc(q, r) = sn * a + c * b2; }
                    if (sub == 0) atomicAdd(&nrot, 1);
                }
            }
            __syncthreads();
        }
        // (a sweep of tiny rotations leaves nothing for the next one to rotate: see k_marg_bj_crit)
        if (sub == 0 && ms2 > 0.0) { atomicMax(&crit_sh[0], (unsigned long long)__double_as_longlong(mc2)); atomicMax(&crit_sh[1], (unsigned long long)__double_as_longlong(ms2)); }
        __syncthreads();
        int done = nrot == 0 || (double)n * (double)n * __longlong_as_double((long long)crit_sh[0]) * __longlong_as_double((long long)crit_sh[1]) <= 1e-30;
        __syncthreads();
        if (done) break;
    }
    return sweeps_done;
}
// d_eigen_root_out: eigenvalues = squared column norms (into lam, LDS); J = the columns as rows, ascending by eigenvalue, r0 = (column . bv) / lambda,
// eigenvalues <= eps dropped (null row, null r0); outJ n x n row-major, outr0 / outw n.  Returns the rank (every thread).
__device__ __forceinline__ int d_eigen_root_out(const double* Mm, const int n, double* lam, const double* bv, const double eps, double* outJ, double* outr0, double* outw) {
    const int tid = threadIdx.x, grp = tid >> 4, sub = tid & 15;
    for (int c = grp; c < n; c += MG_NT / 16) {
        double a = 0;
        for (int r = sub; r < n; r += 16) a += Mc(c, r) * Mc(c, r);
        a = grp16_sum(a);
        if (sub == 0) lam[c] = a;
    }
    __syncthreads();
    int rank = 0;
    for (int c = 0; c < n; c++) rank += lam[c] > eps;                 // (cheap, every thread)
    for (int c = grp; c < n; c += MG_NT / 16) {
        const double lc = lam[c];
        const bool keep = lc > eps;
        int pos = 0;
        for (int k = 0; k < n; k++) pos += (lam[k] < lc) || (lam[k] == lc && k < c);
        double dotb = 0;
        for (int j = sub; j < n; j += 16) { const double v = Mc(c, j); outJ[(size_t)pos * n + j] = keep ? v : 0.0; dotb += v * bv[j]; }
        dotb = grp16_sum(dotb);
        if (sub == 0) { outr0[pos] = keep ? dotb / lc : 0.0; outw[pos] = lc; }
    }
    return rank;
}
