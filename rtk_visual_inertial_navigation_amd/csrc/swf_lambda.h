// swf_lambda.h — batched LAMBDA integer least squares (RTKLIB lambda(), R/gnss/src/lambda.cpp:58-235) on the device.
//
// One problem per workgroup of one wavefront, n <= 64 unknowns.  The discrete decisions of the reference are kept exactly:
//   LD      Q = L^T diag(D) L from the last row upwards (:58-76); a pivot that is not > 0 is a failure (NaN included)
//   reduce  integer Gauss transforms with ROUND(x) = floor(x + 0.5), a permutation when del + 1e-6 < D[j+1], the restart
//           k = j, j = n - 2 (:78-121)
//   search  MLAMBDA zig-zag enumeration with SGN(x) = x <= 0 ? -1 : 1, the radius first set at the (m+1)-th leaf, LOOPMAX
//           loop iterations, candidates sorted by s ascending (:123-191)
// Two departures, neither of which changes a decision:
//   - Z^-1 is carried through the reduction instead of Z (a Gauss transform on column j of Z is the row update
//     Zi[i,:] += mu Zi[j,:], a permutation swaps two rows), so F = Z^-T E = Zi^T E is a sum of integer products: exactly
//     integer-valued, where the reference solves with an LU factor of Z (:226);
//   - z = Z^T a is carried along with the transforms (z_j -= mu z_i, swaps) as the published method does (Chang, Yang & Zhou
//     2005), where the reference forms the product once after the reduction.
// Floating-point contraction is off in this file: every product and sum is rounded as the C source of the method writes it.
//
// Layout: the factor L in LDS, row r = lane r's row (stride ldl, odd); the search's partial sums S(k, i), i <= k, in the upper
// triangle of the same array (lane i's column k): lane i only ever reads and writes its own S entries.  Z^-1 in a second
// array of the same shape.  Per-level scalars of the search (z, zb, step, dist), D, z and the candidates live in registers,
// lane l holding level l; the wave-uniform control reads them with readlane.
//
// BATCH = true adds the prologue and the epilogue of swf_batch_ambiguity_search: the gather Qb = D Qy D^T, bf = D y from the
// tail covariance and the device state, and the ratio test of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:208-253).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/swf_solver.h"

#define LBD_NMAX 64
#define LBD_LOOPMAX 10000
#define LBD_PERMMAX (10 * LBD_LOOPMAX)      // permutations of the reduction; beyond: SWF_LAMBDA_LOOP_LIMIT (the reference has no bound)
// swf_batch_ambiguity_search: one record of doubles per window, so that one copy returns every window's results
#define LBD_REC_F 0                          // F [2][64]
#define LBD_REC_S 128                        // s [2]
#define LBD_REC_RATIO 130                    // ratio [2]
#define LBD_REC_INFO 132                     // info, fixed, n_b (as doubles)
#define LBD_REC_BF 136                       // bf [64]
#define LBD_REC_QB 200                       // Qb [n_b][n_b] row-major; the record stride is LBD_REC_QB + (largest n_b)^2

struct LambdaArgs {
    int n_prob, ld, m, ldl;               // problems, the caller's leading dimension, candidates, LDS row stride (odd, >= every n;
                                          // the workgroup's LDS is 2 ldl^2 doubles)
    const int* n; const double* a; const double* Q;          // stand-alone: n [p], a [p][ld], Q [p][ld][ld] column-major
    double* F; double* s; int* info;                         // F [p][m][ld], s [p][m], info [p]
    // BATCH only
    const int* pair_first; const int4* pairs;                // [n_prob + 1]; per pair: tail a, tail b, state index of a, of b
    const int* pair_count;                                   // null, or (k_lambda<true, true>, the pairs chosen on the device by k_dd_select):
                                                             // window p owns pair_count[p] pairs at p * LBD_NMAX and pair_first is not read
    const double* tcQ; int tc_ld; const int* tc_n; const int* tc_rank;   // swf_batch_tail_covariance outputs: window p's Qy is
                                                             // tc_n[p] x tc_n[p] row-major at tcQ + p tc_ld^2
    const double* x;                                         // the device state
    double* rec; int rec_ld;                                 // the per-window records (LBD_REC_*), stride rec_ld doubles
    double thr;
};

// enqueue k_lambda<batch> (k_lambda<true, true> when batch and A.pair_count is set) for A.n_prob problems on stream st (swf_lambda.hip)
int swf_internal_lambda_launch(const LambdaArgs& A, bool batch, hipStream_t st);

#ifdef SWF_LAMBDA_DEVICE_BODY
// -DSWF_PROFILE_LAMBDA: per-problem phase stamps of the first LBD_PROF_PROBLEMS problems of a launch (swf_debug_lambda_stamps).
// Slots 0-6: s_memtime at the start, after the operands, LtDL, the reduction, the search, the outputs, the ratio test; 8-14: the same
// boundaries in s_memrealtime ticks; 7: search iterations; 15: permutations of the reduction.
#define LBD_PROF_PROBLEMS 4096
#define LBD_PROF_SLOTS 16
#ifdef SWF_PROFILE_LAMBDA
__device__ unsigned long long g_lambda_prof[LBD_PROF_PROBLEMS * LBD_PROF_SLOTS];
#define LBD_STAMP(i) do { if (l == 0 && p < LBD_PROF_PROBLEMS) { g_lambda_prof[p * LBD_PROF_SLOTS + (i)] = __builtin_amdgcn_s_memtime(); \
                                                             g_lambda_prof[p * LBD_PROF_SLOTS + 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define LBD_COUNT(i, v) do { if (l == 0 && p < LBD_PROF_PROBLEMS) g_lambda_prof[p * LBD_PROF_SLOTS + (i)] = (unsigned long long)(v); } while (0)
#else
#define LBD_STAMP(i)
#define LBD_COUNT(i, v)
#endif
namespace {

__device__ __forceinline__ double lbd_lane(double v, int k) {       // the value lane k holds (k wave-uniform)
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double lbd_round(double x) {
#pragma clang fp contract(off)
    return floor(x + 0.5);
}
__device__ __forceinline__ double lbd_sgn(double x) { return x <= 0.0 ? -1.0 : 1.0; }

// Qb(r, c) = Qy[a_r, a_c] - Qy[a_r, b_c] - Qy[b_r, a_c] + Qy[b_r, b_c]
__device__ __forceinline__ double lbd_qb(const double* Qy, int ld, int4 pr, int4 pc) {
#pragma clang fp contract(off)
    return Qy[(size_t)pr.x * ld + pc.x] - Qy[(size_t)pr.x * ld + pc.y] - Qy[(size_t)pr.y * ld + pc.x] + Qy[(size_t)pr.y * ld + pc.y];
}

// SEL (with BATCH) only changes where the window's pairs are found; k_lambda<true> is compiled from the same text as before it existed.
template <bool BATCH, bool SEL = false>
__global__ void __launch_bounds__(64) k_lambda(LambdaArgs A) {
#pragma clang fp contract(off)
    extern __shared__ double lbd_lds[];
    const int p = blockIdx.x, l = threadIdx.x, ldl = A.ldl;
    double* sL = lbd_lds;                       // A -> L (row r = lane r), S in the upper triangle during the search
    double* sZ = lbd_lds + (size_t)ldl * ldl;   // Z^-1; row i of the factorisation before its normalisation during LD
    const int m = A.m, ldo = A.ld;
    int n = 0, status = SWF_LAMBDA_OK;
    double av = 0.0;                            // a (then z = Z^T a): lane l holds entry l
    int4 mypair = make_int4(0, 0, 0, 0);
    const double* Qy = nullptr;
    int f0 = 0, qld = 0;
    double* rec = BATCH ? A.rec + (size_t)p * A.rec_ld : nullptr;
    LBD_STAMP(0);

    // ---------------------------------------------------------------- operands
    if (BATCH) {
        if (SEL) { f0 = p * LBD_NMAX; n = A.pair_count[p]; }
        else { f0 = A.pair_first[p]; n = A.pair_first[p + 1] - f0; }
        if (n < 1 || n > LBD_NMAX || n > ldl || A.tc_rank[p] < 0) {
            status = SWF_LAMBDA_NO_INPUT;
            if (n >= 1 && n <= LBD_NMAX && n <= ldl && l < n) {          // no valid tail covariance: Qb and bf read back as zeros
                for (int c = 0; c < n; c++) rec[LBD_REC_QB + l * n + c] = 0.0;
                rec[LBD_REC_BF + l] = 0.0;
            }
        } else {
            Qy = A.tcQ + (size_t)p * A.tc_ld * A.tc_ld;
            qld = A.tc_n[p];
            if (l < n) mypair = A.pairs[f0 + l];
            for (int c = 0; c < n; c++) {
                const int4 pc = A.pairs[f0 + c];
                if (l < n) {
                    const double q = lbd_qb(Qy, qld, mypair, pc);
                    sL[l * ldl + c] = q;
                    rec[LBD_REC_QB + l * n + c] = q;
                }
            }
            if (l < n) { av = A.x[mypair.z] - A.x[mypair.w]; rec[LBD_REC_BF + l] = av; }
        }
    } else {
        n = A.n[p];
        if (n < 1 || n > LBD_NMAX || n > ldo || n > ldl) status = SWF_LAMBDA_NO_INPUT;
        else if (l < n) {
            const double* Qp = A.Q + (size_t)p * ldo * ldo;
            av = A.a[(size_t)p * ldo + l];
            for (int c = 0; c <= l; c++) sL[l * ldl + c] = Qp[(size_t)c * ldo + l];      // lower triangle, as LD reads it
        }
    }

    const double a_in = av;                     // a (= bf on the batch path), kept for the ratio test
    LBD_STAMP(1);

    // ---------------------------------------------------------------- LD: Q = L^T diag(D) L, last row first
    double Dv = 0.0;                            // D: lane l holds D[l]
    if (status == SWF_LAMBDA_OK) {
        for (int i = n - 1; i >= 0; i--) {
            __syncthreads();
            const double d = sL[i * ldl + i];
            if (!(d > 0.0)) { status = SWF_LAMBDA_NOT_PD; break; }
            const double sa = sqrt(d), lii = d / sa;
            double t = 0.0;
            if (l <= i) { t = sL[i * ldl + l] / sa; sZ[l] = t; }
            if (l == i) Dv = d;
            __syncthreads();
            if (l < i) for (int k = 0; k <= l; k++) sL[l * ldl + k] -= sZ[k] * t;
            if (l <= i) sL[i * ldl + l] = t / lii;
        }
    }
    LBD_STAMP(2);

    // ---------------------------------------------------------------- reduction (z = Z^T a, Qz = L^T D L)
    if (status == SWF_LAMBDA_OK) {
        __syncthreads();
        for (int r = 0; r < n; r++) if (l < n) sZ[r * ldl + l] = r == l ? 1.0 : 0.0;
        int j = n - 2, k = n - 2, nperm = 0;
        while (j >= 0) {
            __syncthreads();
            if (j <= k) {
                // integer Gauss transforms on column j: lane l updates only row l of L (column j held in a register, mu read from
                // lane i) and column l of Z^-1 (row j of Z^-1 does not change in this loop), so the chain needs no barrier
                double cj = l < n ? sL[l * ldl + j] : 0.0;
                const double zrj = l < n ? sZ[j * ldl + l] : 0.0;
                for (int i = j + 1; i < n; i++) {
                    const double mu = lbd_round(lbd_lane(cj, i));
                    if (mu != 0.0) {
                        if (l >= i && l < n) cj -= mu * sL[l * ldl + i];
                        if (l < n) sZ[i * ldl + l] += mu * zrj;
                        const double zi = lbd_lane(av, i);
                        if (l == j) av -= mu * zi;
                    }
                }
                if (l < n) sL[l * ldl + j] = cj;
                __syncthreads();
            }
            const double Dj = lbd_lane(Dv, j), Dj1 = lbd_lane(Dv, j + 1), Lj1j = sL[(j + 1) * ldl + j];
            const double del = Dj + Lj1j * Lj1j * Dj1;
            if (del + 1E-6 < Dj1) {                               // permutation of j and j + 1
                const double eta = Dj / del, lam = Dj1 * Lj1j / del;
                if (l == j) Dv = eta * Dj1;
                if (l == j + 1) Dv = del;
                if (l < j) {
                    const double a0 = sL[j * ldl + l], a1 = sL[(j + 1) * ldl + l];
                    sL[j * ldl + l] = -Lj1j * a0 + a1;
                    sL[(j + 1) * ldl + l] = eta * a0 + lam * a1;
                }
                if (l == j) sL[(j + 1) * ldl + j] = lam;
                if (l >= j + 2 && l < n) { const double t = sL[l * ldl + j]; sL[l * ldl + j] = sL[l * ldl + j + 1]; sL[l * ldl + j + 1] = t; }
                if (l < n) { const double t = sZ[j * ldl + l]; sZ[j * ldl + l] = sZ[(j + 1) * ldl + l]; sZ[(j + 1) * ldl + l] = t; }
                const double zj = lbd_lane(av, j), zj1 = lbd_lane(av, j + 1);
                if (l == j) av = zj1;
                if (l == j + 1) av = zj;
                // the reference restarts at j = n - 2.  A permutation at j changes only what the checks at j - 1, j and j + 1 read
                // (D[j], D[j+1], rows j, j + 1 and columns j, j + 1 of L), and the checks above j + 1 have all been made on their
                // current values without a permutation (no Gauss transform runs above k = j): they would decide the same again.
                // Restarting at j + 1 takes the reference's path exactly.
                k = j; j = j + 1 < n - 2 ? j + 1 : n - 2;
                if (++nperm >= LBD_PERMMAX) { status = SWF_LAMBDA_LOOP_LIMIT; break; }
            } else j--;
        }
        __syncthreads();
        LBD_COUNT(15, nperm);
    }
    LBD_STAMP(3);

    // ---------------------------------------------------------------- MLAMBDA search
    double E0 = 0.0, E1 = 0.0, s0 = 0.0, s1 = 0.0;    // candidates (lane l: entry l) and their distances
    if (status == SWF_LAMBDA_OK) {
        double zb = 0.0, z = 0.0, step = 0.0, dist = 0.0;     // lane l: level l
        int k = n - 1;
        if (l < n) sL[l * ldl + k] = 0.0;                       // S(n-1, :) = 0
        double zbk = lbd_lane(av, k), zk = lbd_round(zbk), y = zbk - zk;
        if (l == k) { dist = 0.0; zb = zbk; z = zk; step = lbd_sgn(y); }
        double maxdist = 1E99;
        int nn = 0, imax = 0, c;
        for (c = 0; c < LBD_LOOPMAX; c++) {
            // the operands of a descent from level k, S(k, l) and L(k, l), loaded ahead of the distance (their LDS latency overlaps the
            // division; the up and leaf moves do not use them)
            double Sk = 0.0, Lk = 0.0;
            if (l < k) { Sk = sL[l * ldl + k]; Lk = sL[k * ldl + l]; }
            const double newdist = lbd_lane(dist, k) + y * y / lbd_lane(Dv, k);
            if (newdist < maxdist) {
                if (k != 0) {
                    const double dz = lbd_lane(z, k) - lbd_lane(zb, k);
                    k--;
                    if (l == k) dist = newdist;
                    double snew = 0.0;
                    if (l <= k) { snew = Sk + dz * Lk; sL[l * ldl + k] = snew; }
                    zbk = lbd_lane(av, k) + lbd_lane(snew, k);
                    zk = lbd_round(zbk);
                    y = zbk - zk;
                    if (l == k) { zb = zbk; z = zk; step = lbd_sgn(y); }
                } else {
                    if (nn < m) {
                        if (nn == 0 || newdist > (imax ? s1 : s0)) imax = nn;
                        if (nn == 0) { E0 = z; s0 = newdist; } else { E1 = z; s1 = newdist; }
                        nn++;
                    } else {
                        if (newdist < (imax ? s1 : s0)) {
                            if (imax == 0) { E0 = z; s0 = newdist; } else { E1 = z; s1 = newdist; }
                            imax = (m > 1 && s0 < s1) ? 1 : 0;
                        }
                        maxdist = imax ? s1 : s0;
                    }
                    const double st0 = lbd_lane(step, 0), z0 = lbd_lane(z, 0) + st0;
                    y = lbd_lane(zb, 0) - z0;
                    if (l == 0) { z = z0; step = -st0 - lbd_sgn(st0); }
                }
            } else {
                if (k == n - 1) break;
                k++;
                const double stk = lbd_lane(step, k), zk2 = lbd_lane(z, k) + stk;
                y = lbd_lane(zb, k) - zk2;
                if (l == k) { z = zk2; step = -stk - lbd_sgn(stk); }
            }
        }
        if (m > 1 && !(s0 < s1)) { double t = s0; s0 = s1; s1 = t; t = E0; E0 = E1; E1 = t; }    // sort by s
        if (c >= LBD_LOOPMAX) status = SWF_LAMBDA_LOOP_LIMIT;
        LBD_COUNT(7, c);
    }
    LBD_STAMP(4);

    // ---------------------------------------------------------------- back-transform F = Z^-T E (integer arithmetic)
    double F0 = 0.0, F1 = 0.0;
    if (status == SWF_LAMBDA_OK) {
        for (int k = 0; k < n; k++) {
            const double zki = l < n ? sZ[k * ldl + l] : 0.0;
            F0 += zki * lbd_lane(E0, k);
            if (m > 1) F1 += zki * lbd_lane(E1, k);
        }
    } else { s0 = s1 = 0.0; }
    if (BATCH) {
        rec[LBD_REC_F + l] = l < n ? F0 : 0.0;
        rec[LBD_REC_F + LBD_NMAX + l] = l < n ? F1 : 0.0;
        if (l == 0) { rec[LBD_REC_S] = s0; rec[LBD_REC_S + 1] = s1; rec[LBD_REC_INFO] = status; rec[LBD_REC_INFO + 2] = n; }
    } else {
        if (l < ldo) {
            A.F[((size_t)p * m) * ldo + l] = l < n ? F0 : 0.0;
            if (m > 1) A.F[((size_t)p * m + 1) * ldo + l] = l < n ? F1 : 0.0;
        }
        if (l == 0) {
            A.s[(size_t)p * m] = s0;
            if (m > 1) A.s[(size_t)p * m + 1] = s1;
            A.info[p] = status;
        }
    }
    LBD_STAMP(5);

    // ---------------------------------------------------------------- ratio test (SWFOptimization::LambdaSearch :208-253)
    if (BATCH) {
        double r0 = 0.0, r1 = 0.0;
        int fx = 0;
        if (status == SWF_LAMBDA_OK) {
            // S = {i : |F1_i - F2_i| < 1e-2}; e = F1 - bf on S, 0 elsewhere; Qb2 = Qb on S x S, the identity elsewhere
            const bool same = l < n && fabs(F0 - F1) < 1e-2;
            const unsigned long long smask = __ballot(same);
            double e = same ? F0 - a_in : 0.0;
            __syncthreads();
            for (int c2 = 0; c2 < n; c2++) {
                if (l < n) {
                    const bool sc = (smask >> c2) & 1ull;
                    sZ[l * ldl + c2] = (same && sc) ? lbd_qb(Qy, qld, mypair, A.pairs[f0 + c2]) : (l == c2 ? 1.0 : 0.0);
                }
            }
            // Cholesky Qb2 = R R^T (lower, right-looking), then u = R^-1 e, same_cost = u^T u
            double same_cost = 0.0;
            bool ok = true;
            for (int jj = 0; jj < n; jj++) {
                __syncthreads();
                const double djj = sZ[jj * ldl + jj];
                if (!(djj > 0.0)) { ok = false; break; }
                const double rjj = sqrt(djj);
                double lrj = 0.0;
                if (l > jj && l < n) { lrj = sZ[l * ldl + jj] / rjj; sZ[l * ldl + jj] = lrj; }
                const double uj = lbd_lane(e, jj) / rjj;
                same_cost += uj * uj;
                if (l > jj && l < n) e -= lrj * uj;
                __syncthreads();
                if (l > jj && l < n) for (int c2 = jj + 1; c2 <= l; c2++) sZ[l * ldl + c2] -= lrj * sZ[c2 * ldl + jj];
            }
            if (!ok) same_cost = __longlong_as_double(0x7ff8000000000000ll);       // NaN: no ratio[1] decision
            const double s1p = s1 - same_cost;
            double s0p = s0 - same_cost;
            if (fabs(s0p) < 1e-3) s0p = 1e-3;
            r0 = s1 / s0; r1 = s1p / s0p;
            fx = (s0 <= 0.0 || r0 >= A.thr || r1 >= A.thr) ? 1 : 0;
        }
        if (l == 0) { rec[LBD_REC_RATIO] = r0; rec[LBD_REC_RATIO + 1] = r1; rec[LBD_REC_INFO + 1] = fx; }
    }
    LBD_STAMP(6);
}

}  // namespace
#endif
