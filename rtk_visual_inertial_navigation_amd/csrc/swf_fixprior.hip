// swf_fixprior.hip — k_fix_prior / k_fix_install (see swf_fixprior.h) for the stand-alone operator swf_prior_fix_batch and for the
// batch engine's swf_batch_fix_prior / swf_batch_install_fixed_prior (swf_engine.hip), which share one body.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_fixprior.h"
#include "swf_lambda.h"
#include "swf_rootdev.h"
#include "swf_stage.h"

void swf_internal_set_error(const std::string& m);
static int fxp_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

#define FXP_NT 1024
static_assert(FXP_MAXN == MG_MAXN && FXP_NT == MG_NT, "k_fix_prior runs the marginalisation consumer's root: same limits, same workgroup");

// ROUND of the reference (R/swf/swf_lambda.cpp: ROUND(x) = floor(x + 0.5)), as the search's kernel rounds
__device__ __forceinline__ double fxp_round(double x) {
#pragma clang fp contract(off)
    return floor(x + 0.5);
}

template <bool BATCH>
__global__ void __launch_bounds__(FXP_NT) k_fix_prior(FixPriorArgs P, DevBatch B) {
    __shared__ double lds[MG_LDS_DOUBLES];            // J (row-major) -> scratch of the group update -> the root's working matrix
    __shared__ double lam[MG_MAXN + 4];               // the rows' values, later the eigenvalues
    __shared__ double bv[MG_MAXN + 4];                // dx (BATCH), then b
    __shared__ double rv[MG_MAXN + 4];                // r at the new point
    __shared__ double pc_dg[MG_MAXN + 4];             // the rows' coordinates and groups (ints), later d_pivoted_chol's running diagonal
    __shared__ int nrot;
    __shared__ unsigned long long crit_sh[2];
    __shared__ int bad_s, nrows_s;
    __shared__ long long off_s[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    int* rc = (int*)pc_dg;                            // row -> prior coordinate
    int* rg = rc + MG_MAXN;                           // row -> group
    double* rval = lam;
    int n = 0, nrows = 0;
    size_t o1 = 0, o2 = 0;
    const double* Jp = nullptr;
    if (tid == 0) { bad_s = 0; nrows_s = 0; }
    __syncthreads();

    // ---------------------------------------------------------------- operands
    if (BATCH) {
        const FixWin fw = P.fw[p];
        const GFac& G = B.gf[fw.gf];
        const int k = G.data;
        n = G.nres;
        o1 = (size_t)p * P.ldn; o2 = (size_t)p * P.ldn * P.ldn;
        Jp = B.prior_J + B.prior_Joff[k];
        // applied iff enabled, the search succeeded, and (ignore_ratio or fixed) — read from the search's record on the device
        const double* rec = P.rec + (size_t)p * P.rec_ld;
        const int f0 = P.pair_first[p], np_all = P.pair_first[p + 1] - f0;
        const int np = fw.n_use < np_all ? fw.n_use : np_all;
        const bool go = fw.enable && np > 0 && n >= 1 && n <= MG_MAXN && (int)rec[LBD_REC_INFO] == SWF_LAMBDA_OK && (P.ignore_ratio || rec[LBD_REC_INFO + 1] != 0.0);
        if (!go) { if (tid == 0) { P.applied[p] = 0; P.rank[p] = 0; } return; }
        // rows: pair i = (a, b) gives (column of a, group b, ROUND(F1[i])); every distinct b gives (column of b, group b, 0) where it
        // first appears.  A value is relative to the point its scalar is linearised at: the scalar's current value is taken off unless
        // scalars_at_zero puts that point at 0.  One thread places them in pair order (a few dozen entries).
        if (tid == 0) {
            const int* tc = P.tailcol + fw.col0;
            int nr = 0;
            for (int i = 0; i < np; i++) {
                const int4 pr = P.pairs[f0 + i];
                bool first = true;
                for (int j = 0; j < i; j++) if (P.pairs[f0 + j].y == pr.y) { first = false; break; }
                const double xa = P.scalars_at_zero ? 0.0 : B.x[pr.z], xb = P.scalars_at_zero ? 0.0 : B.x[pr.w];
                if (first && nr < MG_MAXN) { rc[nr] = tc[pr.y]; rg[nr] = pr.y; rval[nr] = 0.0 - xb; nr++; }
                if (nr < MG_MAXN) { rc[nr] = tc[pr.x]; rg[nr] = pr.y; rval[nr] = fxp_round(rec[LBD_REC_F + i]) - xa; nr++; }
                else bad_s = 1;
            }
            nrows_s = nr;
        }
        // dx of every kept block at the device state (the state swf_batch_download_state would return), and x0' = that state
        const double* x0 = B.prior_x0 + B.prior_x0off[k];
        double* x0n = P.x0n + (size_t)p * P.ldx;
        for (int sl = tid; sl < G.nslot; sl += FXP_NT) {
            const int col = B.s_pcol[G.slot0 + sl], xo = B.s_pxo[G.slot0 + sl], l = B.s_ls[G.slot0 + sl], gs = l == 6 ? 7 : l;
            const double* xs = B.x + B.s_x[G.slot0 + sl];
            double xv[9], tmp[9];
            for (int j = 0; j < gs; j++) xv[j] = (l == 1 && P.scalars_at_zero) ? 0.0 : xs[j];
            prior_block_dx(xv, x0 + xo, gs, tmp);
            for (int j = 0; j < l; j++) bv[col + j] = tmp[j];
            for (int j = 0; j < gs; j++) x0n[xo + j] = xv[j];
        }
    } else {
        // offsets of problem p in the concatenated arrays: sums over the problems before it (integers: exact in any order)
        long long s1 = 0, s2 = 0;
        for (int q = tid; q < p; q += FXP_NT) { const long long d = P.dim[q]; if (d >= 1 && d <= MG_MAXN) { s1 += d; s2 += d * d; } }
        long long* red = (long long*)lds;
        red[tid] = s1; red[FXP_NT + tid] = s2;
        __syncthreads();
        for (int h = FXP_NT / 2; h > 0; h >>= 1) {
            if (tid < h) { red[tid] += red[tid + h]; red[FXP_NT + tid] += red[FXP_NT + tid + h]; }
            __syncthreads();
        }
        if (tid == 0) { off_s[0] = red[0]; off_s[1] = red[FXP_NT]; }
        __syncthreads();
        o1 = (size_t)off_s[0]; o2 = (size_t)off_s[1];
        n = P.dim[p];
        if (n < 1 || n > MG_MAXN) { if (tid == 0) P.rank[p] = -1; return; }
        Jp = P.J + o2;
        const int f0 = P.row_first[p], nr = P.row_first[p + 1] - f0;
        if (nr < 0 || nr > n) { if (tid == 0) P.rank[p] = -1; return; }
        if (tid < nr) { rc[tid] = P.rows[2 * (f0 + tid)]; rg[tid] = P.rows[2 * (f0 + tid) + 1]; rval[tid] = P.vals[f0 + tid]; }
        if (tid < n) rv[tid] = P.r[o1 + tid];
        if (tid == 0) nrows_s = nr;
    }
    for (int e = tid; e < n * n; e += FXP_NT) lds[e] = Jp[e];
    __syncthreads();
    nrows = nrows_s;
    // the rows are checked on the device too (the host entry points refuse them before the launch; device-resident inputs cannot be):
    // a coordinate outside the prior, two rows on one coordinate, a group of one row -> rank -1, nothing else written
    for (int e = tid; e < nrows * nrows; e += FXP_NT) {
        const int a = e / nrows, c = e - a * nrows;
        if (a == c) {
            if (rc[a] < 0 || rc[a] >= n) bad_s = 1;
            int kk = 0;
            for (int q = 0; q < nrows; q++) kk += rg[q] == rg[a];
            if (kk < 2) bad_s = 1;
        } else if (rc[a] == rc[c]) bad_s = 1;
    }
    __syncthreads();
    if (bad_s) { if (tid == 0) { P.rank[p] = -1; if (BATCH) P.applied[p] = 0; } return; }

    // ---------------------------------------------------------------- residual at the new point (BATCH): r = r0 + J dx, a thread per row
    if (BATCH) {
        const double* r0 = B.prior_r0 + B.prior_roff[B.gf[P.fw[p].gf].data];
        if (tid < n) {
            double a = 0;
            for (int j = 0; j < n; j++) a += lds[tid * n + j] * bv[j];
            rv[tid] = r0[tid] + a;
        }
        __syncthreads();
    }

    // ---------------------------------------------------------------- Gram: A0 = J^T J in 4 x 4 register tiles over the lower triangle,
    // rows of J in ascending order (one sum per entry, mirrored: A is symmetric bit for bit); b0 = J^T r
    double* oA = P.A + o2;
    {
        const int nt = (n + 3) >> 2, ntile = nt * (nt + 1) / 2;
        for (int t = tid; t < ntile; t += FXP_NT) {
            int ti = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
            while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
            while (ti * (ti + 1) / 2 > t) ti--;
            const int tj = t - ti * (ti + 1) / 2;
            int ci[4], cj[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { ci[u] = min(4 * ti + u, n - 1); cj[u] = min(4 * tj + u, n - 1); }
            double acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[u][v] = 0.0;
            for (int r = 0; r < n; r++) {
                const double* row = lds + r * n;
                double xi[4], xj[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { xi[u] = row[ci[u]]; xj[u] = row[cj[u]]; }
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int v = 0; v < 4; v++) acc[u][v] += xi[u] * xj[v];
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int i = 4 * ti + u, j = 4 * tj + v;
                    if (i < n && j < n && j <= i) { oA[(size_t)i * n + j] = acc[u][v]; oA[(size_t)j * n + i] = acc[u][v]; }
                }
        }
        if (tid < n) {
            double a = 0;
            for (int r = 0; r < n; r++) a += lds[r * n + tid] * rv[r];
            bv[tid] = a;
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---------------------------------------------------------------- group update (J in LDS is dead: its first 2 nrows doubles hold k and mean(v))
    {
        const double w2 = P.istd * P.istd;
        double* gk = lds; double* gm = lds + MG_MAXN;
        if (tid < nrows) {
            int kk = 0; double sv = 0;
            for (int q = 0; q < nrows; q++) if (rg[q] == rg[tid]) { kk++; sv += rval[q]; }      // row order: a fixed sum
            gk[tid] = (double)kk; gm[tid] = sv / (double)kk;
        }
        __syncthreads();
        // a thread per ordered pair of rows of one group: the coordinates are distinct, so every entry of A is touched at most once
        for (int e = tid; e < nrows * nrows; e += FXP_NT) {
            const int a = e / nrows, c = e - a * nrows;
            if (rg[a] != rg[c]) continue;
            oA[(size_t)rc[a] * n + rc[c]] += w2 * ((a == c ? 1.0 : 0.0) - 1.0 / gk[a]);
        }
        if (tid < nrows) bv[rc[tid]] -= w2 * (rval[tid] - gm[tid]);
    }
    __threadfence_block();
    __syncthreads();
    if (tid < n) P.b[o1 + tid] = bv[tid];

    // ---------------------------------------------------------------- the root
    double* oJ = P.Jn + o2; double* or0 = P.r0 + o1; double* oe = P.eig + o1;
    if (P.form == SWF_PRIOR_CHOLESKY) {
        // A' = L L^T, right-looking in LDS (lower triangle, row-major); J' = L^T, r0' = L^-1 b', eig = diag(L)^2.  A pivot that is not
        // positive (a direction nobody measured) has no Cholesky form: rank -1, zeros — as swf_batch_marginalize's Cholesky form.
        for (int e = tid; e < n * n; e += FXP_NT) lds[e] = oA[e];
        __syncthreads();
        const int ti = tid >> 5, tj = tid & 31;
        bool ok = true;
        for (int k = 0; k < n; k++) {
            const double d = lds[k * n + k];
            if (!(d > 0.0)) { ok = false; break; }      // (uniform: every thread reads the same entry)
            const double sq = sqrt(d);
            __syncthreads();
            if (tid >= k && tid < n) lds[tid * n + k] = tid == k ? sq : lds[tid * n + k] / sq;
            __syncthreads();
            for (int i = k + 1 + ti; i < n; i += 32) {
                const double lik = lds[i * n + k];
                for (int j = k + 1 + tj; j <= i; j += 32) lds[i * n + j] -= lik * lds[j * n + k];
            }
            __syncthreads();
        }
        if (!ok) {
            for (int e = tid; e < n * n; e += FXP_NT) oJ[e] = 0.0;
            if (tid < n) { or0[tid] = 0.0; oe[tid] = 0.0; }
            if (tid == 0) { P.rank[p] = -1; if (BATCH) P.applied[p] = 0; }
            return;
        }
        // forward substitution, column by column: y_k final after step k - 1
        for (int k = 0; k < n; k++) {
            const double yk = bv[k] / lds[k * n + k];
            __syncthreads();
            if (tid == k) bv[k] = yk;
            if (tid > k && tid < n) bv[tid] -= lds[tid * n + k] * yk;
            __syncthreads();
        }
        for (int e = tid; e < n * n; e += FXP_NT) { const int r = e / n, c = e - r * n; oJ[e] = c >= r ? lds[c * n + r] : 0.0; }
        if (tid < n) { or0[tid] = bv[tid]; const double l = lds[tid * n + tid]; oe[tid] = l * l; }
        if (tid == 0) { P.rank[p] = n; if (BATCH) P.applied[p] = 1; }
        return;
    }
    // SWF_PRIOR_EIGEN: G <- the rows of the pivoted Cholesky factor of A' (down to pivots of eps / (16 n): what keeps a weak direction
    // next to the istd^2-sized ones), one-sided Jacobi on its columns, rows of J' = the orthogonalised columns by ascending eigenvalue
    d_pivoted_chol<true>(oA, lds, nullptr, nullptr, pc_dg, nullptr, 0, n, P.eps / (16.0 * n));
    d_jacobi_sweeps(lds, n, nrot, crit_sh, 40);
    const int rank = d_eigen_root_out(lds, n, lam, bv, P.eps, oJ, or0, oe);
    if (tid == 0) { P.rank[p] = rank; if (BATCH) P.applied[p] = 1; }
}

// (J', r0', x0') of every applied window into the batch's own record of that prior, its transposed copy, and — where the prior owns a
// static clique — the clique's C = J^T J over the member columns and its diagonal, accumulated in swf_batch_create's order (rows
// ascending, product and sum rounded separately like the host loop: the installed batch equals a freshly created one bit for bit).
// Windows that were not applied are not touched.
__global__ void __launch_bounds__(FXP_NT) k_fix_install(FixPriorArgs P, DevBatch B) {
#pragma clang fp contract(off)
    __shared__ double lds[MG_LDS_DOUBLES];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (!P.applied[p]) return;
    const GFac& G = B.gf[P.fw[p].gf];
    const int k = G.data, n = G.nres;
    const double* Jn = P.Jn + (size_t)p * P.ldn * P.ldn;
    double* pJ = (double*)B.prior_J + B.prior_Joff[k];
    double* pJt = (double*)B.prior_Jt + B.prior_Joff[k];
    double* pr0 = (double*)B.prior_r0 + B.prior_roff[k];
    double* px0 = (double*)B.prior_x0 + B.prior_x0off[k];
    for (int e = tid; e < n * n; e += FXP_NT) { const double v = Jn[e]; const int r = e / n, c = e - r * n; lds[e] = v; pJ[e] = v; pJt[(size_t)c * n + r] = v; }
    if (tid < n) pr0[tid] = P.r0[(size_t)p * P.ldn + tid];
    const int last = G.slot0 + G.nslot - 1, gsum = B.s_pxo[last] + (B.s_ls[last] == 6 ? 7 : B.s_ls[last]);
    for (int e = tid; e < gsum; e += FXP_NT) px0[e] = P.x0n[(size_t)p * P.ldx + e];
    __syncthreads();
    if (G.clique < 0) return;
    const Clique& C = B.cl[G.clique];
    if (!C.is_static) return;               // a record inside a group-0 block's clique: the evaluation copies its columns at every linearisation
    const int* cc = B.prior_colcc + B.prior_roff[k];
    double* Cm = B.C + C.C_off;
    const int df = C.d_f;
    for (int e = tid; e < n * n; e += FXP_NT) {
        const int a = e / n, c = e - a * n, ma = cc[a], mc = cc[c];
        if (ma < 0 || mc < 0) continue;
        double s = 0;
        for (int r = 0; r < n; r++) s += lds[r * n + a] * lds[r * n + c];
        Cm[(size_t)ma * df + mc] = s;
        if (a == c) B.cv_dgraw[C.v_off + ma] = s;
    }
}

}  // namespace

int swf_internal_fix_prior_launch(const FixPriorArgs& P, const DevBatch& B, bool batch, hipStream_t st) {
    if (P.n_prob <= 0) return SWF_OK;
    if (batch) hipLaunchKernelGGL(k_fix_prior<true>, dim3(P.n_prob), dim3(FXP_NT), 0, st, P, B);
    else hipLaunchKernelGGL(k_fix_prior<false>, dim3(P.n_prob), dim3(FXP_NT), 0, st, P, B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fxp_fail(SWF_E_NODEVICE, std::string("k_fix_prior: ") + hipGetErrorString(e));
    return SWF_OK;
}

int swf_internal_fix_install_launch(const FixPriorArgs& P, const DevBatch& B, hipStream_t st) {
    if (P.n_prob <= 0) return SWF_OK;
    hipLaunchKernelGGL(k_fix_install, dim3(P.n_prob), dim3(FXP_NT), 0, st, P, B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fxp_fail(SWF_E_NODEVICE, std::string("k_fix_install: ") + hipGetErrorString(e));
    return SWF_OK;
}

// the checks of the operator's definition on host-resident rows of one problem (dimension n); 0 or a negative SWF_E_*
int swf_internal_fix_rows_check(int n, int nrows, const int32_t* rows, const char* who) {
    if (nrows < 0 || nrows > n) return fxp_fail(SWF_E_INVALID, std::string(who) + ": more rows than coordinates");
    for (int a = 0; a < nrows; a++) {
        const int c = rows[2 * a];
        if (c < 0 || c >= n) return fxp_fail(SWF_E_INVALID, std::string(who) + ": a row's coordinate is outside the prior");
        int k = 0;
        for (int q = 0; q < nrows; q++) {
            if (q != a && rows[2 * q] == c) return fxp_fail(SWF_E_INVALID, std::string(who) + ": two rows on the same coordinate");
            k += rows[2 * q + 1] == rows[2 * a + 1];
        }
        if (k < 2) return fxp_fail(SWF_E_INVALID, std::string(who) + ": a group with a single row");
    }
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_prior_fix_batch(int32_t n, const int32_t* dim, const double* J, const double* r, const int32_t* row_first,
                                   const int32_t* rows, const double* vals, double istd, double eps, int32_t form,
                                   double* A, double* b, double* Jn, double* r0, double* eig, int32_t* rank,
                                   int32_t on_device, void* stream) {
    const char* who = "swf_prior_fix_batch";
    if (n < 0 || !dim || !J || !r || !row_first) return fxp_fail(SWF_E_INVALID, std::string(who) + ": null argument");
    if (form != SWF_PRIOR_EIGEN && form != SWF_PRIOR_CHOLESKY) return fxp_fail(SWF_E_INVALID, std::string(who) + ": form must be SWF_PRIOR_EIGEN or SWF_PRIOR_CHOLESKY");
    if (!std::isfinite(istd) || !(istd > 0.0) || !std::isfinite(eps) || eps < 0.0) return fxp_fail(SWF_E_INVALID, std::string(who) + ": istd must be positive and eps non-negative");
    if (n == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    FixPriorArgs P{};
    P.n_prob = n; P.form = form; P.istd = istd; P.eps = eps;
    if (on_device) {            // sizes and rows are device memory: the kernel checks them (rank -1)
        if (!rows || !vals || !A || !b || !Jn || !r0 || !eig || !rank) return fxp_fail(SWF_E_INVALID, std::string(who) + ": null argument (device-resident calls take every array)");
        P.dim = dim; P.J = J; P.r = r; P.row_first = row_first; P.rows = rows; P.vals = vals;
        P.A = A; P.b = b; P.Jn = Jn; P.r0 = r0; P.eig = eig; P.rank = rank;
        return swf_internal_fix_prior_launch(P, DevBatch{}, false, st);
    }
    // ---- every argument error is reported before the device is touched
    size_t t1 = 0, t2 = 0;
    if (row_first[0] != 0) return fxp_fail(SWF_E_INVALID, std::string(who) + ": row_first[0] must be 0");
    for (int p = 0; p < n; p++) {
        if (dim[p] < 1) return fxp_fail(SWF_E_INVALID, std::string(who) + ": dim < 1");
        if (dim[p] > FXP_MAXN) return fxp_fail(SWF_E_UNSUPPORTED, std::string(who) + ": dim > 140 (the largest matrix the root keeps in LDS)");
        const int nr = row_first[p + 1] - row_first[p];
        if (nr < 0) return fxp_fail(SWF_E_INVALID, std::string(who) + ": row_first must be non-decreasing");
        if (nr > 0 && (!rows || !vals)) return fxp_fail(SWF_E_INVALID, std::string(who) + ": null rows");
        const int rc = swf_internal_fix_rows_check(dim[p], nr, rows ? rows + 2 * (size_t)row_first[p] : nullptr, who);
        if (rc) return rc;
        t1 += (size_t)dim[p]; t2 += (size_t)dim[p] * dim[p];
    }
    const size_t np = (size_t)n, nrw = (size_t)row_first[n];
    HostStage S(who, st);
    P.dim = S.up(dim, np); P.row_first = S.up(row_first, np + 1);
    P.rows = S.up(rows, nrw * 2, 2); P.vals = S.up(vals, nrw, 1);
    P.J = S.up(J, t2); P.r = S.up(r, t1);
    P.A = S.out<double>(t2); P.b = S.out<double>(t1); P.Jn = S.out<double>(t2); P.r0 = S.out<double>(t1); P.eig = S.out<double>(t1);
    P.rank = S.out<int32_t>(np);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_fix_prior_launch(P, DevBatch{}, false, st);
    if (rc) return rc;
    S.down(A, P.A, t2);
    S.down(b, P.b, t1);
    S.down(Jn, P.Jn, t2);
    S.down(r0, P.r0, t1);
    S.down(eig, P.eig, t1);
    S.down(rank, P.rank, np);
    S.sync();
    return S.rc();
}
