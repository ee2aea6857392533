// swf_gnssepoch.hip — k_gnss_epoch (see swf_gnssepoch.h) and the stand-alone operator swf_gnss_epoch_solve_batch.
// gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_gnssepoch.h"
#include "swf_devutil.h"
#include "swf_stage.h"
// Floating-point contraction is off in this translation unit, gnss_distance and gnss_range_rate included: every product and sum is
// rounded as it is written, so the two instances of the kernel cannot differ in where a multiply-add was fused.
#pragma clang fp contract(off)
#include "swf_gnss_range.h"

void swf_internal_set_error(const std::string& m);
static int ges_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

enum { GES_D_OBS = 6, GES_D_W = 7, GES_D_LAM = 8, GES_D_N = 9 };

__device__ __forceinline__ double ges_lane(double v, int k) {       // the value lane k holds (k wave-uniform)
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Sums q[k] over the wavefront for every k at once.  Halving steps over lane bits 32, 16, ...: a lane whose bit is set keeps the
// upper half of its quantities and hands the lower half to its partner, the partner the reverse; after log2 K steps a lane holds one
// quantity, and the remaining lane bits are a plain butterfly.  Returns, in lane l, the sum of quantity l / (64 / K); IEEE addition
// commutes, so the lanes that share a quantity hold the same bits.  The order of the additions depends on nothing but K.
template <int K>
__device__ __forceinline__ double ges_reduce(double (&q)[K], int lane) {
    int bit = 32;
#pragma unroll
    for (int h = K / 2; h >= 1; h >>= 1) {
        const bool up = (lane & bit) != 0;
#pragma unroll
        for (int i = 0; i < h; i++) {
            const double lo = q[i], hi = q[i + h];                  // (values, not a choice between two addresses)
            const double send = up ? lo : hi, keep = up ? hi : lo;
            q[i] = keep + __shfl_xor(send, bit);
        }
        bit >>= 1;
    }
    double v = q[0];
#pragma unroll
    for (; bit >= 1; bit >>= 1) v = v + __shfl_xor(v, bit);
    return v;
}
template <int K>
__device__ __forceinline__ double ges_get(double v, int k) { return ges_lane(v, k * (64 / K)); }

struct GesRec {
    double d[SWF_GES_DOUBLES];
    int kind, slot, st, pad;
    bool valid;
};

__device__ __forceinline__ void ges_load(const GnssEpochArgs& A, int f0, int n, int i, GesRec& R) {
    R.valid = i < n;
#pragma unroll
    for (int k = 0; k < SWF_GES_DOUBLES; k++) R.d[k] = k == GES_D_LAM ? 1.0 : 0.0;
    R.kind = SWF_GES_SPP_CODE; R.slot = 0; R.st = 0; R.pad = 0;
    if (R.valid) {
        const int* q = A.rec + ((size_t)f0 + i) * 4;
        R.kind = q[0]; R.slot = q[1]; R.st = q[2]; R.pad = q[3];
        const double* dp = A.dat + ((size_t)f0 + i) * SWF_GES_DOUBLES;
#pragma unroll
        for (int k = 0; k < SWF_GES_DOUBLES; k++) R.d[k] = dp[k];
    }
}

// what the host rejects for host memory
__device__ __forceinline__ bool ges_bad(const GesRec& R) {
    if (!R.valid) return false;
    const bool phase = R.kind == SWF_GES_RTK_PHASE || R.kind == SWF_GES_SPP_PHASE;
    bool bad = R.kind < 0 || R.kind > SWF_GES_DOPPLER || R.slot < 0 || R.slot >= SWF_GES_CLOCKS || (R.st & ~SWF_GES_AMB_FREE) != 0 || R.pad != 0;
    bad |= (R.st & SWF_GES_AMB_FREE) != 0 && !phase;
#pragma unroll
    for (int k = 0; k < SWF_GES_DOUBLES; k++) bad |= !swf_finite(R.d[k]);
    bad |= !(R.d[GES_D_W] >= 0.0);
    bad |= phase && !(R.d[GES_D_LAM] > 0.0);
    return bad;
}

// The arithmetic of one record at (xg, vel, clk): the weighted residual r with the record's own N, the weighted Jacobian j on
// [pos, vel], and nfree, the N that makes the residual of a phase row zero.  Sums run left to right as swf_solver.h writes them.
__device__ __forceinline__ void ges_eval(const double (&d)[SWF_GES_DOUBLES], int kind, const double (&xg)[3], const double (&vel)[3], double clk,
                                         double& r, double& nfree, double (&j)[6]) {
    const double w = d[GES_D_W], obs = d[GES_D_OBS], lam = d[GES_D_LAM], N = d[GES_D_N];
    double e[3];
    nfree = N;
    if (kind == SWF_GES_DOPPLER) {
        double ev[3], rr, ee;
        const double rate = gnss_range_rate(xg, vel, d, d + 3, e, ev, &rr, &ee);
        r = w * (rate + clk + obs);
#pragma unroll
        for (int k = 0; k < 3; k++) { j[k] = w * (ev[k] - ee * e[k]) / rr; j[3 + k] = w * e[k]; }
    } else {
        const double rho = gnss_distance(xg, d, e);
        const bool rtk = kind == SWF_GES_RTK_PHASE || kind == SWF_GES_RTK_CODE;
        const bool phase = kind == SWF_GES_RTK_PHASE || kind == SWF_GES_SPP_PHASE;
        double a = rtk ? rho : rho + clk;             // RTK: rho [- N lam] - obs + clk;  SPP: rho + clk [- N lam] - obs
        double b = a;
        if (phase) a = a - N * lam;
        a = a - obs; b = b - obs;
        if (rtk) { a = a + clk; b = b + clk; }
        r = w * a;
        if (phase) nfree = b / lam;
#pragma unroll
        for (int k = 0; k < 3; k++) { j[k] = w * e[k]; j[3 + k] = 0.0; }
    }
}

// One row of the reduced system: zeros for a lane without a record and for a row whose free ambiguity absorbs it.
struct GesRow { double r, jc, j[6]; };
__device__ __forceinline__ GesRow ges_row(const GesRec& R, const double (&xg)[3], const double (&vel)[3], double clkv, bool fp, bool fv) {
    const double clk = __shfl(clkv, R.slot & 15);
    double r, nfree, j[6];
    ges_eval(R.d, R.kind, xg, vel, clk, r, nfree, j);
    const bool inc = R.valid && (R.st & SWF_GES_AMB_FREE) == 0;
    GesRow o;
    o.r = inc ? r : 0.0;
    o.jc = inc ? R.d[GES_D_W] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) o.j[k] = (inc && (k < 3 ? fp : fv)) ? j[k] : 0.0;
    return o;
}

// the eight sums of one clock, q[OFF .. OFF + 7]: its diagonal, its gradient and its column against [pos, vel]
template <int OFF, int K>
__device__ __forceinline__ void ges_clock_terms(const GesRow& w, bool mine, double (&q)[K]) {
    q[OFF] = mine ? w.jc * w.jc : 0.0;
    q[OFF + 1] = mine ? w.jc * w.r : 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) q[OFF + 2 + k] = mine ? w.j[k] * w.jc : 0.0;
}
__host__ __device__ constexpr int ges_tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }      // a <= b: 0 .. 20

template <bool RES>
__global__ void __launch_bounds__(64 * GES_WPB) k_gnss_epoch(GnssEpochArgs A) {
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GES_WPB + (threadIdx.x >> 6)));
    if (e >= A.n_epochs) return;
    // ---------------------------------------------------------------- level 1: the epoch's run of records
    const int f0 = A.first[e], n = A.first[e + 1] - f0;
    if (f0 < 0 || n < 0 || n > (RES ? 64 : SWF_GES_NMAX)) {
        if (lane == 0 && A.status) A.status[e] = -1;
        return;
    }
    const int nch = RES ? 1 : (n + 63) >> 6;
    // ---------------------------------------------------------------- level 2: records (resident instance), the epoch's state
    GesRec R;
    if (RES) ges_load(A, f0, n, lane, R);
    double pos0[3], vel0[3], base[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { pos0[k] = A.pos[(size_t)e * 3 + k]; vel0[k] = A.vel[(size_t)e * 3 + k]; base[k] = A.base[(size_t)e * 3 + k]; }
    const double clk0 = lane < SWF_GES_CLOCKS ? A.clock[(size_t)e * SWF_GES_CLOCKS + lane] : 0.0;       // lane s keeps clock s
    const int mode = A.mode[e], cc = A.clk_const[e];

    // ---------------------------------------------------------------- what the host rejects; the determining rows of every clock
    bool bad = !swf_finite(clk0) || (mode & ~(SWF_GES_FREE_POS | SWF_GES_FREE_VEL)) != 0 || (cc & ~((1 << SWF_GES_CLOCKS) - 1)) != 0;
#pragma unroll
    for (int k = 0; k < 3; k++) bad |= !swf_finite(pos0[k]) || !swf_finite(vel0[k]) || !swf_finite(base[k]);
    int rows = 0;                                                        // lane s: rows without AMB_FREE, w > 0, on clock s
    for (int c = 0; c < nch; c++) {
        if (!RES) ges_load(A, f0, n, c * 64 + lane, R);
        bad |= ges_bad(R);
        const bool det = R.valid && (R.st & SWF_GES_AMB_FREE) == 0 && R.d[GES_D_W] > 0.0;
#pragma unroll
        for (int s = 0; s < SWF_GES_CLOCKS; s++) {
            const int cnt = __popcll(__ballot(det && R.slot == s));
            if (lane == s) rows += cnt;
        }
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0 && A.status) A.status[e] = -1;
        return;
    }
    const bool fp = (mode & SWF_GES_FREE_POS) != 0, fv = (mode & SWF_GES_FREE_VEL) != 0;
    const bool clk_free = lane < SWF_GES_CLOCKS && ((cc >> lane) & 1) == 0 && rows > 0;      // lane s: clock s is an unknown
    const unsigned long long clk_mask = __ballot(clk_free);

    // ---------------------------------------------------------------- Gauss-Newton
    double pos[3] = { pos0[0], pos0[1], pos0[2] }, vel[3] = { vel0[0], vel0[1], vel0[2] };
    double clkv = clk0;
    double infov = 0.0;                                                  // lane k < 36: entry k of the reduced information matrix
    int status = SWF_GES_MAX_ITER, it = 0;
    while (it < A.max_iter) {
        it++;
        const double xg[3] = { pos[0] + base[0], pos[1] + base[1], pos[2] + base[2] };
        bool deficient = false, big = false;
        double dclk = 0.0;                                               // lane s: the step of clock s
        if (fp || fv) {
            double apv = 0.0, ac[3] = { 0.0, 0.0, 0.0 }, a12 = 0.0;
            for (int c = 0; c < nch; c++) {
                if (!RES) ges_load(A, f0, n, c * 64 + lane, R);
                const GesRow w = ges_row(R, xg, vel, clkv, fp, fv);
                {
                    double q[32];
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int b = a; b < 6; b++) q[ges_tri(a, b)] = w.j[a] * w.j[b];
#pragma unroll
                    for (int a = 0; a < 6; a++) q[21 + a] = w.j[a] * w.r;
#pragma unroll
                    for (int k = 27; k < 32; k++) q[k] = 0.0;
                    apv = apv + ges_reduce<32>(q, lane);
                }
#pragma unroll
                for (int g = 0; g < 3; g++) {
                    double q[32];
                    ges_clock_terms<0>(w, R.slot == g * 4, q); ges_clock_terms<8>(w, R.slot == g * 4 + 1, q);
                    ges_clock_terms<16>(w, R.slot == g * 4 + 2, q); ges_clock_terms<24>(w, R.slot == g * 4 + 3, q);
                    ac[g] = ac[g] + ges_reduce<32>(q, lane);
                }
                {
                    double q[8];
                    ges_clock_terms<0>(w, R.slot == 12, q);
                    a12 = a12 + ges_reduce<8>(q, lane);
                }
            }
            // ---- wave-uniform from here: eliminate the clocks, factor [pos, vel], back-substitute
            double S[6][6], rhs[6];
            {
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++) S[a][b] = ges_get<32>(apv, ges_tri(a, b));
#pragma unroll
                for (int a = 0; a < 6; a++) rhs[a] = -ges_get<32>(apv, 21 + a);
            }
            double hd[6];                                                // the diagonal before the clocks are eliminated
#pragma unroll
            for (int a = 0; a < 6; a++) hd[a] = S[a][a];
#pragma unroll
            for (int s = 0; s < SWF_GES_CLOCKS; s++) {
                if (((clk_mask >> s) & 1ull) == 0ull) continue;
                const double src = s < 12 ? ac[(s >> 2) % 3] : a12;
                double hcc, gc, hpc[6], u[6];
                if (s < 12) { hcc = ges_get<32>(src, (s & 3) * 8); gc = ges_get<32>(src, (s & 3) * 8 + 1); }
                else { hcc = ges_get<8>(src, 0); gc = ges_get<8>(src, 1); }
#pragma unroll
                for (int k = 0; k < 6; k++) { hpc[k] = s < 12 ? ges_get<32>(src, (s & 3) * 8 + 2 + k) : ges_get<8>(src, 2 + k); u[k] = hpc[k] / hcc; }
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int b = a; b < 6; b++) S[a][b] = S[a][b] - u[a] * hpc[b];
                    rhs[a] = rhs[a] + u[a] * gc;
                }
            }
            {                                                            // the information matrix of this linearisation, symmetric
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b < 6; b++) if (lane == a * 6 + b) v = a <= b ? S[a][b] : S[b][a];
                infov = v;
            }
            double L[6][6], dx[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const bool act = i < 3 ? fp : fv;
                const double sii = S[i][i];
                double dg = act ? sii : 1.0;                             // a constant part: a unit pivot and a zero step
#pragma unroll
                for (int k = 0; k < i; k++) dg = dg - L[i][k] * L[i][k];
                if (act && (!(sii > A.eps_rank * hd[i]) || !(dg > A.eps_rank * sii))) deficient = true;
                L[i][i] = sqrt(dg);
#pragma unroll
                for (int jx = i + 1; jx < 6; jx++) {
                    double v = S[i][jx];
#pragma unroll
                    for (int k = 0; k < i; k++) v = v - L[i][k] * L[jx][k];
                    L[jx][i] = v / L[i][i];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double v = rhs[i];
#pragma unroll
                for (int k = 0; k < i; k++) v = v - L[i][k] * dx[k];
                dx[i] = v / L[i][i];
            }
#pragma unroll
            for (int i = 5; i >= 0; i--) {
                double v = dx[i];
#pragma unroll
                for (int k = i + 1; k < 6; k++) v = v - L[k][i] * dx[k];
                dx[i] = v / L[i][i];
            }
#pragma unroll
            for (int s = 0; s < SWF_GES_CLOCKS; s++) {
                if (((clk_mask >> s) & 1ull) == 0ull) continue;
                const double src = s < 12 ? ac[(s >> 2) % 3] : a12;
                double hcc, v;
                if (s < 12) { hcc = ges_get<32>(src, (s & 3) * 8); v = -ges_get<32>(src, (s & 3) * 8 + 1); }
                else { hcc = ges_get<8>(src, 0); v = -ges_get<8>(src, 1); }
#pragma unroll
                for (int k = 0; k < 6; k++) v = v - (s < 12 ? ges_get<32>(src, (s & 3) * 8 + 2 + k) : ges_get<8>(src, 2 + k)) * dx[k];
                v = v / hcc;
                if (lane == s) dclk = v;
            }
            if (!deficient) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    pos[k] = pos[k] + dx[k]; vel[k] = vel[k] + dx[3 + k];
                    big |= !(fabs(dx[k]) <= A.step_tol) || !(fabs(dx[3 + k]) <= A.step_tol);
                }
            }
        } else {
            // ---- [pos, vel] constant: every clock step is the weighted mean of its rows
            double acc = 0.0;
            for (int c = 0; c < nch; c++) {
                if (!RES) ges_load(A, f0, n, c * 64 + lane, R);
                const GesRow w = ges_row(R, xg, vel, clkv, false, false);
                double q[32];
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    const bool mine = s < SWF_GES_CLOCKS && R.slot == s;
                    q[s] = mine ? w.jc * w.jc : 0.0;
                    q[16 + s] = mine ? w.jc * w.r : 0.0;
                }
                acc = acc + ges_reduce<32>(q, lane);
            }
            const double hcc = __shfl(acc, (lane & 15) * 2), gc = __shfl(acc, ((lane & 15) + 16) * 2);
            if (clk_free) dclk = -gc / hcc;
        }
        if (deficient) { status = SWF_GES_RANK_DEFICIENT; break; }
        clkv = clkv + dclk;                                              // (dclk is 0 off the unknown clocks)
        big |= __ballot(clk_free && !(fabs(dclk) <= A.step_tol)) != 0ull;
        if (!big) { status = SWF_GES_CONVERGED; break; }
    }
    if (status == SWF_GES_RANK_DEFICIENT) {                              // the state outputs are the inputs
#pragma unroll
        for (int k = 0; k < 3; k++) { pos[k] = pos0[k]; vel[k] = vel0[k]; }
        clkv = clk0;
    }

    // ---------------------------------------------------------------- after the last iteration: absorb, post-fit residuals, cost
    const double xg[3] = { pos[0] + base[0], pos[1] + base[1], pos[2] + base[2] };
    double cost2 = 0.0;
    for (int c = 0; c < nch; c++) {
        if (!RES) ges_load(A, f0, n, c * 64 + lane, R);
        const double clk = __shfl(clkv, R.slot & 15);
        double r, nfree, j[6];
        ges_eval(R.d, R.kind, xg, vel, clk, r, nfree, j);
        const bool fr = (R.st & SWF_GES_AMB_FREE) != 0;
        const double rp = (R.valid && !fr) ? r : 0.0;
        double q[1] = { rp * rp };
        cost2 = cost2 + ges_reduce<1>(q, lane);
        if (R.valid) {
            const size_t at = (size_t)f0 + c * 64 + lane;
            if (A.r_out) A.r_out[at] = rp;
            if (A.N_out) A.N_out[at] = fr ? nfree : R.d[GES_D_N];
        }
    }
    if (lane < 3) {
        const double p0 = pos[0], p1 = pos[1], p2 = pos[2], v0 = vel[0], v1 = vel[1], v2 = vel[2];
        if (A.pos_out) A.pos_out[(size_t)e * 3 + lane] = lane == 0 ? p0 : lane == 1 ? p1 : p2;
        if (A.vel_out) A.vel_out[(size_t)e * 3 + lane] = lane == 0 ? v0 : lane == 1 ? v1 : v2;
    }
    if (lane < SWF_GES_CLOCKS) {
        if (A.clock_out) A.clock_out[(size_t)e * SWF_GES_CLOCKS + lane] = clkv;
        if (A.clk_rows) A.clk_rows[(size_t)e * SWF_GES_CLOCKS + lane] = rows;
    }
    if (lane < 36 && A.info) A.info[(size_t)e * 36 + lane] = infov;
    if (lane == 0) {
        if (A.cost) A.cost[e] = 0.5 * cost2;
        if (A.iters) A.iters[e] = it;
        if (A.status) A.status[e] = status;
    }
}

}  // namespace

int swf_internal_gnss_epoch_launch(const GnssEpochArgs& A, bool resident, hipStream_t st) {
    if (A.n_epochs <= 0) return SWF_OK;
    const dim3 grid((unsigned)((A.n_epochs + GES_WPB - 1) / GES_WPB)), block(64 * GES_WPB);
    if (resident) hipLaunchKernelGGL(k_gnss_epoch<true>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(k_gnss_epoch<false>, grid, block, 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ges_fail(SWF_E_NODEVICE, std::string("k_gnss_epoch: ") + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_gnss_epoch_solve_batch(int32_t n_epochs, const int32_t* first, const double* pos, const double* vel, const double* base,
                                          const double* clock, const int32_t* mode, const int32_t* clk_const, const double* dat,
                                          const int32_t* rec, int32_t max_iter, double step_tol, double eps_rank, double* pos_out,
                                          double* vel_out, double* clock_out, double* N_out, double* r_out, double* cost, int32_t* iters,
                                          int32_t* status, int32_t* clk_rows, double* info, int32_t on_device, void* stream) {
    const char* who = "swf_gnss_epoch_solve_batch";
    if (n_epochs < 0 || !first || !pos || !vel || !base || !clock || !mode || !clk_const || !dat || !rec)
        return ges_fail(SWF_E_INVALID, std::string(who) + ": null argument");
    if (max_iter < 1) return ges_fail(SWF_E_INVALID, std::string(who) + ": max_iter < 1");
    if (!std::isfinite(step_tol) || !std::isfinite(eps_rank)) return ges_fail(SWF_E_INVALID, std::string(who) + ": step_tol or eps_rank is not finite");
    if (n_epochs == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    GnssEpochArgs A{};
    A.n_epochs = n_epochs; A.max_iter = max_iter; A.step_tol = step_tol; A.eps_rank = eps_rank;
    if (on_device) {            // the sizes are device memory: the general instance runs
        A.first = first; A.pos = pos; A.vel = vel; A.base = base; A.clock = clock; A.mode = mode; A.clk_const = clk_const; A.dat = dat; A.rec = rec;
        A.pos_out = pos_out; A.vel_out = vel_out; A.clock_out = clock_out; A.N_out = N_out; A.r_out = r_out; A.cost = cost; A.iters = iters;
        A.status = status; A.clk_rows = clk_rows; A.info = info;
        return swf_internal_gnss_epoch_launch(A, false, st);
    }
    // ---- host memory: every rejection before the device is touched
    if (first[0] != 0) return ges_fail(SWF_E_INVALID, std::string(who) + ": first[0] != 0");
    int nmax = 0;
    for (int e = 0; e < n_epochs; e++) {
        if (first[e + 1] < first[e]) return ges_fail(SWF_E_INVALID, std::string(who) + ": first decreases");
        nmax = std::max(nmax, (int)(first[e + 1] - first[e]));
    }
    for (int e = 0; e < n_epochs; e++) {
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(pos[(size_t)e * 3 + k]) || !std::isfinite(vel[(size_t)e * 3 + k]) || !std::isfinite(base[(size_t)e * 3 + k]))
                return ges_fail(SWF_E_INVALID, std::string(who) + ": a non-finite pos, vel or base");
        for (int k = 0; k < SWF_GES_CLOCKS; k++)
            if (!std::isfinite(clock[(size_t)e * SWF_GES_CLOCKS + k])) return ges_fail(SWF_E_INVALID, std::string(who) + ": a non-finite clock");
        if ((mode[e] & ~(SWF_GES_FREE_POS | SWF_GES_FREE_VEL)) != 0 || (clk_const[e] & ~((1 << SWF_GES_CLOCKS) - 1)) != 0)
            return ges_fail(SWF_E_INVALID, std::string(who) + ": mode or clk_const bits out of range");
        const int f0 = first[e], n = first[e + 1] - f0;
        for (int i = 0; i < n; i++) {
            const int32_t* q = rec + (size_t)(f0 + i) * 4;
            const double* d = dat + (size_t)(f0 + i) * SWF_GES_DOUBLES;
            const bool phase = q[0] == SWF_GES_RTK_PHASE || q[0] == SWF_GES_SPP_PHASE;
            if (q[0] < 0 || q[0] > SWF_GES_DOPPLER || q[1] < 0 || q[1] >= SWF_GES_CLOCKS || (q[2] & ~SWF_GES_AMB_FREE) != 0 || q[3] != 0)
                return ges_fail(SWF_E_INVALID, std::string(who) + ": kind, clock slot or state bits out of range");
            if ((q[2] & SWF_GES_AMB_FREE) != 0 && !phase) return ges_fail(SWF_E_INVALID, std::string(who) + ": AMB_FREE on a row without an ambiguity");
            for (int k = 0; k < SWF_GES_DOUBLES; k++)
                if (!std::isfinite(d[k])) return ges_fail(SWF_E_INVALID, std::string(who) + ": a non-finite record value");
            if (d[GES_D_W] < 0.0) return ges_fail(SWF_E_INVALID, std::string(who) + ": a negative weight");
            if (phase && d[GES_D_LAM] <= 0.0) return ges_fail(SWF_E_INVALID, std::string(who) + ": a wavelength must be positive");
        }
    }
    if (nmax > SWF_GES_NMAX) return ges_fail(SWF_E_UNSUPPORTED, std::string(who) + ": more than 512 records in an epoch");

    const size_t ne = (size_t)n_epochs, nr = (size_t)first[n_epochs];
    HostStage S(who, st);
    A.first = S.up(first, ne + 1); A.pos = S.up(pos, ne * 3); A.vel = S.up(vel, ne * 3); A.base = S.up(base, ne * 3);
    A.clock = S.up(clock, ne * SWF_GES_CLOCKS); A.mode = S.up(mode, ne); A.clk_const = S.up(clk_const, ne);
    A.dat = S.up(dat, nr * SWF_GES_DOUBLES, SWF_GES_DOUBLES); A.rec = S.up(rec, nr * 4, 4);
    A.pos_out = S.out<double>(ne * 3); A.vel_out = S.out<double>(ne * 3); A.clock_out = S.out<double>(ne * SWF_GES_CLOCKS);
    A.N_out = S.out<double>(nr); A.r_out = S.out<double>(nr); A.cost = S.out<double>(ne);
    A.iters = S.out<int32_t>(ne); A.status = S.out<int32_t>(ne); A.clk_rows = S.out<int32_t>(ne * SWF_GES_CLOCKS); A.info = S.out<double>(ne * 36);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_gnss_epoch_launch(A, nmax <= 64, st);
    if (rc) return rc;
    S.down(pos_out, A.pos_out, ne * 3);
    S.down(vel_out, A.vel_out, ne * 3);
    S.down(clock_out, A.clock_out, ne * SWF_GES_CLOCKS);
    S.down(N_out, A.N_out, nr);
    S.down(r_out, A.r_out, nr);
    S.down(cost, A.cost, ne);
    S.down(iters, A.iters, ne);
    S.down(status, A.status, ne);
    S.down(clk_rows, A.clk_rows, ne * SWF_GES_CLOCKS);
    S.down(info, A.info, ne * 36);
    S.sync();
    return S.rc();
}
