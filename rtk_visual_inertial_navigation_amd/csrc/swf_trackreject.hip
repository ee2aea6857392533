// swf_trackreject.hip — k_track_reject (see swf_trackreject.h) and the C-ABI swf_track_reject_batch.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>
#include "swf_trackreject.h"
#include "swf_trk_lift.h"
#include "swf_devutil.h"
#include "swf_stage.h"

void swf_internal_set_error(const std::string& m);
static int trk_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

// trk_lift (PinholeFullCamera::liftProjective) and trk_velocity (ptsVelocity) are in swf_trk_lift.h: the tracker's finishing kernel
// evaluates the same two functions.

// the virtual camera of :273-280, u = focal x + col / 2, two roundings
__device__ __forceinline__ double trk_virtual(double focal, double x, double half) {
#pragma clang fp contract(off)
    return focal * x + half;
}

// OpenCV's symmetric epipolar test, m1 = cur (u1 v1), m2 = prev (u2 v2).  Every operation is written out, so the count of the scoring
// loop and the mask written later from the best hypothesis are the same decisions.  A NaN is no inlier.
__device__ __forceinline__ bool trk_inlier(const double F[9], double u1, double v1, double u2, double v2, double thr2) {
    const double a = fma(F[0], u1, fma(F[1], v1, F[2])), b = fma(F[3], u1, fma(F[4], v1, F[5])), c = fma(F[6], u1, fma(F[7], v1, F[8]));
    const double n2 = fma(u2, a, fma(v2, b, c));
    const double d2 = (n2 * n2) / fma(a, a, b * b);
    const double at = fma(F[0], u2, fma(F[3], v2, F[6])), bt = fma(F[1], u2, fma(F[4], v2, F[7])), ct = fma(F[2], u2, fma(F[5], v2, F[8]));
    const double n1 = fma(u1, at, fma(v1, bt, ct));
    const double d1 = (n1 * n1) / fma(at, at, bt * bt);
    return d1 <= thr2 && d2 <= thr2;
}

#define TRK_OFF(i) ((i) * 9 - (i) * ((i) - 1) / 2)      // reflector i holds components i .. 8

// Hypothesis k of a pair of n points (s_p: u1 | v1 | u2 | v2, each TRK_NMAX long): the sample, and F by the 8-point algorithm.
// false (F not to be used) on an incomplete sample, a mean distance below 2^-23 or a non-finite value.
__device__ __forceinline__ bool trk_hypothesis(const double* s_p, int n, int k, unsigned long long seed, int smp[8], double F[9]) {
    int got = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) smp[q] = -1;
    if (n == 8) {
#pragma unroll
        for (int q = 0; q < 8; q++) smp[q] = q;
        got = 8;
    } else for (int j = 0; j < TRK_DRAWS && got < 8; j++) {
        const unsigned long long x = swf_mix(seed + 64ull * (unsigned long long)k + (unsigned long long)j);
        const int idx = (int)(((x >> 32) * (unsigned long long)n) >> 32);
        bool dup = false;
#pragma unroll
        for (int q = 0; q < 8; q++) dup |= q < got && smp[q] == idx;
        if (!dup) {
#pragma unroll
            for (int q = 0; q < 8; q++) if (q == got) smp[q] = idx;
            got++;
        }
    }
    if (got != 8) return false;
    // ---- Hartley normalisation of the sample in each image: centroid, sqrt(2) / mean distance
    double c[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int q = 0; q < 8; q++) {
#pragma unroll
        for (int w = 0; w < 4; w++) c[w] += s_p[w * TRK_NMAX + smp[q]];
    }
#pragma unroll
    for (int w = 0; w < 4; w++) c[w] *= 0.125;
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const double dx1 = s_p[smp[q]] - c[0], dy1 = s_p[TRK_NMAX + smp[q]] - c[1];
        const double dx2 = s_p[2 * TRK_NMAX + smp[q]] - c[2], dy2 = s_p[3 * TRK_NMAX + smp[q]] - c[3];
        m1 += sqrt(dx1 * dx1 + dy1 * dy1);
        m2 += sqrt(dx2 * dx2 + dy2 * dy2);
    }
    m1 *= 0.125; m2 *= 0.125;
    if (!(m1 >= 0x1p-23) || !(m2 >= 0x1p-23)) return false;
    const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
    // ---- the null vector of the 8 x 9 design matrix: Householder QR of its transpose, row by row; q = H_0 .. H_7 e_8
    double hv[44], hb[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const double x1 = (s_p[smp[j]] - c[0]) * s1, y1 = (s_p[TRK_NMAX + smp[j]] - c[1]) * s1;
        const double x2 = (s_p[2 * TRK_NMAX + smp[j]] - c[2]) * s2, y2 = (s_p[3 * TRK_NMAX + smp[j]] - c[3]) * s2;
        double a[9] = { x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0 };
#pragma unroll
        for (int i = 0; i < j; i++) {
            double d = 0.0;
#pragma unroll
            for (int r = i; r < 9; r++) d += hv[TRK_OFF(i) + r - i] * a[r];
            d *= hb[i];
#pragma unroll
            for (int r = i; r < 9; r++) a[r] -= d * hv[TRK_OFF(i) + r - i];
        }
        double s = 0.0;
#pragma unroll
        for (int r = j; r < 9; r++) s += a[r] * a[r];
        const double nrm = sqrt(s);
        hv[TRK_OFF(j)] = a[j] >= 0.0 ? a[j] + nrm : a[j] - nrm;
#pragma unroll
        for (int r = j + 1; r < 9; r++) hv[TRK_OFF(j) + r - j] = a[r];
        hb[j] = 1.0 / (nrm * (nrm + fabs(a[j])));
    }
    double g[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 };
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        double d = 0.0;
#pragma unroll
        for (int r = i; r < 9; r++) d += hv[TRK_OFF(i) + r - i] * g[r];
        d *= hb[i];
#pragma unroll
        for (int r = i; r < 9; r++) g[r] -= d * hv[TRK_OFF(i) + r - i];
    }
    // ---- rank 2: one-sided Jacobi on the columns of the 3 x 3 (g row-major, G V = U S), the smallest column dropped
    double V[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
    for (int sweep = 0; sweep < TRK_SWEEPS; sweep++) {
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double aa = g[p] * g[p] + g[3 + p] * g[3 + p] + g[6 + p] * g[6 + p];
            const double bb = g[q] * g[q] + g[3 + q] * g[3 + q] + g[6 + q] * g[6 + q];
            const double cc = g[p] * g[q] + g[3 + p] * g[3 + q] + g[6 + p] * g[6 + q];
            const double zeta = (bb - aa) / (2.0 * cc);
            double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            if (cc == 0.0 || !(t == t)) t = 0.0;
            const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double gp = g[3 * r + p], gq = g[3 * r + q], vp = V[3 * r + p], vq = V[3 * r + q];
                g[3 * r + p] = cs * gp - sn * gq; g[3 * r + q] = sn * gp + cs * gq;
                V[3 * r + p] = cs * vp - sn * vq; V[3 * r + q] = sn * vp + cs * vq;
            }
        }
    }
    double nn[3];
#pragma unroll
    for (int p = 0; p < 3; p++) nn[p] = g[p] * g[p] + g[3 + p] * g[3 + p] + g[6 + p] * g[6 + p];
    int drop = 0;
    double least = nn[0];
    if (nn[1] < least) { drop = 1; least = nn[1]; }
    if (nn[2] < least) drop = 2;
    const double w0 = drop == 0 ? 0.0 : 1.0, w1 = drop == 1 ? 0.0 : 1.0, w2 = drop == 2 ? 0.0 : 1.0;
    double F0[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            F0[3 * i + j] = w0 * (g[3 * i] * V[3 * j]) + w1 * (g[3 * i + 1] * V[3 * j + 1]) + w2 * (g[3 * i + 2] * V[3 * j + 2]);
    }
    // ---- F = T2^T F0 T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]
    const double tx1 = -(c[0] * s1), ty1 = -(c[1] * s1), tx2 = -(c[2] * s2), ty2 = -(c[3] * s2);
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        M[3 * i] = F0[3 * i] * s1; M[3 * i + 1] = F0[3 * i + 1] * s1;
        M[3 * i + 2] = F0[3 * i] * tx1 + F0[3 * i + 1] * ty1 + F0[3 * i + 2];
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        F[j] = s2 * M[j]; F[3 + j] = s2 * M[3 + j];
        F[6 + j] = tx2 * M[j] + ty2 * M[3 + j] + M[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && swf_finite(F[i]);
    return ok;
}

__global__ void __launch_bounds__(TRK_THREADS) k_track_reject(TrkArgs A) {
    __shared__ double s_p[4 * TRK_NMAX];                // u1 | v1 | u2 | v2, each TRK_NMAX long (the staged pixels before the lift)
    __shared__ double s_best[9];
    __shared__ int s_count[TRK_HMAX];
    __shared__ int s_pre[2][TRK_THREADS];
    __shared__ int s_scan[5];                           // best, n_iters, best count, a flag, the scan's next k
    const int f = blockIdx.x, tid = threadIdx.x;
    const int p0 = A.first[f], n = A.first[f + 1] - p0;
    if (p0 < 0 || n < 0 || n > TRK_NMAX) {              // device-resident offsets the host could not check: info = -1, nothing else
        if (tid == 0) A.info[f] = -1;
        return;
    }
    const bool as_float = (A.flags & 1) != 0;
    // ---------------------------------------------------------------- stage the pixels; the non-finite test is on what is staged
    const double dt = A.dt[f];
    bool bad = !swf_finite(dt) || !(dt > 0.0);
    for (int i = tid; i < n; i += TRK_THREADS) {
        const size_t g = (size_t)p0 + i;
        double c[4] = { A.cur_px[2 * g], A.cur_px[2 * g + 1], A.prev_px[2 * g], A.prev_px[2 * g + 1] };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (as_float) c[k] = (double)(float)c[k];
            bad |= !swf_finite(c[k]);
            s_p[k * TRK_NMAX + i] = c[k];
        }
    }
    if (tid == 0) s_scan[3] = 0;
    __syncthreads();
    if (bad) s_scan[3] = 1;
    __syncthreads();
    if (s_scan[3]) {
        if (tid == 0) A.info[f] = SWF_TRK_BAD_INPUT;
        return;
    }
    // ---------------------------------------------------------------- lift, velocity, virtual camera (a thread reads what it staged)
    for (int i = tid; i < n; i += TRK_THREADS) {
        const size_t g = (size_t)p0 + i;
        double xc, yc, xp, yp;
        trk_lift(A.cam, s_p[i], s_p[TRK_NMAX + i], xc, yc);
        trk_lift(A.cam, s_p[2 * TRK_NMAX + i], s_p[3 * TRK_NMAX + i], xp, yp);
        double u[4] = { trk_virtual(A.focal, xc, A.half_col), trk_virtual(A.focal, yc, A.half_row),
                        trk_virtual(A.focal, xp, A.half_col), trk_virtual(A.focal, yp, A.half_row) };
        if (as_float) {
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = (double)(float)u[k];
            xc = (double)(float)xc; yc = (double)(float)yc; xp = (double)(float)xp; yp = (double)(float)yp;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) s_p[k * TRK_NMAX + i] = u[k];
        if (A.un_cur) { A.un_cur[2 * g] = xc; A.un_cur[2 * g + 1] = yc; }
        if (A.un_prev) { A.un_prev[2 * g] = xp; A.un_prev[2 * g + 1] = yp; }
        if (A.velocity) { A.velocity[2 * g] = trk_velocity(xc, xp, dt, as_float); A.velocity[2 * g + 1] = trk_velocity(yc, yp, dt, as_float); }
    }
    if (n < 8) {                                        // the reference skips the gate
        if (tid == 0) A.info[f] = SWF_TRK_TOO_FEW;
        return;
    }
    const int H = n == 8 ? 1 : A.iterations;
    const bool exports = A.samples || A.hyp || A.count;
    if (tid == 0) { s_scan[0] = -1; s_scan[1] = H; s_scan[2] = 0; s_scan[4] = 0; }
    __syncthreads();
    // ---------------------------------------------------------------- chunks of TRK_THREADS hypotheses: solve, score, scan
    for (int base = 0; base < H; base += TRK_THREADS) {
        if (base >= s_scan[1]) break;                   // uniform: written before the last barrier
        const int k = base + tid;
        double F[9];
        if (k < H) {
            int smp[8];
            const bool valid = trk_hypothesis(s_p, n, k, A.seed, smp, F);
            int cnt = 0;
            if (valid) for (int i = 0; i < n; i++)
                cnt += trk_inlier(F, s_p[i], s_p[TRK_NMAX + i], s_p[2 * TRK_NMAX + i], s_p[3 * TRK_NMAX + i], A.thr2) ? 1 : 0;
            s_count[k] = cnt;
        }
        __syncthreads();
        if (tid == 0) {                                 // the sequential scan, continued over this chunk
            int best = s_scan[0], n_iters = s_scan[1], best_count = s_scan[2], kk = s_scan[4];
            const int end = min(base + TRK_THREADS, H);
            for (; kk < n_iters && kk < end; kk++) {
                const int c = s_count[kk];
                if (c > max(best_count, 7)) {
                    best = kk; best_count = c;
                    n_iters = swf_update_iters(A.confidence, c, n, 8, n_iters);
                }
            }
            s_scan[0] = best; s_scan[1] = n_iters; s_scan[2] = best_count; s_scan[4] = kk;
        }
        __syncthreads();
        if (k < H && k == s_scan[0]) {
#pragma unroll
            for (int i = 0; i < 9; i++) s_best[i] = F[i];
        }
    }
    __syncthreads();
    const int best = s_scan[0];
    if (best < 0) {                                     // no hypothesis reaches 8 inliers
        if (tid == 0) A.info[f] = SWF_TRK_NO_MODEL;
        return;
    }
    // ---------------------------------------------------------------- the mask of the best hypothesis and its compaction
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = s_best[i];
    int keep[TRK_NMAX / TRK_THREADS], mine = 0;         // thread t owns points 4 t .. 4 t + 3
#pragma unroll
    for (int j = 0; j < TRK_NMAX / TRK_THREADS; j++) {
        const int i = tid * (TRK_NMAX / TRK_THREADS) + j;
        keep[j] = 0;
        if (i < n) keep[j] = trk_inlier(F, s_p[i], s_p[TRK_NMAX + i], s_p[2 * TRK_NMAX + i], s_p[3 * TRK_NMAX + i], A.thr2) ? 1 : 0;
        mine += keep[j];
    }
    s_pre[0][tid] = mine;
    __syncthreads();
    int src = 0;
    for (int s = 1; s < TRK_THREADS; s <<= 1) {          // inclusive prefix sum, two buffers
        s_pre[1 - src][tid] = s_pre[src][tid] + (tid >= s ? s_pre[src][tid - s] : 0);
        src = 1 - src;
        __syncthreads();
    }
    int at = s_pre[src][tid] - mine;
    const int total = s_pre[src][TRK_THREADS - 1];
#pragma unroll
    for (int j = 0; j < TRK_NMAX / TRK_THREADS; j++) {
        const int i = tid * (TRK_NMAX / TRK_THREADS) + j;
        if (i < n) {
            if (A.status) A.status[(size_t)p0 + i] = (unsigned char)keep[j];
            if (keep[j] && A.keep_idx) A.keep_idx[(size_t)p0 + at] = i;
            at += keep[j];
        }
    }
    if (A.keep_idx) for (int i = total + tid; i < n; i += TRK_THREADS) A.keep_idx[(size_t)p0 + i] = -1;
    if (tid == 0) {
        if (A.n_inliers) A.n_inliers[f] = s_scan[2];
        if (A.best) A.best[f] = best;
        if (A.n_iters) A.n_iters[f] = s_scan[1];
        A.info[f] = SWF_TRK_OK;
    }
    if (tid < 9 && A.F) A.F[(size_t)f * 9 + tid] = s_best[tid];
    if (!exports) return;
    // ---------------------------------------------------------------- the stage exports: every hypothesis again, whatever the scan used
    for (int k = tid; k < H; k += TRK_THREADS) {
        const size_t row = (size_t)f * A.iterations + k;
        int smp[8];
        double Fk[9];
        const bool valid = trk_hypothesis(s_p, n, k, A.seed, smp, Fk);
        if (A.samples) {
#pragma unroll
            for (int q = 0; q < 8; q++) A.samples[row * 8 + q] = smp[q];
        }
        if (A.hyp) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int i = 0; i < 9; i++) A.hyp[row * 9 + i] = valid ? Fk[i] : nan;
        }
        if (A.count) {
            int cnt = 0;
            if (valid) for (int i = 0; i < n; i++)
                cnt += trk_inlier(Fk, s_p[i], s_p[TRK_NMAX + i], s_p[2 * TRK_NMAX + i], s_p[3 * TRK_NMAX + i], A.thr2) ? 1 : 0;
            A.count[row] = cnt;
        }
    }
}

}  // namespace

int swf_internal_trk_launch(const TrkArgs& A, hipStream_t st) {
    if (A.n_pairs <= 0) return SWF_OK;
    hipLaunchKernelGGL(k_track_reject, dim3((unsigned)A.n_pairs), dim3(TRK_THREADS), 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trk_fail(SWF_E_NODEVICE, std::string("k_track_reject: ") + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_track_reject_batch(int32_t n_pairs, const int32_t* first, const double* cur_px, const double* prev_px, const double cam[12],
                                      int32_t col, int32_t row, double focal, const double* dt, int32_t iterations, double threshold,
                                      double confidence, uint64_t seed, int32_t flags, uint8_t* status, int32_t* keep_idx, int32_t* n_inliers,
                                      int32_t* best, int32_t* n_iters, int32_t* info, double* F, double* un_cur, double* un_prev,
                                      double* velocity, int32_t* samples, double* hyp, int32_t* count, int32_t on_device, void* stream) {
    const std::string who = "swf_track_reject_batch";
    if (n_pairs < 0 || !first || !cur_px || !prev_px || !cam || !dt || !info) return trk_fail(SWF_E_INVALID, who + ": null argument");
    if (!std::isfinite(threshold) || !(threshold > 0.0) || !std::isfinite(focal) || !(focal > 0.0) || !std::isfinite(confidence))
        return trk_fail(SWF_E_INVALID, who + ": the threshold and the focal length must be finite and positive and the confidence finite");
    for (int k = 0; k < 12; k++) if (!std::isfinite(cam[k])) return trk_fail(SWF_E_INVALID, who + ": non-finite camera parameters");
    if (cam[0] == 0.0 || cam[1] == 0.0) return trk_fail(SWF_E_INVALID, who + ": fx and fy must not be 0");
    if (iterations < 1 || iterations > SWF_TRK_HMAX) return trk_fail(SWF_E_UNSUPPORTED, who + ": iterations outside 1 .. 1024");
    if (n_pairs == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    TrkArgs A{};
    A.n_pairs = n_pairs;
    for (int k = 0; k < 12; k++) A.cam[k] = cam[k];
    A.focal = focal; A.half_col = (double)col / 2.0; A.half_row = (double)row / 2.0;
    A.iterations = iterations; A.flags = flags; A.thr2 = threshold * threshold; A.confidence = confidence; A.seed = seed;
    if (on_device) {            // the offsets are device memory: the kernel makes the checks
        A.first = first; A.cur_px = cur_px; A.prev_px = prev_px; A.dt = dt;
        A.status = status; A.keep_idx = keep_idx; A.n_inliers = n_inliers; A.best = best; A.n_iters = n_iters; A.info = info;
        A.F = F; A.un_cur = un_cur; A.un_prev = un_prev; A.velocity = velocity; A.samples = samples; A.hyp = hyp; A.count = count;
        return swf_internal_trk_launch(A, st);
    }
    // ---- host memory: the argument errors and the BAD_INPUT pairs before the device is touched
    if (first[0] < 0) return trk_fail(SWF_E_INVALID, who + ": a negative point offset");
    for (int i = 0; i < n_pairs; i++) {
        if (first[i + 1] < first[i]) return trk_fail(SWF_E_INVALID, who + ": point offsets must be non-decreasing");
        if (first[i + 1] - first[i] > SWF_TRK_NMAX) return trk_fail(SWF_E_UNSUPPORTED, who + ": a pair of more than 1024 points");
    }
    const bool as_float = (flags & 1) != 0, lifts = un_cur || un_prev || velocity;
    auto staged_finite = [&](double v) { return std::isfinite(as_float ? (double)(float)v : v); };
    std::vector<int32_t> code((size_t)n_pairs);
    int n_go = 0;
    for (int i = 0; i < n_pairs; i++) {
        const int n = first[i + 1] - first[i];
        bool fin = std::isfinite(dt[i]) && dt[i] > 0.0;
        for (size_t g = (size_t)first[i] * 2; g < (size_t)first[i + 1] * 2; g++) fin = fin && staged_finite(cur_px[g]) && staged_finite(prev_px[g]);
        const int c = !fin ? SWF_TRK_BAD_INPUT : n < 8 ? SWF_TRK_TOO_FEW : SWF_TRK_OK;
        code[(size_t)i] = c;
        info[i] = c;
        n_go += c == SWF_TRK_OK || (c == SWF_TRK_TOO_FEW && n > 0 && lifts);
    }
    if (!n_go) return SWF_OK;

    const size_t nf = (size_t)n_pairs, np = (size_t)(first[n_pairs] - first[0]), H = (size_t)iterations;
    std::vector<int32_t> rel(first, first + n_pairs + 1);
    for (auto& v : rel) v -= first[0];
    // a pair leaves what it does not write as the caller had it: the results pass through staging arrays
    std::vector<double> h_F(F ? nf * 9 : 0), h_uc(un_cur ? np * 2 : 0), h_up(un_prev ? np * 2 : 0), h_v(velocity ? np * 2 : 0), h_h(hyp ? nf * H * 9 : 0);
    std::vector<int32_t> h_info(nf), h_k(keep_idx ? np : 0), h_ni(n_inliers ? nf : 0), h_b(best ? nf : 0), h_it(n_iters ? nf : 0);
    std::vector<int32_t> h_s(samples ? nf * H * 8 : 0), h_n(count ? nf * H : 0);
    std::vector<uint8_t> h_st(status ? np : 0);
    HostStage S("swf_track_reject_batch", st);
    A.first = S.up(rel.data(), rel.size());
    A.cur_px = S.up(cur_px + (size_t)first[0] * 2, np * 2);
    A.prev_px = S.up(prev_px + (size_t)first[0] * 2, np * 2);
    A.dt = S.up(dt, nf);
    A.info = S.out<int32_t>(nf);
    if (status) A.status = S.out<uint8_t>(np);
    if (keep_idx) A.keep_idx = S.out<int32_t>(np);
    if (n_inliers) A.n_inliers = S.out<int32_t>(nf);
    if (best) A.best = S.out<int32_t>(nf);
    if (n_iters) A.n_iters = S.out<int32_t>(nf);
    if (F) A.F = S.out<double>(nf * 9);
    if (un_cur) A.un_cur = S.out<double>(np * 2);
    if (un_prev) A.un_prev = S.out<double>(np * 2);
    if (velocity) A.velocity = S.out<double>(np * 2);
    if (samples) A.samples = S.out<int32_t>(nf * H * 8);
    if (hyp) A.hyp = S.out<double>(nf * H * 9);
    if (count) A.count = S.out<int32_t>(nf * H);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_trk_launch(A, st);
    if (rc) return rc;
    S.down(h_info.data(), A.info, h_info.size());
    S.down(h_st.data(), A.status, h_st.size());
    S.down(h_k.data(), A.keep_idx, h_k.size());
    S.down(h_ni.data(), A.n_inliers, h_ni.size());
    S.down(h_b.data(), A.best, h_b.size());
    S.down(h_it.data(), A.n_iters, h_it.size());
    S.down(h_F.data(), A.F, h_F.size());
    S.down(h_uc.data(), A.un_cur, h_uc.size());
    S.down(h_up.data(), A.un_prev, h_up.size());
    S.down(h_v.data(), A.velocity, h_v.size());
    S.down(h_s.data(), A.samples, h_s.size());
    S.down(h_h.data(), A.hyp, h_h.size());
    S.down(h_n.data(), A.count, h_n.size());
    S.sync();
    if (S.failed()) return S.rc();
    for (int i = 0; i < n_pairs; i++) {
        const int32_t c = h_info[(size_t)i];
        if (code[(size_t)i] == SWF_TRK_BAD_INPUT) {
            if (c != SWF_TRK_BAD_INPUT) return trk_fail(SWF_E_STATE, who + ": the device classified a pair differently from the host");
            continue;
        }
        if ((code[(size_t)i] == SWF_TRK_TOO_FEW) != (c == SWF_TRK_TOO_FEW) || c == SWF_TRK_BAD_INPUT || c < 0)
            return trk_fail(SWF_E_STATE, who + ": the device classified a pair differently from the host");
        info[i] = c;
        const size_t fi = (size_t)i, lo = (size_t)rel[fi], hi = (size_t)rel[fi + 1], at = (size_t)first[i];
        if (un_cur) std::copy(h_uc.begin() + lo * 2, h_uc.begin() + hi * 2, un_cur + at * 2);
        if (un_prev) std::copy(h_up.begin() + lo * 2, h_up.begin() + hi * 2, un_prev + at * 2);
        if (velocity) std::copy(h_v.begin() + lo * 2, h_v.begin() + hi * 2, velocity + at * 2);
        if (c != SWF_TRK_OK) continue;
        const size_t rows = hi - lo == 8 ? 1 : H;
        if (status) std::copy(h_st.begin() + lo, h_st.begin() + hi, status + at);
        if (keep_idx) std::copy(h_k.begin() + lo, h_k.begin() + hi, keep_idx + at);
        if (n_inliers) n_inliers[i] = h_ni[fi];
        if (best) best[i] = h_b[fi];
        if (n_iters) n_iters[i] = h_it[fi];
        if (F) std::copy(h_F.begin() + fi * 9, h_F.begin() + fi * 9 + 9, F + fi * 9);
        if (samples) std::copy(h_s.begin() + fi * H * 8, h_s.begin() + (fi * H + rows) * 8, samples + fi * H * 8);
        if (hyp) std::copy(h_h.begin() + fi * H * 9, h_h.begin() + (fi * H + rows) * 9, hyp + fi * H * 9);
        if (count) std::copy(h_n.begin() + fi * H, h_n.begin() + fi * H + rows, count + fi * H);
    }
    return SWF_OK;
}
