// swf_pnp.hip — k_pnp_frame (see swf_pnp.h) and the C-ABI swf_pnp_frame_batch.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>
#include "swf_pnp.h"
#include "swf_devutil.h"
#include "swf_stage.h"

void swf_internal_set_error(const std::string& m);
static int pnp_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

// The inlier test.  Every operation is written out (no contraction left to the compiler), so the count of the scoring loop and the
// mask written later from the best hypothesis are the same decisions.
__device__ __forceinline__ bool pnp_inlier(const double R[9], const double t[3], double X, double Y, double Z, double u, double v, double thr2) {
    const double x = fma(R[2], Z, fma(R[1], Y, fma(R[0], X, t[0])));
    const double y = fma(R[5], Z, fma(R[4], Y, fma(R[3], X, t[1])));
    const double z = fma(R[8], Z, fma(R[7], Y, fma(R[6], X, t[2])));
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z;
    const double rx = fma(x, iz, -u), ry = fma(y, iz, -v);
    return fma(ry, ry, rx * rx) <= thr2;
}

// The two residual rows of one point added to the sums: acc[0..20] the lower triangle of J^T J (row i, column j at i (i + 1) / 2 + j),
// acc[21..26] J^T r.  J = [-J_p [R p_w]_x | J_p].  false when |z| < 1e-12.
__device__ __forceinline__ bool pnp_accumulate(const double R[9], const double t[3], double X, double Y, double Z, double u, double v, double acc[27]) {
    const double qx = R[0] * X + R[1] * Y + R[2] * Z, qy = R[3] * X + R[4] * Y + R[5] * Z, qz = R[6] * X + R[7] * Y + R[8] * Z;
    const double x = qx + t[0], y = qy + t[1], z = qz + t[2];
    if (!(fabs(z) >= 1e-12)) return false;
    const double iz = 1.0 / z, xn = x * iz, yn = y * iz;
    const double jx2 = -(xn * iz), jy2 = -(yn * iz);
    const double g[2][6] = { { jx2 * qy, iz * qz - jx2 * qx, -(iz * qy), iz, 0.0, jx2 },
                             { jy2 * qy - iz * qz, -(jy2 * qx), iz * qx, 0.0, iz, jy2 } };
    const double r[2] = { xn - u, yn - v };
#pragma unroll
    for (int w = 0; w < 2; w++) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int j = 0; j <= i; j++) acc[i * (i + 1) / 2 + j] += g[w][i] * g[w][j];
        }
#pragma unroll
        for (int i = 0; i < 6; i++) acc[21 + i] += g[w][i] * r[w];
    }
    return true;
}

// Unpivoted Cholesky of the 6 x 6 system in acc, x = -(J^T J)^-1 J^T r.  false on a pivot that is not > 0 or a non-finite solution.
__device__ __forceinline__ bool pnp_solve(const double acc[27], double x[6]) {
    double L[21];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = acc[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        ok = ok && d > 0.0;
        d = sqrt(d > 0.0 ? d : 1.0);
        L[j * (j + 1) / 2 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = acc[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s / d;
        }
    }
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = -acc[21 + i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * yv[k];
        yv[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = yv[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + i] * x[k];
        x[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && swf_finite(x[i]);
    return ok;
}

// R <- Exp(x[0..2]) R (Rodrigues; I + [w]_x below |w| = 1e-12), t <- t + x[3..5]
__device__ __forceinline__ void pnp_update(double R[9], double t[3], const double x[6]) {
    const double wx = x[0], wy = x[1], wz = x[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double a = 1.0, c = 0.0;
    if (th >= 1e-12) { a = sin(th) / th; c = (1.0 - cos(th)) / (th * th); }
    const double K[9] = { 0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0 };
    const double W[3] = { wx, wy, wz };
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) E[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K[3 * i + j] + c * (W[i] * W[j] - (i == j ? th2 : 0.0));
    }
    double N[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) N[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = N[i];
    t[0] += x[3]; t[1] += x[4]; t[2] += x[5];
}

__global__ void __launch_bounds__(PNP_THREADS) k_pnp_frame(PnpArgs A) {
    __shared__ double s_p[5 * PNP_NMAX];                // X | Y | Z | u | v, each PNP_NMAX long
    __shared__ double s_red[9 * PNP_THREADS];
    __shared__ double s_best[12];
    __shared__ int s_count[PNP_HMAX];
    __shared__ unsigned char s_in[PNP_NMAX];
    __shared__ int s_scan[4];                           // best, n_iters, best count, a flag
    const int f = blockIdx.x, tid = threadIdx.x;
    const int p0 = A.first[f], n = A.first[f + 1] - p0;
    if (p0 < 0 || n < 0 || n > PNP_NMAX) {              // device-resident offsets the host could not check: info = -1, nothing else
        if (tid == 0) A.info[f] = -1;
        return;
    }
    if (n < 4) {
        if (tid == 0) A.info[f] = SWF_PNP_TOO_FEW;
        return;
    }
    // ---------------------------------------------------------------- stage the points; the non-finite test is on what is staged
    bool bad = false;
    for (int i = tid; i < n; i += PNP_THREADS) {
        const size_t g = (size_t)p0 + i;
        double c[5] = { A.pts_w[3 * g], A.pts_w[3 * g + 1], A.pts_w[3 * g + 2], A.pts_uv[2 * g], A.pts_uv[2 * g + 1] };
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (A.flags & 1) c[k] = (double)(float)c[k];
            bad |= !swf_finite(c[k]);
            s_p[k * PNP_NMAX + i] = c[k];
        }
    }
    double Pp[3], Rp[9];
#pragma unroll
    for (int k = 0; k < 3; k++) { Pp[k] = A.Ps_prev[(size_t)f * 3 + k]; bad |= !swf_finite(Pp[k]); }
#pragma unroll
    for (int k = 0; k < 9; k++) { Rp[k] = A.Rs_prev[(size_t)f * 9 + k]; bad |= !swf_finite(Rp[k]); }
    if (tid == 0) s_scan[3] = 0;
    __syncthreads();
    if (bad) s_scan[3] = 1;
    __syncthreads();
    if (s_scan[3]) {
        if (tid == 0) A.info[f] = SWF_PNP_BAD_INPUT;
        return;
    }
    // ---------------------------------------------------------------- the guess: cam_T_w of the previous frame (:232-233, :170-171)
    double R[9], t[3];
    {
        double RC[9], PC[3], d[3] = { A.tic[0] - A.pbg[0], A.tic[1] - A.pbg[1], A.tic[2] - A.pbg[2] };
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) RC[3 * i + j] = Rp[3 * i] * A.ric[j] + Rp[3 * i + 1] * A.ric[3 + j] + Rp[3 * i + 2] * A.ric[6 + j];
            PC[i] = Rp[3 * i] * d[0] + Rp[3 * i + 1] * d[1] + Rp[3 * i + 2] * d[2] + Pp[i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = RC[3 * j + i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = -(R[3 * i] * PC[0] + R[3 * i + 1] * PC[1] + R[3 * i + 2] * PC[2]);
    }
    const int m = n >= 5 ? 5 : 4, H = n >= 5 ? A.iterations : 1;
    // ---------------------------------------------------------------- lane k: sample, minimal solve, score
    int smp[5] = { -1, -1, -1, -1, -1 };
    bool valid = false;
    int cnt = 0;
    if (tid < H) {
        int got = 0;
        if (n == 4) { smp[0] = 0; smp[1] = 1; smp[2] = 2; smp[3] = 3; got = 4; }
        else for (int j = 0; j < PNP_DRAWS && got < 5; j++) {
            const unsigned long long x = swf_mix(A.seed + 64ull * (unsigned long long)tid + (unsigned long long)j);
            const int idx = (int)(((x >> 32) * (unsigned long long)n) >> 32);
            bool dup = false;
#pragma unroll
            for (int q = 0; q < 5; q++) dup |= q < got && smp[q] == idx;
            if (!dup) {
#pragma unroll
                for (int q = 0; q < 5; q++) if (q == got) smp[q] = idx;
                got++;
            }
        }
        valid = got == m;
        for (int step = 0; step < PNP_K_MIN && valid; step++) {
            double acc[27];
#pragma unroll
            for (int i = 0; i < 27; i++) acc[i] = 0.0;
#pragma unroll
            for (int q = 0; q < 5; q++) if (q < m && valid) {
                const int i = smp[q];
                valid = pnp_accumulate(R, t, s_p[i], s_p[PNP_NMAX + i], s_p[2 * PNP_NMAX + i], s_p[3 * PNP_NMAX + i], s_p[4 * PNP_NMAX + i], acc);
            }
            double x[6];
            if (valid) valid = pnp_solve(acc, x);
            if (valid) pnp_update(R, t, x);
        }
        if (valid) {
#pragma unroll
            for (int i = 0; i < 9; i++) valid = valid && swf_finite(R[i]);
#pragma unroll
            for (int i = 0; i < 3; i++) valid = valid && swf_finite(t[i]);
        }
        if (valid) for (int i = 0; i < n; i++)
            cnt += pnp_inlier(R, t, s_p[i], s_p[PNP_NMAX + i], s_p[2 * PNP_NMAX + i], s_p[3 * PNP_NMAX + i], s_p[4 * PNP_NMAX + i], A.thr2) ? 1 : 0;
        s_count[tid] = cnt;
    }
    __syncthreads();
    // ---------------------------------------------------------------- the scan: one lane
    if (tid == 0) {
        int best = -1, best_count = 0, n_iters = H;
        for (int k = 0; k < n_iters && k < H; k++) {
            const int c = s_count[k];
            if (c > max(best_count, m - 1)) {
                best = k; best_count = c;
                n_iters = swf_update_iters(A.confidence, c, n, m, n_iters);
            }
        }
        s_scan[0] = best; s_scan[1] = n_iters; s_scan[2] = best_count; s_scan[3] = 0;
    }
    __syncthreads();
    const int best = s_scan[0];
    if (best < 0) {                                     // the reference leaves the pose alone
        if (tid == 0) A.info[f] = SWF_PNP_NO_MODEL;
        return;
    }
    if (tid == best) {
#pragma unroll
        for (int i = 0; i < 9; i++) s_best[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) s_best[9 + i] = t[i];
    }
    if (tid < H) {                                      // the stage exports
        const size_t row = (size_t)f * A.iterations + tid;
        if (A.samples) for (int q = 0; q < 5; q++) A.samples[row * 5 + q] = smp[q];
        if (A.hyp) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int i = 0; i < 9; i++) A.hyp[row * 12 + i] = valid ? R[i] : nan;
#pragma unroll
            for (int i = 0; i < 3; i++) A.hyp[row * 12 + 9 + i] = valid ? t[i] : nan;
        }
        if (A.count) A.count[row] = cnt;
    }
    __syncthreads();
    // ---------------------------------------------------------------- the mask of the best hypothesis
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = s_best[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = s_best[9 + i];
    for (int i = tid; i < n; i += PNP_THREADS) {
        const unsigned char in = pnp_inlier(R, t, s_p[i], s_p[PNP_NMAX + i], s_p[2 * PNP_NMAX + i], s_p[3 * PNP_NMAX + i], s_p[4 * PNP_NMAX + i], A.thr2) ? 1 : 0;
        s_in[i] = in;
        A.inlier[(size_t)p0 + i] = in;
    }
    __syncthreads();
    // ---------------------------------------------------------------- refinement over the inliers; every sum in a fixed order
    bool refined = true;
    for (int step = 0; step < PNP_K_REF; step++) {
        double acc[27];
#pragma unroll
        for (int i = 0; i < 27; i++) acc[i] = 0.0;
        bool zok = true;
        for (int i = tid; i < n; i += PNP_THREADS)
            if (s_in[i]) zok = pnp_accumulate(R, t, s_p[i], s_p[PNP_NMAX + i], s_p[2 * PNP_NMAX + i], s_p[3 * PNP_NMAX + i], s_p[4 * PNP_NMAX + i], acc) && zok;
        if (!zok) s_scan[3] = 1;
        int zbad = 0;
#pragma unroll
        for (int c0 = 0; c0 < 27; c0 += 9) {
#pragma unroll
            for (int c = 0; c < 9; c++) s_red[c * PNP_THREADS + tid] = acc[c0 + c];
            __syncthreads();
            for (int s = PNP_THREADS / 2; s > 0; s >>= 1) {
                if (tid < s) {
#pragma unroll
                    for (int c = 0; c < 9; c++) s_red[c * PNP_THREADS + tid] += s_red[c * PNP_THREADS + tid + s];
                }
                __syncthreads();
            }
#pragma unroll
            for (int c = 0; c < 9; c++) acc[c0 + c] = s_red[c * PNP_THREADS];
            zbad = s_scan[3];                           // read before the step's last barrier: the next step's store comes after it
            __syncthreads();
        }
        double x[6];
        if (zbad || !pnp_solve(acc, x)) { refined = false; break; }         // the same values in every thread: a uniform branch
        pnp_update(R, t, x);
    }
    if (refined) {
#pragma unroll
        for (int i = 0; i < 9; i++) refined = refined && swf_finite(R[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) refined = refined && swf_finite(t[i]);
    }
    if (!refined) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = s_best[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = s_best[9 + i];
    }
    // ---------------------------------------------------------------- cam_T_w -> Ps, Rs of the IMU frame (:199-200, :237-238)
    if (tid == 0) {
        double PC[3], RS[9];
        const double d[3] = { A.tic[0] - A.pbg[0], A.tic[1] - A.pbg[1], A.tic[2] - A.pbg[2] };
#pragma unroll
        for (int i = 0; i < 3; i++) PC[i] = R[i] * -t[0] + R[3 + i] * -t[1] + R[6 + i] * -t[2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) RS[3 * i + j] = R[i] * A.ric[3 * j] + R[3 + i] * A.ric[3 * j + 1] + R[6 + i] * A.ric[3 * j + 2];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) A.Ps_out[(size_t)f * 3 + i] = PC[i] - (RS[3 * i] * d[0] + RS[3 * i + 1] * d[1] + RS[3 * i + 2] * d[2]);
#pragma unroll
        for (int i = 0; i < 9; i++) A.Rs_out[(size_t)f * 9 + i] = RS[i];
        A.n_inliers[f] = s_scan[2];
        A.best[f] = best;
        A.n_iters[f] = s_scan[1];
        A.info[f] = refined ? SWF_PNP_OK : SWF_PNP_UNREFINED;
    }
}

}  // namespace

int swf_internal_pnp_launch(const PnpArgs& A, hipStream_t st) {
    if (A.n_frames <= 0) return SWF_OK;
    hipLaunchKernelGGL(k_pnp_frame, dim3((unsigned)A.n_frames), dim3(PNP_THREADS), 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pnp_fail(SWF_E_NODEVICE, std::string("k_pnp_frame: ") + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_pnp_frame_batch(int32_t n_frames, const int32_t* first, const double* pts_w, const double* pts_uv,
                                   const double* Ps_prev, const double* Rs_prev, const double tic[3], const double ric[9], const double pbg[3],
                                   int32_t iterations, double threshold, double confidence, uint64_t seed, int32_t flags,
                                   double* Ps_out, double* Rs_out, int32_t* n_inliers, uint8_t* inlier, int32_t* best, int32_t* n_iters,
                                   int32_t* info, int32_t* samples, double* hyp, int32_t* count, int32_t on_device, void* stream) {
    const std::string who = "swf_pnp_frame_batch";
    if (n_frames < 0 || !first || !pts_w || !pts_uv || !Ps_prev || !Rs_prev || !tic || !ric || !pbg || !Ps_out || !Rs_out || !n_inliers ||
        !inlier || !best || !n_iters || !info) return pnp_fail(SWF_E_INVALID, who + ": null argument");
    if (!std::isfinite(threshold) || !(threshold > 0.0) || !std::isfinite(confidence))
        return pnp_fail(SWF_E_INVALID, who + ": the threshold must be finite and positive and the confidence finite");
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(ric[k]) || !std::isfinite(tic[k % 3]) || !std::isfinite(pbg[k % 3])) return pnp_fail(SWF_E_INVALID, who + ": non-finite extrinsics");
    if (iterations < 1 || iterations > SWF_PNP_HMAX) return pnp_fail(SWF_E_UNSUPPORTED, who + ": iterations outside 1 .. 128");
    if (n_frames == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    PnpArgs A{};
    A.n_frames = n_frames;
    for (int k = 0; k < 3; k++) { A.tic[k] = tic[k]; A.pbg[k] = pbg[k]; }
    for (int k = 0; k < 9; k++) A.ric[k] = ric[k];
    A.iterations = iterations; A.flags = flags; A.thr2 = threshold * threshold; A.confidence = confidence; A.seed = seed;
    if (on_device) {            // the offsets are device memory: the kernel makes the checks
        A.first = first; A.pts_w = pts_w; A.pts_uv = pts_uv; A.Ps_prev = Ps_prev; A.Rs_prev = Rs_prev;
        A.Ps_out = Ps_out; A.Rs_out = Rs_out; A.n_inliers = n_inliers; A.inlier = inlier; A.best = best; A.n_iters = n_iters; A.info = info;
        A.samples = samples; A.hyp = hyp; A.count = count;
        return swf_internal_pnp_launch(A, st);
    }
    // ---- host memory: the argument errors and the TOO_FEW / BAD_INPUT frames before the device is touched
    if (first[0] < 0) return pnp_fail(SWF_E_INVALID, who + ": a negative point offset");
    for (int i = 0; i < n_frames; i++) {
        if (first[i + 1] < first[i]) return pnp_fail(SWF_E_INVALID, who + ": point offsets must be non-decreasing");
        if (first[i + 1] - first[i] > SWF_PNP_NMAX) return pnp_fail(SWF_E_UNSUPPORTED, who + ": a frame of more than 1024 points");
    }
    const bool as_float = (flags & 1) != 0;
    auto staged_finite = [&](double v) { return std::isfinite(as_float ? (double)(float)v : v); };
    std::vector<int32_t> code((size_t)n_frames);
    int n_go = 0;
    for (int i = 0; i < n_frames; i++) {
        const int n = first[i + 1] - first[i];
        int c = SWF_PNP_OK;
        if (n < 4) c = SWF_PNP_TOO_FEW;
        else {
            bool fin = true;
            for (size_t g = (size_t)first[i] * 3; g < (size_t)first[i + 1] * 3; g++) fin = fin && staged_finite(pts_w[g]);
            for (size_t g = (size_t)first[i] * 2; g < (size_t)first[i + 1] * 2; g++) fin = fin && staged_finite(pts_uv[g]);
            for (int k = 0; k < 3; k++) fin = fin && std::isfinite(Ps_prev[(size_t)i * 3 + k]);
            for (int k = 0; k < 9; k++) fin = fin && std::isfinite(Rs_prev[(size_t)i * 9 + k]);
            if (!fin) c = SWF_PNP_BAD_INPUT;
        }
        code[(size_t)i] = c;
        info[i] = c;
        n_go += c == SWF_PNP_OK;
    }
    if (!n_go) return SWF_OK;

    const size_t nf = (size_t)n_frames, np = (size_t)(first[n_frames] - first[0]), H = (size_t)iterations;
    std::vector<int32_t> rel(first, first + n_frames + 1);
    for (auto& v : rel) v -= first[0];
    // a frame without a model leaves the caller's arrays as they are: the results pass through staging arrays
    std::vector<double> h_po(nf * 3), h_ro(nf * 9), h_h(hyp ? nf * H * 12 : 0);
    std::vector<int32_t> h_ni(nf), h_b(nf), h_it(nf), h_info(nf), h_s(samples ? nf * H * 5 : 0), h_c(count ? nf * H : 0);
    std::vector<uint8_t> h_in(np);
    HostStage S("swf_pnp_frame_batch", st);
    A.first = S.up(rel.data(), rel.size());
    A.pts_w = S.up(pts_w + (size_t)first[0] * 3, np * 3);
    A.pts_uv = S.up(pts_uv + (size_t)first[0] * 2, np * 2);
    A.Ps_prev = S.up(Ps_prev, nf * 3);
    A.Rs_prev = S.up(Rs_prev, nf * 9);
    A.Ps_out = S.out<double>(nf * 3);
    A.Rs_out = S.out<double>(nf * 9);
    A.n_inliers = S.out<int32_t>(nf);
    A.inlier = S.out<uint8_t>(np);
    A.best = S.out<int32_t>(nf);
    A.n_iters = S.out<int32_t>(nf);
    A.info = S.out<int32_t>(nf);
    if (samples) A.samples = S.out<int32_t>(nf * H * 5);
    if (hyp) A.hyp = S.out<double>(nf * H * 12);
    if (count) A.count = S.out<int32_t>(nf * H);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_pnp_launch(A, st);
    if (rc) return rc;
    S.down(h_po.data(), A.Ps_out, h_po.size());
    S.down(h_ro.data(), A.Rs_out, h_ro.size());
    S.down(h_ni.data(), A.n_inliers, h_ni.size());
    S.down(h_in.data(), A.inlier, h_in.size());
    S.down(h_b.data(), A.best, h_b.size());
    S.down(h_it.data(), A.n_iters, h_it.size());
    S.down(h_info.data(), A.info, h_info.size());
    S.down(h_s.data(), A.samples, h_s.size());
    S.down(h_h.data(), A.hyp, h_h.size());
    S.down(h_c.data(), A.count, h_c.size());
    S.sync();
    if (S.failed()) return S.rc();
    for (int i = 0; i < n_frames; i++) {
        const int32_t c = h_info[(size_t)i];
        if (code[(size_t)i] != SWF_PNP_OK) {
            if (c != code[(size_t)i]) return pnp_fail(SWF_E_STATE, who + ": the device classified a frame differently from the host");
            continue;
        }
        info[i] = c;
        if (c != SWF_PNP_OK && c != SWF_PNP_UNREFINED) continue;
        const size_t fi = (size_t)i, rows = first[i + 1] - first[i] >= 5 ? H : 1;
        std::copy(h_po.begin() + fi * 3, h_po.begin() + fi * 3 + 3, Ps_out + fi * 3);
        std::copy(h_ro.begin() + fi * 9, h_ro.begin() + fi * 9 + 9, Rs_out + fi * 9);
        n_inliers[i] = h_ni[fi]; best[i] = h_b[fi]; n_iters[i] = h_it[fi];
        std::copy(h_in.begin() + rel[fi], h_in.begin() + rel[fi + 1], inlier + first[i]);
        if (samples) std::copy(h_s.begin() + fi * H * 5, h_s.begin() + (fi * H + rows) * 5, samples + fi * H * 5);
        if (hyp) std::copy(h_h.begin() + fi * H * 12, h_h.begin() + (fi * H + rows) * 12, hyp + fi * H * 12);
        if (count) std::copy(h_c.begin() + fi * H, h_c.begin() + fi * H + rows, count + fi * H);
    }
    return SWF_OK;
}
