// swf_dev.h — device-side data model of the batch engine (gfx950 / CDNA4 only).
//
// One batch = W independent sliding windows laid out back to back in HBM.  Everything that
// depends only on the windows' STRUCTURE (who observes what, elimination order, which
// reduced block pairs are non-zero) is built once on the host ("symbolic phase") into flat
// index arrays; per solve only the parameter blocks change.  All accumulation orders are
// fixed by these arrays — no floating-point atomics anywhere — so results are run-to-run
// bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swf_types.h"

#define SWF_WAVE 64

#include "swf_records.h"       // WinRec, WinState, GFac, JtRec, Clique, Pair, AsmWin, DevBatch + the limits shared with the symbolic phase

// ------------------------------------------------------------------ device math
// quaternions (x, y, z, w), Hamilton product — same formulas as Eigen, which the reference
// uses (R/factor/*.cpp); see oracle/swf_oracle.c for the CPU restatement.
__device__ __forceinline__ void qmul(const double* a, const double* b, double* o) {
    double ax = a[0], ay = a[1], az = a[2], aw = a[3];
    double bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[3] = aw * bw - ax * bx - ay * by - az * bz;
    o[0] = aw * bx + ax * bw + ay * bz - az * by;
    o[1] = aw * by + ay * bw + az * bx - ax * bz;
    o[2] = aw * bz + az * bw + ax * by - ay * bx;
}
__device__ __forceinline__ void qinv(const double* q, double* o) {
    double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    o[0] = -q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = q[3] / n2;
}
// dx of one kept block of a linear prior, as MarginalizationFactor::Evaluate forms it (R/factor/marginalization_factor.cpp:410-446);
// gs = the block's global size (7 = pose: [p - p0 ; +-2 vec(q0^-1 q)], sign of the scalar part)
__device__ __forceinline__ void prior_block_dx(const double* x, const double* x0, int gs, double* dx) {
    if (gs != 7) { for (int k = 0; k < gs; k++) dx[k] = x[k] - x0[k]; return; }
    dx[0] = x[0] - x0[0]; dx[1] = x[1] - x0[1]; dx[2] = x[2] - x0[2];
    double q0i[4], dq[4];
    qinv(x0 + 3, q0i);
    qmul(q0i, x + 3, dq);
    double sg = (dq[3] >= 0) ? 2.0 : -2.0;
    dx[3] = sg * dq[0]; dx[4] = sg * dq[1]; dx[5] = sg * dq[2];
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void qrot(const double* q, const double* v, double* o) {
    double uv[3], t[3];
    cross3(q, v, uv);
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    cross3(q, uv, t);
    o[0] = v[0] + q[3] * uv[0] + t[0];
    o[1] = v[1] + q[3] * uv[1] + t[1];
    o[2] = v[2] + q[3] * uv[2] + t[2];
}
__device__ __forceinline__ void q2R(const double* q, double* R) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    double twx = tx * w, twy = ty * w, twz = tz * w;
    double txx = tx * x, txy = ty * x, txz = tz * x;
    double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
__device__ __forceinline__ void skew3(const double* v, double* S) {
    S[0] = 0;     S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2];  S[4] = 0;     S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0];  S[8] = 0;
}
__device__ __forceinline__ void mat3mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3T(const double* A, double* T) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[i * 3 + j] = A[j * 3 + i];
}
__device__ __forceinline__ void mat3vec(const double* A, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
__device__ __forceinline__ void qleft_br(const double* q, double* M) {
    skew3(q, M);
    M[0] += q[3]; M[4] += q[3]; M[8] += q[3];
}
__device__ __forceinline__ void qleft_qright_br(const double* a, const double* b, double* M) {
    double L[9], Rr[9], S[9];
    qleft_br(a, L);
    skew3(b, S);
#pragma unroll
    for (int i = 0; i < 9; i++) Rr[i] = -S[i];
    Rr[0] += b[3]; Rr[4] += b[3]; Rr[8] += b[3];
    mat3mul(L, Rr, M);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i * 3 + j] += -a[i] * b[j];
}
// PoseLocalParameterization::Plus (R/factor/pose_local_parameterization.cpp:5-19)
__device__ __forceinline__ void pose_plus(const double* x, const double* d, double* o) {
    o[0] = x[0] + d[0]; o[1] = x[1] + d[1]; o[2] = x[2] + d[2];
    double dq[4] = { d[3] / 2, d[4] / 2, d[5] / 2, 1.0 }, q[4];
    qmul(x + 3, dq, q);
    double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    o[3] = q[0] / n; o[4] = q[1] / n; o[5] = q[2] / n; o[6] = q[3] / n;
}
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// broadcast a double from a compile-time-constant lane through SGPRs (v_readlane_b32 x2)
__device__ __forceinline__ double readlane_d(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane); hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}
// 1/sqrt(x) without the IEEE sqrt/div expansions: v_rsq_f64 (measured 2^-24 relative) + 2 Newton steps
// = 2.2 ulp worst case (a third step gives 1.9; tests/microbench/rsq_f64_accuracy.hip).  Explicit fma under
// contract(off): every inlined copy rounds identically.
__device__ __forceinline__ double rsqrt_nr(double x) {
#pragma clang fp contract(off)
    double y = __builtin_amdgcn_rsq(x), h = 0.5 * x;
    y = y * __builtin_fma(-(h * y), y, 1.5);
    y = y * __builtin_fma(-(h * y), y, 1.5);
    return y;
}
// 1/x: v_rcp_f64 + 2 Newton steps (same accuracy class as rsqrt_nr)
__device__ __forceinline__ double rcp_nr(double x) {
#pragma clang fp contract(off)
    double r = __builtin_amdgcn_rcp(x);
    r = r * __builtin_fma(-x, r, 2.0);
    r = r * __builtin_fma(-x, r, 2.0);
    return r;
}
// value of lane (i + N) mod 16 of the same 16-lane row, through the DPP row-rotate path (no LDS crossbar).
// On a value that is already symmetric under the coarser exchanges this equals the xor-N butterfly partner.
template <int N>
__device__ __forceinline__ double row_ror(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x120 + N, 0xf, 0xf, false);
    hi = __builtin_amdgcn_mov_dpp(hi, 0x120 + N, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// all-reduce over the 16 lanes of a row: the butterfly 8, 4, 2, 1 (fixed order => deterministic)
__device__ __forceinline__ double grp16_sum(double v) {
    v += row_ror<8>(v); v += row_ror<4>(v); v += row_ror<2>(v); v += row_ror<1>(v);
    return v;
}
// maximum over the 16-lane row, every lane of the row ends with it (DPP row rotations)
__device__ __forceinline__ double grp16_max(double v) {
    v = fmax(v, row_ror<8>(v)); v = fmax(v, row_ror<4>(v)); v = fmax(v, row_ror<2>(v)); v = fmax(v, row_ror<1>(v));
    return v;
}
// the value lane L holds, as a wave-uniform number (v_readlane)
__device__ __forceinline__ double rows_lane(double v, int L) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), L), __builtin_amdgcn_readlane(__double2loint(v), L));
}
// sum over the four 16-lane rows of a value that is already uniform inside each row (after grp16_sum): v_readlane of lanes 0, 16, 32
// and 48, no LDS crossbar; the result is wave-uniform.  ((row 0 + row 1) + (row 2 + row 3))
__device__ __forceinline__ double rows4_sum(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const double a0 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
    const double a1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
    const double a2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
    const double a3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
    return (a0 + a1) + (a2 + a3);
}
// wave-level all-reduce (butterfly 32, 16, 8, 4, 2, 1: every lane ends with the total)
__device__ __forceinline__ double wave_sum(double v) {
    v += __shfl_xor(v, 32, 64); v += __shfl_xor(v, 16, 64);
    return grp16_sum(v);
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
// block-level sum for blockDim.x = multiple of 64 (<= 1024); scratch >= 16 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    v = wave_sum(v);
    int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[wid] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < nw; i++) s += scratch[i];
    return s;
}
// several block-level reductions behind ONE barrier pair: v[0..NS) are summed, v[NS..NS+NM) maximised; every
// thread gets all results.  Same order as block_sum / block_max (wave butterfly, then waves in order).
// scratch >= 16 * (NS + NM) doubles of LDS.
template <int NS, int NM>
__device__ __forceinline__ void block_reduce(double* v, double* scratch) {
#pragma unroll
    for (int k = 0; k < NS; k++) v[k] = wave_sum(v[k]);
#pragma unroll
    for (int k = 0; k < NM; k++) v[NS + k] = wave_max(v[NS + k]);
    int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS + NM; k++) scratch[k * 16 + wid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; k++) { double s = 0; for (int i = 0; i < nw; i++) s += scratch[k * 16 + i]; v[k] = s; }
#pragma unroll
    for (int k = 0; k < NM; k++) { double s = scratch[(NS + k) * 16]; for (int i = 1; i < nw; i++) s = scratch[(NS + k) * 16 + i] > s ? scratch[(NS + k) * 16 + i] : s; v[NS + k] = s; }
}
__device__ __forceinline__ double block_max(double v, double* scratch) {
    v = wave_max(v);
    int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[wid] = v;
    __syncthreads();
    double s = scratch[0];
    for (int i = 1; i < nw; i++) s = scratch[i] > s ? scratch[i] : s;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Inverse-depth projection factors, one evaluation:
//   kind 0 ProjectionTwoFrameOneCamFactor (R/factor/projection_factor.cpp:179-256), 1 ProjectionTwoFrameTwoCamFactor (:77-166),
//   kind 2 ProjectionOneFrameTwoCamFactor (:269-329; Pi = Pj = identity pose, no lever arm).  e2 = the camera projected into
//   (= ex for kind 0).  J (if jac): d r / d pose_i (2x6 local, row-major) | pose_j | ex | ex2 | lambda (2) = 50 doubles.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void red_out(const double* red, const double* Mx, double sgn, double* Jd, int col) {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Jd[i * 6 + col + j] = sgn * (red[i * 3] * Mx[j] + red[i * 3 + 1] * Mx[3 + j] + red[i * 3 + 2] * Mx[6 + j]);
}

__device__ __forceinline__ void d_idepth_eval(int kind, const double* Pi, const double* Pj, const double* ex, const double* e2, double inv_dep,
                                              const double* pts, double si, const double* pbg, double* r, double* Jq, bool jac) {
    const double* pts_i = pts; const double* pts_j = pts + 3;
    const double lever[3] = { kind == 2 ? 0.0 : pbg[0], kind == 2 ? 0.0 : pbg[1], kind == 2 ? 0.0 : pbg[2] };
    double pci[3] = { pts_i[0] / inv_dep, pts_i[1] / inv_dep, pts_i[2] / inv_dep }, pimu_i[3], pimu_j[3], t[3], pcj[3], qi[4], w[3];
    qrot(ex + 3, pci, pimu_i);
#pragma unroll
    for (int k = 0; k < 3; k++) pimu_i[k] += ex[k] - lever[k];
    if (kind == 2) { pimu_j[0] = pimu_i[0]; pimu_j[1] = pimu_i[1]; pimu_j[2] = pimu_i[2]; }
    else {
        qrot(Pi + 3, pimu_i, w);
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] += Pi[k] - Pj[k];
        qinv(Pj + 3, qi); qrot(qi, w, pimu_j);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = pimu_j[k] + lever[k] - e2[k];
    qinv(e2 + 3, qi); qrot(qi, t, pcj);
    const double dep = pcj[2];
    r[0] = si * (pcj[0] / dep - pts_j[0]);
    r[1] = si * (pcj[1] / dep - pts_j[1]);
    if (!jac) return;
    double red[6] = { si * (1. / dep), 0, si * (-pcj[0] / (dep * dep)), 0, si * (1. / dep), si * (-pcj[1] / (dep * dep)) };
    double Ri[9], Rj[9], ric[9], ric2[9], ric2T[9], RjT[9], Am[9], Bm[9], Cm[9], S[9], M[9];
    q2R(ex + 3, ric); q2R(e2 + 3, ric2); mat3T(ric2, ric2T);
    q2R(Pi + 3, Ri); q2R(Pj + 3, Rj);                   // identities for kind 2
    mat3T(Rj, RjT);
    mat3mul(ric2T, RjT, Am); mat3mul(Am, Ri, Bm); mat3mul(Bm, ric, Cm);
    for (int k = 0; k < 50; k++) Jq[k] = 0.0;
    if (kind != 2) {
        skew3(pimu_i, S); mat3mul(Bm, S, M);
        red_out(red, Am, 1.0, Jq, 0); red_out(red, M, -1.0, Jq, 3);
        skew3(pimu_j, S); mat3mul(ric2T, S, M);
        red_out(red, Am, -1.0, Jq + 12, 0); red_out(red, M, 1.0, Jq + 12, 3);
    }
    if (kind == 0) {
        double T1[9], tmp[3], v[3], w2[3], u[3], S2[9], S3[9], L[9];
#pragma unroll
        for (int k = 0; k < 9; k++) T1[k] = Bm[k] - ric2T[k];
        mat3vec(Cm, pci, tmp);
        skew3(pci, S); mat3mul(Cm, S, L); skew3(tmp, S2);
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = ex[k] - pbg[k];
        mat3vec(Ri, v, w2);
#pragma unroll
        for (int k = 0; k < 3; k++) w2[k] += Pi[k] - Pj[k];
        mat3vec(RjT, w2, u);
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] += pbg[k] - ex[k];
        mat3vec(ric2T, u, v); skew3(v, S3);
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = -L[k] + S2[k] + S3[k];
        red_out(red, T1, 1.0, Jq + 24, 0); red_out(red, M, 1.0, Jq + 24, 3);
    } else {
        skew3(pci, S); mat3mul(Cm, S, M);
        red_out(red, Bm, 1.0, Jq + 24, 0); red_out(red, M, -1.0, Jq + 24, 3);
        skew3(pcj, S);
        red_out(red, ric2T, -1.0, Jq + 36, 0); red_out(red, S, 1.0, Jq + 36, 3);
    }
    double v3[3];
    mat3vec(Cm, pts_i, v3);
#pragma unroll
    for (int i = 0; i < 2; i++) Jq[48 + i] = (red[i * 3] * v3[0] + red[i * 3 + 1] * v3[1] + red[i * 3 + 2] * v3[2]) * -1.0 / (inv_dep * inv_dep);
}
