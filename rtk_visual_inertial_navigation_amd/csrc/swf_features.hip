// swf_features.hip — k_feature_err / k_feature_compact (the post-solve feature check, see swf_features.h) and the symbolic phase
// that builds their observation table from the flat windows.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "swf_features.h"

void swf_internal_set_error(const std::string& m);
static int ft_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

// ------------------------------------------------------------------ device
namespace {
// a pose block [p(3) qx qy qz qw] at state index xi; xi < 0 = the identity
__device__ __forceinline__ void ft_load_pose(const double* __restrict__ x, int xi, double q[7]) {
    if (xi < 0) { q[0] = q[1] = q[2] = q[3] = q[4] = q[5] = 0.0; q[6] = 1.0; return; }
#pragma unroll
    for (int k = 0; k < 7; k++) q[k] = x[xi + k];
}
// rotation of the NORMALISED quaternion (Quaterniond(w, x, y, z).normalized().toRotationMatrix(), R/swf/swf.cpp:192), row-major
__device__ __forceinline__ void ft_rot(const double q7[7], double R[9]) {
    const double nn = sqrt(q7[3] * q7[3] + q7[4] * q7[4] + q7[5] * q7[5] + q7[6] * q7[6]);
    const double x = q7[3] / nn, y = q7[4] / nn, z = q7[5] / nn, w = q7[6] / nn;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
__device__ __forceinline__ void ft_mul(const double R[9], const double v[3], double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
}
__device__ __forceinline__ void ft_mulT(const double R[9], const double v[3], double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = R[r] * v[0] + R[3 + r] * v[1] + R[6 + r] * v[2];
}
}  // namespace

// One lane per observation over a block of whole features of one window (a track longer than FEAT_BLK: one workgroup, several
// chunks).  Loads go out by dependency level: the record, then every state value it names.  Each lane leaves its error in LDS;
// thread t then adds the run of the block's t-th feature left to right — a fixed order, no atomics — and writes the feature's row.
__global__ void __launch_bounds__(FEAT_BLK) k_feature_err(FeatArgs A) {
    __shared__ double s_err[FEAT_BLK];
    __shared__ double s_z[FEAT_BLK];          // pc.z (world point) / lambda (inverse depth) of the observation
    __shared__ unsigned char s_idp[FEAT_BLK];
    const int4 B = A.blk[blockIdx.x];
    const int win = B.x, f0 = B.y, nf = B.z - B.y, tid = threadIdx.x;
    const int o0 = A.f_obs0[f0], o1 = A.f_obs0[B.z];
    const double pbg[3] = { A.w_cst[4 * win], A.w_cst[4 * win + 1], A.w_cst[4 * win + 2] };
    const double sqrt_info = A.w_cst[4 * win + 3];
    const double* __restrict__ x = A.x;
    int r0 = 0, r1 = 0;
    if (tid < nf) { r0 = A.f_obs0[f0 + tid]; r1 = A.f_obs0[f0 + tid + 1]; }
    double acc = 0.0, zfirst = 0.0; bool idp_f = false;
    for (int c0 = o0; c0 == o0 || c0 < o1; c0 += FEAT_BLK) {
        const int o = c0 + tid;
        if (o < o1) {
            // level 1: the record
            const int4 a = A.o_a[o]; const int2 b = A.o_b[o]; const double2 uv = A.o_uv[o];
            // level 2: the state values (17 for a world point)
            double pj[7], pe[7];
            ft_load_pose(x, a.x, pj); ft_load_pose(x, a.y, pe);
            double X[3], zval;
            if (b.x < 0) {
                X[0] = x[a.z]; X[1] = x[a.z + 1]; X[2] = x[a.z + 2];
                zval = 0.0;
            } else {
                // X = R_i (R_ex (pts_i / lambda) + t_ex - pbg) + p_i   (R/swf/swf_image.cpp:275-277)
                double pi[7], pa[7];
                ft_load_pose(x, a.w, pi); ft_load_pose(x, b.x, pa);
                const double lam = x[a.z];
                const double* pt = A.f_pi + 3 * (size_t)b.y;
                const double pc0[3] = { pt[0] / lam, pt[1] / lam, pt[2] / lam };
                double Ra[9], Ri[9], v[3], u[3];
                ft_rot(pa, Ra); ft_rot(pi, Ri);
                ft_mul(Ra, pc0, v);
                for (int k = 0; k < 3; k++) v[k] = v[k] + pa[k] - pbg[k];
                ft_mul(Ri, v, u);
                for (int k = 0; k < 3; k++) X[k] = u[k] + pi[k];
                zval = lam;
            }
            // P_j = p_j - R_j pbg;  pc = R_e^T (R_j^T (X - P_j) - t_e)   (ReprojectionError, R/swf/swf_image.cpp:255-261)
            double Rj[9], Re[9], t[3], P[3], d[3], bj[3], pc[3];
            ft_rot(pj, Rj); ft_rot(pe, Re);
            ft_mul(Rj, pbg, t);
            for (int k = 0; k < 3; k++) { P[k] = pj[k] - t[k]; d[k] = X[k] - P[k]; }
            ft_mulT(Rj, d, bj);
            for (int k = 0; k < 3; k++) bj[k] -= pe[k];
            ft_mulT(Re, bj, pc);
            const double rx = pc[0] / pc[2] - uv.x, ry = pc[1] / pc[2] - uv.y;
            s_err[tid] = sqrt(rx * rx + ry * ry);
            s_z[tid] = b.x < 0 ? pc[2] : zval;
            s_idp[tid] = b.x < 0 ? 0 : 1;
        }
        __syncthreads();
        if (tid < nf) {
            const int ka = max(r0, c0), kb = min(r1, c0 + FEAT_BLK);
            if (r0 >= c0 && r0 < kb) { zfirst = s_z[r0 - c0]; idp_f = s_idp[r0 - c0] != 0; }
            for (int k = ka; k < kb; k++) acc += s_err[k - c0];
        }
        __syncthreads();
    }
    if (tid < nf) {
        const int f = f0 + tid, n = r1 - r0;
        double mean = 0.0, depth = 0.0; unsigned fl = SWF_FEAT_UNOBSERVED;
        if (n > 0) {
            mean = acc / (double)n;
            depth = idp_f ? 1.0 / zfirst : zfirst;
            fl = 0;
            if (mean * sqrt_info > A.thr) fl |= SWF_FEAT_OUTLIER;
            if (zfirst < 0.0) fl |= SWF_FEAT_NEG_DEPTH;          // depth < 0 (world point) / lambda < 0 (inverse depth)
        }
        A.mean_err[f] = mean; A.depth[f] = depth; A.n_obs[f] = n; A.flags[f] = (unsigned char)fl;
    }
}

// One wavefront per window: the indices of its rejected features, ascending, by ballot + popcount prefix.
__global__ void __launch_bounds__(64) k_feature_compact(FeatArgs A) {
    const int win = blockIdx.x, lane = threadIdx.x;
    const int fa = A.w_feat0[win], fb = A.w_feat0[win + 1];
    int count = 0;
    for (int f = fa; f < fb; f += 64) {
        const bool rej = f + lane < fb && (A.flags[f + lane] & (SWF_FEAT_OUTLIER | SWF_FEAT_NEG_DEPTH)) != 0;
        const unsigned long long m = __ballot(rej);
        if (rej) A.rejected[fa + count + __popcll(m & ((1ULL << lane) - 1ULL))] = f + lane - fa;
        count += __popcll(m);
    }
    if (lane == 0) A.n_rejected[win] = count;
}

int swf_internal_feature_launch(const FeatArgs& A, hipStream_t st) {
    if (A.n_blk > 0) hipLaunchKernelGGL(k_feature_err, dim3(A.n_blk), dim3(FEAT_BLK), 0, st, A);
    if (A.n_win > 0) hipLaunchKernelGGL(k_feature_compact, dim3(A.n_win), dim3(64), 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(SWF_E_NODEVICE, std::string("k_feature_err / k_feature_compact: ") + hipGetErrorString(e));
    return SWF_OK;
}

// ------------------------------------------------------------------ symbolic phase
int swf_internal_feature_tables(const std::vector<FeatWinSrc>& src, FeatTables& T) {
    T = FeatTables{};
    T.w_feat0.push_back(0);
    for (size_t wi = 0; wi < src.size(); wi++) {
        const FeatWinSrc& w = src[wi];
        const int xP = w.x_base, xL = w.x_base + 7 * w.n_pose + 9 * w.n_sb, xC = xL + 3 * w.n_lm;
        auto xpose = [&](int p) { return xP + 7 * p; };
        const int n_proj = (int)w.proj_idx.size() / 3, n_idp = (int)w.idp_kind.size();
        const int feat_w0 = (int)T.f_obs0.size();
        // world points: the projection factors of landmark l, in the caller's order
        std::vector<int> first(w.n_lm + 1, 0), slot(n_proj);
        for (int i = 0; i < n_proj; i++) first[w.proj_idx[3 * i + 2] + 1]++;
        for (int l = 0; l < w.n_lm; l++) first[l + 1] += first[l];
        {
            std::vector<int> fill(first.begin(), first.end() - 1);
            for (int i = 0; i < n_proj; i++) slot[fill[w.proj_idx[3 * i + 2]]++] = i;
        }
        for (int l = 0; l < w.n_lm; l++) {
            const int f = (int)T.f_obs0.size();
            T.f_obs0.push_back((int)T.o_a.size());
            T.f_pi.insert(T.f_pi.end(), 3, 0.0);
            for (int q = first[l]; q < first[l + 1]; q++) {
                const int i = slot[q];
                T.o_a.push_back(make_int4(xpose(w.proj_idx[3 * i]), xpose(w.proj_idx[3 * i + 1]), xL + 3 * l, -1));
                T.o_b.push_back(make_int2(-1, f));
                T.o_uv.push_back(make_double2(w.proj_uv[2 * i], w.proj_uv[2 * i + 1]));
            }
        }
        // inverse depths: the distinct scalar blocks the factors name, ascending; the anchor's own observation first (the
        // reference's loop starts at start_frame), then the factors in the caller's order
        std::vector<int> lams;
        for (int i = 0; i < n_idp; i++) lams.push_back(w.idp_idx[5 * i + 4]);
        std::sort(lams.begin(), lams.end());
        lams.erase(std::unique(lams.begin(), lams.end()), lams.end());
        std::vector<std::vector<int>> fac(lams.size());
        for (int i = 0; i < n_idp; i++)
            fac[std::lower_bound(lams.begin(), lams.end(), w.idp_idx[5 * i + 4]) - lams.begin()].push_back(i);
        for (size_t k = 0; k < lams.size(); k++) {
            const int f = (int)T.f_obs0.size();
            T.f_obs0.push_back((int)T.o_a.size());
            const int i0 = fac[k][0];
            const double* pts_i = &w.idp_pts[6 * (size_t)i0];
            int anchor = -1;
            for (int i : fac[k]) if (w.idp_kind[i] != 2) { anchor = w.idp_idx[5 * i]; break; }
            for (int i : fac[k]) {
                const double* q = &w.idp_pts[6 * (size_t)i];
                if (q[0] != pts_i[0] || q[1] != pts_i[1] || q[2] != pts_i[2] || (w.idp_kind[i] != 2 && w.idp_idx[5 * i] != anchor))
                    return ft_fail(SWF_E_INVALID, "feature check: the factors of inverse depth " + std::to_string(lams[k]) + " of window " +
                                   std::to_string(wi) + " disagree on the anchor (pose_i, pts_i)");
            }
            T.f_pi.insert(T.f_pi.end(), pts_i, pts_i + 3);
            const int xi = anchor >= 0 ? xpose(anchor) : -1, xlam = xC + lams[k], xa0 = xpose(w.idp_idx[5 * i0 + 2]);
            T.o_a.push_back(make_int4(xi, xa0, xlam, xi)); T.o_b.push_back(make_int2(xa0, f)); T.o_uv.push_back(make_double2(pts_i[0], pts_i[1]));
            for (int i : fac[k]) {
                const int* ix = &w.idp_idx[5 * i]; const int kd = w.idp_kind[i];
                const int xj = kd == 2 ? xi : xpose(ix[1]), xe = kd == 0 ? xpose(ix[2]) : xpose(ix[3]);
                T.o_a.push_back(make_int4(xj, xe, xlam, xi)); T.o_b.push_back(make_int2(xpose(ix[2]), f));
                T.o_uv.push_back(make_double2(w.idp_pts[6 * (size_t)i + 3], w.idp_pts[6 * (size_t)i + 4]));
            }
        }
        // workgroups: whole features, at most FEAT_BLK observations and FEAT_BLK features; a longer track alone
        const int feat_w1 = (int)T.f_obs0.size();
        T.f_obs0.push_back((int)T.o_a.size());          // (sentinel, removed below)
        int fs = feat_w0, cnt = 0;
        for (int f = feat_w0; f < feat_w1; f++) {
            const int n = T.f_obs0[f + 1] - T.f_obs0[f];
            if (f > fs && (cnt + n > FEAT_BLK || f - fs == FEAT_BLK)) { T.blk.push_back(make_int4((int)wi, fs, f, 0)); fs = f; cnt = 0; }
            cnt += n;
        }
        if (feat_w1 > fs) T.blk.push_back(make_int4((int)wi, fs, feat_w1, 0));
        T.f_obs0.pop_back();
        T.w_feat0.push_back(feat_w1);
        T.w_cst.insert(T.w_cst.end(), w.pbg, w.pbg + 3); T.w_cst.push_back(w.sqrt_info);
    }
    T.f_obs0.push_back((int)T.o_a.size());
    return SWF_OK;
}
