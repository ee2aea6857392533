// The host loop bench_imu_frame.py times against the device: what swf_imu_frame_batch does per frame as plain C++ over
// host arrays: the sample cut, the mid-point prediction, and the pre-integration recursion with its dense 15x15 Jacobian and covariance
// updates (jacobian = F jacobian, covariance = F cov F^T + V Q V^T), as a host estimator runs it per sample.  The final square-root
// information is left out (it is formed when the factor is evaluated).  Same inputs; pred [n][15], and per frame delta_p, delta_q,
// delta_v, sum_dt and the covariance in dpqv_cov [n][11 + 225].  Built by the script with g++ -O3.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {
typedef double M15[15][15];
void mv3(const double* R, const double* x, double* o) { for (int a = 0; a < 3; a++) o[a] = R[3 * a] * x[0] + R[3 * a + 1] * x[1] + R[3 * a + 2] * x[2]; }
void mm3(const double* A, const double* B, double* Cm) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Cm[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
void q2R(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
void skew(const double* v, double* S) { S[0] = 0; S[1] = -v[2]; S[2] = v[1]; S[3] = v[2]; S[4] = 0; S[5] = -v[0]; S[6] = -v[1]; S[7] = v[0]; S[8] = 0; }
void qmul(const double* a, const double* b, double* o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
void put3(double F[15][18], int r, int c, const double* B, double s) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) F[r + i][c + j] = s * B[3 * i + j]; }

struct Pre {
    double dp[3], dq[4], dv[3], sum_dt, acc0[3], gyr0[3], ba[3], bg[3];
    M15 jac, cov;
    void push(double dt, const double* acc1, const double* gyr1, const double* n2) {
        double a0[3], a1[3], w[3], R0[9], R1[9], u0[3], u1[3], hq[4], rq[4];
        for (int k = 0; k < 3; k++) { a0[k] = acc0[k] - ba[k]; a1[k] = acc1[k] - ba[k]; w[k] = 0.5 * (gyr0[k] + gyr1[k]) - bg[k]; hq[k] = w[k] * dt / 2; }
        hq[3] = 1;
        q2R(dq, R0); mv3(R0, a0, u0);
        qmul(dq, hq, rq); q2R(rq, R1); mv3(R1, a1, u1);
        double Rw[9], Ra0[9], Ra1[9], M0[9], M1[9], M2[9], ImRw[9], I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, Ms[9], Rs[9];
        skew(w, Rw); skew(a0, Ra0); skew(a1, Ra1);
        for (int i = 0; i < 9; i++) ImRw[i] = I3[i] - Rw[i] * dt;
        mm3(R0, Ra0, M0); mm3(R1, Ra1, M1); mm3(M1, ImRw, M2);
        for (int i = 0; i < 9; i++) { Ms[i] = M0[i] + M2[i]; Rs[i] = R0[i] + R1[i]; }
        static double F[15][18], V[15][18];
        std::memset(F, 0, sizeof F); std::memset(V, 0, sizeof V);
        for (int i = 0; i < 15; i++) F[i][i] = 1;
        put3(F, 0, 3, Ms, -0.25 * dt * dt); put3(F, 0, 6, I3, dt); put3(F, 0, 9, Rs, -0.25 * dt * dt); put3(F, 0, 12, M1, 0.25 * dt * dt * dt);
        put3(F, 3, 3, ImRw, 1); put3(F, 3, 12, I3, -dt);
        put3(F, 6, 3, Ms, -0.5 * dt); put3(F, 6, 9, Rs, -0.5 * dt); put3(F, 6, 12, M1, 0.5 * dt * dt);
        put3(V, 0, 0, R0, 0.25 * dt * dt); put3(V, 0, 3, M1, -0.125 * dt * dt * dt); put3(V, 0, 6, R1, 0.25 * dt * dt); put3(V, 0, 9, M1, -0.125 * dt * dt * dt);
        put3(V, 3, 3, I3, 0.5 * dt); put3(V, 3, 9, I3, 0.5 * dt);
        put3(V, 6, 0, R0, 0.5 * dt); put3(V, 6, 3, M1, -0.25 * dt * dt); put3(V, 6, 6, R1, 0.5 * dt); put3(V, 6, 9, M1, -0.25 * dt * dt);
        put3(V, 9, 12, I3, dt); put3(V, 12, 15, I3, dt);
        M15 T, T2;
        for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) { double s = 0; for (int k = 0; k < 15; k++) s += F[i][k] * jac[k][j]; T[i][j] = s; }
        std::memcpy(jac, T, sizeof T);
        for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) { double s = 0; for (int k = 0; k < 15; k++) s += F[i][k] * cov[k][j]; T[i][j] = s; }
        for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) { double s = 0; for (int k = 0; k < 15; k++) s += T[i][k] * F[j][k]; T2[i][j] = s; }
        for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) { double s = 0; for (int k = 0; k < 18; k++) s += V[i][k] * n2[k / 3] * V[j][k]; cov[i][j] = T2[i][j] + s; }
        for (int k = 0; k < 3; k++) {
            const double un = 0.5 * (u0[k] + u1[k]);
            dp[k] += dv[k] * dt + 0.5 * un * dt * dt; dv[k] += un * dt; acc0[k] = acc1[k]; gyr0[k] = gyr1[k];
        }
        const double nq = std::sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
        for (int k = 0; k < 4; k++) dq[k] = rq[k] / nq;
        sum_dt += dt;
    }
};
}  // namespace

extern "C" void imu_frame_host(int32_t n_frames, const double* raw, const int32_t* first, const double* t01, const double* seed,
                               const double* state, const double* gyrj_prev, const int32_t* flags, const double* pbg, const double* gw,
                               const double* noise, double* pred, double* dpqv_cov) {
    const double n2[6] = { noise[0] * noise[0], noise[1] * noise[1], noise[0] * noise[0], noise[1] * noise[1], noise[2] * noise[2], noise[3] * noise[3] };
    static Pre pre;
    for (int f = 0; f < n_frames; f++) {
        const double* rw = raw + (size_t)first[f] * 7;
        const int n = first[f + 1] - first[f];
        const double* x = state + (size_t)f * 21;
        const double t1 = t01[2 * f + 1];
        double P[3], R[9], V[3], ba[3], bg[3], acc0[3], gyr0[3], tmp[3], y[3], cr[3], tc = t01[2 * f], la[6] = { 0, 0, 0, 0, 0, 0 };
        for (int k = 0; k < 3; k++) { P[k] = x[k]; V[k] = x[12 + k]; ba[k] = x[15 + k]; bg[k] = x[18 + k]; acc0[k] = seed[6 * f + k]; gyr0[k] = seed[6 * f + 3 + k]; }
        for (int k = 0; k < 9; k++) R[k] = x[3 + k];
        std::memset(&pre, 0, sizeof pre);
        pre.dq[3] = 1;
        for (int k = 0; k < 15; k++) pre.jac[k][k] = 1;
        for (int k = 0; k < 3; k++) { pre.acc0[k] = acc0[k]; pre.gyr0[k] = gyr0[k]; pre.ba[k] = ba[k]; pre.bg[k] = bg[k]; }
        mv3(R, pbg, tmp);
        for (int k = 0; k < 3; k++) { P[k] -= tmp[k]; y[k] = gyrj_prev[3 * f + k] - bg[k]; }
        if (flags[f] & 1) {
            cr[0] = y[1] * pbg[2] - y[2] * pbg[1]; cr[1] = y[2] * pbg[0] - y[0] * pbg[2]; cr[2] = y[0] * pbg[1] - y[1] * pbg[0];
            mv3(R, cr, tmp);
            for (int k = 0; k < 3; k++) V[k] -= tmp[k];
        }
        for (int i = 0; i < n; i++) {
            const double t = rw[7 * i];
            double dt, s[6];
            if (t <= t1) { dt = t - tc; tc = t; for (int k = 0; k < 6; k++) s[k] = la[k] = rw[7 * i + 1 + k]; }
            else {
                const double d1 = t1 - tc, d2 = t - t1, w1 = d2 / (d1 + d2), w2 = d1 / (d1 + d2);
                dt = d1; tc = t1;
                for (int k = 0; k < 6; k++) s[k] = w1 * la[k] + w2 * rw[7 * i + 1 + k];
            }
            pre.push(dt, s, s + 3, n2);
            double a0[3], a1[3], u0[3], u1[3], hq[4], M[9], Rn[9];
            for (int k = 0; k < 3; k++) { a0[k] = acc0[k] - ba[k]; a1[k] = s[k] - ba[k]; hq[k] = (0.5 * (gyr0[k] + s[3 + k]) - bg[k]) * dt / 2; }
            hq[3] = 1;
            mv3(R, a0, u0); q2R(hq, M); mm3(R, M, Rn); mv3(Rn, a1, u1);
            for (int k = 0; k < 3; k++) {
                const double un = 0.5 * ((u0[k] - gw[k]) + (u1[k] - gw[k]));
                P[k] += dt * V[k] + 0.5 * dt * dt * un; V[k] += dt * un; acc0[k] = s[k]; gyr0[k] = s[3 + k];
            }
            std::memcpy(R, Rn, sizeof Rn);
            if (t > t1) break;
        }
        mv3(R, pbg, tmp);
        for (int k = 0; k < 3; k++) { P[k] += tmp[k]; y[k] = gyr0[k] - bg[k]; }
        if (flags[f] & 1) {
            cr[0] = y[1] * pbg[2] - y[2] * pbg[1]; cr[1] = y[2] * pbg[0] - y[0] * pbg[2]; cr[2] = y[0] * pbg[1] - y[1] * pbg[0];
            mv3(R, cr, tmp);
            for (int k = 0; k < 3; k++) V[k] += tmp[k];
        }
        double* o = pred + (size_t)f * 15;
        for (int k = 0; k < 3; k++) { o[k] = P[k]; o[12 + k] = V[k]; }
        for (int k = 0; k < 9; k++) o[3 + k] = R[k];
        double* d = dpqv_cov + (size_t)f * 236;
        for (int k = 0; k < 3; k++) { d[k] = pre.dp[k]; d[7 + k] = pre.dv[k]; }
        for (int k = 0; k < 4; k++) d[3 + k] = pre.dq[k];
        d[10] = pre.sum_dt;
        std::memcpy(d + 11, pre.cov, sizeof pre.cov);
    }
}
