// SWFOptimization::ImuIntegrate (R/swf/swf_imu.cpp:117-177) bound to the device through swf_ceres::ImuIntegrate, on vector and matrix
// types with Eigen's operator() access and on the vector<pair<double, V3>> pairs GetImuInterval returns.  One frame of six samples,
// the last beyond cur_time.  The propagated P / R / V are compared with a plain restatement of the loop in this file, and the record
// with what the frame fixes (sum_dt, gyri, gyrj).  Prints the values and "imu frame ok"; exit status 1 when the call fails (e.g.
// without a GPU) or a comparison does.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>
#include "swf_ceres.hpp"

struct V3 { double v[3]; double& operator()(int i) { return v[i]; } double operator()(int i) const { return v[i]; } };
struct M3 { double m[9]; double& operator()(int i, int j) { return m[3 * i + j]; } double operator()(int i, int j) const { return m[3 * i + j]; } };
typedef std::vector<std::pair<double, V3> > Pairs;

static void mv(const M3& R, const double* x, double* o) { for (int a = 0; a < 3; a++) o[a] = R(a, 0) * x[0] + R(a, 1) * x[1] + R(a, 2) * x[2]; }

int main() {
    const double t0 = 10.0, t1 = 10.0125, noise[4] = { 0.05, 0.005, 0.0005, 0.00005 };
    Pairs acc, gyr;
    for (int i = 0; i < 6; i++) {
        const double t = t0 + 0.0025 * (i + 1) - 0.001;                    // 10.0015 .. 10.0140: the last one is beyond t1
        V3 a = { { 0.3 + 0.01 * i, -0.2 + 0.02 * i, 9.7 + 0.03 * i } }, w = { { 0.10 - 0.01 * i, 0.05 + 0.01 * i, -0.20 + 0.005 * i } };
        acc.push_back(std::make_pair(t, a)); gyr.push_back(std::make_pair(t, w));
    }
    V3 acc_0 = { { 0.29, -0.21, 9.69 } }, gyr_0 = { { 0.11, 0.04, -0.21 } }, P = { { 12.0, -7.0, 3.0 } }, V = { { 1.5, -0.5, 0.25 } };
    V3 Ba = { { 0.02, -0.01, 0.03 } }, Bg = { { 0.001, -0.002, 0.0015 } }, gprev = { { 0.12, 0.03, -0.22 } };
    V3 Pbg = { { -0.005, 0.009, 0.31 } }, gw = { { 0.0, 0.0, 9.8 } };
    M3 R = { { 0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6 } };
    const V3 seed_a = acc_0, seed_w = gyr_0, P0 = P, V0 = V;
    const M3 R0 = R;
    swf_ceres::ImuFrameResult out;
    if (!swf_ceres::ImuIntegrate(acc, gyr, t0, t1, acc_0, gyr_0, P, R, V, Ba, Bg, gprev, true, Pbg, gw, noise, &out)) {
        std::printf("imu frame failed (info %d)\n", out.info);
        return 1;
    }
    // the loop again, in plain C++
    double p[3], v[3], x[3], y[3], a0[3], w0[3], tc = t0, la[3] = { 0, 0, 0 }, lw[3] = { 0, 0, 0 };
    M3 r = R0;
    mv(r, Pbg.v, x);
    for (int k = 0; k < 3; k++) { p[k] = P0(k) - x[k]; v[k] = V0(k); a0[k] = seed_a(k); w0[k] = seed_w(k); y[k] = gprev(k) - Bg(k); }
    const double c0[3] = { y[1] * Pbg(2) - y[2] * Pbg(1), y[2] * Pbg(0) - y[0] * Pbg(2), y[0] * Pbg(1) - y[1] * Pbg(0) };
    mv(r, c0, x);
    for (int k = 0; k < 3; k++) v[k] -= x[k];
    int steps = 0;
    for (size_t i = 0; i < acc.size(); i++) {
        const double t = acc[i].first;
        double dt, a[3], w[3];
        if (t <= t1) {
            dt = t - tc; tc = t;
            for (int k = 0; k < 3; k++) { a[k] = la[k] = acc[i].second(k); w[k] = lw[k] = gyr[i].second(k); }
        } else {
            const double d1 = t1 - tc, d2 = t - t1, w1 = d2 / (d1 + d2), w2 = d1 / (d1 + d2);
            dt = d1; tc = t1;
            for (int k = 0; k < 3; k++) { a[k] = w1 * la[k] + w2 * acc[i].second(k); w[k] = w1 * lw[k] + w2 * gyr[i].second(k); }
        }
        double d0[3], d1v[3], u0[3], u1[3], h[3];
        for (int k = 0; k < 3; k++) { d0[k] = a0[k] - Ba(k); d1v[k] = a[k] - Ba(k); h[k] = (0.5 * (w0[k] + w[k]) - Bg(k)) * dt / 2; }
        mv(r, d0, u0);
        const double qx = h[0], qy = h[1], qz = h[2];                       // toRotationMatrix of the unnormalised (1, theta / 2)
        const M3 M = { { 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz), 2 * (qx * qz + qy), 2 * (qx * qy + qz), 1 - 2 * (qx * qx + qz * qz),
                         2 * (qy * qz - qx), 2 * (qx * qz - qy), 2 * (qy * qz + qx), 1 - 2 * (qx * qx + qy * qy) } };
        M3 rn;
        for (int i2 = 0; i2 < 3; i2++) for (int j = 0; j < 3; j++) rn(i2, j) = r(i2, 0) * M(0, j) + r(i2, 1) * M(1, j) + r(i2, 2) * M(2, j);
        r = rn;
        mv(r, d1v, u1);
        for (int k = 0; k < 3; k++) {
            const double un = 0.5 * ((u0[k] - gw(k)) + (u1[k] - gw(k)));
            p[k] += dt * v[k] + 0.5 * dt * dt * un; v[k] += dt * un; a0[k] = a[k]; w0[k] = w[k];
        }
        steps++;
        if (t > t1) break;
    }
    mv(r, Pbg.v, x);
    for (int k = 0; k < 3; k++) { p[k] += x[k]; y[k] = w0[k] - Bg(k); }
    const double c1[3] = { y[1] * Pbg(2) - y[2] * Pbg(1), y[2] * Pbg(0) - y[0] * Pbg(2), y[0] * Pbg(1) - y[1] * Pbg(0) };
    mv(r, c1, x);
    for (int k = 0; k < 3; k++) v[k] += x[k];
    double worst = 0;
    for (int k = 0; k < 3; k++) { worst = std::fmax(worst, std::fabs(P(k) - p[k])); worst = std::fmax(worst, std::fabs(V(k) - v[k])); }
    for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(R.m[k] - r.m[k]));
    std::printf("rows %d header %.17g sum_dt %.17g\n", out.rows, out.header, out.pre[SWF_PRE_SUMDT]);
    std::printf("P %.17g %.17g %.17g\nV %.17g %.17g %.17g\n", P(0), P(1), P(2), V(0), V(1), V(2));
    std::printf("worst deviation from the host loop %.3g\n", worst);
    int bad = 0;
    bad += !(out.rows == steps + 1 && steps == 6 && out.header == t1);
    bad += !(std::fabs(out.pre[SWF_PRE_SUMDT] - (t1 - t0)) < 1e-12);
    bad += !(worst < 1e-12);
    for (int k = 0; k < 3; k++) {
        bad += !(out.pre[SWF_PRE_GYRI + k] == seed_w(k) && out.pre[SWF_PRE_GYRJ + k] == gyr_0(k) && gyr_0(k) == out.cut[6 * 7 + 4 + k]);
        bad += !(std::fabs(acc_0(k) - a0[k]) < 1e-14 && out.pre[SWF_PRE_LBA + k] == Ba(k) && out.pre[SWF_PRE_LBG + k] == Bg(k));
    }
    swf_ceres::IMUFactor factor(out.pre.data());
    bad += !((int)factor.pre.size() == SWF_PRE_DOUBLES);
    if (bad) { std::printf("imu frame MISMATCH (%d)\n", bad); return 1; }
    std::printf("imu frame ok\n");
    return 0;
}
