// FeatureManager::initFramePoseByPnP (R/feature/feature_manager.cpp:205-243) bound to the device through
// swf_ceres::InitFramePoseByPnP, on vector and matrix types with Eigen's operator() access and point types with cv::Point3f /
// Point2f's members.  One frame of 40 landmarks, 10 of them with a displaced observation, the previous frame's pose 0.1 m and 0.05 rad
// off.  The adapter's pose is compared, bit for bit, with swf_pnp_frame_batch on the same points with flag bit 0, and with the true
// pose; a frame of 3 points must leave the pose alone.  Prints the values and "pnp ok"; exit status 1 when the call fails (e.g.
// without a GPU) or a comparison does.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "swf_ceres.hpp"

struct V3 { double v[3]; double& operator()(int i) { return v[i]; } double operator()(int i) const { return v[i]; } };
struct M3 { double m[9]; double& operator()(int i, int j) { return m[3 * i + j]; } double operator()(int i, int j) const { return m[3 * i + j]; } };
struct Point3f { float x, y, z; };
struct Point2f { float x, y; };

static M3 rotz(double a) { M3 r = { { std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a), 0, 0, 0, 1 } }; return r; }
static M3 rotx(double a) { M3 r = { { 1, 0, 0, 0, std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a) } }; return r; }
static M3 mul(const M3& a, const M3& b) {
    M3 c;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c(i, j) = a(i, 0) * b(0, j) + a(i, 1) * b(1, j) + a(i, 2) * b(2, j);
    return c;
}
static unsigned lcg_state = 12345u;
static double uni() { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) / 16777216.0; }

int main() {
    const double focal = 1000.0, threshold = 8.0 / focal;
    V3 tic[1] = { { { 0.05, -0.02, 0.03 } } }, Pbg = { { 0.1, 0.2, -0.3 } };
    M3 ric[1] = { rotx(0.02) };
    const M3 Rtrue = mul(rotz(0.3), rotx(-0.2));
    const V3 Ptrue = { { 1.0, 2.0, 3.0 } };
    const M3 Rc = mul(Rtrue, ric[0]);
    V3 Pc;
    for (int i = 0; i < 3; i++) Pc(i) = Rtrue(i, 0) * (tic[0](0) - Pbg(0)) + Rtrue(i, 1) * (tic[0](1) - Pbg(1)) + Rtrue(i, 2) * (tic[0](2) - Pbg(2)) + Ptrue(i);
    std::vector<Point3f> pts3D;
    std::vector<Point2f> pts2D;
    for (int k = 0; k < 40; k++) {
        const double z = 4.0 + 11.0 * uni(), x = (uni() - 0.5) * z, y = (uni() - 0.5) * z;
        const double c[3] = { x, y, z };
        Point3f p3 = { (float)(Rc(0, 0) * c[0] + Rc(0, 1) * c[1] + Rc(0, 2) * c[2] + Pc(0)), (float)(Rc(1, 0) * c[0] + Rc(1, 1) * c[1] + Rc(1, 2) * c[2] + Pc(1)),
                       (float)(Rc(2, 0) * c[0] + Rc(2, 1) * c[1] + Rc(2, 2) * c[2] + Pc(2)) };
        Point2f p2 = { (float)(x / z + (uni() - 0.5) / focal), (float)(y / z + (uni() - 0.5) / focal) };
        if (k % 4 == 1) p2.x += (float)(80.0 / focal);
        pts3D.push_back(p3); pts2D.push_back(p2);
    }
    V3 Ps[3]; M3 Rs[3];
    std::memset(Ps, 0, sizeof Ps); std::memset(Rs, 0, sizeof Rs);
    Rs[1] = mul(Rtrue, rotz(0.05));
    for (int i = 0; i < 3; i++) Ps[1](i) = Ptrue(i) + (i == 0 ? 0.08 : i == 1 ? -0.05 : 0.03);
    const V3 P2_before = Ps[2]; const M3 R2_before = Rs[2];

    // too few points: the pose stays as it is (needs no device)
    std::vector<Point3f> few3(pts3D.begin(), pts3D.begin() + 3);
    std::vector<Point2f> few2(pts2D.begin(), pts2D.begin() + 3);
    swf_ceres::PnpFrameResult fr;
    const bool few_ok = swf_ceres::InitFramePoseByPnP(2, Ps, Rs, tic, ric, Pbg, few3, few2, threshold, &fr);
    int bad = 0;
    bad += !(few_ok == false && fr.info == SWF_PNP_TOO_FEW);
    bad += !(std::memcmp(&Ps[2], &P2_before, sizeof(V3)) == 0 && std::memcmp(&Rs[2], &R2_before, sizeof(M3)) == 0);
    bad += !(swf_ceres::InitFramePoseByPnP(0, Ps, Rs, tic, ric, Pbg, pts3D, pts2D, threshold) == false);

    swf_ceres::PnpFrameResult out;
    if (!swf_ceres::InitFramePoseByPnP(2, Ps, Rs, tic, ric, Pbg, pts3D, pts2D, threshold, &out)) {
        std::printf("pnp failed (info %d): %s\n", out.info, swf_last_error());
        return 1;
    }
    // the C-ABI on the same points, flag bit 0
    std::vector<double> pw, uv;
    for (size_t k = 0; k < pts3D.size(); k++) {
        pw.push_back(pts3D[k].x); pw.push_back(pts3D[k].y); pw.push_back(pts3D[k].z);
        uv.push_back(pts2D[k].x); uv.push_back(pts2D[k].y);
    }
    const int32_t first[2] = { 0, (int32_t)pts3D.size() };
    double po[3], ro[9];
    int32_t ni = 0, best = -1, nit = 0, info = -1;
    std::vector<uint8_t> inl(pts3D.size());
    if (swf_pnp_frame_batch(1, first, pw.data(), uv.data(), Ps[1].v, Rs[1].m, tic[0].v, ric[0].m, Pbg.v, 100, threshold, 0.99, 0, 1, po, ro, &ni, inl.data(),
                            &best, &nit, &info, nullptr, nullptr, nullptr, 0, nullptr) != SWF_OK) {
        std::printf("pnp failed: %s\n", swf_last_error());
        return 1;
    }
    bad += !(info == out.info && ni == out.n_inliers && best == out.best && nit == out.n_iters && out.inlier == inl);
    bad += !(std::memcmp(po, Ps[2].v, sizeof po) == 0 && std::memcmp(ro, Rs[2].m, sizeof ro) == 0);
    double worst = 0;
    for (int k = 0; k < 3; k++) worst = std::fmax(worst, std::fabs(Ps[2](k) - Ptrue(k)));
    for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(Rs[2].m[k] - Rtrue.m[k]));
    int marked = 0;
    for (size_t k = 0; k < inl.size(); k++) marked += (k % 4 == 1) && inl[k];
    std::printf("info %d inliers %d best %d n_iters %d\nP %.17g %.17g %.17g\nworst deviation from the true pose %.3g\n", info, ni, best, nit,
                Ps[2](0), Ps[2](1), Ps[2](2), worst);
    bad += !(info == SWF_PNP_OK && ni == 30 && marked == 0 && worst < 5e-3);
    if (bad) { std::printf("pnp MISMATCH (%d)\n", bad); return 1; }
    std::printf("pnp ok\n");
    return 0;
}
