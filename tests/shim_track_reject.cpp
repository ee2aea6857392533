// FeatureTracker::rejectWithF with undistortedPts and ptsVelocity (R/feature/feature_tracker.cpp:265-294, :334-376) bound to the device
// through swf_ceres::RejectWithF, on a point type with cv::Point2f's members.  One pair of 60 tracks of a sideways motion seen through a
// distorted pinhole camera, every fifth track displaced by 40 px.  The adapter's status is compared with swf_track_reject_batch on the
// same points with flag bit 0, the displaced tracks must be dropped and most of the others kept, ReduceVector must compact by the
// status, and a pair of 5 tracks must report SWF_TRK_TOO_FEW with its normalised points filled.  Prints the values and "track reject
// ok"; exit status 1 when the call fails (e.g. without a GPU) or a comparison does.
#include <cmath>
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

struct Point2f { float x, y; };

static unsigned lcg_state = 2468u;
static double uni() { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) / 16777216.0; }

static const double cam[12] = { 1015.0, 1014.5, 357.8, 217.3, -0.39, 0.15, 0.004, 0.004, 0.0, 0.0, 0.0, 0.0 };

static Point2f project(double X, double Y, double Z) {
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y;
    const double cd = 1.0 + ((cam[8] * r2 + cam[5]) * r2 + cam[4]) * r2;
    const double xd = x * cd + 2.0 * cam[6] * x * y + cam[7] * (r2 + 2.0 * x * x), yd = y * cd + cam[6] * (r2 + 2.0 * y * y) + 2.0 * cam[7] * x * y;
    Point2f p = { (float)(cam[0] * xd + cam[2]), (float)(cam[1] * yd + cam[3]) };
    return p;
}

int main() {
    const int col = 752, row = 480;
    const double focal = 1000.0, f_threshold = 1.0, dt = 0.05;
    std::vector<Point2f> cur, prev;
    std::vector<int> ids;
    for (int k = 0; k < 60; k++) {
        const double Z = 4.0 + 12.0 * uni(), X = (uni() - 0.5) * 0.5 * Z, Y = (uni() - 0.5) * 0.3 * Z;
        Point2f c = project(X, Y, Z), p = project(X + 0.6, Y + 0.03 * X, Z + 0.05);     // the previous camera: 0.6 m to the side
        c.x += (float)(0.2 * (uni() - 0.5)); c.y += (float)(0.2 * (uni() - 0.5));
        if (k % 5 == 2) p.y += 40.0f;
        cur.push_back(c); prev.push_back(p); ids.push_back(k);
    }
    int bad = 0;
    // too few tracks: the reference skips the gate (needs the device for the lift)
    std::vector<Point2f> few_c(cur.begin(), cur.begin() + 5), few_p(prev.begin(), prev.begin() + 5);
    swf_ceres::RejectWithFResult out, few;
    if (!swf_ceres::RejectWithF(cur, prev, cam, col, row, focal, f_threshold, dt, &out)) {
        std::printf("track reject failed (info %d): %s\n", out.info, swf_last_error());
        return 1;
    }
    bad += !(swf_ceres::RejectWithF(few_c, few_p, cam, col, row, focal, f_threshold, dt, &few) == false && few.info == SWF_TRK_TOO_FEW);
    bad += !(few.status.empty() && few.un_cur.size() == 10 && few.un_cur[0] == out.un_cur[0] && few.velocity[1] == out.velocity[1]);
    // the C-ABI on the same points, flag bit 0
    std::vector<double> c, p;
    for (size_t k = 0; k < cur.size(); k++) { c.push_back(cur[k].x); c.push_back(cur[k].y); p.push_back(prev[k].x); p.push_back(prev[k].y); }
    const int32_t first[2] = { 0, (int32_t)cur.size() };
    std::vector<uint8_t> st(cur.size());
    std::vector<int32_t> keep(cur.size());
    int32_t ni = 0, best = -1, nit = 0, info = -1;
    if (swf_track_reject_batch(1, first, c.data(), p.data(), cam, col, row, focal, &dt, 1000, f_threshold, 0.99, 0, 1, st.data(), keep.data(), &ni, &best,
                               &nit, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != SWF_OK) {
        std::printf("track reject failed: %s\n", swf_last_error());
        return 1;
    }
    bad += !(info == out.info && ni == out.n_inliers && best == out.best && nit == out.n_iters && out.status == st);
    int marked = 0, kept = 0;
    for (size_t k = 0; k < st.size(); k++) { marked += (k % 5 == 2) && st[k]; kept += st[k]; }
    swf_ceres::ReduceVector(ids, out.status);
    bad += !((int)ids.size() == kept && kept == ni);
    for (size_t j = 0; j < ids.size(); j++) bad += !(ids[j] == keep[j] && st[(size_t)ids[j]]);
    for (size_t j = ids.size(); j < keep.size(); j++) bad += !(keep[j] == -1);
    const double vx = (double)(float)((double)((float)out.un_cur[0] - (float)out.un_prev[0]) / dt);
    bad += !(out.velocity[0] == vx && std::fabs(out.un_cur[0] - (cur[0].x - cam[2]) / cam[0]) < 0.05);
    std::printf("info %d inliers %d of %d best %d n_iters %d\nun_cur[0] %.9g %.9g velocity[0] %.9g %.9g\n", info, ni, (int)st.size(), best, nit,
                out.un_cur[0], out.un_cur[1], out.velocity[0], out.velocity[1]);
    bad += !(info == SWF_TRK_OK && marked == 0 && kept >= 36);
    if (bad) { std::printf("track reject MISMATCH (%d)\n", bad); return 1; }
    std::printf("track reject ok\n");
    return 0;
}
