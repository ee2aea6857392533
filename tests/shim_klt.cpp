// The tracking part of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:98-141) bound to the device through
// swf_ceres::TrackImageKLT, on a point type with cv::Point2f's members.  One pair of 96 x 128 images of a smooth texture shifted by
// (3.3, -2.6) px and 40 points in the interior.  Every point must be kept within 0.5 px of the true flow, the adapter's results must
// equal swf_klt_track_batch on the same points with the reference's arguments, ReduceVector must compact by the status, and the
// prediction branch (1 level from predicted positions) must keep every point too.  Prints the values and "klt ok"; exit status 1
// when the call fails (e.g. without a GPU) or a comparison does.
#include <cmath>
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

struct Point2f { float x, y; };

static unsigned lcg_state = 97531u;
static double uni() { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) / 16777216.0; }

static const int ROWS = 96, COLS = 128, NW = 24;
static double fx[NW], fy[NW], amp[NW], ph[NW], sigma;

static std::vector<uint8_t> texture(double dx, double dy) {
    std::vector<uint8_t> img((size_t)ROWS * COLS);
    for (int y = 0; y < ROWS; y++)
        for (int x = 0; x < COLS; x++) {
            double s = 0.0;
            for (int k = 0; k < NW; k++) s += amp[k] * std::sin(fx[k] * (x + dx) + fy[k] * (y + dy) + ph[k]);
            double v = 127.5 + 127.5 * s / (3.0 * sigma);
            v = v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v;
            img[(size_t)y * COLS + x] = (uint8_t)std::lrint(v);
        }
    return img;
}

int main() {
    double a2 = 0.0;
    for (int k = 0; k < NW; k++) {
        fx[k] = (0.02 + 0.33 * uni()) * (uni() < 0.5 ? -1.0 : 1.0); fy[k] = (0.02 + 0.33 * uni()) * (uni() < 0.5 ? -1.0 : 1.0);
        amp[k] = 0.3 + 0.7 * uni(); ph[k] = 6.283185307179586 * uni();
        a2 += amp[k] * amp[k];
    }
    sigma = std::sqrt(0.5 * a2);
    const double sx = 3.3, sy = -2.6;
    const std::vector<uint8_t> prev_img = texture(0.0, 0.0), cur_img = texture(-sx, -sy);
    std::vector<Point2f> prev, cur, pred, cur2;
    std::vector<int> ids;
    for (int k = 0; k < 40; k++) {
        Point2f p = { (float)(16.0 + (COLS - 33.0) * uni()), (float)(16.0 + (ROWS - 33.0) * uni()) };
        Point2f q = { (float)(p.x + sx + 1.5), (float)(p.y + sy - 1.0) };
        prev.push_back(p); pred.push_back(q); ids.push_back(k);
    }
    int bad = 0;
    swf_ceres::TrackImageKLTResult out, with_pred;
    if (!swf_ceres::TrackImageKLT(prev_img.data(), cur_img.data(), ROWS, COLS, prev, &cur, &out)) {
        std::printf("klt failed (info %d): %s\n", out.info, swf_last_error());
        return 1;
    }
    double worst = 0.0;
    for (size_t k = 0; k < prev.size(); k++)
        worst = std::fmax(worst, std::fmax(std::fabs(cur[k].x - prev[k].x - sx), std::fabs(cur[k].y - prev[k].y - sy)));
    bad += !(out.info == SWF_KLT_OK && out.n_keep == 40 && out.levels == 3 && worst <= 0.5 && cur.size() == prev.size());
    // the C-ABI on the same points with the reference's arguments
    std::vector<double> p, c(80), b(80);
    for (size_t k = 0; k < prev.size(); k++) { p.push_back(prev[k].x); p.push_back(prev[k].y); }
    const int32_t first[2] = { 0, 40 };
    std::vector<uint8_t> st(40);
    std::vector<int32_t> why(40), keep(40);
    int32_t nk = -1, info = -1;
    if (swf_klt_track_batch(1, ROWS, COLS, prev_img.data(), cur_img.data(), first, p.data(), nullptr, 21, 3, 1, 30, 0.01, 1e-4, 0.5, 5, c.data(), b.data(),
                            st.data(), why.data(), keep.data(), &nk, &info, nullptr, nullptr, nullptr, 0, nullptr) != SWF_OK) {
        std::printf("klt failed: %s\n", swf_last_error());
        return 1;
    }
    bad += !(info == out.info && nk == out.n_keep && st == out.status && why == out.why && c == out.cur_px && b == out.back_px);
    for (size_t k = 0; k < cur.size(); k++) bad += !(cur[k].x == (float)c[2 * k] && cur[k].y == (float)c[2 * k + 1]);
    swf_ceres::ReduceVector(ids, out.status);
    bad += !((int)ids.size() == nk);
    for (size_t j = 0; j < ids.size(); j++) bad += !(ids[j] == keep[j]);
    // the prediction branch
    if (!swf_ceres::TrackImageKLT(prev_img.data(), cur_img.data(), ROWS, COLS, prev, &cur2, &with_pred, &pred)) {
        std::printf("klt failed (info %d): %s\n", with_pred.info, swf_last_error());
        return 1;
    }
    double worst2 = 0.0;
    for (size_t k = 0; k < prev.size(); k++)
        worst2 = std::fmax(worst2, std::fmax(std::fabs(cur2[k].x - prev[k].x - sx), std::fabs(cur2[k].y - prev[k].y - sy)));
    bad += !(with_pred.levels == 1 && with_pred.n_keep == 40 && worst2 <= 0.5);
    std::printf("info %d kept %d of 40, largest error %.4f px (3 levels), %.4f px (predicted, 1 level)\ncur[0] %.9g %.9g back[0] %.9g %.9g\n", info, nk,
                worst, worst2, c[0], c[1], b[0], b[1]);
    if (bad) { std::printf("klt MISMATCH (%d)\n", bad); return 1; }
    std::printf("klt ok\n");
    return 0;
}
