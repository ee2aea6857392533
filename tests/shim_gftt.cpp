// Lines 148-165 of FeatureTracker::trackImage (setMask, cv::goodFeaturesToTrack, addPoints) bound to the device through
// swf_ceres::DetectFeatures, on a point type with cv::Point2f's members.  One 96 x 128 frame of pseudo-random bytes, twelve tracked
// points of which some crowd each other and one lies outside, MAX_CNT 60, MIN_DIST 10.  The adapter's state afterwards must be what the
// C-ABI's order and new_px say: the kept points by track_cnt, their ids and counts moved with them, then the new corners with fresh
// ids and count 1; every pair of new corners at least MIN_DIST apart, none inside a kept point's disc; and a second call with a
// cand_cap below the number of candidates must succeed through the retry.  Prints the values and "gftt ok"; exit status 1 when the call
// fails (e.g. without a GPU) or a comparison does.
#include <cmath>
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

struct Point2f { float x, y; };

static unsigned lcg_state = 24680u;
static unsigned lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

int main() {
    const int ROWS = 96, COLS = 128, MAX_CNT = 60, MIN_DIST = 10;
    std::vector<uint8_t> img((size_t)ROWS * COLS);
    for (auto& v : img) v = (uint8_t)(lcg() & 255u);
    const float xy[12][2] = { { 20.f, 20.f }, { 24.f, 23.f }, { 60.f, 40.f }, { 60.5f, 47.f }, { 100.f, 80.f }, { -3.f, 10.f }, { 101.f, 88.f }, { 30.f, 70.f },
                              { 31.f, 71.f }, { 110.f, 15.f }, { 64.f, 90.f }, { 5.f, 50.f } };
    const int cnt[12] = { 3, 7, 2, 2, 9, 4, 1, 5, 5, 6, 8, 2 };
    std::vector<Point2f> pts, pts0;
    std::vector<int> ids, tc, ids0, tc0;
    for (int k = 0; k < 12; k++) { pts.push_back({ xy[k][0], xy[k][1] }); ids.push_back(100 + k); tc.push_back(cnt[k]); }
    pts0 = pts; ids0 = ids; tc0 = tc;
    int n_id = 500, bad = 0;
    swf_ceres::DetectFeaturesResult out;
    if (!swf_ceres::DetectFeatures(img.data(), ROWS, COLS, &pts, &ids, &tc, &n_id, &out, MAX_CNT, MIN_DIST)) {
        std::printf("gftt failed (info %d): %s\n", out.info, swf_last_error());
        return 1;
    }
    // the C-ABI on the same state
    std::vector<double> p(26, 0.0), fresh((size_t)MAX_CNT * 2, 0.0);
    std::vector<int32_t> c(13, 0), order(13, -1), why(13, -1);
    for (int k = 0; k < 12; k++) { p[2 * k] = xy[k][0]; p[2 * k + 1] = xy[k][1]; c[k] = cnt[k]; }
    const int32_t first[2] = { 0, 12 };
    int32_t n_old = -1, n_new = -1, n_cand = -1, info = -1;
    double max_eig = -1.0;
    if (swf_gftt_detect_batch(1, ROWS, COLS, img.data(), nullptr, first, p.data(), c.data(), MAX_CNT, MIN_DIST, 0.01, nullptr, 1 << 15, 1, order.data(), why.data(),
                              &n_old, fresh.data(), &n_new, &n_cand, &max_eig, nullptr, nullptr, nullptr, &info, nullptr, 0, nullptr) != SWF_OK) {
        std::printf("gftt failed: %s\n", swf_last_error());
        return 1;
    }
    bad += !(info == SWF_GFTT_OK && out.info == info && out.n_old == n_old && out.n_new == n_new && out.n_cand == n_cand && out.max_eig == max_eig);
    bad += !(n_old >= 6 && n_old < 12 && n_old + n_new == MAX_CNT && (int)pts.size() == MAX_CNT && ids.size() == pts.size() && tc.size() == pts.size());
    bad += !(n_id == 500 + n_new && why[5] == SWF_GFTT_OUTSIDE && why[4] == SWF_GFTT_KEPT && why[6] == SWF_GFTT_CROWDED && order[0] == 4);
    for (int j = 0; j < n_old; j++) {
        const int i = order[(size_t)j];
        bad += !(pts[(size_t)j].x == xy[i][0] && pts[(size_t)j].y == xy[i][1] && ids[(size_t)j] == 100 + i && tc[(size_t)j] == cnt[i]);
        if (j) bad += !(tc[(size_t)j] <= tc[(size_t)j - 1]);
    }
    for (int j = 0; j < n_new; j++) {
        const size_t at = (size_t)(n_old + j);
        bad += !(pts[at].x == (float)fresh[2 * (size_t)j] && pts[at].y == (float)fresh[2 * (size_t)j + 1] && ids[at] == 500 + j && tc[at] == 1);
        for (int k = 0; k < j; k++) {
            const double dx = fresh[2 * (size_t)j] - fresh[2 * (size_t)k], dy = fresh[2 * (size_t)j + 1] - fresh[2 * (size_t)k + 1];
            bad += !(dx * dx + dy * dy >= (double)(MIN_DIST * MIN_DIST));
        }
        for (int k = 0; k < n_old; k++) {                 // outside the Euclidean disc of every kept point
            const double dx = fresh[2 * (size_t)j] - std::nearbyint((double)pts[(size_t)k].x), dy = fresh[2 * (size_t)j + 1] - std::nearbyint((double)pts[(size_t)k].y);
            bad += !(dx * dx + dy * dy > (double)(MIN_DIST * MIN_DIST));
        }
    }
    // a cand_cap below the candidate count: the adapter asks again with the reported count and ends on the same state
    std::vector<Point2f> pts2 = pts0;
    std::vector<int> ids2 = ids0, tc2 = tc0;
    int n_id2 = 500;
    swf_ceres::DetectFeaturesResult again;
    if (!swf_ceres::DetectFeatures(img.data(), ROWS, COLS, &pts2, &ids2, &tc2, &n_id2, &again, MAX_CNT, MIN_DIST, nullptr, 64)) {
        std::printf("gftt failed (info %d): %s\n", again.info, swf_last_error());
        return 1;
    }
    bad += !(n_cand > 64 && again.n_cand == n_cand && again.n_new == n_new && ids2 == ids && tc2 == tc && n_id2 == n_id && pts2.size() == pts.size());
    for (size_t k = 0; k < pts.size() && k < pts2.size(); k++) bad += !(pts2[k].x == pts[k].x && pts2[k].y == pts[k].y);
    std::printf("info %d kept %d of 12, %d new of %d candidates, max eig %.9g, first new (%g, %g)\n", info, n_old, n_new, n_cand, max_eig, fresh[0], fresh[1]);
    if (bad) { std::printf("gftt MISMATCH (%d)\n", bad); return 1; }
    std::printf("gftt ok\n");
    return 0;
}
