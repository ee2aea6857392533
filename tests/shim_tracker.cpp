// shim_tracker.cpp — swf_ceres::FeatureTracker driven the way the reference's estimator drives its FeatureTracker: one trackImage per
// frame, the returned feature map printed so that tests/test_tracker_gpu.py can compare it with solver.Tracker bit for bit.
// TEST INFRASTRUCTURE.   usage: shim_tracker <file>
// file: int32 n_frames, rows, cols, max_cnt, min_dist, cand_cap, f_iterations, n_remove; double cam[12]; double times[n_frames];
//       int32 remove[n_remove] (removed before the third frame); the frames' bytes.
#include <cinttypes>
#include <cstdio>
#include <set>
#include <vector>
#include "swf_ceres.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[8];
    double cam[12];
    if (std::fread(head, sizeof(int32_t), 8, f) != 8 || std::fread(cam, sizeof(double), 12, f) != 12) return 2;
    const int n = head[0], rows = head[1], cols = head[2];
    std::vector<double> times((size_t)n);
    std::vector<int32_t> rm((size_t)head[7] + 1);
    std::vector<uint8_t> img((size_t)rows * (size_t)cols);
    if (std::fread(times.data(), sizeof(double), (size_t)n, f) != (size_t)n) return 2;
    if (std::fread(rm.data(), sizeof(int32_t), (size_t)head[7], f) != (size_t)head[7]) return 2;
    swf_tracker_options o;
    swf_tracker_default_options(&o);
    o.max_cnt = head[3]; o.min_dist = head[4]; o.cand_cap = head[5]; o.f_iterations = head[6];
    swf_ceres::FeatureTracker tracker(rows, cols, cam, &o);
    if (tracker.last_rc != SWF_OK) { std::printf("create failed: %s\n", swf_last_error()); return 1; }
    for (int k = 0; k < n; k++) {
        if (std::fread(img.data(), 1, img.size(), f) != img.size()) return 2;
        if (k == 2) tracker.removeOutliers(std::set<int>(rm.begin(), rm.begin() + head[7]));
        const swf_ceres::FeatureTracker::FeatureFrame frame = tracker.trackImage(times[(size_t)k], img.data());
        if (tracker.last_rc != SWF_OK) { std::printf("frame %d failed: %s\n", k, swf_last_error()); return 1; }
        std::printf("frame %d n %d info %d\n", k, (int)frame.size(), (int)tracker.info);
        for (const auto& it : frame) {
            if (it.second.size() != 1 || it.second[0].first != 0) return 1;
            std::printf("id %d", it.first);
            for (int j = 0; j < 7; j++) {
                uint64_t bits;
                std::memcpy(&bits, &it.second[0].second[(size_t)j], 8);
                std::printf(" %016" PRIx64, bits);
            }
            std::printf("\n");
        }
    }
    std::fclose(f);
    std::printf("tracker ok\n");
    return 0;
}
