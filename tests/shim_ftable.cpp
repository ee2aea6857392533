// shim_ftable.cpp — swf_ceres::FeatureManager driven through one cycle the way the reference's estimator drives its FeatureManager:
// addFeatureCheckParallax per frame, the PnP gather, triangulate, the listing, the solved points back, removeFailures, CheckParallax,
// removeBack.  Everything it returns and the table's final state are printed as bits for tests/test_ftable_gpu.py.
// TEST INFRASTRUCTURE.   usage: shim_ftable <file>
// file: int32 window, feat_cap, frame_cap, feature_continue, min_track, min_long, long_len, n_frames, n_solved;
//       double tic[3], ric[9], pbg[3], Ps[window][3], Rs[window][9], P1[3], R1[9];
//       per frame int32 n, int32 ids[n], double obs[n][7];  double solved[n_solved][3]; uint8 flags[n_solved].
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

static void hex(const double* v, size_t n) {
    for (size_t k = 0; k < n; k++) {
        uint64_t bits;
        std::memcpy(&bits, v + k, 8);
        std::printf(" %016" PRIx64, bits);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[9];
    if (std::fread(head, sizeof(int32_t), 9, f) != 9) return 2;
    const size_t W = (size_t)head[0];
    double tic[3], ric[9], pbg[3], P1[3], R1[9];
    std::vector<double> Ps(W * 3), Rs(W * 9);
    if (std::fread(tic, 8, 3, f) != 3 || std::fread(ric, 8, 9, f) != 9 || std::fread(pbg, 8, 3, f) != 3) return 2;
    if (std::fread(Ps.data(), 8, W * 3, f) != W * 3 || std::fread(Rs.data(), 8, W * 9, f) != W * 9) return 2;
    if (std::fread(P1, 8, 3, f) != 3 || std::fread(R1, 8, 9, f) != 9) return 2;
    swf_ftable_options o;
    swf_ftable_default_options(&o);
    o.window = head[0]; o.feat_cap = head[1]; o.frame_cap = head[2]; o.feature_continue = head[3];
    o.min_track = head[4]; o.min_long = head[5]; o.long_len = head[6];
    swf_ceres::FeatureManager fm(&o);
    if (fm.last_rc != SWF_OK) { std::printf("create failed: %s\n", swf_last_error()); return 1; }
    for (int k = 0; k < head[7]; k++) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
        std::vector<int32_t> ids((size_t)n + 1);
        std::vector<double> obs((size_t)n * 7 + 1);
        if (std::fread(ids.data(), 4, (size_t)n, f) != (size_t)n || std::fread(obs.data(), 8, (size_t)n * 7, f) != (size_t)n * 7) return 2;
        swf_ceres::FeatureTracker::FeatureFrame frame;
        for (int32_t i = 0; i < n; i++) {
            std::array<double, 7> v;
            for (size_t c = 0; c < 7; c++) v[c] = obs[(size_t)i * 7 + c];
            frame[ids[(size_t)i]].emplace_back(0, v);
        }
        const bool key = fm.addFeatureCheckParallax(k, frame);
        fm.removeOut(k + 1);
        if (fm.last_rc != SWF_OK) { std::printf("frame %d failed: %s\n", k, swf_last_error()); return 1; }
        std::printf("add %d key %d last %d long %d new %d erased %d info %d\n", k, key ? 1 : 0, fm.last_track_num, fm.long_track_num,
                    fm.new_feature_num, (int)fm.counts[SWF_FTABLE_C_ERASED], (int)fm.counts[SWF_FTABLE_C_INFO]);
    }
    std::vector<double> pw, puv;
    fm.pnpPoints(pw, puv);
    std::printf("pnp %d", (int)(pw.size() / 3)); hex(pw.data(), pw.size()); hex(puv.data(), puv.size()); std::printf("\n");
    fm.triangulate(Ps.data(), Rs.data(), tic, ric, pbg);
    swf_ceres::FeatureManager::Listing L;
    fm.listFeatures(L);
    if (fm.last_rc != SWF_OK) { std::printf("list failed: %s\n", swf_last_error()); return 1; }
    std::printf("count %d\n", fm.getFeatureCount());
    for (size_t i = 0; i < L.lm_id.size(); i++) {
        std::printf("lm %d %d %d %d", (int)L.lm_id[i], (int)L.lm_start[i], (int)L.lm_nobs[i], (int)L.lm_valid[i]);
        hex(&L.lm_world[3 * i], 3); std::printf("\n");
    }
    for (size_t i = 0; i < L.proj_frame.size(); i++) {
        std::printf("proj %d %d %d", (int)L.proj_frame[i], (int)L.proj_lm[i], (int)L.proj_new[i]);
        hex(&L.proj_uv[2 * i], 2); std::printf("\n");
    }
    const size_t ns = (size_t)head[8];
    if (ns != L.lm_id.size()) { std::printf("the file's solved points are %d, the listing's %d\n", (int)ns, (int)L.lm_id.size()); return 1; }
    std::vector<double> solved(ns * 3);
    std::vector<uint8_t> flags(ns + 1);
    if (std::fread(solved.data(), 8, ns * 3, f) != ns * 3 || std::fread(flags.data(), 1, ns, f) != ns) return 2;
    std::fclose(f);
    fm.setSolved(solved, flags.data(), Ps.data(), Rs.data(), tic, ric, pbg);
    const std::set<int> gone = fm.removeFailures();
    std::printf("removed");
    for (int id : gone) std::printf(" %d", id);
    std::printf("\n");
    const bool pkey = fm.CheckParallax(head[7] - 1);
    std::printf("parallax key %d num %d", pkey ? 1 : 0, (int)fm.counts[SWF_FTABLE_C_PARALLAX_NUM]); hex(&fm.last_average_parallax, 1); std::printf("\n");
    fm.removeBack(nullptr, nullptr, P1, R1, tic, ric, pbg);
    if (fm.last_rc != SWF_OK) { std::printf("slide failed: %s\n", swf_last_error()); return 1; }
    const size_t F = (size_t)o.feat_cap;
    int32_t n_frames = 0, n_feat = 0;
    std::vector<int32_t> id(F), start(F), n_obs(F), valid(F), flag(F), inp(F * W);
    std::vector<double> idepth(F), world(F * 3), obs(F * W * 7);
    if (swf_ftable_download(fm.handle(), &n_frames, &n_feat, id.data(), start.data(), n_obs.data(), valid.data(), flag.data(), idepth.data(),
                            world.data(), obs.data(), inp.data()) != SWF_OK) { std::printf("download failed: %s\n", swf_last_error()); return 1; }
    std::printf("state frames %d features %d\n", (int)n_frames, (int)n_feat);
    for (size_t i = 0; i < (size_t)n_feat; i++) {
        std::printf("feat %d %d %d %d %d", (int)id[i], (int)start[i], (int)n_obs[i], (int)valid[i], (int)flag[i]);
        hex(&idepth[i], 1); hex(&world[3 * i], 3);
        for (size_t k = 0; k < (size_t)n_obs[i]; k++) { std::printf(" %d", (int)inp[i * W + k]); hex(&obs[(i * W + k) * 7], 7); }
        std::printf("\n");
    }
    std::printf("ftable ok\n");
    return 0;
}
