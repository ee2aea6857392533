// The specification of swf_gftt_detect_batch (include/swf_solver.h) as a compiled host loop, one thread: the yardstick of
// tests/perf/bench_gftt.py, and held to the referee of tests/np_gftt.py bit for bit by tests/test_gftt.py.  It works the way the
// reference does: setMask rasterises a byte mask, the detector sorts all candidates and walks them.
//   g++ -O3 -ffp-contract=off -shared -fPIC -o gftt_host.so gftt_host.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

static inline int r101(int i, int n) {
    i = i < 0 ? -i : i;
    return i > n - 1 ? 2 * (n - 1) - i : i;
}

extern "C" void gftt_host(int32_t n_frames, int32_t rows, int32_t cols, const uint8_t* img, const uint8_t* mask, const int32_t* first, const double* px,
                          const int32_t* track_cnt, int32_t max_cnt, int32_t r, double quality, const int32_t* user_hw, int32_t cand_cap, int32_t flags,
                          int32_t* order, int32_t* why, int32_t* n_old, double* new_px, int32_t* n_new, int32_t* n_cand, double* max_eig,
                          int32_t* pack_first, double* pack_px, int32_t* pack_src, int32_t* info, double* eig_out) {
    const size_t npx = (size_t)rows * (size_t)cols;
    std::vector<int> hw((size_t)r + 1);
    for (int d = 0; d <= r; d++) {
        int h = 0;
        while ((h + 1) * (h + 1) <= r * r - d * d) h++;
        hw[(size_t)d] = user_hw ? user_hw[d] : h;
    }
    std::vector<uint8_t> fm(npx);
    std::vector<int16_t> gx(npx), gy(npx);
    std::vector<double> eig(npx);
    int packed = 0;
    pack_first[0] = 0;
    for (int f = 0; f < n_frames; f++) {
        pack_first[f + 1] = packed;
        const uint8_t* P = img + (size_t)f * npx;
        const int p0 = first[f], n = first[f + 1] - p0;
        std::vector<double> sx((size_t)n), sy((size_t)n);
        bool good = true;
        for (int i = 0; i < n; i++) {
            double x = px[2 * ((size_t)p0 + i)], y = px[2 * ((size_t)p0 + i) + 1];
            if (flags & 1) { x = (double)(float)x; y = (double)(float)y; }
            sx[(size_t)i] = x; sy[(size_t)i] = y;
            good = good && std::isfinite(x) && std::isfinite(y) && track_cnt[p0 + i] >= 0;
        }
        if (!good) { info[f] = 1; continue; }
        // ---- stage A on a rasterised mask
        for (size_t i = 0; i < npx; i++) fm[i] = mask ? (mask[(size_t)f * npx + i] != 0) : 1;
        std::vector<int> walk((size_t)n), kept;
        std::iota(walk.begin(), walk.end(), 0);
        std::stable_sort(walk.begin(), walk.end(), [&](int a, int b) { return track_cnt[p0 + a] > track_cnt[p0 + b]; });
        std::vector<int> code((size_t)n);
        for (int i : walk) {
            const double rx = std::nearbyint(sx[(size_t)i]), ry = std::nearbyint(sy[(size_t)i]);
            if (!(rx >= 0.0 && rx < (double)cols && ry >= 0.0 && ry < (double)rows)) { code[(size_t)i] = 1; continue; }
            const int cx = (int)rx, cy = (int)ry;
            if (!fm[(size_t)cy * cols + cx]) { code[(size_t)i] = 2; continue; }
            code[(size_t)i] = 0;
            kept.push_back(i);
            for (int dy = -r; dy <= r; dy++) {
                const int y = cy + dy, h = hw[(size_t)std::abs(dy)];
                if (y < 0 || y >= rows) continue;
                for (int x = std::max(cx - h, 0); x <= std::min(cx + h, cols - 1); x++) fm[(size_t)y * cols + x] = 0;
            }
        }
        const int nk = (int)kept.size(), budget = max_cnt - nk;
        std::vector<int> fresh;                           // linear indices of the new points
        int nc = 0;
        double m = 0.0;
        if (budget > 0) {
            // ---- stage B
            for (int y = 0; y < rows; y++) {
                const uint8_t* a = P + (size_t)r101(y - 1, rows) * cols; const uint8_t* b = P + (size_t)y * cols; const uint8_t* c = P + (size_t)r101(y + 1, rows) * cols;
                for (int x = 0; x < cols; x++) {
                    const int l = r101(x - 1, cols), q = r101(x + 1, cols);
                    gx[(size_t)y * cols + x] = (int16_t)((a[q] - a[l]) + 2 * (b[q] - b[l]) + (c[q] - c[l]));
                    gy[(size_t)y * cols + x] = (int16_t)((c[l] - a[l]) + 2 * (c[x] - a[x]) + (c[q] - a[q]));
                }
            }
            bool any = false;
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < cols; x++) {
                    int32_t A = 0, B = 0, C = 0;
                    for (int j = -1; j <= 1; j++)
                        for (int i = -1; i <= 1; i++) {
                            const size_t at = (size_t)r101(y + j, rows) * cols + r101(x + i, cols);
                            const int u = gx[at], v = gy[at];
                            A += u * u; B += u * v; C += v * v;
                        }
                    const int64_t d1 = (int64_t)A - C, D = d1 * d1 + 4 * (int64_t)B * B;
                    const double e = ((double)(A + C) - std::sqrt((double)D)) / 18727200.0;
                    eig[(size_t)y * cols + x] = e;
                    if (fm[(size_t)y * cols + x]) { m = any ? std::max(m, e) : e; any = true; }
                }
            if (eig_out) std::copy(eig.begin(), eig.end(), eig_out + (size_t)f * npx);
            // ---- stage C
            std::vector<int> cand;
            if (any && m > 0.0) {
                const double thr = quality * m;
                for (int y = 1; y <= rows - 2; y++)
                    for (int x = 1; x <= cols - 2; x++) {
                        const double e = eig[(size_t)y * cols + x], t = e > thr ? e : 0.0;
                        if (t == 0.0 || !fm[(size_t)y * cols + x]) continue;
                        bool top = true;
                        for (int j = -1; j <= 1 && top; j++)
                            for (int i = -1; i <= 1; i++) {
                                const double en = eig[(size_t)(y + j) * cols + x + i];
                                if (!(t >= (en > thr ? en : 0.0))) { top = false; break; }
                            }
                        if (top) cand.push_back(y * cols + x);
                    }
            }
            nc = (int)cand.size();
            if (nc > cand_cap) { info[f] = 2; n_cand[f] = nc; continue; }
            // ---- stage D
            std::sort(cand.begin(), cand.end(), [&](int a, int b) { return eig[(size_t)a] > eig[(size_t)b] || (eig[(size_t)a] == eig[(size_t)b] && a > b); });
            for (int p : cand) {
                if ((int)fresh.size() >= budget) break;
                const int x = p % cols, y = p / cols;
                bool ok = true;
                for (int q : fresh) {
                    const int dx = x - q % cols, dy = y - q / cols;
                    if (dx * dx + dy * dy < r * r) { ok = false; break; }
                }
                if (ok) fresh.push_back(p);
            }
            if (!any) m = 0.0;
        }
        // ---- outputs
        info[f] = 0; n_old[f] = nk; n_new[f] = (int)fresh.size(); n_cand[f] = nc; max_eig[f] = m;
        for (int i = 0; i < n; i++) { why[p0 + i] = code[(size_t)i]; order[p0 + i] = i < nk ? kept[(size_t)i] : -1; }
        for (int i = 0; i < nk; i++, packed++) {
            pack_px[2 * (size_t)packed] = sx[(size_t)kept[(size_t)i]]; pack_px[2 * (size_t)packed + 1] = sy[(size_t)kept[(size_t)i]];
            pack_src[packed] = kept[(size_t)i];
        }
        for (size_t j = 0; j < fresh.size(); j++, packed++) {
            const double x = (double)(fresh[j] % cols), y = (double)(fresh[j] / cols);
            new_px[((size_t)f * max_cnt + j) * 2] = x; new_px[((size_t)f * max_cnt + j) * 2 + 1] = y;
            pack_px[2 * (size_t)packed] = x; pack_px[2 * (size_t)packed + 1] = y;
            pack_src[packed] = -1;
        }
        pack_first[f + 1] = packed;
    }
}
