// The specification of swf_klt_track_batch as a plain host loop over the pairs, for tests/perf/bench_klt.py and
// tests/test_klt.py: integer pyramids, whole Scharr derivative images per level (what a host tracker keeps; the device forms them per
// patch), the fixed-point template and the iterations with exact integer sums, the reverse pass and the gates.  Same arithmetic as
// the device, so its results are compared bit for bit.  g++ -O3 -ffp-contract=off -shared -fPIC.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Level { int w, h; std::vector<uint8_t> I; std::vector<int16_t> gx, gy; };

inline int r101(int i, int n) {
    i = i < 0 ? -i : i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

void derivatives(Level& L) {
    const int w = L.w, h = L.h;
    L.gx.assign((size_t)w * h, 0); L.gy.assign((size_t)w * h, 0);
    for (int y = 0; y < h; y++) {
        const uint8_t* t = &L.I[(size_t)r101(y - 1, h) * w]; const uint8_t* m = &L.I[(size_t)y * w]; const uint8_t* b = &L.I[(size_t)r101(y + 1, h) * w];
        for (int x = 0; x < w; x++) {
            const int l = r101(x - 1, w), r = r101(x + 1, w);
            L.gx[(size_t)y * w + x] = (int16_t)(3 * (t[r] - t[l]) + 10 * (m[r] - m[l]) + 3 * (b[r] - b[l]));
            L.gy[(size_t)y * w + x] = (int16_t)(3 * (b[l] - t[l]) + 10 * (b[x] - t[x]) + 3 * (b[r] - t[r]));
        }
    }
}

void pyr_down(const Level& S, Level& D) {
    static const int k[5] = { 1, 4, 6, 4, 1 };
    D.w = (S.w + 1) / 2; D.h = (S.h + 1) / 2;
    D.I.resize((size_t)D.w * D.h);
    std::vector<int> rowsum((size_t)D.w);
    for (int y = 0; y < D.h; y++) {
        for (int x = 0; x < D.w; x++) rowsum[(size_t)x] = 0;
        for (int j = 0; j < 5; j++) {
            const uint8_t* row = &S.I[(size_t)r101(2 * y + j - 2, S.h) * S.w];
            for (int x = 0; x < D.w; x++) {
                int s = 0;
                for (int i = 0; i < 5; i++) s += k[i] * row[r101(2 * x + i - 2, S.w)];
                rowsum[(size_t)x] += k[j] * s;
            }
        }
        for (int x = 0; x < D.w; x++) D.I[(size_t)y * D.w + x] = (uint8_t)((rowsum[(size_t)x] + 128) >> 8);
    }
}

std::vector<Level> pyramid(const uint8_t* img, int rows, int cols, int win, int levels) {
    std::vector<Level> P(1);
    P[0].w = cols; P[0].h = rows; P[0].I.assign(img, img + (size_t)rows * cols);
    while ((int)P.size() <= levels) {
        const Level& S = P.back();
        if ((S.w + 1) / 2 <= win || (S.h + 1) / 2 <= win) break;
        Level D;
        pyr_down(S, D);
        P.push_back(D);
    }
    for (auto& L : P) derivatives(L);
    return P;
}

inline bool outside(double fx, double fy, int w, int h, int win) { return !(fx >= (double)-win && fx < (double)w && fy >= (double)-win && fy < (double)h); }

inline void weights(double px, double py, double fx, double fy, int wt[4]) {
    const double a = px - fx, b = py - fy;
    wt[0] = (int)std::rint((1.0 - a) * (1.0 - b) * 16384.0);
    wt[1] = (int)std::rint(a * (1.0 - b) * 16384.0);
    wt[2] = (int)std::rint((1.0 - a) * b * 16384.0);
    wt[3] = 16384 - wt[0] - wt[1] - wt[2];
}

struct Pass { double x, y; bool lost, flat; };

Pass track(const std::vector<Level>& PI, const std::vector<Level>& PJ, double prx, double pry, double inix, double iniy, int top, int win,
           int max_count, double eps2, double min_eig) {
    const double half = (double)((win - 1) / 2);
    const int nel = win * win;
    std::vector<int> It((size_t)nel), Itx((size_t)nel), Ity((size_t)nel);
    Pass R = { 0.0, 0.0, false, false };
    double qx = 0.0, qy = 0.0;
    for (int l = top; l >= 0; l--) {
        const Level& I = PI[(size_t)l]; const Level& J = PJ[(size_t)l];
        const int w = I.w, h = I.h;
        const double scale = 1.0 / (double)(1 << l);
        double px = prx * scale, py = pry * scale;
        if (l == top) { qx = inix * scale; qy = iniy * scale; } else { qx = 2.0 * qx; qy = 2.0 * qy; }
        px = px - half; py = py - half;
        const double fpx = std::floor(px), fpy = std::floor(py);
        if (outside(fpx, fpy, w, h, win)) { if (l == 0) R.lost = true; continue; }
        const int ix = (int)fpx, iy = (int)fpy;
        int wt[4];
        weights(px, py, fpx, fpy, wt);
        int64_t s11 = 0, s12 = 0, s22 = 0;
        for (int j = 0; j < win; j++)
            for (int i = 0; i < win; i++) {
                int v = 0, vx = 0, vy = 0;
                for (int c = 0; c < 4; c++) {
                    const int x = ix + i + (c & 1), y = iy + j + (c >> 1);
                    const size_t at = (size_t)r101(y, h) * w + r101(x, w);
                    v += I.I[at] * wt[c];
                    if (x >= 0 && x < w && y >= 0 && y < h) { vx += I.gx[at] * wt[c]; vy += I.gy[at] * wt[c]; }
                }
                const size_t e = (size_t)j * win + i;
                It[e] = (v + 256) >> 9; Itx[e] = (vx + 8192) >> 14; Ity[e] = (vy + 8192) >> 14;
                s11 += (int64_t)Itx[e] * Itx[e]; s12 += (int64_t)Itx[e] * Ity[e]; s22 += (int64_t)Ity[e] * Ity[e];
            }
        const double A11 = (double)s11 * 0x1p-20, A12 = (double)s12 * 0x1p-20, A22 = (double)s22 * 0x1p-20;
        double D = A11 * A22 - A12 * A12;
        const double min_e = (A22 + A11 - std::sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (double)(2 * win * win);
        if (min_e < min_eig || D < 0x1p-23) { if (l == 0) R.flat = true; continue; }
        D = 1.0 / D;
        qx = qx - half; qy = qy - half;
        double pdx = 0.0, pdy = 0.0;
        for (int it = 0; it < max_count; it++) {
            const double fqx = std::floor(qx), fqy = std::floor(qy);
            if (outside(fqx, fqy, w, h, win)) { if (l == 0) R.lost = true; break; }
            const int jx = (int)fqx, jy = (int)fqy;
            weights(qx, qy, fqx, fqy, wt);
            int64_t sb1 = 0, sb2 = 0;
            for (int j = 0; j < win; j++) {
                const uint8_t* r0 = &J.I[(size_t)r101(jy + j, h) * w]; const uint8_t* r1 = &J.I[(size_t)r101(jy + j + 1, h) * w];
                for (int i = 0; i < win; i++) {
                    const int x0 = r101(jx + i, w), x1 = r101(jx + i + 1, w);
                    const int v = r0[x0] * wt[0] + r0[x1] * wt[1] + r1[x0] * wt[2] + r1[x1] * wt[3];
                    const size_t e = (size_t)j * win + i;
                    const int d = ((v + 256) >> 9) - It[e];
                    sb1 += (int64_t)d * Itx[e]; sb2 += (int64_t)d * Ity[e];
                }
            }
            const double b1 = (double)sb1 * 0x1p-20, b2 = (double)sb2 * 0x1p-20;
            const double dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            qx = qx + dx; qy = qy + dy;
            if (dx * dx + dy * dy <= eps2) break;
            if (it > 0 && std::fabs(dx + pdx) < 0.01 && std::fabs(dy + pdy) < 0.01) { qx = qx - dx * 0.5; qy = qy - dy * 0.5; break; }
            pdx = dx; pdy = dy;
        }
        qx = qx + half; qy = qy + half;
    }
    R.x = qx; R.y = qy;
    return R;
}

}  // namespace

// the arguments of swf_klt_track_batch on host memory, without the stage exports; info 1 for a pair with a non-finite position
extern "C" void klt_host(int32_t n_pairs, int32_t rows, int32_t cols, const uint8_t* prev_img, const uint8_t* cur_img, const int32_t* first,
                         const double* prev_px, const double* guess_px, int32_t win, int32_t max_level, int32_t back_level, int32_t max_count,
                         double eps, double min_eig, double back_dist, int32_t flags, double* cur_px, double* back_px, uint8_t* status,
                         int32_t* why, int32_t* n_keep, int32_t* info) {
    const bool as_float = flags & 1, use_guess = flags & 2, back = flags & 4;
    auto stage = [&](double v) { volatile float r = (float)v; return as_float ? (double)r : v; };   // volatile: the rounding is not to be optimised away
    for (int f = 0; f < n_pairs; f++) {
        bool fin = true;
        for (size_t g = (size_t)first[f] * 2; g < (size_t)first[f + 1] * 2; g++)
            fin = fin && std::isfinite(stage(prev_px[g])) && (!use_guess || std::isfinite(stage(guess_px[g])));
        info[f] = fin ? 0 : 1;
        if (!fin) continue;
        const size_t img = (size_t)rows * cols;
        const int build = max_level > back_level ? max_level : back_level;
        const std::vector<Level> PP = pyramid(prev_img + f * img, rows, cols, win, build), PC = pyramid(cur_img + f * img, rows, cols, win, build);
        const int avail = (int)PP.size() - 1, top_f = max_level < avail ? max_level : avail, top_b = back_level < avail ? back_level : avail;
        int kept = 0;
        for (size_t g = (size_t)first[f]; g < (size_t)first[f + 1]; g++) {
            const double prx = stage(prev_px[2 * g]), pry = stage(prev_px[2 * g + 1]);
            const double inix = use_guess ? stage(guess_px[2 * g]) : prx, iniy = use_guess ? stage(guess_px[2 * g + 1]) : pry;
            Pass F = track(PP, PC, prx, pry, inix, iniy, top_f, win, max_count, eps * eps, min_eig);
            F.x = stage(F.x); F.y = stage(F.y);
            int code = F.lost ? 1 : F.flat ? 2 : 0;
            if (back) {
                Pass B = track(PC, PP, F.x, F.y, prx, pry, top_b, win, max_count, eps * eps, min_eig);
                B.x = stage(B.x); B.y = stage(B.y);
                back_px[2 * g] = B.x; back_px[2 * g + 1] = B.y;
                const double dx = prx - B.x, dy = pry - B.y;
                if (code == 0) code = B.lost ? 3 : B.flat ? 4 : std::sqrt(dx * dx + dy * dy) > back_dist ? 5 : 0;
            }
            if (code == 0) {
                const double rx = std::rint(F.x), ry = std::rint(F.y);
                if (!(rx >= 1.0 && rx < (double)(cols - 1) && ry >= 1.0 && ry < (double)(rows - 1))) code = 6;
            }
            cur_px[2 * g] = F.x; cur_px[2 * g + 1] = F.y;
            why[g] = code; status[g] = code == 0;
            kept += code == 0;
        }
        n_keep[f] = kept;
    }
}
