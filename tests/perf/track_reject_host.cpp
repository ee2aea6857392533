// The algorithm of swf_track_reject_batch as a plain host loop over the pairs, for tests/perf/bench_track_reject.py: the
// lift with its nine steps, the virtual camera, the sampler, the 8-point solves (Householder null vector, Jacobi rank 2), the scoring
// and the scan with the adaptive iteration count, which stops drawing hypotheses where the scan stops.  g++ -O3 -shared -fPIC.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

uint64_t mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void lift(const double* cam, double px, double py, double* out) {
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7];
    const double k3 = cam[8], k4 = cam[9], k5 = cam[10], k6 = cam[11];
    const double x0 = px / fx - cx / fx, y0 = py / fy - cy / fy;
    double x = x0, y = y0;
    for (int j = 0; j < 9; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
    }
    out[0] = x; out[1] = y;
}

bool inlier(const double* F, const double* m, double thr2) {
    const double u1 = m[0], v1 = m[1], u2 = m[2], v2 = m[3];
    const double a = F[0] * u1 + F[1] * v1 + F[2], b = F[3] * u1 + F[4] * v1 + F[5], c = F[6] * u1 + F[7] * v1 + F[8];
    const double n2 = u2 * a + v2 * b + c, d2 = n2 * n2 / (a * a + b * b);
    const double at = F[0] * u2 + F[3] * v2 + F[6], bt = F[1] * u2 + F[4] * v2 + F[7], ct = F[2] * u2 + F[5] * v2 + F[8];
    const double n1 = u1 * at + v1 * bt + ct, d1 = n1 * n1 / (at * at + bt * bt);
    return d1 <= thr2 && d2 <= thr2;
}

int update_iters(double conf, int count, int n, int m, int n_iters) {
    const double p = std::fmin(std::fmax(conf, 0.0), 1.0), ep = std::fmin(std::fmax((double)(n - count) / n, 0.0), 1.0);
    const double num = std::fmax(1.0 - p, DBL_MIN), w = 1.0 - ep;
    double wm = w;
    for (int i = 1; i < m; i++) wm *= w;
    const double d = 1.0 - wm;
    if (d < DBL_MIN) return 0;
    const double ln = std::log(num), ld = std::log(d);
    if (ld >= 0.0 || -ln >= n_iters * -ld) return n_iters;
    return (int)std::rint(ln / ld);
}

// virt [n][4]; false where the hypothesis is invalid
bool hypothesis(const double* virt, int n, int k, uint64_t seed, double* F) {
    int smp[8], got = 0;
    if (n == 8) { for (int q = 0; q < 8; q++) smp[q] = q; got = 8; }
    else for (int j = 0; j < 64 && got < 8; j++) {
        const uint64_t x = mix(seed + 64ull * (uint64_t)k + (uint64_t)j);
        const int idx = (int)(((x >> 32) * (uint64_t)n) >> 32);
        bool dup = false;
        for (int q = 0; q < got; q++) dup |= smp[q] == idx;
        if (!dup) smp[got++] = idx;
    }
    if (got != 8) return false;
    double c[4] = { 0, 0, 0, 0 };
    for (int q = 0; q < 8; q++) for (int w = 0; w < 4; w++) c[w] += virt[4 * smp[q] + w];
    for (int w = 0; w < 4; w++) c[w] *= 0.125;
    double m1 = 0, m2 = 0;
    for (int q = 0; q < 8; q++) {
        const double* m = virt + 4 * smp[q];
        m1 += std::sqrt((m[0] - c[0]) * (m[0] - c[0]) + (m[1] - c[1]) * (m[1] - c[1]));
        m2 += std::sqrt((m[2] - c[2]) * (m[2] - c[2]) + (m[3] - c[3]) * (m[3] - c[3]));
    }
    m1 *= 0.125; m2 *= 0.125;
    if (!(m1 >= 0x1p-23) || !(m2 >= 0x1p-23)) return false;
    const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
    double hv[8][9], hb[8];
    for (int j = 0; j < 8; j++) {
        const double* m = virt + 4 * smp[j];
        const double x1 = (m[0] - c[0]) * s1, y1 = (m[1] - c[1]) * s1, x2 = (m[2] - c[2]) * s2, y2 = (m[3] - c[3]) * s2;
        double a[9] = { x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0 };
        for (int i = 0; i < j; i++) {
            double d = 0;
            for (int r = i; r < 9; r++) d += hv[i][r] * a[r];
            d *= hb[i];
            for (int r = i; r < 9; r++) a[r] -= d * hv[i][r];
        }
        double s = 0;
        for (int r = j; r < 9; r++) s += a[r] * a[r];
        const double nrm = std::sqrt(s);
        for (int r = j; r < 9; r++) hv[j][r] = a[r];
        hv[j][j] = a[j] >= 0.0 ? a[j] + nrm : a[j] - nrm;
        hb[j] = 1.0 / (nrm * (nrm + std::fabs(a[j])));
    }
    double g[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 1 };
    for (int i = 7; i >= 0; i--) {
        double d = 0;
        for (int r = i; r < 9; r++) d += hv[i][r] * g[r];
        d *= hb[i];
        for (int r = i; r < 9; r++) g[r] -= d * hv[i][r];
    }
    double V[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    for (int sweep = 0; sweep < 6; sweep++)
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double aa = g[p] * g[p] + g[3 + p] * g[3 + p] + g[6 + p] * g[6 + p], bb = g[q] * g[q] + g[3 + q] * g[3 + q] + g[6 + q] * g[6 + q];
            const double cc = g[p] * g[q] + g[3 + p] * g[3 + q] + g[6 + p] * g[6 + q];
            const double zeta = (bb - aa) / (2.0 * cc);
            double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
            if (cc == 0.0 || !(t == t)) t = 0.0;
            const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
            for (int r = 0; r < 3; r++) {
                const double gp = g[3 * r + p], gq = g[3 * r + q], vp = V[3 * r + p], vq = V[3 * r + q];
                g[3 * r + p] = cs * gp - sn * gq; g[3 * r + q] = sn * gp + cs * gq;
                V[3 * r + p] = cs * vp - sn * vq; V[3 * r + q] = sn * vp + cs * vq;
            }
        }
    double nn[3];
    for (int p = 0; p < 3; p++) nn[p] = g[p] * g[p] + g[3 + p] * g[3 + p] + g[6 + p] * g[6 + p];
    int drop = 0;
    if (nn[1] < nn[drop]) drop = 1;
    if (nn[2] < nn[drop]) drop = 2;
    double F0[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int p = 0; p < 3; p++) if (p != drop) s += g[3 * i + p] * V[3 * j + p];
        F0[3 * i + j] = s;
    }
    const double tx1 = -(c[0] * s1), ty1 = -(c[1] * s1), tx2 = -(c[2] * s2), ty2 = -(c[3] * s2);
    double M[9];
    for (int i = 0; i < 3; i++) {
        M[3 * i] = F0[3 * i] * s1; M[3 * i + 1] = F0[3 * i + 1] * s1;
        M[3 * i + 2] = F0[3 * i] * tx1 + F0[3 * i + 1] * ty1 + F0[3 * i + 2];
    }
    bool ok = true;
    for (int j = 0; j < 3; j++) {
        F[j] = s2 * M[j]; F[3 + j] = s2 * M[3 + j]; F[6 + j] = tx2 * M[j] + ty2 * M[3 + j] + M[6 + j];
    }
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(F[i]);
    return ok;
}

}  // namespace

extern "C" void track_reject_host(int32_t n_pairs, const int32_t* first, const double* cur_px, const double* prev_px, const double* cam,
                                  int32_t col, int32_t row, double focal, const double* dt, int32_t iterations, double threshold,
                                  double confidence, uint64_t seed, int32_t flags, uint8_t* status, int32_t* n_inliers, int32_t* info,
                                  double* un_cur, double* velocity) {
    const bool fl = (flags & 1) != 0;
    const double thr2 = threshold * threshold;
    std::vector<double> virt;
    for (int f = 0; f < n_pairs; f++) {
        const int p0 = first[f], n = first[f + 1] - p0;
        virt.assign((size_t)n * 4, 0.0);
        bool bad = !std::isfinite(dt[f]) || !(dt[f] > 0.0);
        for (int i = 0; i < n && !bad; i++) {
            double px[4] = { cur_px[2 * (p0 + i)], cur_px[2 * (p0 + i) + 1], prev_px[2 * (p0 + i)], prev_px[2 * (p0 + i) + 1] };
            for (int k = 0; k < 4; k++) { if (fl) px[k] = (double)(float)px[k]; bad = bad || !std::isfinite(px[k]); }
            if (bad) break;
            double xc[2], xp[2];
            lift(cam, px[0], px[1], xc); lift(cam, px[2], px[3], xp);
            double* v = &virt[(size_t)i * 4];
            v[0] = focal * xc[0] + col / 2.0; v[1] = focal * xc[1] + row / 2.0; v[2] = focal * xp[0] + col / 2.0; v[3] = focal * xp[1] + row / 2.0;
            for (int k = 0; k < 2; k++) {
                if (fl) {
                    v[k] = (double)(float)v[k]; v[2 + k] = (double)(float)v[2 + k];
                    xc[k] = (double)(float)xc[k]; xp[k] = (double)(float)xp[k];
                    velocity[2 * (p0 + i) + k] = (double)(float)((double)((float)xc[k] - (float)xp[k]) / dt[f]);
                } else velocity[2 * (p0 + i) + k] = (xc[k] - xp[k]) / dt[f];
                un_cur[2 * (p0 + i) + k] = xc[k];
            }
        }
        if (bad) { info[f] = 3; continue; }
        if (n < 8) { info[f] = 1; continue; }
        const int H = n == 8 ? 1 : iterations;
        int best = -1, best_count = 0, n_iters = H;
        double Fb[9], F[9];
        for (int k = 0; k < n_iters; k++) {
            if (!hypothesis(virt.data(), n, k, seed, F)) continue;
            int cnt = 0;
            for (int i = 0; i < n; i++) cnt += inlier(F, &virt[(size_t)i * 4], thr2);
            if (cnt > (best_count > 7 ? best_count : 7)) {
                best = k; best_count = cnt;
                for (int i = 0; i < 9; i++) Fb[i] = F[i];
                n_iters = update_iters(confidence, cnt, n, 8, n_iters);
            }
        }
        if (best < 0) { info[f] = 2; continue; }
        for (int i = 0; i < n; i++) status[p0 + i] = inlier(Fb, &virt[(size_t)i * 4], thr2);
        n_inliers[f] = best_count; info[f] = 0;
    }
}
