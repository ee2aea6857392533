// The algorithm of swf_pnp_frame_batch as a plain host loop over the frames, for tests/perf/bench_pnp.py: the sampler, the
// minimal solves from the guess, the scoring, the scan with the adaptive iteration count, the refinement over the inliers and the
// conversion back.  Sums are taken point by point in ascending order.  g++ -O3 -shared -fPIC.
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

bool accumulate(const double* R, const double* t, const double* p, double* acc) {
    const double X = p[0], Y = p[1], Z = p[2], u = p[3], v = p[4];
    const double qx = R[0] * X + R[1] * Y + R[2] * Z, qy = R[3] * X + R[4] * Y + R[5] * Z, qz = R[6] * X + R[7] * Y + R[8] * Z;
    const double x = qx + t[0], y = qy + t[1], z = qz + t[2];
    if (!(std::fabs(z) >= 1e-12)) return false;
    const double iz = 1.0 / z, xn = x * iz, yn = y * iz, jx2 = -(xn * iz), jy2 = -(yn * iz);
    const double g[2][6] = { { jx2 * qy, iz * qz - jx2 * qx, -(iz * qy), iz, 0.0, jx2 }, { jy2 * qy - iz * qz, -(jy2 * qx), iz * qx, 0.0, iz, jy2 } };
    const double r[2] = { xn - u, yn - v };
    for (int w = 0; w < 2; w++) {
        for (int i = 0; i < 6; i++) for (int j = 0; j <= i; j++) acc[i * (i + 1) / 2 + j] += g[w][i] * g[w][j];
        for (int i = 0; i < 6; i++) acc[21 + i] += g[w][i] * r[w];
    }
    return true;
}

bool solve(const double* acc, double* x) {
    double L[21], y[6];
    for (int j = 0; j < 6; j++) {
        double d = acc[j * (j + 1) / 2 + j];
        for (int k = 0; k < j; k++) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (!(d > 0.0)) return false;
        d = std::sqrt(d);
        L[j * (j + 1) / 2 + j] = d;
        for (int i = j + 1; i < 6; i++) {
            double s = acc[i * (i + 1) / 2 + j];
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s / d;
        }
    }
    for (int i = 0; i < 6; i++) {
        double s = -acc[21 + i];
        for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * y[k];
        y[i] = s / L[i * (i + 1) / 2 + i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + i] * x[k];
        x[i] = s / L[i * (i + 1) / 2 + i];
    }
    for (int i = 0; i < 6; i++) if (!std::isfinite(x[i])) return false;
    return true;
}

void update(double* R, double* t, const double* x) {
    const double w[3] = { x[0], x[1], x[2] }, th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
    double a = 1.0, c = 0.0;
    if (th >= 1e-12) { a = std::sin(th) / th; c = (1.0 - std::cos(th)) / (th * th); }
    const double K[9] = { 0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0 };
    double E[9], N[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) E[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K[3 * i + j] + c * (w[i] * w[j] - (i == j ? th2 : 0.0));
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) N[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
    for (int i = 0; i < 9; i++) R[i] = N[i];
    for (int i = 0; i < 3; i++) t[i] += x[3 + i];
}

bool inlier(const double* R, const double* t, const double* p, double thr2) {
    const double x = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0], y = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1];
    const double z = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2];
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z, rx = x * iz - p[3], ry = y * iz - p[4];
    return rx * rx + ry * ry <= thr2;
}

int update_iters(double conf, int count, int n, int m, int n_iters) {
    const double p = std::fmin(std::fmax(conf, 0.0), 1.0), ep = (double)(n - count) / (double)n;
    const double num = std::fmax(1.0 - p, DBL_MIN), w = 1.0 - ep;
    double wm = w;
    for (int i = 1; i < m; i++) wm *= w;
    const double d = 1.0 - wm;
    if (d < DBL_MIN) return 0;
    const double ln = std::log(num), ld = std::log(d);
    if (ld >= 0.0 || -ln >= (double)n_iters * -ld) return n_iters;
    return (int)std::rint(ln / ld);
}

}  // namespace

// info per frame: 0 ok, 1 too few, 2 no model, 3 unrefined
extern "C" void pnp_host(int32_t n_frames, const int32_t* first, const double* pts_w, const double* pts_uv, const double* Ps_prev,
                         const double* Rs_prev, const double* tic, const double* ric, const double* pbg, int32_t iterations, double threshold,
                         double confidence, uint64_t seed, int32_t flags, double* Ps_out, double* Rs_out, int32_t* n_inliers, int32_t* info) {
    const double thr2 = threshold * threshold, d[3] = { tic[0] - pbg[0], tic[1] - pbg[1], tic[2] - pbg[2] };
    std::vector<double> pts, hyp((size_t)iterations * 12);
    std::vector<int> count((size_t)iterations);
    std::vector<char> mask;
    for (int f = 0; f < n_frames; f++) {
        const int p0 = first[f], n = first[f + 1] - p0;
        if (n < 4) { info[f] = 1; continue; }
        pts.resize((size_t)n * 5); mask.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            double c[5] = { pts_w[3 * (size_t)(p0 + i)], pts_w[3 * (size_t)(p0 + i) + 1], pts_w[3 * (size_t)(p0 + i) + 2], pts_uv[2 * (size_t)(p0 + i)], pts_uv[2 * (size_t)(p0 + i) + 1] };
            for (int k = 0; k < 5; k++) pts[(size_t)i * 5 + k] = (flags & 1) ? (double)(float)c[k] : c[k];
        }
        const double *Rp = Rs_prev + (size_t)f * 9, *Pp = Ps_prev + (size_t)f * 3;
        double RC[9], PC[3], R0[9], t0[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) RC[3 * i + j] = Rp[3 * i] * ric[j] + Rp[3 * i + 1] * ric[3 + j] + Rp[3 * i + 2] * ric[6 + j];
            PC[i] = Rp[3 * i] * d[0] + Rp[3 * i + 1] * d[1] + Rp[3 * i + 2] * d[2] + Pp[i];
        }
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R0[3 * i + j] = RC[3 * j + i];
        for (int i = 0; i < 3; i++) t0[i] = -(R0[3 * i] * PC[0] + R0[3 * i + 1] * PC[1] + R0[3 * i + 2] * PC[2]);
        const int m = n >= 5 ? 5 : 4, H = n >= 5 ? iterations : 1;
        int best = -1, best_count = 0, n_iters = H;
        for (int k = 0; k < n_iters && k < H; k++) {              // a host loop stops where the scan stops
            int smp[5] = { 0, 1, 2, 3, -1 }, got = 4;
            if (n >= 5) {
                got = 0;
                for (int j = 0; j < 64 && got < 5; j++) {
                    const uint64_t x = mix(seed + 64ull * (uint64_t)k + (uint64_t)j);
                    const int idx = (int)(((x >> 32) * (uint64_t)n) >> 32);
                    bool dup = false;
                    for (int q = 0; q < got; q++) dup |= smp[q] == idx;
                    if (!dup) smp[got++] = idx;
                }
            }
            double* R = &hyp[(size_t)k * 12];
            double* t = R + 9;
            for (int i = 0; i < 9; i++) R[i] = R0[i];
            for (int i = 0; i < 3; i++) t[i] = t0[i];
            bool valid = got == m;
            for (int step = 0; step < 6 && valid; step++) {
                double acc[27] = { 0 }, x[6];
                for (int q = 0; q < m && valid; q++) valid = accumulate(R, t, &pts[(size_t)smp[q] * 5], acc);
                valid = valid && solve(acc, x);
                if (valid) update(R, t, x);
            }
            int c = 0;
            if (valid) for (int i = 0; i < n; i++) c += inlier(R, t, &pts[(size_t)i * 5], thr2);
            count[(size_t)k] = c;
            if (c > (best_count > m - 1 ? best_count : m - 1)) { best = k; best_count = c; n_iters = update_iters(confidence, c, n, m, n_iters); }
        }
        if (best < 0) { info[f] = 2; continue; }
        double R[9], t[3];
        for (int i = 0; i < 9; i++) R[i] = hyp[(size_t)best * 12 + i];
        for (int i = 0; i < 3; i++) t[i] = hyp[(size_t)best * 12 + 9 + i];
        for (int i = 0; i < n; i++) mask[(size_t)i] = inlier(R, t, &pts[(size_t)i * 5], thr2);
        bool refined = true;
        for (int step = 0; step < 10 && refined; step++) {
            double acc[27] = { 0 }, x[6];
            for (int i = 0; i < n && refined; i++) if (mask[(size_t)i]) refined = accumulate(R, t, &pts[(size_t)i * 5], acc);
            refined = refined && solve(acc, x);
            if (refined) update(R, t, x);
        }
        if (!refined) {
            for (int i = 0; i < 9; i++) R[i] = hyp[(size_t)best * 12 + i];
            for (int i = 0; i < 3; i++) t[i] = hyp[(size_t)best * 12 + 9 + i];
        }
        double PCo[3], RS[9];
        for (int i = 0; i < 3; i++) PCo[i] = R[i] * -t[0] + R[3 + i] * -t[1] + R[6 + i] * -t[2];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) RS[3 * i + j] = R[i] * ric[3 * j] + R[3 + i] * ric[3 * j + 1] + R[6 + i] * ric[3 * j + 2];
        for (int i = 0; i < 3; i++) Ps_out[(size_t)f * 3 + i] = PCo[i] - (RS[3 * i] * d[0] + RS[3 * i + 1] * d[1] + RS[3 * i + 2] * d[2]);
        for (int i = 0; i < 9; i++) Rs_out[(size_t)f * 9 + i] = RS[i];
        n_inliers[f] = best_count;
        info[f] = refined ? 0 : 3;
    }
}
