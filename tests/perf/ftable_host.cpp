// ftable_host.cpp — the specification of the resident feature table (swf_ftable_*, include/swf_solver.h) as a compiled host loop, for
// tests/perf/bench_ftable.py to time against the device: one std::vector of features per stream, the frame's ids sorted and looked
// up in a hash map, every erase a stable compaction, the two-view triangulation by a one-sided Jacobi on the 4 x 4 design matrix.
// Only the operations of the steady-state cycle: add, triangulate, list, check_parallax, slide.  g++ -O3 -shared -fPIC.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace {

struct Obs { double v[7]; bool in_problem; };
struct Feature {
    int id, start, valid, flag;
    double idepth, world[3];
    std::vector<Obs> obs;
    int end_frame() const { return start + (int)obs.size() - 1; }
};
struct Stream { int n_frames = 0; std::vector<Feature> feat; };
struct Host {
    int window, fc, min_track, min_long, long_len;
    double new_ratio, min_parallax, focal, init_depth;
    std::vector<Stream> s;
};

double depth_z(const double* w, const double* P, const double* R, const double* tic, const double* ric, const double* pbg) {
    const double d[3] = { w[0] - P[0], w[1] - P[1], w[2] - P[2] };
    double b[3];
    for (int r = 0; r < 3; r++) b[r] = ((R[r] * d[0] + R[3 + r] * d[1]) + R[6 + r] * d[2] + pbg[r]) - tic[r];
    return (ric[2] * b[0] + ric[5] * b[1]) + ric[8] * b[2];
}

// the camera's 3 x 4 pose [Rc^T | -Rc^T t] of frame (P, R)
void camera_pose(const double* P, const double* R, const double* tic, const double* ric, double M[3][4]) {
    double t[3], Rc[9];
    for (int i = 0; i < 3; i++) {
        t[i] = P[i] + R[3 * i] * tic[0] + R[3 * i + 1] * tic[1] + R[3 * i + 2] * tic[2];
        for (int j = 0; j < 3; j++) Rc[3 * i + j] = R[3 * i] * ric[j] + R[3 * i + 1] * ric[3 + j] + R[3 * i + 2] * ric[6 + j];
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) M[i][j] = Rc[3 * j + i];
        M[i][3] = -(Rc[i] * t[0] + Rc[3 + i] * t[1] + Rc[6 + i] * t[2]);
    }
}

// the right singular vector of the smallest singular value of a 4 x 4 matrix: one-sided Jacobi on its columns
void null_vector(double D[4][4], double x[4]) {
    double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 4; r++) { al += D[r][p] * D[r][p]; be += D[r][q] * D[r][q]; ga += D[r][p] * D[r][q]; }
                if (ga == 0.0 || ga * ga <= 1e-30 * (al * be)) continue;
                const double zeta = (be - al) / (2.0 * ga), t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                for (int r = 0; r < 4; r++) {
                    const double a = D[r][p], b = D[r][q], va = V[r][p], vb = V[r][q];
                    D[r][p] = c * a - sn * b; D[r][q] = sn * a + c * b; V[r][p] = c * va - sn * vb; V[r][q] = sn * va + c * vb;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
    int k = 0;
    double best = 0;
    for (int c = 0; c < 4; c++) {
        double n = 0;
        for (int r = 0; r < 4; r++) n += D[r][c] * D[r][c];
        if (c == 0 || n < best) { best = n; k = c; }
    }
    for (int r = 0; r < 4; r++) x[r] = V[r][k];
}

}  // namespace

extern "C" void* fth_create(int n_streams, int window, int fc, int min_track, int min_long, int long_len, double new_ratio, double min_parallax,
                            double focal, double init_depth) {
    Host* h = new Host{ window, fc, min_track, min_long, long_len, new_ratio, min_parallax, focal, init_depth, {} };
    h->s.resize((size_t)n_streams);
    return h;
}

extern "C" void fth_destroy(void* p) { delete (Host*)p; }

extern "C" void fth_add(void* p, const int32_t* first, const int32_t* ids, const double* obs, int32_t* keyframe) {
    Host* h = (Host*)p;
    std::vector<std::pair<int, int>> order;
    std::unordered_map<int, int> where;
    for (size_t si = 0; si < h->s.size(); si++) {
        Stream& S = h->s[si];
        if (S.n_frames >= h->window) { keyframe[si] = 0; continue; }
        const int p0 = first[si], n = first[si + 1] - p0, image_index = S.n_frames;
        order.clear(); where.clear();
        for (int i = 0; i < n; i++) order.emplace_back(ids[p0 + i], i);
        std::sort(order.begin(), order.end());
        for (size_t i = 0; i < S.feat.size(); i++) where[S.feat[i].id] = (int)i;
        int last = 0, lng = 0, fresh = 0;
        for (const auto& it : order) {
            Obs o;
            std::memcpy(o.v, obs + 7 * (size_t)(p0 + it.second), sizeof(o.v));
            o.in_problem = false;
            const auto f = where.find(it.first);
            if (f == where.end()) {
                Feature nf{ it.first, image_index, 0, 0, 0.0, { 0, 0, 0 }, {} };
                nf.obs.push_back(o);
                S.feat.push_back(std::move(nf));
                fresh++;
            } else {
                Feature& ft = S.feat[(size_t)f->second];
                ft.obs.push_back(o);
                last++;
                if ((int)ft.obs.size() >= h->long_len) lng++;
            }
        }
        keyframe[si] = image_index < 2 || last < h->min_track || lng < h->min_long || (double)fresh > h->new_ratio * (double)last;
        S.n_frames++;
        const int nf = S.n_frames, fc = h->fc;
        S.feat.erase(std::remove_if(S.feat.begin(), S.feat.end(), [nf, fc](const Feature& f) { return f.end_frame() != nf - 1 && (int)f.obs.size() < fc; }),
                     S.feat.end());
    }
}

extern "C" void fth_triangulate(void* p, const double* Ps, const double* Rs, const double* tic, const double* ric, const double* pbg) {
    Host* h = (Host*)p;
    for (size_t si = 0; si < h->s.size(); si++) {
        const double* P = Ps + si * (size_t)h->window * 3;
        const double* R = Rs + si * (size_t)h->window * 9;
        for (Feature& f : h->s[si].feat) {
            if (f.valid || f.obs.size() < 2) continue;
            double M0[3][4], M1[3][4], D[4][4], x[4];
            camera_pose(P + 3 * f.start, R + 9 * f.start, tic, ric, M0);
            camera_pose(P + 3 * (f.start + 1), R + 9 * (f.start + 1), tic, ric, M1);
            const double u0 = f.obs[0].v[0], v0 = f.obs[0].v[1], u1 = f.obs[1].v[0], v1 = f.obs[1].v[1];
            for (int c = 0; c < 4; c++) {
                D[0][c] = u0 * M0[2][c] - M0[0][c]; D[1][c] = v0 * M0[2][c] - M0[1][c];
                D[2][c] = u1 * M1[2][c] - M1[0][c]; D[3][c] = v1 * M1[2][c] - M1[1][c];
            }
            null_vector(D, x);
            const double X[3] = { x[0] / x[3], x[1] / x[3], x[2] / x[3] };
            double depth = M0[2][0] * X[0] + M0[2][1] * X[1] + M0[2][2] * X[2] + M0[2][3];
            if (!(depth > 0)) depth = h->init_depth;
            const double pc[3] = { u0 * depth, v0 * depth, depth };
            const double* Pi = P + 3 * f.start; const double* Ri = R + 9 * f.start;
            double pb[3];
            for (int r = 0; r < 3; r++) pb[r] = ric[3 * r] * pc[0] + ric[3 * r + 1] * pc[1] + ric[3 * r + 2] * pc[2] + tic[r] - pbg[r];
            for (int r = 0; r < 3; r++) f.world[r] = Ri[3 * r] * pb[0] + Ri[3 * r + 1] * pb[1] + Ri[3 * r + 2] * pb[2] + Pi[r];
            f.idepth = 1.0 / depth;
            f.valid = 1;
        }
    }
}

extern "C" void fth_list(void* p, int32_t* lm_first, int32_t* proj_first, int32_t* lm_id, double* lm_world, int32_t* lm_start, int32_t* lm_nobs,
                         int32_t* lm_valid, int32_t* proj_frame, int32_t* proj_lm, double* proj_uv, int32_t* proj_new) {
    Host* h = (Host*)p;
    int nl = 0, np = 0;
    for (size_t si = 0; si < h->s.size(); si++) {
        lm_first[si] = nl; proj_first[si] = np;
        int j = 0;
        for (Feature& f : h->s[si].feat) {
            if ((int)f.obs.size() < h->fc) continue;
            lm_id[nl] = f.id; lm_start[nl] = f.start; lm_nobs[nl] = (int)f.obs.size(); lm_valid[nl] = f.valid;
            std::memcpy(lm_world + 3 * (size_t)nl, f.world, sizeof(f.world));
            for (size_t k = 0; k < f.obs.size(); k++) {
                proj_frame[np] = f.start + (int)k; proj_lm[np] = j; proj_uv[2 * (size_t)np] = f.obs[k].v[0]; proj_uv[2 * (size_t)np + 1] = f.obs[k].v[1];
                proj_new[np] = f.obs[k].in_problem ? 0 : 1;
                f.obs[k].in_problem = true;
                np++;
            }
            nl++; j++;
        }
    }
    lm_first[h->s.size()] = nl; proj_first[h->s.size()] = np;
}

extern "C" void fth_parallax(void* p, int32_t* keyframe, double* parallax) {
    Host* h = (Host*)p;
    for (size_t si = 0; si < h->s.size(); si++) {
        const int idx = h->s[si].n_frames - 1;
        double sum = 0;
        int num = 0;
        for (const Feature& f : h->s[si].feat) {
            if (!(f.start <= idx - 2 && f.end_frame() >= idx - 1)) continue;
            const double* oi = f.obs[(size_t)(idx - 2 - f.start)].v; const double* oj = f.obs[(size_t)(idx - 1 - f.start)].v;
            const double du = oi[0] / oi[2] - oj[0], dv = oi[1] / oi[2] - oj[1];
            sum += std::sqrt(du * du + dv * dv);
            num++;
        }
        keyframe[si] = num == 0 || sum / num >= h->min_parallax;
        parallax[si] = num ? sum / num * h->focal : 0.0;
    }
}

extern "C" void fth_slide(void* p, const int32_t* mode, const double* P1, const double* R1, const double* tic, const double* ric, const double* pbg) {
    Host* h = (Host*)p;
    for (size_t si = 0; si < h->s.size(); si++) {
        Stream& S = h->s[si];
        if (mode[si] == 0 || S.n_frames < 2) continue;
        const int front = S.n_frames - 1;
        for (Feature& f : S.feat) {
            if (mode[si] == 1) {
                if (f.start != 0) f.start--;
                else {
                    f.idepth = 1.0 / depth_z(f.world, P1 + 3 * si, R1 + 9 * si, tic, ric, pbg);
                    f.obs.erase(f.obs.begin());
                }
            } else if (f.start == front) f.start--;
            else if (f.end_frame() >= front - 1) f.obs.erase(f.obs.begin() + (front - 1 - f.start));
        }
        S.feat.erase(std::remove_if(S.feat.begin(), S.feat.end(), [](const Feature& f) { return f.obs.empty(); }), S.feat.end());
        S.n_frames--;
        for (Feature& f : S.feat)
            if ((int)f.obs.size() < h->fc)
                for (Obs& o : f.obs) o.in_problem = false;
    }
}

extern "C" void fth_state(void* p, int32_t* n_frames, int32_t* n_feat) {
    Host* h = (Host*)p;
    for (size_t si = 0; si < h->s.size(); si++) { n_frames[si] = h->s[si].n_frames; n_feat[si] = (int)h->s[si].feat.size(); }
}
