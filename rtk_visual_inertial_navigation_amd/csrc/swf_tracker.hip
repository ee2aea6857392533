// swf_tracker.hip — the bookkeeping kernels of the resident feature tracker (see swf_tracker.h) and the C-ABI swf_tracker_*.
// gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_tracker.h"
#include "swf_klt.h"
#include "swf_trackreject.h"
#include "swf_trk_lift.h"

void swf_internal_set_error(const std::string& m);
static int tracker_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int tracker_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the sum of cnt(g) over the streams g < s in front of this workgroup's; every thread calls it, once per kernel
template <class F> __device__ __forceinline__ int tracker_offset(int s, F cnt) {
    __shared__ int s_sum[TRACKER_THREADS / 64];
    const int tid = threadIdx.x;
    int part = 0;
    for (int g = tid; g < s; g += TRACKER_THREADS) part += cnt(g);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    return s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// the points stream g keeps after the KLT: n_keep of a pair the KLT accepted, within what the stream had
__device__ __forceinline__ int tracker_cnt1(const TrackerArgs& P, int g) {
    if (!P.have_klt || P.kinfo[g] != SWF_KLT_OK) return 0;
    return tracker_clamp(P.nk1[g], 0, tracker_clamp(P.S.first[g + 1] - P.S.first[g], 0, P.max_cnt));
}

__global__ void __launch_bounds__(TRACKER_THREADS) k_tracker_after_klt(TrackerArgs P) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int p0 = P.S.first[s], n_in = tracker_clamp(P.S.first[s + 1] - p0, 0, P.max_cnt), cnt = tracker_cnt1(P, s);
    const int off = tracker_offset(s, [&](int g) { return tracker_cnt1(P, g); });
    const int ki = P.have_klt ? P.kinfo[s] : SWF_KLT_OK;
    if (tid == 0) {
        P.first1[s] = off;
        if (s == P.n_streams - 1) P.first1[s + 1] = off + cnt;
        int* c = P.counts + (size_t)s * SWF_TRACKER_NCOUNT;
        c[SWF_TRACKER_C_IN] = n_in; c[SWF_TRACKER_C_KLT] = cnt; c[SWF_TRACKER_C_KLT_INFO] = ki;
        P.info[s] = ki != SWF_KLT_OK ? SWF_TRACKER_STAGE_FAILED : 0;
    }
    for (int j = tid; j < cnt; j += TRACKER_THREADS) {
        const int i = P.k1[(size_t)p0 + j];
        const size_t g = (size_t)p0 + (size_t)(i >= 0 && i < n_in ? i : j), at = (size_t)off + j;
        P.pxp1[2 * at] = P.S.px[2 * g]; P.pxp1[2 * at + 1] = P.S.px[2 * g + 1];
        P.pxc1[2 * at] = P.cur1[2 * g]; P.pxc1[2 * at + 1] = P.cur1[2 * g + 1];
        P.ids1[at] = P.S.ids[g];
        P.tc1[at] = P.S.tc[g] + 1;                          // for (auto& n : track_cnt) n++
        P.lin1[at] = P.S.lin[g];
    }
}

// the points stream g keeps after the gate: the inliers of a pair with a model, every point otherwise (n < 8, no model)
__device__ __forceinline__ int tracker_cnt2(const TrackerArgs& P, int g) {
    const int n = tracker_clamp(P.first1[g + 1] - P.first1[g], 0, P.max_cnt);
    return P.tinfo[g] == SWF_TRK_OK ? tracker_clamp(P.ni2[g], 0, n) : n;
}

__global__ void __launch_bounds__(TRACKER_THREADS) k_tracker_after_f(TrackerArgs P) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int p0 = P.first1[s], n = tracker_clamp(P.first1[s + 1] - p0, 0, P.max_cnt), cnt = tracker_cnt2(P, s), ti = P.tinfo[s];
    const int off = tracker_offset(s, [&](int g) { return tracker_cnt2(P, g); });
    if (tid == 0) {
        P.first2[s] = off;
        if (s == P.n_streams - 1) P.first2[s + 1] = off + cnt;
        int* c = P.counts + (size_t)s * SWF_TRACKER_NCOUNT;
        c[SWF_TRACKER_C_F] = cnt; c[SWF_TRACKER_C_TRK_INFO] = ti;
        if (ti == SWF_TRK_NO_MODEL) P.info[s] |= SWF_TRACKER_NO_MODEL;
        if (ti == SWF_TRK_BAD_INPUT || ti < 0 || ti > SWF_TRK_BAD_INPUT) P.info[s] |= SWF_TRACKER_STAGE_FAILED;
    }
    for (int j = tid; j < cnt; j += TRACKER_THREADS) {
        const int i = ti == SWF_TRK_OK ? P.k2[(size_t)p0 + j] : j;
        const size_t g = (size_t)p0 + (size_t)(i >= 0 && i < n ? i : j), at = (size_t)off + j;
        P.px2[2 * at] = P.pxc1[2 * g]; P.px2[2 * at + 1] = P.pxc1[2 * g + 1];
        P.ids2[at] = P.ids1[g];
        P.tc2[at] = P.tc1[g];
        P.lin2[at] = P.lin1[g];
    }
}

__device__ __forceinline__ const GfttHead* tracker_head(const TrackerArgs& P, int g) {
    return (const GfttHead*)(P.work + (size_t)g * P.L.bytes + P.L.head);
}

// the points of stream g's final list: the detector's packed range, what setMask kept of a TOO_MANY frame, every point otherwise
__device__ __forceinline__ int tracker_cnt3(const TrackerArgs& P, int g) {
    const int n = tracker_clamp(P.first2[g + 1] - P.first2[g], 0, P.max_cnt), gi = P.ginfo[g];
    if (gi == SWF_GFTT_OK) return tracker_clamp(P.pf3[g + 1] - P.pf3[g], 0, P.max_cnt);
    if (gi == SWF_GFTT_TOO_MANY) return tracker_clamp(tracker_head(P, g)->n_old, 0, n);
    return n;
}

__global__ void __launch_bounds__(TRACKER_THREADS) k_tracker_finish(TrackerArgs P) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int p0 = P.first2[s], n = tracker_clamp(P.first2[s + 1] - p0, 0, P.max_cnt), gi = P.ginfo[s], tot = tracker_cnt3(P, s);
    const int off = tracker_offset(s, [&](int g) { return tracker_cnt3(P, g); });
    const int n_old = gi == SWF_GFTT_OK ? tracker_clamp(P.nold3[s], 0, tot) : tot, n_new = tot - n_old;
    const int id0 = P.n_id[s], q0 = gi == SWF_GFTT_OK ? P.pf3[s] : 0;
    const int* kept_i = (const int*)(P.work + (size_t)s * P.L.bytes + P.L.kept_i);
    const double dt = P.dt[s];
    __syncthreads();                                        // n_id[s] is read by every thread before thread 0 moves it on
    if (tid == 0) {
        P.S.first[s] = off; P.ffirst[s] = off;
        if (s == P.n_streams - 1) { P.S.first[s + 1] = off + tot; P.ffirst[s + 1] = off + tot; }
        P.n_id[s] = id0 + n_new;
        int* c = P.counts + (size_t)s * SWF_TRACKER_NCOUNT;
        c[SWF_TRACKER_C_MASK] = n_old; c[SWF_TRACKER_C_NEW] = n_new;
        c[SWF_TRACKER_C_CAND] = gi == SWF_GFTT_OK || gi == SWF_GFTT_TOO_MANY ? P.ncand3[s] : 0;
        c[SWF_TRACKER_C_FINAL] = tot; c[SWF_TRACKER_C_GFTT_INFO] = gi;
        if (gi == SWF_GFTT_TOO_MANY) P.info[s] |= SWF_TRACKER_TOO_MANY;
        if (gi != SWF_GFTT_OK && gi != SWF_GFTT_TOO_MANY) P.info[s] |= SWF_TRACKER_STAGE_FAILED;
    }
    for (int j = tid; j < tot; j += TRACKER_THREADS) {
        const size_t at = (size_t)off + j;
        int src;
        double x, y;
        if (gi == SWF_GFTT_OK) {
            const size_t q = (size_t)q0 + j;
            src = j < n_old ? P.psrc3[q] : -1;
            x = P.ppx3[2 * q]; y = P.ppx3[2 * q + 1];
        } else {
            src = gi == SWF_GFTT_TOO_MANY ? kept_i[j] : j;
        }
        if (src >= n) src = j < n ? j : -1;                 // no valid state gets here
        if (gi != SWF_GFTT_OK) {
            const size_t g = (size_t)p0 + (size_t)max(src, 0);
            x = (double)(float)P.px2[2 * g]; y = (double)(float)P.px2[2 * g + 1];
        }
        int id = id0 + (j - n_old), tc = 1, lin = -1;       // addPoints
        if (src >= 0) { const size_t g = (size_t)p0 + src; id = P.ids2[g]; tc = P.tc2[g]; lin = P.lin2[g]; }
        double ux, uy;
        trk_lift(P.cam, x, y, ux, uy);                      // undistortedPts: the operator's un_cur under flag bit 0
        ux = (double)(float)ux; uy = (double)(float)uy;
        double vx = 0.0, vy = 0.0;
        if (lin >= 0) {                                     // ptsVelocity: the id was in the previous frame's final list
            vx = trk_velocity(ux, P.obs_prev[7 * (size_t)lin], dt, true);
            vy = trk_velocity(uy, P.obs_prev[7 * (size_t)lin + 1], dt, true);
        }
        double* o = P.obs + 7 * at;
        o[0] = ux; o[1] = uy; o[2] = 1.0; o[3] = x; o[4] = y; o[5] = vx; o[6] = vy;
        P.fpx[2 * at] = x; P.fpx[2 * at + 1] = y; P.fids[at] = id; P.ftc[at] = tc;
        P.S.px[2 * at] = x; P.S.px[2 * at + 1] = y; P.S.ids[at] = id; P.S.tc[at] = tc; P.S.lin[at] = (int)at;
    }
}

// removeOutliers, first half: the indices of the points of stream s whose id is not in the stream's list, ascending, and their number
__global__ void __launch_bounds__(TRACKER_THREADS) k_tracker_mark(TrackerArgs P) {
    __shared__ int s_rm[SWF_GFTT_NMAX];
    __shared__ int s_wave[TRACKER_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = P.S.first[s], n = tracker_clamp(P.S.first[s + 1] - p0, 0, P.max_cnt);
    const int r0 = P.rm_first[s], nr = tracker_clamp(P.rm_first[s + 1] - r0, 0, min(P.max_cnt, (int)SWF_GFTT_NMAX));
    for (int i = tid; i < nr; i += TRACKER_THREADS) s_rm[i] = P.rm_ids[(size_t)r0 + i];
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += TRACKER_THREADS) {       // uniform: n is the workgroup's
        const int i = c0 + tid;
        bool keep = i < n;
        if (keep) {
            const int id = P.S.ids[(size_t)p0 + i];
            for (int k = 0; k < nr; k++) keep = keep && s_rm[k] != id;
        }
        const u64 b = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < TRACKER_THREADS / 64; w++) { before += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
        if (keep) P.krm[(size_t)p0 + base + before + __popcll(b & ((1ull << lane) - 1ull))] = i;
        base += all;
        __syncthreads();                                    // s_wave is rewritten by the next chunk
    }
    if (tid == 0) P.nkrm[s] = base;
}

__device__ __forceinline__ int tracker_cntr(const TrackerArgs& P, int g) {
    return tracker_clamp(P.nkrm[g], 0, tracker_clamp(P.S.first[g + 1] - P.S.first[g], 0, P.max_cnt));
}

// removeOutliers, second half: the state gathered into the other set
__global__ void __launch_bounds__(TRACKER_THREADS) k_tracker_gather(TrackerArgs P) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int p0 = P.S.first[s], n = tracker_clamp(P.S.first[s + 1] - p0, 0, P.max_cnt), cnt = tracker_cntr(P, s);
    const int off = tracker_offset(s, [&](int g) { return tracker_cntr(P, g); });
    if (tid == 0) {
        P.D.first[s] = off;
        if (s == P.n_streams - 1) P.D.first[s + 1] = off + cnt;
    }
    for (int j = tid; j < cnt; j += TRACKER_THREADS) {
        const int i = P.krm[(size_t)p0 + j];
        const size_t g = (size_t)p0 + (size_t)(i >= 0 && i < n ? i : j), at = (size_t)off + j;
        P.D.px[2 * at] = P.S.px[2 * g]; P.D.px[2 * at + 1] = P.S.px[2 * g + 1];
        P.D.ids[at] = P.S.ids[g]; P.D.tc[at] = P.S.tc[g]; P.D.lin[at] = P.S.lin[g];
    }
}

}  // namespace

struct swf_tracker {
    int n_streams = 0, rows = 0, cols = 0;
    swf_tracker_options opt{};
    hipStream_t st = nullptr;
    long long frames = 0;                                   // swf_tracker_track calls that were enqueued
    int set = 0;                                            // the state set in use
    std::vector<void*> bufs;
    std::vector<double> prev_time, h_dt;
    unsigned char* img[2] = { nullptr, nullptr };
    unsigned char* mask = nullptr; unsigned char* pyr = nullptr; unsigned char* work = nullptr;
    TrackerState S[2]{};
    double* obs[2] = { nullptr, nullptr };
    double* dt = nullptr;
    int* rm_first = nullptr; int* rm_ids = nullptr;
    TrackerArgs P{};                                        // every pointer that does not change from call to call
    KltArgs K{}; TrkArgs R{}; GfttArgs G{};
};

namespace {

template <class T> bool tracker_alloc(swf_tracker* t, T*& p, size_t n, bool zero) {
    void* d = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 8);
    if (hipMalloc(&d, bytes) != hipSuccess) return false;
    t->bufs.push_back(d);
    p = (T*)d;
    return !zero || hipMemsetAsync(d, 0, bytes, t->st) == hipSuccess;
}

void tracker_free(swf_tracker* t) {
    for (void* p : t->bufs) (void)hipFree(p);
    delete t;
}

bool tracker_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return true;
    swf_internal_set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

}  // namespace

// C-ABI, include/swf_solver.h
extern "C" void swf_tracker_default_options(swf_tracker_options* o) {
    if (!o) return;
    *o = swf_tracker_options{};
    o->max_cnt = 350; o->min_dist = 30; o->quality = 0.01; o->cand_cap = 1 << 15;
    o->win = 21; o->max_level = 3; o->back_level = 1; o->max_count = 30; o->eps = 0.01; o->min_eig = 1e-4; o->back_dist = 0.5; o->flow_back = 1;
    o->f_iterations = 1000; o->f_threshold = 1.0; o->f_confidence = 0.99; o->focal = 1000.0; o->virt_col = 0; o->virt_row = 0;
}

extern "C" int swf_tracker_create(int32_t n_streams, int32_t rows, int32_t cols, const double cam[12], const swf_tracker_options* opt,
                                  void* stream, swf_tracker** out) {
    const std::string who = "swf_tracker_create";
    if (out) *out = nullptr;
    if (!cam || !opt || !out) return tracker_fail(SWF_E_INVALID, who + ": null argument");
    const swf_tracker_options& o = *opt;
    // ---- the limits of swf_klt_track_batch, swf_track_reject_batch and swf_gftt_detect_batch, before the device is touched
    if (!std::isfinite(o.eps) || !(o.eps > 0.0) || !std::isfinite(o.min_eig) || !(o.min_eig > 0.0) || !std::isfinite(o.back_dist) || !(o.back_dist > 0.0))
        return tracker_fail(SWF_E_INVALID, who + ": eps, min_eig and back_dist must be finite and positive");
    if (!std::isfinite(o.f_threshold) || !(o.f_threshold > 0.0) || !std::isfinite(o.focal) || !(o.focal > 0.0) || !std::isfinite(o.f_confidence))
        return tracker_fail(SWF_E_INVALID, who + ": the threshold and the focal length must be finite and positive and the confidence finite");
    for (int k = 0; k < 12; k++) if (!std::isfinite(cam[k])) return tracker_fail(SWF_E_INVALID, who + ": non-finite camera parameters");
    if (cam[0] == 0.0 || cam[1] == 0.0) return tracker_fail(SWF_E_INVALID, who + ": fx and fy must not be 0");
    if (!(o.quality > 0.0) || !(o.quality <= 1.0)) return tracker_fail(SWF_E_INVALID, who + ": quality must lie in (0, 1]");
    if (o.cand_cap < 64) return tracker_fail(SWF_E_INVALID, who + ": cand_cap below 64");
    if (n_streams < 1 || n_streams > 65535) return tracker_fail(SWF_E_UNSUPPORTED, who + ": n_streams outside 1 .. 65535");
    if (o.win < 3 || o.win > SWF_KLT_WMAX || (o.win & 1) == 0) return tracker_fail(SWF_E_UNSUPPORTED, who + ": the window side must be odd, 3 .. 21");
    if (rows <= o.win || cols <= o.win || rows < 8 || cols < 8 || rows > 8192 || cols > 8192)
        return tracker_fail(SWF_E_UNSUPPORTED, who + ": rows and cols must be above win, at least 8 and at most 8192");
    if (o.max_level < 0 || o.max_level > SWF_KLT_LMAX || o.back_level < 0 || o.back_level > SWF_KLT_LMAX)
        return tracker_fail(SWF_E_UNSUPPORTED, who + ": max_level and back_level outside 0 .. 4");
    if (o.max_count < 1 || o.max_count > 1000) return tracker_fail(SWF_E_UNSUPPORTED, who + ": max_count outside 1 .. 1000");
    if (o.max_cnt < 1 || o.max_cnt > SWF_GFTT_NMAX) return tracker_fail(SWF_E_UNSUPPORTED, who + ": max_cnt outside 1 .. 1024");
    if (o.min_dist < 1 || o.min_dist > GFTT_RMAX) return tracker_fail(SWF_E_UNSUPPORTED, who + ": min_dist outside 1 .. 64");
    if (o.cand_cap > (1 << 24)) return tracker_fail(SWF_E_UNSUPPORTED, who + ": cand_cap above 2^24");
    if (o.f_iterations < 1 || o.f_iterations > SWF_TRK_HMAX) return tracker_fail(SWF_E_UNSUPPORTED, who + ": f_iterations outside 1 .. 1024");
    if (o.virt_col < 0 || o.virt_row < 0) return tracker_fail(SWF_E_UNSUPPORTED, who + ": a negative virtual image size");

    swf_tracker* t = new swf_tracker;
    t->n_streams = n_streams; t->rows = rows; t->cols = cols; t->opt = o; t->st = (hipStream_t)stream;
    t->prev_time.assign((size_t)n_streams, 0.0); t->h_dt.assign((size_t)n_streams, 1.0);
    const size_t ns = (size_t)n_streams, T = ns * (size_t)o.max_cnt, img_bytes = (size_t)rows * (size_t)cols;

    // ---- the three operators' arguments, as their entry points set them
    KltArgs& K = t->K;
    K.n_pairs = n_streams; K.rows = rows; K.cols = cols; K.win = o.win; K.max_count = o.max_count; K.flags = o.flow_back ? 5 : 1;
    K.eps2 = o.eps * o.eps; K.min_eig = o.min_eig; K.back_dist = o.back_dist;
    K.lw[0] = cols; K.lh[0] = rows;
    for (int l = 1; l <= KLT_LMAX; l++) { K.lw[l] = (K.lw[l - 1] + 1) / 2; K.lh[l] = (K.lh[l - 1] + 1) / 2; }
    int avail = 0;
    while (avail < KLT_LMAX && K.lw[avail + 1] > o.win && K.lh[avail + 1] > o.win) avail++;
    const int build = std::max(o.max_level, o.back_level);
    K.top_build = std::min(build, avail); K.top_f = std::min(o.max_level, avail); K.top_b = std::min(o.back_level, avail);
    size_t loff = 0;
    for (int l = 1; l <= KLT_LMAX; l++) { K.loff[l] = loff; loff += (size_t)K.lw[l] * (size_t)K.lh[l]; }
    K.half_bytes = swf_klt_pyramid_bytes(rows, cols, build) / 2;
    K.blocks_per_pair = std::max(1, std::min((o.max_cnt + KLT_WAVES - 1) / KLT_WAVES, (int)KLT_BLOCKS_DEVICE));
    TrkArgs& R = t->R;
    R.n_pairs = n_streams;
    for (int k = 0; k < 12; k++) R.cam[k] = cam[k];
    R.focal = o.focal; R.half_col = (double)(o.virt_col ? o.virt_col : cols) / 2.0; R.half_row = (double)(o.virt_row ? o.virt_row : rows) / 2.0;
    R.iterations = o.f_iterations; R.flags = 1; R.thr2 = o.f_threshold * o.f_threshold; R.confidence = o.f_confidence;
    GfttArgs& G = t->G;
    G.n_frames = n_streams; G.rows = rows; G.cols = cols; G.max_cnt = o.max_cnt; G.r = o.min_dist; G.cand_cap = o.cand_cap; G.flags = 1; G.quality = o.quality;
    G.L = gftt_layout(rows, cols, o.cand_cap);
    for (int d = 0; d <= o.min_dist; d++) {                // floor(sqrt(r^2 - d^2)) in integers
        int h = 0;
        while ((h + 1) * (h + 1) <= o.min_dist * o.min_dist - d * d) h++;
        G.hw[d] = (short)h;
    }

    // ---- every buffer the tracker ever needs; the state, the counts and the ids start at 0
    TrackerArgs& P = t->P;
    P.n_streams = n_streams; P.max_cnt = o.max_cnt; P.L = G.L;
    for (int k = 0; k < 12; k++) P.cam[k] = cam[k];
    unsigned char* st1 = nullptr;
    bool ok = tracker_alloc(t, t->img[0], ns * img_bytes, false) && tracker_alloc(t, t->img[1], ns * img_bytes, false) &&
              tracker_alloc(t, t->mask, ns * img_bytes, false) && tracker_alloc(t, t->pyr, ns * 2 * K.half_bytes, false) &&
              tracker_alloc(t, t->work, ns * G.L.bytes, true) && tracker_alloc(t, t->dt, ns, true) &&
              tracker_alloc(t, t->obs[0], T * 7, true) && tracker_alloc(t, t->obs[1], T * 7, true) &&
              tracker_alloc(t, t->rm_first, ns + 1, true) && tracker_alloc(t, t->rm_ids, T, true) && tracker_alloc(t, st1, T, true);
    for (int k = 0; k < 2 && ok; k++)
        ok = tracker_alloc(t, t->S[k].first, ns + 1, true) && tracker_alloc(t, t->S[k].px, T * 2, true) && tracker_alloc(t, t->S[k].ids, T, true) &&
             tracker_alloc(t, t->S[k].tc, T, true) && tracker_alloc(t, t->S[k].lin, T, true);
    ok = ok && tracker_alloc(t, P.n_id, ns, true) && tracker_alloc(t, P.cur1, T * 2, true) && tracker_alloc(t, P.k1, T, true) &&
         tracker_alloc(t, P.nk1, ns, true) && tracker_alloc(t, P.kinfo, ns, true) &&
         tracker_alloc(t, P.first1, ns + 1, true) && tracker_alloc(t, P.pxp1, T * 2, true) && tracker_alloc(t, P.pxc1, T * 2, true) &&
         tracker_alloc(t, P.ids1, T, true) && tracker_alloc(t, P.tc1, T, true) && tracker_alloc(t, P.lin1, T, true) &&
         tracker_alloc(t, P.k2, T, true) && tracker_alloc(t, P.ni2, ns, true) && tracker_alloc(t, P.tinfo, ns, true) &&
         tracker_alloc(t, P.first2, ns + 1, true) && tracker_alloc(t, P.px2, T * 2, true) && tracker_alloc(t, P.ids2, T, true) &&
         tracker_alloc(t, P.tc2, T, true) && tracker_alloc(t, P.lin2, T, true) &&
         tracker_alloc(t, P.pf3, ns + 1, true) && tracker_alloc(t, P.ppx3, T * 2, true) && tracker_alloc(t, P.psrc3, T, true) &&
         tracker_alloc(t, P.nold3, ns, true) && tracker_alloc(t, P.nnew3, ns, true) && tracker_alloc(t, P.ncand3, ns, true) &&
         tracker_alloc(t, P.ginfo, ns, true) &&
         tracker_alloc(t, P.ffirst, ns + 1, true) && tracker_alloc(t, P.fids, T, true) && tracker_alloc(t, P.ftc, T, true) &&
         tracker_alloc(t, P.fpx, T * 2, true) && tracker_alloc(t, P.counts, ns * SWF_TRACKER_NCOUNT, true) && tracker_alloc(t, P.info, ns, true) &&
         tracker_alloc(t, P.krm, T, true) && tracker_alloc(t, P.nkrm, ns, true);
    if (!ok) {
        const std::string m = hipGetErrorString(hipGetLastError());
        tracker_free(t);
        return tracker_fail(SWF_E_NODEVICE, who + ": allocating the tracker: " + m);
    }
    P.dt = t->dt; P.work = t->work; P.rm_first = t->rm_first; P.rm_ids = t->rm_ids;
    K.cur_px = P.cur1; K.status = st1; K.keep_idx = P.k1; K.n_keep = P.nk1; K.info = P.kinfo; K.pyr = t->pyr;
    R.first = P.first1; R.cur_px = P.pxc1; R.prev_px = P.pxp1; R.dt = t->dt; R.keep_idx = P.k2; R.n_inliers = P.ni2; R.info = P.tinfo;
    G.first = P.first2; G.px = P.px2; G.track_cnt = P.tc2; G.n_old = P.nold3; G.n_new = P.nnew3; G.n_cand = P.ncand3;
    G.pack_first = P.pf3; G.pack_px = P.ppx3; G.pack_src = P.psrc3; G.info = P.ginfo; G.work = t->work;
    *out = t;
    return SWF_OK;
}

extern "C" int swf_tracker_track(swf_tracker* t, const double* times, const uint8_t* img, const uint8_t* mask, uint64_t seed, int32_t img_on_device) {
    const std::string who = "swf_tracker_track";
    if (!t || !times || !img) return tracker_fail(SWF_E_INVALID, who + ": null argument");
    const size_t ns = (size_t)t->n_streams, img_bytes = ns * (size_t)t->rows * (size_t)t->cols;
    for (size_t s = 0; s < ns; s++) {
        if (!std::isfinite(times[s])) return tracker_fail(SWF_E_INVALID, who + ": a non-finite time");
        if (t->frames > 0 && !(times[s] > t->prev_time[s])) return tracker_fail(SWF_E_INVALID, who + ": a stream's time must lie above its previous one");
        if (t->frames > 0 && !std::isfinite(times[s] - t->prev_time[s])) return tracker_fail(SWF_E_INVALID, who + ": a time difference that is not finite");
    }
    // ---- from here on everything is enqueued on the tracker's stream: no synchronisation, no allocation, nothing copied from the device
    for (size_t s = 0; s < ns; s++) t->h_dt[s] = t->frames > 0 ? times[s] - t->prev_time[s] : 1.0;   // a first frame has no points: dt is not used
    const int cur = (int)(t->frames & 1);
    const hipMemcpyKind kind = img_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipError_t e = hipMemcpyAsync(t->img[cur], img, img_bytes, kind, t->st);
    if (e == hipSuccess && mask) e = hipMemcpyAsync(t->mask, mask, img_bytes, kind, t->st);
    if (e == hipSuccess) e = hipMemcpyAsync(t->dt, t->h_dt.data(), ns * sizeof(double), hipMemcpyHostToDevice, t->st);
    if (e != hipSuccess) return tracker_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
    TrackerArgs P = t->P;
    P.S = t->S[t->set]; P.D = t->S[1 - t->set];
    P.have_klt = t->frames > 0 ? 1 : 0;
    P.obs = t->obs[cur]; P.obs_prev = t->obs[1 - cur];
    const dim3 grid((unsigned)ns), block(TRACKER_THREADS);
    if (P.have_klt) {
        KltArgs K = t->K;
        K.prev_img = t->img[1 - cur]; K.cur_img = t->img[cur]; K.first = P.S.first; K.prev_px = P.S.px;
        const int rc = swf_internal_klt_launch(K, t->st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_tracker_after_klt, grid, block, 0, t->st, P);
    if (!tracker_launched("k_tracker_after_klt")) return SWF_E_NODEVICE;
    TrkArgs R = t->R;
    R.seed = seed;
    int rc = swf_internal_trk_launch(R, t->st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tracker_after_f, grid, block, 0, t->st, P);
    if (!tracker_launched("k_tracker_after_f")) return SWF_E_NODEVICE;
    GfttArgs G = t->G;
    G.img = t->img[cur]; G.mask = mask ? t->mask : nullptr;
    rc = swf_internal_gftt_launch(G, t->st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tracker_finish, grid, block, 0, t->st, P);
    if (!tracker_launched("k_tracker_finish")) return SWF_E_NODEVICE;
    for (size_t s = 0; s < ns; s++) t->prev_time[s] = times[s];
    t->frames++;
    return SWF_OK;
}

extern "C" int swf_tracker_remove_ids(swf_tracker* t, const int32_t* first, const int32_t* ids) {
    const std::string who = "swf_tracker_remove_ids";
    if (!t || !first || !ids) return tracker_fail(SWF_E_INVALID, who + ": null argument");
    const size_t ns = (size_t)t->n_streams;
    if (first[0] < 0) return tracker_fail(SWF_E_INVALID, who + ": a negative offset");
    for (size_t s = 0; s < ns; s++) {
        if (first[s + 1] < first[s]) return tracker_fail(SWF_E_INVALID, who + ": offsets must be non-decreasing");
        if (first[s + 1] - first[s] > t->opt.max_cnt) return tracker_fail(SWF_E_UNSUPPORTED, who + ": more than max_cnt ids for a stream");
    }
    std::vector<int32_t> rel(first, first + ns + 1);
    for (auto& v : rel) v -= first[0];
    const size_t tot = (size_t)rel[ns];
    hipError_t e = hipMemcpyAsync(t->rm_first, rel.data(), (ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, t->st);
    if (e == hipSuccess && tot) e = hipMemcpyAsync(t->rm_ids, ids + first[0], tot * sizeof(int32_t), hipMemcpyHostToDevice, t->st);
    if (e != hipSuccess) return tracker_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
    TrackerArgs P = t->P;
    P.S = t->S[t->set]; P.D = t->S[1 - t->set];
    const dim3 grid((unsigned)ns), block(TRACKER_THREADS);
    hipLaunchKernelGGL(k_tracker_mark, grid, block, 0, t->st, P);
    if (!tracker_launched("k_tracker_mark")) return SWF_E_NODEVICE;
    hipLaunchKernelGGL(k_tracker_gather, grid, block, 0, t->st, P);
    if (!tracker_launched("k_tracker_gather")) return SWF_E_NODEVICE;
    t->set = 1 - t->set;
    return SWF_OK;
}

extern "C" int swf_tracker_download(swf_tracker* t, int32_t* n, int32_t* ids, int32_t* track_cnt, double* obs, int32_t* counts, int32_t* info) {
    const std::string who = "swf_tracker_download";
    if (!t) return tracker_fail(SWF_E_INVALID, who + ": null argument");
    if (t->frames == 0) return tracker_fail(SWF_E_STATE, who + ": no frame has been tracked");
    const size_t ns = (size_t)t->n_streams;
    std::vector<int32_t> first(ns + 1);
    hipError_t e = hipMemcpyAsync(first.data(), t->P.ffirst, (ns + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, t->st);
    if (e == hipSuccess) e = hipStreamSynchronize(t->st);
    if (e != hipSuccess) return tracker_fail(SWF_E_NODEVICE, who + ": " + hipGetErrorString(e));
    const size_t tot = (size_t)std::max(first[ns], 0);
    if (first[0] != 0 || tot > ns * (size_t)t->opt.max_cnt) return tracker_fail(SWF_E_STATE, who + ": the frame's offsets are out of range");
    const double* d_obs = t->obs[(t->frames - 1) & 1];
    if (n) for (size_t s = 0; s < ns; s++) n[s] = first[s + 1] - first[s];
    if (e == hipSuccess && ids && tot) e = hipMemcpy(ids, t->P.fids, tot * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && track_cnt && tot) e = hipMemcpy(track_cnt, t->P.ftc, tot * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && obs && tot) e = hipMemcpy(obs, d_obs, tot * 7 * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && counts) e = hipMemcpy(counts, t->P.counts, ns * SWF_TRACKER_NCOUNT * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && info) e = hipMemcpy(info, t->P.info, ns * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tracker_fail(SWF_E_NODEVICE, who + ": hipMemcpy: " + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_tracker_device_frame(swf_tracker* t, const int32_t** first, const int32_t** ids, const int32_t** track_cnt,
                                        const double** px, const double** obs) {
    if (!t) return tracker_fail(SWF_E_INVALID, "swf_tracker_device_frame: null argument");
    if (t->frames == 0) return tracker_fail(SWF_E_STATE, "swf_tracker_device_frame: no frame has been tracked");
    if (first) *first = t->P.ffirst;
    if (ids) *ids = t->P.fids;
    if (track_cnt) *track_cnt = t->P.ftc;
    if (px) *px = t->P.fpx;
    if (obs) *obs = t->obs[(t->frames - 1) & 1];
    return SWF_OK;
}

extern "C" int swf_tracker_sync(swf_tracker* t) {
    if (!t) return tracker_fail(SWF_E_INVALID, "swf_tracker_sync: null argument");
    const hipError_t e = hipStreamSynchronize(t->st);
    if (e != hipSuccess) return tracker_fail(SWF_E_NODEVICE, std::string("swf_tracker_sync: ") + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_tracker_destroy(swf_tracker* t) {
    if (!t) return SWF_OK;
    (void)hipStreamSynchronize(t->st);
    tracker_free(t);
    return SWF_OK;
}
