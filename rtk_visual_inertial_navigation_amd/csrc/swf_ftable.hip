// swf_ftable.hip — the kernels of the resident feature table (see swf_ftable.h) and the C-ABI swf_ftable_*.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_ftable.h"

void swf_internal_set_error(const std::string& m);
static int ftable_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

__device__ __forceinline__ int ft_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the sum of cnt(g) over the streams g < s in front of this workgroup's; every thread calls it, once per kernel
template <class F> __device__ __forceinline__ int ft_offset(int s, F cnt) {
    __shared__ int s_sum[FTABLE_THREADS / 64];
    const int tid = threadIdx.x;
    int part = 0;
    for (int g = tid; g < s; g += FTABLE_THREADS) part += cnt(g);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    return s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// the exclusive prefix of v over the workgroup's 256 threads in thread order, and the total; every thread calls it
__device__ __forceinline__ int ft_scan(int v, int& total) {
    __shared__ int s_wave[FTABLE_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    __syncthreads();                                        // the previous call's readers are done with s_wave
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FTABLE_THREADS / 64; w++) { before += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
    total = all;
    return before + inc - v;
}

// the workgroup's stable compaction by ballots: the position of a kept thread among the kept, and their number
__device__ __forceinline__ int ft_compact(bool keep, int& total) {
    __shared__ int s_cnt[FTABLE_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    __syncthreads();
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FTABLE_THREADS / 64; w++) { before += w < wave ? s_cnt[w] : 0; all += s_cnt[w]; }
    total = all;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

struct FtStream { int s, n_frames, n_feat; size_t base; };

__device__ __forceinline__ FtStream ft_stream(const FtableArgs& P) {
    FtStream T;
    T.s = blockIdx.x;
    T.n_frames = ft_clamp(P.S.n_frames[T.s], 0, P.window);
    T.n_feat = ft_clamp(P.S.n_feat[T.s], 0, P.feat_cap);
    T.base = (size_t)T.s * (size_t)P.feat_cap;
    return T;
}

// feature `from` of S becomes feature `to` of D without the observation `skip` (-1: all stay); in_problem is cleared when asked
__device__ __forceinline__ void ft_move(const FtableArgs& P, size_t from, size_t to, int n_obs, int skip, int start, bool clear) {
    P.D.id[to] = P.S.id[from]; P.D.start[to] = start; P.D.valid[to] = P.S.valid[from]; P.D.flag[to] = P.S.flag[from];
    P.D.idepth[to] = P.S.idepth[from];
    for (int k = 0; k < 3; k++) P.D.world[3 * to + k] = P.S.world[3 * from + k];
    int at = 0;
    for (int k = 0; k < n_obs; k++) {
        if (k == skip) continue;
        const size_t a = from * (size_t)P.window + k, b = to * (size_t)P.window + at;
        for (int c = 0; c < 7; c++) P.D.obs[7 * b + c] = P.S.obs[7 * a + c];
        P.D.in_problem[b] = clear ? 0 : P.S.in_problem[a];
        at++;
    }
    P.D.n_obs[to] = at;
}

// z of ric^T (R^T (w - Pp) + pbg - tic); the operation order is the header's
__device__ __forceinline__ double ft_depth_z(const FtableArgs& P, const double* w, const double* Pp, const double* R) {
#pragma clang fp contract(off)
    const double d0 = w[0] - Pp[0], d1 = w[1] - Pp[1], d2 = w[2] - Pp[2];
    double b[3];
    for (int r = 0; r < 3; r++) {
        const double a = (R[r] * d0 + R[3 + r] * d1) + R[6 + r] * d2;
        b[r] = (a + P.pbg[r]) - P.tic[r];
    }
    return (P.ric[2] * b[0] + P.ric[5] * b[1]) + P.ric[8] * b[2];
}

__device__ __forceinline__ double ft_inverse(double z) {
#pragma clang fp contract(off)
    return 1.0 / z;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// addFeatureCheckParallax + removeOut
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_add(FtableArgs P) {
    __shared__ int s_raw[FTABLE_FRAME_MAX], s_id[FTABLE_FRAME_MAX], s_src[FTABLE_FRAME_MAX], s_hit[FTABLE_FRAME_MAX];
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, nf = T.n_frames, n0 = T.n_feat;
    const int p0 = P.f_first[s], n_in = P.f_first[s + 1] - p0;
    bool bad = p0 < 0 || n_in < 0 || n_in > P.frame_cap || n_in > FTABLE_FRAME_MAX;        // uniform
    const int nn = bad ? 0 : n_in;
    bool mine = false;
    for (int i = tid; i < nn; i += FTABLE_THREADS) {
        s_raw[i] = P.f_ids[(size_t)p0 + i];
        s_hit[i] = 0;
        const double* o = P.f_obs + 7 * ((size_t)p0 + i);
        for (int c = 0; c < 7; c++) mine = mine || !isfinite(o[c]);
    }
    __syncthreads();
    for (int i = tid; i < nn; i += FTABLE_THREADS) {         // rank sort by (id, index): at most frame_cap^2 / 256 compares a thread
        const int id = s_raw[i];
        int r = 0;
        for (int j = 0; j < nn; j++) {
            const int o = s_raw[j];
            r += (o < id || (o == id && j < i)) ? 1 : 0;
            mine = mine || (o == id && j != i);
        }
        s_id[r] = id; s_src[r] = i;
    }
    bad = __syncthreads_or(mine ? 1 : 0) != 0 || bad;
    const bool full = nf >= P.window;
    const bool act = !bad && !full;
    const int image_index = nf;
    int kept = 0, last = 0, lng = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {        // uniform: n0 is the workgroup's
        const int i = c0 + tid;
        const size_t from = T.base + (size_t)min(i, n0 - 1);
        bool live = i < n0, found = false;
        int pos = 0, n_obs = 0, start = 0;
        if (live) {
            n_obs = ft_clamp(P.S.n_obs[from], 0, P.window); start = P.S.start[from];
            if (act) {
                const int id = P.S.id[from];
                int lo = 0, hi = nn;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_id[mid] < id) lo = mid + 1; else hi = mid; }
                // a feature that is full already (no valid state has one while n_frames < window) keeps its id out of the new ones
                if (lo < nn && s_id[lo] == id) { found = n_obs < P.window; pos = lo; s_hit[lo] = 1; }
            }
        }
        const int n2 = n_obs + (found ? 1 : 0);
        const bool keep = live && (!act || !(start + n2 - 1 != image_index && n2 < P.feature_continue));
        last += __syncthreads_count(found ? 1 : 0);
        lng += __syncthreads_count(found && n2 >= P.long_len ? 1 : 0);
        int tot;
        const int at = ft_compact(keep, tot);
        if (keep) {
            const size_t to = T.base + (size_t)(kept + at);
            ft_move(P, from, to, n_obs, -1, start, false);
            if (found) {
                const double* o = P.f_obs + 7 * ((size_t)p0 + s_src[pos]);
                const size_t b = to * (size_t)P.window + n_obs;
                for (int c = 0; c < 7; c++) P.D.obs[7 * b + c] = o[c];
                P.D.in_problem[b] = 0;
                P.D.n_obs[to] = n2;
            }
        }
        kept += tot;
    }
    __syncthreads();                                        // every hit is marked
    const int room = max(P.feat_cap - n0, 0);               // the j-th new id is taken while n0 + j < feat_cap
    int fresh = 0;
    for (int c0 = 0; c0 < nn; c0 += FTABLE_THREADS) {
        const int p = c0 + tid;
        const bool isnew = act && p < nn && !s_hit[p];
        int tot;
        const int j = fresh + ft_compact(isnew, tot);
        if (isnew && j < room) {
            const size_t to = T.base + (size_t)(kept + j);   // kept <= n0, so kept + j < feat_cap
            P.D.id[to] = s_id[p]; P.D.start[to] = image_index; P.D.n_obs[to] = 1; P.D.valid[to] = 0; P.D.flag[to] = 0;
            P.D.idepth[to] = 0.0;
            for (int k = 0; k < 3; k++) P.D.world[3 * to + k] = 0.0;
            const double* o = P.f_obs + 7 * ((size_t)p0 + s_src[p]);
            const size_t b = to * (size_t)P.window;
            for (int c = 0; c < 7; c++) P.D.obs[7 * b + c] = o[c];
            P.D.in_problem[b] = 0;
        }
        fresh += tot;
    }
    if (tid == 0) {
        const int taken = min(fresh, room);
        P.D.n_feat[s] = kept + taken; P.D.n_frames[s] = act ? nf + 1 : nf; P.D.n_listed[s] = P.S.n_listed[s];
        int* c = P.counts + (size_t)s * SWF_FTABLE_NCOUNT;
        bool key = false;
        if (act) {
#pragma clang fp contract(off)
            key = image_index < 2 || last < P.min_track || lng < P.min_long || (double)taken > P.new_ratio * (double)last;
        }
        c[SWF_FTABLE_C_KEYFRAME] = key ? 1 : 0; c[SWF_FTABLE_C_LAST_TRACK] = last; c[SWF_FTABLE_C_LONG_TRACK] = lng;
        c[SWF_FTABLE_C_NEW] = taken; c[SWF_FTABLE_C_ERASED] = n0 - kept;
        c[SWF_FTABLE_C_INFO] = (bad ? SWF_FTABLE_BAD_FRAME : 0) | (!bad && full ? SWF_FTABLE_WINDOW_FULL : 0) | (fresh > taken ? SWF_FTABLE_TABLE_FULL : 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the gather of initFramePoseByPnP: pass 0 counts, pass 1 packs
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_pnp(FtableArgs P) {
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, cnt_frame = T.n_frames - 1, n0 = T.n_frames < 2 ? 0 : T.n_feat;
    int off = 0;
    if (P.pass) off = ft_offset(s, [&](int g) { return ft_clamp(P.cnt_a[g], 0, P.feat_cap); });
    int got = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const int idx = cnt_frame - P.S.start[f], n_obs = ft_clamp(P.S.n_obs[f], 0, P.window);
        const bool take = i < n0 && P.S.valid[f] != 0 && idx >= 0 && n_obs >= idx + 1;
        int tot;
        const int at = ft_compact(take, tot);
        if (take && P.pass) {
            const size_t q = (size_t)off + got + at, a = f * (size_t)P.window + idx;
            for (int k = 0; k < 3; k++) P.pnp_w[3 * q + k] = P.S.world[3 * f + k];
            P.pnp_uv[2 * q] = P.S.obs[7 * a]; P.pnp_uv[2 * q + 1] = P.S.obs[7 * a + 1];
        }
        got += tot;
    }
    if (tid == 0) {
        if (!P.pass) P.cnt_a[s] = got;
        else {
            P.pnp_first[s] = off;
            if (s == P.n_streams - 1) P.pnp_first[s + 1] = off + got;
            P.counts[(size_t)s * SWF_FTABLE_NCOUNT + SWF_FTABLE_C_N_PNP] = got;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// triangulate: the inputs of swf_triangulate_batch for every slot, and its results back
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_tri_gather(FtableArgs P) {
    const FtStream T = ft_stream(P);
    for (int i = threadIdx.x; i < P.feat_cap; i += FTABLE_THREADS) {
        const size_t f = T.base + i;
        int st = -1;
        double a[4] = { 0.0, 0.0, 0.0, 0.0 };
        if (i < T.n_feat && P.S.valid[f] == 0 && P.S.n_obs[f] > 1) {
            const int start = P.S.start[f];
            if (start >= 0 && start + 1 < P.window) {
                st = T.s * P.window + start;
                const size_t o = f * (size_t)P.window;
                a[0] = P.S.obs[7 * o]; a[1] = P.S.obs[7 * o + 1]; a[2] = P.S.obs[7 * (o + 1)]; a[3] = P.S.obs[7 * (o + 1) + 1];
            }
        }
        P.tri_start[f] = st;
        P.tri_pt0[2 * f] = a[0]; P.tri_pt0[2 * f + 1] = a[1]; P.tri_pt1[2 * f] = a[2]; P.tri_pt1[2 * f + 1] = a[3];
    }
}

__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_tri_scatter(FtableArgs P) {
    const FtStream T = ft_stream(P);
    for (int i = threadIdx.x; i < T.n_feat; i += FTABLE_THREADS) {
        const size_t f = T.base + i;
        const double depth = P.tri_depth[f];
        if (P.tri_start[f] < 0 || depth == -1.0) continue;
        P.S.idepth[f] = ft_inverse(depth);
        for (int k = 0; k < 3; k++) P.S.world[3 * f + k] = P.tri_world[3 * f + k];
        P.S.valid[f] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// AddFeature2Problem as data: pass 0 counts landmarks and projections, pass 1 packs and sets in_problem
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_list(FtableArgs P) {
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, n0 = T.n_feat;
    int off_lm = 0, off_pr = 0;
    if (P.pass) {
        off_lm = ft_offset(s, [&](int g) { return ft_clamp(P.cnt_a[g], 0, P.feat_cap); });
        __syncthreads();                                    // ft_offset's LDS words are read before they are written again
        off_pr = ft_offset(s, [&](int g) { return ft_clamp(P.cnt_b[g], 0, P.feat_cap * P.window); });
    }
    int n_lm = 0, n_pr = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const int n_obs = ft_clamp(P.S.n_obs[f], 0, P.window);
        const bool take = i < n0 && n_obs >= P.feature_continue;
        int tot_lm, tot_pr;
        const int at = ft_compact(take, tot_lm);
        const int pr = ft_scan(take ? n_obs : 0, tot_pr);
        if (take && P.pass) {
            const size_t q = (size_t)off_lm + n_lm + at;
            const int start = P.S.start[f];
            P.lm_id[q] = P.S.id[f]; P.lm_start[q] = start; P.lm_nobs[q] = n_obs; P.lm_valid[q] = P.S.valid[f];
            for (int k = 0; k < 3; k++) P.lm_world[3 * q + k] = P.S.world[3 * f + k];
            for (int k = 0; k < n_obs; k++) {
                const size_t a = f * (size_t)P.window + k, r = (size_t)off_pr + n_pr + pr + k;
                P.proj_frame[r] = start + k; P.proj_lm[r] = n_lm + at;
                P.proj_uv[2 * r] = P.S.obs[7 * a]; P.proj_uv[2 * r + 1] = P.S.obs[7 * a + 1];
                P.proj_new[r] = P.S.in_problem[a] ? 0 : 1;
                P.S.in_problem[a] = 1;
            }
        }
        n_lm += tot_lm; n_pr += tot_pr;
    }
    if (tid == 0) {
        if (!P.pass) { P.cnt_a[s] = n_lm; P.cnt_b[s] = n_pr; }
        else {
            P.lm_first[s] = off_lm; P.proj_first[s] = off_pr;
            if (s == P.n_streams - 1) { P.lm_first[s + 1] = off_lm + n_lm; P.proj_first[s + 1] = off_pr + n_pr; }
            P.S.n_listed[s] = n_lm;
            int* c = P.counts + (size_t)s * SWF_FTABLE_NCOUNT;
            c[SWF_FTABLE_C_N_LISTED] = n_lm; c[SWF_FTABLE_C_N_PROJ] = n_pr;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the landmark tail of Double2Vector and the verdict of OutliersRejection, in place
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_set_solved(FtableArgs P) {
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, n0 = T.n_feat;
    const int q0 = P.in_first[s], n_in = P.in_first[s + 1] - q0;
    int mine = 0;
    for (int i = tid; i < n0; i += FTABLE_THREADS) mine += ft_clamp(P.S.n_obs[T.base + i], 0, P.window) >= P.feature_continue ? 1 : 0;
    int n_now;
    (void)ft_scan(mine, n_now);
    const bool stale = q0 < 0 || n_now != n_in || n_now != P.S.n_listed[s];
    if (tid == 0) P.counts[(size_t)s * SWF_FTABLE_NCOUNT + SWF_FTABLE_C_INFO] = stale ? SWF_FTABLE_STALE_LIST : 0;
    if (stale) return;                                      // uniform
    int seen = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const bool take = i < n0 && ft_clamp(P.S.n_obs[f], 0, P.window) >= P.feature_continue;
        int tot;
        const int at = ft_compact(take, tot);
        if (take) {
            const size_t q = (size_t)q0 + seen + at;
            double w[3];
            for (int k = 0; k < 3; k++) { w[k] = P.in_world[3 * q + k]; P.S.world[3 * f + k] = w[k]; }
            const size_t pose = (size_t)s * P.window + ft_clamp(P.S.start[f], 0, P.window - 1);
            const double idepth = ft_inverse(ft_depth_z(P, w, P.Ps + 3 * pose, P.Rs + 9 * pose));
            P.S.idepth[f] = idepth;
            int flag = idepth < 0.0 ? 2 : 1;
            if (P.in_flags && (P.in_flags[q] & (SWF_FEAT_OUTLIER | SWF_FEAT_NEG_DEPTH))) flag = 2;
            P.S.flag[f] = flag;
        }
        seen += tot;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// removeFailures: pass 0 counts the erased, pass 1 gathers the survivors into D and packs the erased ids
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_remove(FtableArgs P) {
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, n0 = T.n_feat;
    int off = 0;
    if (P.pass) off = ft_offset(s, [&](int g) { return ft_clamp(P.cnt_a[g], 0, P.feat_cap); });
    int kept = 0, gone = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const bool live = i < n0, out = live && P.S.flag[f] == 2;
        int tot_k, tot_g;
        const int at_k = ft_compact(live && !out, tot_k);
        const int at_g = ft_compact(out, tot_g);
        if (P.pass) {
            if (live && !out) ft_move(P, f, T.base + (size_t)(kept + at_k), ft_clamp(P.S.n_obs[f], 0, P.window), -1, P.S.start[f], false);
            if (out) P.rm_ids[(size_t)off + gone + at_g] = P.S.id[f];
        }
        kept += tot_k; gone += tot_g;
    }
    if (tid == 0) {
        if (!P.pass) P.cnt_a[s] = gone;
        else {
            P.rm_first[s] = off;
            if (s == P.n_streams - 1) P.rm_first[s + 1] = off + gone;
            P.D.n_feat[s] = kept; P.D.n_frames[s] = P.S.n_frames[s]; P.D.n_listed[s] = P.S.n_listed[s];
            P.counts[(size_t)s * SWF_FTABLE_NCOUNT + SWF_FTABLE_C_ERASED] = gone;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// CheckParallax(n_frames - 1): the terms in parallel, compacted in list order; one lane sums them in that order
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_parallax(FtableArgs P) {
#pragma clang fp contract(off)
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, n0 = T.n_feat, idx = T.n_frames - 1;
    int num = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const int start = P.S.start[f], n_obs = ft_clamp(P.S.n_obs[f], 0, P.window);
        const bool take = i < n0 && start >= 0 && start <= idx - 2 && start + n_obs - 1 >= idx - 1;
        int tot;
        const int at = ft_compact(take, tot);
        if (take) {
            const double* oi = P.S.obs + 7 * (f * (size_t)P.window + (idx - 2 - start));
            const double* oj = oi + 7;
            const double u = oi[0] / oi[2], v = oi[1] / oi[2];
            const double du = u - oj[0], dv = v - oj[1];
            P.terms[T.base + num + at] = __dsqrt_rn(du * du + dv * dv);
        }
        num += tot;
    }
    __syncthreads();                                        // the terms are the workgroup's own writes
    if (tid == 0) {
        double sum = 0.0;
        for (int k = 0; k < num; k++) sum = sum + P.terms[T.base + k];
        int* c = P.counts + (size_t)s * SWF_FTABLE_NCOUNT;
        c[SWF_FTABLE_C_PARALLAX_NUM] = num;
        if (num == 0) { c[SWF_FTABLE_C_KEYFRAME] = 1; P.parallax[s] = 0.0; }
        else {
            const double mean = sum / (double)num;
            P.parallax[s] = mean * P.focal;
            c[SWF_FTABLE_C_KEYFRAME] = mean >= P.min_parallax ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// removeBack (mode 1) / removeFront (mode 2), n_frames -= 1 and removeOut2's world-point effect, gathered into D
__global__ void __launch_bounds__(FTABLE_THREADS) k_ftable_slide(FtableArgs P) {
    const FtStream T = ft_stream(P);
    const int s = T.s, tid = threadIdx.x, n0 = T.n_feat, nf = T.n_frames, asked = P.mode[s];
    const bool bad = asked < 0 || asked > 2 || (asked != 0 && nf < 2);
    const int mode = bad ? 0 : asked, front = nf - 1;
    int kept = 0;
    for (int c0 = 0; c0 < n0; c0 += FTABLE_THREADS) {
        const int i = c0 + tid;
        const size_t f = T.base + (size_t)min(i, n0 - 1);
        const bool live = i < n0;
        int start = P.S.start[f], skip = -1;
        const int n_obs = ft_clamp(P.S.n_obs[f], 0, P.window);
        double idepth = P.S.idepth[f];
        if (live && mode == 1) {
            if (start != 0) start--;
            else {
                const double w[3] = { P.S.world[3 * f], P.S.world[3 * f + 1], P.S.world[3 * f + 2] };
                idepth = ft_inverse(ft_depth_z(P, w, P.P1 + 3 * (size_t)s, P.R1 + 9 * (size_t)s));
                skip = 0;
            }
        } else if (live && mode == 2) {
            if (start == front) start--;
            else if (start + n_obs - 1 >= front - 1) skip = front - 1 - start;
        }
        const int left = n_obs - (skip >= 0 && skip < n_obs ? 1 : 0);
        const bool keep = live && left > 0;
        int tot;
        const int at = ft_compact(keep, tot);
        if (keep) {
            const size_t to = T.base + (size_t)(kept + at);
            ft_move(P, f, to, n_obs, skip, start, mode != 0 && left < P.feature_continue);
            P.D.idepth[to] = idepth;
        }
        kept += tot;
    }
    if (tid == 0) {
        P.D.n_feat[s] = kept; P.D.n_frames[s] = mode ? nf - 1 : nf; P.D.n_listed[s] = P.S.n_listed[s];
        int* c = P.counts + (size_t)s * SWF_FTABLE_NCOUNT;
        c[SWF_FTABLE_C_ERASED] = n0 - kept; c[SWF_FTABLE_C_INFO] = bad ? SWF_FTABLE_BAD_SLIDE : 0;
    }
}

}  // namespace

struct swf_ftable {
    int n_streams = 0;
    swf_ftable_options opt{};
    hipStream_t st = nullptr;
    int set = 0;                                            // the state set in use
    std::vector<void*> bufs;
    FtableState S[2]{};
    FtableArgs P{};                                         // every pointer that does not change from call to call
    int* h_first = nullptr; int* h_ids = nullptr; double* h_obs = nullptr;   // device staging of a host-memory frame
    double* d_Ps = nullptr; double* d_Rs = nullptr; double* d_P1 = nullptr; double* d_R1 = nullptr;
    int* d_mode = nullptr; int* d_in_first = nullptr; double* d_in_world = nullptr; unsigned char* d_in_flags = nullptr;
    std::vector<int32_t> rel; std::vector<int32_t> pack_ids; std::vector<double> pack_obs;
    bool removed = false;                                   // a remove_failures has been enqueued
};

namespace {

template <class T> bool ftable_alloc(swf_ftable* t, T*& p, size_t n) {
    void* d = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 8);
    if (hipMalloc(&d, bytes) != hipSuccess) return false;
    t->bufs.push_back(d);
    p = (T*)d;
    return hipMemsetAsync(d, 0, bytes, t->st) == hipSuccess;
}

void ftable_free(swf_ftable* t) {
    for (void* p : t->bufs) (void)hipFree(p);
    delete t;
}

bool ftable_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return true;
    swf_internal_set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

FtableArgs ftable_args(swf_ftable* t) {
    FtableArgs P = t->P;
    P.S = t->S[t->set]; P.D = t->S[1 - t->set];
    return P;
}

bool ftable_finite(const double* v, int n) {
    for (int k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
    return true;
}

void ftable_extrinsics(FtableArgs& P, const double* tic, const double* ric, const double* pbg) {
    for (int k = 0; k < 3; k++) { P.tic[k] = tic[k]; P.pbg[k] = pbg[k]; }
    for (int k = 0; k < 9; k++) P.ric[k] = ric[k];
}

// a host array onto the table's device staging, or the caller's device array as it is
template <class T> const T* ftable_in(swf_ftable* t, const T* src, T* staging, size_t n, int on_device, hipError_t& e) {
    if (on_device) return src;
    if (e == hipSuccess && n) e = hipMemcpyAsync(staging, src, n * sizeof(T), hipMemcpyHostToDevice, t->st);
    return staging;
}

#define FTABLE_LAUNCH(kernel, P) \
    hipLaunchKernelGGL(kernel, dim3((unsigned)t->n_streams), dim3(FTABLE_THREADS), 0, t->st, P); \
    if (!ftable_launched(#kernel)) return SWF_E_NODEVICE

}  // namespace

// C-ABI, include/swf_solver.h
extern "C" void swf_ftable_default_options(swf_ftable_options* o) {
    if (!o) return;
    *o = swf_ftable_options{};
    o->window = 11; o->feat_cap = 4096; o->frame_cap = 350;
    o->feature_continue = 2; o->min_track = 20; o->min_long = 40; o->long_len = 4;
    o->new_ratio = 0.5; o->min_parallax = 10.0 / 1000.0; o->focal = 1000.0; o->init_depth = 5.0;
}

extern "C" int swf_ftable_create(int32_t n_streams, const swf_ftable_options* opt, void* stream, swf_ftable** out) {
    const std::string who = "swf_ftable_create";
    if (out) *out = nullptr;
    if (!opt || !out) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    const swf_ftable_options& o = *opt;
    if (!std::isfinite(o.new_ratio) || !std::isfinite(o.min_parallax) || !std::isfinite(o.focal) || !std::isfinite(o.init_depth))
        return ftable_fail(SWF_E_INVALID, who + ": new_ratio, min_parallax, focal and init_depth must be finite");
    if (n_streams < 1 || n_streams > 65535) return ftable_fail(SWF_E_UNSUPPORTED, who + ": n_streams outside 1 .. 65535");
    if (o.window < 3 || o.window > 32) return ftable_fail(SWF_E_UNSUPPORTED, who + ": window outside 3 .. 32");
    if (o.feat_cap < 1 || o.feat_cap > 65536) return ftable_fail(SWF_E_UNSUPPORTED, who + ": feat_cap outside 1 .. 65536");
    if (o.frame_cap < 1 || o.frame_cap > SWF_PNP_NMAX) return ftable_fail(SWF_E_UNSUPPORTED, who + ": frame_cap outside 1 .. 1024");
    if (o.feature_continue < 2 || o.feature_continue > o.window)
        return ftable_fail(SWF_E_UNSUPPORTED, who + ": feature_continue outside 2 .. window (the N-view triangulation is not covered)");
    const size_t ns = (size_t)n_streams, F = ns * (size_t)o.feat_cap, O = F * (size_t)o.window, fr = ns * ((size_t)o.frame_cap + 1);
    if (O > (size_t)0x7fffffff) return ftable_fail(SWF_E_UNSUPPORTED, who + ": n_streams * feat_cap * window above 2^31 - 1 (the packed offsets are int32)");

    swf_ftable* t = new swf_ftable;
    t->n_streams = n_streams; t->opt = o; t->st = (hipStream_t)stream;
    FtableArgs& P = t->P;
    P.n_streams = n_streams; P.window = o.window; P.feat_cap = o.feat_cap; P.frame_cap = o.frame_cap; P.feature_continue = o.feature_continue;
    P.min_track = o.min_track; P.min_long = o.min_long; P.long_len = o.long_len;
    P.new_ratio = o.new_ratio; P.min_parallax = o.min_parallax; P.focal = o.focal;
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        FtableState& S = t->S[k];
        ok = ftable_alloc(t, S.n_frames, ns) && ftable_alloc(t, S.n_feat, ns) && ftable_alloc(t, S.n_listed, ns) &&
             ftable_alloc(t, S.id, F) && ftable_alloc(t, S.start, F) && ftable_alloc(t, S.n_obs, F) && ftable_alloc(t, S.valid, F) &&
             ftable_alloc(t, S.flag, F) && ftable_alloc(t, S.idepth, F) && ftable_alloc(t, S.world, F * 3) &&
             ftable_alloc(t, S.obs, O * 7) && ftable_alloc(t, S.in_problem, O);
    }
    ok = ok && ftable_alloc(t, P.counts, ns * SWF_FTABLE_NCOUNT) && ftable_alloc(t, P.parallax, ns) &&
         ftable_alloc(t, P.cnt_a, ns) && ftable_alloc(t, P.cnt_b, ns) &&
         ftable_alloc(t, P.pnp_first, ns + 1) && ftable_alloc(t, P.pnp_w, F * 3) && ftable_alloc(t, P.pnp_uv, F * 2) &&
         ftable_alloc(t, P.tri_start, F) && ftable_alloc(t, P.tri_pt0, F * 2) && ftable_alloc(t, P.tri_pt1, F * 2) &&
         ftable_alloc(t, P.tri_depth, F) && ftable_alloc(t, P.tri_world, F * 3) &&
         ftable_alloc(t, P.lm_first, ns + 1) && ftable_alloc(t, P.proj_first, ns + 1) && ftable_alloc(t, P.lm_id, F) &&
         ftable_alloc(t, P.lm_world, F * 3) && ftable_alloc(t, P.lm_start, F) && ftable_alloc(t, P.lm_nobs, F) && ftable_alloc(t, P.lm_valid, F) &&
         ftable_alloc(t, P.proj_frame, O) && ftable_alloc(t, P.proj_lm, O) && ftable_alloc(t, P.proj_uv, O * 2) && ftable_alloc(t, P.proj_new, O) &&
         ftable_alloc(t, P.rm_first, ns + 1) && ftable_alloc(t, P.rm_ids, F) && ftable_alloc(t, P.terms, F) &&
         ftable_alloc(t, t->h_first, ns + 1) && ftable_alloc(t, t->h_ids, fr) && ftable_alloc(t, t->h_obs, fr * 7) &&
         ftable_alloc(t, t->d_Ps, ns * o.window * 3) && ftable_alloc(t, t->d_Rs, ns * o.window * 9) &&
         ftable_alloc(t, t->d_P1, ns * 3) && ftable_alloc(t, t->d_R1, ns * 9) && ftable_alloc(t, t->d_mode, ns) &&
         ftable_alloc(t, t->d_in_first, ns + 1) && ftable_alloc(t, t->d_in_world, F * 3) && ftable_alloc(t, t->d_in_flags, F);
    if (!ok) {
        const std::string m = hipGetErrorString(hipGetLastError());
        ftable_free(t);
        return ftable_fail(SWF_E_NODEVICE, who + ": allocating the table: " + m);
    }
    *out = t;
    return SWF_OK;
}

extern "C" int swf_ftable_add_frame(swf_ftable* t, const int32_t* first, const int32_t* ids, const double* obs, int32_t on_device) {
    const std::string who = "swf_ftable_add_frame";
    if (!t || !first || !ids || !obs) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    const size_t ns = (size_t)t->n_streams;
    FtableArgs P = ftable_args(t);
    if (on_device) { P.f_first = first; P.f_ids = ids; P.f_obs = obs; }
    else {
        if (first[0] < 0) return ftable_fail(SWF_E_INVALID, who + ": a negative offset");
        for (size_t s = 0; s < ns; s++) if (first[s + 1] < first[s]) return ftable_fail(SWF_E_INVALID, who + ": offsets must be non-decreasing");
        // a stream above frame_cap is staged with frame_cap + 1 points: enough for the kernel to call it a bad frame
        const int cap = t->opt.frame_cap + 1;
        t->rel.assign(ns + 1, 0);
        for (size_t s = 0; s < ns; s++) t->rel[s + 1] = t->rel[s] + std::min(first[s + 1] - first[s], cap);
        const size_t tot = (size_t)t->rel[ns];
        t->pack_ids.resize(tot + 1); t->pack_obs.resize((tot + 1) * 7);
        for (size_t s = 0; s < ns; s++) {
            const size_t m = (size_t)(t->rel[s + 1] - t->rel[s]);
            std::copy(ids + first[s], ids + first[s] + m, t->pack_ids.begin() + t->rel[s]);
            std::copy(obs + (size_t)first[s] * 7, obs + ((size_t)first[s] + m) * 7, t->pack_obs.begin() + (size_t)t->rel[s] * 7);
        }
        hipError_t e = hipMemcpyAsync(t->h_first, t->rel.data(), (ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, t->st);
        if (e == hipSuccess && tot) e = hipMemcpyAsync(t->h_ids, t->pack_ids.data(), tot * sizeof(int32_t), hipMemcpyHostToDevice, t->st);
        if (e == hipSuccess && tot) e = hipMemcpyAsync(t->h_obs, t->pack_obs.data(), tot * 7 * sizeof(double), hipMemcpyHostToDevice, t->st);
        if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
        P.f_first = t->h_first; P.f_ids = t->h_ids; P.f_obs = t->h_obs;
    }
    FTABLE_LAUNCH(k_ftable_add, P);
    t->set = 1 - t->set;
    return SWF_OK;
}

extern "C" int swf_ftable_pnp_points(swf_ftable* t, const int32_t** first_out, const double** pts_w, const double** pts_uv) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_pnp_points: null argument");
    FtableArgs P = ftable_args(t);
    P.pass = 0;
    FTABLE_LAUNCH(k_ftable_pnp, P);
    P.pass = 1;
    FTABLE_LAUNCH(k_ftable_pnp, P);
    if (first_out) *first_out = P.pnp_first;
    if (pts_w) *pts_w = P.pnp_w;
    if (pts_uv) *pts_uv = P.pnp_uv;
    return SWF_OK;
}

extern "C" int swf_ftable_triangulate(swf_ftable* t, const double* Ps, const double* Rs, const double tic[3], const double ric[9],
                                      const double pbg[3], int32_t on_device) {
    const std::string who = "swf_ftable_triangulate";
    if (!t || !Ps || !Rs || !tic || !ric || !pbg) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    if (!ftable_finite(tic, 3) || !ftable_finite(ric, 9) || !ftable_finite(pbg, 3)) return ftable_fail(SWF_E_INVALID, who + ": non-finite extrinsics");
    const size_t poses = (size_t)t->n_streams * (size_t)t->opt.window, slots = (size_t)t->n_streams * (size_t)t->opt.feat_cap;
    hipError_t e = hipSuccess;
    const double* dP = ftable_in(t, Ps, t->d_Ps, poses * 3, on_device, e);
    const double* dR = ftable_in(t, Rs, t->d_Rs, poses * 9, on_device, e);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
    FtableArgs P = ftable_args(t);
    FTABLE_LAUNCH(k_ftable_tri_gather, P);
    const int rc = swf_triangulate_batch(dP, dR, (int32_t)poses, tic, ric, pbg, P.tri_start, P.tri_pt0, P.tri_pt1, (int32_t)slots,
                                         t->opt.init_depth, P.tri_depth, P.tri_world, 1, t->st);
    if (rc) return rc;
    FTABLE_LAUNCH(k_ftable_tri_scatter, P);
    return SWF_OK;
}

extern "C" int swf_ftable_list(swf_ftable* t, swf_ftable_listing* out) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_list: null argument");
    FtableArgs P = ftable_args(t);
    P.pass = 0;
    FTABLE_LAUNCH(k_ftable_list, P);
    P.pass = 1;
    FTABLE_LAUNCH(k_ftable_list, P);
    if (out) {
        out->lm_first = P.lm_first; out->proj_first = P.proj_first; out->lm_id = P.lm_id; out->lm_world = P.lm_world;
        out->lm_start = P.lm_start; out->lm_nobs = P.lm_nobs; out->lm_valid = P.lm_valid;
        out->proj_frame = P.proj_frame; out->proj_lm = P.proj_lm; out->proj_uv = P.proj_uv; out->proj_new = P.proj_new;
    }
    return SWF_OK;
}

extern "C" int swf_ftable_set_solved(swf_ftable* t, const int32_t* lm_first, const double* lm_world, const uint8_t* flags,
                                     const double* Ps, const double* Rs, const double tic[3], const double ric[9], const double pbg[3],
                                     int32_t on_device) {
    const std::string who = "swf_ftable_set_solved";
    if (!t || !lm_first || !lm_world || !Ps || !Rs || !tic || !ric || !pbg) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    if (!ftable_finite(tic, 3) || !ftable_finite(ric, 9) || !ftable_finite(pbg, 3)) return ftable_fail(SWF_E_INVALID, who + ": non-finite extrinsics");
    const size_t ns = (size_t)t->n_streams, poses = ns * (size_t)t->opt.window, slots = ns * (size_t)t->opt.feat_cap;
    FtableArgs P = ftable_args(t);
    hipError_t e = hipSuccess;
    if (on_device) { P.in_first = lm_first; P.in_world = lm_world; P.in_flags = flags; }
    else {
        if (lm_first[0] < 0) return ftable_fail(SWF_E_INVALID, who + ": a negative offset");
        for (size_t s = 0; s < ns; s++) if (lm_first[s + 1] < lm_first[s]) return ftable_fail(SWF_E_INVALID, who + ": offsets must be non-decreasing");
        t->rel.assign(lm_first, lm_first + ns + 1);
        for (auto& v : t->rel) v -= lm_first[0];
        const size_t tot = (size_t)t->rel[ns];
        if (tot > slots) return ftable_fail(SWF_E_INVALID, who + ": more landmarks than the table has slots");
        P.in_first = ftable_in(t, (const int32_t*)t->rel.data(), t->d_in_first, ns + 1, 0, e);
        P.in_world = ftable_in(t, lm_world + (size_t)lm_first[0] * 3, t->d_in_world, tot * 3, 0, e);
        P.in_flags = flags ? ftable_in(t, flags + lm_first[0], t->d_in_flags, tot, 0, e) : nullptr;
    }
    P.Ps = ftable_in(t, Ps, t->d_Ps, poses * 3, on_device, e);
    P.Rs = ftable_in(t, Rs, t->d_Rs, poses * 9, on_device, e);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
    ftable_extrinsics(P, tic, ric, pbg);
    FTABLE_LAUNCH(k_ftable_set_solved, P);
    return SWF_OK;
}

extern "C" int swf_ftable_remove_failures(swf_ftable* t, const int32_t** first_out, const int32_t** ids_out) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_remove_failures: null argument");
    FtableArgs P = ftable_args(t);
    P.pass = 0;
    FTABLE_LAUNCH(k_ftable_remove, P);
    P.pass = 1;
    FTABLE_LAUNCH(k_ftable_remove, P);
    t->set = 1 - t->set;
    t->removed = true;
    if (first_out) *first_out = P.rm_first;
    if (ids_out) *ids_out = P.rm_ids;
    return SWF_OK;
}

extern "C" int swf_ftable_fetch(swf_ftable* t, void* dst, const void* device_src, uint64_t bytes) {
    if (!t || (bytes && (!dst || !device_src))) return ftable_fail(SWF_E_INVALID, "swf_ftable_fetch: null argument");
    hipError_t e = hipStreamSynchronize(t->st);
    if (e == hipSuccess && bytes) e = hipMemcpy(dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, std::string("swf_ftable_fetch: ") + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_ftable_removed(swf_ftable* t, int32_t* first, int32_t* ids) {
    const std::string who = "swf_ftable_removed";
    if (!t || !first) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    if (!t->removed) return ftable_fail(SWF_E_STATE, who + ": no swf_ftable_remove_failures yet");
    const size_t ns = (size_t)t->n_streams;
    int rc = swf_ftable_fetch(t, first, t->P.rm_first, (ns + 1) * sizeof(int32_t));
    if (rc) return rc;
    if (first[0] != 0 || first[ns] < 0 || (size_t)first[ns] > ns * (size_t)t->opt.feat_cap) return ftable_fail(SWF_E_STATE, who + ": offsets out of range");
    if (ids && first[ns]) rc = swf_ftable_fetch(t, ids, t->P.rm_ids, (size_t)first[ns] * sizeof(int32_t));
    return rc;
}

extern "C" int swf_ftable_check_parallax(swf_ftable* t) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_check_parallax: null argument");
    FtableArgs P = ftable_args(t);
    FTABLE_LAUNCH(k_ftable_parallax, P);
    return SWF_OK;
}

extern "C" int swf_ftable_slide(swf_ftable* t, const int32_t* mode, const double* P0, const double* R0, const double* P1, const double* R1,
                                const double tic[3], const double ric[9], const double pbg[3], int32_t on_device) {
    const std::string who = "swf_ftable_slide";
    (void)P0; (void)R0;                                     // the reference's arguments of the inverse-depth branch
    if (!t || !mode || !P1 || !R1 || !tic || !ric || !pbg) return ftable_fail(SWF_E_INVALID, who + ": null argument");
    if (!ftable_finite(tic, 3) || !ftable_finite(ric, 9) || !ftable_finite(pbg, 3)) return ftable_fail(SWF_E_INVALID, who + ": non-finite extrinsics");
    const size_t ns = (size_t)t->n_streams;
    FtableArgs P = ftable_args(t);
    hipError_t e = hipSuccess;
    P.mode = ftable_in(t, mode, t->d_mode, ns, 0, e);
    P.P1 = ftable_in(t, P1, t->d_P1, ns * 3, on_device, e);
    P.R1 = ftable_in(t, R1, t->d_R1, ns * 9, on_device, e);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, who + ": hipMemcpyAsync: " + hipGetErrorString(e));
    ftable_extrinsics(P, tic, ric, pbg);
    FTABLE_LAUNCH(k_ftable_slide, P);
    t->set = 1 - t->set;
    return SWF_OK;
}

extern "C" int swf_ftable_download(swf_ftable* t, int32_t* n_frames, int32_t* n_feat, int32_t* id, int32_t* start_frame, int32_t* n_obs,
                                   int32_t* valid, int32_t* solve_flag, double* idepth, double* world, double* obs, int32_t* in_problem) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_download: null argument");
    const size_t ns = (size_t)t->n_streams, F = ns * (size_t)t->opt.feat_cap, O = F * (size_t)t->opt.window;
    const FtableState& S = t->S[t->set];
    hipError_t e = hipStreamSynchronize(t->st);
    auto down = [&](void* dst, const void* src, size_t bytes) { if (e == hipSuccess && dst) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    down(n_frames, S.n_frames, ns * 4); down(n_feat, S.n_feat, ns * 4);
    down(id, S.id, F * 4); down(start_frame, S.start, F * 4); down(n_obs, S.n_obs, F * 4); down(valid, S.valid, F * 4); down(solve_flag, S.flag, F * 4);
    down(idepth, S.idepth, F * 8); down(world, S.world, F * 24); down(obs, S.obs, O * 56); down(in_problem, S.in_problem, O * 4);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, std::string("swf_ftable_download: ") + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_ftable_counts(swf_ftable* t, int32_t* counts, double* parallax) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_counts: null argument");
    const size_t ns = (size_t)t->n_streams;
    int rc = SWF_OK;
    if (counts) rc = swf_ftable_fetch(t, counts, t->P.counts, ns * SWF_FTABLE_NCOUNT * sizeof(int32_t));
    if (!rc && parallax) rc = swf_ftable_fetch(t, parallax, t->P.parallax, ns * sizeof(double));
    if (!rc && !counts && !parallax) rc = swf_ftable_sync(t);
    return rc;
}

extern "C" int swf_ftable_sync(swf_ftable* t) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_sync: null argument");
    const hipError_t e = hipStreamSynchronize(t->st);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, std::string("swf_ftable_sync: ") + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_ftable_clear(swf_ftable* t) {
    if (!t) return ftable_fail(SWF_E_INVALID, "swf_ftable_clear: null argument");
    const size_t ns = (size_t)t->n_streams;
    const FtableState& S = t->S[t->set];
    hipError_t e = hipMemsetAsync(S.n_frames, 0, ns * 4, t->st);
    if (e == hipSuccess) e = hipMemsetAsync(S.n_feat, 0, ns * 4, t->st);
    if (e == hipSuccess) e = hipMemsetAsync(S.n_listed, 0, ns * 4, t->st);
    if (e != hipSuccess) return ftable_fail(SWF_E_NODEVICE, std::string("swf_ftable_clear: ") + hipGetErrorString(e));
    return SWF_OK;
}

extern "C" int swf_ftable_destroy(swf_ftable* t) {
    if (!t) return SWF_OK;
    (void)hipStreamSynchronize(t->st);
    ftable_free(t);
    return SWF_OK;
}
