// swf_gftt.hip — k_gftt_old, k_gftt_eig, k_gftt_max, k_gftt_cand, k_gftt_select, k_gftt_pack (see swf_gftt.h) and the C-ABI
// swf_gftt_detect_batch.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_gftt.h"
#include "swf_devutil.h"
#include "swf_stage.h"

// Every double operation of this file rounds once: the float64 referee evaluates the same expressions and gets the same bits.
#pragma clang fp contract(off)

void swf_internal_set_error(const std::string& m);
static int gftt_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

typedef unsigned long long u64;

// reflect-101 into 0 .. n - 1; what a position outside the specification's reach could still produce is clamped, so no index leaves
// the image whatever the inputs are
__device__ __forceinline__ int gftt_r101(int i, int n) {
    i = i < 0 ? -i : i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// a wave's LDS writes are visible to its own later reads: the hardware keeps a wave's LDS operations in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void gftt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned char* gftt_frame(const GfttArgs& A, int f) { return A.work + (size_t)f * A.L.bytes; }
__device__ __forceinline__ GfttHead* gftt_head(const GfttArgs& A, int f) { return (GfttHead*)(gftt_frame(A, f) + A.L.head); }
__device__ __forceinline__ int gftt_pack(int x, int y) { return (y << 16) | x; }      // 0 <= x, y < 8192

// the half-width table in LDS (s_hw[0 .. r], s_hw[GFTT_RMAX + 1] its maximum); the caller synchronises
__device__ __forceinline__ void gftt_load_hw(const GfttArgs& A, int* s_hw, int tid) {
    if (tid <= A.r) s_hw[tid] = A.user_hw ? A.user_hw[tid] : (int)A.hw[tid];
    if (tid == GFTT_RMAX + 1) {
        int top = -1;
        for (int d = 0; d <= A.r; d++) top = max(top, A.user_hw ? A.user_hw[d] : (int)A.hw[d]);
        s_hw[GFTT_RMAX + 1] = top;
    }
}

// p in disc(c): |dy| <= r and |dx| <= hw[|dy|]
__device__ __forceinline__ bool gftt_in_disc(const int* s_hw, int r, int c, int x, int y) {
    const int dy = abs(y - (c >> 16)), dx = abs(x - (c & 0xFFFF));
    return dy <= r && dx <= s_hw[dy];
}

// Is (x, y) inside the disc of one of list[lo .. hi)?  Four entries per LDS read: the scan is a chain of dependent reads otherwise.
// list is 16-byte aligned; entries below lo (back to a multiple of four) are tested as well, the caller's lists allow that; entries
// from hi on are not looked at.
__device__ __forceinline__ bool gftt_any_disc(const int* s_hw, int r, const int* list, int lo, int hi, int x, int y) {
    for (int j = lo & ~3; j < hi; j += 4) {
        const int4 c = *(const int4*)(list + j);
        const bool hit = gftt_in_disc(s_hw, r, c.x, x, y) || (j + 1 < hi && gftt_in_disc(s_hw, r, c.y, x, y)) ||
                         (j + 2 < hi && gftt_in_disc(s_hw, r, c.z, x, y)) || (j + 3 < hi && gftt_in_disc(s_hw, r, c.w, x, y));
        if (hit) return true;
    }
    return false;
}

__device__ __forceinline__ bool gftt_closer(int c, int x, int y, int r2) {
    const int dx = x - (c & 0xFFFF), dy = y - (c >> 16);
    return dx * dx + dy * dy < r2;
}

// Is (x, y) closer than r to one of list[lo .. hi)?  As gftt_any_disc.
__device__ __forceinline__ bool gftt_any_closer(const int* list, int lo, int hi, int x, int y, int r2) {
    for (int j = lo & ~3; j < hi; j += 4) {
        const int4 c = *(const int4*)(list + j);
        const bool hit = gftt_closer(c.x, x, y, r2) || (j + 1 < hi && gftt_closer(c.y, x, y, r2)) || (j + 2 < hi && gftt_closer(c.z, x, y, r2)) ||
                         (j + 3 < hi && gftt_closer(c.w, x, y, r2));
        if (hit) return true;
    }
    return false;
}

// the kept centres whose disc can reach the rectangle x0 .. x1, y0 .. y1 -> s_near, *s_n; the caller zeroes *s_n and synchronises
// on both sides.  The order of s_near depends on the arrival at the LDS counter; only membership is ever read.
__device__ __forceinline__ void gftt_collect_near(const GfttArgs& A, int f, const int* s_hw, int x0, int y0, int x1, int y1, int* s_near, int* s_n,
                                                  int tid, int stride) {
    const int n_old = gftt_head(A, f)->n_old, wx = s_hw[GFTT_RMAX + 1];
    const int* kept = (const int*)(gftt_frame(A, f) + A.L.kept_c);
    for (int i = tid; i < n_old; i += stride) {
        const int c = kept[i], cx = c & 0xFFFF, cy = c >> 16;
        if (cx + wx >= x0 && cx - wx <= x1 && cy + A.r >= y0 && cy - A.r <= y1) s_near[atomicAdd(s_n, 1)] = c;
    }
}

__device__ __forceinline__ bool gftt_free(const GfttArgs& A, int f, const int* s_hw, const int* s_near, int n_near, int x, int y) {
    if (A.mask && A.mask[((size_t)f * (size_t)A.rows + (size_t)y) * (size_t)A.cols + (size_t)x] == 0) return false;
    return !gftt_any_disc(s_hw, A.r, s_near, 0, n_near, x, y);
}

// ---------------------------------------------------------------------------------------------------------------- stage A
__global__ void __launch_bounds__(GFTT_NMAX) k_gftt_old(GfttArgs A) {
    __shared__ __attribute__((aligned(16))) int s_kept[GFTT_NMAX];
    __shared__ int s_tc[GFTT_NMAX], s_idx[GFTT_NMAX], s_c[GFTT_NMAX], s_kidx[GFTT_NMAX], s_hw[GFTT_RMAX + 2], s_nk;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    GfttHead* H = gftt_head(A, f);
    const int p0 = A.first[f], n = A.first[f + 1] - p0;
    if (tid == 0) { H->n_old = 0; H->n_new = 0; H->n_cand = 0; H->total = 0; H->m = -1.0; H->state = GFTT_FAILED; }
    if (p0 < 0 || n < 0 || n > GFTT_NMAX) {               // device-resident offsets the host could not check: info = -1, nothing else
        if (tid == 0) A.info[f] = -1;
        return;
    }
    double x = 0.0, y = 0.0;
    int tc = 0;
    if (tid < n) {
        x = A.px[2 * ((size_t)p0 + tid)]; y = A.px[2 * ((size_t)p0 + tid) + 1]; tc = A.track_cnt[(size_t)p0 + tid];
        if (A.flags & 1) { x = (double)(float)x; y = (double)(float)y; }
    }
    if (__syncthreads_or((!swf_finite(x) || !swf_finite(y) || tc < 0) ? 1 : 0)) {
        if (tid == 0) A.info[f] = SWF_GFTT_BAD_INPUT;
        return;
    }
    gftt_load_hw(A, s_hw, tid);
    s_tc[tid] = tc;
    __syncthreads();
    if (tid < n) {                                        // rank by counting: track_cnt descending, index ascending
        int rank = 0;
        for (int j = 0; j < n; j++) rank += (s_tc[j] > tc || (s_tc[j] == tc && j < tid)) ? 1 : 0;
        const double rx = rint(x), ry = rint(y);
        const bool inside = rx >= 0.0 && rx < (double)A.cols && ry >= 0.0 && ry < (double)A.rows;
        s_idx[rank] = tid;
        s_c[rank] = inside ? gftt_pack((int)rx, (int)ry) : -1;
    }
    __syncthreads();
    int* w_why = (int*)(gftt_frame(A, f) + A.L.why);
    if (tid < 64) {                                       // one wave: the greedy walk, 64 ranked points at a time
        int nk = 0;
        for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            const bool valid = k < n;
            const int c = valid ? s_c[k] : -1, idx = valid ? s_idx[k] : 0, cx = c & 0xFFFF, cy = c >> 16;
            int code = SWF_GFTT_KEPT;
            bool alive = valid;
            if (alive && c < 0) { code = SWF_GFTT_OUTSIDE; alive = false; }
            if (alive && A.mask && A.mask[((size_t)f * (size_t)A.rows + (size_t)cy) * (size_t)A.cols + (size_t)cx] == 0) { code = SWF_GFTT_CROWDED; alive = false; }
            if (alive && gftt_any_disc(s_hw, A.r, s_kept, 0, nk, cx, cy)) { code = SWF_GFTT_CROWDED; alive = false; }
            for (;;) {
                const u64 live = __ballot(alive);
                if (!live) break;
                const int l = __ffsll((long long)live) - 1;
                const int kc = __shfl(c, l, 64);
                if (lane == l) { s_kept[nk] = c; s_kidx[nk] = idx; alive = false; }
                else if (alive && gftt_in_disc(s_hw, A.r, kc, cx, cy)) { code = SWF_GFTT_CROWDED; alive = false; }
                nk++;
            }
            gftt_wave_sync();
            if (valid) w_why[idx] = code;
        }
        if (lane == 0) s_nk = nk;
    }
    __syncthreads();
    const int nk = s_nk;
    int* w_c = (int*)(gftt_frame(A, f) + A.L.kept_c);
    int* w_i = (int*)(gftt_frame(A, f) + A.L.kept_i);
    if (tid < nk) { w_c[tid] = s_kept[tid]; w_i[tid] = s_kidx[tid]; }
    if (tid == 0) { H->n_old = nk; H->total = nk; H->state = A.max_cnt - nk > 0 ? GFTT_GO : GFTT_SKIP; }
}

// ---------------------------------------------------------------------------------------------------------------- stage B
__global__ void __launch_bounds__(GFTT_THREADS) k_gftt_eig(GfttArgs A) {
    __shared__ unsigned char s_img[GFTT_TH + 4][GFTT_TW + 4];
    __shared__ short s_ix[GFTT_TH + 2][GFTT_TW + 2], s_iy[GFTT_TH + 2][GFTT_TW + 2];
    __shared__ __attribute__((aligned(16))) int s_near[GFTT_NMAX];
    __shared__ int s_hw[GFTT_RMAX + 2], s_nn;
    __shared__ double s_max[GFTT_THREADS / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (gftt_head(A, f)->state != GFTT_GO) return;
    const int ty = blockIdx.x / A.L.tiles_x, tx = blockIdx.x - ty * A.L.tiles_x, x0 = tx * GFTT_TW, y0 = ty * GFTT_TH;
    const unsigned char* img = A.img + (size_t)f * (size_t)A.rows * (size_t)A.cols;
    gftt_load_hw(A, s_hw, tid);
    if (tid == 0) s_nn = 0;
    for (int e = tid; e < (GFTT_TH + 4) * (GFTT_TW + 4); e += GFTT_THREADS) {       // s_img[j][i] = P(r101(x0 - 2 + i), r101(y0 - 2 + j))
        const int j = e / (GFTT_TW + 4), i = e - j * (GFTT_TW + 4);
        s_img[j][i] = img[(size_t)gftt_r101(y0 - 2 + j, A.rows) * (size_t)A.cols + gftt_r101(x0 - 2 + i, A.cols)];
    }
    __syncthreads();
    gftt_collect_near(A, f, s_hw, x0, y0, x0 + GFTT_TW - 1, y0 + GFTT_TH - 1, s_near, &s_nn, tid, GFTT_THREADS);
    // Sobel at the positions of tile + 1.  A position outside the image stands for the product at its reflection q, so the
    // derivatives are those AT q (P around q, again through r101), not those of a reflected image: Ix Iy would change its sign.
    for (int e = tid; e < (GFTT_TH + 2) * (GFTT_TW + 2); e += GFTT_THREADS) {
        const int gj = e / (GFTT_TW + 2), gi = e - gj * (GFTT_TW + 2);
        const int li = min(max(gftt_r101(x0 - 1 + gi, A.cols) - (x0 - 2), 1), GFTT_TW + 2);
        const int lj = min(max(gftt_r101(y0 - 1 + gj, A.rows) - (y0 - 2), 1), GFTT_TH + 2);
        const int tl = s_img[lj - 1][li - 1], tc = s_img[lj - 1][li], tr = s_img[lj - 1][li + 1], ml = s_img[lj][li - 1], mr = s_img[lj][li + 1];
        const int bl = s_img[lj + 1][li - 1], bc = s_img[lj + 1][li], br = s_img[lj + 1][li + 1];
        s_ix[gj][gi] = (short)((tr - tl) + 2 * (mr - ml) + (br - bl));
        s_iy[gj][gi] = (short)((bl - tl) + 2 * (bc - tc) + (br - tr));
    }
    __syncthreads();
    const int n_near = s_nn;
    double* eig = (double*)gftt_frame(A, f);
    double best = -1.0;
#pragma unroll
    for (int k = 0; k < GFTT_TH / 4; k++) {
        const int lx = tid & 63, ly = (tid >> 6) + 4 * k, x = x0 + lx, y = y0 + ly;
        if (x >= A.cols || y >= A.rows) continue;
        int sa = 0, sb = 0, sc = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int gx = s_ix[ly + j][lx + i], gy = s_iy[ly + j][lx + i];
                sa += gx * gx; sb += gx * gy; sc += gy * gy;
            }
        const long long d1 = (long long)sa - (long long)sc, D = d1 * d1 + 4ll * (long long)sb * (long long)sb;
        const double v = ((double)(sa + sc) - sqrt((double)D)) / 18727200.0;
        eig[(size_t)y * (size_t)A.cols + (size_t)x] = v;
        if (gftt_free(A, f, s_hw, s_near, n_near, x, y)) best = fmax(best, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) best = fmax(best, __shfl_xor(best, m, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        double* pmax = (double*)(gftt_frame(A, f) + A.L.pmax);
        pmax[blockIdx.x] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    }
}

__global__ void __launch_bounds__(GFTT_THREADS) k_gftt_max(GfttArgs A) {
    __shared__ double s_max[GFTT_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    GfttHead* H = gftt_head(A, f);
    if (H->state != GFTT_GO) return;
    const double* pmax = (const double*)(gftt_frame(A, f) + A.L.pmax);
    double best = -1.0;
    for (int i = tid; i < A.L.tiles_x * A.L.tiles_y; i += GFTT_THREADS) best = fmax(best, pmax[i]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) best = fmax(best, __shfl_xor(best, m, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) H->m = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
}

// ---------------------------------------------------------------------------------------------------------------- stage C
__global__ void __launch_bounds__(GFTT_THREADS) k_gftt_cand(GfttArgs A) {
    __shared__ double s_e[GFTT_TH + 2][GFTT_TW + 2];
    __shared__ __attribute__((aligned(16))) int s_near[GFTT_NMAX];
    __shared__ int s_hw[GFTT_RMAX + 2], s_nn, s_cnt, s_base;
    const int f = blockIdx.y, tid = threadIdx.x;
    GfttHead* H = gftt_head(A, f);
    if (H->state != GFTT_GO) return;
    const double m = H->m;
    if (!(m > 0.0)) return;                                // no free pixel, or m = 0: no candidates
    const double thr = A.quality * m;
    const int ty = blockIdx.x / A.L.tiles_x, tx = blockIdx.x - ty * A.L.tiles_x, x0 = tx * GFTT_TW, y0 = ty * GFTT_TH;
    const double* eig = (const double*)gftt_frame(A, f);
    gftt_load_hw(A, s_hw, tid);
    if (tid == 0) { s_nn = 0; s_cnt = 0; }
    for (int e = tid; e < (GFTT_TH + 2) * (GFTT_TW + 2); e += GFTT_THREADS) {
        const int gj = e / (GFTT_TW + 2), gi = e - gj * (GFTT_TW + 2), x = x0 - 1 + gi, y = y0 - 1 + gj;
        const bool in = x >= 0 && x < A.cols && y >= 0 && y < A.rows;
        s_e[gj][gi] = in ? eig[(size_t)y * (size_t)A.cols + (size_t)x] : 0.0;
    }
    __syncthreads();
    gftt_collect_near(A, f, s_hw, x0, y0, x0 + GFTT_TW - 1, y0 + GFTT_TH - 1, s_near, &s_nn, tid, GFTT_THREADS);
    __syncthreads();
    const int n_near = s_nn;
    u64* cand_t = (u64*)(gftt_frame(A, f) + A.L.cand_t);
    unsigned* cand_i = (unsigned*)(gftt_frame(A, f) + A.L.cand_i);
    int slot[GFTT_TH / 4];                                 // the tile's candidates take their places in LDS: one global add per workgroup
#pragma unroll
    for (int k = 0; k < GFTT_TH / 4; k++) {
        const int lx = tid & 63, ly = (tid >> 6) + 4 * k, x = x0 + lx, y = y0 + ly;
        slot[k] = -1;
        if (x < 1 || y < 1 || x > A.cols - 2 || y > A.rows - 2) continue;
        const double e = s_e[ly + 1][lx + 1], t = e > thr ? e : 0.0;
        if (t == 0.0) continue;
        bool top = true;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double en = s_e[ly + j][lx + i], tn = en > thr ? en : 0.0;
                top = top && t >= tn;
            }
        if (!top || !gftt_free(A, f, s_hw, s_near, n_near, x, y)) continue;
        slot[k] = atomicAdd(&s_cnt, 1);
    }
    __syncthreads();
    if (tid == 0) s_base = s_cnt ? atomicAdd(&H->n_cand, s_cnt) : 0;      // counts every candidate: n_cand is exact also above cand_cap
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GFTT_TH / 4; k++) {
        const int lx = tid & 63, ly = (tid >> 6) + 4 * k, at = s_base + slot[k];
        if (slot[k] < 0 || at >= A.cand_cap) continue;
        cand_t[at] = (u64)__double_as_longlong(s_e[ly + 1][lx + 1]);      // t = eig here
        cand_i[at] = (unsigned)((y0 + ly) * A.cols + x0 + lx);
    }
}

// ---------------------------------------------------------------------------------------------------------------- stage D
// the 96-bit key (t, i), digits of 8 bits, digit 0 the highest of t
__device__ __forceinline__ bool gftt_less(u64 t, unsigned i, u64 bt, unsigned bi) { return t < bt || (t == bt && i < bi); }
__device__ __forceinline__ int gftt_digit(u64 t, unsigned i, int d) { return d < 8 ? (int)((t >> (56 - 8 * d)) & 255) : (int)((i >> (24 - 8 * (d - 8))) & 255); }
// the digits above d agree with the prefix (pt, pi)
__device__ __forceinline__ bool gftt_match(u64 t, unsigned i, u64 pt, unsigned pi, int d) {
    if (d == 0) return true;
    if (d <= 8) return d == 8 ? t == pt : (t >> (64 - 8 * d)) == (pt >> (64 - 8 * d));
    return t == pt && (i >> (32 - 8 * (d - 8))) == (pi >> (32 - 8 * (d - 8)));
}

__global__ void __launch_bounds__(GFTT_SEL_THREADS) k_gftt_select(GfttArgs A) {
    __shared__ u64 s_t[GFTT_K];
    __shared__ unsigned s_i[GFTT_K];
    __shared__ unsigned s_hist[4][256];
    __shared__ __attribute__((aligned(16))) int s_new[GFTT_NMAX];
    __shared__ unsigned char s_alive[GFTT_SEL_THREADS];
    __shared__ u64 s_pt;
    __shared__ unsigned s_pi;
    __shared__ int s_want, s_nn, s_cnt;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    GfttHead* H = gftt_head(A, f);
    const int state = H->state;
    if (state == GFTT_FAILED) return;                      // k_gftt_old wrote the info
    const int n = H->n_cand, n_old = H->n_old;
    const double m = H->m;
    if (state == GFTT_GO && n > A.cand_cap) {              // info and the true count only
        if (tid == 0) { A.info[f] = SWF_GFTT_TOO_MANY; if (A.n_cand) A.n_cand[f] = n; H->state = GFTT_FAILED; H->total = 0; }
        return;
    }
    const int budget = A.max_cnt - n_old, r2 = A.r * A.r;
    const u64* cand_t = (const u64*)(gftt_frame(A, f) + A.L.cand_t);
    const unsigned* cand_i = (const unsigned*)(gftt_frame(A, f) + A.L.cand_i);
    int n_new = 0, rem = state == GFTT_GO ? n : 0;
    u64 hi_t = ~0ull;                                      // the keys of this round lie below (hi_t, hi_i)
    unsigned hi_i = ~0u;
    while (rem > 0 && n_new < budget) {
        const int take = min(rem, (int)GFTT_K);
        u64 lo_t = 0;
        unsigned lo_i = 0;
        if (rem > GFTT_K) {                                // the GFTT_K-th largest key below hi, digit by digit
            u64 pt = 0;
            unsigned pi = 0;
            int want = GFTT_K;
            for (int d = 0; d < 12; d++) {
                s_hist[tid >> 8][tid & 255] = 0;
                __syncthreads();
                for (int e0 = tid; e0 < n; e0 += 4 * GFTT_SEL_THREADS) {      // four keys in flight per thread; (0, 0) is below every key
                    u64 t4[4];
                    unsigned i4[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int e = e0 + u * GFTT_SEL_THREADS;
                        t4[u] = e < n ? cand_t[e] : 0;
                        i4[u] = e < n ? cand_i[e] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const u64 t = t4[u];
                        const unsigned i = i4[u];
                        if (t == 0 || !gftt_less(t, i, hi_t, hi_i) || !gftt_match(t, i, pt, pi, d)) continue;
                        const int dg = gftt_digit(t, i, d), d0 = __builtin_amdgcn_readfirstlane(dg);
                        if (dg == d0) {                    // the high digits are the same for most keys: one add for the lanes that agree
                            const u64 same = __ballot(1);
                            if (lane == __ffsll((long long)same) - 1) atomicAdd(&s_hist[(tid >> 6) & 3][d0], (unsigned)__popcll(same));
                        } else atomicAdd(&s_hist[(tid >> 6) & 3][dg], 1u);
                    }
                }
                __syncthreads();
                if (tid < 256) s_hist[0][tid] += s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
                __syncthreads();
                if (tid == 0) {
                    int b = 255, above = 0;
                    while (b > 0 && above + (int)s_hist[0][b] < want) { above += (int)s_hist[0][b]; b--; }
                    s_want = want - above;
                    if (d < 8) s_pt = pt | ((u64)b << (56 - 8 * d)); else s_pi = pi | ((unsigned)b << (24 - 8 * (d - 8)));
                    if (d < 8) s_pi = pi; else s_pt = pt;
                }
                __syncthreads();
                pt = s_pt; pi = s_pi; want = s_want;
            }
            lo_t = pt; lo_i = pi;
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int e0 = tid; e0 < n; e0 += 4 * GFTT_SEL_THREADS) {      // gather lo <= key < hi; the sort makes the order of arrival irrelevant
            u64 t4[4];
            unsigned i4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e0 + u * GFTT_SEL_THREADS;
                t4[u] = e < n ? cand_t[e] : 0;
                i4[u] = e < n ? cand_i[e] : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (t4[u] != 0 && gftt_less(t4[u], i4[u], hi_t, hi_i) && !gftt_less(t4[u], i4[u], lo_t, lo_i)) {
                    const int at = atomicAdd(&s_cnt, 1);
                    if (at < GFTT_K) { s_t[at] = t4[u]; s_i[at] = i4[u]; }
                }
        }
        __syncthreads();
        const int cnt = min(s_cnt, (int)GFTT_K);           // == take
        int N2 = 64;
        while (N2 < cnt) N2 <<= 1;
        for (int e = cnt + tid; e < N2; e += GFTT_SEL_THREADS) { s_t[e] = 0; s_i[e] = 0; }   // below every candidate: t != 0
        __syncthreads();
        for (int k = 2; k <= N2; k <<= 1)                  // bitonic network, descending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < N2; e += GFTT_SEL_THREADS) {
                    const int l = e ^ j;
                    if (l > e) {
                        const u64 ta = s_t[e], tb = s_t[l];
                        const unsigned ia = s_i[e], ib = s_i[l];
                        const bool swap = (e & k) == 0 ? gftt_less(ta, ia, tb, ib) : gftt_less(tb, ib, ta, ia);
                        if (swap) { s_t[e] = tb; s_i[e] = ib; s_t[l] = ta; s_i[l] = ia; }
                    }
                }
                __syncthreads();
            }
        // the walk: all threads test 1024 candidates against the points kept before them, one wave walks the survivors
        for (int base = 0; base < cnt && n_new < budget; base += GFTT_SEL_THREADS) {
            {
                const int c = base + tid;
                bool alive = c < cnt;
                if (alive) {
                    const int y = (int)(s_i[c] / (unsigned)A.cols), x = (int)s_i[c] - y * A.cols;
                    alive = !gftt_any_closer(s_new, 0, n_new, x, y, r2);
                }
                s_alive[tid] = alive ? 1 : 0;
            }
            __syncthreads();
            if (tid < 64) {
                const int n0 = n_new;
                int nn = n_new;
                for (int ch = 0; ch < GFTT_SEL_THREADS / 64 && nn < budget; ch++) {
                    const int c = base + ch * 64 + lane;
                    bool alive = c < cnt && s_alive[ch * 64 + lane] != 0;
                    int x = 0, y = 0;
                    if (alive) {
                        y = (int)(s_i[c] / (unsigned)A.cols); x = (int)s_i[c] - y * A.cols;
                        alive = !gftt_any_closer(s_new, n0, nn, x, y, r2);
                    }
                    while (nn < budget) {
                        const u64 live = __ballot(alive);
                        if (!live) break;
                        const int l = __ffsll((long long)live) - 1;
                        const int kx = __shfl(x, l, 64), ky = __shfl(y, l, 64);
                        if (lane == l) { s_new[nn] = gftt_pack(x, y); alive = false; }
                        else if (alive && (x - kx) * (x - kx) + (y - ky) * (y - ky) < r2) alive = false;
                        nn++;
                    }
                    gftt_wave_sync();
                }
                if (lane == 0) s_nn = nn;
            }
            __syncthreads();
            n_new = s_nn;
            __syncthreads();
        }
        hi_t = lo_t; hi_i = lo_i; rem -= take;
    }
    __syncthreads();
    int* w_new = (int*)(gftt_frame(A, f) + A.L.new_c);
    for (int j = tid; j < n_new; j += GFTT_SEL_THREADS) {
        w_new[j] = s_new[j];
        if (A.new_px) {
            A.new_px[((size_t)f * (size_t)A.max_cnt + j) * 2] = (double)(s_new[j] & 0xFFFF);
            A.new_px[((size_t)f * (size_t)A.max_cnt + j) * 2 + 1] = (double)(s_new[j] >> 16);
        }
    }
    if (tid == 0) {
        H->n_new = n_new; H->total = n_old + n_new;
        A.info[f] = SWF_GFTT_OK;
        if (A.n_new) A.n_new[f] = n_new;
        if (A.n_cand) A.n_cand[f] = state == GFTT_GO ? n : 0;
        if (A.max_eig) A.max_eig[f] = state == GFTT_GO && m > 0.0 ? m : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- outputs
__global__ void __launch_bounds__(GFTT_THREADS) k_gftt_pack(GfttArgs A) {
    __shared__ int s_sum[GFTT_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const GfttHead* H = gftt_head(A, f);
    int part = 0;
    for (int g = tid; g < f; g += GFTT_THREADS) part += gftt_head(A, g)->total;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    const int off = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (tid == 0 && A.pack_first) {
        A.pack_first[f] = off;
        if (f == A.n_frames - 1) A.pack_first[f + 1] = off + H->total;
    }
    if (H->state == GFTT_FAILED) return;
    const int p0 = A.first[f], n = A.first[f + 1] - p0, n_old = H->n_old, n_new = H->n_new;
    const int* w_why = (const int*)(gftt_frame(A, f) + A.L.why);
    const int* w_i = (const int*)(gftt_frame(A, f) + A.L.kept_i);
    const int* w_new = (const int*)(gftt_frame(A, f) + A.L.new_c);
    if (tid == 0 && A.n_old) A.n_old[f] = n_old;
    for (int i = tid; i < n; i += GFTT_THREADS) {
        if (A.why) A.why[(size_t)p0 + i] = w_why[i];
        if (A.order) A.order[(size_t)p0 + i] = i < n_old ? w_i[i] : -1;
    }
    for (int j = tid; j < n_old + n_new; j += GFTT_THREADS) {
        const size_t at = (size_t)off + j;
        if (j < n_old) {
            const size_t g = (size_t)p0 + w_i[j];
            double x = A.px[2 * g], y = A.px[2 * g + 1];
            if (A.flags & 1) { x = (double)(float)x; y = (double)(float)y; }
            if (A.pack_px) { A.pack_px[2 * at] = x; A.pack_px[2 * at + 1] = y; }
            if (A.pack_src) A.pack_src[at] = w_i[j];
        } else {
            const int c = w_new[j - n_old];
            if (A.pack_px) { A.pack_px[2 * at] = (double)(c & 0xFFFF); A.pack_px[2 * at + 1] = (double)(c >> 16); }
            if (A.pack_src) A.pack_src[at] = -1;
        }
    }
}

bool gftt_sizes_ok(int rows, int cols, int cand_cap) {
    return rows >= 8 && cols >= 8 && rows <= 8192 && cols <= 8192 && cand_cap >= 64 && cand_cap <= (1 << 24);
}

}  // namespace

GfttLayout gftt_layout(int rows, int cols, int cand_cap) {
    GfttLayout L{};
    L.tiles_x = (cols + GFTT_TW - 1) / GFTT_TW; L.tiles_y = (rows + GFTT_TH - 1) / GFTT_TH;
    size_t at = (size_t)rows * (size_t)cols * 8;                                   // eig
    L.cand_t = at; at += (size_t)cand_cap * 8;
    L.pmax = at; at += (size_t)L.tiles_x * (size_t)L.tiles_y * 8;
    L.head = at; at += GFTT_HEAD;
    L.kept_c = at; at += GFTT_NMAX * 4;
    L.kept_i = at; at += GFTT_NMAX * 4;
    L.new_c = at; at += GFTT_NMAX * 4;
    L.why = at; at += GFTT_NMAX * 4;
    L.cand_i = at; at += (size_t)cand_cap * 4;
    L.bytes = (at + 15) / 16 * 16;
    return L;
}

int swf_internal_gftt_launch(const GfttArgs& A, hipStream_t st) {
    if (A.n_frames <= 0) return SWF_OK;
    const unsigned nf = (unsigned)A.n_frames, tiles = (unsigned)(A.L.tiles_x * A.L.tiles_y);
    const char* what = "k_gftt_old";
    hipLaunchKernelGGL(k_gftt_old, dim3(nf), dim3(GFTT_NMAX), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) { what = "k_gftt_eig"; hipLaunchKernelGGL(k_gftt_eig, dim3(tiles, nf), dim3(GFTT_THREADS), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { what = "k_gftt_max"; hipLaunchKernelGGL(k_gftt_max, dim3(nf), dim3(GFTT_THREADS), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { what = "k_gftt_cand"; hipLaunchKernelGGL(k_gftt_cand, dim3(tiles, nf), dim3(GFTT_THREADS), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { what = "k_gftt_select"; hipLaunchKernelGGL(k_gftt_select, dim3(nf), dim3(GFTT_SEL_THREADS), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { what = "k_gftt_pack"; hipLaunchKernelGGL(k_gftt_pack, dim3(nf), dim3(GFTT_THREADS), 0, st, A); e = hipGetLastError(); }
    if (e != hipSuccess) return gftt_fail(SWF_E_NODEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" size_t swf_gftt_workspace_bytes(int32_t rows, int32_t cols, int32_t cand_cap) {
    if (!gftt_sizes_ok(rows, cols, cand_cap)) return 0;
    return gftt_layout(rows, cols, cand_cap).bytes;
}

extern "C" int swf_gftt_detect_batch(int32_t n_frames, int32_t rows, int32_t cols, const uint8_t* img, const uint8_t* mask,
                                     const int32_t* first, const double* px, const int32_t* track_cnt,
                                     int32_t max_cnt, int32_t min_dist, double quality, const int32_t* disc_halfwidth, int32_t cand_cap, int32_t flags,
                                     int32_t* order, int32_t* why, int32_t* n_old, double* new_px, int32_t* n_new, int32_t* n_cand, double* max_eig,
                                     int32_t* pack_first, double* pack_px, int32_t* pack_src, int32_t* info, uint8_t* work,
                                     int32_t on_device, void* stream) {
    const std::string who = "swf_gftt_detect_batch";
    if (n_frames < 0 || !img || !first || !px || !track_cnt || !info) return gftt_fail(SWF_E_INVALID, who + ": null argument");
    if (!(quality > 0.0) || !(quality <= 1.0)) return gftt_fail(SWF_E_INVALID, who + ": quality must lie in (0, 1]");
    if (cand_cap < 64) return gftt_fail(SWF_E_INVALID, who + ": cand_cap below 64");
    if (rows < 8 || cols < 8 || rows > 8192 || cols > 8192) return gftt_fail(SWF_E_UNSUPPORTED, who + ": rows and cols outside 8 .. 8192");
    if (max_cnt < 1 || max_cnt > SWF_GFTT_NMAX) return gftt_fail(SWF_E_UNSUPPORTED, who + ": max_cnt outside 1 .. 1024");
    if (min_dist < 1 || min_dist > GFTT_RMAX) return gftt_fail(SWF_E_UNSUPPORTED, who + ": min_dist outside 1 .. 64");
    if (cand_cap > (1 << 24)) return gftt_fail(SWF_E_UNSUPPORTED, who + ": cand_cap above 2^24");
    if (flags < 0 || flags > 1) return gftt_fail(SWF_E_UNSUPPORTED, who + ": unknown flag bits");
    if (n_frames > 65535) return gftt_fail(SWF_E_UNSUPPORTED, who + ": more than 65535 frames");
    if (on_device && !work) return gftt_fail(SWF_E_INVALID, who + ": device memory needs the workspace");
    if (n_frames == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    GfttArgs A{};
    A.n_frames = n_frames; A.rows = rows; A.cols = cols; A.max_cnt = max_cnt; A.r = min_dist; A.cand_cap = cand_cap; A.flags = flags; A.quality = quality;
    A.L = gftt_layout(rows, cols, cand_cap);
    for (int d = 0; d <= min_dist; d++) {                // floor(sqrt(r^2 - d^2)) in integers
        int h = 0;
        while ((h + 1) * (h + 1) <= min_dist * min_dist - d * d) h++;
        A.hw[d] = (short)h;
    }
    if (on_device) {            // the offsets are device memory: the kernels make the checks
        A.img = img; A.mask = mask; A.first = first; A.px = px; A.track_cnt = track_cnt; A.user_hw = disc_halfwidth;
        A.order = order; A.why = why; A.n_old = n_old; A.new_px = new_px; A.n_new = n_new; A.n_cand = n_cand; A.max_eig = max_eig;
        A.pack_first = pack_first; A.pack_px = pack_px; A.pack_src = pack_src; A.info = info; A.work = work;
        return swf_internal_gftt_launch(A, st);
    }
    // ---- host memory: the argument errors and the BAD_INPUT frames before the device is touched
    if (first[0] < 0) return gftt_fail(SWF_E_INVALID, who + ": a negative point offset");
    for (int i = 0; i < n_frames; i++) {
        if (first[i + 1] < first[i]) return gftt_fail(SWF_E_INVALID, who + ": point offsets must be non-decreasing");
        if (first[i + 1] - first[i] > SWF_GFTT_NMAX) return gftt_fail(SWF_E_UNSUPPORTED, who + ": a frame of more than 1024 tracked points");
    }
    const bool as_float = (flags & 1) != 0;
    std::vector<int32_t> code((size_t)n_frames);
    bool any = false;
    for (int i = 0; i < n_frames; i++) {
        bool good = true;
        for (size_t g = (size_t)first[i]; g < (size_t)first[i + 1]; g++)
            good = good && std::isfinite(as_float ? (double)(float)px[2 * g] : px[2 * g]) && std::isfinite(as_float ? (double)(float)px[2 * g + 1] : px[2 * g + 1])
                   && track_cnt[g] >= 0;
        code[(size_t)i] = good ? SWF_GFTT_OK : SWF_GFTT_BAD_INPUT;
        info[i] = code[(size_t)i];
        any = any || good;
    }
    if (!any) return SWF_OK;    // every frame is BAD_INPUT: the device is not touched

    const size_t nf = (size_t)n_frames, np = (size_t)(first[n_frames] - first[0]), img_bytes = (size_t)rows * (size_t)cols, mc = (size_t)max_cnt;
    const size_t npack = np + nf * mc;
    std::vector<int32_t> rel(first, first + n_frames + 1);
    for (auto& v : rel) v -= first[0];
    // a frame leaves what it does not write as the caller had it: the results pass through staging arrays
    std::vector<int32_t> h_info(nf), h_order(order ? np : 0), h_why(why ? np : 0), h_nold(nf), h_nnew(nf), h_ncand(n_cand ? nf : 0);
    std::vector<int32_t> h_pfirst(nf + 1), h_psrc(pack_src ? npack : 0);
    std::vector<double> h_new(new_px ? nf * mc * 2 : 0), h_maxe(max_eig ? nf : 0), h_ppx(pack_px ? npack * 2 : 0);
    std::vector<double> h_eig(work ? nf * img_bytes : 0);
    HostStage S("swf_gftt_detect_batch", st);
    A.img = S.up(img, nf * img_bytes);
    if (mask) A.mask = S.up(mask, nf * img_bytes);
    A.first = S.up(rel.data(), rel.size());
    A.px = S.up(px + (size_t)first[0] * 2, np * 2);
    A.track_cnt = S.up(track_cnt + (size_t)first[0], np);
    if (disc_halfwidth) A.user_hw = S.up(disc_halfwidth, (size_t)min_dist + 1);
    A.info = S.out<int32_t>(nf);
    A.work = S.out<uint8_t>(nf * A.L.bytes);
    A.n_old = S.out<int32_t>(nf);
    A.n_new = S.out<int32_t>(nf);
    A.pack_first = S.out<int32_t>(nf + 1);
    if (order) A.order = S.out<int32_t>(np);
    if (why) A.why = S.out<int32_t>(np);
    if (new_px) A.new_px = S.out<double>(nf * mc * 2);
    if (n_cand) A.n_cand = S.out<int32_t>(nf);
    if (max_eig) A.max_eig = S.out<double>(nf);
    if (pack_px) A.pack_px = S.out<double>(npack * 2);
    if (pack_src) A.pack_src = S.out<int32_t>(npack);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_gftt_launch(A, st);
    if (rc) return rc;
    S.down(h_info.data(), A.info, nf);
    S.down(h_nold.data(), A.n_old, nf);
    S.down(h_nnew.data(), A.n_new, nf);
    S.down(h_pfirst.data(), A.pack_first, nf + 1);
    S.down(h_order.data(), A.order, h_order.size());
    S.down(h_why.data(), A.why, h_why.size());
    S.down(h_new.data(), A.new_px, h_new.size());
    S.down(h_ncand.data(), A.n_cand, h_ncand.size());
    S.down(h_maxe.data(), A.max_eig, h_maxe.size());
    S.down(h_ppx.data(), A.pack_px, h_ppx.size());
    S.down(h_psrc.data(), A.pack_src, h_psrc.size());
    if (work)
        for (size_t i = 0; i < nf; i++) S.down(h_eig.data() + i * img_bytes, (const double*)(A.work + i * A.L.bytes), img_bytes);
    S.sync();
    if (S.failed()) return S.rc();
    for (size_t i = 0; i < nf; i++)
        if (h_info[i] < 0 || (h_info[i] == SWF_GFTT_BAD_INPUT) != (code[i] == SWF_GFTT_BAD_INPUT))
            return gftt_fail(SWF_E_STATE, who + ": the device classified a frame differently from the host");
    for (size_t i = 0; i < nf; i++) {
        info[i] = h_info[i];
        if (h_info[i] == SWF_GFTT_TOO_MANY && n_cand) n_cand[i] = h_ncand[i];
        if (h_info[i] != SWF_GFTT_OK) continue;
        const size_t lo = (size_t)rel[i], hi = (size_t)rel[i + 1], at = (size_t)first[i];
        if (order) std::copy(h_order.begin() + lo, h_order.begin() + hi, order + at);
        if (why) std::copy(h_why.begin() + lo, h_why.begin() + hi, why + at);
        if (n_old) n_old[i] = h_nold[i];
        if (n_new) n_new[i] = h_nnew[i];
        if (n_cand) n_cand[i] = h_ncand[i];
        if (max_eig) max_eig[i] = h_maxe[i];
        if (new_px) std::copy(h_new.begin() + i * mc * 2, h_new.begin() + (i * mc + (size_t)h_nnew[i]) * 2, new_px + i * mc * 2);
        // the eig of a frame whose detector ran (budget > 0)
        if (work && max_cnt - h_nold[i] > 0) std::copy(h_eig.begin() + i * img_bytes, h_eig.begin() + (i + 1) * img_bytes, (double*)(work + i * A.L.bytes));
    }
    if (pack_first) std::copy(h_pfirst.begin(), h_pfirst.end(), pack_first);
    const size_t used = (size_t)h_pfirst[nf];
    if (pack_px) std::copy(h_ppx.begin(), h_ppx.begin() + used * 2, pack_px);
    if (pack_src) std::copy(h_psrc.begin(), h_psrc.begin() + used, pack_src);
    return SWF_OK;
}
