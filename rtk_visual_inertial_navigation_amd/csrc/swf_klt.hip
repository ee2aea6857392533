// swf_klt.hip — k_klt_pyrdown, k_klt_track, k_klt_compact (see swf_klt.h) and the C-ABI swf_klt_track_batch.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_klt.h"
#include "swf_devutil.h"
#include "swf_stage.h"

// Every double operation of this file rounds once: the float64 referee evaluates the same expressions and gets the same bits.
#pragma clang fp contract(off)

void swf_internal_set_error(const std::string& m);
static int klt_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

// reflect-101 into 0 .. n - 1.  One reflection covers every index the specification reads (n > win); what a position outside the
// specification could still produce is clamped, so no index leaves the image whatever the inputs are.
__device__ __forceinline__ int klt_r101(int i, int n) {
    i = i < 0 ? -i : i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ const unsigned char* klt_level(const KltArgs& A, int which, int f, int l) {
    if (l == 0) return (which ? A.cur_img : A.prev_img) + (size_t)f * (size_t)A.rows * (size_t)A.cols;
    return A.pyr + ((size_t)f * 2 + (size_t)which) * A.half_bytes + A.loff[l];
}

// a wave's LDS writes are visible to its own later reads: the hardware keeps a wave's LDS operations in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void klt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// the sum over the wave in every lane; the addends are integers below 2^35, so every order gives the same double
__device__ __forceinline__ double klt_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the non-finite test of a pair on what is staged; lanes stride over the 2 n coordinates
__device__ __forceinline__ bool klt_bad_coords(const KltArgs& A, int p0, int n, int at, int stride) {
    const bool as_float = (A.flags & 1) != 0, use_guess = (A.flags & 2) != 0;
    bool bad = false;
    for (int i = at; i < 2 * n; i += stride) {
        double v = A.prev_px[(size_t)p0 * 2 + i];
        if (as_float) v = (double)(float)v;
        bad |= !swf_finite(v);
        if (use_guess) {
            double u = A.guess_px[(size_t)p0 * 2 + i];
            if (as_float) u = (double)(float)u;
            bad |= !swf_finite(u);
        }
    }
    return bad;
}

// Level l from level l - 1 for image blockIdx.x = 2 pair + which: dst(x, y) = (sum k_i k_j src(r101(2x + i - 2), r101(2y + j - 2)) + 128) >> 8,
// k = 1 4 6 4 1.  A thread forms four neighbouring outputs of a row from 5 x 11 bytes.
__global__ void __launch_bounds__(KLT_THREADS) k_klt_pyrdown(KltArgs A, int l) {
    const int f = blockIdx.x >> 1, which = blockIdx.x & 1;
    const int w = A.lw[l - 1], h = A.lh[l - 1], wd = A.lw[l], hd = A.lh[l];
    const int per_row = (wd + 3) >> 2;
    const int u = blockIdx.y * KLT_THREADS + threadIdx.x;
    if (u >= per_row * hd) return;
    const int y = u / per_row, x0 = (u - y * per_row) * 4;
    const unsigned char* src = klt_level(A, which, f, l - 1);
    unsigned char* dst = A.pyr + ((size_t)f * 2 + (size_t)which) * A.half_bytes + A.loff[l];
    int cx[11];
#pragma unroll
    for (int i = 0; i < 11; i++) cx[i] = klt_r101(2 * x0 + i - 2, w);
    int acc[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int kj = j == 2 ? 6 : (j == 1 || j == 3) ? 4 : 1;
        const unsigned char* row = src + (size_t)klt_r101(2 * y + j - 2, h) * (size_t)w;
        int p[11];
#pragma unroll
        for (int i = 0; i < 11; i++) p[i] = row[cx[i]];
#pragma unroll
        for (int o = 0; o < 4; o++) acc[o] += kj * (p[2 * o] + 4 * p[2 * o + 1] + 6 * p[2 * o + 2] + 4 * p[2 * o + 3] + p[2 * o + 4]);
    }
#pragma unroll
    for (int o = 0; o < 4; o++)
        if (x0 + o < wd) dst[(size_t)y * (size_t)wd + x0 + o] = (unsigned char)((acc[o] + 128) >> 8);
}

__global__ void __launch_bounds__(KLT_THREADS) k_klt_track(KltArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned char s_all[KLT_WAVES][(KLT_LDS_WAVE + 15) / 16 * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x / A.blocks_per_pair, bx = blockIdx.x - f * A.blocks_per_pair;
    const int p0 = A.first[f], n = A.first[f + 1] - p0;
    if (p0 < 0 || n < 0 || n > KLT_NMAX) return;          // k_klt_compact reports info = -1
    if (bx * KLT_WAVES + wave >= n) return;
    if (__any(klt_bad_coords(A, p0, n, lane, 64))) return; // k_klt_compact reports SWF_KLT_BAD_INPUT
    const bool as_float = (A.flags & 1) != 0, use_guess = (A.flags & 2) != 0, back = (A.flags & 4) != 0;
    unsigned char* s_foot = s_all[wave];
    short* s_gx = (short*)(s_foot + KLT_FOOT);
    short* s_gy = s_gx + KLT_GRID;
    const int win = A.win, G = win + 1, F = win + 3, nel = win * win, ngrid = G * G, nfoot = F * F;
    const double half = (double)((win - 1) / 2);
    // element e = lane + 64 t of the template is (i, j) = (e % win, e / win); of the corner grid (c, r) = (e % G, e / G)
    int ij[KLT_PER_LANE], rc[KLT_GRID_PER_LANE];
#pragma unroll
    for (int t = 0; t < KLT_PER_LANE; t++) {
        const int e = lane + 64 * t, j = e / win;
        ij[t] = e < nel ? (j << 5) | (e - j * win) : 0;
    }
#pragma unroll
    for (int t = 0; t < KLT_GRID_PER_LANE; t++) {
        const int e = lane + 64 * t, r = e / G;
        rc[t] = e < ngrid ? (r << 8) | (e - r * G) : -1;
    }
    for (int pt = bx * KLT_WAVES + wave; pt < n; pt += KLT_WAVES * A.blocks_per_pair) {
        const size_t g = (size_t)p0 + pt;
        double prx = A.prev_px[2 * g], pry = A.prev_px[2 * g + 1];
        double inix = use_guess ? A.guess_px[2 * g] : prx, iniy = use_guess ? A.guess_px[2 * g + 1] : pry;
        if (as_float) { prx = (double)(float)prx; pry = (double)(float)pry; inix = (double)(float)inix; iniy = (double)(float)iniy; }
        double srcx = prx, srcy = pry;
        double curx = 0.0, cury = 0.0, bkx = 0.0, bky = 0.0;
        int fails = 0;                                    // bit 0 / 1: forward lost / flat, bit 2 / 3: reverse lost / flat
        for (int pass = 0; pass < (back ? 2 : 1); pass++) {
            const int top = pass ? A.top_b : A.top_f;
            int my_it = -1;                               // lane l keeps the trace of level l
            double my_x = 0.0, my_y = 0.0;
            double qx = 0.0, qy = 0.0;
            bool lost = false, flat = false;
            for (int l = top; l >= 0; l--) {
                const int w = A.lw[l], h = A.lh[l];
                const unsigned char* I = klt_level(A, pass, f, l);
                const unsigned char* J = klt_level(A, 1 - pass, f, l);
                const double scale = 1.0 / (double)(1 << l);
                double px = srcx * scale, py = srcy * scale;
                if (l == top) { qx = inix * scale; qy = iniy * scale; }
                else { qx = 2.0 * qx; qy = 2.0 * qy; }
                if (lane == l) { my_it = -1; my_x = qx; my_y = qy; }
                px = px - half; py = py - half;
                const double fpx = floor(px), fpy = floor(py);
                if (!(fpx >= (double)-win && fpx < (double)w && fpy >= (double)-win && fpy < (double)h)) {
                    if (l == 0) lost = true;
                    continue;
                }
                const int ix = (int)fpx, iy = (int)fpy;
                int w00, w01, w10, w11;
                {
                    const double a = px - fpx, b = py - fpy;
                    w00 = (int)rint((1.0 - a) * (1.0 - b) * 16384.0);
                    w01 = (int)rint(a * (1.0 - b) * 16384.0);
                    w10 = (int)rint((1.0 - a) * b * 16384.0);
                    w11 = 16384 - w00 - w01 - w10;
                }
                // ---- the (win + 3)^2 footprint of the template, origin ip - 1
                klt_wave_sync();
                for (int e = lane; e < nfoot; e += 64) {
                    const int r = e / F, c = e - r * F;
                    s_foot[e] = I[(size_t)klt_r101(iy - 1 + r, h) * (size_t)w + klt_r101(ix - 1 + c, w)];
                }
                klt_wave_sync();
                // ---- Scharr on the (win + 1)^2 corner grid: 0 outside the image
#pragma unroll
                for (int t = 0; t < KLT_GRID_PER_LANE; t++) {
                    if (rc[t] < 0) continue;
                    const int r = rc[t] >> 8, c = rc[t] & 255, o = (r + 1) * F + c + 1;
                    const bool inside = (unsigned)(ix + c) < (unsigned)w && (unsigned)(iy + r) < (unsigned)h;
                    const int tl = s_foot[o - F - 1], tc = s_foot[o - F], tr = s_foot[o - F + 1], ml = s_foot[o - 1], mr = s_foot[o + 1];
                    const int bl = s_foot[o + F - 1], bc = s_foot[o + F], br = s_foot[o + F + 1];
                    const int vx = 3 * (tr - tl) + 10 * (mr - ml) + 3 * (br - bl);
                    const int vy = 3 * (bl - tl) + 10 * (bc - tc) + 3 * (br - tr);
                    s_gx[lane + 64 * t] = (short)(inside ? vx : 0);
                    s_gy[lane + 64 * t] = (short)(inside ? vy : 0);
                }
                klt_wave_sync();
                // ---- the template in registers and the sums of A
                int It[KLT_PER_LANE], Itx[KLT_PER_LANE], Ity[KLT_PER_LANE];
                int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
                for (int t = 0; t < KLT_PER_LANE; t++) {
                    const bool valid = lane + 64 * t < nel;
                    const int i = ij[t] & 31, j = ij[t] >> 5, o = (j + 1) * F + i + 1, og = j * G + i;
                    const int v = s_foot[o] * w00 + s_foot[o + 1] * w01 + s_foot[o + F] * w10 + s_foot[o + F + 1] * w11;
                    const int vx = s_gx[og] * w00 + s_gx[og + 1] * w01 + s_gx[og + G] * w10 + s_gx[og + G + 1] * w11;
                    const int vy = s_gy[og] * w00 + s_gy[og + 1] * w01 + s_gy[og + G] * w10 + s_gy[og + G + 1] * w11;
                    It[t] = (v + 256) >> 9;
                    Itx[t] = valid ? (vx + 8192) >> 14 : 0;
                    Ity[t] = valid ? (vy + 8192) >> 14 : 0;
                    s11 += Itx[t] * Itx[t]; s12 += Itx[t] * Ity[t]; s22 += Ity[t] * Ity[t];
                }
                const double A11 = klt_wave_sum((double)s11) * 0x1p-20, A12 = klt_wave_sum((double)s12) * 0x1p-20;
                const double A22 = klt_wave_sum((double)s22) * 0x1p-20;
                double D = A11 * A22 - A12 * A12;
                const double min_e = (A22 + A11 - sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (double)(2 * win * win);
                if (min_e < A.min_eig || D < 0x1p-23) {
                    if (l == 0) flat = true;
                    continue;
                }
                D = 1.0 / D;
                // ---- the iterations
                qx = qx - half; qy = qy - half;
                double pdx = 0.0, pdy = 0.0;
                int cnt = 0;
                for (int it = 0; it < A.max_count; it++) {
                    const double fqx = floor(qx), fqy = floor(qy);
                    if (!(fqx >= (double)-win && fqx < (double)w && fqy >= (double)-win && fqy < (double)h)) {
                        if (l == 0) lost = true;
                        break;
                    }
                    const int jx = (int)fqx, jy = (int)fqy;
                    const double a = qx - fqx, b = qy - fqy;
                    w00 = (int)rint((1.0 - a) * (1.0 - b) * 16384.0);
                    w01 = (int)rint(a * (1.0 - b) * 16384.0);
                    w10 = (int)rint((1.0 - a) * b * 16384.0);
                    w11 = 16384 - w00 - w01 - w10;
                    klt_wave_sync();
#pragma unroll
                    for (int t = 0; t < KLT_GRID_PER_LANE; t++) {
                        if (rc[t] < 0) continue;
                        s_foot[lane + 64 * t] = J[(size_t)klt_r101(jy + (rc[t] >> 8), h) * (size_t)w + klt_r101(jx + (rc[t] & 255), w)];
                    }
                    klt_wave_sync();
                    int b1p = 0, b2p = 0;
#pragma unroll
                    for (int t = 0; t < KLT_PER_LANE; t++) {
                        const int og = (ij[t] >> 5) * G + (ij[t] & 31);
                        const int v = s_foot[og] * w00 + s_foot[og + 1] * w01 + s_foot[og + G] * w10 + s_foot[og + G + 1] * w11;
                        const int d = ((v + 256) >> 9) - It[t];
                        b1p += d * Itx[t]; b2p += d * Ity[t];
                    }
                    const double b1 = klt_wave_sum((double)b1p) * 0x1p-20, b2 = klt_wave_sum((double)b2p) * 0x1p-20;
                    const double dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                    qx = qx + dx; qy = qy + dy;
                    cnt++;
                    if (dx * dx + dy * dy <= A.eps2) break;
                    if (it > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
                        qx = qx - dx * 0.5; qy = qy - dy * 0.5;
                        break;
                    }
                    pdx = dx; pdy = dy;
                }
                qx = qx + half; qy = qy + half;
                if (lane == l) { my_it = cnt; my_x = qx; my_y = qy; }
            }
            if (as_float) { qx = (double)(float)qx; qy = (double)(float)qy; }
            if (lane <= KLT_LMAX) {
                const size_t at = (g * 2 + (size_t)pass) * (KLT_LMAX + 1) + lane;
                if (A.trace_iters) A.trace_iters[at] = my_it;
                if (A.trace_px) { A.trace_px[2 * at] = my_x; A.trace_px[2 * at + 1] = my_y; }
            }
            fails |= ((lost ? 1 : 0) | (flat ? 2 : 0)) << (2 * pass);
            if (pass == 0) {                              // the reverse pass: images swapped, from cur, started at the previous position
                curx = qx; cury = qy;
                srcx = qx; srcy = qy; inix = prx; iniy = pry;
            } else { bkx = qx; bky = qy; }
        }
        if (!back && lane <= KLT_LMAX) {
            const size_t at = (g * 2 + 1) * (KLT_LMAX + 1) + lane;
            if (A.trace_iters) A.trace_iters[at] = -1;
            if (A.trace_px) { A.trace_px[2 * at] = 0.0; A.trace_px[2 * at + 1] = 0.0; }
        }
        if (lane == 0) {
            int code = (fails & 1) ? SWF_KLT_FWD_LOST : (fails & 2) ? SWF_KLT_FWD_FLAT : SWF_KLT_TRACKED;
            if (back && code == SWF_KLT_TRACKED) {
                const double dx = prx - bkx, dy = pry - bky;
                code = (fails & 4) ? SWF_KLT_BACK_LOST : (fails & 8) ? SWF_KLT_BACK_FLAT
                     : sqrt(dx * dx + dy * dy) > A.back_dist ? SWF_KLT_BACK_FAR : SWF_KLT_TRACKED;
            }
            if (code == SWF_KLT_TRACKED) {
                const double rx = rint(curx), ry = rint(cury);
                if (!(rx >= 1.0 && rx < (double)(A.cols - 1) && ry >= 1.0 && ry < (double)(A.rows - 1))) code = SWF_KLT_BORDER;
            }
            const int keep = code == SWF_KLT_TRACKED ? 1 : 0;
            if (A.cur_px) { A.cur_px[2 * g] = curx; A.cur_px[2 * g + 1] = cury; }
            if (A.back_px && back) { A.back_px[2 * g] = bkx; A.back_px[2 * g + 1] = bky; }
            if (A.status) A.status[g] = (unsigned char)keep;
            if (A.why) A.why[g] = code;
            if (!A.status && !A.why && A.keep_idx) A.keep_idx[g] = keep;      // k_klt_compact reads the flags from the first of these three
        }
    }
}

// info of the pair, and the flags of its points -> keep_idx (ascending from first[f], -1 behind), n_keep
__global__ void __launch_bounds__(KLT_THREADS) k_klt_compact(KltArgs A) {
    __shared__ int s_pre[2][KLT_THREADS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int p0 = A.first[f], n = A.first[f + 1] - p0;
    if (p0 < 0 || n < 0 || n > KLT_NMAX) {                // device-resident offsets the host could not check: info = -1, nothing else
        if (tid == 0) A.info[f] = -1;
        return;
    }
    if (__syncthreads_or(klt_bad_coords(A, p0, n, tid, KLT_THREADS) ? 1 : 0)) {
        if (tid == 0) A.info[f] = SWF_KLT_BAD_INPUT;
        return;
    }
    if (tid == 0) A.info[f] = SWF_KLT_OK;
    if (!A.keep_idx && !A.n_keep) return;
    constexpr int PER = KLT_NMAX / KLT_THREADS;           // thread t owns points PER t .. PER t + PER - 1
    int keep[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int i = tid * PER + j;
        keep[j] = 0;
        if (i < n) {
            const size_t g = (size_t)p0 + i;
            keep[j] = A.status ? (A.status[g] != 0) : A.why ? (A.why[g] == SWF_KLT_TRACKED) : (A.keep_idx[g] != 0);
        }
        mine += keep[j];
    }
    s_pre[0][tid] = mine;
    __syncthreads();                                      // every flag is read before keep_idx is written
    int src = 0;
    for (int s = 1; s < KLT_THREADS; s <<= 1) {           // inclusive prefix sum, two buffers
        s_pre[1 - src][tid] = s_pre[src][tid] + (tid >= s ? s_pre[src][tid - s] : 0);
        src = 1 - src;
        __syncthreads();
    }
    int at = s_pre[src][tid] - mine;
    const int total = s_pre[src][KLT_THREADS - 1];
    if (A.keep_idx) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int i = tid * PER + j;
            if (i < n && keep[j]) A.keep_idx[(size_t)p0 + at] = i;
            at += keep[j];
        }
        for (int i = total + tid; i < n; i += KLT_THREADS) A.keep_idx[(size_t)p0 + i] = -1;
    }
    if (tid == 0 && A.n_keep) A.n_keep[f] = total;
}

// level sizes 0 .. KLT_LMAX of a rows x cols image (every level, built or not: the workspace layout depends on the image size alone)
void klt_sizes(int rows, int cols, int lw[KLT_LMAX + 1], int lh[KLT_LMAX + 1]) {
    lw[0] = cols; lh[0] = rows;
    for (int l = 1; l <= KLT_LMAX; l++) { lw[l] = (lw[l - 1] + 1) / 2; lh[l] = (lh[l - 1] + 1) / 2; }
}

}  // namespace

int swf_internal_klt_launch(const KltArgs& A, hipStream_t st) {
    if (A.n_pairs <= 0) return SWF_OK;
    const char* what = "k_klt_pyrdown";
    hipError_t e = hipSuccess;
    for (int l = 1; l <= A.top_build && e == hipSuccess; l++) {
        const int units = ((A.lw[l] + 3) / 4) * A.lh[l];
        hipLaunchKernelGGL(k_klt_pyrdown, dim3((unsigned)A.n_pairs * 2u, (unsigned)((units + KLT_THREADS - 1) / KLT_THREADS)), dim3(KLT_THREADS), 0, st, A, l);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        what = "k_klt_track";
        hipLaunchKernelGGL(k_klt_track, dim3((unsigned)A.n_pairs * (unsigned)A.blocks_per_pair), dim3(KLT_THREADS), 0, st, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        what = "k_klt_compact";
        hipLaunchKernelGGL(k_klt_compact, dim3((unsigned)A.n_pairs), dim3(KLT_THREADS), 0, st, A);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return klt_fail(SWF_E_NODEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" size_t swf_klt_pyramid_bytes(int32_t rows, int32_t cols, int32_t max_level) {
    if (rows < 1 || cols < 1 || rows > 8192 || cols > 8192 || max_level < 0 || max_level > SWF_KLT_LMAX) return 0;
    int lw[KLT_LMAX + 1], lh[KLT_LMAX + 1];
    klt_sizes(rows, cols, lw, lh);
    size_t b = 0;
    for (int l = 1; l <= max_level; l++) b += (size_t)lw[l] * (size_t)lh[l];
    return 2 * b;
}

extern "C" int swf_klt_track_batch(int32_t n_pairs, int32_t rows, int32_t cols, const uint8_t* prev_img, const uint8_t* cur_img,
                                   const int32_t* first, const double* prev_px, const double* guess_px,
                                   int32_t win, int32_t max_level, int32_t back_level, int32_t max_count, double eps, double min_eig,
                                   double back_dist, int32_t flags,
                                   double* cur_px, double* back_px, uint8_t* status, int32_t* why, int32_t* keep_idx, int32_t* n_keep,
                                   int32_t* info, int32_t* trace_iters, double* trace_px, uint8_t* pyr, int32_t on_device, void* stream) {
    const std::string who = "swf_klt_track_batch";
    if (n_pairs < 0 || !prev_img || !cur_img || !first || !prev_px || !info) return klt_fail(SWF_E_INVALID, who + ": null argument");
    if (((flags & 2) != 0) != (guess_px != nullptr)) return klt_fail(SWF_E_INVALID, who + ": guess_px goes with flag bit 1, and only with it");
    if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(min_eig) || !(min_eig > 0.0) || !std::isfinite(back_dist) || !(back_dist > 0.0))
        return klt_fail(SWF_E_INVALID, who + ": eps, min_eig and back_dist must be finite and positive");
    if (win < 3 || win > SWF_KLT_WMAX || (win & 1) == 0) return klt_fail(SWF_E_UNSUPPORTED, who + ": the window side must be odd, 3 .. 21");
    if (rows <= win || cols <= win || rows > 8192 || cols > 8192) return klt_fail(SWF_E_UNSUPPORTED, who + ": rows and cols must be above win and at most 8192");
    if (max_level < 0 || max_level > SWF_KLT_LMAX || back_level < 0 || back_level > SWF_KLT_LMAX)
        return klt_fail(SWF_E_UNSUPPORTED, who + ": max_level and back_level outside 0 .. 4");
    if (max_count < 1 || max_count > 1000) return klt_fail(SWF_E_UNSUPPORTED, who + ": max_count outside 1 .. 1000");
    if (flags < 0 || flags > 7) return klt_fail(SWF_E_UNSUPPORTED, who + ": unknown flag bits");
    if (n_pairs > (1 << 20)) return klt_fail(SWF_E_UNSUPPORTED, who + ": more than 2^20 pairs");
    if (on_device && !pyr) return klt_fail(SWF_E_INVALID, who + ": device memory needs the pyramid workspace");
    if (on_device && n_keep && !status && !why && !keep_idx)
        return klt_fail(SWF_E_INVALID, who + ": n_keep in device memory needs one of status, why and keep_idx to hold the flags");
    if (n_pairs == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    KltArgs A{};
    A.n_pairs = n_pairs; A.rows = rows; A.cols = cols; A.win = win; A.max_count = max_count; A.flags = flags;
    A.eps2 = eps * eps; A.min_eig = min_eig; A.back_dist = back_dist;
    klt_sizes(rows, cols, A.lw, A.lh);
    int avail = 0;                                       // building stops before a level whose width or height would be <= win
    while (avail < KLT_LMAX && A.lw[avail + 1] > win && A.lh[avail + 1] > win) avail++;
    const int build = std::max(max_level, back_level);
    A.top_build = std::min(build, avail); A.top_f = std::min(max_level, avail); A.top_b = std::min(back_level, avail);
    size_t off = 0;
    for (int l = 1; l <= KLT_LMAX; l++) { A.loff[l] = off; off += (size_t)A.lw[l] * (size_t)A.lh[l]; }
    A.half_bytes = swf_klt_pyramid_bytes(rows, cols, build) / 2;
    const size_t pair_bytes = 2 * A.half_bytes, img_bytes = (size_t)rows * (size_t)cols;
    const size_t built_bytes = A.top_build ? A.loff[A.top_build] + (size_t)A.lw[A.top_build] * (size_t)A.lh[A.top_build] : 0;
    if (on_device) {            // the offsets are device memory: the kernels make the checks
        A.prev_img = prev_img; A.cur_img = cur_img; A.first = first; A.prev_px = prev_px; A.guess_px = guess_px;
        A.cur_px = cur_px; A.back_px = back_px; A.status = status; A.why = why; A.keep_idx = keep_idx; A.n_keep = n_keep; A.info = info;
        A.trace_iters = trace_iters; A.trace_px = trace_px; A.pyr = pyr;
        A.blocks_per_pair = KLT_BLOCKS_DEVICE;
        return swf_internal_klt_launch(A, st);
    }
    // ---- host memory: the argument errors and the BAD_INPUT pairs before the device is touched
    if (first[0] < 0) return klt_fail(SWF_E_INVALID, who + ": a negative point offset");
    for (int i = 0; i < n_pairs; i++) {
        if (first[i + 1] < first[i]) return klt_fail(SWF_E_INVALID, who + ": point offsets must be non-decreasing");
        if (first[i + 1] - first[i] > SWF_KLT_NMAX) return klt_fail(SWF_E_UNSUPPORTED, who + ": a pair of more than 4096 points");
    }
    const bool as_float = (flags & 1) != 0, back = (flags & 4) != 0;
    auto staged_finite = [&](double v) { return std::isfinite(as_float ? (double)(float)v : v); };
    std::vector<int32_t> code((size_t)n_pairs);
    int n_go = 0, n_max = 0;
    for (int i = 0; i < n_pairs; i++) {
        bool fin = true;
        for (size_t g = (size_t)first[i] * 2; g < (size_t)first[i + 1] * 2; g++) fin = fin && staged_finite(prev_px[g]) && (!guess_px || staged_finite(guess_px[g]));
        code[(size_t)i] = fin ? SWF_KLT_OK : SWF_KLT_BAD_INPUT;
        info[i] = code[(size_t)i];
        if (fin && first[i + 1] > first[i]) { n_go++; n_max = std::max(n_max, first[i + 1] - first[i]); }
    }
    if (!n_go) {                // no pair has a point to track: the device is not touched
        for (int i = 0; i < n_pairs; i++) if (n_keep && code[(size_t)i] == SWF_KLT_OK) n_keep[i] = 0;
        return SWF_OK;
    }
    A.blocks_per_pair = std::min((n_max + KLT_WAVES - 1) / KLT_WAVES, KLT_NMAX / KLT_WAVES);

    const size_t nf = (size_t)n_pairs, np = (size_t)(first[n_pairs] - first[0]), T = KLT_LMAX + 1;
    std::vector<int32_t> rel(first, first + n_pairs + 1);
    for (auto& v : rel) v -= first[0];
    // a pair leaves what it does not write as the caller had it: the results pass through staging arrays
    std::vector<double> h_cur(cur_px ? np * 2 : 0), h_back(back_px && back ? np * 2 : 0), h_tpx(trace_px ? np * 4 * T : 0);
    std::vector<int32_t> h_info(nf), h_why(why ? np : 0), h_k(keep_idx ? np : 0), h_nk(n_keep ? nf : 0), h_tit(trace_iters ? np * 2 * T : 0);
    std::vector<uint8_t> h_st(status ? np : 0), h_pyr(pyr ? nf * pair_bytes : 0);
    HostStage S("swf_klt_track_batch", st);
    A.prev_img = S.up(prev_img, nf * img_bytes);
    A.cur_img = S.up(cur_img, nf * img_bytes);
    A.first = S.up(rel.data(), rel.size());
    A.prev_px = S.up(prev_px + (size_t)first[0] * 2, np * 2);
    if (guess_px) A.guess_px = S.up(guess_px + (size_t)first[0] * 2, np * 2);
    A.info = S.out<int32_t>(nf);
    A.status = S.out<uint8_t>(np);
    A.pyr = S.out<uint8_t>(nf * pair_bytes);
    if (cur_px) A.cur_px = S.out<double>(np * 2);
    if (back_px && back) A.back_px = S.out<double>(np * 2);
    if (why) A.why = S.out<int32_t>(np);
    if (keep_idx) A.keep_idx = S.out<int32_t>(np);
    if (n_keep) A.n_keep = S.out<int32_t>(nf);
    if (trace_iters) A.trace_iters = S.out<int32_t>(np * 2 * T);
    if (trace_px) A.trace_px = S.out<double>(np * 4 * T);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_klt_launch(A, st);
    if (rc) return rc;
    S.down(h_info.data(), A.info, h_info.size());
    S.down(h_st.data(), A.status, h_st.size());
    S.down(h_pyr.data(), A.pyr, h_pyr.size());
    S.down(h_cur.data(), A.cur_px, h_cur.size());
    S.down(h_back.data(), A.back_px, h_back.size());
    S.down(h_why.data(), A.why, h_why.size());
    S.down(h_k.data(), A.keep_idx, h_k.size());
    S.down(h_nk.data(), A.n_keep, h_nk.size());
    S.down(h_tit.data(), A.trace_iters, h_tit.size());
    S.down(h_tpx.data(), A.trace_px, h_tpx.size());
    S.sync();
    if (S.failed()) return S.rc();
    for (int i = 0; i < n_pairs; i++)
        if (h_info[(size_t)i] != code[(size_t)i]) return klt_fail(SWF_E_STATE, who + ": the device classified a pair differently from the host");
    for (int i = 0; i < n_pairs; i++) {
        if (code[(size_t)i] != SWF_KLT_OK) continue;
        const size_t fi = (size_t)i, lo = (size_t)rel[fi], hi = (size_t)rel[fi + 1], at = (size_t)first[i];
        if (cur_px) std::copy(h_cur.begin() + lo * 2, h_cur.begin() + hi * 2, cur_px + at * 2);
        if (back_px && back) std::copy(h_back.begin() + lo * 2, h_back.begin() + hi * 2, back_px + at * 2);
        if (status) std::copy(h_st.begin() + lo, h_st.begin() + hi, status + at);
        if (why) std::copy(h_why.begin() + lo, h_why.begin() + hi, why + at);
        if (keep_idx) std::copy(h_k.begin() + lo, h_k.begin() + hi, keep_idx + at);
        if (n_keep) n_keep[i] = h_nk[fi];
        if (trace_iters) std::copy(h_tit.begin() + lo * 2 * T, h_tit.begin() + hi * 2 * T, trace_iters + at * 2 * T);
        if (trace_px) std::copy(h_tpx.begin() + lo * 4 * T, h_tpx.begin() + hi * 4 * T, trace_px + at * 4 * T);
        if (pyr) for (size_t which = 0; which < 2; which++) {             // the levels that were built, of either image
            const size_t o = fi * pair_bytes + which * A.half_bytes;
            std::copy(h_pyr.begin() + o, h_pyr.begin() + o + built_bytes, pyr + o);
        }
    }
    return SWF_OK;
}
