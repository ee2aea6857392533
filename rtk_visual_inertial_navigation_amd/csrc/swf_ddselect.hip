// swf_ddselect.hip — k_dd_select (see swf_ddselect.h), instantiated for the stand-alone operator swf_dd_select_batch and for the
// batch engine's swf_batch_select_ambiguity_pairs (swf_engine.hip), which share one body.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_ddselect.h"
#include "swf_stage.h"
// Floating-point contraction is off in this translation unit: the kernel has no product, and every sum is rounded as it is written.
#pragma clang fp contract(off)

void swf_internal_set_error(const std::string& m);
static int dds_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

// C round(): halves away from zero.  x - trunc(x) is exact.
__device__ __forceinline__ double dds_round(double x) {
    double r = trunc(x);
    if (fabs(x - r) >= 0.5) r += copysign(1.0, x);
    return r;
}
__device__ __forceinline__ double dds_frac(double d) { return fabs(d - dds_round(d)); }

__device__ __forceinline__ double dds_shfl_xor(double v, int m) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(unsigned)(b & 0xffffffffll), m), hi = __shfl_xor((int)(unsigned)((unsigned long long)b >> 32), m);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

template <bool BATCH>
__global__ void __launch_bounds__(64) k_dd_select(DdSelectArgs A) {
    __shared__ double s_y[DDS_NMAX];
    __shared__ int s_t[DDS_NMAX];
    __shared__ int s_x[DDS_NMAX];                       // BATCH: the state index of the record's ambiguity
    __shared__ unsigned char s_key[DDS_NMAX];           // class, + 8 when the ambiguity is used (no candidate)
    __shared__ unsigned s_used[DDS_TMAX / 32];
    __shared__ int s_ref[8];
    const int w = blockIdx.x, lane = threadIdx.x;
    const double inf = __builtin_inf();

    // ---------------------------------------------------------------- level 1: the window's runs, then its epochs' runs
    const int e0 = A.epoch_first[w], e1 = A.epoch_first[w + 1];
    const int tail = BATCH ? A.tail[w] : A.y_first[w + 1] - A.y_first[w];
    const double* yw = BATCH ? A.x : A.y + A.y_first[w];
    const double gate = A.gate[w];
    // what the host rejects for host memory (a coordinate twice within an epoch excepted: the kernel does not look for it)
    bool bad = !(gate > 0.0) || !(gate < inf) || e0 < 0 || e1 < e0 || tail < 0 || tail > DDS_TMAX;
    if (!bad) for (int e = e0 + lane; e < e1; e += 64) {
        const int f = A.obs_first[e], n = A.obs_first[e + 1] - f;
        bad |= f < 0 || n < 0 || n > DDS_NMAX;
    }
    bad = __ballot(bad) != 0ull;
    bool nonfinite = false;
    int ob = 0, oe = 0;
    if (!bad) {
        ob = A.obs_first[e0]; oe = A.obs_first[e1];
        for (int i = ob + lane; i < oe; i += 64) {
            const int c = A.obs[2 * (size_t)i], t = A.obs[2 * (size_t)i + 1];
            if (c < 0 || c >= DDS_CLASSES || t < 0 || t >= tail) bad = true;
            else { const double yv = yw[BATCH ? A.xidx[i] : t]; nonfinite |= !(fabs(yv) < inf); }
        }
        bad = __ballot(bad) != 0ull;
    }
    if (bad) {                                          // device-resident inputs the host could not check: info = -1, nothing else
        if (lane < 4 && A.counts) A.counts[(size_t)w * 4 + lane] = lane == 3 ? -1 : 0;
        if (BATCH && lane == 0) { A.pair_count[w] = 0; A.am_first[w] = w * SWF_LAMBDA_NMAX; if (w == A.n_windows - 1) A.am_first[w + 1] = (w + 1) * SWF_LAMBDA_NMAX; }
        return;
    }
    if (__ballot(nonfinite) != 0ull) {                  // the reference would sort NaNs: nothing is reported
        if (A.pairs) { A.pairs[((size_t)w * SWF_LAMBDA_NMAX + lane) * 2] = -1; A.pairs[((size_t)w * SWF_LAMBDA_NMAX + lane) * 2 + 1] = -1; }
        if (lane < 4 && A.counts) A.counts[(size_t)w * 4 + lane] = lane == 3 ? SWF_DDSEL_NONFINITE : 0;
        if (A.refs) for (int i = e0 * DDS_CLASSES + lane; i < e1 * DDS_CLASSES; i += 64) A.refs[i] = -1;
        for (int i = ob + lane; i < oe; i += 64) { if (A.cost) A.cost[i] = -1.0; if (A.role) A.role[i] = SWF_DDSEL_SKIPPED; }
        if (BATCH && lane == 0) { A.pair_count[w] = 0; A.am_first[w] = w * SWF_LAMBDA_NMAX; if (w == A.n_windows - 1) A.am_first[w + 1] = (w + 1) * SWF_LAMBDA_NMAX; }
        return;
    }

    for (int i = lane; i < DDS_TMAX / 32; i += 64) s_used[i] = 0u;
    int npairs = 0, last_count = 0, last_ref = 0;
    for (int e = e0; e < e1; e++) {
        const int f = A.obs_first[e], n = A.obs_first[e + 1] - f;
        __syncthreads();                                // the previous epoch's marks are in place and its records have been read
        // ------------------------------------------------------------ level 2: the epoch's records
        for (int i = lane; i < n; i += 64) {
            const int c = A.obs[2 * ((size_t)f + i)], t = A.obs[2 * ((size_t)f + i) + 1];
            int xi = t;
            if (BATCH) { xi = A.xidx[f + i]; s_x[i] = xi; }
            s_t[i] = t;
            s_y[i] = yw[xi];
            s_key[i] = (unsigned char)(c + (((s_used[t >> 5] >> (t & 31)) & 1u) ? 8 : 0));
        }
        __syncthreads();
        // ------------------------------------------------------------ costs: lane j sums over the candidates of its class, in order
        double cj[DDS_NMAX / 64];
#pragma unroll
        for (int s = 0; s < DDS_NMAX / 64; s++) {
            cj[s] = -1.0;
            if (s * 64 < n) {
                const int j = s * 64 + lane;
                const int kj = j < n ? s_key[j] : 255;  // a used record's key matches no candidate's (bit 3), nor does 255
                const double yj = j < n ? s_y[j] : 0.0;
                double acc = 0.0;
                for (int i = 0; i < n; i++) if (s_key[i] == kj) acc += dds_frac(s_y[i] - yj);
                if (kj < DDS_CLASSES) cj[s] = acc;
            }
        }
        // ------------------------------------------------------------ election: cost ascending, index descending
        int nref = 0;
        for (int c = 0; c < DDS_CLASSES; c++) {
            double bc = inf;
            int bi = -1;
#pragma unroll
            for (int s = 0; s < DDS_NMAX / 64; s++) {
                const int j = s * 64 + lane;
                if (j < n && s_key[j] == c && (bi < 0 || cj[s] <= bc)) { bc = cj[s]; bi = j; }
            }
            for (int m = 32; m > 0; m >>= 1) {
                const double oc = dds_shfl_xor(bc, m);
                const int oi = __shfl_xor(bi, m);
                if (oi >= 0 && (bi < 0 || oc < bc || (oc == bc && oi > bi))) { bc = oc; bi = oi; }
            }
            bi = __builtin_amdgcn_readfirstlane(bi);
            if (lane == 0) s_ref[c] = bi;
            nref += bi >= 0 ? 1 : 0;
        }
        if (e == e0) last_ref = nref;
        __syncthreads();
        if (lane < DDS_CLASSES && A.refs) A.refs[(size_t)e * DDS_CLASSES + lane] = s_ref[lane];
        // ------------------------------------------------------------ pairs, in observation order, 64 records at a time
#pragma unroll
        for (int s = 0; s < DDS_NMAX / 64; s++) {
            if (s * 64 >= n) break;
            const int k = s * 64 + lane;
            int rl = SWF_DDSEL_SKIPPED, r = -1;
            bool pr = false;
            if (k < n) {
                const int key = s_key[k];
                r = s_ref[key & 7];
                if (r < 0) rl = SWF_DDSEL_NO_REFERENCE;
                else if (key & 8) rl = SWF_DDSEL_SKIPPED;
                else if (k == r) rl = SWF_DDSEL_REFERENCE;
                else {
                    const int t = s_t[k];
                    atomicOr(&s_used[t >> 5], 1u << (t & 31));            // marked before the gate
                    pr = dds_frac(s_y[k] - s_y[r]) < gate;
                    rl = pr ? SWF_DDSEL_PAIRED : SWF_DDSEL_GATED_OUT;
                }
            }
            const unsigned long long mk = __ballot(pr);
            const int at = npairs + __popcll(mk & ((1ull << lane) - 1ull));
            if (pr && at < SWF_LAMBDA_NMAX) {
                const size_t q = (size_t)w * SWF_LAMBDA_NMAX + at;
                if (A.pairs) { A.pairs[q * 2] = s_t[k]; A.pairs[q * 2 + 1] = s_t[r]; }
                if (BATCH) A.am_pairs[q] = make_int4(s_t[k], s_t[r], s_x[k], s_x[r]);
            }
            const int np = __popcll(mk);
            npairs += np;
            if (e == e0) last_count += np;
            if (k < n) {
                if (A.cost) A.cost[(size_t)f + k] = cj[s];
                if (A.role) A.role[(size_t)f + k] = (unsigned char)rl;
            }
        }
    }
    // ---------------------------------------------------------------- the window's counts; unused pair slots read -1
    const int info = npairs > SWF_LAMBDA_NMAX ? SWF_DDSEL_OVERFLOW
                   : (tail >= 6 && last_count + last_ref >= 6 && last_count >= 4 && npairs >= 4) ? SWF_DDSEL_OK : SWF_DDSEL_TOO_FEW;
    const int nrep = info == SWF_DDSEL_OVERFLOW ? 0 : npairs;
    __syncthreads();                                    // the pair stores above are complete before a slot is overwritten
    if (A.pairs && lane >= nrep) { A.pairs[((size_t)w * SWF_LAMBDA_NMAX + lane) * 2] = -1; A.pairs[((size_t)w * SWF_LAMBDA_NMAX + lane) * 2 + 1] = -1; }
    if (lane < 4 && A.counts) A.counts[(size_t)w * 4 + lane] = lane == 0 ? nrep : lane == 1 ? last_count : lane == 2 ? last_ref : info;
    if (BATCH && lane == 0) {
        A.pair_count[w] = info == SWF_DDSEL_OK ? npairs : 0;
        A.am_first[w] = w * SWF_LAMBDA_NMAX;
        if (w == A.n_windows - 1) A.am_first[w + 1] = (w + 1) * SWF_LAMBDA_NMAX;
    }
}

}  // namespace

int swf_internal_dd_select_launch(const DdSelectArgs& A, bool batch, hipStream_t st) {
    if (A.n_windows <= 0) return SWF_OK;
    if (batch) hipLaunchKernelGGL(k_dd_select<true>, dim3((unsigned)A.n_windows), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_dd_select<false>, dim3((unsigned)A.n_windows), dim3(64), 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dds_fail(SWF_E_NODEVICE, std::string("k_dd_select: ") + hipGetErrorString(e));
    return SWF_OK;
}

int swf_internal_dd_select_check(const char* who_, int n_windows, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs,
                                 const int32_t* tail, const double* gate) {
    const std::string who(who_);
    if (epoch_first[0] != 0) return dds_fail(SWF_E_INVALID, who + ": epoch_first[0] != 0");
    for (int w = 0; w < n_windows; w++) {
        if (epoch_first[w + 1] < epoch_first[w]) return dds_fail(SWF_E_INVALID, who + ": epoch_first decreases");
        if (!std::isfinite(gate[w]) || !(gate[w] > 0.0)) return dds_fail(SWF_E_INVALID, who + ": a gate must be finite and positive (window " + std::to_string(w) + ")");
        if (tail[w] < 0) return dds_fail(SWF_E_INVALID, who + ": a negative tail dimension (window " + std::to_string(w) + ")");
    }
    const int ne = epoch_first[n_windows];
    if (obs_first[0] != 0) return dds_fail(SWF_E_INVALID, who + ": obs_first[0] != 0");
    for (int e = 0; e < ne; e++) if (obs_first[e + 1] < obs_first[e]) return dds_fail(SWF_E_INVALID, who + ": obs_first decreases");
    if (obs_first[ne] > 0 && !obs) return dds_fail(SWF_E_INVALID, who + ": null obs");
    int nmax = 0, tmax = 0;
    std::vector<int> seen;                              // per tail coordinate: 1 + the last epoch that named it
    for (int w = 0; w < n_windows; w++) {
        seen.assign((size_t)tail[w], 0);
        tmax = std::max(tmax, (int)tail[w]);
        for (int e = epoch_first[w]; e < epoch_first[w + 1]; e++) {
            nmax = std::max(nmax, (int)(obs_first[e + 1] - obs_first[e]));
            for (int i = obs_first[e]; i < obs_first[e + 1]; i++) {
                const int c = obs[2 * (size_t)i], t = obs[2 * (size_t)i + 1];
                if (c < 0 || c >= DDS_CLASSES) return dds_fail(SWF_E_INVALID, who + ": a class outside 0..5 (window " + std::to_string(w) + ")");
                if (t < 0 || t >= tail[w]) return dds_fail(SWF_E_INVALID, who + ": a coordinate outside the tail (window " + std::to_string(w) + ")");
                if (seen[(size_t)t] == e + 1) return dds_fail(SWF_E_INVALID, who + ": one coordinate twice within an epoch (window " + std::to_string(w) + ")");
                seen[(size_t)t] = e + 1;
            }
        }
    }
    if (nmax > DDS_NMAX) return dds_fail(SWF_E_UNSUPPORTED, who + ": more than 256 observations in an epoch");
    if (tmax > DDS_TMAX) return dds_fail(SWF_E_UNSUPPORTED, who + ": a tail of more than 2048 coordinates");
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_dd_select_batch(int32_t n_windows, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs,
                                   const int32_t* y_first, const double* y, const double* gate, int32_t* pairs, int32_t* counts,
                                   int32_t* refs, double* cost, uint8_t* role, int32_t on_device, void* stream) {
    const char* who = "swf_dd_select_batch";
    if (n_windows < 0 || !epoch_first || !obs_first || !y_first || !y || !gate) return dds_fail(SWF_E_INVALID, std::string(who) + ": null argument");
    if (n_windows == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    DdSelectArgs A{};
    A.n_windows = n_windows;
    if (on_device) {            // the sizes are device memory: the kernel makes the checks
        if (!obs) return dds_fail(SWF_E_INVALID, std::string(who) + ": null argument");
        A.epoch_first = epoch_first; A.obs_first = obs_first; A.obs = obs; A.y_first = y_first; A.y = y; A.gate = gate;
        A.pairs = pairs; A.counts = counts; A.refs = refs; A.cost = cost; A.role = role;
        return swf_internal_dd_select_launch(A, false, st);
    }
    // ---- host memory: every rejection before the device is touched
    if (y_first[0] != 0) return dds_fail(SWF_E_INVALID, std::string(who) + ": y_first[0] != 0");
    std::vector<int32_t> tail((size_t)n_windows);
    for (int w = 0; w < n_windows; w++) {
        if (y_first[w + 1] < y_first[w]) return dds_fail(SWF_E_INVALID, std::string(who) + ": y_first decreases");
        tail[(size_t)w] = y_first[w + 1] - y_first[w];
    }
    const int chk = swf_internal_dd_select_check(who, n_windows, epoch_first, obs_first, obs, tail.data(), gate);
    if (chk) return chk;

    const size_t nw = (size_t)n_windows, ne = (size_t)epoch_first[n_windows], no = (size_t)obs_first[ne], ny = (size_t)y_first[n_windows];
    HostStage S(who, st);
    A.epoch_first = S.up(epoch_first, nw + 1); A.obs_first = S.up(obs_first, ne + 1); A.obs = S.up(obs, no * 2, 2);
    A.y_first = S.up(y_first, nw + 1); A.y = S.up(y, ny, 1); A.gate = S.up(gate, nw);
    A.pairs = S.out<int32_t>(nw * SWF_LAMBDA_NMAX * 2); A.counts = S.out<int32_t>(nw * 4); A.refs = S.out<int32_t>(ne * DDS_CLASSES, DDS_CLASSES);
    A.cost = S.out<double>(no); A.role = S.out<uint8_t>(no);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_dd_select_launch(A, false, st);
    if (rc) return rc;
    S.down(pairs, A.pairs, nw * SWF_LAMBDA_NMAX * 2);
    S.down(counts, A.counts, nw * 4);
    S.down(refs, A.refs, ne * DDS_CLASSES);
    S.down(cost, A.cost, no);
    S.down(role, A.role, no);
    S.sync();
    return S.rc();
}
