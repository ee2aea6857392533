// swf_phasescreen.hip — k_phase_screen (see swf_phasescreen.h) and the stand-alone operator swf_phase_screen_batch.
// gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "swf_phasescreen.h"
#include "swf_stage.h"
// Floating-point contraction is off in this translation unit, gnss_distance included: every product and sum is rounded as it is
// written, so the two instances of the kernel cannot differ in where a multiply-add was fused.
#pragma clang fp contract(off)
#include "swf_gnss_range.h"

void swf_internal_set_error(const std::string& m);
static int scr_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

namespace {

__device__ __forceinline__ double scr_lane(double v, int k) {       // the value lane k holds (k wave-uniform)
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// v of record idx of the epoch (slot idx / 64, lane idx % 64); 0 for an idx outside the epoch's slots.  Every lane takes part.
template <int SLOTS>
__device__ __forceinline__ int scr_gather(const int (&v)[SLOTS], int idx) {
    int out = 0;
#pragma unroll
    for (int t = 0; t < SLOTS; t++) {
        const int g = __shfl(v[t], idx & 63);
        if ((idx >> 6) == t) out = g;
    }
    return out;
}

// The arithmetic of one record, d = sat[3] L_lam lam el P N dt: the residual of the un-weighted RTKCarrierPhaseFactor at xg and,
// for a rover-only record, |code - phase| sin^2(el).  Without an ambiguity neither N nor dt is used.
__device__ __forceinline__ void scr_record(const double (&d)[SWF_SCR_DOUBLES], const double (&xg)[3], bool masked, bool has, bool spp,
                                           double& r, double& code) {
    r = 0.0; code = 0.0;
    if (has) {
        const double L = masked ? 0.0 : d[3];
        double e[3];
        const double r1 = gnss_distance(xg, d, e);
        r = r1 - d[7] * d[4] - L + d[8];
        if (spp) {
            const double s = sin(d[5]);
            code = fabs((d[3] + d[7] * d[4]) - d[6]) * s * s;
        }
    }
}

template <int SLOTS>
__global__ void __launch_bounds__(64 * SCR_WPB) k_phase_screen(PhaseScreenArgs A) {
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SCR_WPB + (threadIdx.x >> 6)));
    if (e >= A.n_epochs) return;
    // ---------------------------------------------------------------- level 1: the epoch's run of records
    const int f0 = A.first[e], n = A.first[e + 1] - f0;
    if (f0 < 0 || n < 0 || n > 64 * SLOTS) {
        if (lane == 0 && A.n_reset) A.n_reset[e] = -1;
        return;
    }
    // ---------------------------------------------------------------- level 2: records, pose, base, mode
    int4 rc[SLOTS];
    double d[SLOTS][SWF_SCR_DOUBLES];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        rc[s] = make_int4(0, 0, 0, -1);
#pragma unroll
        for (int k = 0; k < SWF_SCR_DOUBLES; k++) d[s][k] = k == 4 ? 1.0 : 0.0;
        if (i < n) {
            const int* q = A.rec + ((size_t)f0 + i) * 4;
            rc[s] = make_int4(q[0], q[1], q[2], q[3]);
            const double* dp = A.dat + ((size_t)f0 + i) * SWF_SCR_DOUBLES;
#pragma unroll
            for (int k = 0; k < SWF_SCR_DOUBLES; k++) d[s][k] = dp[k];
        }
    }
    const double* pp = A.pos + (size_t)e * 3;
    const double* bp = A.base + (size_t)e * 3;
    const double xg[3] = { pp[0] + bp[0], pp[1] + bp[1], pp[2] + bp[2] };
    const int mode = A.mode[e];

    // ---------------------------------------------------------------- what the host rejects for host memory
    int kindv[SLOTS];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        const int kind = rc[s].x, grp = rc[s].y, st = rc[s].z, pt = rc[s].w;
        const double lam = d[s][4];
        kindv[s] = kind;
        if (i < n) {
            bad |= (kind != SWF_SCR_RTK && kind != SWF_SCR_SPP) || grp < 0 || grp >= SWF_SCR_GROUPS || (st & ~(SWF_SCR_HAS_AMB | SWF_SCR_CONTINUING)) != 0;
            bad |= !(lam > 0.0) || !(lam < __builtin_inf());
            if (kind == SWF_SCR_SPP && pt != -1) bad |= pt < 0 || pt >= n || pt == i;
        }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane, pt = rc[s].w;
        const int pk = scr_gather<SLOTS>(kindv, pt);
        if (i < n && rc[s].x == SWF_SCR_SPP && pt >= 0 && pt < n && pk != SWF_SCR_RTK) bad = true;
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0 && A.n_reset) A.n_reset[e] = -1;
        return;
    }

    // ---------------------------------------------------------------- residuals, one lane-slot per record
    double r[SLOTS], code[SLOTS];
    bool masked[SLOTS], elig[SLOTS];
    int set[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        const bool has = (rc[s].z & SWF_SCR_HAS_AMB) != 0, cont = (rc[s].z & SWF_SCR_CONTINUING) != 0;
        masked[s] = d[s][5] < A.el_min;
        scr_record(d[s], xg, masked[s], i < n && has, rc[s].x == SWF_SCR_SPP, r[s], code[s]);
        elig[s] = i < n && has && cont;
        set[s] = rc[s].x * SWF_SCR_GROUPS + rc[s].y;
    }

    // ---------------------------------------------------------------- medians by counting, one (kind, group) at a time
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double mymed[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) mymed[s] = qnan;
    double med_out = qnan;            // lane S keeps the median and the count of set S
    int cnt_out = 0;
    for (int S = 0; S < SCR_SETS; S++) {
        unsigned long long m[SLOTS];
        int c = 0;
#pragma unroll
        for (int t = 0; t < SLOTS; t++) { m[t] = __ballot(elig[t] && set[t] == S); c += __popcll(m[t]); }
        if (c == 0) continue;
        int rk[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; s++) rk[s] = 0;
#pragma unroll
        for (int t = 0; t < SLOTS; t++) {
            unsigned long long mm = m[t];
            while (mm) {                                        // members in ascending record index: a fixed order
                const int j = __builtin_ctzll(mm);
                mm &= mm - 1ull;
                const double rj = scr_lane(r[t], j);
                const int jj = t * 64 + j;
#pragma unroll
                for (int s = 0; s < SLOTS; s++) {
                    const int i = s * 64 + lane;
                    // does member jj sort before record i?  ascending, ties by record index, NaN last
                    const bool before = rj < r[s] || (rj == r[s] && jj < i) || (r[s] != r[s] && (rj == rj || jj < i));
                    rk[s] += before ? 1 : 0;
                }
            }
        }
        double md = qnan;
#pragma unroll
        for (int s = 0; s < SLOTS; s++) {
            const unsigned long long pm = __ballot(((m[s] >> lane) & 1ull) != 0ull && rk[s] == c / 2);
            if (pm) md = scr_lane(r[s], __builtin_ctzll(pm));
        }
#pragma unroll
        for (int s = 0; s < SLOTS; s++) if ((m[s] >> lane) & 1ull) mymed[s] = md;
        if (lane == S) { med_out = md; cnt_out = c; }
    }

    // ---------------------------------------------------------------- decisions, un-masked records only
    bool slipr[SLOTS], slipc[SLOTS];
    int c3[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        const bool rtk = rc[s].x == SWF_SCR_RTK;
        const bool gate = i < n && !masked[s] && elig[s] && (mode & (rtk ? SWF_SCR_GATE_RTK : SWF_SCR_GATE_SPP)) != 0;
        const double lam = d[s][4];
        slipr[s] = gate && fabs(r[s] - mymed[s]) > (rtk ? lam / 2 : lam);          // a NaN comparison sets no bit
        slipc[s] = gate && !rtk && code[s] > 10.0;
        c3[s] = (rtk && slipr[s]) ? 1 : 0;
    }
    unsigned char fl[SLOTS];
    bool nw[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        const bool rtk = rc[s].x == SWF_SCR_RTK;
        const int pc3 = scr_gather<SLOTS>(c3, rc[s].w);
        const bool fresh = !elig[s];                                               // no ambiguity yet, or its slip counter moved on
        nw[s] = i < n && !masked[s] && (fresh || (rtk ? (slipr[s] || (mode & SWF_SCR_RESET_ALL) != 0)
                                                      : ((rc[s].w >= 0 && pc3 != 0) || slipc[s] || slipr[s])));
        fl[s] = masked[s] ? (unsigned char)SWF_SCR_MASKED
                          : (unsigned char)((slipr[s] ? SWF_SCR_SLIP_RESIDUAL : 0) | (slipc[s] ? SWF_SCR_SLIP_CODE : 0) | (nw[s] ? SWF_SCR_NEW_AMB : 0));
    }

    // ---------------------------------------------------------------- outputs; the reset list compacted 64 flags at a time
    int total = 0;
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        const unsigned long long mk = __ballot(nw[s]);
        const int at = total + __popcll(mk & ((1ull << lane) - 1ull));
        if (nw[s] && A.reset) A.reset[(size_t)f0 + at] = i;
        total += __popcll(mk);
        if (i < n) {
            if (A.r) A.r[(size_t)f0 + i] = r[s];
            if (A.flags) A.flags[(size_t)f0 + i] = fl[s];
        }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int i = s * 64 + lane;
        if (i >= total && i < n && A.reset) A.reset[(size_t)f0 + i] = -1;
    }
    if (lane < SCR_SETS) {
        if (A.med) A.med[(size_t)e * SCR_SETS + lane] = med_out;
        if (A.cnt) A.cnt[(size_t)e * SCR_SETS + lane] = cnt_out;
    }
    if (lane == 0 && A.n_reset) A.n_reset[e] = total;
}

}  // namespace

int swf_internal_phase_screen_launch(const PhaseScreenArgs& A, int slots, hipStream_t st) {
    if (A.n_epochs <= 0) return SWF_OK;
    const dim3 grid((unsigned)((A.n_epochs + SCR_WPB - 1) / SCR_WPB)), block(64 * SCR_WPB);
    if (slots == 1) hipLaunchKernelGGL(k_phase_screen<1>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(k_phase_screen<SWF_SCR_NMAX / 64>, grid, block, 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scr_fail(SWF_E_NODEVICE, std::string("k_phase_screen: ") + hipGetErrorString(e));
    return SWF_OK;
}

// C-ABI, include/swf_solver.h
extern "C" int swf_phase_screen_batch(int32_t n_epochs, const int32_t* first, const double* pos, const double* base, const int32_t* mode,
                                      double el_min, const double* dat, const int32_t* rec, double* r, uint8_t* flags, double* med,
                                      int32_t* cnt, int32_t* reset, int32_t* n_reset, int32_t on_device, void* stream) {
    const char* who = "swf_phase_screen_batch";
    if (n_epochs < 0 || !first || !pos || !base || !mode || !dat || !rec) return scr_fail(SWF_E_INVALID, std::string(who) + ": null argument");
    if (!std::isfinite(el_min)) return scr_fail(SWF_E_INVALID, std::string(who) + ": el_min is not finite");
    if (n_epochs == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    PhaseScreenArgs A{};
    A.n_epochs = n_epochs; A.el_min = el_min;
    if (on_device) {            // the sizes are device memory: the general instance runs
        A.first = first; A.pos = pos; A.base = base; A.mode = mode; A.dat = dat; A.rec = rec;
        A.r = r; A.flags = flags; A.med = med; A.cnt = cnt; A.reset = reset; A.n_reset = n_reset;
        return swf_internal_phase_screen_launch(A, SWF_SCR_NMAX / 64, st);
    }
    // ---- host memory: every rejection before the device is touched
    if (first[0] != 0) return scr_fail(SWF_E_INVALID, std::string(who) + ": first[0] != 0");
    int nmax = 0;
    for (int e = 0; e < n_epochs; e++) {
        if (first[e + 1] < first[e]) return scr_fail(SWF_E_INVALID, std::string(who) + ": first decreases");
        nmax = std::max(nmax, (int)(first[e + 1] - first[e]));
    }
    for (int e = 0; e < n_epochs; e++) {
        const int f0 = first[e], n = first[e + 1] - f0;
        for (int i = 0; i < n; i++) {
            const int32_t* q = rec + (size_t)(f0 + i) * 4;
            const double lam = dat[(size_t)(f0 + i) * SWF_SCR_DOUBLES + 4];
            if ((q[0] != SWF_SCR_RTK && q[0] != SWF_SCR_SPP) || q[1] < 0 || q[1] >= SWF_SCR_GROUPS || (q[2] & ~(SWF_SCR_HAS_AMB | SWF_SCR_CONTINUING)) != 0)
                return scr_fail(SWF_E_INVALID, std::string(who) + ": kind, group or state bits out of range");
            if (!std::isfinite(lam) || lam <= 0.0) return scr_fail(SWF_E_INVALID, std::string(who) + ": a wavelength must be finite and positive");
            if (q[0] == SWF_SCR_SPP && q[3] != -1 && (q[3] < 0 || q[3] >= n || q[3] == i || rec[(size_t)(f0 + q[3]) * 4] != SWF_SCR_RTK))
                return scr_fail(SWF_E_INVALID, std::string(who) + ": a partner must be another record of the epoch, of kind RTK");
        }
    }
    if (nmax > SWF_SCR_NMAX) return scr_fail(SWF_E_UNSUPPORTED, std::string(who) + ": more than 256 records in an epoch");

    const size_t ne = (size_t)n_epochs, nr = (size_t)first[n_epochs];
    HostStage S(who, st);
    A.first = S.up(first, ne + 1); A.pos = S.up(pos, ne * 3); A.base = S.up(base, ne * 3); A.mode = S.up(mode, ne);
    A.dat = S.up(dat, nr * SWF_SCR_DOUBLES, SWF_SCR_DOUBLES); A.rec = S.up(rec, nr * 4, 4);
    A.r = S.out<double>(nr); A.flags = S.out<uint8_t>(nr); A.med = S.out<double>(ne * SCR_SETS); A.cnt = S.out<int32_t>(ne * SCR_SETS);
    A.reset = S.out<int32_t>(nr); A.n_reset = S.out<int32_t>(ne);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_phase_screen_launch(A, nmax <= 64 ? 1 : SWF_SCR_NMAX / 64, st);
    if (rc) return rc;
    S.down(r, A.r, nr);
    S.down(flags, A.flags, nr);
    S.down(med, A.med, ne * SCR_SETS);
    S.down(cnt, A.cnt, ne * SCR_SETS);
    S.down(reset, A.reset, nr);
    S.down(n_reset, A.n_reset, ne);
    S.sync();
    return S.rc();
}
