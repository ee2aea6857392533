// swf_lambda.hip — k_lambda (swf_lambda.h) instantiated for the stand-alone operator swf_lambda_batch and for the batch
// engine's swf_batch_ambiguity_search and swf_batch_ambiguity_search_selected (swf_engine.hip), which share one body.  gfx950 only,
// no CPU path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>
#define SWF_LAMBDA_DEVICE_BODY
#include "swf_lambda.h"
#include "swf_stage.h"

void swf_internal_set_error(const std::string& m);
static int lbd_fail(int code, const std::string& m) { swf_internal_set_error(m); return code; }

int swf_internal_lambda_launch(const LambdaArgs& A, bool batch, hipStream_t st) {
    if (A.n_prob <= 0) return SWF_OK;
    const size_t lds = (size_t)2 * A.ldl * A.ldl * sizeof(double);
    const bool sel = batch && A.pair_count;
    const void* fn = sel ? (const void*)k_lambda<true, true> : batch ? (const void*)k_lambda<true> : (const void*)k_lambda<false>;
    if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return lbd_fail(SWF_E_NODEVICE, "k_lambda: cannot raise the LDS limit");
    if (sel) hipLaunchKernelGGL((k_lambda<true, true>), dim3(A.n_prob), dim3(64), lds, st, A);
    else if (batch) hipLaunchKernelGGL(k_lambda<true>, dim3(A.n_prob), dim3(64), lds, st, A);
    else hipLaunchKernelGGL(k_lambda<false>, dim3(A.n_prob), dim3(64), lds, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lbd_fail(SWF_E_NODEVICE, std::string("k_lambda: ") + hipGetErrorString(e));
    return SWF_OK;
}

// the LDS row stride for problems of up to nmax unknowns: odd (the column walks of the factor are then conflict-free)
static int lbd_ldl(int nmax) { return std::max(1, nmax) | 1; }

// C-ABI, include/swf_solver.h
extern "C" int swf_lambda_batch(int32_t n_problems, int32_t ld, const int32_t* n, const double* a, const double* Q, int32_t m,
                                double* F, double* s, int32_t* info, int32_t on_device, void* stream) {
    if (!n || !a || !Q || !F || !s || !info || n_problems < 0) return lbd_fail(SWF_E_INVALID, "swf_lambda_batch: null argument");
    if (ld < 1 || ld > LBD_NMAX) return lbd_fail(SWF_E_UNSUPPORTED, "swf_lambda_batch: ld must be in [1, 64]");
    if (m < 1 || m > 2) return lbd_fail(SWF_E_UNSUPPORTED, "swf_lambda_batch: m must be 1 or 2");
    if (n_problems == 0) return SWF_OK;
    hipStream_t st = (hipStream_t)stream;
    LambdaArgs A{};
    A.n_prob = n_problems; A.ld = ld; A.m = m;
    if (on_device) {            // the sizes are device memory: the LDS is sized for ld
        A.ldl = lbd_ldl(ld);
        A.n = n; A.a = a; A.Q = Q; A.F = F; A.s = s; A.info = info;
        return swf_internal_lambda_launch(A, false, st);
    }
    int nmax = 1;
    for (int p = 0; p < n_problems; p++) {
        if (n[p] > LBD_NMAX || n[p] > ld) return lbd_fail(SWF_E_UNSUPPORTED, "swf_lambda_batch: n > ld or n > 64");
        nmax = std::max(nmax, (int)n[p]);
    }
    A.ldl = lbd_ldl(nmax);
    const size_t np = (size_t)n_problems;
    HostStage S("swf_lambda_batch", st);
    A.n = S.up(n, np); A.a = S.up(a, np * ld); A.Q = S.up(Q, np * ld * ld);
    A.F = S.out<double>(np * m * ld); A.s = S.out<double>(np * m); A.info = S.out<int32_t>(np);
    if (S.failed()) return S.rc();
    const int rc = swf_internal_lambda_launch(A, false, st);
    if (rc) return rc;
    S.down(F, A.F, np * m * ld);
    S.down(s, A.s, np * m);
    S.down(info, A.info, np);
    S.sync();
    return S.rc();
}

#ifdef SWF_PROFILE_LAMBDA
// the phase stamps of the last k_lambda launch (see swf_lambda.h): out [min(n_problems, LBD_PROF_PROBLEMS)][LBD_PROF_SLOTS]
extern "C" int swf_debug_lambda_stamps(unsigned long long* out, int32_t n_problems) {
    if (!out || n_problems < 0) return SWF_E_INVALID;
    const size_t n = (size_t)std::min<int32_t>(n_problems, LBD_PROF_PROBLEMS) * LBD_PROF_SLOTS;
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lambda_prof), n * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif
