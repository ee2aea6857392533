// swf_engine.hip — host side of the batch engine + the swf_batch_* C-ABI (include/swf_solver.h).
//
// Symbolic phase: flat windows -> index arrays (DevBatch), once per structure: swf_plan.cpp, host-only; uploaded here.
// Numeric phase: a fixed launch sequence per solve, no host synchronisation inside.
// gfx950 only; there is no CPU path: without a HIP device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <memory>
#include <thread>
#include <vector>
#include "../../include/swf_solver.h"
#include "swf_kernels2.h"
#include "swf_kernels3.h"
#include "swf_kernels4.h"
#include "swf_lambda.h"
#include "swf_ddselect.h"
#include "swf_features.h"
#include "swf_fixprior.h"
#include "swf_plan.h"

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(SWF_E_NODEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" const char* swf_last_error(void) { return g_err.c_str(); }
void swf_internal_set_error(const std::string& m) { g_err = m; }
extern "C" int swf_version(void) { return 113; }
extern "C" int swf_abi_sizes(int32_t out[5]) {
    if (!out) return fail(SWF_E_INVALID, "swf_abi_sizes: null");
    out[0] = (int32_t)sizeof(swf_options); out[1] = (int32_t)sizeof(swf_summary); out[2] = (int32_t)sizeof(swf_timing);
    out[3] = (int32_t)sizeof(swf_flat_window); out[4] = (int32_t)sizeof(swf_iteration);
    return SWF_OK;
}
extern "C" int swf_device_count(int32_t* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(SWF_E_NODEVICE, hipGetErrorString(e)); }
    *n = c;
    return SWF_OK;
}
extern "C" int swf_set_device(int32_t d) { HIPCHK(hipSetDevice(d)); return SWF_OK; }
extern "C" void swf_default_options(swf_options* o) {
    if (!o) return;
    *o = swf_options{};
    o->max_num_iterations = 8; o->step_mode = SWF_OPTIMIZE; o->num_threads = 1; o->trust_region_strategy = SWF_DOGLEG; o->jacobi_scaling = 0;
    o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->min_mu = 1e-8; o->max_mu = 1.0; o->mu_increase_factor = 10.0; o->min_diagonal = 1e-6; o->max_diagonal = 1e32;
}

// ------------------------------------------------------------------ device buffer helper
// Every buffer of a batch is carved out of a few slabs (bump allocation, 256-byte aligned): buffers with initial data share
// "data" slabs that are mirrored in one host staging area and reach the device in ONE copy per slab (flush); zero-initialised
// buffers share "zero" slabs that get one memset each.  Released slabs go to a process-wide cache instead of hipFree: the
// ceres::Problem surface rebuilds its batch at every structure change (the estimator adds and removes landmarks every frame,
// R/swf/swf_image.cpp:65-114), and ~100 hipMalloc + hipMemcpy + hipMemset calls per rebuild were most of that path's cost.
// After flush() the pool is sealed: later allocations (the marginalisation consumer's outputs) are initialised on the spot.
#include <mutex>
namespace {
struct SlabCache {
    std::mutex mu; std::vector<std::pair<void*, size_t>> free_; size_t held = 0;
    void* acquire(size_t& bytes) {
        {
            std::lock_guard<std::mutex> g(mu);
            int best = -1;
            for (int i = 0; i < (int)free_.size(); i++)
                if (free_[i].second >= bytes && free_[i].second <= 4 * bytes && (best < 0 || free_[i].second < free_[best].second)) best = i;
            if (best >= 0) { void* p = free_[best].first; bytes = free_[best].second; held -= bytes; free_.erase(free_.begin() + best); return p; }
        }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            trim(0);                                       // give the cache back and try once more
            if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        }
        return p;
    }
    void give(void* p, size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        if (held + bytes > (size_t)2 << 30 || free_.size() >= 32) { (void)hipFree(p); return; }
        free_.push_back({ p, bytes }); held += bytes;
    }
    void trim(size_t keep) {
        std::lock_guard<std::mutex> g(mu);
        while (held > keep && !free_.empty()) { held -= free_.back().second; (void)hipFree(free_.back().first); free_.pop_back(); }
    }
};
// never destroyed: a ceres::Problem with static storage duration may release its batch after this file's statics are gone.
// One cache per device (a slab, a stream or an event belongs to the device it was created on): the CURRENT device's; every
// swf_batch_* entry point runs under the batch's device (DeviceGuard).
constexpr int SWF_MAX_DEVICES = 32;
int current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= SWF_MAX_DEVICES) d = 0; return d; }
SlabCache& slab_cache() { static SlabCache* c = new SlabCache[SWF_MAX_DEVICES]; return c[current_device()]; }
}  // namespace

// streams and events are as expensive to create and destroy as device memory (milliseconds for a non-blocking stream): the
// auxiliary stream + fork / join events of the latency path, and the timing events, are recycled the same way
namespace {
struct HandleCache {
    std::mutex mu; std::vector<hipStream_t> streams; std::vector<hipEvent_t> sync_events, timing_events;
    hipStream_t stream() {
        { std::lock_guard<std::mutex> g(mu); if (!streams.empty()) { hipStream_t s_ = streams.back(); streams.pop_back(); return s_; } }
        hipStream_t s_ = nullptr;
        return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking) == hipSuccess ? s_ : nullptr;
    }
    hipEvent_t event(bool timing) {
        {
            std::lock_guard<std::mutex> g(mu);
            auto& v = timing ? timing_events : sync_events;
            if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; }
        }
        hipEvent_t e = nullptr;
        hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        return rc == hipSuccess ? e : nullptr;
    }
    void give(hipStream_t s_) { if (!s_) return; std::lock_guard<std::mutex> g(mu); if (streams.size() < 16) streams.push_back(s_); else (void)hipStreamDestroy(s_); }
    void give(hipEvent_t e, bool timing) {
        if (!e) return;
        std::lock_guard<std::mutex> g(mu);
        auto& v = timing ? timing_events : sync_events;
        if (v.size() < 4096) v.push_back(e); else (void)hipEventDestroy(e);
    }
};
HandleCache& handle_cache() { static HandleCache* c = new HandleCache[SWF_MAX_DEVICES]; return c[current_device()]; }
// makes a batch's device the current one for the duration of an entry point (several batches on several GPUs may be driven from
// one host thread: swf_solve_batches)
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
}  // namespace

struct DevPool {
    struct Slab { char* dev = nullptr; size_t cap = 0, used = 0, flushed = 0; std::vector<char> host; };
    std::vector<Slab> data, zero;
    bool sealed = false;
    void* bump(std::vector<Slab>& v, size_t bytes, bool mirrored, size_t first) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (v.empty() || v.back().used + bytes > v.back().cap) {
            size_t want = std::max(bytes, v.empty() ? first : std::min<size_t>(2 * v.back().cap, (size_t)256 << 20));
            Slab sl;
            sl.dev = (char*)slab_cache().acquire(want);
            if (!sl.dev) return nullptr;
            sl.cap = want;
            if (mirrored) sl.host.assign(want, 0);
            v.push_back(std::move(sl));
        }
        Slab& sl = v.back();
        void* p = sl.dev + sl.used;
        sl.used += bytes;
        return p;
    }
    template <class T> int put(const std::vector<T>& h, const T** out, size_t min_elems = 1) {
        size_t n = std::max(h.size(), min_elems), bytes = n * sizeof(T);
        void* p = bump(data, bytes, true, (size_t)4 << 20);
        if (!p) return -1;
        Slab& sl = data.back();
        char* m = sl.host.data() + ((char*)p - sl.dev);
        if (!h.empty()) memcpy(m, h.data(), h.size() * sizeof(T));
        if (sealed) {                                      // late allocation: initialise now
            if (hipMemcpy(p, m, (bytes + 255) & ~(size_t)255, hipMemcpyHostToDevice) != hipSuccess) return -1;
            sl.flushed = sl.used;
        }
        *out = (const T*)p;
        return 0;
    }
    template <class T> int zeros(size_t n, T** out) {
        n = std::max<size_t>(n, 1);
        void* p = bump(zero, n * sizeof(T), false, (size_t)16 << 20);
        if (!p) return -1;
        if (sealed) { if (hipMemset(p, 0, n * sizeof(T)) != hipSuccess) return -1; zero.back().flushed = zero.back().used; }
        *out = (T*)p;
        return 0;
    }
    // one host-to-device copy per data slab, one memset per zero slab
    int flush() {
        for (Slab& sl : data) if (sl.used > sl.flushed) { if (hipMemcpy(sl.dev + sl.flushed, sl.host.data() + sl.flushed, sl.used - sl.flushed, hipMemcpyHostToDevice) != hipSuccess) return -1; sl.flushed = sl.used; }
        for (Slab& sl : zero) if (sl.used > sl.flushed) { if (hipMemset(sl.dev + sl.flushed, 0, sl.used - sl.flushed) != hipSuccess) return -1; sl.flushed = sl.used; }
        sealed = true;
        return 0;
    }
    void release() {
        for (Slab& sl : data) slab_cache().give(sl.dev, sl.cap);
        for (Slab& sl : zero) slab_cache().give(sl.dev, sl.cap);
        data.clear(); zero.clear(); sealed = false;
    }
};

struct swf_batch {
    int device = 0;                    // the HIP device the batch lives on (current at swf_batch_create)
    DevBatch D{};
    DevPool pool;
    hipStream_t stream = nullptr;
    std::vector<WinRec> win;
    std::vector<HostWin> hw;
    int max_tiles = 0, max_prior_dim = 0, max_red = 0, min_red = 1 << 30, n_cu = 256;
    bool clc_imu[5] = { false, false, false, false, false };
    // composite IMU-GNSS factors of the batch (swf_kernels4.h): operator arguments, solver-side bookkeeping, initial hidden epochs
    CompArgs CA{}; CompMeta CM{}; int n_comp = 0, comp_nmax = 0, comp_nmin = 1 << 30; long long comp_ne = 0;
    bool comp_eigen_root = false;                      // swf_options::composite_root == SWF_ROOT_EIGEN in the current solve: the composite factors expose the reference's eigen square root
    void* h_sum = nullptr; size_t h_sum_bytes = 0;       // page-locked staging of the per-window states and traces (swf_batch_summaries)
    double* h_x = nullptr;                // page-locked staging of the parameter blocks (state upload / download: one DMA instead of a pageable copy)
    double* co_pose0 = nullptr; double* co_sb0 = nullptr;    // clique class holds IMU factors (its elimination must follow k_eval_imu)
    // marginalisation consumer outputs (allocated at the first swf_batch_marginalize)
    int* mg_tail = nullptr; double* mg_A = nullptr; double* mg_b = nullptr; double* mg_J = nullptr; double* mg_r0 = nullptr; double* mg_w = nullptr; int* mg_rank = nullptr; double* mg_M = nullptr;
    bool mg_valid = false; int mg_ld = 0;
    // host mirror of the consumer's outputs, filled by the first swf_batch_get_prior after a swf_batch_marginalize of a many-window batch
    // (one copy per array instead of six small ones per window: 576 GNSS-epoch priors took 46 ms of hipMemcpy latency)
    bool mg_host = false; std::vector<double> h_mgA, h_mgJ, h_mgb, h_mgr0, h_mgw; std::vector<int> h_mgrank;
    double* mg_resM = nullptr; double* mg_resb = nullptr; int* mg_resok = nullptr;      // k_marg_rescue outputs (rank-deficient tails)
    int* mg_rot = nullptr; int* mg_bjok = nullptr; unsigned long long* mg_crit = nullptr;                                       // k_marg_bj: rotations per sweep, windows taking part
    // ambiguity covariance hand-off outputs (allocated at the first swf_batch_tail_covariance)
    int* tc_tail = nullptr; double* tc_A = nullptr; double* tc_Q = nullptr; double* tc_X = nullptr; int* tc_rank = nullptr; bool tc_valid = false; int tc_ld = 0;
    // integer ambiguity search (allocated at the first swf_batch_ambiguity_search for n_windows x 64 pairs, the most a search may pass):
    // the pair table and one record of results per window (LBD_REC_*, stride am_rec_ld), mirrored to the host by the first getter
    int* am_first = nullptr; int4* am_pairs = nullptr; double* am_rec = nullptr; int am_rec_ld = 0;
    bool am_valid = false, am_host = false; std::vector<double> h_am;
    std::vector<int> am_nb;                             // pairs per window of the last search
    std::vector<int> am_h_first; std::vector<int4> am_h_pairs;      // host staging of the pair upload (outlives the asynchronous copy)
    // double-difference pair selection (swf_ddselect.h).  Per-window outputs from the pool at the first selection; the inputs and the
    // per-epoch / per-observation outputs, whose sizes change from call to call, in two buffers that grow on demand.  dd_h_in stages
    // the upload (gate | epoch_first | obs_first | obs | state index) and keeps the prefix arrays for the getter.
    int* dd_pairs = nullptr; int* dd_counts = nullptr; int* dd_npair = nullptr;
    char* dd_in = nullptr; char* dd_out = nullptr; size_t dd_in_cap = 0, dd_out_cap = 0; int dd_ne = 0, dd_no = 0;
    std::vector<char> dd_h_in, dd_h_out; std::vector<int> dd_h_pairs, dd_h_counts;
    bool dd_valid = false, dd_host = false;
    const int* dd_tail = nullptr;                       // the tail dimensions on the device, when no tail covariance has put them there
    bool am_selected = false, am_sel_host = false;      // the last search ran on the selection; am_h_pairs / am_h_first / am_nb have been read back
    // fix and hold (swf_fixprior.h; allocated at the first swf_batch_fix_prior for the batch's largest linear prior): per-window table,
    // tail-coordinate -> prior-column table, result slabs of fx_ldn^2 / fx_ldn / fx_ldx doubles per window, mirrored to the host by the first getter
    FixWin* fx_win = nullptr; int* fx_tailcol = nullptr; double* fx_A = nullptr; double* fx_b = nullptr; double* fx_J = nullptr; double* fx_r0 = nullptr;
    double* fx_eig = nullptr; double* fx_x0 = nullptr; int* fx_rank = nullptr; int* fx_applied = nullptr; int fx_ldn = 0, fx_ldx = 0;
    bool fx_valid = false, fx_host = false; FixPriorArgs fx_args{};
    std::vector<FixWin> fx_h_win; std::vector<int> fx_h_tailcol, fx_sel;
    std::vector<double> h_fxA, h_fxb, h_fxJ, h_fxr0, h_fxeig, h_fxx0; std::vector<int> h_fxrank, h_fxapplied;
    // post-solve feature check (swf_features.h): the observation table and the output buffer are allocated at the first
    // swf_batch_check_features; fc_out = mean_err | depth | n_obs | rejected | n_rejected | flags, mirrored to the host by the first getter
    bool fc_built = false, fc_valid = false, fc_host = false; FeatArgs fc{}; char* fc_out = nullptr; size_t fc_bytes = 0; int fc_nfeat = 0;
    std::vector<int> fc_feat0; std::vector<char> h_fc;
    // latency path (small batches): an auxiliary stream runs the IMU / clique branch of a linearisation next to the
    // projection / landmark branch; three reusable events carry the dependencies
    hipStream_t aux = nullptr; hipEvent_t ev_fork[3] = { nullptr, nullptr, nullptr };
    ~swf_batch() {
        if (aux) { (void)hipStreamSynchronize(aux); handle_cache().give(aux); }
        for (auto& e : ev_fork) handle_cache().give(e, false);
    }
    WinState* ws_primary = nullptr; WinState* ws_alt = nullptr; WinState* ws_alt2 = nullptr;      // the per-window solver states and the two further buffers the latency path's fused kernels rotate through (k_step_eval, k_decide_lm_clique)
    bool no_decide_fuse = false;          // SWF_NO_DECIDE_FUSE=1: k_decide as its own launch on the latency path too (parity: bit-identical)
    bool no_step_fuse = false;            // SWF_NO_STEP_FUSE=1: k_dogleg and the candidate's evaluation as two launches on the latency path too (parity: bit-identical)
    int n_pch_split = 0;                  // row chunks of priors evaluated by several workgroups (dimension > PRIOR_SPLIT_DIM) with a static clique: k_prior_graw is launched
    bool no_spec = false;                 // SWF_NO_SPEC_EVAL=1: the dogleg loop with a cost pass at the candidate and a Jacobian pass behind k_decide (parity: bit-identical to the speculative flow)
    bool no_comp_fuse = false;            // SWF_NO_COMP_FUSE=1: the composite chain and the visual branch as launches of their own on the latency path too (A/B, parity)
    bool lat_fuse = false;                // latency path: fused grids on one stream (see swf_batch_create)
    bool rr4_has15 = false, rr4_has16 = false;      // some window has 224 < n_red <= 240 / 240 < n_red <= 256: the 15- / 16-column instance of k_chol_rr4 is launched as well
    int rr_nmax = 256;                    // largest reduced system of the register-resident Cholesky (k_chol_rr4)
    bool L_full = false;                  // the L buffer holds the whole factor of the last linear solve
    int asm_programs = 0;                 // distinct assembly programs of the batch (windows of identical structure share one)
    int ls_qpb = 1, ls_var = 0, ls_kms = 8; bool ls_folded = false, s_direct = false;     // k_lm_schur launch shape, fixed at creation (the pair lists depend on it)
    bool full_final = false;              // SWF_FULL_FINAL_ELIM=1: the solve's final linearisation runs the complete group-0 elimination, as every other one does (parity: bit-identical to the gradient-only pass)
    bool no_clq_pack = false;             // SWF_NO_CLIQUE_PACK=1: class 0 as one wavefront per clique (k_clique_elim<48,32,1,0>) instead of two cliques per wavefront (k_clique_pack) (parity, A/B: bit-identical)
    bool no_clq_mfma = false;             // SWF_NO_CLIQUE_MFMA=1: class 1 of the batch path as k_clique_elim<32,48,9,1> (VALU products) instead of k_clique_mm (matrix cores) (parity, A/B: bit-identical)
    int clp_rows = 1, clp_ld = 3;         // k_clique_pack: rows and leading dimension of its LDS Jacobians (the largest class-0 clique of the batch)
    int ls_gqpb = 4;                      // landmark parts per workgroup of the gradient-only landmark pass (it has no ring to fill: chosen for occupancy, not by ls_qpb)
    int timing = 0;                       // bitmask of SWF_K_* brackets
    swf_timing last{};
    std::vector<hipEvent_t> ev;           // event pool (pairs)
    std::vector<int> ev_kind;             // kernel id per recorded pair
    int ev_used = 0;
    int64_t jac_bytes = 0, proj_bytes = 0, chol_flops = 0, lm_schur_flops = 0, lm_schur_flops_sym = 0, lm_schur_mfma = 0;
    int last_mode = -1;
};

// ------------------------------------------------------------------ batch API
// The symbolic phase is swf_plan.cpp (host-only): this function uploads a Plan and computes none of its tables.  The data slabs take
// the tables in a fixed order (put), the zero slabs the mutable buffers (zeros); one copy per data slab and one memset per zero slab.
extern "C" int swf_batch_create(const swf_flat_window* const* windows, int32_t n, void* stream, swf_batch** out) {
    if (!windows || n <= 0 || !out) return fail(SWF_E_INVALID, "swf_batch_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SWF_E_NODEVICE, "no HIP device: this library has no CPU fallback");
    int n_cu = 256;
    { int dev = 0; hipDeviceProp_t pr; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) n_cu = pr.multiProcessorCount; }
    // (the launch-shape knobs that remain are test aids, each exercised by the GPU tier, and are read once, here: no getenv on the latency
    // path or inside the marginalisation's sweep loop, and none that could race a setenv from the per-device enqueue threads of
    // swf_solve_batches.  Nothing that changes RESULTS is an environment variable: those are fields of swf_options.)
    Plan B;
    {
        std::string err;
        int prc = plan_build(windows, n, plan_shape_from_env(n_cu), B, err);
        if (prc != SWF_OK) return fail(prc, err);
    }
    std::unique_ptr<swf_batch> owner(new swf_batch());
    swf_batch* b = owner.get();
    b->device = current_device();
    b->stream = (hipStream_t)stream;
    b->n_cu = n_cu;
    b->no_comp_fuse = getenv("SWF_NO_COMP_FUSE") != nullptr;
    b->no_spec = getenv("SWF_NO_SPEC_EVAL") != nullptr;
    b->no_step_fuse = getenv("SWF_NO_STEP_FUSE") != nullptr;
    b->no_decide_fuse = getenv("SWF_NO_DECIDE_FUSE") != nullptr;
    b->full_final = getenv("SWF_FULL_FINAL_ELIM") != nullptr;
    b->no_clq_pack = getenv("SWF_NO_CLIQUE_PACK") != nullptr;
    b->no_clq_mfma = getenv("SWF_NO_CLIQUE_MFMA") != nullptr;
    // what the launcher reads of the plan
    b->max_tiles = B.max_tiles; b->max_prior_dim = B.max_prior_dim; b->max_red = B.max_red; b->min_red = B.min_red;
    b->rr_nmax = B.rr_nmax; b->rr4_has15 = B.rr4_has15; b->rr4_has16 = B.rr4_has16; b->n_pch_split = B.n_pch_split;
    b->lat_fuse = B.lat_fuse; b->asm_programs = B.asm_programs;
    b->ls_qpb = B.ls_qpb; b->ls_var = B.ls_var; b->ls_kms = B.ls_kms; b->ls_gqpb = B.ls_gqpb; b->ls_folded = B.ls_folded; b->s_direct = B.s_direct;
    for (int k = 0; k < 5; k++) b->clc_imu[k] = B.clc_imu[k];
    b->clp_rows = B.clp_rows; b->clp_ld = B.clp_ld;
    b->n_comp = B.n_comp; b->comp_nmax = B.comp_nmax; b->comp_nmin = B.comp_nmin; b->comp_ne = B.comp_ne;
    b->jac_bytes = B.jac_bytes; b->proj_bytes = B.proj_bytes; b->chol_flops = B.chol_flops;
    b->lm_schur_flops = B.lm_schur_flops; b->lm_schur_flops_sym = B.lm_schur_flops_sym; b->lm_schur_mfma = B.lm_schur_mfma;
    if (B.want_aux) {                                      // fork / join inside a linearisation
        bool ok = (b->aux = handle_cache().stream()) != nullptr;
        for (int i = 0; i < 3 && ok; i++) ok = (b->ev_fork[i] = handle_cache().event(false)) != nullptr;
        if (!ok) { handle_cache().give(b->aux); b->aux = nullptr; }
    }
    DevBatch& D = b->D;
    DevPool& P = b->pool;
    int rc = 0;
    D.n_win = n; D.n_x = (int)B.n_x; D.n_loc_total = (int)B.n_loc; D.max_iter_trace = SWF_MAX_TRACE; D.rr_nmax = B.rr_nmax;
    D.n_lmb = B.n_lmb; D.n_pch = B.n_pch; D.n_proj = B.n_proj; D.n_lm = B.n_lm; D.n_fr = B.n_fr; D.n_fsb = B.n_fsb;
    D.n_gf = (int)B.gf.size(); D.n_imu = (int)B.imu_gf.size(); D.n_sc = (int)B.sc_gf.size(); D.n_prior = (int)B.prior_gf.size(); D.n_idp = (int)B.idp_gf.size();
    D.n_cl = (int)B.cl.size(); D.n_pair = (int)B.pair.size(); D.n_pd = B.n_pd; D.n_po = B.n_po; D.n_cle = B.n_cle;
    for (int k = 0; k < 5; k++) D.n_clc[k] = B.n_clc[k];
    D.as_max_ne = B.as_max_ne; D.as_max_nv = B.as_max_nv;
    // ---- the tables: ONE upload section, in the order the data slabs have always had
#define PUT(field) rc |= P.put(B.field, &D.field)
    PUT(win);
    PUT(lmb_rec); PUT(pch_q); PUT(pch_r0); PUT(prior_nch);
    PUT(blk_xoff); PUT(blk_loc); PUT(blk_gs);
    PUT(loc2x); PUT(x_var);
    PUT(p_win); PUT(p_xpose); PUT(p_xex); PUT(p_xlm);
    PUT(p_lpose); PUT(p_llm); PUT(p_fr); PUT(p_lm); PUT(p_uv);
    PUT(lm_win); PUT(lm_obs0); PUT(lm_loc); PUT(lm_col); PUT(lm_fmask);
    PUT(sch_c0); PUT(sch_rec); PUT(sch_km);
    PUT(fr_obs0); PUT(fr_obs); PUT(fr_red);
    PUT(fsb_rec);
    PUT(fsb_perm); PUT(fsb_foff);
    PUT(gf);
    PUT(s_x); PUT(s_loc); PUT(s_ls); PUT(s_joff); PUT(s_ccol);
    PUT(imu_pre); PUT(cp_dat); PUT(pr_dat); PUT(dop_dat); PUT(sp_w); PUT(gx_dat);
    PUT(imu_gf); PUT(sc_gf); PUT(prior_gf); PUT(idp_gf);
    PUT(sc_jt); PUT(imu_jt); PUT(imu_rec);
    PUT(prior_dim); PUT(prior_Joff); PUT(prior_roff); PUT(prior_x0off);
    PUT(prior_Jt);
    PUT(prior_colloc); PUT(prior_colcc); PUT(s_pcol); PUT(s_pxo);
    PUT(prior_J); PUT(prior_r0); PUT(prior_x0);
    PUT(cl); PUT(cl_fac); PUT(cl_frow); PUT(cm_loc); PUT(cm_ls); PUT(cm_col);
    PUT(cv_loc);
    PUT(pc_coff); PUT(pc_cld); PUT(pc_voff);
    PUT(asw); PUT(s_tnz);
    PUT(as_dst); PUT(as_cnt); PUT(as_src0); PUT(as_aux); PUT(as_src);
    PUT(av_loc); PUT(av_red); PUT(av_cnt); PUT(av_src0); PUT(av_i); PUT(av_src);
    PUT(pair_d); PUT(pair_o);
    PUT(cle_rec);
    for (int k = 0; k < 5; k++) PUT(clc_rec[k]);
#undef PUT
    {
        const double* ci = nullptr; const double* di = nullptr;
        rc |= P.put(B.C_init, &ci); rc |= P.put(B.dgraw_init, &di);
        D.C = (double*)ci; D.cv_dgraw = (double*)di;
    }
    // composite IMU-GNSS factors: operator arguments over the whole batch + where each factor's prior record and clique live
    CompArgs& A = b->CA; CompMeta& Mt = b->CM;
    const int nc = B.n_comp;
    if (nc) {
        A.n = nc; A.want_jac = 1; A.n_iq = (int)B.co_iq_f.size();
        rc |= P.put(B.co_M, &A.M); rc |= P.put(B.co_N, &A.N); rc |= P.put(B.co_eo, &A.e_off); rc |= P.put(B.co_no, &A.n_off);
        rc |= P.put(B.co_pno, &A.pn_off); rc |= P.put(B.co_nno, &A.nn_off); rc |= P.put(B.co_go, &A.g_off); rc |= P.put(B.co_g2o, &A.g2_off);
        { const double* t1 = nullptr; const double* t2 = nullptr; rc |= P.put(B.co_pose, &t1); rc |= P.put(B.co_sb, &t2); A.pose = (double*)t1; A.sb = (double*)t2; }
        { const double* t1 = nullptr; const double* t2 = nullptr; rc |= P.put(B.co_pose, &t1); rc |= P.put(B.co_sb, &t2); b->co_pose0 = (double*)t1; b->co_sb0 = (double*)t2; }
        rc |= P.put(B.co_pose_lin, &A.pose_lin); rc |= P.put(B.co_sb_lin, &A.sb_lin); rc |= P.put(B.co_Hpp, &A.Hpp); rc |= P.put(B.co_HpN, &A.HpN);
        rc |= P.put(B.co_rhs_p, &A.rhs_p); rc |= P.put(B.co_HNN, &A.HNN); rc |= P.put(B.co_rhsN, &A.rhsN); rc |= P.put(B.co_pre, &A.pre); rc |= P.put(B.co_pbgw, &A.pbgw);
        rc |= P.put(B.co_mid, &A.mid); rc |= P.put(B.co_H12, &A.H12);
        rc |= P.put(B.co_iq_f, &A.iq_f); rc |= P.put(B.co_iq_k, &A.iq_k);
        rc |= P.put(B.co_win, &Mt.win); rc |= P.put(B.co_xo_off, &Mt.xo_off); rc |= P.put(B.co_xo, &Mt.xo);
        rc |= P.put(B.co_Joff, &Mt.Joff); rc |= P.put(B.co_roff, &Mt.roff); rc |= P.put(B.co_x0off, &Mt.x0off); rc |= P.put(B.co_Coff, &Mt.Coff); rc |= P.put(B.co_voff, &Mt.voff);
        Mt.prior_J = (double*)D.prior_J; Mt.prior_Jt = (double*)D.prior_Jt; Mt.prior_r0 = (double*)D.prior_r0; Mt.prior_x0 = (double*)D.prior_x0;
    }
    // ---- the mutable buffers: zero slabs
    rc |= P.zeros((size_t)B.fs_tot * FS_VAL, &D.fs_part);
    rc |= P.zeros((size_t)std::max<long long>(B.n_loc, 1), &D.jsc);
    rc |= P.zeros(B.n_x, &D.x); rc |= P.zeros(B.n_x, &D.xc); rc |= P.zeros(B.n_x, &D.x0);
    rc |= P.zeros(B.n_loc, &D.g); rc |= P.zeros(B.n_loc, &D.diag); rc |= P.zeros(B.n_loc, &D.rhs); rc |= P.zeros(B.n_loc, &D.vc);
    rc |= P.zeros(B.n_loc, &D.y); rc |= P.zeros(B.n_loc, &D.step);
    rc |= P.zeros(B.S_tot, &D.S); rc |= P.zeros(B.Lt_tot, &D.L);
    if (B.want_Linv) rc |= P.zeros((size_t)n * (CB_MAXT - 1) * 256, &D.Linv);
    if (B.want_Wk) rc |= P.zeros(B.Lt_tot, &D.Wk);
    rc |= P.zeros((size_t)n, &D.ws); rc |= P.zeros((size_t)n, &b->ws_alt); rc |= P.zeros((size_t)n, &b->ws_alt2); rc |= P.zeros((size_t)n * SWF_MAX_TRACE, &D.trace);
    b->ws_primary = D.ws;
    size_t np = (size_t)D.n_proj;
    rc |= P.zeros(2 * np, &D.p_r); rc |= P.zeros(12 * np, &D.p_Jp); rc |= P.zeros(6 * np, &D.p_Jl);
    rc |= P.zeros((size_t)std::max(1, D.n_fsb), &D.p_cpart); rc |= P.zeros((size_t)std::max(1, D.n_lmb), &D.p_apart);
    rc |= P.zeros((size_t)std::max(1, D.n_pch), &D.pr_cpart); rc |= P.zeros((size_t)std::max(1, D.n_pch), &D.pr_apart);
    rc |= P.zeros(6 * (size_t)D.n_lm, &D.lm_Einv); rc |= P.zeros(3 * (size_t)D.n_lm, &D.lm_g);
    rc |= P.zeros(B.P_tot * GEMM_SPLIT, &D.P);
    rc |= P.zeros((size_t)std::max(1, 6 * B.n_fr) * GEMM_SPLIT, &D.lmq);
    rc |= P.zeros((size_t)B.r_tot, &D.g_r); rc |= P.zeros((size_t)B.j_tot, &D.g_J);
    rc |= P.zeros((size_t)D.n_gf, &D.g_cost); rc |= P.zeros((size_t)D.n_gf, &D.g_aux);
    rc |= P.zeros((size_t)B.v_tot, &D.cv_graw); rc |= P.zeros((size_t)B.v_tot, &D.cv_cs);
    rc |= P.zeros((size_t)B.e_tot, &D.cE);
    if (nc) {
        const size_t ne = (size_t)B.co_eo[nc], nn = (size_t)B.co_no[nc], ng = (size_t)B.co_go[nc], ng2 = (size_t)B.co_g2o[nc];
        rc |= P.zeros(ne * 225, &A.hmn_inv); rc |= P.zeros(ne * 225, &A.hmn_2); rc |= P.zeros(ne * 225, &A.hmn_0);
        rc |= P.zeros((size_t)B.co_pno[nc], &A.hmn_N); rc |= P.zeros(ne * 15, &A.rhsmn);
        rc |= P.zeros(ng2, &A.Hd); rc |= P.zeros(ng, &A.rd); rc |= P.zeros(ng2, &A.Ld); rc |= P.zeros(ng, &A.r0);
        rc |= P.zeros((size_t)nc * 32, &A.old); rc |= P.zeros(nn, &A.N_old); rc |= P.zeros((size_t)nc, &A.history); rc |= P.zeros((size_t)nc, &A.status);
        rc |= P.zeros((size_t)nc * 32, &Mt.outer); rc |= P.zeros(nn, &Mt.Nv); rc |= P.zeros((size_t)nc, &Mt.active);
        A.outer = Mt.outer; A.Nv = Mt.Nv; A.active = Mt.active;
        rc |= P.zeros(ng, &A.res_out); rc |= P.zeros(ng2, &A.jac_out);
        rc |= P.zeros((ne + nc) * 450, &A.Jw); rc |= P.zeros((ne + nc) * 16, &A.rw);
        rc |= P.zeros((size_t)nc, &A.todo);
    }
    if (!rc) rc = P.flush();
    if (rc) { P.release(); return fail(SWF_E_NODEVICE, "device allocation / upload failed"); }
    b->win = std::move(B.win); b->hw = std::move(B.hw);      // the host's copy of the window records, and what it keeps per window
    *out = owner.release();
    int urc = swf_batch_upload_state(b);
    if (urc != SWF_OK) { swf_batch_destroy(b); *out = nullptr; return urc; }
    return SWF_OK;
}

// the static block partition of SURVEY.md 8e (512 windows, 64 per GPU at 8): shard k of G takes `count` consecutive windows from `first`,
// the first n % G shards one more — the same rule as the harness's shard.partition (no device needed)
extern "C" int swf_shard_partition(int32_t n, int32_t G, int32_t k, int32_t* first, int32_t* count) {
    if (n < 0 || G <= 0 || k < 0 || k >= G || !first || !count) return fail(SWF_E_INVALID, "swf_shard_partition: bad arguments");
    const int q = n / G, r = n % G;
    *first = k * q + std::min(k, r); *count = q + (k < r ? 1 : 0);
    return SWF_OK;
}

// ---- several GPUs of one node from one process (windows are independent units, "one host thread + one HIP stream per
// GPU", no data-path collective).  swf_batch_solve only ENQUEUES work on its batch's stream, so a single host thread keeps all devices busy.
extern "C" int swf_batch_create_on(int32_t device, const swf_flat_window* const* windows, int32_t n, void* stream, swf_batch** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SWF_E_NODEVICE, "no HIP device: this library has no CPU fallback");
    if (device < 0 || device >= ndev || device >= SWF_MAX_DEVICES) return fail(SWF_E_INVALID, "swf_batch_create_on: no such device");
    DeviceGuard dg_(device);
    return swf_batch_create(windows, n, stream, out);
}

// windows [0, n) dealt in contiguous, near-equal blocks to the devices of device_mask (bit d = use device d; 0 = every visible device):
// one batch per device that receives windows, out_batches[k] / out_first[k] / out_count[k] for k < *n_batches (capacity: the device count)
extern "C" int swf_batch_create_sharded(const swf_flat_window* const* windows, int32_t n, uint32_t device_mask,
                                        swf_batch** out_batches, int32_t* out_first, int32_t* out_count, int32_t* n_batches) {
    if (!windows || n <= 0 || !out_batches || !n_batches) return fail(SWF_E_INVALID, "swf_batch_create_sharded: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SWF_E_NODEVICE, "no HIP device: this library has no CPU fallback");
    std::vector<int> devs;
    for (int d = 0; d < ndev && d < SWF_MAX_DEVICES; d++) if (device_mask == 0 || ((device_mask >> d) & 1u)) devs.push_back(d);
    if (devs.empty()) return fail(SWF_E_INVALID, "swf_batch_create_sharded: device_mask selects no visible device");
    const int G = (int)std::min<size_t>(devs.size(), (size_t)n);
    *n_batches = 0;
    for (int k = 0; k < G; k++) {
        int32_t lo = 0, cnt = 0;
        swf_shard_partition(n, G, k, &lo, &cnt);
        const int hi = lo + cnt;
        swf_batch* bk = nullptr;
        int rc = swf_batch_create_on(devs[k], windows + lo, hi - lo, nullptr, &bk);
        if (rc != SWF_OK) { for (int q = 0; q < *n_batches; q++) swf_batch_destroy(out_batches[q]); *n_batches = 0; return rc; }
        out_batches[k] = bk;
        if (out_first) out_first[k] = lo;
        if (out_count) out_count[k] = hi - lo;
        *n_batches = k + 1;
    }
    return SWF_OK;
}

extern "C" int swf_batch_device(swf_batch* b, int32_t* device) { if (!b || !device) return fail(SWF_E_INVALID, "bad arguments"); *device = b->device; return SWF_OK; }

extern "C" int swf_batch_destroy(swf_batch* b) {
    if (!b) return SWF_OK;
    DeviceGuard dg_(b->device);
    (void)hipStreamSynchronize(b->stream);
    if (b->aux) (void)hipStreamSynchronize(b->aux);     // nothing of this batch may still run when its slabs go back to the cache
    for (auto& e : b->ev) handle_cache().give(e, true);
    if (b->h_x) (void)hipHostFree(b->h_x);
    if (b->h_sum) (void)hipHostFree(b->h_sum);
    if (b->dd_in) (void)hipFree(b->dd_in);
    if (b->dd_out) (void)hipFree(b->dd_out);
    b->pool.release();
    delete b;
    return SWF_OK;
}

extern "C" int swf_batch_upload_state(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "null batch");
    // the parameter blocks are gathered into ONE page-locked buffer the batch keeps (round 5: a pageable source made the runtime stage the
    // copy through its own pinned chunks: ~0.8 ms for the 6.7 MB of a 512-window batch)
    const size_t nx = (size_t)b->D.n_x;
    if (!b->h_x && nx) HIPCHK(hipHostMalloc((void**)&b->h_x, nx * sizeof(double), hipHostMallocDefault));
    double* xh = b->h_x;
    for (size_t i = 0; i < b->win.size(); i++) {
        const HostWin& h = b->hw[i];
        double* p = xh + b->win[i].x_base;
        memcpy(p, h.pose, sizeof(double) * 7 * h.n_pose); p += 7 * h.n_pose;
        memcpy(p, h.sb, sizeof(double) * 9 * h.n_sb); p += 9 * h.n_sb;
        memcpy(p, h.lm, sizeof(double) * 3 * h.n_lm); p += 3 * h.n_lm;
        memcpy(p, h.sc, sizeof(double) * h.n_sc);
    }
    HIPCHK(hipMemcpyAsync(b->D.x, xh, nx * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->D.x0, b->D.x, nx * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->D.xc, b->D.x, nx * sizeof(double), hipMemcpyDeviceToDevice, b->stream));      // (the candidate's constant blocks: k_dogleg writes the variable ones only)
    std::vector<double> hp, hs;
    if (b->n_comp) {
        hp.resize((size_t)b->comp_ne * 7); hs.resize((size_t)b->comp_ne * 9);
        for (size_t i = 0; i < b->win.size(); i++) {
            const HostWin& h = b->hw[i];
            if (!h.comp_ne) continue;
            memcpy(hp.data() + (size_t)h.comp_e0 * 7, h.comp_pose, sizeof(double) * 7 * h.comp_ne);
            memcpy(hs.data() + (size_t)h.comp_e0 * 9, h.comp_sb, sizeof(double) * 9 * h.comp_ne);
        }
        HIPCHK(hipMemcpyAsync(b->co_pose0, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->co_sb0, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->CA.pose, b->co_pose0, hp.size() * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->CA.sb, b->co_sb0, hs.size() * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HIPCHK(hipMemsetAsync(b->CA.history, 0, (size_t)b->n_comp * sizeof(int), b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));     // staging buffers have stack lifetime
    b->fc_valid = false; b->dd_valid = false;
    return SWF_OK;
}

extern "C" int swf_batch_reset_state(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "null batch");
    b->fc_valid = false; b->dd_valid = false;
    int n = b->D.n_x;
    hipLaunchKernelGGL(k_copy, dim3((n + 255) / 256), dim3(256), 0, b->stream, b->D.x, (const double*)b->D.x0, n);
    HIPCHK(hipGetLastError());
    if (b->n_comp) {       // hidden epochs back to the uploaded values, composite factors forget their last linearisation
        HIPCHK(hipMemcpyAsync(b->CA.pose, b->co_pose0, (size_t)b->comp_ne * 7 * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->CA.sb, b->co_sb0, (size_t)b->comp_ne * 9 * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HIPCHK(hipMemsetAsync(b->CA.history, 0, (size_t)b->n_comp * sizeof(int), b->stream));
    }
    return SWF_OK;
}

static DevOpt to_devopt(const swf_options* o) {
    DevOpt d{};
    d.max_iter = o->max_num_iterations; d.step_mode = o->step_mode; d.strategy = o->trust_region_strategy; d.jacobi = o->jacobi_scaling ? 1 : 0;
    d.r0 = o->initial_trust_region_radius; d.max_r = o->max_trust_region_radius; d.min_r = o->min_trust_region_radius;
    d.min_rel_dec = o->min_relative_decrease; d.ftol = o->function_tolerance; d.gtol = o->gradient_tolerance;
    d.ptol = o->parameter_tolerance; d.min_mu = o->min_mu; d.max_mu = o->max_mu; d.mu_inc = o->mu_increase_factor;
    d.min_diag = o->min_diagonal; d.max_diag = o->max_diagonal;
    return d;
}

#define GRID(n, per) dim3((unsigned)(((n) + (per) - 1) / (per)))
namespace {
struct Launcher {
    swf_batch* b; DevOpt O; hipStream_t st;
    bool lm_folded = false;     // k_lm_schur of the current linearisation wrote ONE folded product (else GEMM_SPLIT partials)
    bool export_full = false;   // k_chol_rr4 writes the whole factor (ASSEMBLE_ELIMINATE_ONLY: marginalisation, swf_batch_export_reduced), else the tail block only
    int lm_next = 0, lm_qpb = 1;                 // first tile of the ranges of k_lm_schur still to launch (with the clique kernels)
    int ls_tiles_per_launch() const { return b->ls_var == 0 ? 16 : b->ls_var == 1 ? 40 : 72; }
    // one launch of the landmark Schur kernel over the tile-list entries [tile_base, tile_base + tiles per launch), by row class
    WinState* ws_next(WinState* p) const { return p == b->ws_primary ? b->ws_alt : p == b->ws_alt ? b->ws_alt2 : b->ws_primary; }
    bool decide_fused = false;  // this iteration's k_decide rides at the head of the elimination grid (k_decide_lm_clique)
    void lm_launch(int tile_base, hipStream_t on, int clique_rows = 0) {
        DevBatch& D = b->D;
        dim3 grid(D.n_win, GEMM_SPLIT / b->ls_qpb);
        const int qpb = b->ls_qpb, sd = b->s_direct ? 1 : 0, lp = tile_base / ls_tiles_per_launch(), kms = b->ls_kms;
        if (clique_rows > 0) {
            const int np = (int)grid.y;
            grid.y += clique_rows;
            if (decide_fused) {
                WinState* out = ws_next(D.ws);                  // (its failure flags were cleared by k_step_eval's lead)
                if (b->ls_var == 0) hipLaunchKernelGGL((k_decide_lm_clique<8, 2, 2, 80>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd, np, out);
                else hipLaunchKernelGGL((k_decide_lm_clique<8, 5, 2, 144>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd, np, out);
                D.ws = out;
                return;
            }
            switch (b->ls_var) {
            case 0: hipLaunchKernelGGL((k_lm_clique<8, 2, 2, 80>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd, np); break;
            case 1: hipLaunchKernelGGL((k_lm_clique<8, 5, 2, 144>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd, np); break;
            default: hipLaunchKernelGGL((k_lm_clique<12, 6, 1, 272>), grid, dim3(LS_NT(12, 1)), 0, on, D, O, qpb, lp, kms, 0, np); break;
            }
            return;
        }
        switch (b->ls_var) {
        case 0: hipLaunchKernelGGL((k_lm_schur<8, 2, 2, 80, true>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd); break;
        case 1: hipLaunchKernelGGL((k_lm_schur<8, 5, 2, 144, true>), grid, dim3(LS_NT(8, 2)), 0, on, D, O, qpb, lp, kms, sd); break;
        case 2: hipLaunchKernelGGL((k_lm_schur<12, 6, 1, 272, true>), grid, dim3(LS_NT(12, 1)), 0, on, D, O, qpb, lp, kms, 0); break;
        default: hipLaunchKernelGGL((k_lm_schur<12, 6, 1, 400, true>), grid, dim3(LS_NT(12, 1)), 0, on, D, O, qpb, lp, kms, 0); break;
        }
    }
    // optional event pair around one launch
    struct Bracket {
        Launcher& L; int slot; hipStream_t bst;
        Bracket(Launcher& l, int kind, hipStream_t on = nullptr) : L(l), slot(-1), bst(on ? on : l.st) {
            swf_batch* b = L.b;
            if (!(b->timing & (1 << kind))) return;
            if ((size_t)(b->ev_used + 1) * 2 > b->ev.size()) {
                size_t old = b->ev.size();
                b->ev.resize(old + 64);
                bool ok = true;
                for (size_t i = old; i < b->ev.size(); i++) { b->ev[i] = handle_cache().event(true); ok = ok && b->ev[i] != nullptr; }
                if (!ok) {                                 // no events to be had: this launch goes untimed
                    for (size_t i = old; i < b->ev.size(); i++) handle_cache().give(b->ev[i], true);
                    b->ev.resize(old); return;
                }
            }
            slot = b->ev_used++;
            b->ev_kind.push_back(kind);
            (void)hipEventRecord(b->ev[2 * slot], bst);
        }
        ~Bracket() { if (slot >= 0) (void)hipEventRecord(L.b->ev[2 * slot + 1], bst); }
    };
    static int nb(size_t n, int per) { return (int)((n + per - 1) / per); }
    // One linearisation.  Dependencies: the cliques need the IMU and the scalar-factor Jacobians (k_eval_imu, k_eval_ps);
    // k_lm_schur needs k_eval_ps; k_assemble_flat needs everything.  With an auxiliary
    // stream (small batches) the IMU / clique branch runs next to the projection / landmark branch.
    // the reference-topology latency path (swf_kernels4.h, k_lm_comp): the composite chain and the visual branch in shared grids
    bool comp_fused = false;
    bool comp_fuse_ok(int write_S) const {
        const DevBatch& D = b->D;
        if (!b->n_comp || !write_S || b->no_comp_fuse || !b->lat_fuse || b->aux || b->comp_eigen_root) return false;
        if (b->comp_nmax > CO_SMALLN || b->ls_var > 1 || !D.n_lm || D.n_imu || D.n_idp || b->max_prior_dim > PRIOR_LDS_DIM) return false;
        if (D.n_clc[0] || D.n_clc[1]) return false;                                     // (the cliques of such a window: classes 2, 4 and — from 19 ambiguities on — 3)
        const int crow = (b->n_comp + D.n_win - 1) / D.n_win;
        return (long long)D.n_win * (GEMM_SPLIT / b->ls_qpb + crow) <= b->n_cu;         // every workgroup of k_lm_comp resident at once
    }
    // spec: the Jacobian evaluation of the dogleg loop's speculative flow — at the candidate of every window with a proposed step
    // (swf_kernels.h: eval_gate / eval_src); the evaluation kernels get a copy of the batch record with the flag set
    void lin_eval(int write_S, bool spec = false) {
        DevBatch Dv = b->D; Dv.spec = spec ? 1 : 0;
        const DevBatch& D = Dv;
        comp_fused = !spec && comp_fuse_ok(write_S);
        if (comp_fused) {
            hipLaunchKernelGGL(k_comp_gather_prep, dim3(b->n_comp), dim3(256), 0, st, D, b->CA, b->CM);
            Segs S{}; S.e[0] = D.n_fsb; S.e[1] = S.e[0] + nb(D.n_sc, 256);
            {   // projection + scalar factors next to the chains' IMU factors
                Bracket t(*this, SWF_K_EVAL_PS);
                hipLaunchKernelGGL(k_eval_ps_comp_imu, dim3(S.e[1] + (b->CA.n_iq + 7) / 8), dim3(256), 0, st, D, S, b->CA);
            }
            {   // the landmark Schur product (first tile range) next to the re-elimination of the hidden epochs
                Bracket t(*this, SWF_K_LM_SCHUR);
                lm_qpb = b->ls_qpb; lm_folded = b->ls_folded;
                const int np = GEMM_SPLIT / b->ls_qpb, crow = (b->n_comp + D.n_win - 1) / D.n_win;
                const int qpb = b->ls_qpb, sd = b->s_direct ? 1 : 0, kms = b->ls_kms;
                dim3 grid(D.n_win, np + crow);
                if (b->ls_var == 0) hipLaunchKernelGGL((k_lm_comp<8, 2, 2, 80>), grid, dim3(LS_NT(8, 2)), 0, st, D, O, b->CA, b->CM, qpb, 0, kms, sd, np);
                else hipLaunchKernelGGL((k_lm_comp<8, 5, 2, 144>), grid, dim3(LS_NT(8, 2)), 0, st, D, O, b->CA, b->CM, qpb, 0, kms, sd, np);
                lm_next = ls_tiles_per_launch();
            }
            if (D.n_prior) {   // the prior records (the composite factors' among them, just rewritten): the prior segment of k_eval_ps alone
                Segs P{}; P.e[2] = D.n_pch;
                hipLaunchKernelGGL((k_eval_ps<true, true>), dim3(P.e[2]), dim3(256), 0, st, D, P);
            }
            return;
        }
        if (b->n_comp && !spec) {
            // composite IMU-GNSS factors of the windows that re-linearise: hidden epochs move, re-elimination, prior records rewritten
            // 1024 threads per factor while the chip holds every factor at once (two such workgroups per CU), 256 for larger batches
            const bool wide = b->n_comp <= 2 * b->n_cu;
            {
            hipLaunchKernelGGL(k_comp_gather_prep, dim3(b->n_comp), dim3(256), 0, st, D, b->CA, b->CM);
            hipLaunchKernelGGL(k_comp_imu, dim3((b->CA.n_iq + 7) / 8), dim3(256), 0, st, b->CA);
            // (an instantiation per class of factor, each passing over the other's: a factor's arithmetic does not depend on its batch)
            if (b->comp_nmin <= CO_SMALLN) {
                if (wide) hipLaunchKernelGGL((k_comp_elim<CO_SMALLN, 1024>), dim3(b->n_comp), dim3(1024), 0, st, b->CA, 0);
                else {
                    // batches: factors of up to 12 ambiguities in the instantiation that fits six workgroups to a CU
                    if (b->comp_nmin <= CO_TINYN) hipLaunchKernelGGL((k_comp_elim<CO_TINYN, 256>), dim3(b->n_comp), dim3(256), 0, st, b->CA, 0);
                    if (b->comp_nmax > CO_TINYN) hipLaunchKernelGGL((k_comp_elim<CO_SMALLN, 256>), dim3(b->n_comp), dim3(256), 0, st, b->CA, CO_TINYN + 1);
                }
            }
            if (b->comp_nmax > CO_SMALLN) {
                if (wide) hipLaunchKernelGGL((k_comp_elim<CO_MAXN, 1024>), dim3(b->n_comp), dim3(1024), 0, st, b->CA, CO_SMALLN + 1);
                else hipLaunchKernelGGL((k_comp_elim<CO_MAXN, 256>), dim3(b->n_comp), dim3(256), 0, st, b->CA, CO_SMALLN + 1);
            }
            if (b->comp_eigen_root) {
                if (b->comp_nmax <= CO_SMALLN) hipLaunchKernelGGL(k_comp_eigroot<CO_SMALLN>, dim3(b->n_comp), dim3(256), 0, st, b->CA);
                else hipLaunchKernelGGL(k_comp_eigroot<CO_MAXN>, dim3(b->n_comp), dim3(512), 0, st, b->CA);
            }
            hipLaunchKernelGGL(k_comp_scatter, dim3(b->n_comp), dim3(256), 0, st, D, b->CA, b->CM);
            }
        }
        // (speculative flow: k_decide, on the main stream, reads every family's candidate costs — the whole evaluation stays on the main
        // stream, and the fork event the clique branch waits for is recorded behind k_decide, see swf_batch_solve)
        const bool fork = b->aux && !spec;
        hipStream_t sa = fork ? b->aux : st;
        if (fork) { (void)hipEventRecord(b->ev_fork[0], st); (void)hipStreamWaitEvent(b->aux, b->ev_fork[0], 0); }
        bool imu_fused = false;
        if (D.n_proj + D.n_sc + D.n_prior) {
            Bracket t(*this, SWF_K_EVAL_PS);
            bool pf = b->max_prior_dim <= PRIOR_LDS_DIM;          // priors fused as a segment
            // (the projection segment: one workgroup per frame-sum block, the per-frame sums formed in the same kernel)
            Segs S{}; S.e[0] = D.n_fsb; S.e[1] = S.e[0] + nb(D.n_sc, 256); S.e[2] = S.e[1] + (pf ? D.n_pch : 0);
            imu_fused = b->lat_fuse && D.n_imu > 0;          // latency path: the IMU factors as a segment of this grid
            S.e[3] = S.e[2] + (imu_fused ? nb(D.n_imu, IMU_FPB) : 0);
            if (imu_fused) hipLaunchKernelGGL((k_eval_ps<true, true, true>), dim3(S.e[3]), dim3(256), 0, st, D, S);
            else hipLaunchKernelGGL((k_eval_ps<true, true>), dim3(S.e[2]), dim3(256), 0, st, D, S);
        }
        if (D.n_idp) hipLaunchKernelGGL(k_eval_idp<true>, GRID(D.n_idp, 128), dim3(128), 0, st, D);
        // (large priors before the fork event: a prior-type record inside a group-0 clique writes its rows into that clique's Jacobian, and a
        // clique class with IMU factors runs on the auxiliary stream behind ev_fork[1] alone)
        if (D.n_prior && b->max_prior_dim > PRIOR_LDS_DIM) { Bracket t(*this, SWF_K_EVAL_PRIOR); hipLaunchKernelGGL(k_eval_prior<true>, dim3(D.n_pch), dim3(256), (2 * b->max_prior_dim + 16) * sizeof(double), st, D); }
        if (fork) (void)hipEventRecord(b->ev_fork[1], st);
        if (D.n_imu && !imu_fused) { Bracket t(*this, SWF_K_EVAL_IMU, sa); hipLaunchKernelGGL(k_eval_imu<true>, GRID(D.n_imu, IMU_FPB), dim3(IMU_FPB * IMU_LPF), 0, sa, D); }
    }
    void lin_elim(int write_S) {
        DevBatch& D = b->D;
        bool clq_fused = false;
        if (comp_fused) {
            // (k_lm_comp of lin_eval took the first tile range of the landmark product)
            Bracket t(*this, SWF_K_CLIQUE_ELIM);
            if (D.n_clc[3]) {
                // class 3 next to class 2 in one grid; class 4 (other factors of the batch with fewer ambiguities) on its own
                hipLaunchKernelGGL(k_clique_big2, dim3(D.n_clc[3] + D.n_clc[2]), dim3(CB_NT), 0, st, D, O);
                if (D.n_clc[4]) hipLaunchKernelGGL(k_clique_tall<false>, dim3(D.n_clc[4]), dim3(256), 0, st, D, O);
            } else if (D.n_clc[4] + D.n_clc[2]) hipLaunchKernelGGL(k_clique_tall2, dim3(D.n_clc[4] + D.n_clc[2]), dim3(256), 0, st, D, O);
        } else if (D.n_lm) {
            Bracket t(*this, write_S ? SWF_K_LM_SCHUR : SWF_K_LM_ELIM);
            lm_qpb = b->ls_qpb; lm_folded = b->ls_folded;
            if (!write_S && !b->full_final) {
                // cost / gradient pass (the solve's final linearisation; k_finalize reads the gradient alone): g, diag and vc of the landmarks —
                // producer waves only, no panel, no inverse, at a workgroup size of its own
                dim3 grid(D.n_win, GEMM_SPLIT / b->ls_gqpb);
                hipLaunchKernelGGL((k_lm_schur<8, 2, 2, 80, false, true>), grid, dim3(256), 0, st, D, O, b->ls_gqpb, 0, 0, 0);
            } else if (!write_S) {
                // (SWF_FULL_FINAL_ELIM: the elimination alone, Einv and g_l included)
                dim3 grid(D.n_win, GEMM_SPLIT / lm_qpb);
                hipLaunchKernelGGL((k_lm_schur<8, 2, 2, 80, false>), grid, dim3(256), 0, st, D, O, lm_qpb, 0, 0, 0);
            } else {
                // latency path: the one-wavefront cliques ride in the same grid (k_lm_clique); the 64-frame class has no LDS to spare for them
                // (a workgroup of that grid fills a CU: only while all of them — landmark parts and cliques — are resident at once)
                const int crow = D.n_win > 0 ? (D.n_clc[2] + D.n_win - 1) / D.n_win : 0;
                clq_fused = clq_fuse_ok();
                lm_launch(0, st, clq_fused ? crow : 0);
                lm_next = ls_tiles_per_launch();        // further tile ranges: launched below, on the auxiliary stream when there is one
            }
        }
        {
            hipStream_t sa = b->aux ? b->aux : st;
            if (b->aux) (void)hipStreamWaitEvent(b->aux, b->ev_fork[1], 0);          // scalar-factor Jacobians (k_eval_ps)
            // latency path: a class without IMU factors needs only k_eval_ps and runs on the main stream, next to the IMU branch
            auto cstream = [&](int cls) { return (b->aux && !b->clc_imu[cls]) ? st : sa; };
            if (comp_fused) {
                for (; lm_next < b->max_tiles; lm_next += ls_tiles_per_launch()) { Bracket t(*this, SWF_K_LM_SCHUR, sa); lm_launch(lm_next, sa); }
            } else {
            // (the final linearisation: the gradient-only instantiations of the same function; k_clique_big has none and runs in full)
            const bool grad = !write_S && !b->full_final;
            if (D.n_clc[1]) {
                Bracket t(*this, SWF_K_CLIQUE_ELIM, cstream(1));
                if (grad) hipLaunchKernelGGL((k_clique_elim<32, 48, 9, 1, true>), dim3(D.n_clc[1]), dim3(64), 0, cstream(1), D, O);
                else if (b->no_clq_mfma) hipLaunchKernelGGL((k_clique_elim<32, 48, 9, 1>), dim3(D.n_clc[1]), dim3(64), 0, cstream(1), D, O);
                else hipLaunchKernelGGL((k_clique_mm<32, 48, 9>), dim3(D.n_clc[1]), dim3(64), 0, cstream(1), D, O);      // batch path: J^T J and the C update on the matrix cores, same bits
            }
            if (D.n_clc[0]) {
                Bracket t(*this, SWF_K_CLIQUE_ELIM, cstream(0));
                // two cliques per wavefront, LDS for the batch's largest class-0 clique (two halves of Jc | rv | Me | T | Ei | Eg)
                // (one wavefront per workgroup: four independent ones measured slower, 29.4 against 25.7 us per launch: profiles/r09)
                constexpr int CLP_NW = 1;
                const size_t lds = CLP_NW * 2 * ((size_t)(b->clp_rows + 2) * b->clp_ld + b->clp_rows + 2) * sizeof(double);
                const dim3 cgrid(((D.n_clc[0] + 1) / 2 + CLP_NW - 1) / CLP_NW);
                if (b->no_clq_pack) {
                    if (grad) hipLaunchKernelGGL((k_clique_elim<48, 32, 1, 0, true>), dim3(D.n_clc[0]), dim3(64), 0, cstream(0), D, O);
                    else hipLaunchKernelGGL((k_clique_elim<48, 32, 1, 0>), dim3(D.n_clc[0]), dim3(64), 0, cstream(0), D, O);
                }
                else if (grad) hipLaunchKernelGGL((k_clique_pack<true, CLP_NW>), cgrid, dim3(64 * CLP_NW), lds, cstream(0), D, O, b->clp_rows, b->clp_ld);
                else hipLaunchKernelGGL((k_clique_pack<false, CLP_NW>), cgrid, dim3(64 * CLP_NW), lds, cstream(0), D, O, b->clp_rows, b->clp_ld);
            }
            if (D.n_clc[2] && !clq_fused) {
                Bracket t(*this, SWF_K_CLIQUE_ELIM, cstream(2));
                if (b->lat_fuse) {      // latency form: four waves per clique, same bits
                    if (grad) hipLaunchKernelGGL(k_clique_elim4<true>, dim3(D.n_clc[2]), dim3(256), 0, cstream(2), D, O);
                    else hipLaunchKernelGGL(k_clique_elim4<false>, dim3(D.n_clc[2]), dim3(256), 0, cstream(2), D, O);
                }
                else if (grad) hipLaunchKernelGGL((k_clique_elim<64, 64, 9, 2, true>), dim3(D.n_clc[2]), dim3(64), 0, cstream(2), D, O);
                else hipLaunchKernelGGL((k_clique_elim<64, 64, 9, 2>), dim3(D.n_clc[2]), dim3(64), 0, cstream(2), D, O);
            }
            if (D.n_clc[3]) { Bracket t(*this, SWF_K_CLIQUE_ELIM, cstream(3)); hipLaunchKernelGGL(k_clique_big, dim3(D.n_clc[3]), dim3(CB_NT), 0, cstream(3), D, O); }
            if (D.n_clc[4]) {
                Bracket t(*this, SWF_K_CLIQUE_ELIM, cstream(4));
                if (grad) hipLaunchKernelGGL(k_clique_tall<true>, dim3(D.n_clc[4]), dim3(256), 0, cstream(4), D, O);
                else hipLaunchKernelGGL(k_clique_tall<false>, dim3(D.n_clc[4]), dim3(256), 0, cstream(4), D, O);
            }
            if (write_S && D.n_lm) {
                // further tile ranges write nothing but their tiles of P (k_lm_schur: outs), so on the latency path they run behind the
                // IMU / clique branch, next to the first range
                for (; lm_next < b->max_tiles; lm_next += ls_tiles_per_launch()) { Bracket t(*this, SWF_K_LM_SCHUR, sa); lm_launch(lm_next, sa); }
            }
            }
            if (b->aux) (void)hipEventRecord(b->ev_fork[2], b->aux);
        }
        // chunked priors with a static clique: graw = J^T r over column chunks, from the rows the evaluation left in g_r
        if (b->n_pch_split) hipLaunchKernelGGL(k_prior_graw, dim3(D.n_pch), dim3(256), 0, st, D);
        if (b->aux) (void)hipStreamWaitEvent(st, b->ev_fork[2], 0);                  // join before the assembly
        if (D.n_pd) {
            Bracket t(*this, SWF_K_ASSEMBLE);
            const int nbS = write_S ? nb((size_t)D.as_max_ne, 256) : 0, nbV = nb((size_t)D.as_max_nv, 256);
            hipLaunchKernelGGL(k_assemble_flat, dim3(nbS + nbV, D.n_win), dim3(256), 0, st, D, O, write_S, nbS);
        }
    }
    void reduced() {
        DevBatch& D = b->D;
        Bracket t(*this, SWF_K_CHOL);
        if (b->max_red <= CB_NMAX) {
            // per-window choice (each kernel skips the other's windows): register-resident tiles up to 240 dimensions, streamed above
            if (b->min_red <= b->rr_nmax) {
                if (b->min_red <= 224) hipLaunchKernelGGL(k_chol_rr4<14>, dim3(D.n_win), dim3(R4_NT), 0, st, D, export_full ? 1 : 0);
                if (b->rr4_has15) hipLaunchKernelGGL(k_chol_rr4<15>, dim3(D.n_win), dim3(R4_NT), 0, st, D, export_full ? 1 : 0);
                if (b->rr4_has16) hipLaunchKernelGGL(k_chol_rr4<16>, dim3(D.n_win), dim3(R4_NT), 0, st, D, export_full ? 1 : 0);
            }
            if (b->max_red > b->rr_nmax && D.Wk) {
                const int Tc = (b->max_red + 15) / 16;
                const int nbw = std::max(1, std::min(CC_NB, b->n_cu / D.n_win));       // the chip divided by the windows
                for (int j = 0; j < Tc; j += 2) hipLaunchKernelGGL(k_chol_col, dim3(D.n_win, nbw), dim3(CC_NT), 0, st, D, j);
                hipLaunchKernelGGL(k_chol_big<true>, dim3(D.n_win), dim3(1024), 0, st, D);      // backward substitution
            } else if (b->max_red > b->rr_nmax) hipLaunchKernelGGL(k_chol_big<false>, dim3(D.n_win), dim3(1024), 0, st, D);
        }
        else if (b->max_red + 1 <= 256) hipLaunchKernelGGL(k_chol_solve<256>, dim3(D.n_win), dim3(256), 0, st, D);
        else hipLaunchKernelGGL(k_chol_solve<1024>, dim3(D.n_win), dim3(1024), 0, st, D);
    }
    void step_rest() {
        DevBatch& D = b->D;
        {
            Bracket t(*this, SWF_K_POST_CHOL);
            Segs S{};
            S.e[0] = D.n_lmb; S.e[1] = S.e[0] + nb((size_t)D.n_cle * 16, 256);
            S.e[2] = S.e[1]; S.e[3] = S.e[2] + nb(D.n_sc, 256);                                 // (J D^-2 g of the projections rides in segment 0)
            S.e[4] = S.e[3] + nb((size_t)D.n_imu * 16, 256); S.e[5] = S.e[4] + D.n_pch;        // one workgroup per prior row chunk
            if (D.n_win < b->n_cu) { if (S.e[5]) hipLaunchKernelGGL(k_post_chol<0>, dim3(S.e[5]), dim3(256), 0, st, D, O, S); }
            else {
                // two launches from n_cu windows up: measured against the one grid, not a matter of registers any more (the comment
                // above k_post_chol has the figures)
                if (S.e[0]) hipLaunchKernelGGL(k_post_chol<1>, dim3(S.e[0]), dim3(256), 0, st, D, O, S);
                if (S.e[5] > S.e[0]) hipLaunchKernelGGL(k_post_chol<2>, dim3(S.e[5] - S.e[0]), dim3(256), 0, st, D, O, S);
            }
        }
        if (!step_fused) dogleg();
    }
    bool step_fused = false;    // this solve runs k_dogleg inside the candidate's evaluation (k_step_eval): one window on the latency path, speculative flow
    void dogleg() {
        DevBatch& D = b->D;
        Bracket t(*this, SWF_K_DOGLEG);
        if (b->lat_fuse) hipLaunchKernelGGL((k_dogleg<16, 4>), dim3(D.n_win), dim3(CTL_NT), 0, st, D, O);
        else hipLaunchKernelGGL((k_dogleg<4, 2>), dim3(D.n_win), dim3(CTL_NT), 0, st, D, O);
    }
    bool clq_fuse_ok() const {
        const DevBatch& D = b->D;
        const int crow = D.n_win > 0 ? (D.n_clc[2] + D.n_win - 1) / D.n_win : 0;
        return b->lat_fuse && b->ls_var <= 2 && D.n_lm > 0 && D.n_clc[2] > 0 && !D.n_clc[0] && !D.n_clc[1]
               && (long long)D.n_win * (GEMM_SPLIT / b->ls_qpb + crow) <= b->n_cu;
    }
    // k_decide at the head of the elimination grid: one window, the fused step kernel in front (three state buffers in rotation), the
    // cliques in the landmark product's grid, the two smaller size classes of that grid (the third has no LDS to spare)
    bool decide_fuse_ok() const { return step_fused && !b->no_decide_fuse && clq_fuse_ok() && b->ls_var <= 1 && b->max_tiles <= ls_tiles_per_launch(); }
    // (spec = false: the two-pass flows — Levenberg-Marquardt, windows with composite factors — whose cost-only candidate evaluation takes the step the same way)
    bool step_fuse_ok() const {
        const DevBatch& D = b->D;
        return b->lat_fuse && !b->no_step_fuse && !b->aux && D.n_win == 1 && b->win[0].x_n <= XCL_MAX && b->max_prior_dim <= PRIOR_LDS_DIM && !D.n_idp
               && D.n_fsb + nb(D.n_sc, 256) + D.n_pch + nb(D.n_imu, IMU_FPB) > 0;
    }
    // k_dogleg + the Jacobian evaluation at its candidate in one grid (k_step_eval); the window's state moves to the other buffer
    void step_eval(bool jac = true) {
        DevBatch& D = b->D;
        Bracket t(*this, jac ? SWF_K_EVAL_PS : SWF_K_POST_DOGLEG);
        Segs S{}; S.e[0] = D.n_fsb; S.e[1] = S.e[0] + nb(D.n_sc, 256); S.e[2] = S.e[1] + D.n_pch;
        const bool imu = D.n_imu > 0;
        S.e[3] = S.e[2] + (imu ? nb(D.n_imu, IMU_FPB) : 0);
        WinState* out = ws_next(D.ws);
        WinState* clr = decide_fused ? ws_next(out) : nullptr;      // the buffer k_decide_lm_clique will write: its failure flags go down here
        if (!jac) {
            if (imu) hipLaunchKernelGGL((k_step_eval<true, false>), dim3(S.e[3]), dim3(256), 0, st, D, O, S, out, b->win[0], clr);
            else hipLaunchKernelGGL((k_step_eval<false, false>), dim3(S.e[2]), dim3(256), 0, st, D, O, S, out, b->win[0], clr);
        } else if (imu) hipLaunchKernelGGL((k_step_eval<true>), dim3(S.e[3]), dim3(256), 0, st, D, O, S, out, b->win[0], clr);
        else hipLaunchKernelGGL((k_step_eval<false>), dim3(S.e[2]), dim3(256), 0, st, D, O, S, out, b->win[0], clr);
        D.ws = out;
    }
    void decide() {
        DevBatch& D = b->D;
        { Bracket t(*this, SWF_K_DECIDE); hipLaunchKernelGGL(k_decide, dim3(D.n_win), dim3(CTL_NT), 0, st, D, O); }
    }
    void cand_eval() {
        DevBatch& D = b->D;
        {
            Bracket t(*this, SWF_K_POST_DOGLEG);
            Segs S{};
            S.e[0] = D.n_fsb; S.e[1] = S.e[0] + nb(D.n_sc, 256);            // (the projection segment: one workgroup per frame-sum block, as in the Jacobian evaluation)
            S.e[2] = S.e[1] + (b->max_prior_dim <= PRIOR_LDS_DIM ? D.n_pch : 0);
            // small batches (latency path): the candidate IMU residuals ride along as a segment; large batches keep them in
            // their own launch (the segment's LDS would cost the memory-bound segments occupancy).  Same results either way.
            bool fuse_imu = D.n_win < b->n_cu;
            S.e[3] = S.e[2] + (fuse_imu ? nb(D.n_imu, IMU_FPB) : 0);
            if (S.e[3] && fuse_imu) hipLaunchKernelGGL((k_post_dogleg<true, 0>), dim3(S.e[3]), dim3(256), 0, st, D, O, S);
            else if (S.e[3]) {
                if (S.e[0]) hipLaunchKernelGGL((k_post_dogleg<false, 1>), dim3(S.e[0]), dim3(256), 0, st, D, O, S);
                if (S.e[3] > S.e[0]) hipLaunchKernelGGL((k_post_dogleg<false, 2>), dim3(S.e[3] - S.e[0]), dim3(256), 0, st, D, O, S);
            }
            if (!fuse_imu && D.n_imu) hipLaunchKernelGGL(k_eval_imu<false>, GRID(D.n_imu, IMU_FPB), dim3(IMU_FPB * IMU_LPF), 0, st, D);
            if (D.n_idp) hipLaunchKernelGGL(k_eval_idp<false>, GRID(D.n_idp, 128), dim3(128), 0, st, D);
        }
        {
            Bracket t(*this, SWF_K_CAND_EVAL);
            if (D.n_prior && b->max_prior_dim > PRIOR_LDS_DIM) hipLaunchKernelGGL(k_eval_prior<false>, dim3(D.n_pch), dim3(256), (2 * b->max_prior_dim + 16) * sizeof(double), st, D);
        }
        decide();
    }
};
}  // namespace

extern "C" int swf_batch_solve(swf_batch* b, const swf_options* opt) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || !opt) return fail(SWF_E_INVALID, "swf_batch_solve: bad arguments");
    if (opt->max_num_iterations < 0 || opt->max_num_iterations >= SWF_MAX_TRACE) return fail(SWF_E_INVALID, "max_num_iterations out of range");
    if (opt->trust_region_strategy != SWF_DOGLEG && opt->trust_region_strategy != SWF_LEVENBERG_MARQUARDT) return fail(SWF_E_INVALID, "unknown trust_region_strategy");
    if (opt->composite_root != SWF_ROOT_PIVOTED_CHOLESKY && opt->composite_root != SWF_ROOT_EIGEN) return fail(SWF_E_INVALID, "unknown composite_root");
    b->comp_eigen_root = opt->composite_root == SWF_ROOT_EIGEN;
    if (opt->jacobi_scaling && opt->trust_region_strategy == SWF_DOGLEG && opt->step_mode == SWF_OPTIMIZE)
        return fail(SWF_E_UNSUPPORTED, "jacobi_scaling with the dogleg strategy (the reference sets jacobi_scaling = 0 wherever it selects DOGLEG: R/swf/swf.cpp:26-27)");
    DevBatch& D = b->D;
    Launcher L{ b, to_devopt(opt), b->stream };
    L.export_full = opt->step_mode == SWF_ASSEMBLE_ELIMINATE_ONLY;
    b->L_full = L.export_full || b->min_red > b->rr_nmax || b->max_red > CB_NMAX;
    hipStream_t st = b->stream;
    b->ev_used = 0; b->ev_kind.clear();
    int nlin = 0;
    {
        Launcher::Bracket total(L, SWF_K_TOTAL);
        hipLaunchKernelGGL(k_init, dim3(D.n_win), dim3(256), 0, st, D, L.O);
        auto LIN = [&](int write_S) { L.lin_eval(write_S); L.lin_elim(write_S); nlin++; };
        LIN(1);
        if (opt->step_mode == SWF_ASSEMBLE_ELIMINATE_ONLY) {
            L.reduced();
        } else {
            // Speculative flow (dogleg, no composite factors): the candidate of a proposed step is evaluated WITH its Jacobians — an accepted
            // candidate is the next linearisation point, a rejected dogleg step re-uses the reduced system it came from, an invalid one never
            // gets a candidate (k_dogleg) — so the cost pass at the candidate and the Jacobian pass at the same point that followed it
            // are one pass, and the elimination kernels behind k_decide find the new point's Jacobians in place.  Levenberg-Marquardt
            // re-linearises at the UNCHANGED point after a rejected step (new damping) and keeps the two passes.
            const bool spec = opt->trust_region_strategy == SWF_DOGLEG && !b->n_comp && !b->no_spec;
            L.step_fused = L.step_fuse_ok();
            for (int it = 1; it <= opt->max_num_iterations; it++) {
                L.reduced();
                L.step_rest();
                if (spec) {
                    L.decide_fused = it < opt->max_num_iterations && L.decide_fuse_ok();
                    if (L.step_fused) L.step_eval(); else L.lin_eval(1, true);
                    if (!L.decide_fused) L.decide();
                    if (b->aux) (void)hipEventRecord(b->ev_fork[1], st);          // the auxiliary stream's clique branch starts behind k_decide
                    L.lin_elim(it < opt->max_num_iterations ? 1 : 0); nlin++;
                }
                else {
                    if (L.step_fused) { L.decide_fused = false; L.step_eval(false); L.decide(); } else L.cand_eval();
                    LIN(it < opt->max_num_iterations ? 1 : 0);
                }
            }
        }
        hipLaunchKernelGGL(k_finalize, dim3(D.n_win), dim3(256), 0, st, D, L.O, b->ws_primary);
        D.ws = b->ws_primary;
    }
    HIPCHK(hipGetLastError());
    b->last = swf_timing{};
    b->last.jacobian_bytes = b->jac_bytes; b->last.proj_bytes = b->proj_bytes; b->last.chol_flops = b->chol_flops;
    b->last.lm_schur_flops = b->lm_schur_flops; b->last.n_obs = b->D.n_proj;
    b->last.lm_schur_flops_sym = b->lm_schur_flops_sym; b->last.lm_schur_mfma = b->lm_schur_mfma;
    b->last.n_linearizations = nlin;
    b->last_mode = opt->step_mode; b->mg_valid = false; b->tc_valid = false; b->am_valid = false; b->fx_valid = false; b->fc_valid = false; b->dd_valid = false;      // consumer outputs belong to the previous solve
    return SWF_OK;
}

extern "C" int swf_batch_sync(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "null batch");
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < b->ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, b->ev[2 * i], b->ev[2 * i + 1]) == hipSuccess) {
            int k = b->ev_kind[i];
            b->last.ms[k] += ms; b->last.calls[k]++;
        }
    }
    b->ev_used = 0; b->ev_kind.clear();
    return SWF_OK;
}

// one call for the whole node: every batch's solve is enqueued on its own device first, then all are awaited
extern "C" int swf_solve_batches(swf_batch* const* batches, int32_t n, const swf_options* opt) {
    if (!batches || n <= 0 || !opt) return fail(SWF_E_INVALID, "swf_solve_batches: bad arguments");
    for (int i = 0; i < n; i++) if (!batches[i]) return fail(SWF_E_INVALID, "swf_solve_batches: null batch");
    // Enqueue: one host thread per DEVICE (a solve is ~90 launches; at 64 windows per GPU one thread enqueueing eight devices in turn
    // would put that host time on the critical path).  Batches that share a device are enqueued by that device's thread, in order.
    std::vector<int> rcs((size_t)n, SWF_OK);
    std::vector<std::string> msgs((size_t)n);
    std::vector<int> devs;
    for (int i = 0; i < n; i++) if (std::find(devs.begin(), devs.end(), batches[i]->device) == devs.end()) devs.push_back(batches[i]->device);
    auto enqueue_device = [&](int dev) {
        for (int i = 0; i < n; i++) {
            if (batches[i]->device != dev) continue;
            rcs[(size_t)i] = swf_batch_solve(batches[i], opt);
            if (rcs[(size_t)i] != SWF_OK) msgs[(size_t)i] = g_err;          // (g_err is thread-local: carried back to the caller below)
        }
    };
    if (devs.size() <= 1) enqueue_device(devs.empty() ? 0 : devs[0]);
    else {
        std::vector<std::thread> th;
        for (size_t d = 1; d < devs.size(); d++) th.emplace_back(enqueue_device, devs[d]);
        enqueue_device(devs[0]);
        for (auto& t : th) t.join();
    }
    // Await EVERY batch that was enqueued, whatever happened to the others: a caller that reads states or destroys windows after an
    // error return must not race work still in flight.  The first error is the one reported.
    int rc_all = SWF_OK; std::string msg;
    for (int i = 0; i < n; i++) if (rcs[(size_t)i] != SWF_OK && rc_all == SWF_OK) { rc_all = rcs[(size_t)i]; msg = msgs[(size_t)i]; }
    for (int i = 0; i < n; i++) {
        // (also a batch whose enqueue FAILED: swf_batch_solve can fail at a launch check with dozens of kernels already on its stream)
        if (!batches[i]) continue;
        int rc = swf_batch_sync(batches[i]);
        if (rc != SWF_OK && rc_all == SWF_OK) { rc_all = rc; msg = g_err; }
    }
    if (rc_all != SWF_OK) g_err = msg;
    return rc_all;
}

extern "C" int swf_batch_enable_timing(swf_batch* b, int32_t mask) { if (!b) return fail(SWF_E_INVALID, "null batch"); b->timing = mask; return SWF_OK; }
extern "C" int swf_batch_timing(swf_batch* b, swf_timing* out) { if (!b || !out) return fail(SWF_E_INVALID, "bad arguments"); *out = b->last; return SWF_OK; }

extern "C" int swf_batch_download_state(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "null batch");
    const size_t nx = (size_t)b->D.n_x;
    if (!b->h_x && nx) HIPCHK(hipHostMalloc((void**)&b->h_x, nx * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(b->h_x, b->D.x, nx * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t i = 0; i < b->win.size(); i++) {
        const HostWin& h = b->hw[i];
        const double* p = b->h_x + b->win[i].x_base;
        memcpy(h.pose, p, sizeof(double) * 7 * h.n_pose); p += 7 * h.n_pose;
        memcpy(h.sb, p, sizeof(double) * 9 * h.n_sb); p += 9 * h.n_sb;
        memcpy(h.lm, p, sizeof(double) * 3 * h.n_lm); p += 3 * h.n_lm;
        memcpy(h.sc, p, sizeof(double) * h.n_sc);
    }
    if (b->n_comp) {       // the hidden GNSS epochs are parameter memory too
        std::vector<double> hp((size_t)b->comp_ne * 7), hs((size_t)b->comp_ne * 9);
        HIPCHK(hipMemcpy(hp.data(), b->CA.pose, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hs.data(), b->CA.sb, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < b->win.size(); i++) {
            const HostWin& h = b->hw[i];
            if (!h.comp_ne) continue;
            memcpy(h.comp_pose, hp.data() + (size_t)h.comp_e0 * 7, sizeof(double) * 7 * h.comp_ne);
            memcpy(h.comp_sb, hs.data() + (size_t)h.comp_e0 * 9, sizeof(double) * 9 * h.comp_ne);
        }
    }
    return SWF_OK;
}

extern "C" int swf_batch_summaries(swf_batch* b, swf_summary* out) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || !out) return fail(SWF_E_INVALID, "bad arguments");
    size_t n = b->win.size();
    // (page-locked staging kept by the batch: the traces are 2.4 MB for 512 windows)
    const size_t ws_b = (n * sizeof(WinState) + 63) & ~(size_t)63, tr_b = n * SWF_MAX_TRACE * sizeof(swf_iteration);
    if (b->h_sum_bytes < ws_b + tr_b) {
        if (b->h_sum) (void)hipHostFree(b->h_sum);
        b->h_sum = nullptr; b->h_sum_bytes = 0;
        HIPCHK(hipHostMalloc(&b->h_sum, ws_b + tr_b, hipHostMallocDefault));
        b->h_sum_bytes = ws_b + tr_b;
    }
    WinState* ws = (WinState*)b->h_sum;
    swf_iteration* tr = (swf_iteration*)((char*)b->h_sum + ws_b);
    HIPCHK(hipMemcpyAsync(ws, b->D.ws, n * sizeof(WinState), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(tr, b->D.trace, tr_b, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t i = 0; i < n; i++) {
        swf_summary& s = out[i];
        memset(&s, 0, sizeof(s));
        s.initial_cost = ws[i].initial_cost; s.final_cost = ws[i].x_cost;
        s.minimizer_time_in_seconds = b->last.ms[SWF_K_TOTAL] * 1e-3;
        s.num_successful_steps = ws[i].nsucc; s.num_unsuccessful_steps = ws[i].nunsucc;
        s.num_iterations = ws[i].iter; s.termination = ws[i].status;
        s.reduced_dim = b->win[i].n_red; s.tail_dim = b->hw[i].tail_dim;
        memcpy(s.trace, tr + i * SWF_MAX_TRACE, sizeof(swf_iteration) * SWF_MAX_TRACE);
    }
    return SWF_OK;
}

extern "C" int swf_batch_dims(swf_batch* b, int32_t w, int32_t* n_loc, int32_t* n_e, int32_t* n_red) {
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (n_loc) *n_loc = b->win[w].n_loc; if (n_e) *n_e = b->win[w].n_e; if (n_red) *n_red = b->win[w].n_red;
    return SWF_OK;
}

extern "C" int swf_batch_export_reduced(swf_batch* b, int32_t w, double* S, double* rhs, double* L) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (b->last_mode < 0) return fail(SWF_E_STATE, "export before any solve");
    const WinRec& W = b->win[w];
    size_t n = (size_t)W.n_red;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (S) {
        HIPCHK(hipMemcpy(S, b->D.S + W.S_base, n * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; r++) for (size_t c = r + 1; c < n; c++) S[r * n + c] = S[c * n + r];   // device keeps the lower triangle
    }
    if (rhs) HIPCHK(hipMemcpy(rhs, b->D.rhs + W.loc_base + W.n_e, n * sizeof(double), hipMemcpyDeviceToHost));
    if (L) {
        std::vector<double> Lt((n + 1) * (n + 1));
        HIPCHK(hipMemcpy(Lt.data(), b->D.L + W.Lt_base, Lt.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool rr = b->max_red <= CB_NMAX;      // k_chol_rr4 / k_chol_big write row-major lower, ld = n
        // k_chol_rr4 on a solve path keeps the factor in registers and writes only the block its readers use: the parameter_head
        // tail (from the 16-aligned row / column at or before its start).  Everything else is returned as zero.
        size_t first = 0;
        if (!b->L_full && n <= (size_t)b->rr_nmax) { const size_t td = (size_t)b->hw[w].tail_dim; first = td ? ((n - td) >> 4) << 4 : n; }
        for (size_t r = 0; r < n; r++) for (size_t c = 0; c < n; c++)
            L[r * n + c] = (c <= r && c >= first) ? (rr ? Lt[r * n + c] : Lt[c * (n + 1) + r]) : 0.0;
    }
    return SWF_OK;
}

extern "C" int swf_batch_marginalize(swf_batch* b, double eps, int32_t form) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || (form != SWF_PRIOR_EIGEN && form != SWF_PRIOR_CHOLESKY) || !(eps >= 0.0)) return fail(SWF_E_INVALID, "swf_batch_marginalize: bad arguments");
    if (b->last_mode != SWF_ASSEMBLE_ELIMINATE_ONLY) return fail(SWF_E_STATE, "swf_batch_marginalize needs a preceding solve with step_mode = SWF_ASSEMBLE_ELIMINATE_ONLY");
    if (b->max_red > CB_NMAX) return fail(SWF_E_UNSUPPORTED, "marginalisation needs the row-major Cholesky factor (n_red <= 640)");
    int nw = (int)b->win.size(), ldn = 1;
    for (int w = 0; w < nw; w++) ldn = std::max(ldn, b->hw[w].tail_dim);
    if (form == SWF_PRIOR_EIGEN && ldn > MG_BIGN) return fail(SWF_E_UNSUPPORTED, "eigen square root: parameter_head tail larger than 640 dimensions (use SWF_PRIOR_CHOLESKY)");
    b->mg_ld = ldn;
    if (!b->mg_A) {
        std::vector<int> td(nw);
        for (int w = 0; w < nw; w++) td[w] = b->hw[w].tail_dim;
        const int* tdp = nullptr;
        int rc = b->pool.put(td, &tdp);
        b->mg_tail = (int*)tdp;
        rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->mg_A); rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->mg_J);
        rc |= b->pool.zeros((size_t)nw * ldn, &b->mg_b); rc |= b->pool.zeros((size_t)nw * ldn, &b->mg_r0); rc |= b->pool.zeros((size_t)nw * ldn, &b->mg_w);
        rc |= b->pool.zeros((size_t)nw, &b->mg_rank);
        rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->mg_resM); rc |= b->pool.zeros((size_t)nw * ldn, &b->mg_resb); rc |= b->pool.zeros((size_t)nw, &b->mg_resok);
        if (rc) return fail(SWF_E_NODEVICE, "device allocation failed");
    }
    const bool big = form == SWF_PRIOR_EIGEN && ldn > MG_MAXN;
    if (big && !b->mg_M && b->pool.zeros((size_t)nw * ldn * ldn, &b->mg_M)) return fail(SWF_E_NODEVICE, "device allocation failed");
    // windows whose factorisation broke down in the tail (a marginal that is singular on the kept states): partial factorisation +
    // rank-revealing factor of A; every other window leaves this kernel at once
    // rows of V the pivoted Cholesky (d_pivoted_chol) takes per pass over its pool: what 150 KB of LDS leave next to 25 rows of the tail
    const int mg_rc = std::max(16, std::min(ldn, (int)((150 * 1024 / 8 - (RS_POOL + 1) * (long)ldn) / RS_POOL)));
    const int force = getenv("SWF_FORCE_MARG_RESCUE") ? 1 : 0;      // (read once per call, outside the sweep loop: the tests toggle it between two calls on one batch)      // testing aid: healthy windows through the rank-deficient path too
    if (form == SWF_PRIOR_EIGEN)
        {
            // dynamic LDS: the 16-column panel over (n_red + 1) rows, later the pivoted Cholesky's pool (24 rows of the tail), its diagonal
            // and the staging of 24 x rc entries of V^T (rc = rows of V per pass: all of them up to 400 dimensions)
            const size_t l1 = (size_t)(b->max_red + 1) * (RS_NB + 1), l2 = (size_t)(RS_POOL + 1) * (size_t)ldn + (size_t)RS_POOL * (size_t)mg_rc;
            const size_t lds = sizeof(double) * std::max(l1, l2);
            if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_marg_rescue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);      // (up to 150 KB at 640 dimensions)
            hipLaunchKernelGGL(k_marg_rescue, dim3(nw), dim3(1024), lds, b->stream, b->D, (const int*)b->mg_tail, ldn, b->mg_resM, b->mg_resb, b->mg_resok, force, eps, b->mg_J, mg_rc);
        }
    hipLaunchKernelGGL(k_marginalize<false>, dim3(nw), dim3(MG_NT), 0, b->stream, b->D, (const int*)b->mg_tail, eps, (int)form, ldn,
                       b->mg_A, b->mg_b, b->mg_J, b->mg_r0, b->mg_w, b->mg_rank, (double*)nullptr,
                       (const double*)b->mg_resM, (const double*)b->mg_resb, (const int*)b->mg_resok, force, 0, (int*)nullptr);
    if (form == SWF_PRIOR_CHOLESKY)      // A = J^T J, one thread per entry (full-length sums: the zeros of the triangular J add exact zeros)
        hipLaunchKernelGGL(k_marg_gram, dim3((ldn * ldn + 255) / 256, nw), dim3(256), 0, b->stream, (const int*)b->mg_tail, ldn, (const double*)b->mg_J, b->mg_A, (const int*)nullptr);
    if (big) {
        // large tails: set-up, the block-Jacobi sweeps over many workgroups (fixed launch schedule; converged windows return at once), write-out
        if (!b->mg_rot && (b->pool.zeros((size_t)nw * MG_SWEEPS, &b->mg_rot) || b->pool.zeros((size_t)nw, &b->mg_bjok) || b->pool.zeros((size_t)nw * 2, &b->mg_crit))) return fail(SWF_E_NODEVICE, "device allocation failed");
        HIPCHK(hipMemsetAsync(b->mg_rot, 0, (size_t)nw * MG_SWEEPS * sizeof(int), b->stream));
        HIPCHK(hipMemsetAsync(b->mg_crit, 0, (size_t)nw * 2 * sizeof(unsigned long long), b->stream));
        auto phase = [&](int ph) {
            hipLaunchKernelGGL(k_marginalize<true>, dim3(nw), dim3(MG_NT), 0, b->stream, b->D, (const int*)b->mg_tail, eps, (int)form, ldn,
                               b->mg_A, b->mg_b, b->mg_J, b->mg_r0, b->mg_w, b->mg_rank, b->mg_M,
                               (const double*)b->mg_resM, (const double*)b->mg_resb, (const int*)b->mg_resok, force, ph, b->mg_bjok);
        };
        {
            phase(1);
            hipLaunchKernelGGL(k_marg_gram, dim3((ldn * ldn + 255) / 256, nw), dim3(256), 0, b->stream, (const int*)b->mg_tail, ldn, (const double*)b->mg_M, b->mg_A, (const int*)b->mg_bjok);
            {
                // the Jacobi preconditioner: pivoted Cholesky of A into the G slab (9 sweeps instead of 16 at the 263-dimension tail)
                const size_t lds = sizeof(double) * ((size_t)(RS_POOL + 1) * (size_t)ldn + (size_t)RS_POOL * (size_t)mg_rc);
                if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_marg_pchol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL(k_marg_pchol, dim3(nw), dim3(1024), lds, b->stream, (const int*)b->mg_tail, ldn, (const double*)b->mg_A, b->mg_resM, b->mg_M, (const int*)b->mg_bjok, mg_rc, eps);
            }
            // block size by window: 8 columns up to 576 dimensions (17 workgroups per launch at 263 dimensions, 8 inner steps each; 16-column
            // blocks halve the launches but leave a step to 9 workgroups whose 16 waves share 4 SIMDs: 49 us per launch against 16), 4 above.
            // One launch schedule per class, sized by the class's largest tail; every window follows its own round-robin inside it.
            int ldA = 0, ldB = 0;
            for (int w = 0; w < nw; w++) { const int t = b->hw[w].tail_dim; if (t > MG_MAXN && t <= 576) ldA = std::max(ldA, t); else if (t > 576) ldB = std::max(ldB, t); }
            std::vector<int> hrot((size_t)nw * MG_SWEEPS);
            // from the sixth sweep on, one look at the rotation counts per sweep: 30 us of synchronisation against the 34 launches of a
            // 263-dimension sweep (0.55 ms) that a check every fourth sweep ran up to three times too often
            const int mg_first_check = 6;
            for (int sweep = 0; sweep < MG_SWEEPS; sweep++) {
                if (sweep >= mg_first_check) {
                    // every four sweeps: has every window reported a sweep without rotations?  (the launches of a converged window return
                    // at once, but a 263-dimension sweep is still 34 launches)
                    HIPCHK(hipMemcpyAsync(hrot.data(), b->mg_rot, hrot.size() * sizeof(int), hipMemcpyDeviceToHost, b->stream));
                    HIPCHK(hipStreamSynchronize(b->stream));
                    bool all = true;
                    for (int w = 0; w < nw && all; w++) { bool done = false; for (int k = 0; k < sweep; k++) done = done || hrot[(size_t)w * MG_SWEEPS + k] == 0; all = done; }
                    if (all) break;
                }
#define BJ_LAUNCH(BS_, LDM_, NR_) hipLaunchKernelGGL((k_marg_bj<BS_, LDM_, NR_>), grid, dim3(1024), 0, b->stream, (const int*)b->mg_tail, ldn, b->mg_M, b->mg_rot, b->mg_crit, (const int*)b->mg_bjok, sweep, st)
                if (ldA) {
                    const int bs = 8, nbe = ((ldA + bs - 1) / bs + 1) & ~1;
                    for (int st = -1; st < nbe - 1; st++) {
                        dim3 grid(nbe / 2, nw);
                        if (ldA <= 320) BJ_LAUNCH(8, 576, 5);
                        else BJ_LAUNCH(8, 576, 9);
                    }
                }
                if (ldB) {
                    const int nbe = ((ldB + 3) / 4 + 1) & ~1;
                    for (int st = -1; st < nbe - 1; st++) { dim3 grid(nbe / 2, nw); BJ_LAUNCH(4, 640, 10); }
                }
#undef BJ_LAUNCH
                hipLaunchKernelGGL(k_marg_bj_crit, dim3((nw + 63) / 64), dim3(64), 0, b->stream, (const int*)b->mg_tail, nw, b->mg_rot, b->mg_crit, (const int*)b->mg_bjok, sweep);
            }
            phase(2);
        }
    }
    HIPCHK(hipGetLastError());
    b->mg_valid = true; b->mg_host = false;
    return SWF_OK;
}

// ambiguity covariance hand-off: information and covariance of the parameter_head tail from the factor of the last linear solve
extern "C" int swf_batch_tail_covariance(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "swf_batch_tail_covariance: null batch");
    if (b->last_mode < 0) return fail(SWF_E_STATE, "swf_batch_tail_covariance needs a preceding solve");
    if (b->max_red > CB_NMAX) return fail(SWF_E_UNSUPPORTED, "the tail covariance needs the row-major Cholesky factor (n_red <= 640)");
    int nw = (int)b->win.size(), ldn = 1;
    for (int w = 0; w < nw; w++) ldn = std::max(ldn, b->hw[w].tail_dim);
    if (!b->tc_A) {
        std::vector<int> td(nw);
        for (int w = 0; w < nw; w++) td[w] = b->hw[w].tail_dim;
        const int* tdp = nullptr;
        int rc = b->pool.put(td, &tdp);
        b->tc_tail = (int*)tdp;
        rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->tc_A); rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->tc_Q);
        rc |= b->pool.zeros((size_t)nw * ldn * ldn, &b->tc_X); rc |= b->pool.zeros((size_t)nw, &b->tc_rank);
        if (rc) return fail(SWF_E_NODEVICE, "device allocation failed");
    }
    b->tc_ld = ldn;
    hipLaunchKernelGGL(k_tail_cov, dim3(nw), dim3(256), 0, b->stream, b->D, (const int*)b->tc_tail, ldn, b->tc_A, b->tc_Q, b->tc_X, b->tc_rank);
    HIPCHK(hipGetLastError());
    b->tc_valid = true;
    return SWF_OK;
}

extern "C" int swf_batch_get_tail_covariance(swf_batch* b, int32_t w, double* A, double* Qy, int32_t* n_out) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->tc_valid) return fail(SWF_E_STATE, "swf_batch_get_tail_covariance before swf_batch_tail_covariance");
    HIPCHK(hipStreamSynchronize(b->stream));
    size_t n = (size_t)b->hw[w].tail_dim, o2 = (size_t)w * b->tc_ld * b->tc_ld;
    int32_t rk = 0;
    HIPCHK(hipMemcpy(&rk, b->tc_rank + w, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_out) *n_out = rk < 0 ? -1 : (int32_t)n;
    if (rk < 0) return fail(SWF_E_STATE, "tail covariance: the window has no valid factor (failed linear solve or empty tail)");
    if (A) HIPCHK(hipMemcpy(A, b->tc_A + o2, n * n * sizeof(double), hipMemcpyDeviceToHost));
    if (Qy) HIPCHK(hipMemcpy(Qy, b->tc_Q + o2, n * n * sizeof(double), hipMemcpyDeviceToHost));
    return SWF_OK;
}

// the search's device buffers, sized for the most a search may pass (n_windows x 64 pairs)
static int am_alloc(swf_batch* b) {
    if (b->am_rec) return 0;
    const size_t nw = b->win.size();
    int rc = 0;
    rc |= b->pool.zeros(nw + 1, &b->am_first);
    rc |= b->pool.zeros(nw * SWF_LAMBDA_NMAX, &b->am_pairs);
    rc |= b->pool.zeros(nw * (LBD_REC_QB + SWF_LAMBDA_NMAX * SWF_LAMBDA_NMAX), &b->am_rec);
    return rc;
}

// integer ambiguity search (LambdaSearch's numeric core): gather D Qy D^T and D y, LAMBDA with m = 2, ratio test — one k_lambda<true>
extern "C" int swf_batch_ambiguity_search(swf_batch* b, const int32_t* pair_first, const int32_t* pairs, double ratio_threshold) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || !pair_first) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: null argument");
    if (!b->tc_valid) return fail(SWF_E_STATE, "swf_batch_ambiguity_search needs a swf_batch_tail_covariance after the last solve");
    const int nw = (int)b->win.size();
    if (pair_first[0] != 0) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: pair_first[0] must be 0");
    std::vector<int> nb(nw);
    int nmax = 1;
    for (int w = 0; w < nw; w++) {
        nb[w] = pair_first[w + 1] - pair_first[w];
        if (nb[w] < 0) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: pair_first must be non-decreasing");
        if (nb[w] > SWF_LAMBDA_NMAX) return fail(SWF_E_UNSUPPORTED, "swf_batch_ambiguity_search: more than 64 pairs in a window");
        nmax = std::max(nmax, nb[w]);
    }
    const int total = pair_first[nw];
    if (total > 0 && !pairs) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: null pairs");
    std::vector<int4>& pr = b->am_h_pairs;
    pr.assign((size_t)std::max(total, 1), make_int4(0, 0, 0, 0));
    for (int w = 0; w < nw; w++) {
        const HostWin& h = b->hw[w];
        for (int q = pair_first[w]; q < pair_first[w + 1]; q++) {
            const int ta = pairs[2 * q], tb = pairs[2 * q + 1];
            if (ta < 0 || tb < 0 || ta >= h.tail_dim || tb >= h.tail_dim || ta == tb)
                return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: pair index outside the tail, or a == b (window " + std::to_string(w) + ")");
            const int xa = h.tail_x[ta], xb = h.tail_x[tb];
            if (xa < 0 || xb < 0) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search: a pair on a tail block whose size is not 1 (window " + std::to_string(w) + ")");
            pr[q] = make_int4(ta, tb, xa, xb);
        }
    }
    if (am_alloc(b)) return fail(SWF_E_NODEVICE, "device allocation failed");
    b->dd_valid = false;                         // the pair table is this search's from here on
    b->am_h_first.assign(pair_first, pair_first + nw + 1);
    HIPCHK(hipMemcpyAsync(b->am_first, b->am_h_first.data(), (size_t)(nw + 1) * sizeof(int), hipMemcpyHostToDevice, b->stream));
    if (total > 0) HIPCHK(hipMemcpyAsync(b->am_pairs, pr.data(), (size_t)total * sizeof(int4), hipMemcpyHostToDevice, b->stream));
    LambdaArgs A{};
    A.n_prob = nw; A.ld = SWF_LAMBDA_NMAX; A.m = 2; A.ldl = std::max(1, nmax) | 1;
    A.pair_first = b->am_first; A.pairs = b->am_pairs;
    A.tcQ = b->tc_Q; A.tc_ld = b->tc_ld; A.tc_n = b->tc_tail; A.tc_rank = b->tc_rank; A.x = b->D.x;
    A.rec = b->am_rec; A.rec_ld = LBD_REC_QB + nmax * nmax; A.thr = ratio_threshold;
    b->am_valid = false; b->fx_valid = false;
    const int rc = swf_internal_lambda_launch(A, true, b->stream);
    if (rc) return rc;
    b->am_nb = nb; b->am_rec_ld = A.rec_ld;
    b->am_valid = true; b->am_host = false; b->am_selected = false;
    return SWF_OK;
}

// ---- the pairs chosen on the device (k_dd_select<true>) and the search on them (k_lambda<true, true>)
static size_t dd_up8(size_t n) { return (n + 7) & ~(size_t)7; }
struct DdLayout {           // byte offsets in dd_in / dd_out for nw windows, ne epochs, no observations
    size_t gate, efirst, ofirst, obs, xidx, in_bytes, cost, refs, role, out_bytes;
    DdLayout(size_t nw, size_t ne, size_t no) {
        gate = 0; efirst = gate + nw * sizeof(double); ofirst = dd_up8(efirst + (nw + 1) * sizeof(int)); obs = dd_up8(ofirst + (ne + 1) * sizeof(int));
        xidx = dd_up8(obs + std::max<size_t>(no, 1) * 2 * sizeof(int)); in_bytes = dd_up8(xidx + std::max<size_t>(no, 1) * sizeof(int));
        cost = 0; refs = std::max<size_t>(no, 1) * sizeof(double); role = dd_up8(refs + std::max<size_t>(ne, 1) * DDS_CLASSES * sizeof(int));
        out_bytes = dd_up8(role + std::max<size_t>(no, 1));
    }
};

extern "C" int swf_batch_select_ambiguity_pairs(swf_batch* b, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs, const double* gate) {
    DeviceGuard dg_(b ? b->device : -1);
    const char* who = "swf_batch_select_ambiguity_pairs";
    if (!b || !epoch_first || !obs_first || !gate) return fail(SWF_E_INVALID, std::string(who) + ": null argument");
    if (b->last_mode < 0) return fail(SWF_E_STATE, std::string(who) + " needs a preceding solve");
    const int nw = (int)b->win.size();
    std::vector<int32_t> tail((size_t)nw);
    for (int w = 0; w < nw; w++) tail[(size_t)w] = b->hw[w].tail_dim;
    const int chk = swf_internal_dd_select_check(who, nw, epoch_first, obs_first, obs, tail.data(), gate);
    if (chk) return chk;
    const int ne = epoch_first[nw], no = obs_first[ne];
    const DdLayout L((size_t)nw, (size_t)ne, (size_t)no);
    // validated into a local staging area: a refused call leaves the previous selection as it was
    std::vector<char> in(L.in_bytes, 0);
    memcpy(in.data() + L.gate, gate, (size_t)nw * sizeof(double));
    memcpy(in.data() + L.efirst, epoch_first, (size_t)(nw + 1) * sizeof(int));
    memcpy(in.data() + L.ofirst, obs_first, (size_t)(ne + 1) * sizeof(int));
    if (no) memcpy(in.data() + L.obs, obs, (size_t)no * 2 * sizeof(int));
    int* xi = (int*)(in.data() + L.xidx);
    for (int w = 0; w < nw; w++) {
        const HostWin& h = b->hw[w];
        for (int i = obs_first[epoch_first[w]]; i < obs_first[epoch_first[w + 1]]; i++) {
            xi[i] = h.tail_x[(size_t)obs[2 * (size_t)i + 1]];
            if (xi[i] < 0) return fail(SWF_E_INVALID, std::string(who) + ": an observation on a tail block whose size is not 1 (window " + std::to_string(w) + ")");
        }
    }
    if (am_alloc(b)) return fail(SWF_E_NODEVICE, "device allocation failed");
    if (!b->dd_pairs) {
        int rc = 0;
        rc |= b->pool.zeros((size_t)nw * SWF_LAMBDA_NMAX * 2, &b->dd_pairs); rc |= b->pool.zeros((size_t)nw * 4, &b->dd_counts); rc |= b->pool.zeros((size_t)nw, &b->dd_npair);
        if (rc) return fail(SWF_E_NODEVICE, "device allocation failed");
    }
    if (L.in_bytes > b->dd_in_cap || L.out_bytes > b->dd_out_cap) {      // (hipFree waits for the work that still reads the old buffers)
        if (b->dd_in) (void)hipFree(b->dd_in);
        if (b->dd_out) (void)hipFree(b->dd_out);
        b->dd_in = b->dd_out = nullptr; b->dd_in_cap = b->dd_out_cap = 0; b->dd_valid = false;
        HIPCHK(hipMalloc((void**)&b->dd_in, L.in_bytes * 2));
        HIPCHK(hipMalloc((void**)&b->dd_out, L.out_bytes * 2));
        b->dd_in_cap = L.in_bytes * 2; b->dd_out_cap = L.out_bytes * 2;
    }
    if (!b->tc_tail && !b->dd_tail) {            // the tail dimensions on the device (swf_batch_tail_covariance keeps its own copy likewise)
        std::vector<int> td(tail.begin(), tail.end());
        if (b->pool.put(td, &b->dd_tail)) return fail(SWF_E_NODEVICE, "device allocation failed");
    }
    // from here on the pair table and the selection buffers belong to this call
    b->dd_valid = false; b->am_valid = false; b->fx_valid = false;
    b->dd_h_in.swap(in); b->dd_ne = ne; b->dd_no = no;
    HIPCHK(hipMemcpyAsync(b->dd_in, b->dd_h_in.data(), L.in_bytes, hipMemcpyHostToDevice, b->stream));
    DdSelectArgs A{};
    A.n_windows = nw;
    A.gate = (const double*)(b->dd_in + L.gate); A.epoch_first = (const int*)(b->dd_in + L.efirst); A.obs_first = (const int*)(b->dd_in + L.ofirst);
    A.obs = (const int*)(b->dd_in + L.obs); A.xidx = (const int*)(b->dd_in + L.xidx);
    A.tail = b->tc_tail ? b->tc_tail : b->dd_tail; A.x = b->D.x;
    A.pairs = b->dd_pairs; A.counts = b->dd_counts; A.pair_count = b->dd_npair;
    A.cost = (double*)(b->dd_out + L.cost); A.refs = (int*)(b->dd_out + L.refs); A.role = (unsigned char*)(b->dd_out + L.role);
    A.am_pairs = b->am_pairs; A.am_first = b->am_first;
    const int rc = swf_internal_dd_select_launch(A, true, b->stream);
    if (rc) return rc;
    b->dd_valid = true; b->dd_host = false;
    return SWF_OK;
}

// one transfer per array: the selection of every window on the host
static int dd_fetch(swf_batch* b) {
    if (b->dd_host) return SWF_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    const size_t nw = b->win.size();
    const DdLayout L(nw, (size_t)b->dd_ne, (size_t)b->dd_no);
    b->dd_h_pairs.resize(nw * SWF_LAMBDA_NMAX * 2); b->dd_h_counts.resize(nw * 4); b->dd_h_out.resize(L.out_bytes);
    HIPCHK(hipMemcpy(b->dd_h_pairs.data(), b->dd_pairs, b->dd_h_pairs.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b->dd_h_counts.data(), b->dd_counts, b->dd_h_counts.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (b->dd_ne) HIPCHK(hipMemcpy(b->dd_h_out.data() + L.refs, b->dd_out + L.refs, (size_t)b->dd_ne * DDS_CLASSES * sizeof(int), hipMemcpyDeviceToHost));
    if (b->dd_no) {
        HIPCHK(hipMemcpy(b->dd_h_out.data() + L.cost, b->dd_out + L.cost, (size_t)b->dd_no * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->dd_h_out.data() + L.role, b->dd_out + L.role, (size_t)b->dd_no, hipMemcpyDeviceToHost));
    }
    b->dd_host = true;
    return SWF_OK;
}

extern "C" int swf_batch_get_ambiguity_pairs(swf_batch* b, int32_t w, int32_t* pairs, int32_t* counts, int32_t* refs, double* cost, uint8_t* role) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->dd_valid) return fail(SWF_E_STATE, "swf_batch_get_ambiguity_pairs before swf_batch_select_ambiguity_pairs (or after a new solve, state upload or reset)");
    const int rc = dd_fetch(b);
    if (rc) return rc;
    const size_t nw = b->win.size();
    const DdLayout L(nw, (size_t)b->dd_ne, (size_t)b->dd_no);
    const int* ef = (const int*)(b->dd_h_in.data() + L.efirst); const int* of = (const int*)(b->dd_h_in.data() + L.ofirst);
    const size_t e0 = (size_t)ef[w], e1 = (size_t)ef[w + 1], o0 = (size_t)of[e0], o1 = (size_t)of[e1];
    if (pairs) memcpy(pairs, b->dd_h_pairs.data() + (size_t)w * SWF_LAMBDA_NMAX * 2, SWF_LAMBDA_NMAX * 2 * sizeof(int));
    if (counts) memcpy(counts, b->dd_h_counts.data() + (size_t)w * 4, 4 * sizeof(int));
    if (refs && e1 > e0) memcpy(refs, b->dd_h_out.data() + L.refs + e0 * DDS_CLASSES * sizeof(int), (e1 - e0) * DDS_CLASSES * sizeof(int));
    if (cost && o1 > o0) memcpy(cost, b->dd_h_out.data() + L.cost + o0 * sizeof(double), (o1 - o0) * sizeof(double));
    if (role && o1 > o0) memcpy(role, b->dd_h_out.data() + L.role + o0, o1 - o0);
    return SWF_OK;
}

extern "C" int swf_batch_ambiguity_search_selected(swf_batch* b, double ratio_threshold) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "swf_batch_ambiguity_search_selected: null batch");
    if (!b->dd_valid) return fail(SWF_E_STATE, "swf_batch_ambiguity_search_selected needs a swf_batch_select_ambiguity_pairs after the last solve");
    if (!b->tc_valid) return fail(SWF_E_STATE, "swf_batch_ambiguity_search_selected needs a swf_batch_tail_covariance after the last solve");
    const int nw = (int)b->win.size();
    int nmax = 1;                // a window appends at most one pair per tail coordinate (each pair marks a new coordinate used)
    for (int w = 0; w < nw; w++) nmax = std::max(nmax, std::min(b->hw[w].tail_dim, (int)SWF_LAMBDA_NMAX));
    LambdaArgs A{};
    A.n_prob = nw; A.ld = SWF_LAMBDA_NMAX; A.m = 2; A.ldl = nmax | 1;
    A.pair_first = b->am_first; A.pairs = b->am_pairs; A.pair_count = b->dd_npair;
    A.tcQ = b->tc_Q; A.tc_ld = b->tc_ld; A.tc_n = b->tc_tail; A.tc_rank = b->tc_rank; A.x = b->D.x;
    A.rec = b->am_rec; A.rec_ld = LBD_REC_QB + nmax * nmax; A.thr = ratio_threshold;
    b->am_valid = false; b->fx_valid = false;
    const int rc = swf_internal_lambda_launch(A, true, b->stream);
    if (rc) return rc;
    b->am_nb.assign((size_t)nw, 0); b->am_rec_ld = A.rec_ld;          // the counts are on the device: filled when the host first reads them
    b->am_valid = true; b->am_host = false; b->am_selected = true; b->am_sel_host = false;
    return SWF_OK;
}

// after a selected search: the pairs and the counts the search ran on, as swf_batch_ambiguity_search would have staged them
static int am_selected_fetch(swf_batch* b) {
    if (b->am_sel_host) return SWF_OK;
    const int rc = dd_fetch(b);              // (a selection newer than the search would have invalidated the search)
    if (rc) return rc;
    const int nw = (int)b->win.size();
    b->am_h_first.resize((size_t)nw + 1); b->am_h_pairs.assign((size_t)nw * SWF_LAMBDA_NMAX, make_int4(0, 0, 0, 0)); b->am_nb.assign((size_t)nw, 0);
    for (int w = 0; w <= nw; w++) b->am_h_first[(size_t)w] = w * SWF_LAMBDA_NMAX;
    for (int w = 0; w < nw; w++) {
        const int* c = b->dd_h_counts.data() + (size_t)w * 4;
        const int n = c[3] == SWF_DDSEL_OK ? c[0] : 0;
        b->am_nb[(size_t)w] = n;
        const HostWin& h = b->hw[w];
        for (int i = 0; i < n; i++) {
            const int* q = b->dd_h_pairs.data() + ((size_t)w * SWF_LAMBDA_NMAX + i) * 2;
            b->am_h_pairs[(size_t)w * SWF_LAMBDA_NMAX + i] = make_int4(q[0], q[1], h.tail_x[(size_t)q[0]], h.tail_x[(size_t)q[1]]);
        }
    }
    b->am_sel_host = true;
    return SWF_OK;
}

extern "C" int swf_batch_get_ambiguity_fix(swf_batch* b, int32_t w, double* F, double* s, double* ratio, int32_t* fixed,
                                           double* Qb, double* bf, int32_t* n_b, int32_t* info) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->am_valid) return fail(SWF_E_STATE, "swf_batch_get_ambiguity_fix before swf_batch_ambiguity_search (or after a new solve)");
    if (!b->am_host) {          // the first getter after a search copies every window's record in one transfer
        HIPCHK(hipStreamSynchronize(b->stream));
        b->h_am.resize((size_t)b->win.size() * b->am_rec_ld);
        HIPCHK(hipMemcpy(b->h_am.data(), b->am_rec, b->h_am.size() * sizeof(double), hipMemcpyDeviceToHost));
        b->am_host = true;
    }
    const double* r = b->h_am.data() + (size_t)w * b->am_rec_ld;
    const size_t n = b->am_selected ? (size_t)r[LBD_REC_INFO + 2] : (size_t)b->am_nb[w];      // a selected search: the count is the device's
    if (n_b) *n_b = (int32_t)n;
    if (F) for (int j = 0; j < 2; j++) memcpy(F + j * n, r + LBD_REC_F + j * SWF_LAMBDA_NMAX, n * sizeof(double));
    if (s) memcpy(s, r + LBD_REC_S, 2 * sizeof(double));
    if (ratio) memcpy(ratio, r + LBD_REC_RATIO, 2 * sizeof(double));
    if (fixed) *fixed = (int32_t)r[LBD_REC_INFO + 1];
    if (Qb) memcpy(Qb, r + LBD_REC_QB, n * n * sizeof(double));
    if (bf) memcpy(bf, r + LBD_REC_BF, n * sizeof(double));
    if (info) *info = (int32_t)r[LBD_REC_INFO];
    return SWF_OK;
}

// fix and hold: the accepted integers of the last search folded into a linear prior of every window (k_fix_prior<true>)
extern "C" int swf_batch_fix_prior(swf_batch* b, const int32_t* prior_sel, const int32_t* n_use, const uint8_t* enable, int32_t ignore_ratio,
                                   int32_t scalars_at_zero, double istd, double eps, int32_t form) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "swf_batch_fix_prior: null batch");
    if (!b->am_valid) return fail(SWF_E_STATE, "swf_batch_fix_prior needs a swf_batch_ambiguity_search after the last solve");
    if (form != SWF_PRIOR_EIGEN && form != SWF_PRIOR_CHOLESKY) return fail(SWF_E_INVALID, "swf_batch_fix_prior: form must be SWF_PRIOR_EIGEN or SWF_PRIOR_CHOLESKY");
    if (!std::isfinite(istd) || !(istd > 0.0) || !std::isfinite(eps) || eps < 0.0) return fail(SWF_E_INVALID, "swf_batch_fix_prior: istd must be positive and eps non-negative");
    if (b->am_selected) { const int frc = am_selected_fetch(b); if (frc) return frc; }      // the one synchronisation of the device chain
    const int nw = (int)b->win.size();
    // validated into locals and copied into the batch's staging on success: a refused call leaves the previous call's tables as they were
    std::vector<FixWin> fw((size_t)nw, FixWin{ 0, 0, 0, 0 });
    std::vector<int> tc;
    std::vector<int> sel((size_t)nw, -1);
    int cap_n = 1, cap_x = 1;
    for (int w = 0; w < nw; w++) for (const HostWin::LinPrior& lp : b->hw[w].lin_prior) if (lp.dim <= FXP_MAXN) { cap_n = std::max(cap_n, lp.dim); cap_x = std::max(cap_x, lp.gsum); }
    for (int w = 0; w < nw; w++) {
        const HostWin& h = b->hw[w];
        const int np_all = b->am_nb[w];
        const int k = prior_sel ? prior_sel[w] : 0;
        const bool en = !enable || enable[w];
        int nu = n_use ? n_use[w] : np_all;
        if (nu < 0) return fail(SWF_E_INVALID, "swf_batch_fix_prior: n_use < 0 (window " + std::to_string(w) + ")");
        nu = std::min(nu, np_all);
        fw[w].col0 = (int)tc.size(); fw[w].n_use = nu; fw[w].enable = (en && nu > 0) ? 1 : 0;
        tc.resize(tc.size() + (size_t)h.tail_dim, -1);
        if (!fw[w].enable) continue;             // nothing of this window is read
        if (k < 0 || k >= (int)h.lin_prior.size())
            return fail(SWF_E_INVALID, "swf_batch_fix_prior: prior_sel names no linear prior of the window (a composite factor's record cannot be fixed) (window " + std::to_string(w) + ")");
        const HostWin::LinPrior& lp = h.lin_prior[(size_t)k];
        if (lp.dim > FXP_MAXN) return fail(SWF_E_UNSUPPORTED, "swf_batch_fix_prior: prior of more than 140 dimensions (window " + std::to_string(w) + ")");
        fw[w].gf = lp.gf; sel[w] = k;
        int* tcw = tc.data() + fw[w].col0;
        for (int t = 0; t < h.tail_dim; t++) if (h.tail_x[t] >= 0)
            for (int c = 0; c < lp.dim; c++) if (lp.col_x[c] == h.tail_x[t]) { tcw[t] = c; break; }
        // the rows this window will form: every coordinate kept by the prior, no coordinate twice, no group of one row
        std::vector<int32_t> rows;
        const int4* pr = b->am_h_pairs.data() + b->am_h_first[w];
        for (int i = 0; i < nu; i++) {
            bool first = true;
            for (int j = 0; j < i; j++) if (pr[j].y == pr[i].y) { first = false; break; }
            if (tcw[pr[i].x] < 0 || tcw[pr[i].y] < 0)
                return fail(SWF_E_INVALID, "swf_batch_fix_prior: a pair names a tail coordinate whose block the prior does not keep (window " + std::to_string(w) + ")");
            if (first) { rows.push_back(tcw[pr[i].y]); rows.push_back(pr[i].y); }
            rows.push_back(tcw[pr[i].x]); rows.push_back(pr[i].y);
        }
        if ((int)rows.size() / 2 > lp.dim) return fail(SWF_E_INVALID, "swf_batch_fix_prior: more rows than coordinates (window " + std::to_string(w) + ")");
        const int rc = swf_internal_fix_rows_check(lp.dim, (int)rows.size() / 2, rows.data(), "swf_batch_fix_prior");
        if (rc) return rc;
    }
    if (!b->fx_win) {
        int total_tail = 0;
        for (int w = 0; w < nw; w++) total_tail += b->hw[w].tail_dim;
        int rc = 0;
        b->fx_ldn = cap_n; b->fx_ldx = cap_x;
        rc |= b->pool.zeros((size_t)nw, &b->fx_win); rc |= b->pool.zeros((size_t)total_tail, &b->fx_tailcol);
        rc |= b->pool.zeros((size_t)nw * cap_n * cap_n, &b->fx_A); rc |= b->pool.zeros((size_t)nw * cap_n * cap_n, &b->fx_J);
        rc |= b->pool.zeros((size_t)nw * cap_n, &b->fx_b); rc |= b->pool.zeros((size_t)nw * cap_n, &b->fx_r0); rc |= b->pool.zeros((size_t)nw * cap_n, &b->fx_eig);
        rc |= b->pool.zeros((size_t)nw * cap_x, &b->fx_x0); rc |= b->pool.zeros((size_t)nw, &b->fx_rank); rc |= b->pool.zeros((size_t)nw, &b->fx_applied);
        if (rc) return fail(SWF_E_NODEVICE, "device allocation failed");
    }
    b->fx_valid = false;                         // from here on the device tables belong to this call
    b->fx_h_win = fw; b->fx_h_tailcol = tc;      // (copied, not swapped: the staging keeps its storage from call to call, like am_h_pairs)
    HIPCHK(hipMemcpyAsync(b->fx_win, b->fx_h_win.data(), (size_t)nw * sizeof(FixWin), hipMemcpyHostToDevice, b->stream));
    if (!b->fx_h_tailcol.empty()) HIPCHK(hipMemcpyAsync(b->fx_tailcol, b->fx_h_tailcol.data(), b->fx_h_tailcol.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    FixPriorArgs P{};
    P.n_prob = nw; P.form = form; P.istd = istd; P.eps = eps;
    P.A = b->fx_A; P.b = b->fx_b; P.Jn = b->fx_J; P.r0 = b->fx_r0; P.eig = b->fx_eig; P.rank = b->fx_rank;
    P.fw = b->fx_win; P.tailcol = b->fx_tailcol; P.pair_first = b->am_first; P.pairs = b->am_pairs; P.rec = b->am_rec; P.rec_ld = b->am_rec_ld;
    P.ignore_ratio = ignore_ratio ? 1 : 0; P.scalars_at_zero = scalars_at_zero ? 1 : 0; P.ldn = b->fx_ldn; P.ldx = b->fx_ldx;
    P.x0n = b->fx_x0; P.applied = b->fx_applied;
    const int rc = swf_internal_fix_prior_launch(P, b->D, true, b->stream);
    if (rc) return rc;
    b->fx_args = P; b->fx_sel = sel;
    b->fx_valid = true; b->fx_host = false;
    return SWF_OK;
}

extern "C" int swf_batch_get_fixed_prior(swf_batch* b, int32_t w, double* A, double* bv, double* J, double* r0, double* x0, double* eig,
                                         int32_t* n, int32_t* rank, int32_t* applied) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->fx_valid) return fail(SWF_E_STATE, "swf_batch_get_fixed_prior before swf_batch_fix_prior (or after a new solve)");
    if (!b->fx_host) {          // the first getter after a fix copies every window's results, one transfer per array
        HIPCHK(hipStreamSynchronize(b->stream));
        const size_t nw = b->win.size(), l1 = (size_t)b->fx_ldn, lx = (size_t)b->fx_ldx;
        b->h_fxA.resize(nw * l1 * l1); b->h_fxJ.resize(nw * l1 * l1); b->h_fxb.resize(nw * l1); b->h_fxr0.resize(nw * l1); b->h_fxeig.resize(nw * l1);
        b->h_fxx0.resize(nw * lx); b->h_fxrank.resize(nw); b->h_fxapplied.resize(nw);
        HIPCHK(hipMemcpy(b->h_fxA.data(), b->fx_A, b->h_fxA.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxJ.data(), b->fx_J, b->h_fxJ.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxb.data(), b->fx_b, b->h_fxb.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxr0.data(), b->fx_r0, b->h_fxr0.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxeig.data(), b->fx_eig, b->h_fxeig.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxx0.data(), b->fx_x0, b->h_fxx0.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxrank.data(), b->fx_rank, nw * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b->h_fxapplied.data(), b->fx_applied, nw * sizeof(int), hipMemcpyDeviceToHost));
        b->fx_host = true;
    }
    const int ap = b->h_fxapplied[(size_t)w];
    if (applied) *applied = ap;
    if (rank) *rank = b->h_fxrank[(size_t)w];
    const int k = b->fx_sel[(size_t)w];
    const size_t dim = k >= 0 ? (size_t)b->hw[w].lin_prior[(size_t)k].dim : 0, gsum = k >= 0 ? (size_t)b->hw[w].lin_prior[(size_t)k].gsum : 0;
    if (n) *n = (int32_t)dim;
    if (!ap) return SWF_OK;                      // a window that was not applied has no results: nothing is written
    const size_t l1 = (size_t)b->fx_ldn, o2 = (size_t)w * l1 * l1, o1 = (size_t)w * l1;
    if (A) memcpy(A, b->h_fxA.data() + o2, dim * dim * sizeof(double));
    if (J) memcpy(J, b->h_fxJ.data() + o2, dim * dim * sizeof(double));
    if (bv) memcpy(bv, b->h_fxb.data() + o1, dim * sizeof(double));
    if (r0) memcpy(r0, b->h_fxr0.data() + o1, dim * sizeof(double));
    if (eig) memcpy(eig, b->h_fxeig.data() + o1, dim * sizeof(double));
    if (x0) memcpy(x0, b->h_fxx0.data() + (size_t)w * b->fx_ldx, gsum * sizeof(double));
    return SWF_OK;
}

extern "C" int swf_batch_install_fixed_prior(swf_batch* b) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "swf_batch_install_fixed_prior: null batch");
    if (!b->fx_valid) return fail(SWF_E_STATE, "swf_batch_install_fixed_prior before swf_batch_fix_prior (or after a new solve)");
    return swf_internal_fix_install_launch(b->fx_args, b->D, b->stream);
}

// post-solve feature check (OutliersRejection + the depth sign of Double2Vector): k_feature_err, k_feature_compact
extern "C" int swf_batch_check_features(swf_batch* b, double max_mean_error) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b) return fail(SWF_E_INVALID, "swf_batch_check_features: null batch");
    if (!std::isfinite(max_mean_error) || max_mean_error < 0) return fail(SWF_E_INVALID, "swf_batch_check_features: max_mean_error must be finite and >= 0");
    const int nw = (int)b->win.size();
    if (!b->fc_built) {          // symbolic phase of the check, once per batch
        std::vector<FeatWinSrc> src(nw);
        for (int w = 0; w < nw; w++) src[w] = b->hw[w].feat;
        FeatTables T;
        const int rc0 = swf_internal_feature_tables(src, T);
        if (rc0) return rc0;
        const size_t nf = T.f_obs0.size() - 1;
        FeatArgs& A = b->fc;
        int rc = 0;
        rc |= b->pool.put(T.o_a, &A.o_a); rc |= b->pool.put(T.o_b, &A.o_b); rc |= b->pool.put(T.o_uv, &A.o_uv);
        rc |= b->pool.put(T.f_obs0, &A.f_obs0); rc |= b->pool.put(T.f_pi, &A.f_pi); rc |= b->pool.put(T.blk, &A.blk);
        rc |= b->pool.put(T.w_feat0, &A.w_feat0); rc |= b->pool.put(T.w_cst, &A.w_cst);
        // one output buffer, 8-byte fields first: mean_err [nf] | depth [nf] | n_obs [nf] | rejected [nf] | n_rejected [nw] | flags [nf]
        b->fc_bytes = nf * (2 * sizeof(double) + 2 * sizeof(int) + 1) + (size_t)nw * sizeof(int);
        rc |= b->pool.zeros(b->fc_bytes, &b->fc_out);
        if (rc) return fail(SWF_E_NODEVICE, "device allocation failed");
        HIPCHK(hipStreamSynchronize(nullptr));      // the pool initialises late allocations on the default stream; the kernels run on the batch's
        A.mean_err = (double*)b->fc_out; A.depth = A.mean_err + nf; A.n_obs = (int*)(A.depth + nf); A.rejected = A.n_obs + nf;
        A.n_rejected = A.rejected + nf; A.flags = (unsigned char*)(A.n_rejected + nw);
        A.n_blk = (int)T.blk.size(); A.n_win = nw;
        b->fc_nfeat = (int)nf; b->fc_feat0 = T.w_feat0;
        for (int w = 0; w < nw; w++) b->hw[w].feat = FeatWinSrc{};          // the table has them now
        b->fc_built = true;
    }
    b->fc.x = b->D.x; b->fc.thr = max_mean_error;
    b->fc_valid = false;
    const int rc = swf_internal_feature_launch(b->fc, b->stream);
    if (rc) return rc;
    b->fc_valid = true; b->fc_host = false;
    return SWF_OK;
}

extern "C" int swf_batch_get_feature_check(swf_batch* b, int32_t w, double* mean_err, double* depth, int32_t* n_obs, uint8_t* flags,
                                           int32_t* rejected, int32_t* n_rejected, int32_t* n_feat) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->fc_valid) return fail(SWF_E_STATE, "swf_batch_get_feature_check before swf_batch_check_features (or after a new solve / state upload)");
    if (!b->fc_host) {           // the first getter after a check copies every window's results in one transfer
        b->h_fc.resize(b->fc_bytes);
        HIPCHK(hipMemcpyAsync(b->h_fc.data(), b->fc_out, b->fc_bytes, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        b->fc_host = true;
    }
    const size_t nf = (size_t)b->fc_nfeat, nw = b->win.size(), f0 = (size_t)b->fc_feat0[w], n = (size_t)b->fc_feat0[w + 1] - f0;
    const double* h_mean = (const double*)b->h_fc.data(); const double* h_depth = h_mean + nf;
    const int* h_nobs = (const int*)(h_depth + nf); const int* h_rej = h_nobs + nf; const int* h_nrej = h_rej + nf;
    const unsigned char* h_flags = (const unsigned char*)(h_nrej + nw);
    if (n_feat) *n_feat = (int32_t)n;
    if (mean_err) memcpy(mean_err, h_mean + f0, n * sizeof(double));
    if (depth) memcpy(depth, h_depth + f0, n * sizeof(double));
    if (n_obs) memcpy(n_obs, h_nobs + f0, n * sizeof(int));
    if (flags) memcpy(flags, h_flags + f0, n);
    if (rejected) memcpy(rejected, h_rej + f0, (size_t)h_nrej[w] * sizeof(int));
    if (n_rejected) *n_rejected = h_nrej[w];
    return SWF_OK;
}

extern "C" int swf_batch_get_prior(swf_batch* b, int32_t w, double* A, double* bv, double* J, double* r0, double* eig, int32_t* n_out, int32_t* rank) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (!b->mg_valid) return fail(SWF_E_STATE, "swf_batch_get_prior before swf_batch_marginalize");
    HIPCHK(hipStreamSynchronize(b->stream));
    size_t n = (size_t)b->hw[w].tail_dim, o2 = (size_t)w * b->mg_ld * b->mg_ld, o1 = (size_t)w * b->mg_ld;
    if (n_out) *n_out = (int32_t)n;
    const size_t nw = b->win.size(), tot2 = nw * b->mg_ld * b->mg_ld, tot1 = nw * b->mg_ld;
    if (nw >= 8 && tot2 <= ((size_t)1 << 23)) {
        if (!b->mg_host) {
            b->h_mgA.resize(tot2); b->h_mgJ.resize(tot2); b->h_mgb.resize(tot1); b->h_mgr0.resize(tot1); b->h_mgw.resize(tot1); b->h_mgrank.resize(nw);
            HIPCHK(hipMemcpy(b->h_mgA.data(), b->mg_A, tot2 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->h_mgJ.data(), b->mg_J, tot2 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->h_mgb.data(), b->mg_b, tot1 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->h_mgr0.data(), b->mg_r0, tot1 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->h_mgw.data(), b->mg_w, tot1 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b->h_mgrank.data(), b->mg_rank, nw * sizeof(int), hipMemcpyDeviceToHost));
            b->mg_host = true;
        }
        if (A) memcpy(A, b->h_mgA.data() + o2, n * n * sizeof(double));
        if (J) memcpy(J, b->h_mgJ.data() + o2, n * n * sizeof(double));
        if (bv) memcpy(bv, b->h_mgb.data() + o1, n * sizeof(double));
        if (r0) memcpy(r0, b->h_mgr0.data() + o1, n * sizeof(double));
        if (eig) memcpy(eig, b->h_mgw.data() + o1, n * sizeof(double));
        if (rank) *rank = b->h_mgrank[(size_t)w];
        return SWF_OK;
    }
    if (A) HIPCHK(hipMemcpy(A, b->mg_A + o2, n * n * sizeof(double), hipMemcpyDeviceToHost));
    if (J) HIPCHK(hipMemcpy(J, b->mg_J + o2, n * n * sizeof(double), hipMemcpyDeviceToHost));
    if (bv) HIPCHK(hipMemcpy(bv, b->mg_b + o1, n * sizeof(double), hipMemcpyDeviceToHost));
    if (r0) HIPCHK(hipMemcpy(r0, b->mg_r0 + o1, n * sizeof(double), hipMemcpyDeviceToHost));
    if (eig) HIPCHK(hipMemcpy(eig, b->mg_w + o1, n * sizeof(double), hipMemcpyDeviceToHost));
    if (rank) HIPCHK(hipMemcpy(rank, b->mg_rank + w, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SWF_OK;
}

extern "C" int swf_batch_export_vectors(swf_batch* b, int32_t w, double* grad, double* diag, double* y) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    const WinRec& W = b->win[w];
    size_t n = (size_t)W.n_loc;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (grad) HIPCHK(hipMemcpy(grad, b->D.g + W.loc_base, n * sizeof(double), hipMemcpyDeviceToHost));
    if (diag) HIPCHK(hipMemcpy(diag, b->D.diag + W.loc_base, n * sizeof(double), hipMemcpyDeviceToHost));
    if (y) HIPCHK(hipMemcpy(y, b->D.y + W.loc_base, n * sizeof(double), hipMemcpyDeviceToHost));
    return SWF_OK;
}

// Debug / parity export: the step of window w's last proposed candidate (k_dogleg / k_step_eval), n_loc doubles in elimination order.
extern "C" int swf_batch_export_step(swf_batch* b, int32_t w, double* step) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    if (b->last_mode != SWF_OPTIMIZE) return fail(SWF_E_STATE, "swf_batch_export_step before an optimising solve");
    const WinRec& W = b->win[w];
    HIPCHK(hipStreamSynchronize(b->stream));
    if (step) HIPCHK(hipMemcpy(step, b->D.step + W.loc_base, (size_t)W.n_loc * sizeof(double), hipMemcpyDeviceToHost));
    return SWF_OK;
}

// Debug / parity export: residual vector and dense Jacobian of window w as the device holds them after its last
// linearisation (see include/swf_solver.h).  Host-side gather of the device buffers; nothing here is on the solve path.
extern "C" int swf_batch_export_jacobian(swf_batch* b, int32_t w, double* r, double* J, int32_t* n_res_out, int32_t* n_loc_out) {
    DeviceGuard dg_(b ? b->device : -1);
    if (!b || w < 0 || w >= (int)b->win.size()) return fail(SWF_E_INVALID, "bad window index");
    const WinRec& W = b->win[w];
    const DevBatch& D = b->D;
    const int ngf = W.gf1 - W.gf0, nobs = W.proj1 - W.proj0;
    std::vector<GFac> gf((size_t)std::max(ngf, 0));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (ngf > 0) HIPCHK(hipMemcpy(gf.data(), D.gf + W.gf0, (size_t)ngf * sizeof(GFac), hipMemcpyDeviceToHost));
    const int nproj_all = b->hw[w].n_proj_all;
    int nres = 2 * nproj_all;
    for (const GFac& G : gf) if (G.type != GF_PROJX) nres += G.nres;
    if (n_res_out) *n_res_out = nres;
    if (n_loc_out) *n_loc_out = W.n_loc;
    if (!r && !J) return SWF_OK;
    if (b->last_mode < 0) return fail(SWF_E_STATE, "swf_batch_export_jacobian before any solve");
    const size_t nl = (size_t)W.n_loc, N = (size_t)D.n_proj;
    if (J) memset(J, 0, (size_t)nres * nl * sizeof(double));
    auto dl = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    bool ok = true;
    if (nobs > 0) {
        std::vector<double> pr(2 * (size_t)nobs), Jp(12 * (size_t)nobs), Jl(6 * (size_t)nobs);
        std::vector<int> lp((size_t)nobs), ll((size_t)nobs);
        for (int k = 0; k < 2; k++) ok &= dl(pr.data() + (size_t)k * nobs, D.p_r + k * N + W.proj0, (size_t)nobs * 8);
        for (int k = 0; k < 12; k++) ok &= dl(Jp.data() + (size_t)k * nobs, D.p_Jp + k * N + W.proj0, (size_t)nobs * 8);
        for (int k = 0; k < 6; k++) ok &= dl(Jl.data() + (size_t)k * nobs, D.p_Jl + k * N + W.proj0, (size_t)nobs * 8);
        ok &= dl(lp.data(), D.p_lpose + W.proj0, (size_t)nobs * 4); ok &= dl(ll.data(), D.p_llm + W.proj0, (size_t)nobs * 4);
        if (!ok) return fail(SWF_E_NODEVICE, "download failed");
        for (int q = 0; q < nobs; q++) {
            const size_t row = 2 * (size_t)b->hw[w].p_orig[q];
            for (int a = 0; a < 2; a++) {
                if (r) r[row + a] = pr[(size_t)a * nobs + q];
                if (!J) continue;
                // (the translation half of Jp is not stored next to a variable landmark: it is -Jl)
                if (lp[q] >= 0) for (int c = 0; c < 6; c++) J[(row + a) * nl + (lp[q] - W.loc_base) + c] = (c < 3 && ll[q] >= 0) ? -Jl[(size_t)(a * 3 + c) * nobs + q] : Jp[(size_t)(a * 6 + c) * nobs + q];
                if (ll[q] >= 0) for (int c = 0; c < 3; c++) J[(row + a) * nl + (ll[q] - W.loc_base) + c] = Jl[(size_t)(a * 3 + c) * nobs + q];
            }
        }
    }
    size_t row_seq = 2 * (size_t)nproj_all;
    for (const GFac& G : gf) {
        // generic-path projection factors sit at the caller's projection index; every other family follows in factor order
        const size_t row = G.type == GF_PROJX ? 2 * (size_t)G.pad : row_seq;
        std::vector<int> sloc((size_t)G.nslot), sls((size_t)G.nslot), sj((size_t)G.nslot), spc((size_t)G.nslot);
        ok &= dl(sloc.data(), D.s_loc + G.slot0, (size_t)G.nslot * 4); ok &= dl(sls.data(), D.s_ls + G.slot0, (size_t)G.nslot * 4);
        ok &= dl(sj.data(), D.s_joff + G.slot0, (size_t)G.nslot * 4); ok &= dl(spc.data(), D.s_pcol + G.slot0, (size_t)G.nslot * 4);
        if (r) ok &= dl(r + row, D.g_r + G.roff, (size_t)G.nres * 8);
        if (J && G.type == GF_PRIOR) {
            // linearised prior (and composite factors, whose record k_comp_scatter rewrites): the constant row-major J of the record
            int dim = 0; long long jo = 0;
            ok &= dl(&dim, D.prior_dim + G.data, 4); ok &= dl(&jo, D.prior_Joff + G.data, 8);
            std::vector<double> PJ((size_t)dim * dim);
            ok &= dl(PJ.data(), D.prior_J + jo, PJ.size() * 8);
            for (int sl = 0; sl < G.nslot; sl++) {
                if (sloc[sl] < 0) continue;
                for (int k = 0; k < G.nres; k++) for (int c = 0; c < sls[sl]; c++)
                    J[(row + k) * nl + (sloc[sl] - W.loc_base) + c] = PJ[(size_t)k * dim + spc[sl] + c];
            }
        } else if (J) {
            for (int sl = 0; sl < G.nslot; sl++) {
                if (sloc[sl] < 0 || sj[sl] < 0) continue;
                std::vector<double> blk((size_t)sls[sl] * G.jld);
                ok &= dl(blk.data(), D.g_J + sj[sl], (((size_t)sls[sl] - 1) * G.jld + G.nres) * 8);
                for (int k = 0; k < G.nres; k++) for (int c = 0; c < sls[sl]; c++)
                    J[(row + k) * nl + (sloc[sl] - W.loc_base) + c] = blk[(size_t)c * G.jld + k];
            }
        }
        if (G.type != GF_PROJX) row_seq += G.nres;
    }
    if (!ok) return fail(SWF_E_NODEVICE, "download failed");
    return SWF_OK;
}

// The symbolic phase alone, with no device: plan_build + plan_validate for the given chip size and launch-shape knobs (flags: 1 =
// SWF_NO_LAT_FUSE, 2 = SWF_NO_CHOL_COL); the validator's finding is left in swf_last_error.  corrupt_table 1 .. 8 damages entry
// corrupt_index of as_src / sch_rec / s_tnz / prior_colloc / loc2x / co_voff / pair_o / imu_rec in this call's own plan before it is validated (the negative control of the validator).
// info (may be null), 12 ints: ls_var, ls_qpb, ls_gqpb, ls_folded, lat_fuse, want_aux, want_Linv, want_Wk, asm_programs, n_pch_split, max_red, n_pch.
extern "C" int swf_debug_plan_check(const swf_flat_window* const* windows, int32_t n, int32_t n_cu, int32_t ls_variant, int32_t ls_qpb, int32_t ls_grad_qpb,
                                    int32_t flags, int32_t corrupt_table, int32_t corrupt_index, int32_t* info) {
    if (!windows || n <= 0 || n_cu <= 0) return fail(SWF_E_INVALID, "swf_debug_plan_check: bad arguments");
    PlanShape sh;
    sh.n_cu = n_cu; sh.ls_variant = ls_variant; sh.ls_qpb = ls_qpb; sh.ls_grad_qpb = ls_grad_qpb; sh.no_lat_fuse = flags & 1; sh.no_chol_col = flags & 2;
    Plan B; std::string err;
    int rc = plan_build(windows, n, sh, B, err);
    if (rc != SWF_OK) return fail(rc, err);
    if (corrupt_table) {
        const size_t i = (size_t)corrupt_index;
        if (corrupt_table == 1 && i < B.as_src.size()) B.as_src[i] += 1 << 28;
        else if (corrupt_table == 2 && i < B.sch_rec.size()) B.sch_rec[i] ^= 1;
        else if (corrupt_table == 3 && i < B.s_tnz.size() && B.s_tnz[i]) B.s_tnz[i] &= B.s_tnz[i] - 1;      // its lowest set bit
        else if (corrupt_table == 4 && i < B.prior_colloc.size()) B.prior_colloc[i] ^= 1;
        else if (corrupt_table == 5 && i < B.loc2x.size()) B.loc2x[i] ^= 1;
        else if (corrupt_table == 6 && i < B.co_voff.size()) B.co_voff[i] += 1 << 28;
        else if (corrupt_table == 7 && i < B.pair_o.size()) B.pair_o[i].q_base += 8;
        else if (corrupt_table == 8 && i < B.imu_rec.size()) B.imu_rec[i].xo[3] ^= 1;
        else return fail(SWF_E_INVALID, "swf_debug_plan_check: nothing to corrupt there");
    }
    if (info) {
        const int v[12] = { B.ls_var, B.ls_qpb, B.ls_gqpb, B.ls_folded, B.lat_fuse, B.want_aux, B.want_Linv, B.want_Wk, B.asm_programs, B.n_pch_split, B.max_red, B.n_pch };
        for (int k = 0; k < 12; k++) info[k] = v[k];
    }
    rc = plan_validate(B, err);
    return rc == SWF_OK ? SWF_OK : fail(rc, err);
}

// One v_mfma_f64_16x16x4_f64 on the given operands (host pointers, row-major: A 16 x 4, B 4 x 16, C and D 16 x 16): what k_clique_mm
// rests on is the order in which the instruction accumulates its four k-slots (tests/test_clique_mfma_gpu.py).
extern "C" int swf_debug_mfma_f64(const double* A, const double* Bm, const double* C, double* D) {
    if (!A || !Bm || !C || !D) return fail(SWF_E_INVALID, "swf_debug_mfma_f64: bad arguments");
    double* dv = nullptr;
    if (hipMalloc(&dv, (64 + 64 + 256 + 256) * sizeof(double)) != hipSuccess) return fail(SWF_E_NODEVICE, "swf_debug_mfma_f64: allocation failed");
    bool ok = hipMemcpy(dv, A, 64 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(dv + 64, Bm, 64 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(dv + 128, C, 256 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_debug_mfma_f64, dim3(1), dim3(64), 0, 0, dv, dv + 64, dv + 128, dv + 384);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(D, dv + 384, 256 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dv);
    return ok ? SWF_OK : fail(SWF_E_NODEVICE, "swf_debug_mfma_f64: the device run failed");
}

#ifdef SWF_PROFILE_CHOL
extern "C" int swf_debug_chol_stamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chol_stamps), 64 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif

#ifdef SWF_PROFILE_CHOLW
extern "C" int swf_debug_chol_wstep(int step) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    unsigned long long z[16 * 8] = { 0 };
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_chol_wst), z, sizeof(z)) != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_chol_wstep), &step, sizeof(int)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
extern "C" int swf_debug_chol_wstamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chol_wst), 16 * 8 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
extern "C" int swf_debug_chol_pstamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chol_pst), 16 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
extern "C" int swf_debug_chol_cstamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chol_cst), 32 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif

#ifdef SWF_PROFILE_DOG
extern "C" int swf_debug_dog_stamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dog_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif

#ifdef SWF_PROFILE_CLQ
extern "C" int swf_debug_clq_stamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clq_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif

#ifdef SWF_PROFILE_EVAL
extern "C" int swf_debug_eval_stamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_eval_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif

#ifdef SWF_PROFILE_GEMM
extern "C" int swf_debug_gemm_stamps(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return SWF_E_NODEVICE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gemm_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return SWF_E_NODEVICE;
    return SWF_OK;
}
#endif


// =====================================================================================================================
// Composite IMU-GNSS factors as a batched operator (include/swf_solver.h, swf_kernels4.h).  Stateful like the reference's
// IMUGNSSBase: the handle owns the hidden epochs, the saved elimination blocks and the last linearisation.
// =====================================================================================================================
struct swf_composite {
    CompArgs A{};
    std::vector<void*> bufs;
    int n = 0, nmax = 0, nmin = 0; long long sumM = 0, sumN = 0, sumG = 0, sumG2 = 0;
    std::vector<int> M;
    bool eigen_root = false;
    hipStream_t stream = nullptr;
    ~swf_composite() { for (void* p : bufs) (void)hipFree(p); }
};

extern "C" int swf_composite_destroy(swf_composite* c) { delete c; return SWF_OK; }

extern "C" int swf_composite_create(int32_t n, const int32_t* M, const int32_t* N, const double* pose, const double* sb,
                                    const double* pose_lin, const double* sb_lin, const double* Hpp, const double* HpN,
                                    const double* rhs_p, const double* HNN, const double* rhsN, const double* pre,
                                    const double pbg[3], const double gw[3], void* stream, swf_composite** out) {
    if (!out || n <= 0 || !M || !N || !pose || !sb || !pose_lin || !sb_lin || !Hpp || !HpN || !rhs_p || !HNN || !rhsN || !pre || !pbg || !gw)
        return fail(SWF_E_INVALID, "swf_composite_create: null argument");
    std::vector<int> eo(n + 1, 0), no(n + 1, 0);
    std::vector<long long> pno(n + 1, 0), nno(n + 1, 0), go(n + 1, 0), g2o(n + 1, 0);
    int nmax_ = 0, nmin_ = 1 << 30;
    for (int f = 0; f < n; f++) {
        if (M[f] < 1) return fail(SWF_E_INVALID, "composite factor without hidden epochs");
        if (N[f] < 0 || N[f] > CO_MAXN) return fail(SWF_E_UNSUPPORTED, "composite factor with more than 64 ambiguities");
        nmax_ = std::max(nmax_, (int)N[f]); nmin_ = std::min(nmin_, (int)N[f]);
        eo[f + 1] = eo[f] + M[f]; no[f + 1] = no[f] + N[f];
        pno[f + 1] = pno[f] + 15LL * M[f] * N[f]; nno[f + 1] = nno[f] + (long long)N[f] * N[f];
        go[f + 1] = go[f] + 30 + N[f]; g2o[f + 1] = g2o[f] + (long long)(30 + N[f]) * (30 + N[f]);
    }
    std::unique_ptr<swf_composite> c(new swf_composite());
    c->n = n; c->nmax = nmax_; c->nmin = nmin_; c->sumM = eo[n]; c->sumN = no[n]; c->sumG = go[n]; c->sumG2 = g2o[n]; c->stream = (hipStream_t)stream;
    bool bad = false;
    auto up = [&](const void* src, size_t bytes) -> void* {
        void* d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) { bad = true; return nullptr; }
        c->bufs.push_back(d);
        if (src) { if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) bad = true; }
        else if (hipMemset(d, 0, std::max<size_t>(bytes, 8)) != hipSuccess) bad = true;
        return d;
    };
    CompArgs& A = c->A;
    const size_t D = sizeof(double);
    A.n = n;
    A.M = (const int*)up(M, n * sizeof(int)); A.N = (const int*)up(N, n * sizeof(int));
    A.e_off = (const int*)up(eo.data(), (n + 1) * sizeof(int)); A.n_off = (const int*)up(no.data(), (n + 1) * sizeof(int));
    A.pn_off = (const long long*)up(pno.data(), (n + 1) * sizeof(long long)); A.nn_off = (const long long*)up(nno.data(), (n + 1) * sizeof(long long));
    A.g_off = (const long long*)up(go.data(), (n + 1) * sizeof(long long)); A.g2_off = (const long long*)up(g2o.data(), (n + 1) * sizeof(long long));
    A.pose = (double*)up(pose, c->sumM * 7 * D); A.sb = (double*)up(sb, c->sumM * 9 * D);
    A.pose_lin = (const double*)up(pose_lin, c->sumM * 7 * D); A.sb_lin = (const double*)up(sb_lin, c->sumM * 9 * D);
    A.Hpp = (const double*)up(Hpp, c->sumM * 225 * D); A.HpN = (const double*)up(HpN, pno[n] * D); A.rhs_p = (const double*)up(rhs_p, c->sumM * 15 * D);
    A.HNN = (const double*)up(HNN, nno[n] * D); A.rhsN = (const double*)up(rhsN, c->sumN * D);
    A.pre = (const double*)up(pre, (size_t)(c->sumM + n) * SWF_PRE_DOUBLES * D);
    {
        std::vector<double> pg((size_t)n * 6);
        for (int f = 0; f < n; f++) for (int k = 0; k < 3; k++) { pg[(size_t)f * 6 + k] = pbg[k]; pg[(size_t)f * 6 + 3 + k] = gw[k]; }
        A.pbgw = (const double*)up(pg.data(), pg.size() * D);
    }
    A.active = nullptr;
    A.hmn_inv = (double*)up(nullptr, c->sumM * 225 * D); A.hmn_2 = (double*)up(nullptr, c->sumM * 225 * D); A.hmn_0 = (double*)up(nullptr, c->sumM * 225 * D);
    A.hmn_N = (double*)up(nullptr, pno[n] * D); A.rhsmn = (double*)up(nullptr, c->sumM * 15 * D);
    A.Hd = (double*)up(nullptr, c->sumG2 * D); A.rd = (double*)up(nullptr, c->sumG * D); A.Ld = (double*)up(nullptr, c->sumG2 * D); A.r0 = (double*)up(nullptr, c->sumG * D);
    A.old = (double*)up(nullptr, (size_t)n * 32 * D); A.N_old = (double*)up(nullptr, c->sumN * D);
    A.history = (int*)up(nullptr, n * sizeof(int)); A.status = (int*)up(nullptr, n * sizeof(int));
    A.outer = (const double*)up(nullptr, (size_t)n * 32 * D); A.Nv = (const double*)up(nullptr, c->sumN * D);
    A.res_out = (double*)up(nullptr, c->sumG * D); A.jac_out = (double*)up(nullptr, c->sumG2 * D);
    A.Jw = (double*)up(nullptr, (size_t)(c->sumM + n) * 450 * D); A.rw = (double*)up(nullptr, (size_t)(c->sumM + n) * 16 * D);
    {
        std::vector<int> qf, qk;
        for (int f = 0; f < n; f++) for (int k = 0; k <= M[f]; k++) { qf.push_back(f); qk.push_back(k); }
        A.n_iq = (int)qf.size();
        A.iq_f = (const int*)up(qf.data(), qf.size() * sizeof(int)); A.iq_k = (const int*)up(qk.data(), qk.size() * sizeof(int));
        A.todo = (int*)up(nullptr, n * sizeof(int));
    }
    A.mid = (const int*)up(nullptr, n * sizeof(int)); A.H12 = (const double*)up(nullptr, (size_t)n * 225 * D);
    c->M.assign(M, M + n);
    if (bad) return fail(SWF_E_NODEVICE, "swf_composite_create: device allocation / upload failed");
    *out = c.release();
    return SWF_OK;
}

extern "C" int swf_composite_evaluate(swf_composite* c, const double* outer, const double* Nv, int32_t want_jac,
                                      double* residual, double* jac, double* Hd, double* rd, int32_t* status) {
    if (!c || !outer || (!Nv && c->sumN) || !residual) return fail(SWF_E_INVALID, "swf_composite_evaluate: null argument");
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync((void*)c->A.outer, outer, (size_t)c->n * 32 * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->sumN) HIPCHK(hipMemcpyAsync((void*)c->A.Nv, Nv, c->sumN * sizeof(double), hipMemcpyHostToDevice, st));
    CompArgs A = c->A;
    A.want_jac = want_jac ? 1 : 0;
    hipLaunchKernelGGL(k_comp_prep, dim3(c->n), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_comp_imu, dim3((A.n_iq + 7) / 8), dim3(256), 0, st, A);
    if (c->nmin <= CO_SMALLN) hipLaunchKernelGGL((k_comp_elim<CO_SMALLN, 256>), dim3(c->n), dim3(256), 0, st, A, 0);
    if (c->nmax > CO_SMALLN) hipLaunchKernelGGL((k_comp_elim<CO_MAXN, 256>), dim3(c->n), dim3(256), 0, st, A, CO_SMALLN + 1);
    if (c->eigen_root) {
        if (c->nmax <= CO_SMALLN) hipLaunchKernelGGL(k_comp_eigroot<CO_SMALLN>, dim3(c->n), dim3(256), 0, st, A);
        else hipLaunchKernelGGL(k_comp_eigroot<CO_MAXN>, dim3(c->n), dim3(512), 0, st, A);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(residual, c->A.res_out, c->sumG * sizeof(double), hipMemcpyDeviceToHost, st));
    if (jac && want_jac) HIPCHK(hipMemcpyAsync(jac, c->A.jac_out, c->sumG2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (Hd) HIPCHK(hipMemcpyAsync(Hd, c->A.Hd, c->sumG2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (rd) HIPCHK(hipMemcpyAsync(rd, c->A.rd, c->sumG * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(hipMemcpyAsync(status, c->A.status, c->n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SWF_OK;
}

extern "C" int swf_composite_set_root(swf_composite* c, int32_t form) {
    if (!c || (form != SWF_ROOT_PIVOTED_CHOLESKY && form != SWF_ROOT_EIGEN)) return fail(SWF_E_INVALID, "swf_composite_set_root: bad arguments");
    c->eigen_root = form == SWF_ROOT_EIGEN;
    return SWF_OK;
}

extern "C" int swf_composite_set_mid_links(swf_composite* c, const int32_t* mid, const double* H12) {
    if (!c || !mid || !H12) return fail(SWF_E_INVALID, "swf_composite_set_mid_links: null argument");
    for (int f = 0; f < c->n; f++)
        if (mid[f] != 0 && (mid[f] < 1 || mid[f] > c->M[(size_t)f] - 1)) return fail(SWF_E_INVALID, "swf_composite_set_mid_links: a link must lie between two hidden epochs (1..M-1)");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy((void*)c->A.mid, mid, (size_t)c->n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void*)c->A.H12, H12, (size_t)c->n * 225 * sizeof(double), hipMemcpyHostToDevice));
    return SWF_OK;
}

extern "C" int swf_composite_hidden(swf_composite* c, double* pose, double* sb) {
    if (!c || !pose || !sb) return fail(SWF_E_INVALID, "swf_composite_hidden: null argument");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(pose, c->A.pose, c->sumM * 7 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sb, c->A.sb, c->sumM * 9 * sizeof(double), hipMemcpyDeviceToHost));
    return SWF_OK;
}
