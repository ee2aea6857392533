// The symbolic phase under the host sanitizers, with no device and no HIP: this program is compiled from csrc/swf_plan.cpp and
// csrc/swf_problem.cpp with -fsanitize=address,undefined (tests/test_plan_host.py).  It runs the scenes of shim_example.cpp and
// shim_reference_solve.cpp — estimator code in the reference's style, through include/swf_ceres.hpp — against a stand-in engine:
// its swf_batch_create builds and validates the plan of the window the problem hands over, at a full-size and at a tiny chip, and
// then reports that there is no device, which is what those scenes see on a machine without a GPU.
#include <cstdio>
#include <string>
#include "swf_solver.h"
#include "../rtk_visual_inertial_navigation_amd/csrc/swf_plan.h"

static std::string g_err;
static int g_plans = 0, g_bad = 0;
void swf_internal_set_error(const std::string& m) { g_err = m; }

extern "C" {
const char* swf_last_error(void) { return g_err.c_str(); }
int swf_device_count(int32_t* n) { *n = 0; g_err = "no HIP device"; return SWF_E_NODEVICE; }
void swf_default_options(swf_options* o) {
    *o = swf_options{};
    o->max_num_iterations = 8; o->num_threads = 1; o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->min_mu = 1e-8; o->max_mu = 1.0; o->mu_increase_factor = 10.0; o->min_diagonal = 1e-6; o->max_diagonal = 1e32;
}
int swf_batch_create(const swf_flat_window* const* windows, int32_t n, void*, swf_batch** out) {
    *out = nullptr;
    for (int n_cu : { 256, 8, 1 }) {
        PlanShape sh; sh.n_cu = n_cu;
        Plan plan; std::string err;
        int rc = plan_build(windows, n, sh, plan, err);
        if (rc == SWF_OK) rc = plan_validate(plan, err);
        g_plans++;
        if (rc != SWF_OK) { g_bad++; std::printf("plan (n_cu %d): %d %s\n", n_cu, rc, err.c_str()); }
    }
    g_err = "no HIP device: this library has no CPU fallback";
    return SWF_E_NODEVICE;
}
// the rest of the engine's surface swf_problem.cpp refers to: never reached, there is no batch
static int no_batch() { g_err = "no batch"; return SWF_E_STATE; }
int swf_batch_destroy(swf_batch*) { return SWF_OK; }
int swf_batch_upload_state(swf_batch*) { return no_batch(); }
int swf_batch_enable_timing(swf_batch*, int32_t) { return no_batch(); }
int swf_batch_solve(swf_batch*, const swf_options*) { return no_batch(); }
int swf_batch_sync(swf_batch*) { return no_batch(); }
int swf_batch_download_state(swf_batch*) { return no_batch(); }
int swf_batch_summaries(swf_batch*, swf_summary*) { return no_batch(); }
int swf_batch_export_reduced(swf_batch*, int32_t, double*, double*, double*) { return no_batch(); }
int swf_batch_marginalize(swf_batch*, double, int32_t) { return no_batch(); }
int swf_batch_get_prior(swf_batch*, int32_t, double*, double*, double*, double*, double*, int32_t*, int32_t*) { return no_batch(); }
int swf_batch_tail_covariance(swf_batch*) { return no_batch(); }
int swf_batch_get_tail_covariance(swf_batch*, int32_t, double*, double*, int32_t*) { return no_batch(); }
int swf_batch_check_features(swf_batch*, double) { return no_batch(); }
int swf_batch_get_feature_check(swf_batch*, int32_t, double*, double*, int32_t*, unsigned char*, int32_t*, int32_t*, int32_t*) { return no_batch(); }
// (swf_problem_fix_prior's two operators, which the scenes never call)
int swf_prior_reset_linearization_point(int32_t, const int32_t*, const double* const*, int32_t, const double*, const double*, double*, double*, double*) { return no_batch(); }
int swf_prior_fix_batch(int32_t, const int32_t*, const double*, const double*, const int32_t*, const int32_t*, const double*, double, double, int32_t, double*, double*, double*, double*,
                        double*, int32_t*, int32_t, void*) { return no_batch(); }
}

#define main shim_example_main
#include "shim_example.cpp"
#undef main
#define main shim_reference_solve_main
#include "shim_reference_solve.cpp"
#undef main

int main() {
    const int r1 = shim_example_main(), r2 = shim_reference_solve_main();      // both end with the no-device failure convention
    std::printf("scenes returned %d %d; plans validated: %d of %d\n", r1, r2, g_plans - g_bad, g_plans);
    std::fflush(stdout);
    return (g_plans >= 6 && g_bad == 0 && r1 == 1 && r2 == 1) ? 0 : 1;
}
