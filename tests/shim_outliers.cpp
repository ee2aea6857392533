// ImagePostprocess's outlier step (R/swf/swf_image.cpp:115-121) bound to the device through swf_ceres::OutliersRejection: solve a
// small two-view window in which one feature's observations were displaced, ask for the failed blocks, print them together with the
// solved state (tests/test_feature_check.py replays the state through the numpy referee).  Exit status 0 on success, 1 when the
// solve or the check fails (e.g. without a GPU).
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"
namespace ceres = swf_ceres;
using namespace swf_ceres;

int main() {
    ceres::Problem my_problem;
    ceres::Solver::Options my_options;
    my_options.linear_solver_type = ceres::DENSE_SCHUR;
    my_options.max_num_iterations = 8;
    my_options.jacobi_scaling = 0;
    my_options.trust_region_strategy_type = ceres::DOGLEG;
    my_options.linear_solver_ordering.reset(new ceres::ParameterBlockOrdering());

    const int n = 6, bad = 4;
    double pose0[7] = {0, 0, 0, 0, 0, 0, 1}, pose1[7] = {0.4, 0, 0, 0, 0, 0, 1}, ex[7] = {0, 0, 0, 0, 0, 0, 1};
    double pt[n][3] = {{0.5, 0.3, 6}, {-0.4, 0.2, 7}, {0.2, -0.5, 8}, {-0.3, -0.3, 9}, {0.6, -0.2, 7.5}, {-0.1, 0.4, 6.5}};
    double blackvalue2 = 0;
    my_problem.AddParameterBlock(pose0, 7, new PoseLocalParameterization());
    my_problem.AddParameterBlock(pose1, 7, new PoseLocalParameterization());
    my_problem.AddParameterBlock(ex, 7, new PoseLocalParameterization());
    my_problem.SetParameterBlockConstant(ex);
    my_problem.SetParameterBlockConstant(pose0);
    for (int i = 0; i < n; i++) {
        // the displaced feature moves up in one view and down in the other: no depth explains a vertical disparity
        const double dy = i == bad ? 0.04 : 0.0;
        double u0[3] = {pt[i][0] / pt[i][2], pt[i][1] / pt[i][2] + dy, 1}, u1[3] = {(pt[i][0] - 0.4) / pt[i][2] + 1e-3, pt[i][1] / pt[i][2] - dy, 1};
        my_problem.AddResidualBlock(new projection_factor(u0), new ceres::CauchyLoss(1.0), pose0, ex, pt[i]);
        my_problem.AddResidualBlock(new projection_factor(u1), new ceres::CauchyLoss(1.0), pose1, ex, pt[i]);
    }
    my_problem.AddResidualBlock(new InitialBlackFactor(1), 0, &blackvalue2);
    ceres::ParameterBlockOrdering* ordering = my_options.linear_solver_ordering.get();
    ordering->AddElementToGroup(&blackvalue2, 0);
    for (int i = 0; i < n; i++) ordering->AddElementToGroup(pt[i], 0);
    ordering->AddElementToGroup(pose1, 1);
    ceres::internal::is_optimize = true;
    ceres::Solver::Summary summary;
    ceres::Solve(my_options, &my_problem, &summary);
    if (!(summary.final_cost < 1e10)) { std::printf("solve failed: %s\n", swf_last_error()); return 1; }

    std::vector<double*> failed;
    if (!ceres::OutliersRejection(my_problem, 2.0, failed)) { std::printf("OutliersRejection failed: %s\n", swf_last_error()); return 1; }
    std::printf("failed %d:", (int)failed.size());
    for (double* k : failed) for (int i = 0; i < n; i++) if (k == pt[i]) std::printf(" %d", i);
    std::printf("\n");
    std::printf("pose1 %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", pose1[0], pose1[1], pose1[2], pose1[3], pose1[4], pose1[5], pose1[6]);
    for (int i = 0; i < n; i++) {
        double mean = 0, depth = 0; int32_t n_obs = 0, flags = 0;
        if (swf_problem_get_feature_check(my_problem.handle(), pt[i], &mean, &depth, &n_obs, &flags) != SWF_OK) return 1;
        std::printf("point %d %.17g %.17g %.17g mean %.17g depth %.17g n_obs %d flags %d\n", i, pt[i][0], pt[i][1], pt[i][2], mean, depth, n_obs, flags);
    }
    return 0;
}
