// The second half of LambdaSearch (R/swf/swf_lambda.cpp:254-353) bound to the device through swf_ceres::FixAndHoldPrior, under the
// reference's -std=c++14: a window prior over [pose, speed-bias, S ambiguities], double differences fixed to integers, the prior
// swapped as the reference swaps last_marg_info.  Input (argv[1], text; without it a small built-in case): S scalars_at_zero eigen,
// J (dim x dim, dim = 15 + S), r0, x0 (16 + S), the blocks' current values (16 + S), n pairs, then n lines "amb ref N21".
// Prints dim, rank, J', r0', x0' (%.17g); exit status 0 on success, 1 when the call fails (e.g. without a GPU).
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

int main(int argc, char** argv) {
    int S = 3, saz = 1, eigen = 1, np = 2;
    std::vector<double> J, r0, x0, cur;
    std::vector<int> pa, pb; std::vector<double> N21;
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "r");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
        auto rd = [&](std::vector<double>& v, size_t n) { v.resize(n); for (size_t i = 0; i < n; i++) if (std::fscanf(f, "%lf", &v[i]) != 1) return false; return true; };
        bool ok = std::fscanf(f, "%d %d %d", &S, &saz, &eigen) == 3;
        const size_t dim = 15 + (size_t)S;
        ok = ok && rd(J, dim * dim) && rd(r0, dim) && rd(x0, dim + 1) && rd(cur, dim + 1) && std::fscanf(f, "%d", &np) == 1;
        pa.resize(np); pb.resize(np); N21.resize(np);
        for (int i = 0; ok && i < np; i++) ok = std::fscanf(f, "%d %d %lf", &pa[i], &pb[i], &N21[i]) == 3;
        std::fclose(f);
        if (!ok) { std::printf("malformed input\n"); return 2; }
    } else {
        const int dim = 15 + S;
        J.assign((size_t)dim * dim, 0.0); r0.assign(dim, 0.0); x0.assign(dim + 1, 0.0); x0[6] = 1.0;
        for (int i = 0; i < dim; i++) { J[(size_t)i * dim + i] = 2.0 + 0.1 * i; if (i) J[(size_t)i * dim + i - 1] = 0.3; r0[i] = 0.01 * i; }
        cur = x0; cur[0] = 0.1; cur[16] = 3.2; cur[17] = -1.9; cur[18] = 0.4;
        pa = { 0, 1 }; pb = { 2, 2 }; N21 = { 3.0, -2.0 };
    }
    const int dim = 15 + S;
    std::vector<double> pose(cur.begin(), cur.begin() + 7), sb(cur.begin() + 7, cur.begin() + 16), amb(cur.begin() + 16, cur.end());
    swf_ceres::Problem problem;
    problem.AddParameterBlock(pose.data(), 7, new swf_ceres::PoseLocalParameterization());
    problem.AddParameterBlock(sb.data(), 9);
    std::vector<double*> blocks = { pose.data(), sb.data() };
    for (int i = 0; i < S; i++) { problem.AddParameterBlock(&amb[i], 1); blocks.push_back(&amb[i]); }
    swf_ceres::ResidualBlockId prior =
        problem.AddResidualBlock(new swf_ceres::MarginalizationFactor(J.data(), r0.data(), x0.data(), dim, dim + 1), nullptr, blocks);
    std::vector<double*> ka, kb;
    for (int i = 0; i < np; i++) { ka.push_back(&amb[pa[i]]); kb.push_back(&amb[pb[i]]); }
    swf_ceres::MarginalPrior out;
    const double* x0n = nullptr;
    if (!swf_ceres::FixAndHoldPrior(&problem, prior, ka, kb, N21, &out, &x0n, saz != 0, 1.0 / 0.03, eigen != 0, 1e-8)) {
        std::printf("FixAndHoldPrior failed: %s\n", swf_last_error());
        return 1;
    }
    std::printf("%d %d\n", out.n, out.rank);
    for (int i = 0; i < out.n * out.n; i++) std::printf("%.17g\n", out.linearized_jacobians[i]);
    for (int i = 0; i < out.n; i++) std::printf("%.17g\n", out.linearized_residuals[i]);
    for (int i = 0; i < dim + 1; i++) std::printf("%.17g\n", x0n[i]);
    // the swap of R/swf/swf_lambda.cpp:344-354
    swf_ceres::MarginalizationFactor* nf = new swf_ceres::MarginalizationFactor(out.linearized_jacobians, out.linearized_residuals, x0n, out.n, dim + 1);
    problem.RemoveResidualBlock(prior);
    problem.AddResidualBlock(nf, nullptr, blocks);
    return problem.NumResidualBlocks() == 1 ? 0 : 1;
}
