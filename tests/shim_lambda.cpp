// LambdaSearch's call of RTKLIB's lambda() (R/swf/swf_lambda.cpp:201) bound to the device through swf_ceres::lambda: the same
// arguments (column-major Qb, F n x m), the same return convention.  Prints the candidates; exit status 0 on success, 1 when the
// call fails (e.g. without a GPU).
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

int main() {
    const int n = 4, m = 2;
    // Qb = D Qy D^T of four double-differenced ambiguities (column-major, symmetric) and their float values
    const double Q[n * n] = { 0.090, 0.042, 0.031, 0.020,
                              0.042, 0.070, 0.025, 0.018,
                              0.031, 0.025, 0.060, 0.015,
                              0.020, 0.018, 0.015, 0.050 };
    const double b[n] = { 3.12, -1.94, 7.05, 0.38 };
    std::vector<double> F(n * m);
    double s[m];
    const int info = swf_ceres::lambda(n, m, b, Q, F.data(), s);
    if (info) { std::printf("lambda failed: %d\n", info); return 1; }
    for (int j = 0; j < m; j++) {
        std::printf("candidate %d s %.17g F", j, s[j]);
        for (int i = 0; i < n; i++) std::printf(" %.17g", F[j * n + i]);
        std::printf("\n");
    }
    return 0;
}
