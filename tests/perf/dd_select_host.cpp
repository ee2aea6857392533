// The host loop bench_dd_select.py times against the device: the pair selection of swf_dd_select_batch as a plain
// C++ loop over host arrays, same inputs, pairs [n_windows][64][2] and counts [n_windows][4] out.  Built by the script with g++ -O2.
#include <cmath>
#include <cstdint>
#include <vector>

extern "C" void dd_select_host(int32_t n_windows, const int32_t* epoch_first, const int32_t* obs_first, const int32_t* obs,
                               const int32_t* y_first, const double* y_all, const double* gate, int32_t* pairs, int32_t* counts) {
    std::vector<char> used;
    std::vector<int> cand;
    std::vector<double> cost;
    for (int w = 0; w < n_windows; w++) {
        const double* y = y_all + y_first[w];
        const int tail = y_first[w + 1] - y_first[w];
        used.assign((size_t)tail, 0);
        int np = 0, last_count = 0, last_ref = 0;
        int32_t* pw = pairs + (size_t)w * 128;
        for (int e = epoch_first[w]; e < epoch_first[w + 1]; e++) {
            const int f = obs_first[e], n = obs_first[e + 1] - f;
            int ref[6];
            for (int c = 0; c < 6; c++) {
                ref[c] = -1;
                cand.clear();
                for (int k = 0; k < n; k++) if (obs[2 * (f + k)] == c && !used[(size_t)obs[2 * (f + k) + 1]]) cand.push_back(k);
                if (cand.empty()) continue;
                cost.assign(cand.size(), 0.0);
                double lo = INFINITY;
                for (size_t j = 0; j < cand.size(); j++) {
                    const double yj = y[obs[2 * (f + cand[j]) + 1]];
                    for (size_t i = 0; i < cand.size(); i++) { const double s = y[obs[2 * (f + cand[i]) + 1]] - yj; cost[j] += std::fabs(s - std::round(s)); }
                    if (cost[j] < lo) lo = cost[j];
                }
                for (size_t j = 0; j < cand.size(); j++) if (cost[j] == lo) ref[c] = cand[j];
            }
            if (e == epoch_first[w]) for (int c = 0; c < 6; c++) last_ref += ref[c] >= 0;
            for (int k = 0; k < n; k++) {
                const int c = obs[2 * (f + k)], t = obs[2 * (f + k) + 1];
                if (ref[c] < 0 || used[(size_t)t] || k == ref[c]) continue;
                used[(size_t)t] = 1;
                const int tr = obs[2 * (f + ref[c]) + 1];
                const double d = y[t] - y[tr];
                if (std::fabs(d - std::round(d)) < gate[w]) {
                    if (np < 64) { pw[2 * np] = t; pw[2 * np + 1] = tr; }
                    np++;
                    if (e == epoch_first[w]) last_count++;
                }
            }
        }
        const int info = np > 64 ? 2 : (tail >= 6 && last_count + last_ref >= 6 && last_count >= 4 && np >= 4) ? 0 : 1;
        counts[4 * w] = info == 2 ? 0 : np; counts[4 * w + 1] = last_count; counts[4 * w + 2] = last_ref; counts[4 * w + 3] = info;
    }
}
