// The reference election and the D3 loop of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:8-53, 118-188) bound to the device
// through swf_ceres::SelectDoubleDifferences, on structs shaped like the reference's mea_t / ObsMea / PBtype.  Two epochs, two
// classes.  Prints the pairs and the counts; exit status 0 on success, 1 when the call fails (e.g. without a GPU).
#include <cstdio>
#include <vector>
#include "swf_ceres.hpp"

struct PBtype { double value; bool use; };
struct ObsMea { int sys; PBtype* RTK_Npoint[2]; };
struct mea_t { int obs_count; ObsMea* obs_data; };

int main() {
    // eight ambiguities in the tail, in this order; a ninth that is not in it
    PBtype N[9] = { { 3.02, false }, { -7.05, false }, { 11.00, false }, { 0.96, false }, { 5.51, false }, { -2.47, false },
                    { 8.49, false }, { 4.03, false }, { 1.25, false } };
    ObsMea newest[5] = { { 0, { &N[0], &N[4] } }, { 0, { &N[1], &N[5] } }, { 0, { &N[2], &N[6] } }, { 0, { &N[3], nullptr } }, { 1, { &N[8], nullptr } } };
    ObsMea older[3] = { { 0, { &N[3], &N[4] } }, { 0, { &N[7], nullptr } }, { 0, { &N[2], nullptr } } };
    mea_t r0 = { 3, older }, r1 = { 5, newest };
    std::vector<mea_t*> rovers;
    rovers.push_back(&r0); rovers.push_back(&r1);
    auto tail_of = [&](const double* v) -> int {
        for (int i = 0; i < 8; i++) if (v == &N[i].value) return i;
        return -1;
    };
    swf_ceres::DoubleDifferenceSelection sel;
    if (!swf_ceres::SelectDoubleDifferences(rovers, 2, tail_of, 8, 1.4, &sel)) { std::printf("selection failed\n"); return 1; }
    std::printf("counts %d %d %d %d\n", (int)sel.pairs.size(), sel.last_count, sel.last_ref_count, sel.info);
    for (size_t i = 0; i < sel.pairs.size(); i++) std::printf("pair %d %d\n", sel.pairs[i].first, sel.pairs[i].second);
    return 0;
}
