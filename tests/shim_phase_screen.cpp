// GnssPreprocess's pre-fit screen (R/swf/swf_gnss.cpp:337-499) bound to the device through swf_ceres::PhaseScreen, driven with
// stand-in structs that carry the reference's member names.  One epoch of ten observations: a clean majority, an RTK slip of one
// cycle (observation 2), an observation under the elevation mask (3), a rover-only slip of three cycles (4), a code-minus-phase
// jump (1), an RTK phase without an ambiguity (6), one whose slip counter moved on (7) and an unhealthy satellite (9).
// Prints the epoch as it was handed over and the flags that came back; exit status 0 on success, 1 when the call fails (e.g.
// without a GPU).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "swf_ceres.hpp"

namespace {
const int NFREQ = 2, MAXOBS = 16;
struct Amb { double value; uint8_t SLIP_COUNT; };
struct Obs {
    uint8_t sat, sys, SVH;
    uint8_t RTK_SLIP_COUNT[NFREQ], SPP_SLIP_COUNT[NFREQ];
    double SPP_P[NFREQ], SPP_L[NFREQ], RTK_L[NFREQ];
    double satellite_pos[3], el;
    Amb* RTK_Npoint[NFREQ];
    Amb* SPP_Npoint[NFREQ];
};
struct Epoch { int obs_count; Obs obs_data[MAXOBS]; double base_xyz[3]; };

double range_m(const double* rr, const double* rs) {          // geometric range plus the Earth-rotation term
    const double dx = rr[0] - rs[0], dy = rr[1] - rs[1], dz = rr[2] - rs[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz) + 7.2921151467E-5 * (rs[0] * rr[1] - rs[1] * rr[0]) / 299792458.0;
}
}  // namespace

int main() {
    static Epoch ep;
    static Amb rtk_amb[MAXOBS], spp_amb[MAXOBS];
    const double pose[7] = { 10.0, -20.0, 5.0, 0, 0, 0, 1 };
    const double base[3] = { -2.1e6, 4.6e6, 3.9e6 };
    const double lams[3][2] = { { 0.1903, 0.2442 }, { 0.1920, 0.2484 }, { 0.2548, 0.2362 } };
    double dt[12];
    for (int k = 0; k < 12; k++) dt[k] = 3.0 * k - 11.5;
    const double el_min = 25.0 * 3.14159265358979323846 / 180.0;
    const int mode = SWF_SCR_GATE_RTK | SWF_SCR_GATE_SPP;
    const int sys_of[10] = { 0, 0, 0, 0, 0, 1, 1, 2, 2, 0 };
    const double xg[3] = { pose[0] + base[0], pose[1] + base[1], pose[2] + base[2] };
    ep.obs_count = 10;
    for (int k = 0; k < 3; k++) ep.base_xyz[k] = base[k];
    for (int i = 0; i < ep.obs_count; i++) {
        Obs& d = ep.obs_data[i];
        d = Obs();
        d.sat = (uint8_t)(i + 1); d.sys = (uint8_t)sys_of[i]; d.SVH = i == 9 ? 1 : 0;
        const double a = 0.7 * i + 0.3, b = 0.4 + 0.1 * i;
        d.satellite_pos[0] = 2.2e7 * std::cos(a) * std::cos(b); d.satellite_pos[1] = 2.2e7 * std::sin(a) * std::cos(b);
        d.satellite_pos[2] = 2.2e7 * std::sin(b);
        d.el = i == 3 ? 0.30 : 0.6 + 0.08 * i;
        const double lam = lams[d.sys][0], rho = range_m(xg, d.satellite_pos), noise = 1e-3 * (i % 3 - 1);
        rtk_amb[i].value = 100.0 + 7.0 * i; rtk_amb[i].SLIP_COUNT = 3;
        spp_amb[i].value = -50.0 + 11.0 * i; spp_amb[i].SLIP_COUNT = 5;
        d.RTK_SLIP_COUNT[0] = i == 7 ? 4 : 3; d.SPP_SLIP_COUNT[0] = 5;
        d.RTK_Npoint[0] = i == 6 ? nullptr : &rtk_amb[i];
        d.SPP_Npoint[0] = &spp_amb[i];
        d.RTK_L[0] = (rho - rtk_amb[i].value * lam + dt[d.sys * 2] - (0.4 + noise)) / lam + (i == 2 ? 1.0 : 0.0);
        d.SPP_L[0] = (rho - spp_amb[i].value * lam + dt[6 + d.sys * 2] - (-0.7 + noise)) / lam + (i == 4 ? 3.0 : 0.0);
        const double s = std::sin(d.el);
        d.SPP_P[0] = (d.SPP_L[0] + spp_amb[i].value) * lam + (i == 1 ? 30.0 : 2.0) / (s * s);
    }
    std::printf("epoch %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g\n", pose[0], pose[1], pose[2], base[0], base[1], base[2], mode, el_min);
    for (int s = 0; s < 3; s++) for (int f = 0; f < NFREQ; f++) std::printf("lam %d %d %.17g\n", s, f, lams[s][f]);
    for (int k = 0; k < 12; k++) std::printf("dt %d %.17g\n", k, dt[k]);
    for (int i = 0; i < ep.obs_count; i++) {
        const Obs& d = ep.obs_data[i];
        std::printf("obs %d %d %d %.17g %.17g %.17g %.17g\n", i, (int)d.SVH, (int)d.sys, d.el, d.satellite_pos[0], d.satellite_pos[1], d.satellite_pos[2]);
        for (int f = 0; f < NFREQ; f++) {
            const Amb* r = d.RTK_Npoint[f]; const Amb* p = d.SPP_Npoint[f];
            std::printf("obsf %d %d %.17g %.17g %.17g %d %.17g %d %d %.17g %d\n", i, f, d.RTK_L[f], d.SPP_L[f], d.SPP_P[f],
                        r ? 1 : 0, r ? r->value : 0.0, r && r->SLIP_COUNT == d.RTK_SLIP_COUNT[f] ? 1 : 0,
                        p ? 1 : 0, p ? p->value : 0.0, p && p->SLIP_COUNT == d.SPP_SLIP_COUNT[f] ? 1 : 0);
        }
    }
    swf_ceres::PhaseScreenResult res;
    if (!swf_ceres::PhaseScreen(ep, pose, ep.base_xyz, lams, dt, mode, el_min, &res, NFREQ)) {
        std::printf("PhaseScreen failed: %s\n", swf_last_error());
        return 1;
    }
    for (int i = 0; i < ep.obs_count; i++)
        for (int f = 0; f < NFREQ; f++)
            std::printf("flag %d %d %d %d %.17g %.17g\n", i, f, (int)res.rtk[i * NFREQ + f], (int)res.spp[i * NFREQ + f],
                        res.rtk_r[i * NFREQ + f], res.spp_r[i * NFREQ + f]);
    std::printf("reset");
    for (size_t k = 0; k < res.reset.size(); k++) std::printf(" %d", (int)res.reset[k]);
    std::printf("\n");
    for (int k = 0; k < 2; k++) for (int g = 0; g < SWF_SCR_GROUPS; g++) std::printf("med %d %d %d %.17g\n", k, g, (int)res.cnt[k][g], res.med[k][g]);
    const bool expected = res.new_rtk(2, 0) && res.new_spp(2, 0) && !res.new_rtk(0, 0) && res.new_spp(1, 0) && res.new_spp(4, 0) &&
                          res.new_rtk(6, 0) && res.new_rtk(7, 0) && res.rtk[3 * NFREQ] == SWF_SCR_MASKED && res.rtk[9 * NFREQ] == 0;
    std::printf("expected %d\n", expected ? 1 : 0);
    return expected ? 0 : 2;
}
