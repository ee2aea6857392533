// The seed mini-solve of GnssPreprocess (R/swf/swf_gnss.cpp:534-575) and the first fix of GnssProcess (:203-215) bound to the device
// through swf_ceres::GnssEpochSolve, driven with stand-in structs that carry the reference's member names.  One epoch of twelve
// observations over three systems at a known truth: observation 3 is under the elevation mask, 9 is unhealthy (the reference still
// takes its carrier phase), 6 has no RTK ambiguity, 5 has a pseudorange sigma above the limit; ambiguities 0, 4 and 8 are young
// (continue_count <= 10) and carry a wrong value.  Run 1 is the seed preset with every switch on; run 2 the first fix on the rover-only
// rows (no base) with the start-up weight, from 4 km off.  Prints what was handed over and what came back; exit status 0 on success,
// 1 when the call fails (e.g. without a GPU), 2 when the solution is not the truth.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "swf_ceres.hpp"

namespace {
const int NFREQ = 2, MAXOBS = 16;
struct Amb { double value; int continue_count; };
struct Obs {
    uint8_t sat, sys, SVH;
    double RTK_L[NFREQ], RTK_Lstd[NFREQ], RTK_P[NFREQ], RTK_Pstd[NFREQ];
    double SPP_P[NFREQ], SPP_Pstd[NFREQ], SPP_L[NFREQ], SPP_Lstd[NFREQ], SPP_P0[NFREQ], SPP_D[NFREQ], SPP_Dstd[NFREQ];
    double ion_var, trop_var, sat_var;
    double satellite_pos[3], satellite_vel[3], el;
    Amb* RTK_Npoint[NFREQ];
    Amb* SPP_Npoint[NFREQ];
    Amb* SPP_Npoint_PCottections[NFREQ];
};
struct Epoch { int obs_count; Obs obs_data[MAXOBS]; double base_xyz[3]; double br_time_diff; };

const double CL = 299792458.0, OM = 7.2921151467E-5;
double range_m(const double* rr, const double* rs) {          // geometric range plus the Earth-rotation term
    const double dx = rr[0] - rs[0], dy = rr[1] - rs[1], dz = rr[2] - rs[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz) + OM * (rs[0] * rr[1] - rs[1] * rr[0]) / CL;
}
double rate_ms(const double* xg, const double* v, const double* rs, const double* vs) {
    double e[3] = { xg[0] - rs[0], xg[1] - rs[1], xg[2] - rs[2] };
    const double r = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    double ee = 0;
    for (int k = 0; k < 3; k++) ee += (v[k] - vs[k]) * e[k] / r;
    return ee + OM / CL * (vs[1] * xg[0] + rs[1] * v[0] - vs[0] * xg[1] - rs[0] * v[1]);
}

void print_run(const char* tag, const double* pose, const double* sb, const double* base, const double* dt, const swf_ceres::GnssEpochResult& res) {
    std::printf("in %s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, pose[0], pose[1], pose[2], sb[0], sb[1], sb[2], base[0], base[1], base[2]);
    std::printf("clk %s", tag);
    for (int k = 0; k < SWF_GES_CLOCKS; k++) std::printf(" %.17g", dt[k]);
    std::printf("\n");
    for (size_t k = 0; k < res.rows.size(); k++) {
        std::printf("rec %s %d %d %d %d %d %d", tag, res.rows[k].obs, res.rows[k].f, res.rows[k].kind, res.rows[k].correction ? 1 : 0,
                    (int)res.rec[k * 4 + 1], (int)res.rec[k * 4 + 2]);
        for (int j = 0; j < SWF_GES_DOUBLES; j++) std::printf(" %.17g", res.dat[k * SWF_GES_DOUBLES + j]);
        std::printf("\n");
    }
}
void print_out(const char* tag, const swf_ceres::GnssEpochResult& res) {
    std::printf("out %s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", tag, res.pos[0], res.pos[1], res.pos[2], res.vel[0], res.vel[1], res.vel[2],
                res.cost, (int)res.iters, (int)res.status);
    std::printf("oclk %s", tag);
    for (int k = 0; k < SWF_GES_CLOCKS; k++) std::printf(" %.17g", res.clock[k]);
    std::printf("\n");
    for (size_t k = 0; k < res.rows.size(); k++) std::printf("row %s %d %.17g %.17g\n", tag, (int)k, res.N[k], res.r[k]);
}
}  // namespace

int main() {
    static Epoch ep;
    static Amb rtk_amb[MAXOBS], spp_amb[MAXOBS], cor_amb[MAXOBS];
    const double pos_t[3] = { 120.0, -340.0, 55.0 }, vel_t[3] = { 4.0, -7.5, 0.5 };
    const double base[3] = { -2.1e6, 4.6e6, 3.9e6 };
    const double lams[3][2] = { { 0.1903, 0.2442 }, { 0.1920, 0.2484 }, { 0.2548, 0.2362 } };
    double dt_t[SWF_GES_CLOCKS];
    for (int k = 0; k < SWF_GES_CLOCKS; k++) dt_t[k] = k == 12 ? -35.0 : 2.0e4 * (k - 5.5);
    const int sys_of[12] = { 0, 0, 0, 0, 0, 1, 1, 1, 2, 0, 2, 2 };
    const double xg[3] = { pos_t[0] + base[0], pos_t[1] + base[1], pos_t[2] + base[2] };
    const double up[3] = { base[0] / 6.4e6, base[1] / 6.4e6, base[2] / 6.4e6 };
    ep.obs_count = 12; ep.br_time_diff = 0.4;
    for (int k = 0; k < 3; k++) ep.base_xyz[k] = base[k];
    for (int i = 0; i < ep.obs_count; i++) {
        Obs& d = ep.obs_data[i];
        d = Obs();
        d.sat = (uint8_t)(i + 1); d.sys = (uint8_t)sys_of[i]; d.SVH = i == 9 ? 1 : 0;
        // a direction around the local vertical: tilt 0.25 .. 1.0 rad, azimuth stepping by 2.4 rad
        const double tilt = 0.25 + 0.07 * i, az = 2.4 * i;
        double a[3] = { -up[1], up[0], 0.0 }, na = std::sqrt(a[0] * a[0] + a[1] * a[1]);
        for (int k = 0; k < 3; k++) a[k] /= na;
        const double b[3] = { up[1] * a[2] - up[2] * a[1], up[2] * a[0] - up[0] * a[2], up[0] * a[1] - up[1] * a[0] };
        for (int k = 0; k < 3; k++) {
            d.satellite_pos[k] = base[k] + 2.2e7 * (std::cos(tilt) * up[k] + std::sin(tilt) * (std::cos(az) * a[k] + std::sin(az) * b[k]));
            d.satellite_vel[k] = 1500.0 * std::sin(1.3 * i + k) + 600.0 * (k - 1);
        }
        d.el = i == 3 ? 0.30 : 1.5707963267948966 - tilt;
        d.ion_var = 0.4; d.trop_var = 0.1; d.sat_var = 0.2;
        const double lam = lams[d.sys][0], rho = range_m(xg, d.satellite_pos), z = 1e-3 * (i % 3 - 1);
        rtk_amb[i].value = 100.0 + 7.0 * i; rtk_amb[i].continue_count = 40;
        spp_amb[i].value = -50.0 + 11.0 * i; spp_amb[i].continue_count = 40;
        cor_amb[i].value = 3.0 + i; cor_amb[i].continue_count = 40;
        d.RTK_Npoint[0] = i == 6 ? nullptr : &rtk_amb[i];
        d.SPP_Npoint[0] = &spp_amb[i];
        d.SPP_Npoint_PCottections[0] = i % 2 ? &cor_amb[i] : nullptr;
        d.RTK_L[0] = (rho - rtk_amb[i].value * lam + dt_t[d.sys * 2] - 2 * z) / lam; d.RTK_Lstd[0] = 0.01;
        d.RTK_P[0] = rho + dt_t[d.sys * 2] + 100 * z; d.RTK_Pstd[0] = i == 5 ? 2.5 : 0.3;
        d.SPP_P[0] = rho + dt_t[6 + d.sys * 2] - 150 * z; d.SPP_Pstd[0] = 0.5;
        d.SPP_L[0] = (rho + dt_t[6 + d.sys * 2] - spp_amb[i].value * lam + 3 * z) / lam; d.SPP_Lstd[0] = 0.02;
        d.SPP_P0[0] = rho + dt_t[6 + d.sys * 2] - cor_amb[i].value * lam + 80 * z;
        d.SPP_D[0] = (-(rate_ms(xg, vel_t, d.satellite_pos, d.satellite_vel) + dt_t[12]) + 20 * z) / lam; d.SPP_Dstd[0] = 0.05;
    }
    for (int i = 0; i < 12; i += 4) { rtk_amb[i].continue_count = 3; rtk_amb[i].value += 500.0; spp_amb[i].continue_count = 10; spp_amb[i].value -= 900.0; }
    for (int i = 0; i < ep.obs_count; i++) {
        const Obs& d = ep.obs_data[i];
        std::printf("obs %d %d %d %.17g %.17g %.17g\n", i, (int)d.SVH, (int)d.sys, d.el, d.RTK_Pstd[0], ep.br_time_diff);
    }
    int bad = 0;
    {   // ---- the seed preset: pose and speed-bias at the truth, clocks 12 m off
        double pose[7] = { pos_t[0], pos_t[1], pos_t[2], 0, 0, 0, 1 }, sb[9] = { vel_t[0], vel_t[1], vel_t[2], 0, 0, 0, 0, 0, 0 }, dt[SWF_GES_CLOCKS];
        for (int k = 0; k < SWF_GES_CLOCKS; k++) dt[k] = dt_t[k] + (k % 2 ? 12.0 : -12.0);
        swf_ceres::GnssEpochOptions opt;
        opt.use_spp_correction = true; opt.nfreq = 1;
        swf_ceres::GnssEpochResult res;
        double dt_in[SWF_GES_CLOCKS];
        for (int k = 0; k < SWF_GES_CLOCKS; k++) dt_in[k] = dt[k];
        if (!swf_ceres::GnssEpochSolve(ep, pose, sb, dt, lams, opt, swf_ceres::GnssEpochSeed, &res)) {
            std::printf("GnssEpochSolve (seed) failed: %s\n", swf_last_error());
            return 1;
        }
        print_run("seed", pose, sb, ep.base_xyz, dt_in, res);
        print_out("seed", res);
        for (int k = 0; k < SWF_GES_CLOCKS; k++) if (res.clk_rows[k] > 0 && std::fabs(dt[k] - dt_t[k]) > 0.5) bad++;
        if (std::fabs(rtk_amb[0].value - 100.0) > 0.5 || std::fabs(spp_amb[4].value - (-50.0 + 44.0)) > 0.5) bad++;       // the young ones were re-seeded
        if (rtk_amb[1].value != 107.0 || res.status != SWF_GES_CONVERGED || !res.have_base) bad++;
    }
    {   // ---- the first fix on the rover-only rows, 4 km off, zero velocity and clocks
        double pose[7] = { pos_t[0] + 2500.0, pos_t[1] - 2400.0, pos_t[2] + 2000.0, 0, 0, 0, 1 }, sb[9] = { 0 }, dt[SWF_GES_CLOCKS] = { 0 };
        const double pose_in[3] = { pose[0], pose[1], pose[2] }, sb_in[3] = { 0, 0, 0 }, dt_in[SWF_GES_CLOCKS] = { 0 };
        swf_ceres::GnssEpochOptions opt;
        opt.use_rtk = false; opt.use_rtd = false; opt.startup = true; opt.nfreq = 1;
        swf_ceres::GnssEpochResult res;
        if (!swf_ceres::GnssEpochSolve(ep, pose, sb, dt, lams, opt, swf_ceres::GnssEpochFirstFix, &res)) {
            std::printf("GnssEpochSolve (first fix) failed: %s\n", swf_last_error());
            return 1;
        }
        print_run("fix", pose_in, sb_in, ep.base_xyz, dt_in, res);
        print_out("fix", res);
        for (int k = 0; k < 3; k++) if (std::fabs(pose[k] - pos_t[k]) > 2.0 || std::fabs(sb[k] - vel_t[k]) > 0.5) bad++;
        if (res.status != SWF_GES_CONVERGED || res.have_base) bad++;
    }
    std::printf("expected %d\n", bad == 0 ? 1 : 0);
    return bad == 0 ? 0 : 2;
}
