// swf_ceres.hpp — header-only C++ adapter: the ceres::Problem / ceres::Solver names the
// reference's estimator uses, implemented over the C-ABI of swf_solver.h.
//
// Purpose: estimator code written in the reference's style —
//     ceres::LossFunction* loss = new ceres::CauchyLoss(1.0);
//     projection_factor* f = new projection_factor(pts);
//     my_problem.AddResidualBlock(f, loss, para_pose[j], para_ex_Pose[0], point.data());
//     ceres::Solve(my_options, &my_problem, &summary);
// — compiles against this header instead of <ceres/ceres.h> + the reference's factor headers.
// The factor classes below carry only the CONSTRUCTOR ARGUMENTS (data); their arithmetic runs in
// the HIP kernels.  Nothing here evaluates a residual on the CPU.
//
// Mapping (reference file:line -> here):
//   projection_factor(pts)                      R/factor/projection_factor.h:9-18     -> swf_add_projection
//   IMUFactor(pre_integration)                  R/factor/imu_factor.h:7-19            -> swf_add_imu (SWF_PRE_DOUBLES record; from an
//                                                                                        IntegrationBase* or from the record itself)
//   RTKCarrierPhaseFactor(...)                  R/factor/gnss_factor.h:8-40           -> swf_add_rtk_carrier_phase
//   RTKPseudorangeFactor(...)                   R/factor/gnss_factor.h:43-66          -> swf_add_rtk_pseudorange
//   SppDopplerFactor(...)                       R/factor/gnss_factor.h:108-131        -> swf_add_doppler
//   SppPseudorangeFactor(...)                   R/factor/gnss_factor.h:70-83          -> swf_add_spp_pseudorange
//   SppCarrierPhaseFactor(...)                  R/factor/gnss_factor.h:88-104         -> swf_add_spp_carrier_phase
//   FixedIntegerFactor(N21, istd)               R/factor/gnss_factor.h:135-143        -> swf_add_fixed_integer
//   ProjectionTwoFrameOneCamFactor(pts_i, pts_j) / TwoFrameTwoCam / OneFrameTwoCam
//                                               R/factor/projection_factor.h:33-66    -> swf_add_projection_inverse_depth
//   IMUGNSSFactor(IMUGNSSBase*)                 R/factor/gnss_imu_factor.h:19-151     -> swf_add_imu_gnss (IMUGNSSInfo below)
//   InitialBlackFactor(istd)                    R/factor/initial_factor.h:42-48       -> swf_add_scalar_prior
//   MarginalizationFactor(info)                 R/factor/marginalization_factor.h:104-110 -> swf_add_linear_prior (from a
//                                                                                        MarginalizationInfo* or from J, r0, x0)
//   ImuIntegrate() + IMUProcess()               R/swf/swf_imu.cpp:117-213             -> swf_imu_frame_batch (ImuIntegrate below)
//   initFramePoseByPnP() + solvePoseByPnP()     R/feature/feature_manager.cpp:164-243 -> swf_pnp_frame_batch (InitFramePoseByPnP below)
//   rejectWithF() + undistortedPts() + ptsVelocity()  R/feature/feature_tracker.cpp:265-294, :334-376 -> swf_track_reject_batch (RejectWithF below)
//   trackImage(): calcOpticalFlowPyrLK forward + reverse, the 0.5 px gate, inBorder   R/feature/feature_tracker.cpp:98-141 -> swf_klt_track_batch (TrackImageKLT below)
//   trackImage(): setMask() + cv::goodFeaturesToTrack + addPoints()   R/feature/feature_tracker.cpp:148-165, :44-79 -> swf_gftt_detect_batch (DetectFeatures below)
//   FeatureTracker::trackImage() + removeOutliers(), the state from frame to frame   R/feature/feature_tracker.cpp:88-263 -> swf_tracker_* (FeatureTracker below)
//   FeatureManager: addFeatureCheckParallax() removeOut() triangulate() removeFailures() CheckParallax() removeBack() removeFront()
//                                               R/feature/feature_manager.cpp         -> swf_ftable_* (FeatureManager below)
//   ceres::internal::{parameter_head,is_optimize,lhs_out,rhs_out,lhs_out2,hs_row}
//                                               R/swf/swf_gnss.cpp:25-94              -> swf_ceres::internal::* below
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "swf_solver.h"

namespace swf_ceres {

enum LinearSolverType { DENSE_SCHUR };
enum TrustRegionStrategyType { LEVENBERG_MARQUARDT, DOGLEG };      // ceres' default is LEVENBERG_MARQUARDT; R/swf/swf.cpp:26 sets DOGLEG

class LossFunction { public: virtual ~LossFunction() {} virtual double a() const = 0; };
class CauchyLoss : public LossFunction { public: explicit CauchyLoss(double a) : a_(a) {} double a() const override { return a_; } private: double a_; };
class LocalParameterization { public: virtual ~LocalParameterization() {} };

// ---- typed cost functions (data carriers) ------------------------------------------------
struct CostFunction { virtual ~CostFunction() {} };
struct projection_factor : CostFunction {
    double uv[2];
    static double& sqrt_info() { static double v = 1000.0 / 1.5; return v; }   // R/swf/swf.cpp:47
    template <class V3> explicit projection_factor(const V3& pts) { uv[0] = pts[0]; uv[1] = pts[1]; }
};
struct IMUFactor : CostFunction {
    std::vector<double> pre;   // SWF_PRE_DOUBLES record, see include/swf_types.h
    explicit IMUFactor(const double* record) : pre(record, record + SWF_PRE_DOUBLES) {}
    // The reference's own constructor, IMUFactor(IntegrationBase* _pre_integration) (R/factor/imu_factor.h:11): any type with the
    // member names of R/factor/integration_base.h:28-47 (Eigen or not: only operator()(i), operator()(i, j) and x() y() z() w() are
    // used) is copied into the record — delta_p / delta_q / delta_v, the linearisation biases, the five bias blocks of `jacobian`
    // (O_P = 0, O_R = 3, O_V = 6, O_BA = 9, O_BG = 12, R/factor/integration_base.h and utility.h), sum_dt, gyri / gyrj, and
    // get_sqrtinfo() (what IMUFactor::Evaluate whitens with, R/factor/imu_factor.cpp:26).  A snapshot: re-propagate -> a new factor,
    // as the reference does (it deletes and re-adds its IMU factors with every window, R/swf/swf_image.cpp:198-251).
    template <class IB, class = decltype(std::declval<IB&>().delta_p(0)), class = decltype(std::declval<IB&>().get_sqrtinfo())>
    explicit IMUFactor(IB* ib) : pre(SWF_PRE_DOUBLES, 0.0) {
        for (int k = 0; k < 3; k++) {
            pre[SWF_PRE_DP + k] = ib->delta_p(k); pre[SWF_PRE_DV + k] = ib->delta_v(k);
            pre[SWF_PRE_LBA + k] = ib->linearized_ba(k); pre[SWF_PRE_LBG + k] = ib->linearized_bg(k);
            pre[SWF_PRE_GYRI + k] = ib->gyri(k); pre[SWF_PRE_GYRJ + k] = ib->gyrj(k);
        }
        pre[SWF_PRE_DQ + 0] = ib->delta_q.x(); pre[SWF_PRE_DQ + 1] = ib->delta_q.y(); pre[SWF_PRE_DQ + 2] = ib->delta_q.z(); pre[SWF_PRE_DQ + 3] = ib->delta_q.w();
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
            pre[SWF_PRE_DP_DBA + 3 * i + j] = ib->jacobian(0 + i, 9 + j); pre[SWF_PRE_DP_DBG + 3 * i + j] = ib->jacobian(0 + i, 12 + j);
            pre[SWF_PRE_DQ_DBG + 3 * i + j] = ib->jacobian(3 + i, 12 + j);
            pre[SWF_PRE_DV_DBA + 3 * i + j] = ib->jacobian(6 + i, 9 + j); pre[SWF_PRE_DV_DBG + 3 * i + j] = ib->jacobian(6 + i, 12 + j);
        }
        pre[SWF_PRE_SUMDT] = ib->sum_dt;
        const auto si = ib->get_sqrtinfo();
        for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) pre[SWF_PRE_SQRTINFO + 15 * i + j] = si(i, j);
    }
};
struct RTKCarrierPhaseFactor : CostFunction {
    double dat[SWF_CP_DOUBLES];
    RTKCarrierPhaseFactor(const double* sat, double L1_lam, double lam, double el, double br_time_diff, double mea_var,
                          const double* /*base_pos: window constant*/, bool use_istd, int /*sys*/, int /*f*/) {
        dat[0] = sat[0]; dat[1] = sat[1]; dat[2] = sat[2]; dat[3] = L1_lam; dat[4] = lam; dat[5] = el;
        dat[6] = br_time_diff; dat[7] = mea_var; dat[8] = use_istd ? 1.0 : 0.0;
    }
};
struct RTKPseudorangeFactor : CostFunction {
    double dat[SWF_PR_DOUBLES];
    RTKPseudorangeFactor(const double* sat, double P1, double el, double br_time_diff, double mea_var, const double* /*base_pos*/) {
        dat[0] = sat[0]; dat[1] = sat[1]; dat[2] = sat[2]; dat[3] = P1; dat[4] = el; dat[5] = br_time_diff; dat[6] = mea_var;
    }
};
struct SppDopplerFactor : CostFunction {
    double dat[SWF_DOP_DOUBLES];
    SppDopplerFactor(const double* satv, const double* sat, const double* /*xyzt*/, double D1_lam, double istd, const double* /*base_pos*/) {
        for (int k = 0; k < 3; k++) { dat[k] = sat[k]; dat[3 + k] = satv[k]; }
        dat[6] = D1_lam; dat[7] = istd;
    }
};
struct SppPseudorangeFactor : CostFunction {
    double dat[SWF_SPR_DOUBLES];
    SppPseudorangeFactor(const double* sat, double P1, double istd, const double* /*base_pos*/) {
        dat[0] = sat[0]; dat[1] = sat[1]; dat[2] = sat[2]; dat[3] = P1; dat[4] = istd;
    }
};
struct SppCarrierPhaseFactor : CostFunction {
    double dat[SWF_SCP_DOUBLES];
    SppCarrierPhaseFactor(const double* sat, double L1_lam, double istd, const double* /*base_pos*/, double lam) {
        dat[0] = sat[0]; dat[1] = sat[1]; dat[2] = sat[2]; dat[3] = L1_lam; dat[4] = istd; dat[5] = lam;
    }
};
struct FixedIntegerFactor : CostFunction { double N21, istd; FixedIntegerFactor(double N21_, double istd_) : N21(N21_), istd(istd_) {} };
// What IMUGNSSBase holds when SetLastImuFactor adds its factor (R/factor/gnss_imu_factor.cpp:99-119), as plain arrays: a maintainer
// fills it from gnss_poses / gnss_speed_bias (the hidden epochs' parameter memory, updated in place by every Solve), their
// *_lin points, pose_hessians, pose_phase_biases_hessians, pose_rhses, phase_biases_hessians, phase_biases_rhs and the M + 1
// pre-integrations (imu_factors[k]->pre_integration, last_imu_factor) in SWF_PRE_DOUBLES records.
// (the static sqrt_info of each class lives in a class template's static member: one definition across translation units without
// C++17 inline variables — the reference builds with -std=c++14, rtk_visual_inertial/CMakeLists.txt:5)
template <class Tag> struct SqrtInfoOf { static double sqrt_info; };
template <class Tag> double SqrtInfoOf<Tag>::sqrt_info = 0;
struct ProjectionTwoFrameOneCamFactor : CostFunction, SqrtInfoOf<ProjectionTwoFrameOneCamFactor> {
    double pi[3], pj[3];
    ProjectionTwoFrameOneCamFactor(const double* pts_i, const double* pts_j) { for (int k = 0; k < 3; k++) { pi[k] = pts_i[k]; pj[k] = pts_j[k]; } }
};
struct ProjectionTwoFrameTwoCamFactor : CostFunction, SqrtInfoOf<ProjectionTwoFrameTwoCamFactor> {
    double pi[3], pj[3];
    ProjectionTwoFrameTwoCamFactor(const double* pts_i, const double* pts_j) { for (int k = 0; k < 3; k++) { pi[k] = pts_i[k]; pj[k] = pts_j[k]; } }
};
struct ProjectionOneFrameTwoCamFactor : CostFunction, SqrtInfoOf<ProjectionOneFrameTwoCamFactor> {
    double pi[3], pj[3];
    ProjectionOneFrameTwoCamFactor(const double* pts_i, const double* pts_j) { for (int k = 0; k < 3; k++) { pi[k] = pts_i[k]; pj[k] = pts_j[k]; } }
};
struct IMUGNSSInfo {
    int M = 0;                                     // hidden GNSS epochs
    double* hidden_pose = nullptr; double* hidden_sb = nullptr;        // [M][7], [M][9]
    std::vector<double> pose_lin, sb_lin, Hpp, HpN, rhs_p, HNN, rhsN, pre;
    int mid = 0; std::vector<double> H12;          // AddMidMargInfo's product (gnss_Index, pose1_pose2_hessians): link mid in 1..M-1, 15 x 15; 0 = none
    // filled by IMUGNSSFactor(IMUGNSSBase*) only: the reference keeps every hidden epoch in its own allocation (gnss_poses[k],
    // gnss_speed_bias[k]); the C-ABI wants [M][7] / [M][9], so the adapter owns contiguous copies (hidden_pose / hidden_sb point at
    // them), Solve() gathers them from the epochs' memory before the solve and scatters the updated values back after it
    std::vector<double*> pose_ptr, sb_ptr;
    std::vector<double> pose_buf, sb_buf;
    void gather() { for (size_t k = 0; k < pose_ptr.size(); k++) { std::memcpy(&pose_buf[7 * k], pose_ptr[k], 7 * sizeof(double)); std::memcpy(&sb_buf[9 * k], sb_ptr[k], 9 * sizeof(double)); } }
    void scatter() const { for (size_t k = 0; k < pose_ptr.size(); k++) { std::memcpy(pose_ptr[k], &pose_buf[7 * k], 7 * sizeof(double)); std::memcpy(sb_ptr[k], &sb_buf[9 * k], 9 * sizeof(double)); } }
};
struct IMUGNSSFactor : CostFunction {
    IMUGNSSInfo* info; std::unique_ptr<IMUGNSSInfo> owned;
    explicit IMUGNSSFactor(IMUGNSSInfo* i) : info(i) {}
    // The reference's own constructor, IMUGNSSFactor(IMUGNSSBase* IMUGNSS_info_) (R/factor/gnss_imu_factor.h:145-151): any type with the
    // member names of IMUGNSSBase (R/factor/gnss_imu_factor.h:19-140) as SetLastImuFactor leaves them (R/factor/gnss_imu_factor.cpp:99-119):
    // gnss_poses / gnss_speed_bias (the M hidden epochs' parameter memory) and their *_lin points, pose_hessians[k] (15 x 15),
    // pose_phase_biases_hessians[k] (15 x N), pose_rhses[k], phase_biases_hessians (N x N), phase_biases_rhs, the M pre-integrations
    // imu_factors[k]->pre_integration (epoch k-1 -> k; k = 0 starts at para_pose0) and last_imu_factor->pre_integration (epoch M-1 -> the
    // second visual frame), and — after AddMidMargInfo (:121-240) — gnss_middle_marginfo != 0, gnss_Index, pose1_pose2_hessians.
    // Only operator()(i), operator()(i, j) and size() of the matrix members are used (Eigen or not).  A snapshot, like the other
    // factors' constructors: the reference builds a new IMUGNSSFactor whenever it re-adds the residual block (SetLastImuFactor).
    template <class GB, class = decltype(std::declval<GB&>().gnss_poses), class = decltype(std::declval<GB&>().pose_phase_biases_hessians),
              class = decltype(std::declval<GB&>().last_imu_factor)>
    explicit IMUGNSSFactor(GB* b) : info(nullptr), owned(new IMUGNSSInfo()) {
        IMUGNSSInfo& I = *owned; info = owned.get();
        const int M = (int)b->gnss_poses.size(), N = (int)b->gnss_phase_biases.size();
        if (M < 1 || (int)b->gnss_speed_bias.size() != M || (int)b->imu_factors.size() != M || !b->last_imu_factor || (int)b->pose_hessians.size() != M)
            throw std::invalid_argument("IMUGNSSFactor: IMUGNSSBase holds no complete chain of hidden epochs");
        I.M = M;
        I.pose_ptr.assign(b->gnss_poses.begin(), b->gnss_poses.end()); I.sb_ptr.assign(b->gnss_speed_bias.begin(), b->gnss_speed_bias.end());
        I.pose_buf.resize((size_t)7 * M); I.sb_buf.resize((size_t)9 * M); I.gather();
        I.hidden_pose = I.pose_buf.data(); I.hidden_sb = I.sb_buf.data();
        I.pose_lin.resize((size_t)7 * M); I.sb_lin.resize((size_t)9 * M);
        I.Hpp.resize((size_t)225 * M); I.HpN.assign((size_t)15 * N * M, 0.0); I.rhs_p.resize((size_t)15 * M);
        I.HNN.resize((size_t)N * N); I.rhsN.resize((size_t)N); I.pre.resize((size_t)SWF_PRE_DOUBLES * (M + 1));
        for (int k = 0; k < M; k++) {
            std::memcpy(&I.pose_lin[7 * k], b->gnss_poses_lin[k], 7 * sizeof(double));
            std::memcpy(&I.sb_lin[9 * k], b->gnss_speed_bias_lin[k], 9 * sizeof(double));
            for (int i = 0; i < 15; i++) {
                for (int j = 0; j < 15; j++) I.Hpp[(size_t)225 * k + 15 * i + j] = b->pose_hessians[k](i, j);
                for (int j = 0; j < N; j++) I.HpN[((size_t)15 * k + i) * N + j] = b->pose_phase_biases_hessians[k](i, j);
                I.rhs_p[(size_t)15 * k + i] = b->pose_rhses[k](i);
            }
            const IMUFactor rec(b->imu_factors[k]->pre_integration);
            std::memcpy(&I.pre[(size_t)SWF_PRE_DOUBLES * k], rec.pre.data(), SWF_PRE_DOUBLES * sizeof(double));
        }
        const IMUFactor last(b->last_imu_factor->pre_integration);
        std::memcpy(&I.pre[(size_t)SWF_PRE_DOUBLES * M], last.pre.data(), SWF_PRE_DOUBLES * sizeof(double));
        for (int i = 0; i < N; i++) { I.rhsN[i] = b->phase_biases_rhs(i); for (int j = 0; j < N; j++) I.HNN[(size_t)i * N + j] = b->phase_biases_hessians(i, j); }
        if (b->gnss_middle_marginfo) {
            I.mid = b->gnss_Index; I.H12.resize(225);
            for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) I.H12[15 * i + j] = b->pose1_pose2_hessians(i, j);
        }
    }
};
struct InitialBlackFactor : CostFunction { double istd; explicit InitialBlackFactor(double w) : istd(w) {} };
// MarginalizationInfo's product: the linearised prior (J, r0, x0) over its kept blocks
struct MarginalizationFactor : CostFunction {
    std::vector<double> J, r0, x0;
    MarginalizationFactor(const double* J_, const double* r0_, const double* x0_, int dim, int global_sum)
        : J(J_, J_ + (size_t)dim * dim), r0(r0_, r0_ + dim), x0(x0_, x0_ + global_sum) {}
    // The reference's own constructor, MarginalizationFactor(MarginalizationInfo*) (R/factor/marginalization_factor.h:106,
    // .cpp:401-408): any type with its members n, m, keep_block_size (global sizes), keep_block_idx (position of the block's local
    // dimensions among the prior's columns, offset by m), keep_block_data (the linearisation point per block), linearized_jacobians
    // (n x n) and linearized_residuals (n), as MarginalizationFactor::Evaluate reads them (R/factor/marginalization_factor.cpp:410-446).
    // The columns are re-filed in the order of the blocks — the order of the parameter blocks handed to AddResidualBlock, which is the
    // order swf_add_linear_prior expects — so a keep_block_idx that does not ascend with the blocks is handled here.
    template <class MI, class = decltype(std::declval<MI&>().keep_block_idx), class = decltype(std::declval<MI&>().linearized_jacobians(0, 0))>
    explicit MarginalizationFactor(MI* mi) {
        const int n = mi->n, m = mi->m, nb = (int)mi->keep_block_size.size();
        J.assign((size_t)n * n, 0.0); r0.resize(n);
        for (int k = 0; k < n; k++) r0[k] = mi->linearized_residuals(k);
        int col = 0;
        for (int b = 0; b < nb; b++) {
            const int gs = mi->keep_block_size[b], ls = gs == 7 ? 6 : gs, idx = mi->keep_block_idx[b] - m;
            for (int r = 0; r < n; r++) for (int c = 0; c < ls; c++) J[(size_t)r * n + col + c] = mi->linearized_jacobians(r, idx + c);
            x0.insert(x0.end(), mi->keep_block_data[b], mi->keep_block_data[b] + gs);
            col += ls;
        }
        if (col != n) throw std::invalid_argument("MarginalizationFactor: the kept blocks' local sizes do not add up to n");
    }
};

class PoseLocalParameterization : public LocalParameterization {};   // R/factor/pose_local_parameterization.h

class ParameterBlockOrdering {
  public:
    void Clear() { keys_.clear(); groups_.clear(); }
    void AddElementToGroup(double* p, int group) { keys_.push_back(p); groups_.push_back(group); }
    int NumElements() const { return (int)keys_.size(); }
    std::vector<double*> keys_; std::vector<int32_t> groups_;
};

class Problem;
namespace internal {
// the modified Ceres' private globals under their own names, as the reference reads and writes them (R/swf/swf_gnss.cpp:20-94:
// the bodies of UpdateSchur / UpdateSchurHessianOnly compile unchanged against these): one object per program without C++17
// inline variables (the reference builds with -std=c++14) — the objects are static members of a class template, the names are
// namespace-scope references bound to them at static-initialisation time; no macros leak into the including translation unit.
// lhs_out (hs_row x hs_row, full symmetric, row-major) / rhs_out / lhs_out2 (the lower factor, row-major) /
// hs_row belong to the LAST successful Solve; a failed Solve and the destruction of the Problem they point into reset them to null.
// (Non-const pointers because the reference maps them with Eigen::Map<VectorXd> / Map<ceres::Matrix>; the memory is the solver's:
// read only.)
template <class = void> struct Globals {
    static std::vector<double*> parameter_head; static bool is_optimize;
    static double* lhs_out; static double* rhs_out; static double* lhs_out2; static int hs_row; static const Problem* owner;
};
template <class T> std::vector<double*> Globals<T>::parameter_head;
template <class T> bool Globals<T>::is_optimize = true;
template <class T> double* Globals<T>::lhs_out = nullptr;
template <class T> double* Globals<T>::rhs_out = nullptr;
template <class T> double* Globals<T>::lhs_out2 = nullptr;
template <class T> int Globals<T>::hs_row = 0;
template <class T> const Problem* Globals<T>::owner = nullptr;
#if defined(__GNUC__)
#define SWF_CERES_UNUSED __attribute__((unused))
#else
#define SWF_CERES_UNUSED
#endif
static std::vector<double*>& parameter_head SWF_CERES_UNUSED = Globals<>::parameter_head;
static bool& is_optimize SWF_CERES_UNUSED = Globals<>::is_optimize;
static double*& lhs_out SWF_CERES_UNUSED = Globals<>::lhs_out;
static double*& rhs_out SWF_CERES_UNUSED = Globals<>::rhs_out;
static double*& lhs_out2 SWF_CERES_UNUSED = Globals<>::lhs_out2;
static int& hs_row SWF_CERES_UNUSED = Globals<>::hs_row;
#undef SWF_CERES_UNUSED
inline void reset_exports() { Globals<>::lhs_out = Globals<>::rhs_out = Globals<>::lhs_out2 = nullptr; Globals<>::hs_row = 0; Globals<>::owner = nullptr; }
// the same four values as one struct (the accessor of rounds 1-4, kept for callers written against it)
struct Exports { const double* lhs_out = nullptr; const double* rhs_out = nullptr; const double* lhs_out2 = nullptr; int hs_row = 0; const Problem* owner = nullptr; };
inline Exports exports() { Exports e; e.lhs_out = Globals<>::lhs_out; e.rhs_out = Globals<>::rhs_out; e.lhs_out2 = Globals<>::lhs_out2; e.hs_row = Globals<>::hs_row; e.owner = Globals<>::owner; return e; }
// ceres::internal::ResidualBlock as the estimator sees it: a handle whose public is_use flag it flips directly
// (R/swf/swf_image.cpp:353-365,422; R/swf/swf_gnss.cpp:653).  Solve() carries the flags over to swf_factor_set_enabled.
struct ResidualBlock { bool is_use = true; swf_factor_id id = -1; };
}  // namespace internal

typedef internal::ResidualBlock* ResidualBlockId;

class Problem {
  public:
    Problem() { if (swf_problem_create(&h_) != SWF_OK) throw std::runtime_error("swf_problem_create"); }
    ~Problem() {
        if (internal::Globals<>::owner == this) internal::reset_exports();
        swf_problem_destroy(h_);
    }
    Problem(const Problem&) = delete;
    swf_problem* handle() { return h_; }

    void AddParameterBlock(double* p, int size, LocalParameterization* lp = nullptr) {
        chk(swf_add_parameter_block(h_, p, size, lp ? SWF_MANIFOLD_POSE : SWF_MANIFOLD_NONE), "AddParameterBlock");
        delete lp;                       // Problem takes ownership, as in ceres
    }
    bool HasParameterBlock(const double* p) const { return swf_has_parameter_block(h_, p) != 0; }
    void RemoveParameterBlock(double* p) { chk(swf_remove_parameter_block(h_, p), "RemoveParameterBlock"); }
    void SetParameterBlockConstant(double* p) { chk(swf_set_parameter_block_constant(h_, p), "SetParameterBlockConstant"); }
    void SetParameterBlockVariable(double* p) { chk(swf_set_parameter_block_variable(h_, p), "SetParameterBlockVariable"); }
    bool IsParameterBlockConstant(const double* p) const { return swf_is_parameter_block_constant(h_, p) != 0; }
    int ParameterBlockSize(const double* p) const { return swf_parameter_block_size(h_, p); }
    int NumParameterBlocks() const { return swf_num_parameter_blocks(h_); }
    int NumResidualBlocks() const { return swf_num_residual_blocks(h_); }
    void RemoveResidualBlock(ResidualBlockId rb) { chk(swf_remove_factor(h_, rb->id), "RemoveResidualBlock"); hidden_.erase(rb->id); }
    // the query surface GlobalMarge / FeatureManager walk (R/swf/swf_image.cpp:350-367, R/swf/swf.cpp:413-422)
    void GetResidualBlocks(std::vector<ResidualBlockId>* out) const {
        int32_t n = 0; chk(swf_get_residual_blocks(h_, nullptr, 0, &n), "GetResidualBlocks");
        std::vector<swf_factor_id> ids((size_t)n); chk(swf_get_residual_blocks(h_, ids.data(), n, &n), "GetResidualBlocks");
        out->clear(); for (swf_factor_id i : ids) out->push_back(handle_of(i));
    }
    void GetResidualBlocksForParameterBlock(const double* p, std::vector<ResidualBlockId>* out) const {
        int32_t n = 0; chk(swf_get_residual_blocks_for_parameter_block(h_, p, nullptr, 0, &n), "GetResidualBlocksForParameterBlock");
        std::vector<swf_factor_id> ids((size_t)n); chk(swf_get_residual_blocks_for_parameter_block(h_, p, ids.data(), n, &n), "GetResidualBlocksForParameterBlock");
        out->clear(); for (swf_factor_id i : ids) out->push_back(handle_of(i));
    }
    void GetParameterBlocks(std::vector<double*>* out) const {
        int32_t n = 0; chk(swf_get_parameter_blocks(h_, nullptr, 0, &n), "GetParameterBlocks");
        out->assign((size_t)n, nullptr); chk(swf_get_parameter_blocks(h_, out->data(), n, &n), "GetParameterBlocks");
    }
    void GetParameterBlocksForResidualBlock(const ResidualBlockId rb, std::vector<double*>* out) const {
        int32_t n = 0; chk(swf_get_parameter_blocks_for_residual_block(h_, rb->id, nullptr, 0, &n), "GetParameterBlocksForResidualBlock");
        out->assign((size_t)n, nullptr); chk(swf_get_parameter_blocks_for_residual_block(h_, rb->id, out->data(), n, &n), "GetParameterBlocksForResidualBlock");
    }
    // ResidualBlock::is_use -> swf_factor_set_enabled for every live residual block (called by Solve)
    int SyncIsUse() {
        int32_t n = 0; int rc = swf_get_residual_blocks(h_, nullptr, 0, &n);
        if (rc != SWF_OK) return rc;
        std::vector<swf_factor_id> ids((size_t)n);
        if ((rc = swf_get_residual_blocks(h_, ids.data(), n, &n)) != SWF_OK) return rc;
        for (swf_factor_id i : ids) if ((rc = swf_factor_set_enabled(h_, i, handle_of(i)->is_use ? 1 : 0)) != SWF_OK) return rc;
        return SWF_OK;
    }
    // hidden epochs of composite factors built from an IMUGNSSBase: epochs' own memory <-> the contiguous copies the solver works on
    void GatherHiddenEpochs() { for (auto& kv : hidden_) kv.second->gather(); }
    void ScatterHiddenEpochs() const { for (const auto& kv : hidden_) kv.second->scatter(); }
    void SetConstants(const double* pbg, const double* gw, const double* base) { chk(swf_set_constants(h_, pbg, gw, base), "SetConstants"); }

    // AddResidualBlock overloads by cost-function type; Problem takes ownership of cost and loss
    ResidualBlockId AddResidualBlock(projection_factor* f, LossFunction* loss, double* pose, double* ex, double* pt) {
        swf_factor_id id = swf_add_projection(h_, pose, ex, pt, f->uv, projection_factor::sqrt_info(), loss ? loss->a() : 0.0);
        delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(IMUFactor* f, LossFunction* loss, double* pi, double* si, double* pj, double* sj) {
        swf_factor_id id = swf_add_imu(h_, pi, si, pj, sj, f->pre.data()); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(RTKCarrierPhaseFactor* f, LossFunction* loss, double* pose, double* amb, double* clk) {
        swf_factor_id id = swf_add_rtk_carrier_phase(h_, pose, amb, clk, f->dat); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(RTKPseudorangeFactor* f, LossFunction* loss, double* pose, double* clk) {
        swf_factor_id id = swf_add_rtk_pseudorange(h_, pose, clk, f->dat); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(SppDopplerFactor* f, LossFunction* loss, double* sb, double* drift, double* pose) {
        swf_factor_id id = swf_add_doppler(h_, sb, drift, pose, f->dat); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(SppPseudorangeFactor* f, LossFunction* loss, double* pose, double* clk) {
        swf_factor_id id = swf_add_spp_pseudorange(h_, pose, clk, f->dat); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(SppCarrierPhaseFactor* f, LossFunction* loss, double* pose, double* clk, double* amb) {
        swf_factor_id id = swf_add_spp_carrier_phase(h_, pose, clk, amb, f->dat); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(FixedIntegerFactor* f, LossFunction* loss, double* n_a, double* n_b) {
        swf_factor_id id = swf_add_fixed_integer(h_, n_a, n_b, f->N21, f->istd); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(ProjectionTwoFrameOneCamFactor* f, LossFunction* loss, double* pose_i, double* pose_j, double* ex, double* inv_depth) {
        swf_factor_id id = swf_add_projection_inverse_depth(h_, 0, pose_i, pose_j, ex, nullptr, inv_depth, f->pi, f->pj, ProjectionTwoFrameOneCamFactor::sqrt_info, loss ? loss->a() : 0.0);
        delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(ProjectionTwoFrameTwoCamFactor* f, LossFunction* loss, double* pose_i, double* pose_j, double* ex, double* ex2, double* inv_depth) {
        swf_factor_id id = swf_add_projection_inverse_depth(h_, 1, pose_i, pose_j, ex, ex2, inv_depth, f->pi, f->pj, ProjectionTwoFrameTwoCamFactor::sqrt_info, loss ? loss->a() : 0.0);
        delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(ProjectionOneFrameTwoCamFactor* f, LossFunction* loss, double* ex, double* ex2, double* inv_depth) {
        swf_factor_id id = swf_add_projection_inverse_depth(h_, 2, nullptr, nullptr, ex, ex2, inv_depth, f->pi, f->pj, ProjectionOneFrameTwoCamFactor::sqrt_info, loss ? loss->a() : 0.0);
        delete f; delete loss; return ck(id);
    }
    // param = { pose_i, speed_bias_i, pose_j, speed_bias_j, ambiguity_0 .. ambiguity_N-1 } as SetLastImuFactor builds it
    ResidualBlockId AddResidualBlock(IMUGNSSFactor* f, LossFunction* loss, const std::vector<double*>& param) {
        const IMUGNSSInfo& I = *f->info;
        const int N = (int)param.size() - 4;
        swf_factor_id id = swf_add_imu_gnss(h_, param[0], param[1], param[2], param[3], param.data() + 4, N, I.M, I.hidden_pose, I.hidden_sb,
                                              I.pose_lin.data(), I.sb_lin.data(), I.Hpp.data(), I.HpN.data(), I.rhs_p.data(), I.HNN.data(), I.rhsN.data(), I.pre.data());
        if (id >= 0 && I.mid > 0 && swf_set_imu_gnss_mid_link(h_, id, I.mid, I.H12.data()) != SWF_OK) throw std::runtime_error(swf_last_error());
        if (id >= 0 && f->owned) hidden_[id] = std::move(f->owned);      // built from an IMUGNSSBase: the Problem keeps the contiguous hidden epochs alive
        delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(InitialBlackFactor* f, LossFunction* loss, double* scalar) {
        swf_factor_id id = swf_add_scalar_prior(h_, scalar, f->istd); delete f; delete loss; return ck(id);
    }
    ResidualBlockId AddResidualBlock(MarginalizationFactor* f, LossFunction* loss, const std::vector<double*>& blocks) {
        swf_factor_id id = swf_add_linear_prior(h_, blocks.data(), (int32_t)blocks.size(), f->J.data(), f->r0.data(), f->x0.data());
        delete f; delete loss; return ck(id);
    }

  private:
    static void chk(int rc, const char* what) { if (rc != SWF_OK) throw std::runtime_error(std::string(what) + ": " + swf_last_error()); }
    // factor id -> the handle the caller holds; handles live as long as the Problem (a removed block's handle dangles
    // logically, as in ceres, but never physically)
    ResidualBlockId ck(swf_factor_id id) {
        if (id < 0) throw std::runtime_error(std::string("AddResidualBlock: ") + swf_last_error());
        if (rb_.size() <= (size_t)id) rb_.resize((size_t)id + 1);
        rb_[(size_t)id].reset(new internal::ResidualBlock());
        rb_[(size_t)id]->id = id;
        return rb_[(size_t)id].get();
    }
    // the handle of a live factor id; created on demand for factors that were added through handle() and the C API
    // (is_use = true, like a freshly added block)
    ResidualBlockId handle_of(swf_factor_id id) const {
        if (id < 0) throw std::runtime_error("residual block id out of range");
        if (rb_.size() <= (size_t)id) rb_.resize((size_t)id + 1);
        if (!rb_[(size_t)id]) { rb_[(size_t)id].reset(new internal::ResidualBlock()); rb_[(size_t)id]->id = id; }
        return rb_[(size_t)id].get();
    }
    swf_problem* h_ = nullptr;
    mutable std::vector<std::unique_ptr<internal::ResidualBlock>> rb_;
    std::map<swf_factor_id, std::unique_ptr<IMUGNSSInfo>> hidden_;
};

struct Solver {
    struct Options {
        LinearSolverType linear_solver_type = DENSE_SCHUR;
        TrustRegionStrategyType trust_region_strategy_type = LEVENBERG_MARQUARDT;      // ceres' default; the window solves set DOGLEG
        int max_num_iterations = 50;         // ceres' default; R/swf/swf.cpp:25 sets MAX_NUM_ITERATIONS
        int num_threads = 1;                 // accepted, unused: the device decides its own parallelism
        bool jacobi_scaling = true;          // ceres' default, in force for the reference's default-options solves (R/swf/swf_gnss.cpp:205-214, 562-572:
                                             // Levenberg-Marquardt, where it is supported); every Options block that selects DOGLEG sets it to 0 (R/swf/swf.cpp:26-27)
        double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16;
        std::shared_ptr<ParameterBlockOrdering> linear_solver_ordering;      // null: automatic ordering (swf_set_ordering, n = 0)
        int swf_composite_root = SWF_ROOT_PIVOTED_CHOLESKY;                  // extension (not in ceres): swf_options::composite_root; SWF_ROOT_EIGEN = UpdateSchurComponent's own root
    };
    struct Summary {
        double initial_cost = 0, final_cost = 0, minimizer_time_in_seconds = 0;
        int num_successful_steps = 0, num_unsuccessful_steps = 0, termination = 0;
        std::string message;                 // swf_last_error() of a failed Solve, empty otherwise
        swf_summary raw;
        std::string BriefReport() const {
            char b[256];
            snprintf(b, sizeof b, "swf (MI355X) Report: Iterations: %d, Initial cost: %e, Final cost: %e, Termination: %d",
                     raw.num_iterations, initial_cost, final_cost, termination);
            return message.empty() ? std::string(b) : std::string(b) + " [" + message + "]";
        }
    };
};

// ceres::Solve(options, &problem, &summary) — R/swf/swf_image.cpp:219.  Ceres reports failures through the summary, never by
// throwing, and the estimator only tests summary.final_cost > 1e10: a failed solve therefore sets final_cost = 1e300, keeps the
// reason in summary.message, prints it to stderr and clears the exports (UpdateSchur must not read a previous solve's buffers).
inline void Solve(const Solver::Options& o, Problem* p, Solver::Summary* s) {
    swf_options opt; swf_options_default(&opt);
    opt.max_num_iterations = o.max_num_iterations;
    opt.initial_trust_region_radius = o.initial_trust_region_radius;
    opt.max_trust_region_radius = o.max_trust_region_radius;
    opt.step_mode = internal::is_optimize ? SWF_OPTIMIZE : SWF_ASSEMBLE_ELIMINATE_ONLY;
    opt.trust_region_strategy = o.trust_region_strategy_type == DOGLEG ? SWF_DOGLEG : SWF_LEVENBERG_MARQUARDT;
    std::memset(&s->raw, 0, sizeof(s->raw));
    s->message.clear();
    int rc = SWF_OK;
    opt.composite_root = o.swf_composite_root;
    opt.jacobi_scaling = o.jacobi_scaling ? 1 : 0;       // (with DOGLEG the engine refuses it: SWF_E_UNSUPPORTED, reported below like any failure)
    if (rc == SWF_OK) rc = p->SyncIsUse();
    if (rc == SWF_OK) {
        const ParameterBlockOrdering* ord = o.linear_solver_ordering.get();
        rc = swf_set_ordering(p->handle(), ord ? ord->keys_.data() : nullptr, ord ? ord->groups_.data() : nullptr, ord ? ord->NumElements() : 0);
    }
    if (rc == SWF_OK) rc = swf_set_export_tail(p->handle(), internal::parameter_head.data(), (int32_t)internal::parameter_head.size());
    if (rc == SWF_OK) {
        p->GatherHiddenEpochs();
        rc = swf_problem_solve(p->handle(), &opt, &s->raw);
        if (rc == SWF_OK) p->ScatterHiddenEpochs();
    }
    internal::reset_exports();
    if (rc == SWF_OK) {
        const double *lo = nullptr, *ro = nullptr, *lo2 = nullptr; int32_t hr = 0;
        if (swf_get_reduced(p->handle(), &lo, &ro, &lo2, &hr) == SWF_OK) {
            internal::Globals<>::lhs_out = const_cast<double*>(lo); internal::Globals<>::rhs_out = const_cast<double*>(ro);
            internal::Globals<>::lhs_out2 = const_cast<double*>(lo2); internal::Globals<>::hs_row = hr; internal::Globals<>::owner = p;
        }
    } else {
        if (s->message.empty()) s->message = swf_last_error();
        std::fprintf(stderr, "swf_ceres::Solve failed (%d): %s\n", rc, s->message.c_str());
    }
    s->initial_cost = s->raw.initial_cost; s->final_cost = rc == SWF_OK ? s->raw.final_cost : 1e300;   // callers test final_cost > 1e10
    s->minimizer_time_in_seconds = s->raw.minimizer_time_in_seconds;
    s->num_successful_steps = s->raw.num_successful_steps; s->num_unsuccessful_steps = s->raw.num_unsuccessful_steps;
    s->termination = s->raw.termination;
}

// The marginalisation consumer in one call: what SWFOptimization::UpdateSchur (R/swf/swf_gnss.cpp:25-61) followed by
// MarginalizationInfo::setmarginalizeinfo(addr, sizes, A, b, true) (R/factor/marginalization_factor.cpp:449-488)
// compute from the export of an is_optimize = false Solve.  Call it right after that Solve (GlobalMarge,
// R/swf/swf_image.cpp:404-418).  linearized_jacobians / linearized_residuals are n x n row-major / n, solver-owned,
// valid until the next Solve; A / b are the marginal system UpdateSchur leaves in SWFOptimization::A, b.
struct MarginalPrior {
    const double* linearized_jacobians = nullptr; const double* linearized_residuals = nullptr;
    const double* A = nullptr; const double* b = nullptr;
    int n = 0, rank = 0;
};
// eigen = true: the reference's eigen square root (tails up to 640 dimensions); false: the Cholesky square root (same quadratic, cheaper)
inline bool UpdateSchurAndSetMarginalizeInfo(Problem* p, MarginalPrior* out, bool eigen = true, double eps = 1e-8) {
    int32_t n = 0, rank = 0;
    int rc = swf_problem_marginalize(p->handle(), eps, eigen ? SWF_PRIOR_EIGEN : SWF_PRIOR_CHOLESKY, &out->linearized_jacobians,
                                     &out->linearized_residuals, &out->A, &out->b, &n, &rank);
    out->n = n; out->rank = rank;
    internal::parameter_head.clear();                       // as the reference's reader does (swf_gnss.cpp:58)
    return rc == SWF_OK && rank >= 0;
}

// MarginalizationInfo::ResetLinearizationPoint (R/factor/marginalization_factor.cpp:232-258; R/swf/swf_core.cpp:636-637): shift the prior
// (linearized_jacobians J, linearized_residuals r0, optionally the marginal system A, b) to the kept blocks' current values.  sizes = the
// kept blocks' global sizes (7 = pose) in kept order, parameters[i] = block i's current values, x0 = keep_block_data concatenated.
inline bool ResetLinearizationPoint(const std::vector<int32_t>& sizes, const std::vector<const double*>& parameters, int n,
                                    const double* J, const double* A, double* r0, double* b, double* x0) {
    return swf_prior_reset_linearization_point((int32_t)sizes.size(), sizes.data(), parameters.data(), n, J, A, r0, b, x0) == SWF_OK;
}

// SWFOptimization::UpdateSchurHessianOnly (R/swf/swf_gnss.cpp:65-94) after an optimising Solve: A = A3 A3^T over the
// parameter_head states, plus the covariance Qy = A^-1 LambdaSearch computes from it (R/swf/swf_lambda.cpp:94-99).
struct TailCovariance { const double* A = nullptr; const double* Qy = nullptr; int n = 0; };
inline bool UpdateSchurHessianOnly(Problem* p, TailCovariance* out) {
    int32_t n = 0;
    int rc = swf_problem_tail_covariance(p->handle(), &out->A, &out->Qy, &n);
    out->n = n;
    internal::parameter_head.clear();                       // swf_gnss.cpp:91
    return rc == SWF_OK && n > 0;
}

// RTKLIB's lambda(n, m, a, Q, F, s) (R/gnss/src/lambda.cpp:213-235) with its contract — column-major Q (n x n), F n x m, returns 0
// on success and non-zero otherwise — computed on the device (swf_lambda_batch, one problem; n <= 64, m <= 2).  The reference's
// LambdaSearch binds to it by qualifying its one call (R/swf/swf_lambda.cpp:201): swf_ceres::lambda(Qb.rows(), 2, b.data(), Qb.data(), F, s).
inline int lambda(int n, int m, const double* a, const double* Q, double* F, double* s) {
    if (n <= 0 || m <= 0 || !a || !Q || !F || !s) return -1;
    const int32_t nn = n;
    int32_t info = -1;
    std::vector<double> Fo((size_t)n * m);
    if (swf_lambda_batch(1, nn, &nn, a, Q, m, Fo.data(), s, &info, 0, nullptr) != SWF_OK) return -1;
    if (info != SWF_LAMBDA_OK) return info;
    std::memcpy(F, Fo.data(), Fo.size() * sizeof(double));   // F[(0 * m + j) * n + i] = column j of the n x m matrix
    return 0;
}

// Fix and hold: the second half of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:254-353) on the device.  The reference builds a
// MarginalizationInfo from last_marg_info, adds FixedIntegerFactor(ROUND(F), 1 / 0.03) per double difference and
// FixedIntegerFactor(0, 1 / 0.03) per reference ambiguity on the hidden tf offsets, marginalises the tf and makes the result the new
// last_marg_info.  Here: `prior` = the window prior's residual block, amb[i] / ref[i] = the two ambiguity blocks of double difference i,
// N21[i] = ROUND(F[i]).  scalars_at_zero = true (the default, as in the Python bindings) evaluates every one-dimensional kept block at 0,
// which is what the reference has between PhaseBiasSaveAndReset and PhaseBiasRestore: the call gives the reference's prior wherever it
// is made, inside that bracket or without it.  false reads those blocks at their current values (the same quadratic).  On success *out holds the new
// (linearized_jacobians, linearized_residuals) and x0 the new keep_block_data, solver-owned until the next call; the caller swaps the
// prior as the reference does (:344-354): RemoveResidualBlock(prior), AddResidualBlock(new MarginalizationFactor(J, r0, x0, n, ...)).
inline bool FixAndHoldPrior(Problem* p, ResidualBlockId prior, const std::vector<double*>& amb, const std::vector<double*>& ref,
                            const std::vector<double>& N21, MarginalPrior* out, const double** x0, bool scalars_at_zero = true,
                            double istd = 1.0 / 0.03, bool eigen = true, double eps = 1e-8) {
    if (!p || !prior || !out || amb.empty() || amb.size() != ref.size() || amb.size() != N21.size()) return false;
    int32_t n = 0, rank = 0;
    const int rc = swf_problem_fix_prior(p->handle(), prior->id, amb.data(), ref.data(), N21.data(), (int32_t)amb.size(), scalars_at_zero ? 1 : 0,
                                         istd, eps, eigen ? SWF_PRIOR_EIGEN : SWF_PRIOR_CHOLESKY, &out->linearized_jacobians,
                                         &out->linearized_residuals, x0, &n, &rank);
    out->A = nullptr; out->b = nullptr; out->n = n; out->rank = rank;
    return rc == SWF_OK && rank >= 0;
}

// SWFOptimization::OutliersRejection (R/swf/swf_image.cpp:263-308) together with the depth-sign test of Double2Vector
// (R/swf/swf.cpp:214-229), on the device, after Solve: `failed` receives the parameter blocks (landmarks / inverse depths) whose
// mean reprojection error times FOCAL_LENGTH / FEATUREWEIGHTINVERSE exceeds `threshold` (the reference: 2) or whose depth is
// negative — the blocks ImagePostprocess hands to FeatureManager::removeFailures.  False when the check could not run.
inline bool OutliersRejection(Problem& p, double threshold, std::vector<double*>& failed) {
    failed.clear();
    if (swf_problem_check_features(p.handle(), threshold) != SWF_OK) return false;
    int32_t n = 0;
    if (swf_problem_rejected_features(p.handle(), nullptr, 0, &n) != SWF_OK) return false;
    failed.resize((size_t)n);
    return n == 0 || swf_problem_rejected_features(p.handle(), failed.data(), n, &n) == SWF_OK;
}

// The pre-fit carrier-phase screen: the first half of SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:337-499) for one epoch on
// the device (swf_phase_screen_batch with one epoch; a caller that batches epochs builds the same records and makes one call).
//   rover      the new epoch (the reference's mea_t*): obs_count, obs_data[i].{SVH, sys, el, satellite_pos, RTK_L, SPP_L, SPP_P,
//              RTK_SLIP_COUNT, SPP_SLIP_COUNT, RTK_Npoint, SPP_Npoint}, Npoint->value, Npoint->SLIP_COUNT; read only
//   pose       para_pose[g2f[ir]] (its first three entries);  base_xyz: rover->base_xyz;  lams[sys][f];  gnss_dt = para_gnss_dt[0]
//   mode       SWF_SCR_GATE_RTK | SWF_SCR_GATE_SPP | SWF_SCR_RESET_ALL as the reference's conditions hold (:407, :417, :433)
// One record per (observation, frequency, kind) that the reference evaluates or decides on: an observation with SVH set has none
// (:347); a phase that is zero has one only if its Npoint exists (the reference still pushes that residual into the median, :354-362,
// and decides nothing for it, :406 / :416): it is handed over as masked, which is exactly that.  The SPP record's partner is the
// RTK record of the same observation and frequency (the reference's condition3, :454).  The reference also zeroes RTK_L / SPP_L /
// SPP_P0 of an observation below the mask in place (:351-353): that write, like every PBtype the flags ask for, stays with the caller.
// On success out->rtk / out->spp hold the flags (SWF_SCR_*) per observation and frequency, 0 where there is no record, the residuals
// and the medians; new_rtk(i, f) / new_spp(i, f) say whether the reference would create a new ambiguity there.
struct PhaseScreenResult {
    int nfreq = 0;
    std::vector<uint8_t> rtk, spp;               // [obs_count * nfreq] flags
    std::vector<double> rtk_r, spp_r;            // [obs_count * nfreq] residuals (0 where there is no record)
    double med[2][SWF_SCR_GROUPS];               // kind, group = sys * 2 + f
    int32_t cnt[2][SWF_SCR_GROUPS];
    std::vector<int32_t> reset;                  // the records with NEW_AMB, as (observation * nfreq + f) * 2 + kind, ascending by record
    bool new_rtk(int i, int f) const { return (rtk[(size_t)i * nfreq + f] & SWF_SCR_NEW_AMB) != 0; }
    bool new_spp(int i, int f) const { return (spp[(size_t)i * nfreq + f] & SWF_SCR_NEW_AMB) != 0; }
};
template <class Rover, class Lams>
inline bool PhaseScreen(const Rover& rover, const double* pose, const double* base_xyz, const Lams& lams, const double* gnss_dt,
                        int mode, double el_min, PhaseScreenResult* out, int nfreq = 2) {
    if (!pose || !base_xyz || !gnss_dt || !out || nfreq < 1 || nfreq > 2 || rover.obs_count < 0) return false;
    const int nobs = rover.obs_count;
    const double below = -1e300;                             // an elevation under every mask
    std::vector<double> dat;
    std::vector<int32_t> rec, where;                         // where[record] = (observation * nfreq + f) * 2 + kind
    for (int i = 0; i < nobs; i++) {
        const auto& d = rover.obs_data[i];
        if (d.SVH) continue;
        const int sys = d.sys;
        for (int f = 0; f < nfreq; f++) {
            if (sys < 0 || sys * 2 + f >= SWF_SCR_GROUPS) return false;
            const double lam = lams[sys][f];
            int32_t partner = -1;
            for (int kind = SWF_SCR_RTK; kind <= SWF_SCR_SPP; kind++) {
                const bool rtk = kind == SWF_SCR_RTK;
                const double L = rtk ? d.RTK_L[f] : d.SPP_L[f];
                const auto* np_ = rtk ? d.RTK_Npoint[f] : d.SPP_Npoint[f];
                if (L == 0 && !np_) continue;
                const int slip = rtk ? d.RTK_SLIP_COUNT[f] : d.SPP_SLIP_COUNT[f];
                const double row[SWF_SCR_DOUBLES] = { d.satellite_pos[0], d.satellite_pos[1], d.satellite_pos[2], L * lam, lam,
                                                      L == 0 ? below : d.el, rtk ? 0.0 : d.SPP_P[f], np_ ? np_->value : 0.0,
                                                      gnss_dt[rtk ? sys * 2 + f : 6 + sys * 2] };
                dat.insert(dat.end(), row, row + SWF_SCR_DOUBLES);
                const int32_t me = (int32_t)where.size();
                const int32_t q[4] = { kind, sys * 2 + f, (np_ ? SWF_SCR_HAS_AMB : 0) | (np_ && np_->SLIP_COUNT == slip ? SWF_SCR_CONTINUING : 0),
                                       rtk ? -1 : partner };
                rec.insert(rec.end(), q, q + 4);
                where.push_back((i * nfreq + f) * 2 + kind);
                if (rtk) partner = me;
            }
        }
    }
    const int32_t n = (int32_t)where.size(), first[2] = { 0, n }, m = mode;
    std::vector<double> r((size_t)n + 1);
    std::vector<uint8_t> fl((size_t)n + 1);
    std::vector<int32_t> rs((size_t)n + 1);
    int32_t nr = 0;
    dat.resize(dat.size() + SWF_SCR_DOUBLES); rec.resize(rec.size() + 4);          // (valid pointers for an epoch without records)
    if (swf_phase_screen_batch(1, first, pose, base_xyz, &m, el_min, dat.data(), rec.data(), r.data(), fl.data(), &out->med[0][0],
                               &out->cnt[0][0], rs.data(), &nr, 0, nullptr) != SWF_OK || nr < 0) return false;
    out->nfreq = nfreq;
    out->rtk.assign((size_t)nobs * nfreq, 0); out->spp.assign((size_t)nobs * nfreq, 0);
    out->rtk_r.assign((size_t)nobs * nfreq, 0.0); out->spp_r.assign((size_t)nobs * nfreq, 0.0);
    for (int32_t k = 0; k < n; k++) {
        const size_t at = (size_t)(where[k] >> 1);
        if (where[k] & 1) { out->spp[at] = fl[k]; out->spp_r[at] = r[k]; } else { out->rtk[at] = fl[k]; out->rtk_r[at] = r[k]; }
    }
    out->reset.clear();
    for (int32_t k = 0; k < nr; k++) out->reset.push_back(where[rs[k]]);
    return true;
}

// The double-difference pairs of the ambiguity search: FindReferenceSatellites and the loop of SWFOptimization::LambdaSearch that builds
// D3 (R/swf/swf_lambda.cpp:8-53, 118-188) for one window on the device (swf_dd_select_batch with one window; a caller that batches
// windows builds the same records and makes one call, or stays on the device with swf_batch_select_ambiguity_pairs).
//   rovers     the window's epochs, oldest first as the reference keeps them (rovers[0 .. rover_count-1], each a mea_t*): obs_count,
//              obs_data[i].{sys, RTK_Npoint}, Npoint->value; read only.  The epochs are handed over newest first (:126).
//   tail_of    tail_of(&Npoint->value) = the ambiguity's coordinate in the parameter_head tail, parameter_block_idx[...] - m of the
//              reference's MarginalizationInfo (:17, :151), or a negative number when the block is absent or not in the tail: such an
//              observation is left out, as it can produce neither a candidate nor a pair.  n = the tail dimension.
//   gate       last_fix ? 0.2 : 1.4 (:163)
// On success out->pairs holds the rows of D in the reference's order, (a, b) = +1 at a, -1 at b; out->go() is false where the
// reference returns early (:96, :178, :184).  The `use` marks, the fix counter and last_fix stay with the caller.
struct DoubleDifferenceSelection {
    std::vector<std::pair<int, int> > pairs;
    int last_count = 0, last_ref_count = 0, info = -1;       // info: SWF_DDSEL_*
    bool go() const { return info == SWF_DDSEL_OK; }
};
template <class Rovers, class TailOf>
inline bool SelectDoubleDifferences(const Rovers& rovers, int rover_count, TailOf tail_of, int n, double gate,
                                    DoubleDifferenceSelection* out, int nfreq = 2) {
    if (!out || rover_count < 0 || n < 0 || nfreq < 1 || nfreq > 2) return false;
    std::vector<int32_t> obs_first(1, 0), obs;
    std::vector<double> y((size_t)n + 1, 0.0);
    for (int ir = rover_count - 1; ir >= 0; ir--) {
        const auto& rover = *rovers[ir];
        for (int i = 0; i < rover.obs_count; i++) {
            const auto& d = rover.obs_data[i];
            for (int f = 0; f < nfreq; f++) {
                const auto* np_ = d.RTK_Npoint[f];
                if (!np_) continue;
                const int a = (int)tail_of(&np_->value);
                if (a < 0 || a >= n) continue;
                if (d.sys < 0 || d.sys * 2 + f >= 6) return false;
                obs.push_back(d.sys * 2 + f); obs.push_back(a);
                y[(size_t)a] = np_->value;
            }
        }
        obs_first.push_back((int32_t)(obs.size() / 2));
    }
    const int32_t epoch_first[2] = { 0, (int32_t)rover_count }, y_first[2] = { 0, (int32_t)n };
    int32_t pairs[SWF_LAMBDA_NMAX * 2], counts[4] = { 0, 0, 0, -1 };
    obs.resize(obs.size() + 2);                              // (a valid pointer for a window without observations)
    if (swf_dd_select_batch(1, epoch_first, obs_first.data(), obs.data(), y_first, y.data(), &gate, pairs, counts, nullptr, nullptr, nullptr,
                            0, nullptr) != SWF_OK) return false;
    out->pairs.clear();
    for (int i = 0; i < counts[0]; i++) out->pairs.push_back(std::make_pair((int)pairs[2 * i], (int)pairs[2 * i + 1]));
    out->last_count = counts[1]; out->last_ref_count = counts[2]; out->info = counts[3];
    return true;
}

// The single-epoch GNSS solve: the seed mini-solve of SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:534-575) and the first fix of
// GnssProcess (:203-215) for one epoch on the device (swf_gnss_epoch_solve_batch with one epoch; a caller that batches epochs builds
// the same records and makes one call).  The rows and their weights are those of AddGnssResidual (R/swf/swf_core.cpp:105-203):
//   USE_RTK    RTKCarrierPhaseFactor per frequency with an RTK_Npoint, el >= el_min (:106-120); clock sys * 2 + f
//   USE_RTD    RTKPseudorangeFactor per frequency with RTK_P != 0, SVH == 0, RTK_Pstd <= 2, el >= el_min (:122-137); clock sys * 2 + f
//   then per observation with SVH == 0 and el >= el_min (:140-189), clock 6 + sys * 2:
//              SppPseudorangeFactor if SPP_P[0] != 0, SPP_Pstd[0] < 2 and no row above was added (have_base); x10 weight when `startup`
//              SppCarrierPhaseFactor if USE_SPP_PHASE, SPP_L[0] != 0 and an SPP_Npoint[0]
//              SppCarrierPhaseFactor on SPP_P0[0] if USE_SPP_CORRECTION, SPP_P0[0] != 0 and an SPP_Npoint_PCottections[0]
//   USE_DOPPLER SppDopplerFactor if SPP_D[0] != 0, SVH == 0, SPP_Dstd[0] <= 2, el >= el_min (:190-203); clock 12
// The RTK weights are 1 / sqrt(varerr2) with the reference's float sine (R/factor/gnss_factor.cpp:98-103).
//   rover      the epoch (the reference's mea_t*): obs_count, base_xyz, br_time_diff, obs_data[i].{SVH, sys, el, satellite_pos,
//              satellite_vel, RTK_L, RTK_Lstd, RTK_P, RTK_Pstd, SPP_P, SPP_Pstd, SPP_L, SPP_Lstd, SPP_P0, SPP_D, SPP_Dstd, ion_var, trop_var,
//              sat_var, RTK_Npoint, SPP_Npoint, SPP_Npoint_PCottections}, Npoint->{value, continue_count}
//   pose, speed_bias, gnss_dt   para_pose[g2f[ir]], para_speed_bias[g2f[ir]], para_gnss_dt[0] (13 scalars)
// Presets: GnssEpochSeed holds pose and speed-bias constant, frees the ambiguities with continue_count <= 10 and runs 2 iterations;
// GnssEpochFirstFix frees position, velocity, clocks and every ambiguity (the reference sets nothing constant there) and runs 20.
// The solved values go where ceres::Solve would have left them: pose[0..2], speed_bias[0..2], gnss_dt and the value of every freed
// ambiguity; a rank-deficient epoch writes nothing back.  The dummy anchor InitialBlackFactor shares no row with the rest
// and is not part of the operator.
struct GnssEpochOptions {
    bool use_rtk = true, use_rtd = true, use_spp_phase = true, use_spp_correction = false, use_doppler = true;
    bool startup = false;                        // rover_count_accumulate - rover_count + ir < 100 (:154): x10 on the rover-only code weight
    double el_min = 25.0 * 3.14159265358979323846 / 180.0;      // AZELMIN
    int nfreq = 2;                               // NFREQ
    double step_tol = 1e-4, eps_rank = 1e-8;
};
enum GnssEpochPreset { GnssEpochSeed = 0, GnssEpochFirstFix = 1 };
struct GnssEpochRow { int obs, f, kind; bool correction; };           // where a record came from; correction: the SPP_P0 row
struct GnssEpochResult {
    std::vector<double> dat;                     // [n][SWF_GES_DOUBLES] as handed over
    std::vector<int32_t> rec;                    // [n][4]
    std::vector<GnssEpochRow> rows;              // [n]
    std::vector<double> N, r;                    // [n]
    double pos[3], vel[3], clock[SWF_GES_CLOCKS], cost, info[36];
    int32_t iters, status, clk_rows[SWF_GES_CLOCKS];
    bool have_base;
};
inline double GnssEpochVarerr2(double el, double dt, double mea_var) {
    const double b = 299792458.0 * 5e-12 * dt, s = (double)sinf((float)el);
    return mea_var / s / s + b * b;
}
template <class Rover, class Lams>
inline bool GnssEpochSolve(Rover& rover, double* pose, double* speed_bias, double* gnss_dt, const Lams& lams, const GnssEpochOptions& opt,
                           GnssEpochPreset preset, GnssEpochResult* out) {
    if (!pose || !speed_bias || !gnss_dt || !out || opt.nfreq < 1 || opt.nfreq > 2 || rover.obs_count < 0) return false;
    const bool seed = preset == GnssEpochSeed;
    out->dat.clear(); out->rec.clear(); out->rows.clear();
    std::vector<double*> amb;                    // where a freed ambiguity lives
    auto put = [&](int i, int f, int kind, bool corr, const double* sat, const double* sv, double obs, double w, double lam, int slot, double* N,
                   int continue_count) {
        const bool fr = N && (!seed || continue_count <= 10);
        const double row[SWF_GES_DOUBLES] = { sat[0], sat[1], sat[2], sv ? sv[0] : 0.0, sv ? sv[1] : 0.0, sv ? sv[2] : 0.0, obs, w, lam, N ? *N : 0.0 };
        out->dat.insert(out->dat.end(), row, row + SWF_GES_DOUBLES);
        const int32_t q[4] = { kind, slot, fr ? SWF_GES_AMB_FREE : 0, 0 };
        out->rec.insert(out->rec.end(), q, q + 4);
        out->rows.push_back(GnssEpochRow{ i, f, kind, corr });
        amb.push_back(fr ? N : nullptr);
    };
    const int nobs = rover.obs_count;
    bool have_base = false;
    if (opt.use_rtk)
        for (int i = 0; i < nobs; i++) {
            auto& d = rover.obs_data[i];
            for (int f = 0; f < opt.nfreq; f++) {
                if (!d.RTK_Npoint[f] || d.el < opt.el_min) continue;
                if (d.sys * 2 + f >= 6) return false;
                have_base = true;
                const double lam = lams[d.sys][f], sd = d.RTK_Lstd[f] * lam;
                put(i, f, SWF_GES_RTK_PHASE, false, d.satellite_pos, nullptr, d.RTK_L[f] * lam, 1.0 / std::sqrt(GnssEpochVarerr2(d.el, rover.br_time_diff, sd * sd)),
                    lam, d.sys * 2 + f, &d.RTK_Npoint[f]->value, (int)d.RTK_Npoint[f]->continue_count);
            }
        }
    if (opt.use_rtd)
        for (int i = 0; i < nobs; i++) {
            auto& d = rover.obs_data[i];
            for (int f = 0; f < opt.nfreq; f++) {
                if (d.RTK_P[f] == 0.0 || d.SVH != 0 || d.RTK_Pstd[f] > 2 || d.el < opt.el_min) continue;
                if (d.sys * 2 + f >= 6) return false;
                have_base = true;
                put(i, f, SWF_GES_RTK_CODE, false, d.satellite_pos, nullptr, d.RTK_P[f],
                    1.0 / std::sqrt(GnssEpochVarerr2(d.el, rover.br_time_diff, d.RTK_Pstd[f] * d.RTK_Pstd[f])), 1.0, d.sys * 2 + f, nullptr, 0);
            }
        }
    for (int i = 0; i < nobs; i++) {
        auto& d = rover.obs_data[i];
        if (d.SVH != 0 || d.el < opt.el_min) continue;
        if (d.sys > 2) return false;
        const double s = std::sin(d.el), atm = d.ion_var * 0.125 * 0.125 + d.trop_var * 0.7 * 0.7 + d.sat_var * 0.35 * 0.35, lam = lams[d.sys][0];
        if (d.SPP_P[0] != 0.0 && d.SPP_Pstd[0] < 2 && !have_base) {
            double istd = s * s / std::sqrt(d.SPP_Pstd[0] * d.SPP_Pstd[0] + (atm + 1));
            if (opt.startup) istd *= 10;
            put(i, 0, SWF_GES_SPP_CODE, false, d.satellite_pos, nullptr, d.SPP_P[0], istd, 1.0, 6 + d.sys * 2, nullptr, 0);
        }
        if (opt.use_spp_phase && d.SPP_L[0] != 0.0 && d.SPP_Npoint[0]) {
            const double sd = d.SPP_Lstd[0] * lam;
            put(i, 0, SWF_GES_SPP_PHASE, false, d.satellite_pos, nullptr, d.SPP_L[0] * lam, s * s / std::sqrt(sd * sd + atm), lam, 6 + d.sys * 2,
                &d.SPP_Npoint[0]->value, (int)d.SPP_Npoint[0]->continue_count);
        }
        if (opt.use_spp_correction && d.SPP_P0[0] != 0.0 && d.SPP_Npoint_PCottections[0])
            put(i, 0, SWF_GES_SPP_PHASE, true, d.satellite_pos, nullptr, d.SPP_P0[0], s * s / std::sqrt(d.SPP_Pstd[0] * d.SPP_Pstd[0] + atm), lam, 6 + d.sys * 2,
                &d.SPP_Npoint_PCottections[0]->value, (int)d.SPP_Npoint_PCottections[0]->continue_count);
    }
    if (opt.use_doppler)
        for (int i = 0; i < nobs; i++) {
            auto& d = rover.obs_data[i];
            if (d.SPP_D[0] == 0.0 || d.SVH != 0 || d.SPP_Dstd[0] > 2 || d.el < opt.el_min) continue;
            if (d.sys > 2) return false;
            const double s = std::sin(d.el), lam = lams[d.sys][0];
            put(i, 0, SWF_GES_DOPPLER, false, d.satellite_pos, d.satellite_vel, d.SPP_D[0] * lam, s * s / (d.SPP_Dstd[0] * lam), 1.0, 12, nullptr, 0);
        }
    out->have_base = have_base;
    const int32_t n = (int32_t)out->rows.size(), first[2] = { 0, n }, mode = seed ? 0 : (SWF_GES_FREE_POS | SWF_GES_FREE_VEL), cc = 0;
    out->N.assign((size_t)n + 1, 0.0); out->r.assign((size_t)n + 1, 0.0);
    std::vector<double> dat = out->dat;
    std::vector<int32_t> rec = out->rec;
    dat.resize(dat.size() + SWF_GES_DOUBLES); rec.resize(rec.size() + 4);          // (valid pointers for an epoch without records)
    if (swf_gnss_epoch_solve_batch(1, first, pose, speed_bias, rover.base_xyz, gnss_dt, &mode, &cc, dat.data(), rec.data(), seed ? 2 : 20,
                                   opt.step_tol, opt.eps_rank, out->pos, out->vel, out->clock, out->N.data(), out->r.data(), &out->cost,
                                   &out->iters, &out->status, out->clk_rows, out->info, 0, nullptr) != SWF_OK || out->status < 0) return false;
    out->N.resize((size_t)n); out->r.resize((size_t)n);
    if (out->status != SWF_GES_RANK_DEFICIENT) {
        for (int k = 0; k < 3; k++) { pose[k] = out->pos[k]; speed_bias[k] = out->vel[k]; }
        for (int k = 0; k < SWF_GES_CLOCKS; k++) gnss_dt[k] = out->clock[k];
        for (int32_t k = 0; k < n; k++) if (amb[(size_t)k]) *amb[(size_t)k] = out->N[(size_t)k];
    }
    return true;
}

// The IMU front of a frame: SWFOptimization::ImuIntegrate with its IMUProcess calls (R/swf/swf_imu.cpp:117-213) for one frame on the
// device (swf_imu_frame_batch with one frame; a caller with many streams builds the same arrays and makes one call).
//   accVector, gyrVector   the vector<pair<double, Vector3d>> pairs GetImuInterval returned (any vector type with operator()(i))
//   prev_time, cur_time    the previous frame's time (the reference's static current_time on entry) and this frame's
//   acc_0, gyr_0           the estimator's members on entry; on success they hold the last effective sample, as IMUProcess leaves them
//   P, R, V                Ps[j], Rs[j], Vs[j] of the new frame j (operator()(i), operator()(i, j)); replaced by the propagated values
//   Ba, Bg                 Bas[j], Bgs[j]
//   gyrj_prev              pre_integrations[j - 1]->gyrj;  lever_velocity = (j > 5)
//   Pbg, g_w               the antenna lever arm and Rwgw * G;  noise = ACC_N, GYR_N, ACC_W, GYR_W
// On success out->pre is the record IMUFactor(const double*) takes, out->header the frame's headers[] entry (cur_time when the last
// sample was blended onto it, else the last stamp used) and out->cut the effective samples (SlideWindowFrame's push of interval k+1
// onto interval k is swf_preintegrate_runs_batch over two such blocks).  Returns false, with out->info = SWF_IMUF_*, where the
// reference asserts; P, R, V, acc_0, gyr_0 are then untouched.  Frame index 0 is neither pushed nor propagated by the reference: do
// not call this for it.  The IMU queues, GetImuInterval's popping, headers[] and adding the IMUFactor block stay with the caller.
struct ImuFrameResult {
    std::vector<double> pre;                     // SWF_PRE_DOUBLES
    std::vector<double> cut;                     // [rows][7]: the seed with dt 0, then (dt, acc, gyr) per IMUProcess call
    int rows = 0, info = -1;
    double header = 0;
};
template <class Pairs, class V3, class M3>
inline bool ImuIntegrate(const Pairs& accVector, const Pairs& gyrVector, double prev_time, double cur_time, V3& acc_0, V3& gyr_0,
                         V3& P, M3& R, V3& V, const V3& Ba, const V3& Bg, const V3& gyrj_prev, bool lever_velocity, const V3& Pbg,
                         const V3& g_w, const double noise[4], ImuFrameResult* out) {
    if (!out || !noise || accVector.size() != gyrVector.size()) return false;
    const int32_t n = (int32_t)accVector.size(), first[2] = { 0, n }, flags = lever_velocity ? 1 : 0;
    std::vector<double> raw((size_t)(n + 1) * 7, 0.0);
    for (int32_t i = 0; i < n; i++) {
        raw[(size_t)i * 7] = accVector[(size_t)i].first;
        for (int k = 0; k < 3; k++) { raw[(size_t)i * 7 + 1 + k] = accVector[(size_t)i].second(k); raw[(size_t)i * 7 + 4 + k] = gyrVector[(size_t)i].second(k); }
    }
    const double t01[2] = { prev_time, cur_time };
    double seed[6], state[21], gp[3], pbg[3], gw[3], pred[15];
    for (int k = 0; k < 3; k++) {
        seed[k] = acc_0(k); seed[3 + k] = gyr_0(k); state[k] = P(k); state[12 + k] = V(k); state[15 + k] = Ba(k); state[18 + k] = Bg(k);
        gp[k] = gyrj_prev(k); pbg[k] = Pbg(k); gw[k] = g_w(k);
        for (int j = 0; j < 3; j++) state[3 + 3 * k + j] = R(k, j);
    }
    out->pre.assign(SWF_PRE_DOUBLES, 0.0); out->cut.assign((size_t)(n + 1) * 7, 0.0); out->rows = 0; out->info = -1;
    int32_t info = -1;
    if (swf_imu_frame_batch(raw.data(), first, 1, t01, seed, state, gp, &flags, pbg, gw, noise, out->cut.data(), out->pre.data(), pred,
                            &info, 0, nullptr) != SWF_OK) return false;
    out->info = info;
    if (info != SWF_IMUF_OK) return false;
    int32_t used = 0;                                        // raw samples used: up to and including the first beyond cur_time
    while (used < n && raw[(size_t)used * 7] <= cur_time) used++;
    const bool blended = used < n;
    used += blended ? 1 : 0;
    out->rows = used + 1; out->cut.resize((size_t)out->rows * 7);
    out->header = blended ? cur_time : raw[(size_t)(used - 1) * 7];
    for (int k = 0; k < 3; k++) {
        P(k) = pred[k]; V(k) = pred[12 + k];
        acc_0(k) = out->cut[(size_t)used * 7 + 1 + k]; gyr_0(k) = out->cut[(size_t)used * 7 + 4 + k];
        for (int j = 0; j < 3; j++) R(k, j) = pred[3 + 3 * k + j];
    }
    return true;
}

// The pose of a new image frame from the landmarks it observes: FeatureManager::initFramePoseByPnP with solvePoseByPnP
// (R/feature/feature_manager.cpp:164-243) for one frame on the device (swf_pnp_frame_batch with one frame and flag bit 0: the points
// pass through float, as the reference's cv::Point3f / Point2f do; a caller with many streams builds the same arrays and makes one call).
//   frameCnt, Ps, Rs, tic, ric, Pbg   the reference's arguments (operator()(i), operator()(i, j)); Ps / Rs[frameCnt - 1] is the guess
//   pts3D, pts2D                      what the loop of :210-228 collects (members x, y, z / x, y); that loop stays with the caller
//   threshold                         8.0 / FOCAL_LENGTH in the reference; iterations 100, confidence 0.99
// Returns true and writes Ps / Rs[frameCnt] on SWF_PNP_OK / SWF_PNP_UNREFINED; otherwise (frameCnt <= 0 included) both are untouched,
// as in the reference.  out, when given, receives the codes and the inlier mask.
struct PnpFrameResult {
    int info = -1, n_inliers = 0, best = -1, n_iters = 0;
    std::vector<uint8_t> inlier;
};
template <class V3, class M3, class Pts3, class Pts2>
inline bool InitFramePoseByPnP(int frameCnt, V3 Ps[], M3 Rs[], const V3 tic[], const M3 ric[], const V3& Pbg, const Pts3& pts3D,
                               const Pts2& pts2D, double threshold, PnpFrameResult* out = nullptr, uint64_t seed = 0,
                               int32_t iterations = 100, double confidence = 0.99) {
    if (frameCnt <= 0 || pts3D.size() != pts2D.size()) return false;
    const int32_t n = (int32_t)pts3D.size(), first[2] = { 0, n };
    std::vector<double> pw((size_t)(n + 1) * 3, 0.0), uv((size_t)(n + 1) * 2, 0.0);
    for (int32_t i = 0; i < n; i++) {
        pw[(size_t)i * 3] = pts3D[(size_t)i].x; pw[(size_t)i * 3 + 1] = pts3D[(size_t)i].y; pw[(size_t)i * 3 + 2] = pts3D[(size_t)i].z;
        uv[(size_t)i * 2] = pts2D[(size_t)i].x; uv[(size_t)i * 2 + 1] = pts2D[(size_t)i].y;
    }
    double pp[3], rp[9], t[3], r[9], pbg[3], po[3], ro[9];
    for (int k = 0; k < 3; k++) {
        pp[k] = Ps[frameCnt - 1](k); t[k] = tic[0](k); pbg[k] = Pbg(k);
        for (int j = 0; j < 3; j++) { rp[3 * k + j] = Rs[frameCnt - 1](k, j); r[3 * k + j] = ric[0](k, j); }
    }
    std::vector<uint8_t> inl((size_t)n + 1, 0);
    int32_t ni = 0, best = -1, nit = 0, info = -1;
    if (swf_pnp_frame_batch(1, first, pw.data(), uv.data(), pp, rp, t, r, pbg, iterations, threshold, confidence, seed, 1, po, ro, &ni,
                            inl.data(), &best, &nit, &info, nullptr, nullptr, nullptr, 0, nullptr) != SWF_OK) return false;
    const bool ok = info == SWF_PNP_OK || info == SWF_PNP_UNREFINED;
    if (out) {
        out->info = info; out->n_inliers = ok ? ni : 0; out->best = ok ? best : -1; out->n_iters = ok ? nit : 0;
        inl.resize(ok ? (size_t)n : 0); out->inlier = inl;
    }
    if (!ok) return false;
    for (int k = 0; k < 3; k++) {
        Ps[frameCnt](k) = po[k];
        for (int j = 0; j < 3; j++) Rs[frameCnt](k, j) = ro[3 * k + j];
    }
    return true;
}

// The geometric gate of the feature tracker: FeatureTracker::rejectWithF (R/feature/feature_tracker.cpp:265-294) with undistortedPts
// (:334-343) and ptsVelocity (:345-376) for one frame pair on the device (swf_track_reject_batch with one pair and flag bit 0: the
// points pass through float wherever the reference holds a cv::Point2f; a caller with many streams builds the same arrays and makes one
// call).
//   cur_pts, prev_pts          the tracker's vectors of the same tracks (members x, y)
//   cam                        fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 of the PINHOLE_FULL camera; col, row, focal: the image size and FOCAL_LENGTH
//   f_threshold, dt            F_THRESHOLD; cur_time - prev_time
// Returns true on SWF_TRK_OK: out->status is then what cv::findFundamentalMat's status is to the reference, for ReduceVector below.
// With fewer than 8 tracks (SWF_TRK_TOO_FEW, the reference skips the gate) or without a model it returns false and out->status is
// empty; un_cur, un_prev and velocity are filled in all three cases.  setMask, goodFeaturesToTrack, the id maps and track_cnt stay with
// the caller; the KLT tracking in front of it is TrackImageKLT below.
struct RejectWithFResult {
    int info = -1, n_inliers = 0, best = -1, n_iters = 0;
    std::vector<uint8_t> status;
    std::vector<double> un_cur, un_prev, velocity;      // [n][2]
};
template <class Pts>
inline bool RejectWithF(const Pts& cur_pts, const Pts& prev_pts, const double cam[12], int col, int row, double focal, double f_threshold,
                        double dt, RejectWithFResult* out, uint64_t seed = 0, int32_t iterations = 1000, double confidence = 0.99) {
    if (!out || cur_pts.size() != prev_pts.size()) return false;
    const int32_t n = (int32_t)cur_pts.size(), first[2] = { 0, n };
    std::vector<double> c((size_t)(n + 1) * 2, 0.0), p((size_t)(n + 1) * 2, 0.0);
    for (int32_t i = 0; i < n; i++) {
        c[(size_t)i * 2] = cur_pts[(size_t)i].x; c[(size_t)i * 2 + 1] = cur_pts[(size_t)i].y;
        p[(size_t)i * 2] = prev_pts[(size_t)i].x; p[(size_t)i * 2 + 1] = prev_pts[(size_t)i].y;
    }
    std::vector<uint8_t> st((size_t)n + 1, 0);
    out->un_cur.assign((size_t)(n + 1) * 2, 0.0); out->un_prev.assign((size_t)(n + 1) * 2, 0.0); out->velocity.assign((size_t)(n + 1) * 2, 0.0);
    int32_t ni = 0, best = -1, nit = 0, info = -1;
    const int rc = swf_track_reject_batch(1, first, c.data(), p.data(), cam, col, row, focal, &dt, iterations, f_threshold, confidence, seed, 1,
                                          st.data(), nullptr, &ni, &best, &nit, &info, nullptr, out->un_cur.data(), out->un_prev.data(),
                                          out->velocity.data(), nullptr, nullptr, nullptr, 0, nullptr);
    const bool ok = rc == SWF_OK && info == SWF_TRK_OK;
    const bool lifted = rc == SWF_OK && info != SWF_TRK_BAD_INPUT;
    out->info = rc == SWF_OK ? info : -1; out->n_inliers = ok ? ni : 0; out->best = ok ? best : -1; out->n_iters = ok ? nit : 0;
    st.resize(ok ? (size_t)n : 0); out->status = st;
    out->un_cur.resize(lifted ? (size_t)n * 2 : 0); out->un_prev.resize(lifted ? (size_t)n * 2 : 0); out->velocity.resize(lifted ? (size_t)n * 2 : 0);
    return ok;
}

// The sparse optical flow of the feature tracker: the tracking part of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:98-141)
// for one image pair on the device (swf_klt_track_batch with one pair and flag bit 0; a caller with many streams builds the same arrays
// and makes one call).
//   prev_img, cur_img          8-bit grey, rows x cols, dense rows (cv::Mat::data of a continuous CV_8UC1 image)
//   prev_pts                   the tracker's vector of the previous positions (members x, y)
//   predict_pts                the reference's hasPrediction branch (null: none): the forward pass starts from these positions with 1
//                              pyramid level; when fewer than 10 points succeed it is run again without them with 3 levels, as there
//   flow_back                  FLOW_BACK: the reverse pass from the previous positions with 1 level and the 0.5 px gate
// Returns true when the call succeeded and the pair is SWF_KLT_OK: cur_pts holds the tracked positions, out->status is what the
// reference's status is after the reverse check and inBorder, for ReduceVector below; out->why says which test dropped a point.
// A non-finite position (SWF_KLT_BAD_INPUT) returns false with an empty status.  The n++ of track_cnt, setPrediction itself and the
// stereo branch stay with the caller; setMask, goodFeaturesToTrack and addPoints are DetectFeatures below.
struct TrackImageKLTResult {
    int info = -1, n_keep = 0, levels = 0;              // levels: max_level of the forward pass that gave the result (1 or 3)
    std::vector<uint8_t> status;
    std::vector<int32_t> why;
    std::vector<double> cur_px, back_px;                // [n][2]
};
template <class Pts>
inline bool TrackImageKLT(const uint8_t* prev_img, const uint8_t* cur_img, int rows, int cols, const Pts& prev_pts, Pts* cur_pts,
                          TrackImageKLTResult* out, const Pts* predict_pts = nullptr, bool flow_back = true) {
    if (!out || !cur_pts || (predict_pts && predict_pts->size() != prev_pts.size())) return false;
    const int32_t n = (int32_t)prev_pts.size(), first[2] = { 0, n };
    std::vector<double> p((size_t)(n + 1) * 2, 0.0), g((size_t)(n + 1) * 2, 0.0);
    for (int32_t i = 0; i < n; i++) {
        p[(size_t)i * 2] = prev_pts[(size_t)i].x; p[(size_t)i * 2 + 1] = prev_pts[(size_t)i].y;
        if (predict_pts) { g[(size_t)i * 2] = (*predict_pts)[(size_t)i].x; g[(size_t)i * 2 + 1] = (*predict_pts)[(size_t)i].y; }
    }
    std::vector<uint8_t> st((size_t)n + 1, 0);
    std::vector<int32_t> why((size_t)n + 1, 0);
    out->cur_px.assign((size_t)(n + 1) * 2, 0.0); out->back_px.assign((size_t)(n + 1) * 2, 0.0);
    int32_t info = -1, nk = 0;
    int rc = SWF_OK, levels = 3;
    bool done = false;
    if (predict_pts) {
        levels = 1;
        rc = swf_klt_track_batch(1, rows, cols, prev_img, cur_img, first, p.data(), g.data(), 21, 1, 1, 30, 0.01, 1e-4, 0.5, 1 | 2 | (flow_back ? 4 : 0),
                                 out->cur_px.data(), out->back_px.data(), st.data(), why.data(), nullptr, &nk, &info, nullptr, nullptr, nullptr, 0, nullptr);
        int succ = 0;
        for (int32_t i = 0; i < n; i++) succ += why[(size_t)i] != SWF_KLT_FWD_LOST && why[(size_t)i] != SWF_KLT_FWD_FLAT;
        done = rc != SWF_OK || info != SWF_KLT_OK || succ >= 10;
    }
    if (!done) {
        levels = 3;
        rc = swf_klt_track_batch(1, rows, cols, prev_img, cur_img, first, p.data(), nullptr, 21, 3, 1, 30, 0.01, 1e-4, 0.5, 1 | (flow_back ? 4 : 0),
                                 out->cur_px.data(), out->back_px.data(), st.data(), why.data(), nullptr, &nk, &info, nullptr, nullptr, nullptr, 0, nullptr);
    }
    const bool ok = rc == SWF_OK && info == SWF_KLT_OK;
    out->info = rc == SWF_OK ? info : -1; out->n_keep = ok ? nk : 0; out->levels = levels;
    st.resize(ok ? (size_t)n : 0); why.resize(ok ? (size_t)n : 0);
    out->status = st; out->why = why;
    out->cur_px.resize(ok ? (size_t)n * 2 : 0); out->back_px.resize(ok && flow_back ? (size_t)n * 2 : 0);
    if (ok) {
        cur_pts->resize((size_t)n);
        for (int32_t i = 0; i < n; i++) { (*cur_pts)[(size_t)i].x = (float)out->cur_px[(size_t)i * 2]; (*cur_pts)[(size_t)i].y = (float)out->cur_px[(size_t)i * 2 + 1]; }
    }
    return ok;
}

// Where the points to track come from: setMask(), cv::goodFeaturesToTrack(cur_img, n_pts, MAX_CNT - cur_pts.size(), 0.01, MIN_DIST, mask)
// and addPoints() of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:148-165) for one tracker state on the device
// (swf_gftt_detect_batch with one frame and flag bit 0; a caller with many streams builds the same arrays and makes one call).
//   img                        8-bit grey, rows x cols, dense rows;  mask: the caller's own mask (0 = blocked) or null
//   cur_pts, ids, track_cnt    the tracker's vectors after rejectWithF and the n++ of track_cnt; on success they are what setMask and
//                              addPoints leave: the kept points by track_cnt descending (ties by index), then the new corners with
//                              ids *n_id, *n_id + 1, .. and track_cnt 1
//   max_cnt, min_dist          MAX_CNT, MIN_DIST
// Returns true when the call succeeded and the frame is SWF_GFTT_OK.  More candidates than cand_cap (SWF_GFTT_TOO_MANY) makes one more
// call with the count the first one reported.  On failure (a non-finite position, a negative track_cnt, no device) the state is
// left as it was.  The declared differences from OpenCV are those of swf_gftt_detect_batch.
struct DetectFeaturesResult {
    int info = -1, n_old = 0, n_new = 0, n_cand = 0;
    double max_eig = 0.0;
    std::vector<int32_t> why;                           // per point of the state as it came in
};
template <class Pts>
inline bool DetectFeatures(const uint8_t* img, int rows, int cols, Pts* cur_pts, std::vector<int>* ids, std::vector<int>* track_cnt, int* n_id,
                           DetectFeaturesResult* out, int max_cnt = 350, int min_dist = 30, const uint8_t* mask = nullptr, int cand_cap = 1 << 15) {
    if (!out || !cur_pts || !ids || !track_cnt || !n_id || ids->size() != cur_pts->size() || track_cnt->size() != cur_pts->size()) return false;
    const int32_t n = (int32_t)cur_pts->size(), first[2] = { 0, n };
    std::vector<double> p((size_t)(n + 1) * 2, 0.0), fresh((size_t)(max_cnt > 0 ? max_cnt : 1) * 2, 0.0);
    std::vector<int32_t> tc((size_t)n + 1, 0), order((size_t)n + 1, -1), why((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++) {
        p[(size_t)i * 2] = (*cur_pts)[(size_t)i].x; p[(size_t)i * 2 + 1] = (*cur_pts)[(size_t)i].y;
        tc[(size_t)i] = (*track_cnt)[(size_t)i];
    }
    int32_t info = -1, n_old = 0, n_new = 0, n_cand = 0;
    double max_eig = 0.0;
    int rc = SWF_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        rc = swf_gftt_detect_batch(1, rows, cols, img, mask, first, p.data(), tc.data(), max_cnt, min_dist, 0.01, nullptr, cand_cap, 1, order.data(), why.data(),
                                   &n_old, fresh.data(), &n_new, &n_cand, &max_eig, nullptr, nullptr, nullptr, &info, nullptr, 0, nullptr);
        if (rc != SWF_OK || info != SWF_GFTT_TOO_MANY) break;
        cand_cap = n_cand;
    }
    const bool ok = rc == SWF_OK && info == SWF_GFTT_OK;
    out->info = rc == SWF_OK ? info : -1;
    out->n_old = ok ? n_old : 0; out->n_new = ok ? n_new : 0; out->n_cand = rc == SWF_OK && info != SWF_GFTT_BAD_INPUT ? n_cand : 0; out->max_eig = ok ? max_eig : 0.0;
    why.resize(ok ? (size_t)n : 0);
    out->why = why;
    if (!ok) return false;
    Pts pts;
    std::vector<int> new_ids, new_cnt;
    for (int32_t j = 0; j < n_old; j++) {                 // setMask: the kept points in walk order
        const size_t i = (size_t)order[(size_t)j];
        pts.push_back((*cur_pts)[i]); new_ids.push_back((*ids)[i]); new_cnt.push_back((*track_cnt)[i]);
    }
    for (int32_t j = 0; j < n_new; j++) {                 // addPoints
        typename Pts::value_type q = typename Pts::value_type();
        q.x = (float)fresh[(size_t)j * 2]; q.y = (float)fresh[(size_t)j * 2 + 1];
        pts.push_back(q); new_ids.push_back((*n_id)++); new_cnt.push_back(1);
    }
    *cur_pts = pts; *ids = new_ids; *track_cnt = new_cnt;
    return true;
}

// what the reference's reduceVector (:21-35) does with a status: the kept elements move to the front, in order
template <class T>
inline void ReduceVector(std::vector<T>& v, const std::vector<uint8_t>& status) {
    const size_t n = v.size() < status.size() ? v.size() : status.size();
    size_t kept = 0;
    for (size_t i = 0; i < n; i++) {
        if (!status[i]) continue;
        if (kept != i) v[kept] = v[i];
        kept++;
    }
    v.resize(kept);
}

// The whole tracker: FeatureTracker::trackImage (R/feature/feature_tracker.cpp:88-263) and removeOutliers for one camera, its state
// (prev_img, prev_pts, ids, track_cnt, n_id, the previous normalised points, prev_time) resident on the device (swf_tracker_* with one
// stream; a caller with many cameras or sequences creates one swf_tracker with as many streams and makes one call per frame).  The
// three stages above run chained in device memory; nothing but the image goes up and the feature frame comes down.
//   FeatureTracker(rows, cols, cam, options)   cam = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6; options: null for the reference's values
//   trackImage(t, img)                         the reference's featureFrame: feature id -> [(camera id 0, x y 1 u v vx vy)]; a failed
//                                              call (last_rc != SWF_OK) returns an empty map
//   removeOutliers(ids)                        as the reference
// info and counts of the last frame are the words of swf_tracker_download.  setPrediction, the stereo branch and drawTrack are not
// covered.  The seed of the F gate's sampling is the frame number, so a sequence is reproducible.
class FeatureTracker {
public:
    typedef std::map<int, std::vector<std::pair<int, std::array<double, 7>>>> FeatureFrame;
    FeatureTracker(int rows, int cols, const double cam[12], const swf_tracker_options* options = nullptr) {
        swf_tracker_options o;
        swf_tracker_default_options(&o);
        if (options) o = *options;
        max_cnt_ = o.max_cnt;
        last_rc = swf_tracker_create(1, rows, cols, cam, &o, nullptr, &t_);
    }
    ~FeatureTracker() { swf_tracker_destroy(t_); }
    FeatureTracker(const FeatureTracker&) = delete;
    FeatureTracker& operator=(const FeatureTracker&) = delete;

    FeatureFrame trackImage(double cur_time, const uint8_t* img, const uint8_t* mask = nullptr) {
        FeatureFrame frame;
        if (!t_) return frame;
        last_rc = swf_tracker_track(t_, &cur_time, img, mask, (uint64_t)n_frames_, 0);
        if (last_rc != SWF_OK) return frame;
        n_frames_++;
        const size_t cap = (size_t)(max_cnt_ > 0 ? max_cnt_ : 1);
        int32_t n = 0;
        ids.assign(cap, 0); track_cnt.assign(cap, 0);
        std::vector<double> obs(cap * 7, 0.0);
        last_rc = swf_tracker_download(t_, &n, ids.data(), track_cnt.data(), obs.data(), counts, &info);
        if (last_rc != SWF_OK) n = 0;
        ids.resize((size_t)n); track_cnt.resize((size_t)n);
        for (int32_t i = 0; i < n; i++) {
            std::array<double, 7> v;
            for (int k = 0; k < 7; k++) v[(size_t)k] = obs[(size_t)i * 7 + (size_t)k];
            frame[ids[(size_t)i]].emplace_back(0, v);
        }
        return frame;
    }
    void removeOutliers(const std::set<int>& removePtsIds) {
        if (!t_) return;
        const std::vector<int32_t> list(removePtsIds.begin(), removePtsIds.end());
        const int32_t first[2] = { 0, (int32_t)list.size() }, none = 0;
        last_rc = swf_tracker_remove_ids(t_, first, list.empty() ? &none : list.data());
    }

    int last_rc = SWF_OK;
    int32_t info = 0, counts[SWF_TRACKER_NCOUNT] = { 0 };
    std::vector<int32_t> ids, track_cnt;                // of the last frame, in the tracker's order
private:
    swf_tracker* t_ = nullptr;
    int max_cnt_ = 0;
    long long n_frames_ = 0;
};

// The track table: FeatureManager (R/feature/feature_manager.cpp) for one window, resident on the device (swf_ftable_* with one
// stream; a caller with many windows creates one swf_ftable with as many streams).  World-point mode (USE_INVERSE_DEPTH 0),
// no stereo.  Poses are plain arrays by image frame: Ps [window][3], Rs [window][9] row-major; tic [3], ric [9] row-major, pbg [3].
//   addFeatureCheckParallax(image_index, image)   takes FeatureTracker's featureFrame; image_index must be the table's frame count.
//                                                 removeOut runs in the same enqueue, so removeOut() itself has nothing left to do
//   pnpPoints(pts_w, pts_uv)                      the gather of initFramePoseByPnP, the input of InitFramePoseByPnP above
//   triangulate(Ps, Rs, tic, ric, pbg)            the two-view branch, bit-identical to swf_triangulate_batch
//   listFeatures(L)                               AddFeature2Problem as data (Listing below); setSolved() takes the solve's points back
//   removeFailures()                              returns the erased ids: the argument of FeatureTracker::removeOutliers
//   CheckParallax(image_index), removeBack(P0, R0, P1, R1, tic, ric, pbg), removeFront(image_index), ClearState(), getFeatureCount()
// counts are the words of swf_ftable_counts after the last call that read them; info is counts[SWF_FTABLE_C_INFO].
class FeatureManager {
public:
    struct Listing {
        std::vector<int32_t> lm_id, lm_start, lm_nobs, lm_valid, proj_frame, proj_lm, proj_new;
        std::vector<double> lm_world, proj_uv;          // [..][3], [..][2]
    };
    explicit FeatureManager(const swf_ftable_options* options = nullptr) {
        swf_ftable_default_options(&opt_);
        if (options) opt_ = *options;
        last_rc = swf_ftable_create(1, &opt_, nullptr, &t_);
    }
    ~FeatureManager() { swf_ftable_destroy(t_); }
    FeatureManager(const FeatureManager&) = delete;
    FeatureManager& operator=(const FeatureManager&) = delete;

    void ClearState() { if (t_) last_rc = swf_ftable_clear(t_); }
    bool addFeatureCheckParallax(int image_index, const FeatureTracker::FeatureFrame& image) {
        if (!t_) return true;
        std::vector<int32_t> ids;
        std::vector<double> obs;
        for (const auto& id_pts : image) {
            if (id_pts.second.empty()) continue;
            ids.push_back(id_pts.first);
            for (int k = 0; k < 7; k++) obs.push_back(id_pts.second[0].second[(size_t)k]);
        }
        const int32_t first[2] = { 0, (int32_t)ids.size() }, none = 0;
        const double zero[7] = { 0, 0, 0, 0, 0, 0, 0 };
        last_rc = swf_ftable_add_frame(t_, first, ids.empty() ? &none : ids.data(), obs.empty() ? zero : obs.data(), 0);
        if (last_rc == SWF_OK) fetch();
        last_track_num = counts[SWF_FTABLE_C_LAST_TRACK]; long_track_num = counts[SWF_FTABLE_C_LONG_TRACK];
        new_feature_num = counts[SWF_FTABLE_C_NEW];
        (void)image_index;
        return last_rc != SWF_OK || counts[SWF_FTABLE_C_KEYFRAME] != 0;
    }
    void removeOut(int /*windowsize*/) {}
    bool CheckParallax(int /*image_index*/) {
        if (!t_) return true;
        last_rc = swf_ftable_check_parallax(t_);
        if (last_rc == SWF_OK) fetch();
        last_average_parallax = parallax_;
        return last_rc != SWF_OK || counts[SWF_FTABLE_C_KEYFRAME] != 0;
    }
    void pnpPoints(std::vector<double>& pts_w, std::vector<double>& pts_uv) {
        pts_w.clear(); pts_uv.clear();
        if (!t_) return;
        const int32_t* f = nullptr; const double* w = nullptr; const double* uv = nullptr;
        int32_t first[2] = { 0, 0 };
        last_rc = swf_ftable_pnp_points(t_, &f, &w, &uv);
        if (last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, first, f, sizeof(first));
        if (last_rc != SWF_OK || first[1] <= 0) return;
        pts_w.resize((size_t)first[1] * 3); pts_uv.resize((size_t)first[1] * 2);
        last_rc = swf_ftable_fetch(t_, pts_w.data(), w, pts_w.size() * sizeof(double));
        if (last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, pts_uv.data(), uv, pts_uv.size() * sizeof(double));
    }
    void triangulate(const double* Ps, const double* Rs, const double tic[3], const double ric[9], const double pbg[3]) {
        if (t_) last_rc = swf_ftable_triangulate(t_, Ps, Rs, tic, ric, pbg, 0);
    }
    void listFeatures(Listing& L) {
        L = Listing();
        if (!t_) return;
        swf_ftable_listing d;
        int32_t lf[2] = { 0, 0 }, pf[2] = { 0, 0 };
        last_rc = swf_ftable_list(t_, &d);
        if (last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, lf, d.lm_first, sizeof(lf));
        if (last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, pf, d.proj_first, sizeof(pf));
        if (last_rc != SWF_OK) return;
        const size_t n = (size_t)(lf[1] > 0 ? lf[1] : 0), m = (size_t)(pf[1] > 0 ? pf[1] : 0);
        auto ints = [&](std::vector<int32_t>& v, const int32_t* src, size_t k) { v.resize(k); if (k && last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, v.data(), src, k * sizeof(int32_t)); };
        auto reals = [&](std::vector<double>& v, const double* src, size_t k) { v.resize(k); if (k && last_rc == SWF_OK) last_rc = swf_ftable_fetch(t_, v.data(), src, k * sizeof(double)); };
        ints(L.lm_id, d.lm_id, n); ints(L.lm_start, d.lm_start, n); ints(L.lm_nobs, d.lm_nobs, n); ints(L.lm_valid, d.lm_valid, n);
        reals(L.lm_world, d.lm_world, n * 3);
        ints(L.proj_frame, d.proj_frame, m); ints(L.proj_lm, d.proj_lm, m); ints(L.proj_new, d.proj_new, m);
        reals(L.proj_uv, d.proj_uv, m * 2);
    }
    int getFeatureCount() {                             // the features a listing would hold; in_problem is not touched
        if (!t_) return 0;
        std::vector<int32_t> n((size_t)opt_.feat_cap, 0);
        int32_t n_feat = 0;
        last_rc = swf_ftable_download(t_, nullptr, &n_feat, nullptr, nullptr, n.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        int cnt = 0;
        for (int32_t i = 0; last_rc == SWF_OK && i < n_feat; i++) cnt += n[(size_t)i] >= opt_.feature_continue ? 1 : 0;
        return cnt;
    }
    // lm_world [n][3] in the order of the last listFeatures; flags [n] (swf_batch_get_feature_check's) or null
    void setSolved(const std::vector<double>& lm_world, const uint8_t* flags, const double* Ps, const double* Rs, const double tic[3],
                   const double ric[9], const double pbg[3]) {
        if (!t_) return;
        const int32_t first[2] = { 0, (int32_t)(lm_world.size() / 3) };
        const double zero[3] = { 0, 0, 0 };
        last_rc = swf_ftable_set_solved(t_, first, lm_world.empty() ? zero : lm_world.data(), flags, Ps, Rs, tic, ric, pbg, 0);
    }
    std::set<int> removeFailures() {
        std::set<int> gone;
        if (!t_) return gone;
        last_rc = swf_ftable_remove_failures(t_, nullptr, nullptr);
        int32_t first[2] = { 0, 0 };
        std::vector<int32_t> ids((size_t)opt_.feat_cap, 0);
        if (last_rc == SWF_OK) last_rc = swf_ftable_removed(t_, first, ids.data());
        for (int32_t i = 0; last_rc == SWF_OK && i < first[1]; i++) gone.insert(ids[(size_t)i]);
        return gone;
    }
    void removeBack(const double P0[3], const double R0[9], const double P1[3], const double R1[9], const double tic[3], const double ric[9],
                    const double pbg[3]) {
        const int32_t mode = 1;
        if (t_) last_rc = swf_ftable_slide(t_, &mode, P0, R0, P1, R1, tic, ric, pbg, 0);
    }
    void removeFront(int /*image_index*/) {
        const int32_t mode = 2;
        const double z3[3] = { 0, 0, 0 }, eye[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        if (t_) last_rc = swf_ftable_slide(t_, &mode, nullptr, nullptr, z3, eye, z3, eye, z3, 0);
    }
    swf_ftable* handle() { return t_; }

    int last_rc = SWF_OK;
    int last_track_num = 0, new_feature_num = 0, long_track_num = 0;
    double last_average_parallax = 0.0;
    int32_t counts[SWF_FTABLE_NCOUNT] = { 0 };
private:
    void fetch() { last_rc = swf_ftable_counts(t_, counts, &parallax_); }
    swf_ftable* t_ = nullptr;
    swf_ftable_options opt_;
    double parallax_ = 0.0;
};

}  // namespace swf_ceres
