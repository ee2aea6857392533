"""Cases of tests/test_step_componentwise.py — TEST INFRASTRUCTURE.  A case is a window (most of them schur_cases' own) and the options of the
ONE trust-region iteration that is judged: strategy, Jacobi scaling and the initial trust-region radius, which selects the dogleg branch.

The radii of the branch cases were found with the oracle on the CPU (the scaled Gauss-Newton norm |sqrt(D) y| and the Cauchy length
alpha |g / sqrt(D)| of the first iteration are printed by test_case_reaches_its_branch): below the Cauchy length the clipped Cauchy step,
between the two the interpolation, above the Gauss-Newton norm the Gauss-Newton step.  Every radius sits at least 20 % from either
threshold; the test asserts 1e-6."""
import numpy as np

import bitwise
import schur_cases as sc
from rtk_visual_inertial_navigation_amd import synth
from rtk_visual_inertial_navigation_amd.flat import default_options

GN, CAUCHY, INTERP = 0, 1, 2
DOGLEG, LM = 0, 1


def _constant_landmark():
    w = synth.make_window(3, K=6, F=30, S=5, seed=1021)
    return bitwise.with_constant(w, [w.bid_lm(int(np.bincount(w.a["proj_idx"].reshape(-1, 3)[:, 2]).argmax()))])      # the longest track's landmark


# windows of this file alone
WINDOWS = {
    # one landmark held constant (no local columns: lloc < 0 in the back-substitution of its observations)
    "constant_landmark": _constant_landmark,
    # 12 frames, 60 landmarks: more than 256 observations, the landmark blocks span more than one back-substitution block
    "obs_over_256": lambda: synth.make_window(3, K=12, F=60, S=5, seed=31),
    # a few frames and about 350 landmarks: n_loc > 1024, the strided tail loops of k_dogleg<4, 2> (launch-shape case, GPU only)
    "n_loc_over_1024": lambda: synth.make_window(2, K=4, F=350, S=0, seed=41),
    # n_loc > 4096 and few frames: k_dogleg<16, 4>'s range (launch-shape case, GPU only)
    "n_loc_over_4096": lambda: synth.make_window(2, K=4, F=1400, S=0, seed=43),
}


def window(name):
    return WINDOWS[name]() if name in WINDOWS else sc.window(name)


def options(strategy=DOGLEG, jacobi=0, radius=1e4, **kw):
    o = default_options(max_num_iterations=1, strategy=strategy, jacobi_scaling=jacobi, **kw)
    o.initial_trust_region_radius = radius
    return o


# case name -> (window name, dict(strategy, jacobi, radius), expected branch or None = whatever the default radius gives)
CASES = {}
for _n in ("tiny_vi", "tiny_rtk", "ragged", "doppler", "spp_fixed", "idepth_short", "idepth_long", "var_extrinsic", "dense_prior",
           "composite_landmarks", "constant_pose", "frames_22", "tracks_33", "constant_landmark", "obs_over_256",
           "n_red_241", "n_red_256", "n_red_278", "n_red_550"):
    CASES[_n] = (_n, dict(), None)
# the dogleg branches: (Gauss-Newton inside the radius, clipped Cauchy, interpolation)
BRANCH_RADII = {"tiny_vi": (1e4, 1.8e3, 4.6e3), "ragged": (4e4, 3e3, 1e4), "dense_prior": (4e4, 5e3, 1.45e4)}
for _n, (_a, _b, _c) in BRANCH_RADII.items():
    CASES[_n + "-gn"] = (_n, dict(radius=_a), GN)
    CASES[_n + "-cauchy"] = (_n, dict(radius=_b), CAUCHY)
    CASES[_n + "-interp"] = (_n, dict(radius=_c), INTERP)
for _n in ("tiny_rtk", "ragged"):
    CASES[_n + "-lm"] = (_n, dict(strategy=LM), GN)
    CASES[_n + "-lm-jacobi"] = (_n, dict(strategy=LM, jacobi=1), GN)

# the mutation controls run on these (back-substitution controls on the first, dogleg controls on the second of each pair)
CONTROL = (("tiny_vi-gn", "tiny_vi-interp"), ("ragged-gn", "ragged-interp"), ("dense_prior-gn", "dense_prior-interp"))

# launch shapes of the GPU tier
KNOBS = ({"SWF_NO_STEP_FUSE": "1"}, {"SWF_NO_SPEC_EVAL": "1"}, {"SWF_NO_LAT_FUSE": "1"})
KNOB_CASES = ("ragged-interp", "tiny_rtk", "dense_prior-cauchy")
BATCH_HEAD = sc.BATCH_HEAD
BATCH_N = sc.BATCH_N
