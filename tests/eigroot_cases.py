"""Seeded windows of tests/test_eigroot_componentwise.py — TEST INFRASTRUCTURE.

Each is the smallest window that still reaches the path of the square root named next to it (csrc/swf_kernels3.h, csrc/swf_rootdev.h).
The tail of synth.make_window(3, K, F, S, head="frames") has 15 (K - 1) + S dimensions (head="ambiguities": S); every case states its
tail dimension and the tests assert it.  F is kept small (three landmarks per frame, or the existing test's window).

The three window edits (weak and strong tail scalars, an unobservable pair, a singular marginalised block) are those of
tests/test_gpu_parity.py, which imports them from here."""
import numpy as np

from rtk_visual_inertial_navigation_amd import synth

# The constants of the componentwise rules of tests/np_eigroot.py: name = ceil(8 x the largest ratio of the float64 routes over every case),
# held to the measured ratios by test_constants_are_the_measured_ones; the ratio, the route and the case it came from
M_JTJ = 14.0      # J^T J                  1.71  row-cyclic route, hbm_first (the oracle: 2181 there, normwise only, does not count)
M_JJT = 3.0       # J J^T off-diagonal     0.34  device order, weak_strong_k4
M_EIG = 61.0      # eig / row norm         7.62  row-cyclic route, lds_last (a plain 140-term sum)
M_LAM = 20.0      # eig / lambda           2.46  the oracle, odd — within 8 x of routes 1 / 2 (1.02, device order, odd): it counts
M_R0 = 2.0        # r0                     0.13  device order, tiny (the oracle: 1.65 on lds_last, 12.7 x, does not count)
M_JTR = 19.0      # J^T r0                 2.37  device order, odd
M_CHD = 4.0       # Cholesky-form eig      0.47  Cholesky form, tiny

WEAK = (3e-3, 1e-3, 3e-4)          # informations 9e-6, 1e-6, 9e-8: above the 1e-8 threshold, below 1e-14 x 1e10


def with_unobservable_pair(w0, istd=40.0):
    """Two extra scalars constrained only through their difference (one FixedIntegerFactor), appended to parameter_head: their
    marginal istd^2 [[1, -1], [-1, 1]] is exactly singular — the shape of an unobservable camera extrinsic or a yaw nobody measured."""
    from rtk_visual_inertial_navigation_amd.flat import FlatWindow
    w = w0.copy()
    n_sc = w.n_sc
    a = {k: v.copy() for k, v in w.a.items()}
    a["sc"] = np.concatenate([a["sc"], [0.3, -0.2]])
    a["is_const"] = np.concatenate([a["is_const"], [0, 0]]).astype(np.uint8)
    a["fix_idx"] = np.concatenate([a["fix_idx"].ravel(), [n_sc, n_sc + 1]]).astype(np.int32)
    a["fix_dat"] = np.concatenate([a["fix_dat"].ravel(), [2.0, istd]])
    nb = w.n_blocks
    g = int(a["order_group"].max()) + 1
    a["order_block"] = np.concatenate([a["order_block"], [nb, nb + 1]]).astype(np.int32)
    a["order_group"] = np.concatenate([a["order_group"], [g, g + 1]]).astype(np.int32)
    return FlatWindow(n_tail=w.n_tail + 2, proj_sqrt_info=w.proj_sqrt_info, proj_loss_a=w.proj_loss_a, pbg=w.pbg, gw=w.gw, base=w.base, meta=dict(w.meta), **a)


def with_singular_marginalised_block(w0, istd=40.0, free_scalar=True):
    """Extra scalars in the MARGINALISED part of the reduced system (ordered just ahead of the parameter_head tail): a pair constrained
    only through its difference (one FixedIntegerFactor: a null direction that is not a coordinate axis) and, optionally, a scalar no
    factor touches at all (a zero row and column) — S_mm is exactly singular, as for a state whose residual blocks GlobalMarge
    switched off (is_use = false, R/swf/swf_image.cpp:353-365) or a direction only a combination of which is measured."""
    from rtk_visual_inertial_navigation_amd.flat import FlatWindow
    w = w0.copy()
    n_sc = w.n_sc
    a = {k: v.copy() for k, v in w.a.items()}
    extra = [0.3, -0.2] + ([0.1] if free_scalar else [])
    a["sc"] = np.concatenate([a["sc"], extra])
    a["is_const"] = np.concatenate([a["is_const"], [0] * len(extra)]).astype(np.uint8)
    a["fix_idx"] = np.concatenate([a["fix_idx"].ravel(), [n_sc, n_sc + 1]]).astype(np.int32)
    a["fix_dat"] = np.concatenate([a["fix_dat"].ravel(), [2.0, istd]])
    nb = w.n_blocks
    ob_, og_ = a["order_block"], a["order_group"]
    cut = len(ob_) - w.n_tail
    g0 = int(og_[cut]) if w.n_tail else int(og_.max()) + 1
    ne = len(extra)
    a["order_block"] = np.concatenate([ob_[:cut], nb + np.arange(ne), ob_[cut:]]).astype(np.int32)
    a["order_group"] = np.concatenate([og_[:cut], g0 + np.arange(ne), og_[cut:] + ne]).astype(np.int32)
    return FlatWindow(n_tail=w.n_tail, proj_sqrt_info=w.proj_sqrt_info, proj_loss_a=w.proj_loss_a, pbg=w.pbg, gw=w.gw, base=w.base, meta=dict(w.meta), **a)


def with_weak_and_strong_tail_scalars(w0, weak=WEAK, strong=1e5):
    """Extra scalars INSIDE the parameter_head tail, each touched by one scalar prior only (InitialBlackFactor, information w^2):
    one of information `strong`^2 = 1e10 and some of information 1e-5 .. 1e-7 — states the estimator has barely observed yet (a carrier-phase
    ambiguity of a satellite that has just risen) next to a very well known one."""
    from rtk_visual_inertial_navigation_amd.flat import FlatWindow
    w = w0.copy()
    n_sc = w.n_sc
    a = {k: v.copy() for k, v in w.a.items()}
    ws = [strong] + list(weak)
    ne = len(ws)
    a["sc"] = np.concatenate([a["sc"], 0.01 * np.arange(1, ne + 1)])
    a["is_const"] = np.concatenate([a["is_const"], [0] * ne]).astype(np.uint8)
    a["sp_idx"] = np.concatenate([a["sp_idx"].ravel(), n_sc + np.arange(ne)]).astype(np.int32)
    a["sp_w"] = np.concatenate([a["sp_w"].ravel(), ws])
    nb = w.n_blocks
    g1 = int(a["order_group"].max()) + 1
    a["order_block"] = np.concatenate([a["order_block"], nb + np.arange(ne)]).astype(np.int32)
    a["order_group"] = np.concatenate([a["order_group"], g1 + np.arange(ne)]).astype(np.int32)
    return FlatWindow(n_tail=w.n_tail + ne, proj_sqrt_info=w.proj_sqrt_info, proj_loss_a=w.proj_loss_a, pbg=w.pbg, gw=w.gw, base=w.base, meta=dict(w.meta), **a)


def _tiny():
    return synth.make_window(3, K=6, F=30, S=6, seed=21, head="ambiguities")


def _ws4():
    return with_weak_and_strong_tail_scalars(synth.make_window(3, K=4, F=20, S=8, seed=91, head="ambiguities"))


def _unobs():
    return with_unobservable_pair(_tiny())


# name -> dict(make, tail, forms (0 = eigen, 1 = Cholesky), force = SWF_FORCE_MARG_RESCUE, jacobi = judged against jacobi_ld (tail <= 141),
#              full = the marginal is of full rank, term = the terminations a step_mode = 1 solve may report)
def _case(make, tail, forms=(0, 1), force=False, jacobi=True, full=True, term=(7,)):
    return dict(make=make, tail=tail, forms=forms, force=force, jacobi=jacobi, full=full, term=term)


CASES = {
    # one pair per group of the round-robin
    "tiny": _case(_tiny, 6),
    # an odd tail: the bye of the round-robin
    "odd": _case(lambda: synth.make_window(3, K=3, F=9, S=5, seed=41, head="frames"), 35),
    # the last LDS-resident M, the INPLACE preconditioner
    "lds_last": _case(lambda: synth.make_window(3, K=10, F=30, S=5, seed=42, head="frames"), 140),
    # the first tail of k_marg_pchol + k_marg_bj<8>
    "hbm_first": _case(lambda: synth.make_window(3, K=10, F=30, S=6, seed=43, head="frames"), 141),
    # the block-size switch of k_marg_bj: product rules only
    "bj8_last": _case(lambda: synth.make_window(3, K=39, F=40, S=6, seed=44, head="frames"), 576, jacobi=False),
    "bj4_first": _case(lambda: synth.make_window(3, K=39, F=40, S=7, seed=44, head="frames"), 577, jacobi=False),
    # informations 1e10 next to 9e-8, on both Jacobi paths (the windows of test_eigen_prior_keeps_weakly_observed_states_...)
    "weak_strong_k4": _case(_ws4, 12),
    "weak_strong_k10": _case(lambda: with_weak_and_strong_tail_scalars(synth.make_window(3, K=10, F=60, S=6, seed=93, head="frames")), 145, jacobi=False),
    # rank n - 1, whichever way the factorisation went (the Cholesky form reports rank -1 when it broke down)
    "unobservable": _case(_unobs, 8, forms=(0,), full=False, term=(6, 7)),
    # the null-pivot skip of k_marg_rescue
    "singular_mm": _case(lambda: with_singular_marginalised_block(_tiny()), 6, forms=(0,), term=(6, 7)),
    # the rescue factor as G
    "rescue_forced_tiny": _case(_tiny, 6, forms=(0,), force=True),
    "rescue_forced_lds_last": _case(lambda: CASES["lds_last"]["make"](), 140, forms=(0,), force=True),
    "rescue_forced_hbm_first": _case(lambda: CASES["hbm_first"]["make"](), 141, forms=(0,), force=True),
    # the predicted finding: weak states next to a strong one through k_marg_rescue's rank-revealing factorisation
    "rescue_weak_forced": _case(_ws4, 12, forms=(0,), force=True),
    "rescue_weak_unobservable": _case(lambda: with_weak_and_strong_tail_scalars(_unobs()), 12, forms=(0,), full=False, term=(6, 7)),
    # (the singular pair can slip through the device's Cholesky on a pivot of a few ulp — the window is then healthy and the line above
    # takes the regular path; forced, it takes k_marg_rescue either way)
    "rescue_weak_unobservable_forced": _case(lambda: with_weak_and_strong_tail_scalars(_unobs()), 12, forms=(0,), force=True, full=False, term=(6, 7)),
}

# the cases whose marginal the CPU routes can form (a definite S) and that are not a second run of the same window
CPU_FULL = ("tiny", "odd", "lds_last", "hbm_first", "weak_strong_k4", "weak_strong_k10")
CPU_DEFICIENT = ("unobservable", "singular_mm", "rescue_weak_unobservable")
CYCLIC_MAX_N = 171                 # the row-cyclic float64 route and the oracle's two-sided Jacobi are run up to this tail
BATCH = ("tiny", "odd", "lds_last", "hbm_first", "weak_strong_k4", "weak_strong_k10", "unobservable")


def window(name):
    return CASES[name]["make"]()


def tail_dim(w):
    """local dimension of the window's parameter_head tail: its last n_tail blocks in elimination order"""
    _, l = w.block_sizes()
    return int(sum(l[b] for b in w.a["order_block"][len(w.a["order_block"]) - w.n_tail:]))
