"""Class-0 cliques of the batch path (receiver clocks, the dummy, small free groups) are eliminated two per wavefront by
k_clique_pack, out of LDS sized by the batch's largest class-0 clique.  SWF_NO_CLIQUE_PACK=1 keeps the one-wavefront-per-clique
k_clique_elim<48,32,1,0[,true]>; the two must give the same BYTES.  The knob is read when a batch is created, so each side of a
comparison is a fresh child process (tests/bitwise.py: it calls child() of this file on the named case and saves every output):
states, every summary field, the whole iteration trace, and export_reduced / export_vectors of an ASSEMBLE_ELIMINATE_ONLY solve of
the same windows.  Both children set SWF_NO_LAT_FUSE=1, so that a handful of windows takes the batch path and class 0 exists.

A cfg3 window has 21 class-0 cliques (20 clocks and the dummy), so a batch of an odd number of windows has an odd total (the last
wavefront's upper half idles) and every second window boundary falls inside a wavefront (a pair that straddles two windows)."""
import numpy as np
import pytest

import bitwise

KNOB = "SWF_NO_CLIQUE_PACK"


# ---------------------------------------------------------------------------------------------------------------- child side
def _mixed(synth):
    """Clock cliques of 20 x 17 (cfg3 default), 10 x 12 (S = 5) and 40 x 27 (S = 20) in one batch of five windows: paired halves
    differ in n_rows and d, the LDS is sized by the largest."""
    return [synth.make_window(3, seed=910), synth.make_window(3, K=6, F=30, S=5, seed=911), synth.make_window(3, K=6, F=30, S=20, seed=912),
            synth.make_window(3, seed=913), synth.make_window(3, K=6, F=30, S=5, seed=914)]


def _case(name):
    """-> (windows, options)"""
    from rtk_visual_inertial_navigation_amd import synth
    from rtk_visual_inertial_navigation_amd.flat import default_options
    if name in ("mixed", "mixed_full_final"):
        return _mixed(synth), default_options()
    if name == "mixed_lm":
        return _mixed(synth), default_options(strategy=1)
    if name == "envelope":
        # S = 24: 48 rows x 31 columns, the class's row limit and its leading dimension of 33
        return [synth.make_window(3, K=6, F=30, S=24, seed=920), synth.make_window(3, seed=921), synth.make_window(3, K=6, F=30, S=5, seed=922)], default_options()
    if name == "early_stop":
        still = synth.make_window(2, seed=706, perturb=False)
        return ([synth.make_window(config_id=3, F=103, seed=701), still, synth.make_window(3, seed=707), still.copy(),
                 synth.make_window(config_id=3, F=205, seed=702)], default_options(max_num_iterations=20))
    if name == "member_sets":
        base = synth.make_window(3, seed=930)
        return [bitwise.with_constant(base, [2]), synth.make_window(3, K=6, F=30, S=5, seed=931, doppler=True),
                synth.with_spp_and_fixed(synth.make_window(3, seed=932), seed=12, n_fix=2)], default_options()
    if name == "nan_pivot":
        ws = [synth.make_window(3, seed=940 + i) for i in range(3)]
        ws[1].a["pose"].reshape(-1, 7)[1, 0] = np.nan              # an input value: the window's clock pivots are not positive
        return ws, default_options()
    raise KeyError(name)


def child(name):
    from rtk_visual_inertial_navigation_amd import solver
    # the linearisation at the uploaded state alone (not of the NaN case), then the solve
    out = {} if name == "nan_pivot" else bitwise.dump_elimination(_case(name)[0])
    ws, opt = _case(name)
    bs = solver.BatchSolver(ws)
    out.update(bitwise.dump_solve(ws, bs.solve(opt)))
    bs.close()
    return out


# ----------------------------------------------------------------------------------------------------------------- test side
def _solve_in_child(name, path, env):
    return bitwise.solve_in_child("test_clique_pack_gpu", name, path, env, batch_kernels=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "mixed_lm", "mixed_full_final", "envelope", "early_stop", "member_sets", "nan_pivot"])
def test_two_cliques_per_wavefront_equal_one_per_wavefront_bitwise(name, tmp_path):
    both = {"SWF_FULL_FINAL_ELIM": "1"} if name == "mixed_full_final" else {}
    pack = _solve_in_child(name, str(tmp_path / "pack.npz"), dict(both))
    one = _solve_in_child(name, str(tmp_path / "one.npz"), dict(both, **{KNOB: "1"}))
    bitwise.assert_same_bytes(pack, one)
    n_win = len([k for k in pack if k.endswith("_summary_num_iterations")])
    nit = [int(pack["w%d_summary_num_iterations" % i]) for i in range(n_win)]
    term = [int(pack["w%d_summary_termination" % i]) for i in range(n_win)]
    print(name, "iterations per window:", nit, "termination:", term)
    assert n_win % 2 == 1                                                          # an odd number of windows: an odd total of class-0 cliques
    if name == "early_stop":
        assert max(nit[1], nit[2], nit[3]) < min(nit[0], nit[4]), nit             # the case is a case: some windows stopped before the others
    if name == "nan_pivot":
        # the window with the NaN failed, and took neither neighbour with it
        assert not np.all(np.isfinite(pack["w1_trace_cost"])) or term[1] != term[0], (term, pack["w1_trace_cost"])
        for i in (0, 2):
            assert all(np.all(np.isfinite(pack[k])) for k in pack if k.startswith("w%d_state_" % i) or k in ("w%d_trace_cost" % i, "w%d_trace_gradient_max_norm" % i)), i
            assert nit[i] > 1, nit
    else:
        assert any(k.endswith("_elim_S") for k in pack)
        assert all(np.all(np.isfinite(pack[k])) for k in pack if k.endswith("_trace_gradient_max_norm") or k.endswith("_elim_S"))
