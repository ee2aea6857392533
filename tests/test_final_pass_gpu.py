"""The solve's final linearisation forms the gradient alone (k_finalize reads nothing else of it): the clique kernels stop behind
g / diag / vc / graw / dgraw, the landmark pass skips the 3x3 inverse and its records.  SWF_FULL_FINAL_ELIM=1 restores the complete
elimination in that pass.  The knob is read when a batch is created, so each side of a comparison is a fresh child process
(tests/bitwise.py: it calls child() of this file on the named case and saves every output); the two files must hold the same bytes:
states, every summary field, the whole iteration trace (gradient_max_norm of every iteration included), and what tail_covariance /
ambiguity_search / check_features return behind the solve — no consumer reads what the final pass no longer writes.

The second group is about the |J D^-2 g|^2 pass of k_post_chol (g_aux): model_cost_change and the trust-region radius of every
iteration are the same bits in the speculative flow and in the two-pass flow (SWF_NO_SPEC_EVAL=1), and for a window alone and
inside a batch."""
import numpy as np
import pytest

import bitwise

KNOB = "SWF_FULL_FINAL_ELIM"
S_AMB = 9


# ---------------------------------------------------------------------------------------------------------------- child side
def _case(name):
    """-> (windows, options, consumers?)"""
    from rtk_visual_inertial_navigation_amd import synth
    from rtk_visual_inertial_navigation_amd.flat import default_options
    cfg3 = lambda: [synth.make_window(3, seed=810 + i) for i in range(5)] + [synth.make_window(3, K=6, F=30, S=5, seed=816),
                                                                                synth.make_window(config_id=3, F=103, seed=817)]
    if name == "cfg3_dogleg":
        return cfg3(), default_options(), False
    if name == "cfg3_lm":
        return cfg3(), default_options(strategy=1), False
    if name == "single_latency":
        return [synth.make_window(3, seed=820)], default_options(), False
    if name == "composite":
        import composite_gen as cg
        rng = np.random.default_rng(91)
        return [cg.make_window(rng, 5, 2, 8, F=30)], default_options(), False
    if name == "constant_blocks":
        base = synth.make_window(3, seed=830)
        return [bitwise.with_constant(base, [2]), bitwise.with_constant(base, [base.bid_lm(3)]), base], default_options(), False
    if name == "early_stop":
        still = synth.make_window(2, seed=706, perturb=False)
        return ([synth.make_window(config_id=3, F=103, seed=701), still, synth.make_window(3, seed=707), still.copy(),
                 synth.make_window(config_id=3, F=205, seed=702)], default_options(max_num_iterations=20), False)
    if name == "consumers":
        return [synth.make_window(3, S=S_AMB, seed=900 + i, head="ambiguities") for i in range(3)], default_options(), True
    if name == "aux_batch":
        return ([synth.make_window(3, seed=840), synth.make_window(3, K=6, F=30, S=5, seed=841, doppler=True),
                 synth.with_spp_and_fixed(synth.make_window(3, seed=842), seed=12, n_fix=2)], default_options(), False)
    if name.startswith("aux_single"):
        ws, opt, _ = _case("aux_batch")
        return [ws[int(name[len("aux_single"):])]], opt, False
    raise KeyError(name)


def child(name):
    from rtk_visual_inertial_navigation_amd import solver
    ws, opt, consumers = _case(name)
    bs = solver.BatchSolver(ws)
    out = bitwise.dump_solve(ws, bs.solve(opt))
    if consumers:
        tc = bs.tail_covariance()
        am = bs.ambiguity_search([[(j, 0) for j in range(1, S_AMB)]] * len(ws))
        fc = bs.check_features(2.0)
        for i in range(len(ws)):
            assert tc[i]["n"] == S_AMB
            out["w%d_tail_A" % i] = tc[i]["A"]; out["w%d_tail_Qy" % i] = tc[i]["Qy"]
            for k in ("F", "s", "ratio", "Qb", "bf"):
                out["w%d_amb_%s" % (i, k)] = am[i][k]
            out["w%d_amb_flags" % i] = np.array([int(am[i]["fixed"]), am[i]["n_b"], am[i]["info"]])
            for k in ("mean_err", "depth", "n_obs", "flags", "rejected"):
                out["w%d_feat_%s" % (i, k)] = fc[i][k]
    bs.close()
    return out


# ----------------------------------------------------------------------------------------------------------------- test side
def _solve_in_child(name, path, env):
    """The children run without SWF_NO_LAT_FUSE: a case takes the launch path its own batch size gives it."""
    return bitwise.solve_in_child("test_final_pass_gpu", name, path, env, batch_kernels=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3_dogleg", "cfg3_lm", "single_latency", "composite", "constant_blocks", "early_stop", "consumers"])
def test_gradient_only_final_pass_equals_full_elimination_bitwise(name, tmp_path):
    grad = _solve_in_child(name, str(tmp_path / "grad.npz"), {})
    full = _solve_in_child(name, str(tmp_path / "full.npz"), {KNOB: "1"})
    bitwise.assert_same_bytes(grad, full, nan_equal=False)                 # the same bytes, and no NaN anywhere
    nit = [int(grad[k]) for k in sorted(grad) if k.endswith("_summary_num_iterations")]
    print(name, "iterations per window:", nit)
    assert all(np.all(np.isfinite(grad[k])) for k in grad if k.endswith("_trace_gradient_max_norm"))
    if name == "early_stop":
        assert max(nit[1], nit[2], nit[3]) < min(nit[0], nit[4]), nit      # the case is a case: some windows stopped before the others
    if name == "consumers":
        assert any(k.endswith("_amb_F") for k in grad) and any(k.endswith("_feat_mean_err") for k in grad)


@pytest.mark.gpu
def test_cauchy_pass_outputs_equal_two_pass_flow_and_single_window_bitwise(tmp_path):
    """model_cost_change and the trust-region radius come from |J D^-2 g|^2 (g_aux, k_post_chol's factor segments)."""
    aux = lambda d: [k for k in sorted(d) if k.endswith("_trace_model_cost_change") or k.endswith("_trace_trust_region_radius")]
    spec = _solve_in_child("aux_batch", str(tmp_path / "spec.npz"), {})
    two = _solve_in_child("aux_batch", str(tmp_path / "two.npz"), {"SWF_NO_SPEC_EVAL": "1"})
    assert len(aux(spec)) == 6
    bitwise.assert_same_bytes(spec, two, nan_equal=False)
    for i in range(3):
        one = _solve_in_child("aux_single%d" % i, str(tmp_path / ("one%d.npz" % i)), {})
        for k in sorted(one):
            kb = "w%d_" % i + k[len("w0_"):]
            assert np.array_equal(one[k], spec[kb]), (i, k)
        assert np.any(one["w0_trace_model_cost_change"] != 0.0)
