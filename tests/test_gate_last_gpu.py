"""What loading with the window's gate last can get wrong.  The IMU evaluation (d_eval_imu: k_eval_imu, the IMU segment of
k_eval_ps / k_step_eval) and k_clique_mm request, behind their block's record, the window's flag TOGETHER with the values that hang
off the record (lanes past the last factor take the last record's loads), and test the flag afterwards: a closed gate, a block that
is not filled or a record at the end of its array must neither read out of bounds nor change a byte.  The cases also cover what the
same rule touches in k_assemble_flat, k_chol_rr4, k_clique_pack and the clique segment of k_post_chol<2> (built in round 11,
measured, not kept: profiles/r11/README.md).

Every case is batch == the same windows solved alone, bit for bit (states, iteration counts, the cost and step_is_successful
columns of the trace), with the helpers of tests/bitwise.py; the batches are created with SWF_NO_LAT_FUSE=1 (no_lat_fuse=True), so that three to five
small windows take the batch kernels; the single windows run without it (the latency path: other launches, the same sums) except
under Levenberg-Marquardt (see that case).  The reduced system of an ASSEMBLE_ELIMINATE_ONLY solve of the batch is compared with
the CPU oracle at the tolerances of tests/test_gpu_parity.py (S, g, diag 1e-11; rhs 1e-10)."""
import numpy as np
import pytest

import oracle_binding as ob
from bitwise import (ELIMINATE_ONLY, assert_batch_equals_singles, assert_window_equal, batch_kernels, multi_processor_count, rel, solve_alone,
                     solve_batch, with_constant_pose_and_landmark)
from rtk_visual_inertial_navigation_amd import synth, solver
from rtk_visual_inertial_navigation_amd.flat import default_options

pytestmark = pytest.mark.gpu


def small(K, seed, **kw):
    return synth.make_window(3, K=K, F=30, S=5, seed=seed, **kw)


def assert_reduced_system_matches_oracle(ws):
    opt = default_options(step_mode=ELIMINATE_ONLY)
    with batch_kernels():
        bs = solver.BatchSolver([w.copy() for w in ws])
        bs.solve(opt)
        got = [(bs.export_reduced(i), bs.export_vectors(i)) for i in range(len(ws))]
        bs.close()
    for i, w in enumerate(ws):
        (S, rhs, _), (g, dg, _) = got[i]
        _, eo = ob.solve(w.copy(), opt)
        assert rel(S, eo["S"]) < 1e-11 and np.abs(S - S.T).max() == 0, i
        assert rel(rhs, eo["rhs"]) < 1e-10, i
        assert rel(g, eo["grad"]) < 1e-11 and rel(dg, eo["diag"]) < 1e-11, i


def test_unfilled_last_blocks_and_odd_clique_count_equal_single_bitwise():
    """K = 5, 6 and 7 frames: 4 + 5 + 6 = 15 IMU factors do not fill the last block of 8, the class-0 cliques of the three windows
    are an odd number (the last pair's upper half sits out), and K = 6 ends on a speed-bias clique of a single IMU factor."""
    ws = [small(5, 1101), small(6, 1102), small(7, 1103)]
    _, sms = assert_batch_equals_singles(ws, default_options(), no_lat_fuse=True)
    assert min(sm.num_iterations for sm in sms) > 1
    assert_reduced_system_matches_oracle(ws)


def test_finished_windows_at_both_ends_of_the_batch_equal_single_bitwise():
    """A window that starts at the truth converges before its neighbours (tests/test_load_levels_gpu.py: after 17 of 20 iterations,
    the window of seed 701 runs all 20).  One opens the batch and one closes it: their gates are closed while the loads of their
    blocks run, and their records are the first and the last of every table."""
    still = synth.make_window(2, seed=706, perturb=False)
    ws = [still, synth.make_window(config_id=3, F=103, seed=701), small(5, 1111), still.copy()]
    _, sms = assert_batch_equals_singles(ws, default_options(max_num_iterations=20), no_lat_fuse=True)
    its = [sm.num_iterations for sm in sms]
    print("iterations per window:", its)
    assert its[0] == its[3] and its[0] < max(its[1], its[2]), its      # the case is a case: both ends stopped while the middle ran


def test_constant_pose_and_landmark_equal_single_bitwise():
    """A constant pose and a constant landmark (their factors carry Jacobian offsets of -1; the pose's IMU factors leave columns
    of their cliques out), in the window that ends the batch."""
    wc = with_constant_pose_and_landmark(small(6, 1121))
    assert wc.a["is_const"][2] == 1
    ws = [small(7, 1122), small(5, 1123), wc]
    assert_batch_equals_singles(ws, default_options(), no_lat_fuse=True)
    assert_reduced_system_matches_oracle(ws)


def test_nan_pose_between_healthy_windows_leaves_the_neighbours_alone():
    ws = [small(6, 1131), small(5, 1132), small(7, 1133)]
    ws[1].a["pose"].reshape(-1, 7)[1, 0] = np.nan
    opt = default_options()
    singles = [solve_alone(w, opt) for w in ws]
    batch, sms = solve_batch(ws, opt, no_lat_fuse=True)
    for i in (0, 2):
        assert_window_equal(i, singles[i], batch[i], sms[i])
        assert sms[i].num_iterations > 1 and np.all(np.isfinite(batch[i].a["pose"]))
    # the failed window: its summary is the single window's (which NaN an instruction hands on is not part of the contract)
    assert sms[1].num_iterations == singles[1][1] and sms[1].termination == singles[1][4]
    assert not np.all(np.isfinite([r["cost"] for r in sms[1].rows()])) or sms[1].termination != sms[0].termination


def test_levenberg_marquardt_equal_single_bitwise():
    """Under Levenberg-Marquardt the latency path and the batch launches are not the same bytes (before round 11 either: window 0
    of this case, cost of iteration 7, 24.96931854727333 against 24.96931854727422), so the windows alone take the batch kernels
    too: one window per launch against three."""
    ws = [small(5, 1141), with_constant_pose_and_landmark(small(6, 1142)), small(7, 1143)]
    _, sms = assert_batch_equals_singles(ws, default_options(strategy=1), no_lat_fuse=True, batch_shapes=True)
    assert min(sm.num_iterations for sm in sms) > 1


def test_more_windows_than_compute_units_equal_single_bitwise():
    """multi_processor_count + 1 tiny windows: k_post_chol<1> / <2> run as launches of their own and k_chol_rr4 goes into a
    second round of blocks.  Three distinct windows, repeated: each copy must end on its single solve's bytes."""
    n = multi_processor_count() + 1
    kinds = [synth.make_window(3, K=4, F=6, S=2, seed=1151 + i) for i in range(3)]
    opt = default_options()
    singles = [solve_alone(w, opt) for w in kinds]
    batch, sms = solve_batch([kinds[i % 3] for i in range(n)], opt, no_lat_fuse=True)
    assert len(batch) == n
    for i in range(n):
        assert_window_equal(i, singles[i % 3], batch[i], sms[i])
    assert min(sm.num_iterations for sm in sms) > 1
