"""The flat evaluation record of an IMU factor (ImuRec, csrc/swf_records.h: window, factor, residual row, pre-integration record,
Jacobian stride, the four state offsets and the four Jacobian offsets) is built by the plan next to the J v records, one per entry
of imu_gf, and plan_validate holds every field against the factor it copies and against its array with the full extent a lane of
d_eval_imu touches before it tests the window's gate.  On the CPU, through swf_debug_plan_check (plan_build + plan_validate, no
device): the records validate for batches of mixed shapes on a full-size and a tiny chip, with the latency path on and off, and a
damaged record is reported."""
import pytest

from bitwise import with_constant_pose_and_landmark
from plan_cases import clique_batches, plan_check
from rtk_visual_inertial_navigation_amd import synth

E_INVALID = -2
IMU_REC = 8                       # corrupt_table id of imu_rec (swf_debug_plan_check)


@pytest.mark.parametrize("name", ["mixed", "envelope", "beyond", "one", "free"])
def test_imu_records_validate(name):
    wins = clique_batches()[name]
    for n_cu in (256, 8):
        for flags in (0, 1):
            rc, msg, _ = plan_check(wins, n_cu, flags=flags)
            assert rc == 0, (name, n_cu, flags, msg)


def test_a_damaged_imu_record_is_reported():
    wins = clique_batches()["mixed"]
    n_imu = sum(int(w.a["imu_idx"].size) // 4 for w in wins)
    assert n_imu >= 10
    for flags in (0, 1):
        assert plan_check(wins, flags=flags)[0] == 0
        for index in (0, n_imu // 2, n_imu - 1):              # the first, one inside and the last record of the batch
            rc, msg, _ = plan_check(wins, flags=flags, corrupt=(IMU_REC, index))
            assert rc == E_INVALID and msg.startswith("plan_validate: imu_rec"), (flags, index, msg)
    # past the last record there is nothing to damage: the hook says so
    rc, msg, _ = plan_check(wins, corrupt=(IMU_REC, n_imu))
    assert rc == E_INVALID and "nothing to corrupt" in msg, msg
    # a window with a constant pose (Jacobian offsets of -1 in its records) validates
    wc = with_constant_pose_and_landmark(synth.make_window(3, K=6, F=30, S=5, seed=931))
    for flags in (0, 1):
        rc, msg, _ = plan_check([wins[1], wc], flags=flags)
        assert rc == 0, msg
