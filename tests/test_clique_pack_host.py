"""The plan records, for the class-0 cliques of the batch path, the largest n_rows and the leading dimension that holds the largest d
(Plan::clp_rows / clp_ld: k_clique_pack sizes its LDS by them), and plan_validate checks both against every class-0 record.  On the
CPU, through swf_debug_plan_check (plan_build + plan_validate, no device) with its 12-int info: a batch of mixed clique shapes, a
batch at the class envelope (48 rows, leading dimension 33) and a one-window batch validate — with the latency path switched off
(flags = 1, SWF_NO_LAT_FUSE), where class 0 exists, on a full-size and on a tiny chip, and on the latency path, where it is empty."""
import pytest

from rtk_visual_inertial_navigation_amd import synth
from test_plan_host import plan_check


def _batches():
    mixed = [synth.make_window(3, seed=910), synth.make_window(3, K=6, F=30, S=5, seed=911), synth.make_window(3, K=6, F=30, S=20, seed=912),
             synth.make_window(3, seed=913), synth.make_window(3, K=6, F=30, S=5, seed=914)]
    # S = 24 satellites: clock cliques of 48 rows x 31 columns (the class's row limit; (31 + 1) | 1 = 33, its largest leading dimension);
    # S = 25 would be 50 rows and leaves class 0
    envelope = [synth.make_window(3, K=6, F=30, S=24, seed=920), synth.make_window(3, seed=921), synth.make_window(3, K=6, F=30, S=5, seed=922)]
    beyond = [synth.make_window(3, K=6, F=30, S=25, seed=923), synth.make_window(3, K=6, F=30, S=5, seed=922)]
    one = [synth.make_window(3, seed=924)]
    free = [synth.make_window(2, K=3, F=5, S=0, seed=3), synth.make_window(3, K=4, F=6, S=2, seed=2)]        # no satellites: the dummy and free groups alone
    return dict(mixed=mixed, envelope=envelope, beyond=beyond, one=one, free=free)


@pytest.mark.parametrize("name", ["mixed", "envelope", "beyond", "one", "free"])
def test_class0_lds_extent_validates(name):
    wins = _batches()[name]
    for n_cu, flags in ((256, 1), (8, 1), (8, 3), (256, 0)):
        rc, msg, info = plan_check(wins, n_cu, flags=flags)
        assert rc == 0, (name, n_cu, flags, msg)
        if flags & 1:
            assert info["lat_fuse"] == 0, (name, n_cu)              # the batch path: class 0 is populated, its extent was checked
