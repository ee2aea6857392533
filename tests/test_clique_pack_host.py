"""The plan records, for the class-0 cliques of the batch path, the largest n_rows and the leading dimension that holds the largest d
(Plan::clp_rows / clp_ld: k_clique_pack sizes its LDS by them), and plan_validate checks both against every class-0 record.  On the
CPU, through swf_debug_plan_check (plan_build + plan_validate, no device) with its 12-int info: a batch of mixed clique shapes, a
batch at the class envelope (48 rows, leading dimension 33) and a one-window batch validate — with the latency path switched off
(flags = 1, SWF_NO_LAT_FUSE), where class 0 exists, on a full-size and on a tiny chip, and on the latency path, where it is empty."""
import pytest

from plan_cases import clique_batches, plan_check


@pytest.mark.parametrize("name", ["mixed", "envelope", "beyond", "one", "free"])
def test_class0_lds_extent_validates(name):
    wins = clique_batches()[name]
    for n_cu, flags in ((256, 1), (8, 1), (8, 3), (256, 0)):
        rc, msg, info = plan_check(wins, n_cu, flags=flags)
        assert rc == 0, (name, n_cu, flags, msg)
        if flags & 1:
            assert info["lat_fuse"] == 0, (name, n_cu)              # the batch path: class 0 is populated, its extent was checked
