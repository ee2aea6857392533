"""What the landmark back-substitution (d_backsub_lm, k_post_chol<1>) can get wrong once its per-landmark loads (lm_g, lm_Einv,
lm_loc, lm_obs0) are requested behind the Jacobian derivation, in front of the block's reduction, and y / D^-2 g at the pose and
at the landmark behind proj_core: the lanes past a block's last landmark take the block's first landmark's loads, the final block
of the batch ends at the end of lm_g / lm_Einv / lm_obs0, and a closed or failed gate must leave every byte alone.

The landmark segment is launched by itself only from multi_processor_count windows up, so every case is a batch of
multi_processor_count + 1 windows: tiny fillers (K = 4, F = 6, S = 2, three kinds, repeated) around the windows that carry the
case.  Every case is batch == the same windows solved alone, bit for bit (states, iteration counts, the cost and
step_is_successful columns of the trace), with the helpers of tests/bitwise.py, the batches created with SWF_NO_LAT_FUSE=1.

The carrying window has K = 10 frames and F = 60 landmarks of five observations each: 300 observations, two landmark blocks, the
first nearly full (51 landmarks, 255 observations) and a short last one (9 landmarks, 45 observations).  (F = 30 gives 150
observations, one block.)  What a case claims about its windows is asserted from the windows themselves before anything runs."""
import functools

import numpy as np
import pytest

from rtk_visual_inertial_navigation_amd import synth
from rtk_visual_inertial_navigation_amd.flat import default_options
from bitwise import assert_window_equal, multi_processor_count, solve_alone, solve_batch, with_constant_pose_and_landmark

pytestmark = pytest.mark.gpu

LMB = 256                         # observations (and landmarks) per landmark back-substitution block, at most (csrc/swf_plan.cpp)
_singles = {}                     # (kind, max_num_iterations) -> the window solved alone: computed once, shared, never changed


def landmark_blocks(w):
    """(landmarks, observations) of the window's landmark back-substitution blocks, as plan_lm_blocks cuts them: consecutive
    landmarks while the block holds at most 256 of them and at most 256 observations."""
    lm = w.a["proj_idx"][:, 2]
    assert np.all(np.diff(lm) >= 0)
    cnt = np.unique(lm, return_counts=True)[1]
    out, i = [], 0
    while i < len(cnt):
        j, c = i, 0
        while j < len(cnt) and j - i < LMB and c + cnt[j] <= LMB:
            c += int(cnt[j]); j += 1
        assert j > i
        out.append((j - i, c)); i = j
    return out


@functools.lru_cache(maxsize=None)
def filler(i):
    """One of the three filler kinds; generated once (a batch holds the same object many times: solve_batch copies)."""
    return synth.make_window(3, K=4, F=6, S=2, seed=1151 + i)


@functools.lru_cache(maxsize=None)
def _big(seed):
    w = synth.make_window(3, K=10, F=60, S=5, seed=seed)
    blocks = landmark_blocks(w)
    # the case is a case: several blocks, a nearly full one and a short last one
    assert len(blocks) == 2 and blocks[0][1] >= LMB - 8 and blocks[1][1] < LMB // 4, blocks
    return w


def big(seed=1302):
    return _big(seed).copy()


def single(kind, w, opt, its):
    if (kind, its) not in _singles:
        _singles[(kind, its)] = solve_alone(w, opt)
    return _singles[(kind, its)]


def run_case(placed, its=None):
    """placed: {position: (kind, window)}, negative positions from the end.  Returns (n, singles by position, batch, summaries)."""
    n = multi_processor_count() + 1
    opt = default_options() if its is None else default_options(max_num_iterations=its)
    placed = {(p if p >= 0 else n + p): v for p, v in placed.items()}
    kinds = [placed[i] if i in placed else ("filler%d" % (i % 3), None) for i in range(n)]
    ws = [w if w is not None else filler(i % 3) for i, (_, w) in enumerate(kinds)]
    ref = [single(k, ws[i], opt, its) for i, (k, _) in enumerate(kinds)]
    batch, sms = solve_batch(ws, opt, no_lat_fuse=True)
    assert len(batch) == n
    return n, ref, batch, sms


@pytest.mark.parametrize("where", ["first", "last"])
def test_window_of_several_landmark_blocks_at_either_end_equals_single_bitwise(where):
    """The two-block window opens the batch (its blocks are records 0 and 1) or closes it (the deferred per-landmark loads of its short
    last block end at the end of lm_g / lm_Einv / lm_obs0)."""
    n, ref, batch, sms = run_case({(0 if where == "first" else -1): ("big", big())})
    for i in range(n):
        assert_window_equal(i, ref[i], batch[i], sms[i])
    assert min(sm.num_iterations for sm in sms) > 1


def test_constant_pose_and_landmark_in_a_window_of_several_blocks_equals_single_bitwise():
    """A constant pose (lp < 0 on its observations) and a constant landmark that is observed (loc < 0 on its observations, lloc < 0
    on its own lane: nothing written for it), in the two-block window, which ends the batch; a healthy one opens it."""
    wc = with_constant_pose_and_landmark(big())
    K, pi = wc.meta["K"], wc.a["proj_idx"]
    assert wc.a["is_const"][2] == 1 and wc.a["is_const"][(K + 1) + K + 3] == 1
    assert (pi[:, 2] == 3).sum() >= 2 and (pi[:, 0] == 2).sum() >= 2          # both constants are observed
    assert len(landmark_blocks(wc)) == 2
    n, ref, batch, sms = run_case({0: ("big", big()), -1: ("big const", wc)})
    for i in range(n):
        assert_window_equal(i, ref[i], batch[i], sms[i])
    assert np.array_equal(batch[n - 1].a["lm"][3], wc.a["lm"][3])              # the constant landmark stayed where it was
    assert min(sm.num_iterations for sm in sms) > 1


def test_nan_pose_in_a_window_of_several_blocks_leaves_its_landmarks_and_the_neighbours_alone():
    """A NaN in one pose of a two-block window between healthy windows (a two-block one in front, fillers behind): the failed window's
    landmarks stay unwritten (the CPU oracle leaves them so too), the neighbours end on their single solves' bytes."""
    wn = big(1303)
    wn.a["pose"].reshape(-1, 7)[1, 0] = np.nan
    n, ref, batch, sms = run_case({1: ("big", big()), 2: ("big nan", wn), -1: ("big", big())})
    for i in range(n):
        if i == 2:
            continue
        assert_window_equal(i, ref[i], batch[i], sms[i])
        assert sms[i].num_iterations > 1 and np.all(np.isfinite(batch[i].a["lm"]))
    assert np.array_equal(batch[2].a["lm"], wn.a["lm"]) and np.array_equal(ref[2][0].a["lm"], wn.a["lm"])
    assert sms[2].num_iterations == ref[2][1] and sms[2].termination == ref[2][4]


def test_windows_that_finish_early_at_both_ends_equal_single_bitwise():
    """A window that starts at the truth converges after 17 of 20 iterations, and so does the two-block window with a constant pose and
    landmark (the CPU oracle: 17 against the 20 of the plain two-block window and of every filler).  They open and close the batch:
    their gates are closed while their blocks' loads run, next to windows that go on."""
    still = synth.make_window(2, seed=706, perturb=False)
    wc = with_constant_pose_and_landmark(big())
    n, ref, batch, sms = run_case({0: ("still", still), 1: ("big", big()), -2: ("big const", wc), -1: ("still", still.copy())}, its=20)
    for i in range(n):
        assert_window_equal(i, ref[i], batch[i], sms[i])
    its = [sm.num_iterations for sm in sms]
    print("iterations per window:", its[:3], its[-3:])
    assert its[0] == its[-1] and max(its[0], its[-2]) < min(its[1:-2]), (its[:3], its[-3:])   # the case is a case
