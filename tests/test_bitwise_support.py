"""tests/bitwise.py on the CPU: what assert_same_bytes lets through and what it does not, what with_constant changes and what it
leaves alone, and the list of environment knobs against the library's source."""
import glob
import os
import re

import numpy as np
import pytest

import bitwise
from rtk_visual_inertial_navigation_amd import synth
from rtk_visual_inertial_navigation_amd.ordering import my_ordering

CSRC = os.path.join(bitwise.ROOT, "rtk_visual_inertial_navigation_amd", "csrc")


def _nan(payload):
    return np.array([0x7ff8000000000000 | payload], np.uint64).view(np.float64)


def _fails(a, b, **kw):
    with pytest.raises(AssertionError):
        bitwise.assert_same_bytes(a, b, **kw)
    return True


def test_assert_same_bytes_passes_on_equal_dicts():
    a = {"x": np.arange(6.0).reshape(2, 3), "n": np.array(3), "f": np.array([True, False])}
    bitwise.assert_same_bytes(a, {k: v.copy() for k, v in a.items()})
    bitwise.assert_same_bytes(a, {k: v.copy() for k, v in a.items()}, nan_equal=False)


def test_assert_same_bytes_tells_the_zeros_apart():
    a, b = {"x": np.array([1.0, 0.0])}, {"x": np.array([1.0, -0.0])}
    assert np.array_equal(a["x"], b["x"])                       # the comparison that lets it through
    assert _fails(a, b) and _fails(a, b, nan_equal=False)


def test_assert_same_bytes_fails_on_dtype_shape_and_key_set():
    a = {"x": np.zeros(4, np.int32), "y": np.zeros(2)}
    assert _fails(a, {"x": np.zeros(2, np.int64), "y": np.zeros(2)})          # the same 16 zero bytes under another dtype
    assert _fails(a, {"x": np.zeros((2, 2), np.int32), "y": np.zeros(2)})
    assert _fails(a, {"x": np.zeros(4, np.int32)})
    assert _fails(a, dict(a, z=np.zeros(1)))
    assert _fails(a, {"x": np.zeros(4, np.int32)}, keys=["x"])               # the key sets are compared whatever `keys` says


def test_assert_same_bytes_and_nans():
    a, same, other = {"x": _nan(0)}, {"x": _nan(0)}, {"x": _nan(1)}
    bitwise.assert_same_bytes(a, same)
    assert _fails(a, same, nan_equal=False)
    assert _fails(a, other) and _fails(a, other, nan_equal=False)


def test_assert_same_bytes_honours_keys():
    a, b = {"x": np.array([1.0]), "y": np.array([2.0])}, {"x": np.array([1.0]), "y": np.array([3.0])}
    assert _fails(a, b)
    bitwise.assert_same_bytes(a, b, keys=["x"])
    assert _fails(a, b, keys=["y"])


def test_with_constant_edits_the_flags_and_the_ordering_and_nothing_else():
    w = synth.make_window(3, K=4, F=6, S=2, seed=1151)
    before = w.copy()
    ids = [2, w.bid_lm(3)]
    assert not w.a["is_const"][ids].any()
    c = bitwise.with_constant(w, ids)
    # the input is unchanged
    assert sorted(w.a) == sorted(before.a) and all(w.a[k].tobytes() == before.a[k].tobytes() for k in w.a)
    assert w.n_tail == before.n_tail and w.meta["roles"] == before.meta["roles"]
    # is_const is set at exactly those ids
    assert np.array_equal(np.nonzero(c.a["is_const"] != w.a["is_const"])[0], sorted(ids)) and c.a["is_const"][ids].all()
    assert c.a["is_const"].dtype == np.uint8
    # the ordering is the one my_ordering issues for the new flags
    o_b, o_g, nt = my_ordering(w.meta["roles"], c.a["is_const"])
    assert np.array_equal(c.a["order_block"], o_b) and np.array_equal(c.a["order_group"], o_g) and c.n_tail == int(nt)
    assert not set(ids) & set(c.a["order_block"].tolist()) and c.a["order_block"].size == w.a["order_block"].size - 2
    # every other array is byte-equal to the input's
    assert sorted(c.a) == sorted(w.a)
    for k in w.a:
        if k not in ("is_const", "order_block", "order_group"):
            assert c.a[k].dtype == w.a[k].dtype and c.a[k].tobytes() == w.a[k].tobytes(), k
    assert bitwise.with_constant_pose_and_landmark(w).a["is_const"].tobytes() == c.a["is_const"].tobytes()


def test_scrub_list_is_every_knob_the_library_reads():
    """Every "SWF_..." string literal of a csrc/ file that calls getenv is the name of a knob (some reach getenv through a helper
    that takes the name), and every direct getenv("SWF_...") is among them."""
    names, direct = set(), set()
    files = [f for ext in ("hip", "cpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext))]
    assert len(files) > 10
    for f in files:
        src = open(f).read()
        if "getenv" in src:
            names |= set(re.findall(r'"(SWF_[A-Z0-9_]+)"', src))
            direct |= set(re.findall(r'getenv\(\s*"(SWF_[A-Z0-9_]+)"', src))
    assert len(direct) >= 11 and direct <= names
    assert len(bitwise.ENV_KNOBS) == len(set(bitwise.ENV_KNOBS))
    assert set(bitwise.ENV_KNOBS) == names, sorted(names ^ set(bitwise.ENV_KNOBS))
