"""Batched pyramidal Lucas-Kanade tracking on the device (swf_klt_track_batch) against the float64 referee of
tests/np_klt.py.  Every sum of the operator is a sum of integers and everything else a fixed sequence of double operations, so every
comparison here is bitwise and no point, pair or output is left out: pyr, cur_px, back_px, status, why, trace_iters, trace_px,
keep_idx, n_keep and info.  The cases are those of tests/klt_cases.py; tests/test_klt.py checks on the CPU that they reach every
`why` code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import klt_cases as kc
import np_klt as nk
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
ISENT = -7
PYR_FILL = 0xA5
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pb = C.POINTER(C.c_uint8)
POINT_KEYS = ("cur_px", "back_px", "status", "why", "keep_idx", "trace_iters", "trace_px")
OUT_ORDER = ("cur_px", "back_px", "status", "why", "keep_idx", "n_keep", "info", "trace_iters", "trace_px", "pyr")
KIND = dict(cur_px=pd, back_px=pd, status=pb, why=pi, keep_idx=pi, n_keep=pi, info=pi, trace_iters=pi, trace_px=pd, pyr=pb)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run(cases, flags=None):
    """one host-memory call through solver.klt_track_batch for cases that agree on the image size and the arguments"""
    a = dict(cases[0]["args"])
    assert all(c["args"] == a and c["prev"].shape == cases[0]["prev"].shape for c in cases)
    if flags is not None:
        a["flags"] = flags
    guess = [c["guess"] for c in cases] if a["flags"] & 2 else None
    return solver.klt_track_batch(np.stack([c["prev"] for c in cases]), np.stack([c["cur"] for c in cases]), [c["pts"] for c in cases], guess,
                                  fill=SENTINEL, stages=True, **a)


def pair_of(res, k):
    """everything pair k owns in a result"""
    lo, hi = int(res["first"][k]), int(res["first"][k + 1])
    out = {key: res[key][lo:hi] for key in POINT_KEYS}
    out.update(n_keep=int(res["n_keep"][k]), info=int(res["info"][k]), pyr=res["pyr"][k])
    return out


def same_bits(a, b, keys=POINT_KEYS + ("n_keep", "info", "pyr")):
    return [k for k in keys if not np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k])))]


def check(got, ref, what, back=True, pyr_fill=0):
    """a pair of a result against the referee's: every output, bit for bit"""
    assert got["info"] == ref["info"], what
    if ref["info"] != nk.OK:                          # the pair wrote its info only
        assert got["n_keep"] == ISENT and (got["status"] == 255).all() and (got["cur_px"] == SENTINEL).all() and (got["why"] == ISENT).all()
        assert (got["keep_idx"] == ISENT).all() and (got["trace_iters"] == ISENT).all() and (got["trace_px"] == SENTINEL).all(), what
        return
    keys = tuple(k for k in POINT_KEYS if back or k != "back_px") + ("n_keep", "pyr")
    bad = same_bits(got, ref, keys)
    assert not bad, (what, bad)
    if not back:
        assert (got["back_px"] == SENTINEL).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_pyramids_equal_the_referee(k):
    c, ref = kc.pyramid_cases()[k], kc.referee("pyramid")[k]
    got = pair_of(run([c]), 0)
    assert got["pyr"].size == nk.pyramid_bytes(c["prev"].shape[0], c["prev"].shape[1], c["args"]["max_level"]) > 0
    check(got, ref, c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["truth", "count"])
@pytest.mark.parametrize("flags", [5, 4])
def test_truth_and_point_counts_bitwise(group, flags):
    """the four truth cases and 1, 63, 65 and 257 points, with flag bit 0 both ways"""
    cases = kc.truth_cases() if group == "truth" else kc.count_cases()
    for c, ref in zip(cases, kc.referee(group, flags)):
        check(pair_of(run([c], flags), 0), ref, (c["name"], flags))
        if group == "truth":
            assert ref["n_keep"] == 64


@pytest.mark.gpu
def test_edges_bitwise():
    """start points on, near and outside the border, a flow that leaves the image or ends on the border rows, flat patches, an unrelated
    second image"""
    seen = set()
    for c, ref in zip(kc.edge_cases(), kc.referee("edge")):
        check(pair_of(run([c]), 0), ref, c["name"])
        seen |= set(ref["why"].tolist())
    assert seen == set(range(7))


@pytest.mark.gpu
def test_options_bitwise():
    """the prediction branch, no reverse pass, win 5 and 11, one iteration, back_level 0 and a back_level above max_level"""
    for c, ref in zip(kc.option_cases(), kc.referee("option")):
        check(pair_of(run([c]), 0), ref, c["name"], back=bool(c["args"]["flags"] & 4))


def _hip(call, *args):
    rc = getattr(solver.lib(), call)(*args)
    assert rc == 0, (call, rc)


class DeviceArrays:
    def __init__(self):
        self.bufs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = C.c_void_p()
        _hip("hipMalloc", C.byref(d), C.c_size_t(max(a.nbytes, 8)))
        self.bufs.append(d)
        if a.nbytes:
            _hip("hipMemcpy", d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1))
        return d

    def down(self, d, a):
        if a.nbytes:
            _hip("hipMemcpy", C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), C.c_int(2))

    def free(self):
        for d in self.bufs:
            solver.lib().hipFree(d)


def _arrays(cases):
    a = cases[0]["args"]
    n = len(cases)
    first = np.concatenate([[0], np.cumsum([c["pts"].shape[0] for c in cases])]).astype(np.int32)
    tot = int(first[-1])
    rows, cols = cases[0]["prev"].shape
    nb = nk.pyramid_bytes(rows, cols, max(a["max_level"], a["back_level"]))
    ins = dict(prev=np.stack([c["prev"] for c in cases]), cur=np.stack([c["cur"] for c in cases]), first=first,
               pts=np.concatenate([c["pts"] for c in cases] + [np.zeros((0, 2))]))
    out = dict(cur_px=np.full((tot, 2), SENTINEL), back_px=np.full((tot, 2), SENTINEL), status=np.full(tot, 255, np.uint8),
               why=np.full(tot, ISENT, np.int32), keep_idx=np.full(tot, ISENT, np.int32), n_keep=np.full(n, ISENT, np.int32),
               info=np.full(n, -9, np.int32), trace_iters=np.full((tot, 2, 5), ISENT, np.int32), trace_px=np.full((tot, 2, 5, 2), SENTINEL),
               pyr=np.full((n, nb), PYR_FILL, np.uint8))
    return a, n, rows, cols, ins, out


def _call(a, n, rows, cols, p, o, on_device):
    return solver.lib().swf_klt_track_batch(C.c_int32(n), C.c_int32(rows), C.c_int32(cols), p["prev"], p["cur"], p["first"], p["pts"], None,
                                            C.c_int32(a["win"]), C.c_int32(a["max_level"]), C.c_int32(a["back_level"]), C.c_int32(a["max_count"]),
                                            C.c_double(a["eps"]), C.c_double(a["min_eig"]), C.c_double(a["back_dist"]), C.c_int32(a["flags"]),
                                            *[o[k] for k in OUT_ORDER], C.c_int32(on_device), None)


def _split(out, n):
    res = dict(out)
    return [pair_of(res, k) for k in range(n)]


def device_memory_call(cases):
    """on_device = 1 over hipMalloc'ed buffers pre-filled with sentinels; returns the per-pair dicts"""
    a, n, rows, cols, ins, out = _arrays(cases)
    D = DeviceArrays()
    try:
        p = dict(prev=C.cast(D.up(ins["prev"]), pb), cur=C.cast(D.up(ins["cur"]), pb), first=C.cast(D.up(ins["first"]), pi), pts=C.cast(D.up(ins["pts"]), pd))
        d = {k: D.up(v) for k, v in out.items()}
        rc = _call(a, n, rows, cols, p, {k: C.cast(d[k], KIND[k]) for k in OUT_ORDER}, 1)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in out.items():
            D.down(d[k], v)
    finally:
        D.free()
    out["first"] = ins["first"]
    return _split(out, n)


def host_memory_call(cases, drop=None):
    """the raw C call on host memory with every output pre-filled; `drop` names an output passed as null"""
    a, n, rows, cols, ins, out = _arrays(cases)
    p = dict(prev=ins["prev"].ctypes.data_as(pb), cur=ins["cur"].ctypes.data_as(pb), first=ins["first"].ctypes.data_as(pi),
             pts=np.ascontiguousarray(np.concatenate([ins["pts"], np.zeros((1, 2))])).ctypes.data_as(pd))
    rc = _call(a, n, rows, cols, p, {k: None if k == drop else out[k].ctypes.data_as(KIND[k]) for k in OUT_ORDER}, 0)
    assert rc == 0, solver.lib().swf_last_error()
    out["first"] = ins["first"]
    return out, _split(out, n)


@pytest.mark.gpu
def test_ragged_call_alone_again_host_and_device_memory():
    """nine pairs of 0 to 130 points with a BAD_INPUT pair in one call: equal to the referee, to the same call again, to every pair run
    alone and to the call on device memory; what the failed pair does not write keeps its sentinel there too"""
    cases, refs = kc.ragged_cases(), kc.referee("ragged")
    assert [c["pts"].shape[0] for c in cases] == [0, 1, 7, 64, 9, 65, 130, 3, 64] and [r["info"] for r in refs].count(nk.BAD_INPUT) == 1
    full, again = run(cases), run(cases)
    dev = device_memory_call(cases)
    for k, (c, ref) in enumerate(zip(cases, refs)):
        got = pair_of(full, k)
        check(got, ref, c["name"])
        assert not same_bits(pair_of(again, k), got), k
        own = POINT_KEYS + ("n_keep", "info") + (("pyr",) if c["pts"].shape[0] else ())      # a call without a point does not touch the device
        assert not same_bits(pair_of(run([c]), 0), got, own), k
        alone = device_memory_call([c])[0]
        for d in (dev[k], alone):
            if ref["info"] == nk.OK:                  # device memory: the levels that are not built keep the fill, as in the referee
                assert not same_bits(d, kc.referee_of(c, pyr_fill=PYR_FILL)), k
            else:                                     # the pyramid is a workspace and written for every pair; nothing else is
                assert d["info"] == nk.BAD_INPUT and not same_bits(d, got, POINT_KEYS + ("n_keep",)), k


@pytest.mark.gpu
def test_outputs_may_be_null():
    """every output but info null in turn: the others do not change"""
    cases = kc.ragged_cases()[3:6]
    full, _ = host_memory_call(cases)
    for drop in OUT_ORDER:
        if drop == "info":
            continue
        out, _ = host_memory_call(cases, drop=drop)
        for k in OUT_ORDER:
            if k == drop:
                assert (out[k] == (PYR_FILL if k == "pyr" else 255 if k == "status" else ISENT if out[k].dtype == np.int32 else SENTINEL)).all(), (drop, k)
            else:
                assert np.array_equal(bits(out[k]), bits(full[k])), (drop, k)


@pytest.mark.gpu
def test_chained_with_track_reject_on_device_memory():
    """cur_px, prev_px and keep_idx stay on the device: the kept tracks gathered there and handed to swf_track_reject_batch give the same
    bits as the same chain through host memory"""
    c = kc.truth_cases()[1]
    n = c["pts"].shape[0]
    a = c["args"]
    host = pair_of(run([c]), 0)
    keep = host["keep_idx"][:host["n_keep"]]
    assert keep.size >= 8
    cam = np.array([100.0, 100.0, 64.0, 48.0, -0.1, 0.01, 0.001, 0.001, 0, 0, 0, 0])
    trk = dict(col=128, row=96, focal=100.0, iterations=64, threshold=1.0, confidence=0.99, seed=3, flags=1)
    via_host = solver.track_reject_batch([host["cur_px"][keep]], [c["pts"][keep]], cam, [0.05], fill=SENTINEL, **trk)
    D = DeviceArrays()
    try:
        d_prev, d_cur, d_first, d_pts = D.up(c["prev"]), D.up(c["cur"]), D.up(np.array([0, n], np.int32)), D.up(c["pts"])
        d_cpx, d_keep, d_int = D.up(np.zeros((n, 2))), D.up(np.full(n, -5, np.int32)), D.up(np.zeros(2, np.int32))
        d_pyr = D.up(np.zeros(nk.pyramid_bytes(96, 128, 3), np.uint8))
        rc = solver.lib().swf_klt_track_batch(C.c_int32(1), C.c_int32(96), C.c_int32(128), C.cast(d_prev, pb), C.cast(d_cur, pb), C.cast(d_first, pi),
                                              C.cast(d_pts, pd), None, C.c_int32(a["win"]), C.c_int32(a["max_level"]), C.c_int32(a["back_level"]),
                                              C.c_int32(a["max_count"]), C.c_double(a["eps"]), C.c_double(a["min_eig"]), C.c_double(a["back_dist"]),
                                              C.c_int32(a["flags"]), C.cast(d_cpx, pd), None, None, None, C.cast(d_keep, pi), C.cast(d_int, pi),
                                              C.cast(C.c_void_p(d_int.value + 4), pi), None, None, C.cast(d_pyr, pb), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        got_keep, got_int = np.zeros(n, np.int32), np.zeros(2, np.int32)
        D.down(d_keep, got_keep); D.down(d_int, got_int)
        assert got_int[1] == nk.OK and got_int[0] == keep.size and np.array_equal(got_keep, host["keep_idx"])
        m = keep.size
        d_c2, d_p2 = D.up(np.zeros((m, 2))), D.up(np.zeros((m, 2)))
        for j, i in enumerate(keep):                  # the gather: 16 bytes per kept track, device to device
            _hip("hipMemcpy", C.c_void_p(d_c2.value + 16 * j), C.c_void_p(d_cpx.value + 16 * int(i)), C.c_size_t(16), C.c_int(3))
            _hip("hipMemcpy", C.c_void_p(d_p2.value + 16 * j), C.c_void_p(d_pts.value + 16 * int(i)), C.c_size_t(16), C.c_int(3))
        d_f2, d_dt, d_st, d_F, d_i2 = D.up(np.array([0, m], np.int32)), D.up(np.array([0.05])), D.up(np.zeros(m, np.uint8)), D.up(np.zeros(9)), D.up(np.zeros(4, np.int32))
        at = lambda d, off: C.cast(C.c_void_p(d.value + off), pi)
        rc = solver.lib().swf_track_reject_batch(C.c_int32(1), C.cast(d_f2, pi), C.cast(d_c2, pd), C.cast(d_p2, pd), (C.c_double * 12)(*cam), C.c_int32(128),
                                                 C.c_int32(96), C.c_double(100.0), C.cast(d_dt, pd), C.c_int32(64), C.c_double(1.0), C.c_double(0.99),
                                                 C.c_uint64(3), C.c_int32(1), C.cast(d_st, pb), None, at(d_i2, 0), at(d_i2, 4), at(d_i2, 8), at(d_i2, 12),
                                                 C.cast(d_F, pd), None, None, None, None, None, None, C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        st, F, i2 = np.zeros(m, np.uint8), np.zeros(9), np.zeros(4, np.int32)
        D.down(d_st, st); D.down(d_F, F); D.down(d_i2, i2)
    finally:
        D.free()
    assert i2[3] == via_host["info"][0]
    if i2[3] == 0:
        assert np.array_equal(st, via_host["status"]) and np.array_equal(bits(F), bits(via_host["F"][0]))
        assert (i2[0], i2[1], i2[2]) == (via_host["n_inliers"][0], via_host["best"][0], via_host["n_iters"][0])


@pytest.mark.gpu
def test_klt_adapter_runs(tmp_path):
    exe = compile_shim(tmp_path, "shim_klt")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "klt ok" in out.stdout, out.stdout
