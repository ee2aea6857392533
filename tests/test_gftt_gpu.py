"""Batched corner detection on the device (swf_gftt_detect_batch) against the float64 / int64 referee of tests/np_gftt.py.
Everything up to D is integer arithmetic and the rest a fixed sequence of double operations, so every comparison here is bitwise and no
frame, point or output is left out: eig, order, why, n_old, new_px up to n_new, n_new, n_cand, max_eig, pack_first, pack_px, pack_src
and info.  The cases are those of tests/gftt_cases.py; tests/test_gftt.py checks on the CPU that they reach every code and branch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gftt_cases as gc
import klt_cases as kc
import np_gftt as ng
import np_klt as nk
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import solver

SENTINEL = -7.0
ISENT = -7
WORK_FILL = 0xA5
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pb = C.POINTER(C.c_uint8)
OUT_ORDER = ("order", "why", "n_old", "new_px", "n_new", "n_cand", "max_eig", "pack_first", "pack_px", "pack_src", "info", "work")
KIND = dict(order=pi, why=pi, n_old=pi, new_px=pd, n_new=pi, n_cand=pi, max_eig=pd, pack_first=pi, pack_px=pd, pack_src=pi, info=pi, work=pb)
FRAME_KEYS = ("order", "why", "n_old", "new_px", "n_new", "n_cand", "max_eig", "eig", "info")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def call_args(cases):
    a = dict(cases[0]["args"])
    assert all(c["args"] == a and c["img"].shape == cases[0]["img"].shape and (c["mask"] is None) == (cases[0]["mask"] is None) for c in cases)
    return a


def run(cases):
    """one host-memory call through solver.gftt_detect_batch for cases that agree on the image size and the arguments"""
    a = call_args(cases)
    mask = None if cases[0]["mask"] is None else np.stack([c["mask"] for c in cases])
    return solver.gftt_detect_batch(np.stack([c["img"] for c in cases]), [c["px"] for c in cases], [c["tc"] for c in cases], mask=mask,
                                    fill=SENTINEL, stages=True, **a)


def frame_of(res, k):
    """everything frame k owns in a result"""
    lo, hi = int(res["first"][k]), int(res["first"][k + 1])
    out = dict(order=res["order"][lo:hi], why=res["why"][lo:hi], new_px=res["new_px"][k], eig=res["eig"][k])
    out.update({key: res[key][k] for key in ("n_old", "n_new", "n_cand", "max_eig", "info")})
    return out


def check(got, ref, what, eig_fill=None):
    """a frame of a result against the referee's: every output, bit for bit; what the frame must not write keeps its sentinel"""
    unwritten_eig = np.full(got["eig"].shape, SENTINEL) if eig_fill is None else eig_fill
    assert got["info"] == ref["info"], what
    if ref["info"] != ng.OK:
        assert got["n_cand"] == (ref["n_cand"] if ref["info"] == ng.TOO_MANY else ISENT), what
        assert got["n_old"] == ISENT and got["n_new"] == ISENT and same(got["max_eig"], np.float64(SENTINEL)), what
        assert (got["order"] == ISENT).all() and (got["why"] == ISENT).all() and (got["new_px"] == SENTINEL).all(), what
        return                  # eig is workspace: a TOO_MANY frame has been through stage B
    n = ref["n_new"]
    for key in ("order", "why", "n_old", "n_new", "n_cand", "max_eig"):
        assert same(got[key], ref[key]), (what, key, got[key], ref[key])
    assert same(got["new_px"][:n], ref["new_px"]) and (got["new_px"][n:] == SENTINEL).all(), (what, "new_px")
    assert same(got["eig"], unwritten_eig if ref["eig"] is None else ref["eig"]), (what, "eig")


def check_pack(res, refs, what):
    if all(r["info"] == ng.BAD_INPUT for r in refs):     # the device is not touched: nothing but info is written
        assert (res["pack_first"] == ISENT).all() and res["pack_px"].size == 0 and res["pack_src"].size == 0, what
        return
    first, px, src = ng.pack(refs)
    assert same(res["pack_first"], first) and same(res["pack_px"], px) and same(res["pack_src"], src), what


def check_group(group, names=None):
    cases = dict(image=gc.image_cases, point=gc.point_cases, option=gc.option_cases)[group]()
    for c, ref in zip(cases, gc.referee(group)):
        if names is None or c["name"] in names:
            res = run([c])
            check(frame_of(res, 0), ref, c["name"])
            check_pack(res, [ref], c["name"])


IMAGE_NAMES = [c["name"] for c in gc.image_cases()]
POINT_NAMES = [c["name"] for c in gc.point_cases()]
OPTION_NAMES = [c["name"] for c in gc.option_cases()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_image_case_bitwise(name):
    check_group("image", {name})


@pytest.mark.gpu
@pytest.mark.parametrize("name", POINT_NAMES)
def test_tracked_point_case_bitwise(name):
    check_group("point", {name})


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPTION_NAMES)
def test_option_case_bitwise(name):
    check_group("option", {name})


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
    a = call_args(cases)
    n = len(cases)
    rows, cols = cases[0]["img"].shape
    first = np.concatenate([[0], np.cumsum([c["px"].shape[0] for c in cases])]).astype(np.int32)
    tot, mc = int(first[-1]), a["max_cnt"]
    wb = solver.gftt_workspace_bytes(rows, cols, a["cand_cap"])
    assert wb >= rows * cols * 8 and wb % 16 == 0
    ins = dict(img=np.stack([c["img"] for c in cases]), mask=None if cases[0]["mask"] is None else np.stack([c["mask"] for c in cases]), first=first,
               px=np.concatenate([c["px"] for c in cases] + [np.zeros((1, 2))]), tc=np.concatenate([c["tc"] for c in cases] + [np.zeros(1, np.int32)]).astype(np.int32),
               hw=None if a["disc_halfwidth"] is None else np.asarray(a["disc_halfwidth"], np.int32))
    out = dict(order=np.full(tot + 1, ISENT, np.int32), why=np.full(tot + 1, ISENT, np.int32), n_old=np.full(n, ISENT, np.int32),
               new_px=np.full((n, mc, 2), SENTINEL), n_new=np.full(n, ISENT, np.int32), n_cand=np.full(n, ISENT, np.int32), max_eig=np.full(n, SENTINEL),
               pack_first=np.full(n + 1, ISENT, np.int32), pack_px=np.full((tot + n * mc + 1, 2), SENTINEL), pack_src=np.full(tot + n * mc + 1, ISENT, np.int32),
               info=np.full(n, -9, np.int32), work=np.full((n, wb), WORK_FILL, np.uint8))
    return a, n, rows, cols, ins, out


def _call(a, n, rows, cols, p, o, on_device):
    return solver.lib().swf_gftt_detect_batch(C.c_int32(n), C.c_int32(rows), C.c_int32(cols), p["img"], p["mask"], p["first"], p["px"], p["tc"],
                                              C.c_int32(a["max_cnt"]), C.c_int32(a["min_dist"]), C.c_double(a["quality"]), p["hw"], C.c_int32(a["cand_cap"]),
                                              C.c_int32(a["flags"]), *[o[k] for k in OUT_ORDER], C.c_int32(on_device), None)


def _finish(out, ins, n, rows, cols):
    out["first"] = ins["first"]
    out["eig"] = np.ascontiguousarray(out["work"][:, :rows * cols * 8]).view(np.float64).reshape(n, rows, cols)
    return out


def device_memory_call(cases):
    """on_device = 1 over hipMalloc'ed buffers pre-filled with sentinels; returns the outputs as arrays"""
    a, n, rows, cols, ins, out = _arrays(cases)
    D = DeviceArrays()
    try:
        kinds = dict(img=pb, mask=pb, first=pi, px=pd, tc=pi, hw=pi)
        p = {k: None if v is None else C.cast(D.up(v), kinds[k]) for k, v in ins.items()}
        d = {k: D.up(v) for k, v in out.items()}
        rc = _call(a, n, rows, cols, p, {k: C.cast(d[k], KIND[k]) for k in OUT_ORDER}, 1)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in out.items():
            D.down(d[k], v)
    finally:
        D.free()
    return _finish(out, ins, n, rows, cols)


def host_memory_call(cases, drop=None):
    """the raw C call on host memory with every output pre-filled; `drop` names an output passed as null"""
    a, n, rows, cols, ins, out = _arrays(cases)
    kinds = dict(img=pb, mask=pb, first=pi, px=pd, tc=pi, hw=pi)
    p = {k: None if v is None else v.ctypes.data_as(kinds[k]) for k, v in ins.items()}
    rc = _call(a, n, rows, cols, p, {k: None if k == drop else out[k].ctypes.data_as(KIND[k]) for k in OUT_ORDER}, 0)
    assert rc == 0, solver.lib().swf_last_error()
    return _finish(out, ins, n, rows, cols)


def frames_equal(a, b, keys=FRAME_KEYS):
    return [k for k in keys if not same(a[k], b[k])]


@pytest.mark.gpu
def test_ragged_call_alone_again_host_and_device_memory():
    """nine frames in one call: equal to the referee, to the same call again, to every frame run alone and to the call on device
    memory; what a BAD_INPUT or a TOO_MANY frame must not write keeps its sentinel in all of them"""
    cases, refs = gc.ragged_cases(), gc.referee("ragged")
    assert sorted(r["info"] for r in refs) == [ng.OK] * 7 + [ng.BAD_INPUT, ng.TOO_MANY]
    full, again = run(cases), run(cases)
    check_pack(full, refs, "ragged")
    dev = device_memory_call(cases)
    fill_eig = np.ascontiguousarray(np.full(96 * 128 * 8, WORK_FILL, np.uint8)).view(np.float64).reshape(96, 128)
    first, px, src = ng.pack(refs)
    used = int(first[-1])
    assert same(dev["pack_first"], first) and same(dev["pack_px"][:used], px) and same(dev["pack_src"][:used], src)
    assert (dev["pack_px"][used:] == SENTINEL).all() and (dev["pack_src"][used:] == ISENT).all()
    for key in ("pack_first", "pack_px", "pack_src"):
        assert same(again[key], full[key]), key
    for k, (c, ref) in enumerate(zip(cases, refs)):
        got = frame_of(full, k)
        check(got, ref, c["name"])
        assert not frames_equal(frame_of(again, k), got), k
        alone = run([c])
        # through host memory the eig of a frame that is not OK is not copied back; alone, a BAD_INPUT frame does not reach the device
        assert not frames_equal(frame_of(alone, 0), got), k
        check_pack(alone, [ref], c["name"])
        d = frame_of(dev, k)
        if ref["info"] == ng.OK:
            check(d, ref, (c["name"], "device memory"), eig_fill=fill_eig)
        else:                                          # eig is workspace there: compare everything else
            assert not frames_equal(d, got, tuple(key for key in FRAME_KEYS if key != "eig")), k
        d1 = frame_of(device_memory_call([c]), 0)
        assert not frames_equal(d1, d, FRAME_KEYS if ref["info"] != ng.TOO_MANY else tuple(key for key in FRAME_KEYS if key != "eig")), k


@pytest.mark.gpu
def test_outputs_may_be_null():
    """every output but info null in turn, on host memory: the others do not change, and the dropped one is not touched"""
    cases = gc.ragged_cases()[1:6]
    full = host_memory_call(cases)
    for drop in OUT_ORDER:
        if drop == "info":
            continue
        out = host_memory_call(cases, drop=drop)
        for k in OUT_ORDER:
            if k == drop:
                want = WORK_FILL if k == "work" else ISENT if out[k].dtype == np.int32 else SENTINEL
                assert (out[k] == want).all(), (drop, k)
            elif k != "work":
                assert same(out[k], full[k]), (drop, k)
        if drop != "work":
            assert same(out["eig"], full["eig"]), drop


@pytest.mark.gpu
def test_outputs_may_be_null_in_device_memory():
    """everything but info and the workspace null at once on device memory: info and eig are those of the full call"""
    cases = gc.ragged_cases()[1:6]
    full = device_memory_call(cases)
    a, n, rows, cols, ins, out = _arrays(cases)
    D = DeviceArrays()
    try:
        kinds = dict(img=pb, mask=pb, first=pi, px=pd, tc=pi, hw=pi)
        p = {k: None if v is None else C.cast(D.up(v), kinds[k]) for k, v in ins.items()}
        d_info, d_work = D.up(out["info"]), D.up(out["work"])
        o = {k: None for k in OUT_ORDER}
        o.update(info=C.cast(d_info, pi), work=C.cast(d_work, pb))
        rc = _call(a, n, rows, cols, p, o, 1)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        D.down(d_info, out["info"]); D.down(d_work, out["work"])
    finally:
        D.free()
    got = _finish(out, ins, n, rows, cols)
    assert same(got["info"], full["info"]) and same(got["eig"], full["eig"])


@pytest.mark.gpu
def test_chained_with_klt_on_device_memory():
    """pack_first and pack_px of a detection on frame A stay on the device and are the first / prev_px of swf_klt_track_batch for
    A -> B: the same bits as the same chain through host memory"""
    c = kc.truth_cases()[1]                             # 96 x 128, known flow
    ka = c["args"]
    rows, cols = c["prev"].shape
    ga = dict(max_cnt=60, min_dist=10, quality=0.01, cand_cap=4096, flags=1)
    host = solver.gftt_detect_batch(c["prev"][None], [np.zeros((0, 2))], [np.zeros(0, np.int32)], **ga)
    m = int(host["pack_first"][1])
    assert host["info"][0] == ng.OK and m == host["n_new"][0] >= 20
    via_host = solver.klt_track_batch(c["prev"][None], c["cur"][None], [host["pack_px"]], **ka)
    wb = solver.gftt_workspace_bytes(rows, cols, ga["cand_cap"])
    D = DeviceArrays()
    try:
        d_prev, d_cur = D.up(c["prev"]), D.up(c["cur"])
        d_first, d_px, d_tc = D.up(np.zeros(2, np.int32)), D.up(np.zeros(2)), D.up(np.zeros(1, np.int32))
        d_pf, d_ppx, d_info, d_work = D.up(np.full(2, -5, np.int32)), D.up(np.zeros((ga["max_cnt"], 2))), D.up(np.full(1, -5, np.int32)), D.up(np.zeros(wb, np.uint8))
        rc = solver.lib().swf_gftt_detect_batch(C.c_int32(1), C.c_int32(rows), C.c_int32(cols), C.cast(d_prev, pb), None, C.cast(d_first, pi), C.cast(d_px, pd),
                                                C.cast(d_tc, pi), C.c_int32(ga["max_cnt"]), C.c_int32(ga["min_dist"]), C.c_double(ga["quality"]), None,
                                                C.c_int32(ga["cand_cap"]), C.c_int32(ga["flags"]), None, None, None, None, None, None, None,
                                                C.cast(d_pf, pi), C.cast(d_ppx, pd), None, C.cast(d_info, pi), C.cast(d_work, pb), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        d_cpx, d_st, d_kinfo = D.up(np.zeros((ga["max_cnt"], 2))), D.up(np.zeros(ga["max_cnt"], np.uint8)), D.up(np.full(1, -5, np.int32))
        d_pyr = D.up(np.zeros(nk.pyramid_bytes(rows, cols, max(ka["max_level"], ka["back_level"])), np.uint8))
        rc = solver.lib().swf_klt_track_batch(C.c_int32(1), C.c_int32(rows), C.c_int32(cols), C.cast(d_prev, pb), C.cast(d_cur, pb), C.cast(d_pf, pi),
                                              C.cast(d_ppx, pd), None, C.c_int32(ka["win"]), C.c_int32(ka["max_level"]), C.c_int32(ka["back_level"]),
                                              C.c_int32(ka["max_count"]), C.c_double(ka["eps"]), C.c_double(ka["min_eig"]), C.c_double(ka["back_dist"]),
                                              C.c_int32(ka["flags"]), C.cast(d_cpx, pd), None, C.cast(d_st, pb), None, None, None, C.cast(d_kinfo, pi), None, None,
                                              C.cast(d_pyr, pb), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        pf, info, kinfo = np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        cpx, st = np.zeros((ga["max_cnt"], 2)), np.zeros(ga["max_cnt"], np.uint8)
        for dst, src in ((pf, d_pf), (info, d_info), (kinfo, d_kinfo), (cpx, d_cpx), (st, d_st)):
            D.down(src, dst)
    finally:
        D.free()
    assert pf.tolist() == [0, m] and info[0] == ng.OK and kinfo[0] == nk.OK == via_host["info"][0]
    assert same(cpx[:m], via_host["cur_px"]) and same(st[:m], via_host["status"]) and via_host["status"].sum() >= 10


@pytest.mark.gpu
def test_gftt_adapter_runs(tmp_path):
    exe = compile_shim(tmp_path, "shim_gftt")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "gftt ok" in out.stdout, out.stdout
