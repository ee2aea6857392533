"""Batched track outlier rejection on the device (swf_track_reject_batch) against the numpy referee of
tests/np_trackreject.py, stage by stage: each stage is checked against the referee fed with the device's own previous stage, so one
flipped decision can neither cascade into a false failure nor hide a real one.

  un_cur, un_prev    within M_LIFT x 2^-52 x the running sum of magnitudes of the longdouble lift (plus half a float ulp with flag bit 0)
  velocity           without the flag within M_LIFT x its bracket of the longdouble referee; with it, where every operation is exactly
                     rounded, equal to the recomputation from the device's own un_cur / un_prev
  samples            equal the referee's table, exactly
  hyp                unit Frobenius norm, sign by the largest entry: within M_HYP x 2^-52 kappa of the longdouble 8-point solves on the
                     same samples and the device's own virtual pixels, for the hypotheses with kappa <= 1e10 of the pairs with a translation
  count, status      recomputed in longdouble from the device's hyp: equal outside a relative margin of 1e-9 on d1, d2 against thr^2;
                     sure count <= count <= sure count + borderline points
  best, n_iters      equal a replay of the scan on the device's own count;  F equals hyp[best] bit for bit
  keep_idx           equals nonzero(status), -1 behind
  end to end         the decided pairs (trackreject_cases.undecided) equal the pure referee in info, best, n_iters, n_inliers and status

M_HYP = 43, M_LIFT = 3 are derived in tests/test_track_reject.py.  Every test prints the largest `deviation / bracket`.  Largest on
MI355X: hyp 8.52 (the 257-pair call; 3.33 on the end-to-end set, 1.76 on the truth pairs, 0.32 on the point counts), lift 0.258 (the
float64 referee's own figure: the lift is compiled without contraction and gives that referee's bits)."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import np_pnp as npp
import np_trackreject as npt
import pnp_gen as pg
import trackreject_cases as tc
import trackreject_gen as tg
from shim import compile_shim
from trackreject_cases import M_HYP, M_LIFT
from rtk_visual_inertial_navigation_amd import solver

SENTINEL = -7.0
MARGIN = 1e-9
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pb = C.POINTER(C.c_uint8)
PAIR_KEYS = ("n_inliers", "best", "n_iters", "info", "F", "samples", "hyp", "count")
POINT_KEYS = ("status", "keep_idx", "un_cur", "un_prev", "velocity")
LIFT_KEYS = ("un_cur", "un_prev", "velocity")


def _flag(pairs):
    """flag bit 0 and the camera are arguments of the call: its pairs agree on them"""
    assert len({p["flags"] for p in pairs}) == 1
    return pairs[0]["flags"]


def run(pairs, iterations=tg.ITERATIONS):
    return solver.track_reject_batch(*tg.pack(pairs), col=tg.COL, row=tg.ROW, focal=tg.FOCAL, iterations=iterations, threshold=tg.THRESHOLD,
                                     confidence=tg.CONFIDENCE, seed=tg.SEED, flags=_flag(pairs), fill=SENTINEL, stages=True)


def pair_of(res, k):
    """everything pair k owns in a result, as a dict of arrays"""
    lo, hi = int(res["first"][k]), int(res["first"][k + 1])
    out = {key: res[key][k] for key in PAIR_KEYS}
    out.update({key: res[key][lo:hi] for key in POINT_KEYS})
    return out


def run_mixed(pairs, iterations=tg.ITERATIONS):
    """pairs of both flag values go in two calls; returns the per-pair dicts in the pairs' order"""
    out = [None] * len(pairs)
    for fl in (0, 1):
        idx = [k for k, p in enumerate(pairs) if p["flags"] == fl]
        if idx:
            part = run([pairs[k] for k in idx], iterations)
            for j, k in enumerate(idx):
                out[k] = pair_of(part, j)
    return out


@functools.lru_cache(maxsize=None)
def device(which):
    pairs = tc.pairs_of(which)
    if which == "shape":
        return run_mixed(pairs)
    res = run(pairs, tc.TRUTH_ITERATIONS if which == "truth" else tg.ITERATIONS)
    return [pair_of(res, k) for k in range(len(pairs))]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return all(np.array_equal(bits(a[key]), bits(b[key])) for key in PAIR_KEYS + POINT_KEYS)


def untouched(d, keys):
    return all((d[key] == (255 if key == "status" else SENTINEL if d[key].dtype == np.float64 else int(SENTINEL))).all() for key in keys)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_lift(p, d, tag):
    """stage 1; returns (largest deviation / bracket, the device's virtual pixels [n][4] in float64)"""
    cur, prev = npt.stage_pixels(p["cur"], p["prev"], p["flags"])
    q = npt.lift_stage(cur, prev, p["cam"], p["dt"], tg.COL, tg.ROW, tg.FOCAL, p["flags"], np.longdouble)
    worst = 0.0
    for key, raw, e in (("un_cur", "raw_cur", "e_cur"), ("un_prev", "raw_prev", "e_prev")):
        dev = np.abs(d[key] - q[raw]).astype(np.float64)
        if p["flags"]:
            dev = np.maximum(dev - 0.5 * ulp32(d[key]), 0.0)
            assert np.array_equal(d[key], npt.f32(d[key])), tag
        ratio = float((dev / (tc.EPS * q[e])).max()) if dev.size else 0.0
        worst = max(worst, ratio)
        assert ratio <= M_LIFT, tag + (key, ratio)
    assert np.array_equal(bits(d["velocity"]), bits(np.asarray(npt.velocity_of(d["un_cur"], d["un_prev"], p["dt"], p["flags"]), np.float64))), tag
    if not p["flags"] and d["velocity"].size:
        ratio = float((np.abs(d["velocity"] - q["velocity"]).astype(np.float64) / (tc.EPS * q["e_vel"])).max())
        worst = max(worst, ratio)
        assert ratio <= M_LIFT, tag + ("velocity", ratio)
    if p["flags"]:                  # the unrounded lift is not exported: the float64 referee's, which the device's rounds to
        r = npt.lift_stage(cur, prev, p["cam"], p["dt"], tg.COL, tg.ROW, tg.FOCAL, 1)
        assert np.array_equal(r["un_cur"], d["un_cur"]) and np.array_equal(r["un_prev"], d["un_prev"]), tag
        virt = r["virt"]
    else:
        virt = npt.virtual_of(d["un_cur"], d["un_prev"], tg.COL, tg.ROW, tg.FOCAL, 0)
    return worst, virt


def check_stages(pairs, res, iterations, pure, label, longdouble=True):
    """the stage checks and the sentinel check for per-pair results; returns the largest deviation / bracket of hyp and of the lift"""
    worst_h = worst_l = 0.0
    decided = 0
    dtype = np.longdouble if longdouble else np.float64
    for k, (p, d) in enumerate(zip(pairs, res)):
        code = tc.expected_code(p)
        tag = (label, k, p["seed"])
        assert d["info"] == code, tag + (int(d["info"]),)
        if code == npt.BAD_INPUT:
            assert untouched(d, [key for key in PAIR_KEYS + POINT_KEYS if key != "info"]), tag
            continue
        wl, virt = check_lift(p, d, tag)
        worst_l = max(worst_l, wl)
        if code != npt.OK:
            assert untouched(d, [key for key in PAIR_KEYS + POINT_KEYS if key != "info" and key not in LIFT_KEYS]), tag
            continue
        n = p["n"]
        # the samples
        samples, _ = npt.sample_table(n, iterations, tg.SEED)
        H = samples.shape[0]
        assert np.array_equal(d["samples"][:H], samples), tag
        for key in ("samples", "hyp", "count"):                              # a pair of 8 points owns one row: the tail keeps the sentinel
            assert (d[key][H:] == int(SENTINEL)).all(), tag
        hyp, count = d["hyp"][:H], d["count"][:H]
        valid = np.isfinite(hyp).all(axis=1)
        assert (np.isnan(hyp).all(axis=1) == ~valid).all(), tag            # a row is whole or NaN
        # the 8-point solves
        if longdouble and p["motion"] != "rotation":
            ms = npt.minimal_solves(virt, samples, np.longdouble)
            use = ms["kappa"] <= tc.KAPPA_MAX
            assert valid[use].all(), tag
            if use.any():
                ratio = tc.hyp_deviation(hyp, ms["hyp"])[use] / npt.hyp_bracket(ms["kappa"])[use]
                worst_h = max(worst_h, float(ratio.max()))
                assert ratio.max() <= M_HYP, tag + (float(ratio.max()),)
        # the counts and the status, from the device's own hypotheses
        sc = npt.score(virt, hyp, tg.THRESHOLD, dtype)
        thr2 = sc["thr2"]
        with np.errstate(all="ignore"):
            near = lambda v: np.abs(v - thr2) <= MARGIN * thr2
            border = sc["valid"][:, None] & (near(sc["d1"]) | near(sc["d2"]))
        sure = (sc["mask"] & ~border).sum(axis=1)
        assert (count[~valid] == 0).all(), tag
        assert ((sure <= count) & (count <= sure + border.sum(axis=1))).all(), tag
        # the scan, on the device's own counts
        sn = npt.scan(count, n, iterations, tg.CONFIDENCE)
        assert (d["best"], d["n_iters"], d["n_inliers"]) == (sn["best"], sn["n_iters"], sn["best_count"]), tag
        b = sn["best"]
        status = d["status"]
        assert set(status.tolist()) <= {0, 1} and status.sum() == count[b], tag
        free = ~border[b]
        assert np.array_equal(status.astype(bool)[free], sc["mask"][b][free]), tag
        assert np.array_equal(bits(d["F"]), bits(hyp[b])), tag
        idx = np.flatnonzero(status)
        assert np.array_equal(d["keep_idx"][:idx.size], idx) and (d["keep_idx"][idx.size:] == -1).all(), tag
        # end to end against the pure referee, where no decision is within reach of rounding
        r = pure[k]
        if not tc.undecided(r, M_HYP):
            decided += 1
            assert (d["info"], d["best"], d["n_iters"], d["n_inliers"]) == (r["info"], r["best"], r["n_iters"], r["n_inliers"]), tag
            assert np.array_equal(status.astype(bool), r["status"]), tag
    print("%s: %d pairs (%d decided), deviation / bracket: hyp %.3f (M_HYP %.0f), lift %.4f (M_LIFT %.0f)" %
          (label, len(pairs), decided, worst_h, M_HYP, worst_l, M_LIFT))
    return worst_h, worst_l, decided


@pytest.mark.gpu
def test_point_counts_match_referee():
    """7, 8, 9, 63, 64, 65, 200 and 1024 points, flag bit 0 both ways (a call per flag value; the pairs without the flag see the camera
    with the rational terms), and each pair alone, bit for bit"""
    pairs = tc.shape_pairs()
    res = device("shape")
    check_stages(pairs, res, tg.ITERATIONS, tc.referee("shape"), "all point counts")
    for k, p in enumerate(pairs):
        one = run([p])
        assert same_bits(pair_of(one, 0), res[k]), (p["n"], p["flags"])


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", tc.ITERATIONS)
def test_iteration_counts(iterations):
    """1, 255, 256, 257 and 1000 hypotheses (one lane each, in chunks of 256) on 9, 65 and 200 points; at 1000 the scan replay and the
    status against a float64 recomputation only, no longdouble pass"""
    pairs = tc.iteration_pairs()
    full = run(pairs, iterations)
    res = [pair_of(full, k) for k in range(len(pairs))]
    long = iterations == tc.LONG_ITERATIONS
    pure = tc.referee_iterations(iterations)
    for k, r in enumerate(pure):                      # with few hypotheses a pair may have no model: the referee says which
        if not tc.undecided(r, M_HYP):
            assert res[k]["info"] == r["info"], (iterations, k)
        if res[k]["info"] == npt.NO_MODEL:
            assert untouched(res[k], [key for key in PAIR_KEYS + POINT_KEYS if key != "info" and key not in LIFT_KEYS]), (iterations, k)
    keep = [k for k, r in enumerate(pure) if r["info"] == npt.OK and res[k]["info"] == npt.OK]
    assert keep or iterations == 1
    check_stages([pairs[k] for k in keep], [res[k] for k in keep], iterations, [pure[k] for k in keep], "%d iterations" % iterations, not long)


@pytest.mark.gpu
def test_ragged_batch_with_failures():
    """one call of 257 pairs of 0 to 120 points with TOO_FEW, BAD_INPUT and NO_MODEL pairs mixed in: the stages, and the sentinel in
    everything a failed pair does not write"""
    pairs = tc.batch_pairs()
    res = device("batch")
    assert len(res) == 257
    check_stages(pairs, res, tg.ITERATIONS, tc.referee("batch"), "257 pairs")
    assert sorted({int(d["info"]) for d in res}) == [npt.OK, npt.TOO_FEW, npt.NO_MODEL, npt.BAD_INPUT]


@pytest.mark.gpu
def test_truth_pairs_at_a_thousand_iterations():
    """the pairs of the referee's truth test at OpenCV's 1000 iterations, all stages with the longdouble pass"""
    check_stages(tc.truth_pairs(), device("truth"), tc.TRUTH_ITERATIONS, tc.referee("truth"), "truth pairs")


@pytest.mark.gpu
def test_end_to_end_on_the_decided_set():
    """the 48 pairs of trackreject_cases.e2e_pairs: at least 90 % are decided, and those equal the pure referee in every decision"""
    pairs = tc.e2e_pairs()
    _, _, decided = check_stages(pairs, device("e2e"), tg.ITERATIONS, tc.referee("e2e"), "end-to-end set")
    assert decided >= 0.9 * len(pairs)


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


def _device_memory_call(pairs, iterations=tg.ITERATIONS):
    """on_device = 1 over hipMalloc'ed buffers pre-filled with the sentinel; returns the per-pair dicts"""
    cur, prev, cam, dt = tg.pack(pairs)
    nf = len(pairs)
    first = np.concatenate([[0], np.cumsum([p.shape[0] for p in cur])]).astype(np.int32)
    tot = int(first[-1])
    isent = int(SENTINEL)
    out = dict(status=np.full(tot, 255, np.uint8), keep_idx=np.full(tot, isent, np.int32), n_inliers=np.full(nf, isent, np.int32),
               best=np.full(nf, isent, np.int32), n_iters=np.full(nf, isent, np.int32), info=np.full(nf, -1, np.int32), F=np.full((nf, 9), SENTINEL),
               un_cur=np.full((tot, 2), SENTINEL), un_prev=np.full((tot, 2), SENTINEL), velocity=np.full((tot, 2), SENTINEL),
               samples=np.full((nf, iterations, 8), isent, np.int32), hyp=np.full((nf, iterations, 9), SENTINEL),
               count=np.full((nf, iterations), isent, np.int32))
    D = DeviceArrays()
    try:
        ins = [D.up(a) for a in (first, np.concatenate(cur), np.concatenate(prev), dt)]
        o = {k: D.up(v) for k, v in out.items()}
        rc = solver.lib().swf_track_reject_batch(C.c_int32(nf), C.cast(ins[0], pi), C.cast(ins[1], pd), C.cast(ins[2], pd), (C.c_double * 12)(*cam),
                                                 C.c_int32(tg.COL), C.c_int32(tg.ROW), C.c_double(tg.FOCAL), C.cast(ins[3], pd), C.c_int32(iterations),
                                                 C.c_double(tg.THRESHOLD), C.c_double(tg.CONFIDENCE), C.c_uint64(tg.SEED), C.c_int32(_flag(pairs)),
                                                 C.cast(o["status"], pb), C.cast(o["keep_idx"], pi), C.cast(o["n_inliers"], pi), C.cast(o["best"], pi),
                                                 C.cast(o["n_iters"], pi), C.cast(o["info"], pi), C.cast(o["F"], pd), C.cast(o["un_cur"], pd),
                                                 C.cast(o["un_prev"], pd), C.cast(o["velocity"], pd), C.cast(o["samples"], pi), C.cast(o["hyp"], pd),
                                                 C.cast(o["count"], pi), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in out.items():
            D.down(o[k], v)
    finally:
        D.free()
    out["first"] = first
    return [pair_of(out, k) for k in range(nf)]


@pytest.mark.gpu
def test_alone_in_the_batch_host_and_device_memory_bitwise():
    """the one call of 257 pairs from host memory, the same call again, the same call from device memory, and pairs of it run alone:
    the same bits in every output; what a failed pair does not write stays untouched in device memory too"""
    pairs = tc.batch_pairs()
    assert len(pairs) == 257 and {p["fail"] for p in pairs} == {None, "few", "bad", "nomodel"}
    full = device("batch")
    again = run(pairs)
    dev = _device_memory_call(pairs)
    for k, p in enumerate(pairs):
        assert same_bits(pair_of(again, k), full[k]), k
        assert same_bits(dev[k], full[k]), k
    for k in (0, 1, 2, 4, 17, 19, 20, 40, 254, 256):
        one = run([pairs[k]])
        assert same_bits(pair_of(one, 0), full[k]), k
        alone = _device_memory_call([pairs[k]])
        assert same_bits(alone[0], full[k]), k


@pytest.mark.gpu
def test_outputs_may_be_null_and_exports_change_nothing():
    """every output but info is optional, and the scan's early end without the stage exports gives the same results as with them"""
    pairs = tc.iteration_pairs()
    cur, prev, cam, dt = tg.pack(pairs)
    first = np.concatenate([[0], np.cumsum([p.shape[0] for p in cur])]).astype(np.int32)
    fc, fp = np.ascontiguousarray(np.concatenate(cur)), np.ascontiguousarray(np.concatenate(prev))
    full = run(pairs, 1000)
    info = np.full(len(pairs), -9, np.int32)
    status = np.full(fc.shape[0], 255, np.uint8)
    nit = np.full(len(pairs), -9, np.int32)
    rc = solver.lib().swf_track_reject_batch(C.c_int32(len(pairs)), first.ctypes.data_as(pi), fc.ctypes.data_as(pd), fp.ctypes.data_as(pd),
                                             (C.c_double * 12)(*cam), C.c_int32(tg.COL), C.c_int32(tg.ROW), C.c_double(tg.FOCAL),
                                             np.ascontiguousarray(dt).ctypes.data_as(pd), C.c_int32(1000), C.c_double(tg.THRESHOLD),
                                             C.c_double(tg.CONFIDENCE), C.c_uint64(tg.SEED), C.c_int32(1), status.ctypes.data_as(pb), None, None, None,
                                             nit.ctypes.data_as(pi), info.ctypes.data_as(pi), None, None, None, None, None, None, None, C.c_int32(0), None)
    assert rc == 0, solver.lib().swf_last_error()
    assert np.array_equal(info, full["info"]) and np.array_equal(status, full["status"]) and np.array_equal(nit, full["n_iters"])
    assert (full["n_iters"] < 1000 - 256).any()                               # a scan did end chunks early


@pytest.mark.gpu
def test_chained_with_pnp_on_device_memory():
    """the kept tracks' un_cur, gathered on the device by keep_idx into the observations swf_pnp_frame_batch reads there: the same pose
    bits as through the host"""
    p = tc.shape_pairs()[2 * tc.SHAPE_N.index(65) + 1]
    host = pair_of(run([p]), 0)
    assert host["info"] == npt.OK and p["flags"] == 1
    keep = host["keep_idx"][:host["n_inliers"]]
    uv = host["un_cur"][keep]
    rng = np.random.default_rng(5)
    f = pg.gen_frame(77, keep.size, outliers=0.0)                          # a pose and its extrinsics; the landmarks are placed on the rays
    z = rng.uniform(3.0, 20.0, keep.size)
    pts_w = np.concatenate([uv * z[:, None], z[:, None]], axis=1) @ f["Rc_true"].T + f["Pc_true"]
    args = dict(iterations=pg.ITERATIONS, threshold=pg.THRESHOLD, confidence=pg.CONFIDENCE, seed=pg.SEED, flags=1)
    via_host = solver.pnp_frame_batch([pts_w], [uv], f["Ps_prev"][None], f["Rs_prev"].reshape(1, 9), pg.TIC, pg.RIC, pg.PBG, **args)
    assert via_host["info"][0] == npp.OK
    D = DeviceArrays()
    vec = lambda v, k: (C.c_double * k)(*np.asarray(v, np.float64).reshape(k))
    n = p["n"]
    try:
        d_first, d_cur, d_prev, d_dt = (D.up(a) for a in (np.array([0, n], np.int32), p["cur"], p["prev"], np.array([p["dt"]])))
        d_un, d_keep, d_int = D.up(np.zeros((n, 2))), D.up(np.full(n, -5, np.int32)), D.up(np.zeros(4, np.int32))
        rc = solver.lib().swf_track_reject_batch(C.c_int32(1), C.cast(d_first, pi), C.cast(d_cur, pd), C.cast(d_prev, pd), (C.c_double * 12)(*p["cam"]),
                                                 C.c_int32(tg.COL), C.c_int32(tg.ROW), C.c_double(tg.FOCAL), C.cast(d_dt, pd), C.c_int32(tg.ITERATIONS),
                                                 C.c_double(tg.THRESHOLD), C.c_double(tg.CONFIDENCE), C.c_uint64(tg.SEED), C.c_int32(1), None,
                                                 C.cast(d_keep, pi), C.cast(d_int, pi), None, None, C.cast(C.c_void_p(d_int.value + 4), pi), None,
                                                 C.cast(d_un, pd), None, None, None, None, None, C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        got_keep, got_int = np.zeros(n, np.int32), np.zeros(4, np.int32)
        D.down(d_keep, got_keep); D.down(d_int, got_int)
        assert got_int[1] == npt.OK and got_int[0] == keep.size and np.array_equal(got_keep[:keep.size], keep)
        d_uv = D.up(np.zeros((keep.size, 2)))
        for j, i in enumerate(keep):                                          # the gather: 16 bytes per kept track, device to device
            _hip("hipMemcpy", C.c_void_p(d_uv.value + 16 * j), C.c_void_p(d_un.value + 16 * int(i)), C.c_size_t(16), C.c_int(3))
        d_f2, d_pw, d_pp, d_rp = (D.up(a) for a in (np.array([0, keep.size], np.int32), pts_w, f["Ps_prev"], f["Rs_prev"]))
        d_Ps, d_Rs, d_i2, d_in = D.up(np.zeros(3)), D.up(np.zeros(9)), D.up(np.zeros(4, np.int32)), D.up(np.zeros(keep.size, np.uint8))
        at = lambda d, off: C.c_void_p(d.value + off)
        rc = solver.lib().swf_pnp_frame_batch(C.c_int32(1), C.cast(d_f2, pi), C.cast(d_pw, pd), C.cast(d_uv, pd), C.cast(d_pp, pd), C.cast(d_rp, pd),
                                              vec(pg.TIC, 3), vec(pg.RIC, 9), vec(pg.PBG, 3), C.c_int32(pg.ITERATIONS), C.c_double(pg.THRESHOLD),
                                              C.c_double(pg.CONFIDENCE), C.c_uint64(pg.SEED), C.c_int32(1), C.cast(d_Ps, pd), C.cast(d_Rs, pd),
                                              C.cast(d_i2, pi), C.cast(d_in, pb), C.cast(at(d_i2, 4), pi), C.cast(at(d_i2, 8), pi),
                                              C.cast(at(d_i2, 12), pi), None, None, None, C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        Ps, Rs, i2 = np.zeros(3), np.zeros(9), np.zeros(4, np.int32)
        D.down(d_Ps, Ps); D.down(d_Rs, Rs); D.down(d_i2, i2)
    finally:
        D.free()
    assert i2[3] == npp.OK and i2[0] == via_host["n_inliers"][0]
    assert np.array_equal(bits(Ps), bits(via_host["Ps"][0])) and np.array_equal(bits(Rs), bits(via_host["Rs"][0]))


@pytest.mark.gpu
def test_track_reject_adapter_runs(tmp_path):
    exe = compile_shim(tmp_path, "shim_track_reject")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "track reject ok" in out.stdout, out.stdout
