"""The IMU frame front on the device (swf_imu_frame_batch / solver.imu_frame_batch / swf_ceres::ImuIntegrate) and pre-integration over a
gather list (swf_preintegrate_runs_batch / solver.preintegrate_runs_batch): the sample cut, the mid-point prediction and the record of
SWFOptimization::ImuIntegrate + IMUProcess (R/swf/swf_imu.cpp:117-213) and SlideWindowFrame's sample push (R/swf/swf.cpp:241-247)
against the numpy referee of tests/np_imu_frame.py on the inputs of tests/imu_frame_gen.py.

cut: an interior row's dt is one subtraction and its acc / gyr are copies: exact.  The blended row: within 4 ulp of its operands'
magnitude (two divisions, two products and a sum of positive weights).
pre: bitwise equal to solver.preintegrate_batch on the cut rows; against the oracle at the tolerances of
test_gpu_parity.py::test_batched_preintegration_matches_oracle.
pred: within M_TOL x bracket of the longdouble referee, per frame, n = effective samples, T = the frame's span, maxima over the steps:
    P: 2^-52 n max(|P| + |V| T + |un_acc| T^2)      V: 2^-52 n max(|V| + |un_acc| T)      R: 2^-52 n max|R|
M_TOL is measured, not chosen (test_tolerance_constant_is_the_measured_one): the float64 referee in two legitimate operation orders
against the longdouble referee on exactly the inputs below: largest ratio of a deviation to the bracket = 0.93, times the margin of 8
for the device's fused multiply-adds, rounded up: M_TOL = 8.
Largest device deviation on MI355X, in units of the bracket: 0.912 (the 257-frame call); every GPU test prints it (`deviation / bracket`)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import np_imu_frame as nif
import imu_frame_gen as ig
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import build, solver, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
M_TOL = 8.0
E_INVALID = -2
SENTINEL = -7.5
NOISE = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
SHAPES = [(1, "at"), (2, "beyond"), (3, "beyond"), (16, "beyond"), (17, "beyond"), (40, "beyond"), (41, "beyond"), (40, "at"), (400, "beyond")]
PBGS = (np.zeros(3), ig.PBG)
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def shape_frames():
    """every raw-sample count of the issue, flag bit 0 both ways"""
    return [ig.gen_frame(100 + 2 * i + fl, n, last, flag=fl) for i, (n, last) in enumerate(SHAPES) for fl in (0, 1)]


@functools.lru_cache(maxsize=None)
def batch_frames():
    """257 ragged frames of 1 .. 24 raw samples, with the three failure codes mixed in"""
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 25, 257)
    sizes[:8] = [1, 2, 3, 16, 17, 24, 5, 4]
    out = []
    for i in range(257):
        fail = {5: "empty", 37: "no_inner", 38: "order", 39: "order0", 130: "empty", 131: "order", 200: "no_inner", 256: "order"}.get(i)
        n = max(int(sizes[i]), 3) if fail == "order" else int(sizes[i])
        last = "at" if (i % 7 == 3 or n == 1) and fail is None else "beyond"
        out.append(ig.gen_frame(1000 + i, n, last, flag=int(rng.integers(0, 2)), fail=fail))
    return out


def all_frames():
    return shape_frames() + batch_frames()


@functools.lru_cache(maxsize=None)
def referee(which, ipbg, dtype_name="float64", order="reference"):
    """the referee's result for every frame of shape_frames / batch_frames, computed once"""
    frames = shape_frames() if which == "shape" else batch_frames()
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return [nif.frame(f, PBGS[ipbg], ig.G_W, dtype, order) for f in frames]


def expected_code(f):
    return {None: nif.OK, "empty": nif.EMPTY, "no_inner": nif.NO_INNER, "order": nif.TIME_ORDER, "order0": nif.TIME_ORDER}[f["fail"]]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def frame_rows(res, k):
    lo, hi = int(res["first"][k]) + k, int(res["first"][k + 1]) + k + 1
    return res["cut"][lo:hi]


def check_frames(frames, res, ref64, refld, label):
    """asserts 1, 2 (bitwise part), 3 and 5 of the issue for one call; returns the largest deviation / bracket of pred"""
    worst = 0.0
    ok_rows = []
    for k, f in enumerate(frames):
        r64, rld = ref64[k], refld[k]
        assert res["info"][k] == r64["code"] == expected_code(f), (label, k)
        rows = frame_rows(res, k)
        if r64["code"] != nif.OK:
            assert (rows == SENTINEL).all() and (res["pre"][k] == SENTINEL).all() and (res["pred"][k] == SENTINEL).all(), (label, k)
            continue
        m = r64["cut"].shape[0]
        got = rows[:m]
        assert (rows[m:] == SENTINEL).all(), (label, k)
        blended = f["raw"][m - 2, 0] > f["t01"][1]
        exact = m - 1 if blended else m
        assert np.array_equal(bits(got[:exact]), bits(r64["cut"][:exact])), (label, k)
        if blended:
            assert got[m - 1, 0] == r64["cut"][m - 1, 0]                                     # dt_1 = t1 - t_prev: one subtraction
            mag = np.maximum(np.abs(f["raw"][m - 3, 1:]) if m >= 3 else 0.0, np.abs(f["raw"][m - 2, 1:]))
            assert (np.abs(got[m - 1, 1:] - r64["cut"][m - 1, 1:]) <= 4 * EPS * mag).all(), (label, k)
        ok_rows.append((k, got))
        ratio = float((np.abs(res["pred"][k] - rld["pred"].astype(np.float64)) / rld["bracket"]).max())
        worst = max(worst, ratio)
    if ok_rows:
        again = solver.preintegrate_batch([g for _, g in ok_rows], np.array([frames[k]["state"][15:21] for k, _ in ok_rows]), NOISE)
        for j, (k, _) in enumerate(ok_rows):
            assert np.array_equal(bits(res["pre"][k]), bits(again[j])), (label, k)
    print("%s: %d frames, pred deviation / bracket %.3f (M_TOL %.0f)" % (label, len(frames), worst, M_TOL))
    assert worst <= M_TOL, (label, worst)
    return worst


def run(frames, ipbg):
    return solver.imu_frame_batch(*ig.pack(frames), PBGS[ipbg], ig.G_W, NOISE, fill=SENTINEL)


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_imu_frame_symbols_exported():
    build.build()
    lib = C.CDLL(solver.LIB_PATH)
    for s in ("swf_imu_frame_batch", "swf_preintegrate_runs_batch"):
        assert hasattr(lib, s), s
        assert s in solver.EXPORTED
    assert callable(solver.imu_frame_batch) and callable(solver.preintegrate_runs_batch)
    hdr = open(os.path.join(ROOT, "include", "swf_solver.h")).read()
    for s in ("int swf_imu_frame_batch(", "int swf_preintegrate_runs_batch(", "SWF_IMUF_OK = 0", "SWF_IMUF_EMPTY = 1", "SWF_IMUF_NO_INNER = 2",
              "SWF_IMUF_TIME_ORDER = 3"):
        assert s in hdr, s
    assert "ImuIntegrate(" in open(os.path.join(ROOT, "include", "swf_ceres.hpp")).read()
    assert (solver.IMUF_OK, solver.IMUF_EMPTY, solver.IMUF_NO_INNER, solver.IMUF_TIME_ORDER) == (nif.OK, nif.EMPTY, nif.NO_INNER, nif.TIME_ORDER)


def test_referee_sample_on_t1_takes_no_interpolation():
    f = ig.gen_frame(1, 6, "at")
    code, rows = nif.cut(f["raw"], *f["t01"])
    assert code == nif.OK and rows.shape[0] == 6
    assert np.array_equal(rows[:, 1:], f["raw"][:, 1:])
    assert np.array_equal(rows[:, 0], np.diff(np.concatenate([[f["t01"][0]], f["raw"][:, 0]])))
    assert rows[:, 0].sum() == f["t01"][1] - f["t01"][0]                 # (the stamps lie on a binary grid: sums are exact)


def test_referee_blend_is_linear_at_t1():
    f = ig.gen_frame(2, 6, "beyond")
    t0, t1 = f["t01"]
    code, rows = nif.cut(f["raw"], t0, t1)
    assert code == nif.OK and rows.shape[0] == 6
    assert np.array_equal(rows[:5, 1:], f["raw"][:5, 1:])
    ta, tb = f["raw"][4, 0], f["raw"][5, 0]
    assert ta < t1 < tb and rows[5, 0] == t1 - ta and rows[:, 0].sum() == t1 - t0
    lin = f["raw"][4, 1:] + (f["raw"][5, 1:] - f["raw"][4, 1:]) * ((t1 - ta) / (tb - ta))
    assert np.abs(rows[5, 1:] - lin).max() <= 4 * EPS * np.abs(f["raw"][4:6, 1:]).max()
    # a sample further beyond t1 is not used
    g = dict(f, raw=np.vstack([f["raw"], f["raw"][5] + np.array([0.0025, 0, 0, 0, 0, 0, 0])]))
    assert np.array_equal(nif.cut(g["raw"], t0, t1)[1], rows)
    # the failure codes
    assert nif.cut(np.zeros((0, 7)), t0, t1)[0] == nif.EMPTY
    assert nif.cut(f["raw"][5:], t0, t1)[0] == nif.NO_INNER
    assert nif.cut(f["raw"][[0, 2, 1, 3, 4, 5]], t0, t1)[0] == nif.TIME_ORDER


def test_referee_rotation_update_is_the_unnormalised_one():
    """M(theta) = toRotationMatrix of (1, theta / 2) without normalisation: M - I = (1 + |theta|^2 / 4) (Rn - I) with Rn the rotation of
    the normalised quaternion, so M misses Rn by |theta|^2 / 4 (Rn - I): second order relative to the increment.  A restatement that
    normalises first (or takes the exponential map) fails this."""
    for theta in (np.array([0.02, -0.01, 0.03]), np.array([0.3, 0.2, -0.4])):
        M, Rn = nif.M_theta(theta), nif.rotation_of(theta)
        s = float(theta @ theta) / 4
        assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-15
        gap = M - Rn
        assert np.abs(gap - s * (Rn - np.eye(3))).max() <= 8 * EPS
        assert np.abs(gap).max() >= 0.5 * s * np.abs(theta).max()                        # and that is not rounding
        assert np.abs(M.T @ M - np.eye(3)).max() >= s * s                                 # M is not orthonormal: M^T M - I = 4 s (s I - v v^T)
    # one IMUProcess step of the referee multiplies by exactly this M
    f = ig.gen_frame(3, 1, "at")
    f["seed"][3:] = [0.3, -0.2, 0.25]; f["raw"][0, 4:] = [0.3, -0.2, 0.25]
    out = nif.frame(f, np.zeros(3), ig.G_W)
    R0 = f["state"][3:12].reshape(3, 3)
    dt = f["t01"][1] - f["t01"][0]
    want = R0 @ nif.M_theta((np.array([0.3, -0.2, 0.25]) - f["state"][18:21]) * dt)
    assert np.abs(out["pred"][3:12].reshape(3, 3) - want).max() <= 4 * EPS


def test_inputs_are_decisive():
    """every |t - t1| of every test input is exactly 0 or at least 1e-6 s; the inputs cover what the issue lists"""
    ats = beyonds = 0
    for f in all_frames():
        if f["raw"].shape[0] == 0:
            continue
        d = np.abs(f["raw"][:, 0] - f["t01"][1])
        assert ((d == 0) | (d >= 1e-6)).all()
        ats += int((d == 0).any()); beyonds += int((f["raw"][:, 0] > f["t01"][1]).any())
    assert ats >= 20 and beyonds >= 150
    assert [(f["raw"].shape[0]) for f in shape_frames()[::2]] == [n for n, _ in SHAPES]
    codes = [expected_code(f) for f in batch_frames()]
    assert {nif.OK, nif.EMPTY, nif.NO_INNER, nif.TIME_ORDER} == set(codes) and codes.count(nif.OK) == 257 - 8
    assert {f["flag"] for f in batch_frames()} == {0, 1}
    for which in ("shape", "batch"):
        frames = shape_frames() if which == "shape" else batch_frames()
        assert [r["code"] for r in referee(which, 1)] == [expected_code(f) for f in frames]


def test_tolerance_constant_is_the_measured_one():
    """M_TOL = 8 x the largest ratio, over the test inputs, of |float64 referee (either operation order) - longdouble referee| to the
    bracket, rounded up to the next integer."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    worst = 0.0
    for which in ("shape", "batch"):
        for ipbg in (0, 1):
            ld = referee(which, ipbg, "longdouble")
            for order in ("reference", "alt"):
                for r, q in zip(referee(which, ipbg, "float64", order), ld):
                    if q["code"] == nif.OK:
                        worst = max(worst, float((np.abs(r["pred"] - q["pred"]).astype(np.float64) / q["bracket"]).max()))
    print("largest float64 / longdouble deviation in units of the bracket: %.3f" % worst)
    assert 8.0 * worst <= M_TOL
    assert M_TOL <= 8.0 * worst + 1.0          # rounded up to the next integer, not padded


def _raw_call(frames, drop=None, first=None, n=None):
    """swf_imu_frame_batch on host memory; returns (code, info, cut, pre, pred)"""
    raw, t01, seed, state, gp, flags = ig.pack(frames)
    nf = len(frames)
    fst = np.concatenate([[0], np.cumsum([r.shape[0] for r in raw])]).astype(np.int32) if first is None else np.asarray(first, np.int32)
    flat = np.ascontiguousarray(np.concatenate(raw + [np.zeros((1, 7))]))
    cut = np.full((flat.shape[0] + nf, 7), SENTINEL); pre = np.full((nf, 293), SENTINEL); pred = np.full((nf, 15), SENTINEL)
    info = np.full(nf, -9, np.int32)
    v3 = lambda v: (C.c_double * 3)(*v)
    args = dict(raw=flat.ctypes.data_as(pd), first=fst.ctypes.data_as(pi), t01=t01.ctypes.data_as(pd), seed=seed.ctypes.data_as(pd),
                state=state.ctypes.data_as(pd), gp=gp.ctypes.data_as(pd), flags=flags.ctypes.data_as(pi), pbg=v3(ig.PBG), gw=v3(ig.G_W),
                noise=(C.c_double * 4)(*NOISE), cut=cut.ctypes.data_as(pd), pre=pre.ctypes.data_as(pd), pred=pred.ctypes.data_as(pd),
                info=info.ctypes.data_as(pi))
    if drop:
        args[drop] = None
    a = args
    rc = solver.lib().swf_imu_frame_batch(a["raw"], a["first"], C.c_int32(nf if n is None else n), a["t01"], a["seed"], a["state"], a["gp"], a["flags"],
                                          a["pbg"], a["gw"], a["noise"], a["cut"], a["pre"], a["pred"], a["info"], C.c_int32(0), None)
    return rc, info, cut, pre, pred


def test_host_side_validation_needs_no_device():
    """SWF_E_INVALID on a null pointer or a decreasing `first`; the three per-frame failure codes from host memory.  A call whose frames
    all fail returns SWF_OK without touching the device, so this runs anywhere."""
    build.build()
    bad = [ig.gen_frame(50, 0, fail="empty"), ig.gen_frame(51, 1, fail="no_inner"), ig.gen_frame(52, 5, fail="order"),
           ig.gen_frame(53, 4, fail="order0"), ig.gen_frame(54, 7, fail="no_inner")]
    rc, info, cut, pre, pred = _raw_call(bad)
    assert rc == 0, solver.lib().swf_last_error()
    assert info.tolist() == [nif.EMPTY, nif.NO_INNER, nif.TIME_ORDER, nif.TIME_ORDER, nif.NO_INNER]
    assert (cut == SENTINEL).all() and (pre == SENTINEL).all() and (pred == SENTINEL).all()
    res = solver.imu_frame_batch(*ig.pack(bad), ig.PBG, ig.G_W, NOISE, fill=SENTINEL)
    assert res["info"].tolist() == info.tolist() and (res["pred"] == SENTINEL).all()
    for drop in ("raw", "first", "t01", "seed", "state", "gp", "flags", "pbg", "gw", "noise", "cut", "pre", "pred", "info"):
        rc, info, cut, pre, pred = _raw_call(bad, drop=drop)
        assert rc == E_INVALID and (info == -9).all() if drop != "info" else rc == E_INVALID, drop
    rc, info, *_ = _raw_call(bad, first=[0, 0, 1, 6, 5, 17])
    assert rc == E_INVALID and (info == -9).all()
    rc, info, *_ = _raw_call(bad, n=-1)
    assert rc == E_INVALID
    rc, info, *_ = _raw_call(bad, n=0)
    assert rc == 0 and (info == -9).all()
    # the gather list: malformed lists are refused before the device is touched
    smp = np.zeros((10, 7)); bias = np.zeros((2, 6))
    for runs in ([[(0, 4)], [(8, 3)]], [[(-1, 2)], [(0, 2)]], [[(0, -2)], [(0, 2)]]):
        with pytest.raises(solver.SwfError):
            solver.preintegrate_runs_batch(smp, runs, bias, NOISE)
    lib = solver.lib()
    out = np.zeros((2, 293)); rn = np.array([[0, 4], [4, 3]], np.int32); rf = np.array([0, 2, 1], np.int32)
    nz = (C.c_double * 4)(*NOISE)
    assert lib.swf_preintegrate_runs_batch(smp.ctypes.data_as(pd), C.c_int32(10), rn.ctypes.data_as(pi), rf.ctypes.data_as(pi), C.c_int32(2),
                                           bias.ctypes.data_as(pd), nz, out.ctypes.data_as(pd), C.c_int32(0), None) == E_INVALID
    assert lib.swf_preintegrate_runs_batch(smp.ctypes.data_as(pd), C.c_int32(10), None, rf.ctypes.data_as(pi), C.c_int32(2),
                                           bias.ctypes.data_as(pd), nz, out.ctypes.data_as(pd), C.c_int32(0), None) == E_INVALID


def test_imu_frame_adapter_compiles_as_cxx14(tmp_path):
    """ImuIntegrate binds to swf_ceres::ImuIntegrate under the reference's -std=c++14; without a GPU the shim exits non-zero with a
    message."""
    exe = compile_shim(tmp_path, "shim_imu_frame")
    if solver.device_count() == 0:
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode != 0 and "failed" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _oracle_agrees(g, rows, bias):
    """the tolerances of test_gpu_parity.py::test_batched_preintegration_matches_oracle"""
    import oracle_binding as ob
    ref = ob.preintegrate(rows, bias[:3], bias[3:], *NOISE)
    U0 = 68
    assert np.abs(g[:U0] - ref[:U0]).max() <= 1e-12 * max(1.0, np.abs(ref[:U0]).max())
    Ug, Ur = g[U0:].reshape(15, 15), ref[U0:].reshape(15, 15)
    if not Ur.any():
        assert rows.shape[0] <= 2 and not Ug.any()
        return
    assert np.all(np.tril(Ug, -1) == 0) and np.all(np.diag(Ug) > 0)
    info = Ur.T @ Ur
    cond = np.linalg.cond(info)
    assert np.abs(Ug - Ur).max() <= 1e-15 * cond * np.abs(Ur).max(), cond
    d = 1 / np.sqrt(np.diag(info))
    assert np.abs((Ug.T @ Ug - info) * np.outer(d, d)).max() <= 1e-15 * cond


@pytest.mark.gpu
@pytest.mark.parametrize("ipbg", [0, 1])
def test_sample_counts_match_referee(ipbg):
    """1 (on t1), 2, 3, 16, 17, 40, 41 and 400 raw samples, flag bit 0 both ways, each frame alone and all in one call; the record also
    against the oracle."""
    frames = shape_frames()
    r64, rld = referee("shape", ipbg), referee("shape", ipbg, "longdouble")
    res = run(frames, ipbg)
    worst = check_frames(frames, res, r64, rld, "all sample counts, pbg %d" % ipbg)
    for k, f in enumerate(frames):
        one = run([f], ipbg)
        worst = max(worst, check_frames([f], one, r64[k:k + 1], rld[k:k + 1], "%d raw samples, flag %d" % (f["raw"].shape[0], f["flag"])))
        assert np.array_equal(bits(one["pre"][0]), bits(res["pre"][k])) and np.array_equal(bits(one["pred"][0]), bits(res["pred"][k]))
        assert np.array_equal(bits(frame_rows(one, 0)), bits(frame_rows(res, k)))
        _oracle_agrees(res["pre"][k], r64[k]["cut"], f["state"][15:21])
    # one raw sample beyond t1: nothing to interpolate from
    f = ig.gen_frame(60, 1, fail="no_inner")
    one = run([f], ipbg)
    assert one["info"].tolist() == [nif.NO_INNER] and (one["cut"] == SENTINEL).all() and (one["pre"] == SENTINEL).all() and (one["pred"] == SENTINEL).all()
    print("largest device deviation in units of the bracket: %.3f" % worst)


@pytest.mark.gpu
def test_frames_per_call_and_batch_independence():
    """1, 3, 4, 5 and 64 frames per call (four frames share a wavefront) and the ragged 257 with the three failure codes mixed in: every
    frame equals the frame run alone, bit for bit; failed frames leave the sentinel."""
    frames = batch_frames()
    r64, rld = referee("batch", 1), referee("batch", 1, "longdouble")
    full = run(frames, 1)
    worst = check_frames(frames, full, r64, rld, "257 frames")
    assert sorted(set(full["info"].tolist())) == [0, 1, 2, 3]
    for cnt in (1, 3, 4, 5, 64):
        for lo in (0, 36):                                                     # (36 .. : the failures at 37, 38, 39 inside the group)
            part = run(frames[lo:lo + cnt], 1)
            worst = max(worst, check_frames(frames[lo:lo + cnt], part, r64[lo:lo + cnt], rld[lo:lo + cnt], "%d frames from %d" % (cnt, lo)))
            for k in range(cnt):
                assert part["info"][k] == full["info"][lo + k]
                assert np.array_equal(bits(part["pre"][k]), bits(full["pre"][lo + k])), (cnt, lo, k)
                assert np.array_equal(bits(part["pred"][k]), bits(full["pred"][lo + k])), (cnt, lo, k)
                assert np.array_equal(bits(frame_rows(part, k)), bits(frame_rows(full, lo + k))), (cnt, lo, k)
    for k in (0, 6, 40, 255):
        one = run([frames[k]], 1)
        assert np.array_equal(bits(one["pre"][0]), bits(full["pre"][k])) and np.array_equal(bits(one["pred"][0]), bits(full["pred"][k]))
    print("largest device deviation in units of the bracket: %.3f" % worst)


def _hip(call, *args):
    rc = getattr(solver.lib(), call)(*args)
    assert rc == 0, (call, rc)


@pytest.mark.gpu
def test_device_memory_equals_host_memory_bitwise():
    """on_device = 1 over hipMalloc'ed buffers pre-filled with the sentinel: the same bits as the host-memory call, failed frames
    untouched."""
    frames = batch_frames()[:70] + shape_frames()[:6]
    raw, t01, seed, state, gp, flags = ig.pack(frames)
    nf = len(frames)
    first = np.concatenate([[0], np.cumsum([r.shape[0] for r in raw])]).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate(raw))
    outs = dict(cut=np.full((flat.shape[0] + nf, 7), SENTINEL), pre=np.full((nf, 293), SENTINEL), pred=np.full((nf, 15), SENTINEL),
                info=np.full(nf, -9, np.int32))
    bufs = []

    def up(a):
        d = C.c_void_p()
        _hip("hipMalloc", C.byref(d), C.c_size_t(a.nbytes))
        bufs.append(d)
        _hip("hipMemcpy", d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1))
        return d
    try:
        ins = [up(np.ascontiguousarray(a)) for a in (flat, first, t01, seed, state, gp, flags)]
        o = {k: up(v) for k, v in outs.items()}
        v3 = lambda v: (C.c_double * 3)(*v)
        rc = solver.lib().swf_imu_frame_batch(C.cast(ins[0], pd), C.cast(ins[1], pi), C.c_int32(nf), C.cast(ins[2], pd), C.cast(ins[3], pd),
                                              C.cast(ins[4], pd), C.cast(ins[5], pd), C.cast(ins[6], pi), v3(ig.PBG), v3(ig.G_W), (C.c_double * 4)(*NOISE),
                                              C.cast(o["cut"], pd), C.cast(o["pre"], pd), C.cast(o["pred"], pd), C.cast(o["info"], pi), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in outs.items():
            _hip("hipMemcpy", C.c_void_p(v.ctypes.data), o[k], C.c_size_t(v.nbytes), C.c_int(2))
    finally:
        for d in bufs:
            solver.lib().hipFree(d)
    host = run(frames, 1)
    assert np.array_equal(outs["info"], host["info"]) and (host["info"] != 0).sum() >= 4
    for k in ("cut", "pre", "pred"):
        assert np.array_equal(bits(outs[k]), bits(host[k])), k


@pytest.mark.gpu
def test_preintegrate_runs_equals_concatenation_bitwise():
    """Two-run and three-run intervals, a run of one row, a first run holding only the seed, an empty run, and the slide merge of two
    frames' cut rows: the record of the gather list is, bit for bit, the record of the concatenated copy."""
    rng = np.random.default_rng(5)
    frames = [f for f in batch_frames()[:40] if f["fail"] is None]
    res = run(frames, 1)
    smp = res["cut"]
    fo = [int(res["first"][k]) + k for k in range(len(frames) + 1)]             # frame k owns rows fo[k] .. fo[k + 1] - 1
    runs = []
    for k in range(len(frames) - 1):                                            # the slide: frame k, then frame k + 1 without its seed
        runs.append([(fo[k], fo[k + 1] - fo[k]), (fo[k + 1] + 1, fo[k + 2] - fo[k + 1] - 1)])
    runs.append([(fo[3], 1), (fo[5] + 1, 7)])                                   # a first run holding only the seed
    runs.append([(fo[7], 4), (fo[2] + 2, 1), (fo[9] + 1, 9)])                   # three runs, one of a single row
    runs.append([(fo[1], 0), (fo[4], 5), (fo[4], 0), (fo[6] + 1, 3)])           # empty runs in front and in between
    runs.append([(fo[8], fo[9] - fo[8])])                                       # one run: the contiguous case
    runs.append([(fo[10], 1)])                                                  # the seed alone: no push_back
    runs.append([])                                                             # no run at all
    bias = np.concatenate([rng.normal(0, 0.05, (len(runs), 3)), rng.normal(0, 0.005, (len(runs), 3))], axis=1)
    got = solver.preintegrate_runs_batch(smp, runs, bias, NOISE)
    cat = [np.concatenate([smp[o:o + c] for o, c in r]) if r else np.zeros((0, 7)) for r in runs]
    want = solver.preintegrate_batch(cat, bias, NOISE)
    assert np.array_equal(bits(got), bits(want))
    assert got[-2][6] == 1.0 and not got[-2][68:].any()
    # the merged interval of a slide is the pre-integration of the two frames' joined effective samples
    r64 = referee("batch", 1)
    idx = [k for k, f in enumerate(batch_frames()[:40]) if f["fail"] is None]
    joined = [nif.merged_rows(r64[idx[k]]["cut"], r64[idx[k + 1]]["cut"]) for k in range(4)]
    ref = solver.preintegrate_batch(joined, bias[:4], NOISE)
    for k in range(4):
        assert np.array_equal(bits(cat[k][:, 0]), bits(joined[k][:, 0]))
        assert np.abs(cat[k] - joined[k]).max() <= 4 * EPS * np.abs(joined[k]).max()
        _oracle_agrees(got[k], cat[k], bias[k])
        assert np.abs(got[k][:68] - ref[k][:68]).max() <= 1e-12 * max(1.0, np.abs(ref[k][:68]).max())
    # a single interval alone equals itself in the batch
    one = solver.preintegrate_runs_batch(smp, [runs[1]], bias[1:2], NOISE)
    assert np.array_equal(bits(one[0]), bits(got[1]))


def _quat_of(R):
    """unit quaternion (x, y, z, w) of a nearly orthonormal R"""
    w = 0.5 * np.sqrt(max(1e-300, 1 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def _rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.gpu
def test_window_fed_by_the_frame_front_evaluates_as_with_the_referee():
    """A K = 4 window whose three IMU records and newest pose and speed come from swf_imu_frame_batch has the initial cost of the same
    window fed by the referee's prediction and the oracle's records (1e-9 relative)."""
    import oracle_binding as ob
    from rtk_visual_inertial_navigation_amd.flat import default_options
    w = synth.make_window(2, K=4, F=10, S=0, seed=3)
    pose, sb = w.a["pose"].reshape(-1, 7), w.a["sb"].reshape(-1, 9)
    frames = []
    for k in range(1, 4):
        f = ig.gen_frame(700 + k, 41, "beyond", flag=k & 1)
        q = pose[k, 3:7]
        if abs(q[3]) < 0.3:                                                    # (keep w away from 0 for _quat_of)
            q = np.array([0.1, -0.2, 0.15, 0.96]); q /= np.linalg.norm(q)
        f["state"] = np.concatenate([pose[k, :3], _rot_of(q).ravel(), sb[k, :3], sb[k - 1, 3:9]])
        frames.append(f)
    pbg = synth.PBG
    res = solver.imu_frame_batch(*ig.pack(frames), pbg, ig.G_W, NOISE)
    assert (res["info"] == 0).all()
    refs = [nif.frame(f, pbg, ig.G_W) for f in frames]
    wd, wo = w.copy(), w.copy()
    wd.a["imu_pre"][...] = res["pre"].reshape(wd.a["imu_pre"].shape)
    wo.a["imu_pre"][...] = np.concatenate([ob.preintegrate(refs[k]["cut"], frames[k]["state"][15:18], frames[k]["state"][18:21], *NOISE)
                                           for k in range(3)]).reshape(wo.a["imu_pre"].shape)
    for win, pred in ((wd, res["pred"][2]), (wo, refs[2]["pred"])):
        p, s = win.a["pose"].reshape(-1, 7), win.a["sb"].reshape(-1, 9)
        p[3, :3] = pred[:3]; p[3, 3:7] = _quat_of(pred[3:12].reshape(3, 3)); s[3, :3] = pred[12:15]
    bs = solver.BatchSolver([wd])
    sg = bs.solve(default_options(step_mode=1))[0]
    so, _ = ob.solve(wo, default_options(step_mode=1))
    bs.close()
    print("initial cost: device-fed %.17g, referee-fed %.17g" % (sg.initial_cost, so.initial_cost))
    assert abs(sg.initial_cost - so.initial_cost) <= 1e-9 * so.initial_cost


@pytest.mark.gpu
def test_imu_frame_adapter_runs(tmp_path):
    exe = compile_shim(tmp_path, "shim_imu_frame")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "imu frame ok" in out.stdout, out.stdout
