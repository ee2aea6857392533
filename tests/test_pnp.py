"""Batched RANSAC PnP (swf_pnp_frame_batch / solver.pnp_frame_batch / swf_ceres::InitFramePoseByPnP), the part that needs
no GPU: the exported symbol, the host-side rejections, the sampler, the numpy referee of tests/np_pnp.py against the truth on the
frames of tests/pnp_gen.py, the conditions on those frames that tests/test_pnp_gpu.py relies on, and the tolerance constants.

hyp (the minimal solves) and Ps_out / Rs_out (the refinement) are compared with the longdouble referee in units of the bracket
2^-52 cond(A) max(1, |t|), cond(A) the largest condition number of the 6 x 6 normal equations over the Gauss-Newton steps.  M_HYP and
M_REF are measured, not chosen (test_tolerance_constants_are_the_measured_ones): the float64 referee in two summation orders against
the longdouble referee on the inputs of pnp_cases.py (the three frame sets at 100 iterations and the iteration-count frames at 1 to 128),
over the frames that get a pose (a frame without one exports nothing to compare; its minimal solves, which do not converge, reach 1.39):
largest ratios 0.151 (hyp) and 0.0173 (refinement), times the margin of 8 for the device's fused multiply-adds, rounded up:
M_HYP = 2, M_REF = 1.  Largest device deviations on MI355X: 0.142 and 0.0150 (tests/test_pnp_gpu.py prints them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_pnp as npp
import pnp_cases as pc
import pnp_gen as pg
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import build, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -2, -3
SENTINEL = -7.0
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pb = C.POINTER(C.c_uint8)
GOLDEN = os.path.join(ROOT, "tests", "golden", "pnp_samples_seed.json")


def test_pnp_symbol_exported():
    build.build()
    lib = C.CDLL(solver.LIB_PATH)
    assert hasattr(lib, "swf_pnp_frame_batch")
    assert "swf_pnp_frame_batch" in solver.EXPORTED and callable(solver.pnp_frame_batch)
    hdr = open(os.path.join(ROOT, "include", "swf_solver.h")).read()
    for s in ("int swf_pnp_frame_batch(", "SWF_PNP_OK = 0", "SWF_PNP_TOO_FEW = 1", "SWF_PNP_NO_MODEL = 2", "SWF_PNP_UNREFINED = 3",
              "SWF_PNP_BAD_INPUT = 4", "#define SWF_PNP_NMAX 1024", "#define SWF_PNP_HMAX 128"):
        assert s in hdr, s
    assert "InitFramePoseByPnP(" in open(os.path.join(ROOT, "include", "swf_ceres.hpp")).read()
    assert (solver.PNP_OK, solver.PNP_TOO_FEW, solver.PNP_NO_MODEL, solver.PNP_UNREFINED, solver.PNP_BAD_INPUT) == \
        (npp.OK, npp.TOO_FEW, npp.NO_MODEL, npp.UNREFINED, npp.BAD_INPUT)
    assert (solver.PNP_NMAX, solver.PNP_HMAX) == (npp.NMAX, npp.HMAX)
    assert lib.swf_version() == 113


def _raw_call(frames, drop=None, first=None, n=None, iterations=100, threshold=pg.THRESHOLD, flags=1):
    """swf_pnp_frame_batch on host memory with every output pre-filled; returns (code, outputs)"""
    pw, uv, pp, rp = pg.pack(frames)
    nf = len(frames)
    fst = np.concatenate([[0], np.cumsum([p.shape[0] for p in pw])]).astype(np.int32) if first is None else np.asarray(first, np.int32)
    fw = np.ascontiguousarray(np.concatenate(pw + [np.zeros((1, 3))])); fu = np.ascontiguousarray(np.concatenate(uv + [np.zeros((1, 2))]))
    H = max(min(iterations, 128), 1)
    o = dict(Ps=np.full((nf, 3), SENTINEL), Rs=np.full((nf, 9), SENTINEL), ni=np.full(nf, -9, np.int32), inl=np.full(fw.shape[0], 77, np.uint8),
             best=np.full(nf, -9, np.int32), nit=np.full(nf, -9, np.int32), info=np.full(nf, -9, np.int32),
             samples=np.full((nf, H, 5), -9, np.int32), hyp=np.full((nf, H, 12), SENTINEL), count=np.full((nf, H), -9, np.int32))
    vec = lambda v, k: (C.c_double * k)(*np.asarray(v, np.float64).reshape(k))
    a = dict(first=fst.ctypes.data_as(pi), pw=fw.ctypes.data_as(pd), uv=fu.ctypes.data_as(pd), pp=pp.ctypes.data_as(pd), rp=rp.ctypes.data_as(pd),
             tic=vec(pg.TIC, 3), ric=vec(pg.RIC, 9), pbg=vec(pg.PBG, 3), Ps=o["Ps"].ctypes.data_as(pd), Rs=o["Rs"].ctypes.data_as(pd),
             ni=o["ni"].ctypes.data_as(pi), inl=o["inl"].ctypes.data_as(pb), best=o["best"].ctypes.data_as(pi), nit=o["nit"].ctypes.data_as(pi),
             info=o["info"].ctypes.data_as(pi), samples=o["samples"].ctypes.data_as(pi), hyp=o["hyp"].ctypes.data_as(pd), count=o["count"].ctypes.data_as(pi))
    if drop:
        a[drop] = None
    rc = solver.lib().swf_pnp_frame_batch(C.c_int32(nf if n is None else n), a["first"], a["pw"], a["uv"], a["pp"], a["rp"], a["tic"], a["ric"], a["pbg"],
                                          C.c_int32(iterations), C.c_double(threshold), C.c_double(pg.CONFIDENCE), C.c_uint64(pg.SEED), C.c_int32(flags),
                                          a["Ps"], a["Rs"], a["ni"], a["inl"], a["best"], a["nit"], a["info"], a["samples"], a["hyp"], a["count"],
                                          C.c_int32(0), None)
    return rc, o


def _untouched(o, info=False):
    return ((o["Ps"] == SENTINEL).all() and (o["Rs"] == SENTINEL).all() and (o["hyp"] == SENTINEL).all() and (o["inl"] == 77).all()
            and all((o[k] == -9).all() for k in ("ni", "best", "nit", "samples", "count") + (("info",) if info else ())))


def test_host_side_validation_needs_no_device():
    """A call whose frames are all TOO_FEW / BAD_INPUT returns SWF_OK with those codes and nothing else written, without touching the
    device, so this runs anywhere; the argument errors return their codes and write nothing."""
    build.build()
    bad = [pg.gen_frame(40, 3, fail="few"), pg.gen_frame(41, 9, fail="bad"), pg.gen_frame(42, 0, fail="few"), pg.gen_frame(43, 64, fail="bad"),
           pg.gen_frame(44, 30)]
    bad[4]["Rs_prev"] = bad[4]["Rs_prev"].copy(); bad[4]["Rs_prev"][1, 2] = np.inf
    big = pg.gen_frame(45, 5); big["pts_w"] = big["pts_w"].copy(); big["pts_w"][2, 0] = 1e39       # finite as a double, infinite as a float
    rc, o = _raw_call(bad + [big])
    assert rc == 0, solver.lib().swf_last_error()
    assert o["info"].tolist() == [npp.TOO_FEW, npp.BAD_INPUT, npp.TOO_FEW, npp.BAD_INPUT, npp.BAD_INPUT, npp.BAD_INPUT]
    assert _untouched(o)
    res = solver.pnp_frame_batch(*pg.pack(bad), *pc.ARGS, seed=pg.SEED, fill=SENTINEL, stages=True)
    assert res["info"].tolist() == o["info"].tolist()[:5] and (res["Ps"] == SENTINEL).all() and (res["hyp"] == SENTINEL).all()
    for drop in ("first", "pw", "uv", "pp", "rp", "tic", "ric", "pbg", "Ps", "Rs", "ni", "inl", "best", "nit", "info"):
        rc, o = _raw_call(bad, drop=drop)
        assert rc == E_INVALID and _untouched(o, info=True), drop
    for drop in ("samples", "hyp", "count"):                                  # optional
        rc, o = _raw_call(bad, drop=drop)
        assert rc == 0 and _untouched(o), drop
    rc, o = _raw_call(bad, first=[0, 3, 12, 11, 76, 106])
    assert rc == E_INVALID and _untouched(o, info=True)
    rc, o = _raw_call(bad, first=[-1, 3, 12, 12, 76, 106])
    assert rc == E_INVALID and _untouched(o, info=True)
    for it in (0, -1, 129):
        rc, o = _raw_call(bad, iterations=it)
        assert rc == E_UNSUPPORTED and _untouched(o, info=True), it
    for thr in (0.0, -1.0, np.nan, np.inf):
        rc, o = _raw_call(bad, threshold=thr)
        assert rc == E_INVALID and _untouched(o, info=True), thr
    rc, o = _raw_call(bad, n=-1)
    assert rc == E_INVALID
    rc, o = _raw_call(bad, n=0)
    assert rc == 0 and _untouched(o, info=True)
    many = pg.gen_frame(46, 1025)
    rc, o = _raw_call([bad[0], many])
    assert rc == E_UNSUPPORTED and _untouched(o, info=True)
    with pytest.raises(solver.SwfError):
        solver.pnp_frame_batch(*pg.pack(bad), *pc.ARGS, iterations=129)


def test_sampler_indices_distinct_and_in_range():
    total_rejected = {}
    for n in (4, 5, 6, 64, 65, 200, 1024):
        s, rejected = npp.sample_table(n, 128, pg.SEED)
        total_rejected[n] = rejected
        if n == 4:
            assert s.tolist() == [[0, 1, 2, 3, -1]]
            continue
        assert s.shape == (128, 5) and (s >= 0).all() and (s < n).all(), n
        assert all(len(set(row)) == 5 for row in s.tolist()), n
    assert total_rejected[5] > 0                                              # the rejection path is taken
    # the hash itself: splitmix64's first outputs from state 0 are those of the published generator
    assert npp.splitmix64(0) == 0xE220A8397B1DCDAF and npp.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_sampler_golden_table():
    import json
    g = json.load(open(GOLDEN))
    for key, rows in g["tables"].items():
        n, H = (int(v) for v in key.split("x"))
        s, _ = npp.sample_table(n, H, int(g["seed"]))
        assert s.tolist() == rows, key


def test_referee_recovers_the_true_pose():
    """n >= 33, at most 40 % outliers: the mask holds at least 95 % of the true inliers, and the RMS of the residual norm over the true
    inliers at the refined pose is at most 3 sigma (expected: sqrt(2) sigma)."""
    for f, r in zip(pc.truth_frames(), pc.referee("truth")):
        assert r["info"] == npp.OK, f["seed"]
        true_in = ~f["outlier"]
        assert (r["inlier"] & true_in).sum() >= 0.95 * true_in.sum(), f["seed"]
        pw, uv = npp.stage_points(f["pts_w"], f["pts_uv"], f["flags"])
        _, _, _, _, res = npp.residuals(r["R"][None], r["t"][None], pw[true_in][None], uv[true_in][None])
        rms = float(np.sqrt((res[0] ** 2).sum(axis=1).mean()))
        print("n %d outliers %d: inliers %d of %d, rms / sigma %.3f, position error %.2e m" %
              (f["n"], f["outlier"].sum(), r["n_inliers"], true_in.sum(), rms / pg.SIGMA, np.abs(r["Ps"] - f["Ps_true"]).max()))
        assert rms <= 3.0 * pg.SIGMA, f["seed"]


def test_inputs_are_decisive():
    """The conditions the GPU tests rely on, on the referee alone: (i) at most 10 % of all hypotheses meet a condition number above 1e8;
    (ii) no frame rounds a stopping-rule quotient within 1e-9 of a half-integer; (iii) at most 5 % of the frames have a squared error
    within 1e-6 of the threshold or a |z| <= 1e-6 in some hypothesis-point pair.  And every frame gets the code it was generated for."""
    n_hyp = n_ill = n_frames = n_undecided = 0
    for which in ("shape", "batch", "truth"):
        for f, r in zip(pc.frames_of(which), pc.referee(which)):
            assert r["info"] == pc.expected_code(f), (which, f["seed"], r["info"])
            if "hyp" not in r:
                continue
            n_frames += 1
            n_hyp += len(r["hyp_cond"]); n_ill += int((~(r["hyp_cond"] <= pc.COND_MAX)).sum())
            assert not pc.near_half(r), (which, f["seed"])
            n_undecided += pc.undecided(r)
    print("hypotheses above 1e8 or invalid: %d of %d; undecided frames: %d of %d" % (n_ill, n_hyp, n_undecided, n_frames))
    assert n_ill <= 0.10 * n_hyp
    assert n_undecided <= 0.05 * n_frames
    codes = [r["info"] for r in pc.referee("batch")]
    assert sorted(set(codes)) == [npp.OK, npp.TOO_FEW, npp.NO_MODEL, npp.BAD_INPUT]


def measured_constants():
    """over every comparison the GPU tests make: the three frame sets at 100 iterations and the iteration-count frames at each count"""
    worst_h = worst_r = 0.0
    sets = [(lambda d, o, w=w: pc.referee(w, d, o)) for w in ("shape", "batch", "truth")]
    sets += [(lambda d, o, it=it: pc.referee_iterations(it, d, o)) for it in pc.ITERATIONS]
    for get in sets:
        ld = get("longdouble", 0)
        for order in (0, 1):
            for r, q in zip(get("float64", order), ld):
                if q["info"] != npp.OK:                  # a frame without a pose exports no hypotheses: nothing of it is compared
                    continue
                assert np.array_equal(r["samples"], q["samples"])
                use = (q["hyp_cond"] <= pc.COND_MAX) & (r["hyp_cond"] <= pc.COND_MAX)
                if use.any():
                    dev = np.abs(r["hyp"][use] - q["hyp"][use]).astype(np.float64).max(axis=1)
                    worst_h = max(worst_h, float((dev / pc.hyp_bracket(q["hyp_cond"], q["hyp"])[use]).max()))
                if q["info"] == npp.OK and r["info"] == npp.OK and r["best"] == q["best"] and np.array_equal(r["inlier"], q["inlier"]):
                    br = pc.EPS * q["ref_cond"] * pc.tnorm(q["t"])
                    dev = max(np.abs(r["Ps"] - q["Ps"]).max(), np.abs(r["Rs"] - q["Rs"]).max())
                    worst_r = max(worst_r, float(dev) / br)
    return worst_h, worst_r


def test_tolerance_constants_are_the_measured_ones():
    """M_HYP, M_REF = 8 x the largest ratio, over the test inputs that get a pose, of |float64 referee (either summation order) - longdouble referee| to
    the bracket 2^-52 cond(A) max(1, |t|), rounded up to the next integer.  Measured: 0.151 (hyp), 0.0173 (refinement): M_HYP = 2, M_REF = 1."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    worst_h, worst_r = measured_constants()
    print("largest float64 / longdouble deviation in units of the bracket: hyp %.4f, refinement %.4f" % (worst_h, worst_r))
    for worst, m in ((worst_h, pc.M_HYP), (worst_r, pc.M_REF)):
        assert 8.0 * worst <= m
        assert m <= 8.0 * worst + 1.0          # rounded up to the next integer, not padded


def test_pnp_adapter_compiles_as_cxx14(tmp_path):
    """InitFramePoseByPnP binds under the reference's -std=c++14; without a GPU the shim exits non-zero with a message."""
    exe = compile_shim(tmp_path, "shim_pnp")
    if solver.device_count() == 0:
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode != 0 and "failed" in r.stdout, r.stdout
