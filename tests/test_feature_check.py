"""Post-solve feature check on the device (swf_batch_check_features / swf_problem_check_features / swf_ceres::OutliersRejection):
the mean reprojection error of SWFOptimization::OutliersRejection and the depth sign of Double2Vector per feature, against the numpy
referee of tests/np_features.py evaluated at the state the device holds.

Tolerance of the values.  Two correct evaluations differ where `X - P_j` cancels: per feature
    tol_f = M_TOL * 2^-52 * (1 + max_k (|X| + |p_j| + |pbg| + |t_e|) / |pc.z|).
M_TOL is measured, not chosen (test_tolerance_constant_is_the_measured_one): the float64 referee in both legitimate operation
orders (OutliersRejection's `P_j = p_j - R_j pbg` first; the projection factor's `R_j^T (X - p_j) + pbg`) against the longdouble
referee on the inputs below, solved by the CPU oracle: largest ratio of a deviation to the bracket = 0.50 (mean_err), 2.14 (depth, on a
landmark 3e5 m behind the camera); times the margin of 8 for the device's fused multiply-adds, rounded up: M_TOL = 18.
Largest device deviation on MI355X, in units of the bracket: not measured; every GPU test prints it (`deviation / bracket`)."""
import functools
import re
import subprocess

import numpy as np
import pytest

import bitwise
import idepth_gen
import np_features as nf
import oracle_binding as ob
from shim import compile_shim
from stereo_gen import stereo_window
from rtk_visual_inertial_navigation_amd import build, solver, synth
from rtk_visual_inertial_navigation_amd.flat import FlatWindow, default_options

EPS = 2.0 ** -52
M_TOL = 18.0
SINGLE = [(2, 11, 8), (2, 13, 8), (3, 21, 24), (3, 22, 24)]          # (config, seed, injected landmarks)
E_INVALID, E_NOTFOUND, E_STATE = -2, -4, -5
NEW_SYMBOLS = ["swf_batch_check_features", "swf_batch_get_feature_check", "swf_problem_check_features",
               "swf_problem_get_feature_check", "swf_problem_rejected_features"]


# ---------------------------------------------------------------------------------------------------------------- inputs
def single_window(cfg, s, n_bad):
    w = synth.make_window(cfg, seed=s)
    nf.inject(w, np.random.default_rng(s + 99), n_bad)
    return w


def batch_windows():
    ws = synth.make_batch(64)
    for i in range(0, 64, 4):
        nf.inject(ws[i], np.random.default_rng(1000 + i), 24)
    return ws


@functools.lru_cache(maxsize=None)
def oracle_solved_inputs():
    """Every input of the issue, solved in place by the CPU oracle (8 iterations): [(label, injected?, window)]."""
    out = [("cfg %d seed %d" % (c, s), True, single_window(c, s, nb)) for c, s, nb in SINGLE]
    out += [("batch window %d" % i, i % 4 == 0, w) for i, w in enumerate(batch_windows())]
    for _, _, w in out:
        ob.solve(w, default_options(max_num_iterations=8), export=False)
    return out


def deviation_ratio(ref, got):
    """largest deviation of (mean_err, depth) from the referee in units of the bracket 2^-52 (1 + cond)"""
    br = EPS * (1.0 + ref["cond"].astype(np.float64))
    dm = np.abs((got["mean_err"] - ref["mean_err"]).astype(np.float64)) / br
    dd = np.abs((got["depth"] - ref["depth"]).astype(np.float64)) / (br * np.maximum(1.0, np.abs(ref["depth"].astype(np.float64))))
    return (float(dm.max()) if dm.size else 0.0), (float(dd.max()) if dd.size else 0.0)


def assert_matches_referee(w, got, threshold=2.0, label=""):
    """`got` (device) against the float64 referee at w's state: counts, flags and the rejected list exactly, values within tol_f."""
    ref = nf.check(w, threshold)
    assert got["n_feat"] == ref["n_feat"], label
    assert np.array_equal(got["n_obs"], ref["n_obs"]), label
    rm, rd = deviation_ratio(ref, got)
    print("%s: %d features, %d rejected, deviation / bracket: mean_err %.3f depth %.3f" % (label, ref["n_feat"], ref["rejected"].size, rm, rd))
    assert np.array_equal(got["flags"], ref["flags"]), (label, np.nonzero(got["flags"] != ref["flags"])[0])
    assert np.array_equal(got["rejected"], ref["rejected"]), label
    tol = M_TOL * EPS * (1.0 + ref["cond"])
    assert (np.abs(got["mean_err"] - ref["mean_err"]) <= tol).all(), (label, rm)
    assert (np.abs(got["depth"] - ref["depth"]) <= tol * np.maximum(1.0, np.abs(ref["depth"]))).all(), (label, rd)
    return rm, rd


def bitwise_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint8) if a[k].dtype != np.uint8 else a[k], b[k].view(np.uint8) if b[k].dtype != np.uint8 else b[k])
               for k in ("mean_err", "depth", "n_obs", "flags", "rejected")) and a["n_feat"] == b["n_feat"]


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_feature_symbols_exported():
    import ctypes
    build.build()
    lib = ctypes.CDLL(solver.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in solver.EXPORTED, s
    assert lib.swf_version() >= 108


def test_referee_inputs_are_decisive():
    """On the issue's inputs, solved by the CPU oracle, the referee alone separates the classes with room to spare: no feature
    within 0.05 of the threshold or within 1e-3 of zero depth, every injected window rejects some and keeps some, and the
    negative-depth class occurs.  This is what lets the GPU tests ask for exact flag equality with nothing left out."""
    neg = 0
    for label, injected, w in oracle_solved_inputs():
        r = nf.check(w)
        seen = r["n_obs"] > 0
        gap = np.abs(r["whitened"][seen] - 2.0).min(); zmin = np.abs(r["depth"][seen]).min()
        nneg = int(((r["flags"] & nf.NEG_DEPTH) != 0).sum()); neg += nneg
        print("%s: rejected %d of %d, closest whitened mean to 2: %.3f away, smallest |depth| %.3g, negatives %d"
              % (label, r["rejected"].size, r["n_feat"], gap, zmin, nneg))
        assert gap >= 0.05, label
        assert zmin >= 1e-3, label
        if injected:
            assert 1 <= r["rejected"].size < r["n_feat"], label
    assert neg >= 1


def test_tolerance_constant_is_the_measured_one():
    """M_TOL = 8 x the largest ratio, over the issue's inputs, of |float64 referee (either operation order) - longdouble referee|
    to the bracket 2^-52 (1 + cond)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    worst_m = worst_d = 0.0
    for label, _, w in oracle_solved_inputs():
        tab = nf.table(w)
        ref = nf.check(w, dtype=np.longdouble, tab=tab)
        for order in ("reference", "factor"):
            rm, rd = deviation_ratio(ref, nf.check(w, order=order, tab=tab))
            worst_m, worst_d = max(worst_m, rm), max(worst_d, rd)
    print("largest float64 / longdouble deviation in units of the bracket: mean_err %.3f depth %.3f" % (worst_m, worst_d))
    assert 8.0 * max(worst_m, worst_d) <= M_TOL
    assert M_TOL <= 8.0 * max(worst_m, worst_d) + 1.0          # rounded up to the next integer, not padded


def test_referee_refuses_disagreeing_anchors():
    w = idepth_gen.convert_short_tracks(synth.make_window(3, K=6, F=30, S=5, seed=41))
    ipts = w.a["idp_pts"].reshape(-1, 6); iidx = w.a["idp_idx"].reshape(-1, 5)
    c = iidx[0, 4]
    assert (iidx[:, 4] == c).sum() >= 2
    ipts[np.nonzero(iidx[:, 4] == c)[0][1], 0] += 1e-3
    with pytest.raises(ValueError):
        nf.table(w)


def test_outliers_adapter_compiles_as_cxx14(tmp_path):
    """ImagePostprocess's call binds to swf_ceres::OutliersRejection under the reference's -std=c++14; without a GPU the shim
    exits non-zero with a message."""
    exe = compile_shim(tmp_path, "shim_outliers")
    if solver.device_count() == 0:
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode != 0 and "failed" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def solve_and_check(windows, threshold=2.0):
    bs = solver.BatchSolver(windows)
    bs.solve(default_options())                          # (downloads the accepted state into the windows)
    return bs, bs.check_features(threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,n_bad", SINGLE)
def test_single_windows_match_referee(cfg, seed, n_bad):
    w = single_window(cfg, seed, n_bad)
    bs, res = solve_and_check([w])
    assert_matches_referee(w, res[0], label="cfg %d seed %d" % (cfg, seed))
    assert 1 <= res[0]["rejected"].size < res[0]["n_feat"]
    bs.close()


@pytest.mark.gpu
def test_batch_matches_referee_and_equals_single_bitwise():
    """All 64 windows against the referee; a window's results inside the batch are bit for bit those of the window alone; two
    checks in a row are bit for bit equal."""
    ws = batch_windows()
    alone = {}
    for i in (0, 5, 40, 56, 63):
        c = ws[i].copy()
        b1, r1 = solve_and_check([c])
        alone[i] = r1[0]
        b1.close()
    bs, res = solve_and_check(ws)
    worst = (0.0, 0.0)
    for i, w in enumerate(ws):
        rm, rd = assert_matches_referee(w, res[i], label="batch window %d" % i)
        worst = (max(worst[0], rm), max(worst[1], rd))
        if i % 4 == 0:
            assert 1 <= res[i]["rejected"].size < res[i]["n_feat"], i
    print("largest device deviation in units of the bracket: mean_err %.3f depth %.3f" % worst)
    for i, r in alone.items():
        assert bitwise_equal(r, res[i]), i
    again = bs.check_features(2.0)
    for i in range(len(ws)):
        assert bitwise_equal(res[i], again[i]), i
    bs.close()


def _exports(bs, ws):
    return ([bs.export_reduced(i) for i in range(len(ws))],
            [(s.initial_cost, s.final_cost, s.num_iterations, s.termination, [tuple(sorted(r.items())) for r in s.rows()]) for s in bs.summaries()],
            [w.state() for w in ws])


def _same(e1, e2):
    for (S, r, L), (S2, r2, L2) in zip(e1[0], e2[0]):
        assert np.array_equal(S, S2) and np.array_equal(r, r2) and np.array_equal(L, L2)
    assert e1[1] == e2[1]
    for s1, s2 in zip(e1[2], e2[2]):
        for k in s1:
            assert np.array_equal(s1[k], s2[k]), k


@pytest.mark.gpu
def test_check_is_read_only():
    """A solve's exports (S, rhs, L, summaries, state) are bit for bit the same with a check issued before them, and a second solve
    after a check equals a second solve without one."""
    base = [single_window(3, 21, 24), single_window(2, 11, 8), synth.make_window(3, seed=23)]
    wa = [w.copy() for w in base]; wb = [w.copy() for w in base]
    ba = solver.BatchSolver(wa); ba.solve(default_options())
    bb = solver.BatchSolver(wb); bb.solve(default_options()); bb.check_features(2.0)
    _same(_exports(ba, wa), _exports(bb, wb))
    ba.solve(default_options())
    bb.check_features(2.0)
    bb.solve(default_options())
    _same(_exports(ba, wa), _exports(bb, wb))
    ba.close(); bb.close()
    # the tail covariance and the ambiguity search behind a check, too (windows whose parameter_head tail holds the ambiguities)
    S = 9
    base = [synth.make_window(3, S=S, seed=900 + i, head="ambiguities") for i in range(2)]
    pairs = [[(i, 0) for i in range(1, S)]] * 2
    wa = [w.copy() for w in base]; wb = [w.copy() for w in base]
    ba = solver.BatchSolver(wa); ba.solve(default_options())
    bb = solver.BatchSolver(wb); bb.solve(default_options()); bb.check_features(2.0)
    ta = ba.tail_covariance(); tb = bb.tail_covariance()
    bb.check_features(2.0)
    sa = ba.ambiguity_search(pairs); sb = bb.ambiguity_search(pairs)
    for x, y in zip(ta, tb):
        assert x["n"] == S and np.array_equal(x["A"], y["A"]) and np.array_equal(x["Qy"], y["Qy"])
    for x, y in zip(sa, sb):
        assert x["info"] == y["info"] and x["fixed"] == y["fixed"]
        for k in ("F", "s", "ratio", "Qb", "bf"):
            assert np.array_equal(x[k], y[k]), k
    ba.close(); bb.close()


@pytest.mark.gpu
def test_generic_path_and_constant_landmarks():
    """Factors with a variable extrinsic (GF_PROJX on the generic path) and constant landmarks are covered like any other."""
    w = single_window(3, 21, 24)
    wx = synth.with_variable_extrinsic(w)
    wc = bitwise.with_constant(w, [w.bid_lm(l) for l in (0, 3, 7, 11)])
    bs, res = solve_and_check([wx, wc])
    assert_matches_referee(wx, res[0], label="variable extrinsic")
    assert_matches_referee(wc, res[1], label="constant landmarks")
    assert res[0]["rejected"].size >= 1 and res[1]["rejected"].size >= 1
    bs.close()


@pytest.mark.gpu
def test_inverse_depth_windows_and_negative_lambda():
    """convert_short_tracks windows (kind 0) after a solve; then some inverse depths set negative and checked at the uploaded state."""
    ws = [idepth_gen.convert_short_tracks(single_window(3, 22, 24)), idepth_gen.convert_short_tracks(synth.make_window(2, seed=12))]
    bs, res = solve_and_check(ws)
    for i, w in enumerate(ws):
        assert w.a["idp_kind"].size > 0
        assert_matches_referee(w, res[i], label="inverse depth %d" % i)
    for w in ws:
        lams = np.unique(w.a["idp_idx"].reshape(-1, 5)[:, 4])
        w.a["sc"][lams[::3]] *= -1.0
    bs.upload_state()
    res = bs.check_features(2.0)
    for i, w in enumerate(ws):
        lams = np.unique(w.a["idp_idx"].reshape(-1, 5)[:, 4])
        assert_matches_referee(w, res[i], label="negative lambda %d" % i)
        neg = (res[i]["flags"][w.n_lm:] & nf.NEG_DEPTH) != 0
        assert np.array_equal(neg, w.a["sc"][lams] < 0) and neg[::3].any(), i
    bs.close()


@pytest.mark.gpu
def test_stereo_factors_kinds_1_2_and_unobserved_landmark_at_uploaded_state():
    w, lone = stereo_window()
    assert set(w.a["idp_kind"].tolist()) == {0, 1, 2}
    bs = solver.BatchSolver([w])
    res = bs.check_features(2.0)[0]
    assert_matches_referee(w, res, label="stereo window")
    assert res["flags"][0] == nf.UNOBSERVED and res["n_obs"][0] == 0 and res["mean_err"][0] == 0 and res["depth"][0] == 0
    assert 0 not in res["rejected"]
    lams = np.unique(w.a["idp_idx"].reshape(-1, 5)[:, 4])
    f_lone = w.n_lm + int(np.nonzero(lams == lone)[0][0])
    assert res["n_obs"][f_lone] == 2 and res["depth"][f_lone] == 1.0 / 0.2
    # another threshold, the same values
    r0 = bs.check_features(0.0)[0]
    assert np.array_equal(r0["mean_err"], res["mean_err"])
    assert_matches_referee(w, r0, threshold=0.0, label="stereo window, threshold 0")
    bs.close()


@pytest.mark.gpu
def test_disagreeing_anchor_is_invalid_at_the_check_not_at_create():
    w = idepth_gen.convert_short_tracks(synth.make_window(3, K=6, F=30, S=5, seed=41))
    ipts = w.a["idp_pts"].reshape(-1, 6); iidx = w.a["idp_idx"].reshape(-1, 5)
    ipts[np.nonzero(iidx[:, 4] == iidx[0, 4])[0][1], 0] += 1e-3
    bs = solver.BatchSolver([w])                         # create behaves as before
    rc = solver.lib().swf_batch_check_features(bs._h, solver.C.c_double(2.0))
    assert rc == E_INVALID and b"disagree" in solver.lib().swf_last_error()
    bs.close()


@pytest.mark.gpu
def test_state_rules_and_bad_arguments():
    import ctypes as C
    L = solver.lib()
    w = single_window(2, 11, 8)
    bs = solver.BatchSolver([w])
    nfeat = C.c_int32(-1)
    get = lambda wi: L.swf_batch_get_feature_check(bs._h, C.c_int32(wi), None, None, None, None, None, None, C.byref(nfeat))
    assert get(0) == E_STATE                                             # before any check
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.swf_batch_check_features(bs._h, C.c_double(bad)) == E_INVALID
    assert L.swf_batch_check_features(None, C.c_double(2.0)) == E_INVALID
    assert L.swf_batch_check_features(bs._h, C.c_double(2.0)) == 0       # upload-only state
    assert get(0) == 0 and nfeat.value == w.n_lm
    assert get(1) == E_INVALID and get(-1) == E_INVALID
    bs.solve(default_options())
    assert get(0) == E_STATE                                             # invalidated by the solve
    assert L.swf_batch_check_features(bs._h, C.c_double(2.0)) == 0 and get(0) == 0
    bs.upload_state()
    assert get(0) == E_STATE
    assert L.swf_batch_check_features(bs._h, C.c_double(2.0)) == 0 and get(0) == 0
    bs.reset_state()
    assert get(0) == E_STATE
    bs.close()
    # a window without features is valid
    with np.errstate(all="ignore"):
        we = synth.make_window(2, F=0, seed=11)
    assert we.n_lm == 0 and we.a["proj_idx"].size == 0
    be = solver.BatchSolver([we])
    r = be.check_features(2.0)[0]
    assert r["n_feat"] == 0 and r["rejected"].size == 0
    be.close()


@pytest.mark.gpu
def test_problem_api_by_key():
    """problem_from_window + CheckFeatures: the referee's answer at the problem's solved blocks, by key; the batch's flags."""
    w = single_window(2, 13, 8)
    P, blocks = solver.problem_from_window(w)
    with pytest.raises(solver.SwfError):
        P.CheckFeatures()                                # before a solve
    P.Solve(default_options())
    get, rejected = P.CheckFeatures(2.0)
    ws = w.copy()
    ws.set_state(dict(pose=np.array(blocks[:w.n_pose]), sb=np.array(blocks[w.n_pose:w.n_pose + w.n_sb]),
                      lm=np.array(blocks[w.bid_lm(0):w.bid_lm(0) + w.n_lm]), sc=np.concatenate(blocks[w.bid_sc(0):]) if w.n_sc else np.zeros(0)))
    rows = [get(blocks[w.bid_lm(l)]) for l in range(w.n_lm)]
    got = dict(n_feat=w.n_lm, mean_err=np.array([r["mean_err"] for r in rows]), depth=np.array([r["depth"] for r in rows]),
               n_obs=np.array([r["n_obs"] for r in rows], np.int32), flags=np.array([r["flags"] for r in rows], np.uint8),
               rejected=np.array([l for l in range(w.n_lm) if blocks[w.bid_lm(l)].ctypes.data in rejected], np.int32))
    assert [blocks[w.bid_lm(l)].ctypes.data for l in got["rejected"]] == rejected          # feature order
    assert_matches_referee(ws, got, label="problem")
    assert len(rejected) >= 1
    wb = w.copy()
    bs, res = solve_and_check([wb])
    assert np.array_equal(res[0]["flags"], got["flags"])
    bs.close()
    import ctypes as C
    m = C.c_double()
    rc = solver.lib().swf_problem_get_feature_check(P._h, blocks[0].ctypes.data_as(solver._pd), C.byref(m), None, None, None)
    assert rc == E_NOTFOUND                              # a pose is no feature
    P.close()


@pytest.mark.gpu
def test_outliers_adapter_run_matches_referee(tmp_path):
    exe = compile_shim(tmp_path, "shim_outliers")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    failed = [int(v) for v in re.search(r"^failed \d+:(.*)$", out.stdout, re.M).group(1).split()]
    pose1 = [float(v) for v in re.search(r"^pose1 (.*)$", out.stdout, re.M).group(1).split()]
    pts = {int(m.group(1)): [float(v) for v in m.group(2).split()] for m in re.finditer(r"^point (\d+) (\S+ \S+ \S+) mean", out.stdout, re.M)}
    mean = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"^point (\d+) .* mean (\S+) depth", out.stdout, re.M)}
    # the shim's window, restated
    n, bad = 6, 4
    pt0 = np.array([[0.5, 0.3, 6], [-0.4, 0.2, 7], [0.2, -0.5, 8], [-0.3, -0.3, 9], [0.6, -0.2, 7.5], [-0.1, 0.4, 6.5]])
    idx, uv = [], []
    for i in range(n):
        dy = 0.04 if i == bad else 0.0
        idx += [[0, 2, i], [1, 2, i]]
        uv += [[pt0[i, 0] / pt0[i, 2], pt0[i, 1] / pt0[i, 2] + dy], [(pt0[i, 0] - 0.4) / pt0[i, 2] + 1e-3, pt0[i, 1] / pt0[i, 2] - dy]]
    w = FlatWindow(pose=np.array([[0, 0, 0, 0, 0, 0, 1.0], pose1, [0, 0, 0, 0, 0, 0, 1.0]]), lm=np.array([pts[i] for i in range(n)]),
                   sc=np.zeros(1), is_const=np.zeros(3 + n + 1, np.uint8), proj_idx=np.array(idx, np.int32), proj_uv=np.array(uv), pbg=np.zeros(3))
    ref = nf.check(w)
    assert failed == list(ref["rejected"]) and failed == [bad]
    for i in range(n):
        assert abs(mean[i] - ref["mean_err"][i]) <= M_TOL * EPS * (1 + ref["cond"][i]), i
