"""The three stand-alone producer kernels of csrc/swf_producers.hip against longdouble referees with a bound per compared quantity:
k_preintegrate (solver.preintegrate_batch, solver.preintegrate_runs_batch), k_triangulate (solver.triangulate_batch) and k_eval_idepth
(solver.eval_inverse_depth_batch).  Referees: tests/np_producers.py (plain numpy from the reference's lines, dtype = float64 or
longdouble); inputs: tests/producer_cases.py.

A compared quantity q of the device must lie within M x 2^-52 x bracket(q) of the longdouble referee.  The brackets are derived in
np_producers.py's docstrings (pre-integration: push_backs x the largest magnitude the quantity's own recursion terms reach, sqrt_info
rows with the covariance's scaled condition number; triangulation: first-order perturbation of the smallest right singular vector;
inverse depth: the magnitudes of the terms summed, 1 / z where the projection divides).  M is measured on the CPU, never on the device:
M = ceil(8 x the largest ratio, over the inputs below and two float64 operation orders, of |float64 referee - longdouble referee| to
2^-52 x bracket); the 8 is the project's margin for a further legitimate order, FMA contraction and the last ulp of a reciprocal square
root.  A bracket is sharp when that largest ratio lies in [1/32, 4].  Measured (test_*_tolerance_constant_is_the_measured_one print them):

  pre-integration  dp 0.22  dq 0.74  dv 0.52  sum_dt 0.18  dp_dba 1.01  dp_dbg 1.78  dq_dbg 0.23  dv_dba 0.74  dv_dbg 1.61
                   sqrt_info rows 0.16  (the largest ones on one-push_back intervals)        largest 1.78 -> M_PRE = 15
  triangulation    depth 0.27, world 0.68 with the one-sided Jacobi in float64; depth 5.45, world 5.18 with LAPACK's SVD: one
                   feature of 600 (0.17 m deep, the next largest is 3.2) leaves the window's upper end.  The bracket is the
                   first-order one as specified and is not inflated for it; the measured ratio sets M.      largest 5.45 -> M_TRI = 44
  inverse depth    r 0.29  J_pose_i 0.15  J_pose_j 0.13  J_ex 0.17  J_ex2 0.29  J_lambda 0.13            largest 0.29 -> M_IDP = 3

The oracle (oracle/swf_oracle.c through oracle_binding) is held to the same bounds on the CPU; its sqrt_info alone takes the reference's
explicit-inverse route and is held to push_backs x cond(covariance) x 2^-52 x the row's largest entry instead.

Largest device deviation on MI355X, in units of the bracket: pre-integration 1.781 (dp_dbg of a one-push_back interval; sqrt_info rows
0.192; over runs 0.430), triangulation 0.684 (world point; depth 0.272), inverse depth 0.562 (J_pose_i); every GPU test prints
`deviation / bracket`.  Adding 2 M x 2^-52 x bracket to one expected value (dp_dbg of the 3-sample interval: 1.3e-14 of the block's largest
entry; a sqrt_info row; a depth; a world coordinate; an entry of J_ex, J_lambda, J_pose_i) made the corresponding GPU test fail."""
import functools
import math

import numpy as np
import pytest

import np_producers as npp
import producer_cases as pc

EPS = 2.0 ** -52
M_PRE, M_TRI, M_IDP = 15.0, 44.0, 3.0
SHARP = (1.0 / 32, 4.0)
# central differences in longdouble with a step of h_rel = 1e-6 of the smallest depth in play: truncation (h_rel L)^2 with L <= 30 the
# largest lever-arm-to-depth ratio of the inputs, rounding 2^-63 / h_rel: together below 1e-9 of the bracket; a wrong term of a Jacobian
# shows at 1e-2 of it or more
FD_TOL = 1e-9
# the first-order bracket of the triangulation holds while the second-order term, eps / gap relative to it, is negligible
TRI_MIN_GAP = 2.0 ** -26
JNAMES = ("J_pose_i", "J_pose_j", "J_ex", "J_ex2", "J_lambda")

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps,
                                      reason="np.longdouble is no wider than float64 on this platform")


def _ld(a):
    return np.asarray(a).astype(np.longdouble)


def _ratio(dev, ref, bracket):
    """|dev - ref| / (2^-52 bracket), elementwise; a zero deviation counts as 0 whatever the bracket"""
    d = np.abs(_ld(dev) - _ld(ref)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / (EPS * np.asarray(bracket, np.float64)))


# ---------------------------------------------------------------------------------------------------------------- referees, cached
ZERO_NOISE = (0.0, 0.0, 0.0, 0.0)


def _pre_inputs():
    """(name, samples, bias, noise) of every interval the pre-integration tests use: the cases, the gathered runs, one zero-noise call"""
    out = [(c["name"], c["samples"], c["bias"], pc.NOISE) for c in pc.preint_cases()]
    _, _, rows, bias = pc.preint_runs_case()
    out += [("runs%d" % i, rows[i], bias[i], pc.NOISE) for i in range(len(rows))]
    out += [(c["name"], c["samples"], c["bias"], pc.NOISE) for c in pc.one_push_back_cases()]
    c = pc.preint_cases()
    out += [("zero_noise_" + c[k]["name"], c[k]["samples"], c[k]["bias"], ZERO_NOISE) for k in (2, 3, 6)]
    return out


@functools.lru_cache(maxsize=None)
def pre_ref(dtype="longdouble", order="reference"):
    dt = np.longdouble if dtype == "longdouble" else np.float64
    return {name: npp.preintegrate(s, b[:3], b[3:], nz, dt, order) for name, s, b, nz in _pre_inputs()}


@functools.lru_cache(maxsize=None)
def tri_ref(which="scene", dtype="longdouble", order="reference"):
    sc = pc.tri_scene() if which == "scene" else pc.tri_two_frames()
    dt = np.longdouble if dtype == "longdouble" else np.float64
    return npp.triangulate(*pc.tri_args(sc), init_depth=pc.INIT_DEPTH, dtype=dt, order=order)


def _idp_args(F, q):
    P = F["poses"][4 * q:4 * q + 4]
    return (int(F["kind"][q]), P[0], P[1], P[2], P[3], F["lam"][q], F["pts"][q, :3], F["pts"][q, 3:], pc.SQRT_INFO, pc.PBG)


@functools.lru_cache(maxsize=None)
def idp_ref(dtype="longdouble"):
    F = pc.idepth_factors()
    dt = np.longdouble if dtype == "longdouble" else np.float64
    return [npp.eval_idepth(*_idp_args(F, q), dtype=dt, fd=(dtype == "longdouble")) for q in range(len(F["kind"]))]


# ---------------------------------------------------------------------------------------------------------------- comparisons
def pre_ratios(rec, ref):
    """name -> deviation / bracket of one record against one longdouble referee result (sqrt_info: the largest over its rows)"""
    return {k: v / EPS for k, v in npp.record_ratios(np.asarray(rec), ref).items()}


def check_record(rec, ref, M, label, sqrt_info_bracket=None):
    """one 293-double record against the longdouble referee: the copied fields exactly, every compared quantity within M x bracket,
    sqrt_info upper triangular with a positive diagonal, or all zero where the covariance is rank-deficient.  Returns the ratios."""
    rec = np.asarray(rec, np.float64)
    e = ref["record"]
    for off, n in ((npp.LBA, 3), (npp.LBG, 3), (npp.GYRI, 3), (npp.GYRJ, 3)):
        assert np.array_equal(rec[off:off + n], e[off:off + n].astype(np.float64)), (label, off)
    U = rec[npp.SQRTINFO:].reshape(15, 15)
    if not ref["regular"]:
        assert not U.any(), (label, "sqrt_info of a rank-deficient covariance must be zero")
    else:
        assert np.all(np.tril(U, -1) == 0) and np.all(np.diag(U) > 0), label
    r = pre_ratios(rec, ref)
    if sqrt_info_bracket is not None and ref["regular"]:
        r["sqrt_info"] = float(_ratio(U, e[npp.SQRTINFO:].reshape(15, 15), sqrt_info_bracket[:, None]).max())
    for k, v in r.items():
        assert v <= M, (label, k, v)
    return r


def tri_classes(ref):
    """(decided, undecided, excluded) masks over the in-range features of a longdouble triangulation"""
    bd = ref["bracket_depth"]
    ok = ref["in_range"] & np.isfinite(bd) & (ref["gap"] >= TRI_MIN_GAP)
    with np.errstate(invalid="ignore"):
        far = np.abs(ref["raw_depth"]).astype(np.float64) >= 4 * M_TRI * EPS * bd
    return ok & far, ok & ~far, ref["in_range"] & ~ok


def check_triangulation(depth, world, ref, M, label):
    """device (or oracle) depth / world against the longdouble referee; returns (ratio of depth, ratio of world) over the decided features"""
    depth, world = np.asarray(depth), np.asarray(world)
    dec, und, exc = tri_classes(ref)
    out = ~ref["in_range"]
    assert np.all(depth[out] == -1.0) and not world[out].any(), label
    loose = und | exc
    assert np.all(np.isfinite(depth[loose])) and np.all(np.isfinite(world[loose])) and np.all(depth[loose] > 0), label
    # the branch, exactly
    pos = ref["positive"]
    assert np.array_equal(depth[dec & ~pos], np.full((dec & ~pos).sum(), pc.INIT_DEPTH)), label
    rd = _ratio(depth[dec], ref["depth"][dec], ref["bracket_depth"][dec])
    rd = np.where(pos[dec], rd, 0.0)
    rw = _ratio(world[dec], ref["world"][dec], ref["bracket_world"][dec])
    assert rd.max() <= M, (label, "depth", float(rd.max()), int(np.nonzero(dec)[0][np.argmax(rd)]))
    assert rw.max() <= M, (label, "world", float(rw.max()), int(np.nonzero(dec)[0][np.argmax(rw.max(axis=1))]))
    return float(rd.max()), float(rw.max())


def check_idepth(r, J, refs, M, label):
    """device (or oracle) r [n][2], J [n][50] against refs[:n]; the blocks a kind does not have exactly zero.  Returns name -> ratio."""
    F = pc.idepth_factors()
    worst = dict(r=0.0, **{k: 0.0 for k in JNAMES})
    for q in range(len(r)):
        ref, k = refs[q], int(F["kind"][q])
        got = (J[q, 0:12].reshape(2, 6), J[q, 12:24].reshape(2, 6), J[q, 24:36].reshape(2, 6), J[q, 36:48].reshape(2, 6), J[q, 48:50])
        if k == 2:
            assert not got[0].any() and not got[1].any(), (label, q)
        if k == 0:
            assert not got[3].any(), (label, q)
        worst["r"] = max(worst["r"], float(_ratio(r[q], ref["r"], ref["br_r"]).max()))
        for b, name in enumerate(JNAMES):
            worst[name] = max(worst[name], float(_ratio(got[b], ref["J"][b], ref["br_J"][b]).max()))
        for name, v in worst.items():
            assert v <= M, (label, q, k, name, v)
    return worst


def _show(title, ratios):
    print("%s deviation / bracket: %s" % (title, "  ".join("%s %.3f" % (k, v) for k, v in ratios.items())))


def _measured(M, worst):
    """M is 8 x the largest measured ratio, rounded up to the next integer: neither smaller nor padded"""
    assert 8.0 * worst <= M, (M, worst)
    assert M == float(math.ceil(8.0 * worst)), (M, worst)


# ---------------------------------------------------------------------------------------------------------------- CPU tests
@needs_longdouble
def test_preintegration_tolerance_constant_is_the_measured_one():
    """float64 referee in both operation orders against the longdouble referee on every interval the tests use: per compared
    quantity the largest ratio lies in [1/32, 4] (the bracket is sharp) and M_PRE = ceil(8 x the largest of them)."""
    ld = pre_ref("longdouble")
    worst = {}
    for order in ("reference", "alt"):
        f = pre_ref("float64", order)
        for name in ld:
            assert f[name]["regular"] == ld[name]["regular"], name
            for k, v in pre_ratios(f[name]["record"], ld[name]).items():
                worst[k] = max(worst.get(k, 0.0), v)
    _show("pre-integration, float64 referee:", worst)
    for k, v in worst.items():
        assert SHARP[0] <= v <= SHARP[1], (k, v)
    print("M_PRE = %d" % math.ceil(8 * max(worst.values())))
    _measured(M_PRE, max(worst.values()))
    # the inputs do what they are there for
    assert {n for n in ld if not ld[n]["regular"]} >= {"len1", "len2", "one_sample", "one_push_back", "one_push_back_b", "push_back_then_dt0",
                                                          "zero_noise_len3", "zero_noise_len41", "zero_noise_len17"}
    conds = [ld[n]["cond"] for n in ld if ld[n]["regular"]]
    print("scaled condition number of the covariance: %.1f .. %.1f" % (min(conds), max(conds)))
    assert max(conds) < 400


@needs_longdouble
def test_sqrt_info_routes_agree_in_longdouble():
    """The inverse of the reverse Cholesky factor (the device's route) is the matrix the reference forms, LLT(cov^-1).matrixL()^T: in
    longdouble the two agree per row to 60 roundings (two factorisations and two triangular solves of a 15 x 15) x the scaled condition
    number: ten thousand times closer than the bound the device is held to."""
    epl = float(np.finfo(np.longdouble).eps)
    worst = 0.0
    for name, ref in pre_ref("longdouble").items():
        if not ref["regular"]:
            continue
        Ua, Ub = ref["record"][npp.SQRTINFO:].reshape(15, 15), ref["sqrt_info_b"]
        assert np.all(np.tril(Ub, -1) == 0)
        dev = (np.abs(Ua - Ub).max(axis=1) / np.abs(Ua).max(axis=1)).astype(np.float64) / (epl * ref["cond"])
        worst = max(worst, float(dev.max()))
        assert dev.max() <= 60, (name, float(dev.max()))
        # and it is the square root of the information matrix: U^T U cov = I
        C = ref["covariance"]
        d = 1 / np.sqrt(np.diag(C))
        res = np.abs(((Ua.T @ Ua) / np.outer(d, d)) @ (C * np.outer(d, d)) - np.eye(15)).astype(np.float64).max()
        assert res <= 60 * 15 * epl * ref["cond"], (name, res)
    print("largest row deviation between the two routes: %.2f x 2^-63 x cond" % worst)


@needs_longdouble
def test_triangulation_tolerance_constant_is_the_measured_one():
    """float64 one-sided Jacobi and float64 LAPACK SVD against the longdouble Jacobi over the decided features of both scenes."""
    worst = {}
    for which in ("scene", "two"):
        ld = tri_ref(which)
        dec, _, _ = tri_classes(ld)
        for order in ("reference", "alt"):
            f = tri_ref(which, "float64", order)
            assert np.array_equal(f["positive"][dec], ld["positive"][dec]), (which, order)
            rd = np.where(ld["positive"][dec], _ratio(f["depth"][dec], ld["depth"][dec], ld["bracket_depth"][dec]), 0.0)
            rw = _ratio(f["world"][dec], ld["world"][dec], ld["bracket_world"][dec])
            for k, v in (("depth", rd.max()), ("world", rw.max())):
                worst[(order, k)] = max(worst.get((order, k), 0.0), float(v))
    _show("triangulation, float64 referee:", {"%s/%s" % k: v for k, v in worst.items()})
    for k in ("depth", "world"):
        assert SHARP[0] <= worst[("reference", k)] <= SHARP[1], (k, worst)
        assert worst[("alt", k)] >= SHARP[0]
    print("M_TRI = %d" % math.ceil(8 * max(worst.values())))
    _measured(M_TRI, max(worst.values()))


@needs_longdouble
def test_triangulation_inputs_are_decisive():
    """Of the features that are not degenerate by construction at most 2 % are undecided (depth within 4 M brackets of zero) or
    excluded (no gap between the two smallest singular values); the degenerate ones are what their names say."""
    for which, sc in (("scene", pc.tri_scene()), ("two", pc.tri_two_frames())):
        ld = tri_ref(which)
        dec, und, exc = tri_classes(ld)
        plain = sc["tag"] == ""
        loose = (und | exc) & plain
        print("%s: %d features, %d not degenerate by construction, of those %d undecided or excluded" % (which, len(plain), plain.sum(), loose.sum()))
        assert loose.sum() <= 0.02 * plain.sum()
        assert not ld["in_range"][sc["tag"] == "out_of_range"].any() and ld["in_range"][sc["tag"] != "out_of_range"].all()
    sc, ld = pc.tri_scene(), tri_ref("scene")
    dec, und, exc = tri_classes(ld)
    assert und[sc["tag"] == "pure_rotation"].all()                  # one camera centre: the rays meet in it, depth 0
    assert (dec & ~ld["positive"])[sc["tag"] == ""].sum() >= 3       # behind-the-camera solutions among the decided ones
    d = np.abs(ld["raw_depth"][dec & (sc["tag"] == "")]).astype(np.float64)
    assert d.min() < 0.25 and d.max() > 250
    assert set(int(s) for s in sc["start"][dec]) >= {0, len(sc["Ps"]) - 2}
    assert pc.tri_two_frames()["Ps"].shape[0] == 2


@needs_longdouble
def test_inverse_depth_tolerance_constant_is_the_measured_one():
    ld, f = idp_ref("longdouble"), idp_ref("float64")
    worst = dict(r=0.0, **{k: 0.0 for k in JNAMES})
    for a, b in zip(f, ld):
        worst["r"] = max(worst["r"], float(_ratio(a["r"], b["r"], b["br_r"]).max()))
        for i, name in enumerate(JNAMES):
            worst[name] = max(worst[name], float(_ratio(a["J"][i], b["J"][i], b["br_J"][i]).max()))
    _show("inverse depth, float64 referee:", worst)
    for k, v in worst.items():
        assert SHARP[0] <= v <= SHARP[1], (k, v)
    print("M_IDP = %d" % math.ceil(8 * max(worst.values())))
    _measured(M_IDP, max(worst.values()))
    F = pc.idepth_factors()
    z = np.array([r["z"] for r in ld])
    assert np.allclose(z[30:42], pc.Z_NEAR, rtol=1e-9) and set(F["lam"]) >= set(pc.LAMBDAS)


@needs_longdouble
def test_inverse_depth_referee_jacobians_are_the_derivatives():
    """Every analytic block of the longdouble referee against central differences of its residual on the manifold, within FD_TOL of the
    block's bracket: the referee the device is judged by is itself checked against the definition of a Jacobian."""
    worst = 0.0
    for q, ref in enumerate(idp_ref("longdouble")):
        for b, name in enumerate(JNAMES):
            d = np.abs(ref["J"][b] - ref["J_fd"][b]).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = float(np.where(d == 0, 0.0, d / ref["br_J"][b]).max())
            worst = max(worst, r)
            assert r <= FD_TOL, (q, name, r)
    print("largest |analytic - central difference| / bracket: %.2e (bound %.0e)" % (worst, FD_TOL))


@needs_longdouble
def test_oracle_against_the_referees():
    """The C oracle at the bounds the device is held to.  Its sqrt_info goes through an explicit inverse: push_backs x cond(covariance)
    instead of the scaled condition number."""
    import oracle_binding as ob
    worst = {}
    for name, s, b, nz in _pre_inputs():
        ref = pre_ref("longdouble")[name]
        rec = ob.preintegrate(s, b[:3], b[3:], *nz)
        sb = None
        if ref["regular"]:
            U = ref["record"][npp.SQRTINFO:].reshape(15, 15).astype(np.float64)
            sb = ref["n_pb"] * float(np.linalg.cond(ref["covariance"].astype(np.float64))) * np.abs(U).max(axis=1)
        for k, v in check_record(rec, ref, M_PRE, "oracle " + name, sqrt_info_bracket=sb).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show("oracle, pre-integration:", worst)
    for which, sc in (("scene", pc.tri_scene()), ("two", pc.tri_two_frames())):
        d, W = ob.triangulate(*pc.tri_args(sc), init_depth=pc.INIT_DEPTH)
        rd, rw = check_triangulation(d, W, tri_ref(which), M_TRI, "oracle " + which)
        _show("oracle, triangulation (%s):" % which, dict(depth=rd, world=rw))
    F = pc.idepth_factors()
    n = len(F["kind"])
    r, J = np.zeros((n, 2)), np.zeros((n, 50))
    for q in range(n):
        k, Pi, Pj, ex, ex2, lam, pts_i, pts_j, si, pbg = _idp_args(F, q)
        ro, Ji, Jj, Jex, Jex2, Jl = ob.eval_proj_idepth(k, Pi, Pj, ex, ex2, lam, pts_i, pts_j, si, pbg)
        z = np.zeros((2, 6))
        r[q] = ro
        J[q] = np.concatenate([(Ji if k != 2 else z).ravel(), (Jj if k != 2 else z).ravel(), Jex.ravel(), (Jex2 if k != 0 else z).ravel(), Jl])
    _show("oracle, inverse depth:", check_idepth(r, J, idp_ref("longdouble"), M_IDP, "oracle"))


# ---------------------------------------------------------------------------------------------------------------- GPU tests
def _solver():
    from rtk_visual_inertial_navigation_amd import solver
    return solver


@pytest.mark.gpu
def test_gpu_preintegration_matches_the_longdouble_referee():
    """All intervals as one batch (wavefronts of very different lengths) against the longdouble referee, per block of the record; the
    same intervals in calls of 1, 3, 4 and 5 and in reverse order: a record does not depend on the batch it came in, bit for bit; all-zero
    noise densities leave sqrt_info zero and the rest of the record as it was.
    Largest device deviation on MI355X, in units of the bracket: 1.061 (dp_dbg), sqrt_info rows 0.192."""
    solver = _solver()
    cases = pc.preint_cases()
    ld = pre_ref("longdouble")
    smp, bias = [c["samples"] for c in cases], np.array([c["bias"] for c in cases])
    got = solver.preintegrate_batch(smp, bias, pc.NOISE)
    worst = {}
    for i, c in enumerate(cases):
        for k, v in check_record(got[i], ld[c["name"]], M_PRE, c["name"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show("pre-integration, device:", worst)
    for m in pc.PREINT_SUBBATCHES:
        for i0 in range(0, len(cases), m):
            part = solver.preintegrate_batch(smp[i0:i0 + m], bias[i0:i0 + m], pc.NOISE)
            assert np.array_equal(part, got[i0:i0 + m]), (m, i0)
    rev = solver.preintegrate_batch(smp[::-1], bias[::-1], pc.NOISE)
    assert np.array_equal(rev[::-1], got)
    # all-zero noise densities: the covariance is zero, sqrt_info is zero, everything else as before
    ks = (2, 3, 6)
    zn = solver.preintegrate_batch([smp[k] for k in ks], bias[list(ks)], ZERO_NOISE)
    for j, k in enumerate(ks):
        check_record(zn[j], ld["zero_noise_" + cases[k]["name"]], M_PRE, "zero noise " + cases[k]["name"])
        assert np.array_equal(zn[j][:npp.SQRTINFO], got[k][:npp.SQRTINFO]) and not zn[j][npp.SQRTINFO:].any()


@pytest.mark.gpu
def test_gpu_one_push_back_never_yields_a_sqrt_info():
    """96 intervals of one push_back: the covariance has rank 12 by construction (rows 0-2 of V are dt / 2 times rows 6-8), so the last
    three pivots of its factorisation are rounding residue of either sign.  sqrt_info must be zero for every one of them, as the oracle
    and the referee have it; a test on the residue's sign lets about one interval in ten through with entries of 1e13 and more (14 of
    these 96 on MI355X before the kernel compared the pivot with its own diagonal entry).  The rest of the record is held to its brackets
    as everywhere.
    Largest device deviation on MI355X, in units of the bracket: 1.781 (dp_dbg), 1.605 (dv_dbg)."""
    solver = _solver()
    cases = pc.one_push_back_cases()
    ld = pre_ref("longdouble")
    got = solver.preintegrate_batch([c["samples"] for c in cases], np.array([c["bias"] for c in cases]), pc.NOISE)
    bad = [c["name"] for i, c in enumerate(cases) if got[i][npp.SQRTINFO:].any()]
    print("one push_back: %d of %d intervals came back with a non-zero sqrt_info" % (len(bad), len(cases)))
    assert not bad, bad
    worst = {}
    for i, c in enumerate(cases):
        for k, v in check_record(got[i], ld[c["name"]], M_PRE, c["name"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show("pre-integration, one push_back, device:", worst)


@pytest.mark.gpu
def test_gpu_preintegration_over_runs_matches_the_longdouble_referee():
    """swf_preintegrate_runs_batch on two-run gathers against the referee on the concatenated rows, and bitwise against the contiguous kernel.
    Largest device deviation on MI355X, in units of the bracket: 0.430 (dp_dbg)."""
    solver = _solver()
    pool, runs, rows, bias = pc.preint_runs_case()
    got = solver.preintegrate_runs_batch(pool, runs, bias, pc.NOISE)
    ld = pre_ref("longdouble")
    worst = {}
    for i in range(len(runs)):
        for k, v in check_record(got[i], ld["runs%d" % i], M_PRE, "runs%d" % i).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show("pre-integration over runs, device:", worst)
    assert np.array_equal(got, solver.preintegrate_batch(rows, bias, pc.NOISE))


@pytest.mark.gpu
def test_gpu_triangulation_matches_the_longdouble_referee():
    """1, 255, 256, 257 and 600 features (256 lanes per block) and the two-frame scene: depth and world point of every decided feature
    within M_TRI brackets, the depth > 0 branch exactly, out-of-range starts flagged, the undecided finite and positive; a feature's
    result does not depend on how many features the call has.
    Largest device deviation on MI355X, in units of the bracket: 0.684 (world point), 0.272 (depth)."""
    solver = _solver()
    sc = pc.tri_scene()
    d, W = solver.triangulate_batch(*pc.tri_args(sc), init_depth=pc.INIT_DEPTH)
    rd, rw = check_triangulation(d, W, tri_ref("scene"), M_TRI, "scene")
    _show("triangulation, device (600 features):", dict(depth=rd, world=rw))
    for n in pc.TRI_COUNTS[:-1]:
        dn, Wn = solver.triangulate_batch(*pc.tri_args(sc, n), init_depth=pc.INIT_DEPTH)
        assert np.array_equal(dn, d[:n]) and np.array_equal(Wn, W[:n]), n
    s2 = pc.tri_two_frames()
    d2, W2 = solver.triangulate_batch(*pc.tri_args(s2), init_depth=pc.INIT_DEPTH)
    rd, rw = check_triangulation(d2, W2, tri_ref("two"), M_TRI, "two frames")
    _show("triangulation, device (two frames):", dict(depth=rd, world=rw))


@pytest.mark.gpu
def test_gpu_inverse_depth_matches_the_longdouble_referee():
    """1, 127, 128, 129 and 300 factors (128 lanes per block), kinds mixed, lambda from 1e-3 to 5, points 0.05 in front of the camera: the
    residual and every Jacobian block within M_IDP of its own bracket; the blocks a kind does not have exactly zero.
    Largest device deviation on MI355X, in units of the bracket: 0.562 (J_pose_i), residual 0.274."""
    solver = _solver()
    F = pc.idepth_factors()
    refs = idp_ref("longdouble")
    r, J = solver.eval_inverse_depth_batch(F["kind"], F["idx"], F["poses"], F["lam"], F["pts"], pc.SQRT_INFO, pc.PBG)
    _show("inverse depth, device (300 factors):", check_idepth(r, J, refs, M_IDP, "device"))
    for n in pc.IDEPTH_COUNTS[:-1]:
        rn, Jn = solver.eval_inverse_depth_batch(F["kind"][:n], F["idx"][:n], F["poses"][:4 * n], F["lam"][:n], F["pts"][:n], pc.SQRT_INFO, pc.PBG)
        assert np.array_equal(rn, r[:n]) and np.array_equal(Jn, J[:n]), n
