"""The single-epoch GNSS solve on the device (swf_gnss_epoch_solve_batch / solver.gnss_epoch_solve_batch / swf_ceres::GnssEpochSolve): the
seed mini-solve of GnssPreprocess (R/swf/swf_gnss.cpp:534-575) and the first fix of GnssProcess (:203-215) against the longdouble referee
of tests/np_gnss_epoch.py on the inputs of tests/gnss_epoch_gen.py.

status, iters and clk_rows are compared exactly: by the longdouble referee no step of any input lies within a factor of ten of step_tol
and no relative pivot between 1e-12 and 1e-5 (test_inputs_are_decisive), while rounding is ~1e-8 m.

Tolerance (computed here, not fitted to the device; test_tolerance_is_measured_on_the_cpu prints it).  Per call, epoch and output quantity:
the largest deviation from the longdouble referee of the float64 structured referee with the records summed in 8 random orders and of the
float64 dense form, times 8, with a floor of one ulp (2^-52) of the quantity's bracket |xg| + |sat| + |obs| + |clk| (divided by lam for N,
times w for r).  cost and info are compared relatively (info against sum w^2 of the rows of the reduced system) with their own measured unit and a floor of one
ulp.  The measured unit of pos / clock is 1e-9 to 1e-8 m on these inputs.
Largest device deviation on MI355X: 0.134 of the tolerance (clock, 'no ambiguity free'), i.e. 1.07 x the float64 referee's own spread;
every GPU test prints it (`deviation / tol`)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gnss_epoch_gen as gg
import np_factors as npf
import np_gnss_epoch as nge
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import build, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
LD = np.longdouble
E_INVALID, E_UNSUPPORTED = -2, -3
SIZES = [0, 1, 2, 63, 64, 65, 129, 512]
STEP_TOL, EPS_RANK = 1e-4, 1e-8
N_ORDERS = 8
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
FLOAT_KEYS = ("pos", "vel", "clock", "N", "r", "cost", "info")
EXACT_KEYS = ("iters", "status", "clk_rows")


# ---------------------------------------------------------------------------------------------------------------- inputs
def _filter(e, keep):
    e = dict(e); e["dat"], e["rec"] = e["dat"][keep], e["rec"][keep]
    return e


@functools.lru_cache(maxsize=None)
def calls():
    """{label: (packed arrays, max_iter)} of every call the GPU tests compare with the referee."""
    out = {}
    for preset, kw in (("seed", nge.SEED), ("first_fix", nge.FIRST_FIX)):
        out["sizes, " + preset] = (gg.pack([gg.gen_epoch(100 + n, n, preset) for n in SIZES]), kw["max_iter"])
    for label, e, it in branch_epochs():
        out[label] = (gg.pack([e]), it)
    return out


@functools.lru_cache(maxsize=None)
def branch_epochs():
    b = []
    b.append(("every ambiguity free", gg.gen_epoch(400, 50, "first_fix", all_free=True), 20))
    b.append(("no ambiguity free", gg.gen_epoch(401, 50, "first_fix", none_free=True), 20))
    e = gg.gen_epoch(402, 45, "seed")                              # slot 4 (RTK, system 2): the code rows gone, every phase row free
    e = _filter(e, ~((e["rec"][:, 1] == 4) & (e["rec"][:, 0] == nge.RTK_CODE)))
    e["rec"][(e["rec"][:, 1] == 4), 2] = nge.AMB_FREE
    assert (e["rec"][:, 1] == 4).sum() >= 2
    b.append(("a clock whose rows are all absorbed", e, 2))
    e = gg.gen_epoch(403, 50, "first_fix"); e["clk_const"] = (1 << 12) | (1 << 6); e["clock"] = e["truth"][2] + 0.01
    b.append(("constant clocks, first fix", e, 20))
    e = gg.gen_epoch(404, 40, "seed"); e["clk_const"] = 1 << 2
    b.append(("a constant clock, seed", e, 2))
    e = gg.gen_epoch(405, 50, "first_fix"); e["mode"] = nge.FREE_VEL; e["pos"] = e["truth"][0] + 0.01
    e["vel"] = e["truth"][1] + 0.01       # (the rate's Sagnac term is not differentiated: from 15 m/s off the second step would be ~5e-5)
    b.append(("FREE_VEL without FREE_POS", e, 20))
    e = gg.gen_epoch(406, 12, "first_fix", kinds=(4,)); e["mode"] = nge.FREE_VEL; e["pos"] = e["truth"][0] + 0.01
    e["vel"] = e["truth"][1] + 0.01
    b.append(("Doppler rows only", e, 20))
    e = gg.gen_epoch(407, 60, "first_fix"); e["dat"][::4, 7] = 0.0
    e["dat"][e["rec"][:, 1] == 8, 7] = 0.0                           # and every row of clock 8: it keeps its value
    b.append(("w = 0 rows", e, 20))
    b.append(("max_iter = 1", gg.gen_epoch(408, 50, "first_fix"), 1))
    e = gg.gen_epoch(409, 16, "first_fix", kinds=(0, 1, 2, 3), deficient=True); e["mode"] = nge.FREE_POS
    b.append(("deficient", e, 20))
    return b


@functools.lru_cache(maxsize=None)
def batch_epochs():
    """37 epochs of mixed sizes and presets, at most 64 records each (the call takes the resident instance unless a larger one is appended)."""
    rng = np.random.default_rng(11)
    sizes = rng.integers(40, 65, 37)
    sizes[:6] = [0, 64, 1, 63, 2, 45]
    return [gg.gen_epoch(2000 + i, int(sizes[i]), "seed" if i % 3 == 0 else "first_fix") for i in range(37)]


def referee_call(packed, max_iter, dtype=np.float64, form=nge.solve, **kw):
    return nge.solve_batch(*packed, max_iter=max_iter, step_tol=STEP_TOL, eps_rank=EPS_RANK, dtype=dtype, form=form, **kw)


@functools.lru_cache(maxsize=None)
def referee(label):
    """The longdouble structured referee of a call (computed once, shared by the tests)."""
    packed, it = calls()[label]
    return referee_call(packed, it, LD)


def _epoch_of(first):
    return np.repeat(np.arange(first.size - 1), np.diff(first))


def _per_epoch_max(v, first):
    out = np.zeros(first.size - 1)
    if v.size:
        np.maximum.at(out, _epoch_of(first), v)
    return out


def deviations(packed, ref, got):
    """{quantity: [E] largest deviation of `got` from `ref` per epoch}; cost and info relative (info: to sum w^2 of its rows)."""
    first = packed[0]
    a = lambda k: np.asarray(got[k]).astype(LD) - np.asarray(ref[k]).astype(LD)
    E = first.size - 1
    d = {k: np.abs(a(k)).reshape(E, -1).max(1).astype(np.float64) if E else np.zeros(0) for k in ("pos", "vel", "clock")}
    for k in ("N", "r"):
        d[k] = _per_epoch_max(np.abs(a(k)).astype(np.float64), first)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.abs(np.asarray(ref["cost"]).astype(np.float64))
        d["cost"] = np.where(c > 0, np.abs(a("cost")).astype(np.float64) / c, np.abs(a("cost")).astype(np.float64))
        # info against sum w^2 over the rows of the reduced system, the scale of its entries before the clocks are eliminated (an epoch
        # whose reduced matrix cancels to rounding noise has no scale of its own)
        inc = (packed[8][:, 2] & nge.AMB_FREE) == 0
        m = np.zeros(E)
        np.add.at(m, _epoch_of(first)[inc], packed[7][inc, 7] ** 2)
        di = np.abs(a("info")).reshape(E, -1).max(1).astype(np.float64)
        d["info"] = np.where(m > 0, di / m, di)
    return d


def _ratio(d, t):
    """d / t, 0 where d is 0 (an epoch without records has a zero bracket for N and r)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d == 0, 0.0, d / t)


def floors(packed, ref):
    """one ulp of the bracket of every quantity, per epoch"""
    first, pos, vel, base, clock, mode, cc, dat, rec = packed
    E = first.size - 1
    br = np.asarray(ref["bracket"]).astype(np.float64)
    xg = np.sqrt(((pos + base) ** 2).sum(1))
    b_ep = np.maximum(_per_epoch_max(br, first), xg + np.abs(clock).max(1))
    f = {k: EPS * b_ep for k in ("pos", "vel", "clock")}
    f["N"] = EPS * np.maximum(_per_epoch_max(br / dat[:, 8], first), 0.0)
    f["r"] = EPS * np.maximum(_per_epoch_max(br * dat[:, 7], first), 0.0)
    f["cost"] = np.full(E, EPS); f["info"] = np.full(E, EPS)
    return f


@functools.lru_cache(maxsize=None)
def tolerance(label):
    """{quantity: [E] tol}: 8 x the largest float64 deviation (8 record orders of the structured form, and the dense form) from the
    longdouble referee, floored at one ulp of the bracket.  Also returns the measured units."""
    packed, it = calls()[label]
    ref = referee(label)
    first = packed[0]
    unit = {k: np.zeros(first.size - 1) for k in FLOAT_KEYS}
    rng = np.random.default_rng(5)
    variants = []
    for _ in range(N_ORDERS):
        orders = [rng.permutation(int(first[e + 1] - first[e])) for e in range(first.size - 1)]
        E = first.size - 1
        res = [nge.solve(packed[1][e], packed[2][e], packed[3][e], packed[4][e], int(packed[5][e]), int(packed[6][e]),
                         packed[7][first[e]:first[e + 1]], packed[8][first[e]:first[e + 1]], it, STEP_TOL, EPS_RANK, np.float64, order=orders[e])
               for e in range(E)]
        variants.append(_stack(res))
    dense = referee_call(packed, it, np.float64, nge.solve_dense)
    dense["info"] = ref["info"]                                    # (the dense form has no reduced matrix of its own)
    variants.append(dense)
    for v in variants:
        assert np.array_equal(v["status"], ref["status"]) and np.array_equal(v["iters"], ref["iters"]), label
        d = deviations(packed, ref, v)
        for k in FLOAT_KEYS:
            unit[k] = np.maximum(unit[k], d[k])
    fl = floors(packed, ref)
    return {k: np.maximum(8.0 * unit[k], fl[k]) for k in FLOAT_KEYS}, unit


def _stack(res):
    cat = lambda k: np.concatenate([np.atleast_1d(q[k]) for q in res]) if res else np.zeros(0)
    out = dict(N=cat("N"), r=cat("r"))
    for k in ("pos", "vel", "clock", "cost", "iters", "status", "clk_rows", "info"):
        out[k] = np.array([q[k] for q in res])
    return out


def assert_matches_referee(label, got, packed=None, ref=None, tol=None):
    """`got` (device) against the longdouble referee: status, iters, clk_rows exactly; the rest within the CPU-measured tolerance."""
    packed = calls()[label][0] if packed is None else packed
    ref = referee(label) if ref is None else ref
    tol = tolerance(label)[0] if tol is None else tol
    for k in EXACT_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), (label, k, got[k], ref[k])
    d = deviations(packed, ref, got)
    worst = {k: float(_ratio(d[k], tol[k]).max()) if d[k].size else 0.0 for k in FLOAT_KEYS}
    print("%s: %d epochs, %d records, deviation / tol: %s" % (label, packed[0].size - 1, packed[7].shape[0],
                                                              " ".join("%s %.3f" % (k, worst[k]) for k in FLOAT_KEYS)))
    for k in FLOAT_KEYS:
        assert worst[k] <= 1.0, (label, k, worst[k], d[k], tol[k])
    return worst


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


ALL_KEYS = FLOAT_KEYS + EXACT_KEYS


def epoch_slice(res, first, e):
    lo, hi = int(first[e]), int(first[e + 1])
    out = {k: np.asarray(res[k])[e] for k in ("pos", "vel", "clock", "cost", "iters", "status", "clk_rows", "info")}
    out["N"], out["r"] = res["N"][lo:hi], res["r"][lo:hi]
    return out


def bitwise_equal(a, b):
    return all(np.array_equal(bits(np.atleast_1d(a[k])), bits(np.atleast_1d(b[k]))) for k in ALL_KEYS)


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_gnss_epoch_symbols_exported():
    build.build()
    lib = C.CDLL(solver.LIB_PATH)
    assert hasattr(lib, "swf_gnss_epoch_solve_batch")
    assert "swf_gnss_epoch_solve_batch" in solver.EXPORTED
    assert callable(solver.gnss_epoch_solve_batch) and callable(solver.gnss_epoch_records)
    assert lib.swf_version() >= 111
    hdr = open(os.path.join(ROOT, "include", "swf_solver.h")).read() + open(os.path.join(ROOT, "include", "swf_types.h")).read()
    for s in ("int swf_gnss_epoch_solve_batch(", "SWF_GES_DOUBLES = 10", "#define SWF_GES_NMAX 512", "SWF_GES_AMB_FREE = 1", "SWF_GES_FREE_VEL = 2",
              "SWF_GES_DOPPLER = 4", "SWF_GES_RANK_DEFICIENT = 2", "SWF_GES_CLOCKS = 13"):
        assert s in hdr, s
    assert "GnssEpochSolve(" in open(os.path.join(ROOT, "include", "swf_ceres.hpp")).read()
    assert (solver.GES_DOUBLES, solver.GES_CLOCKS, solver.GES_NMAX) == (nge.DOUBLES, nge.CLOCKS, nge.NMAX)
    assert (solver.GES_RTK_PHASE, solver.GES_RTK_CODE, solver.GES_SPP_CODE, solver.GES_SPP_PHASE, solver.GES_DOPPLER) == (0, 1, 2, 3, 4)
    assert (solver.GES_CONVERGED, solver.GES_MAX_ITER, solver.GES_RANK_DEFICIENT) == (nge.CONVERGED, nge.MAX_ITER, nge.RANK_DEFICIENT)


def test_gnss_epoch_adapter_compiles_as_cxx14(tmp_path):
    """The seed solve and the first fix bind to swf_ceres::GnssEpochSolve under the reference's -std=c++14; without a GPU the shim exits
    non-zero with a message."""
    exe = compile_shim(tmp_path, "shim_gnss_epoch")
    if solver.device_count() == 0:
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode != 0 and "failed" in r.stdout, r.stdout


def test_structured_and_dense_referees_agree_in_longdouble():
    """The absorbed-row shortcut, the scalar clock elimination and the Cholesky of the structured definition give what Gauss-Newton on the
    full Jacobian gives, ambiguity columns included: in longdouble, at every test input, to the rounding of the brackets.  The bound is
    64 ulp (2^-63) of the bracket: a few hundred roundings of that size enter every sum and the reduced systems have cond <= 4e3 in units
    where a rounding of the state is one of the bracket; the largest ratio seen is printed."""
    assert np.finfo(LD).eps < 2.0 ** -60, "longdouble is not wider than float64 here"
    eps_ld = float(np.finfo(LD).eps)
    worst = 0.0
    for label, (packed, it) in calls().items():
        a = referee(label)
        b = referee_call(packed, it, LD, nge.solve_dense)
        for k in EXACT_KEYS:
            assert np.array_equal(a[k], b[k]), (label, k)
        b["info"] = a["info"]
        d = deviations(packed, a, b)
        fl = floors(packed, a)
        # cost = 1/2 sum r^2 moves by sum |r| dr: its unit is sum |r| (bracket w), relative to the cost
        rr, br = np.abs(np.asarray(a["r"]).astype(np.float64)), np.asarray(a["bracket"]).astype(np.float64)
        csum = np.zeros(packed[0].size - 1)
        np.add.at(csum, _epoch_of(packed[0]), rr * br * packed[7][:, 7])
        fl["cost"] = EPS * _ratio(csum, np.asarray(a["cost"]).astype(np.float64))
        for k in ("pos", "vel", "clock", "N", "r", "cost"):
            ratio = float(_ratio(d[k], fl[k] / EPS * eps_ld).max()) if d[k].size else 0.0
            worst = max(worst, ratio)
            assert ratio <= 64.0, (label, k, ratio)
    print("structured against dense in longdouble: largest deviation %.2f ulp of the bracket" % worst)


def test_residuals_are_those_of_the_factors():
    """Per kind, the residual of a record converted by solver.gnss_epoch_records equals np_factors' residual of the factor record (to 4 ulp
    of the bracket times w: the two restatements round the norm differently), and the RTK weights are 1 / sqrt(varerr2)."""
    rng = np.random.default_rng(3)
    k = 6
    e = gg.gen_epoch(77, 30, "seed")
    base, pos, vel, clock = e["base"], e["pos"], e["vel"], e["clock"]
    sat = e["dat"][:k, 0:3]; sv = e["dat"][:k, 3:6]
    rng_obs = np.sqrt(((pos + base - sat) ** 2).sum(1))
    el, dtb, mv, lam, N = rng.uniform(0.45, 1.4, k), rng.uniform(0.0, 1.0, k), rng.uniform(1e-5, 1e-2, k), np.full(k, 0.1903), np.round(rng.uniform(-99, 99, k))
    istd = rng.uniform(0.5, 200.0, k)
    cp = np.column_stack([sat, rng_obs + rng.normal(0, 3, k), lam, el, dtb, mv, np.array([1, 1, 0, 1, 0, 1.0])])
    pr = np.column_stack([sat, rng_obs + rng.normal(0, 3, k), el, dtb, mv * 100])
    spr = np.column_stack([sat, rng_obs + rng.normal(0, 3, k), istd])
    scp = np.column_stack([sat, rng_obs + rng.normal(0, 3, k), istd, lam])
    dop = np.column_stack([sat, sv, rng.normal(0, 300, k), istd])
    slot = lambda lo: rng.integers(lo, lo + 6, k)
    s_cp, s_pr, s_spr, s_scp = slot(0), slot(0), slot(6), slot(6)
    free = np.array([0, 1, 0, 0, 1, 0])
    dat, rec = solver.gnss_epoch_records(cp=(cp, s_cp, N, free), pr=(pr, s_pr), spr=(spr, s_spr), scp=(scp, s_scp, N + 1, free), dop=(dop, None))
    assert dat.shape == (5 * k, nge.DOUBLES) and rec.shape == (5 * k, 4)
    assert rec[:, 0].tolist() == [0] * k + [1] * k + [2] * k + [3] * k + [4] * k and (rec[4 * k:, 1] == 12).all() and not rec[:, 3].any()
    assert rec[:k, 2].tolist() == free.tolist() and rec[3 * k:4 * k, 2].tolist() == free.tolist() and not rec[k:3 * k, 2].any()
    r, _J, _nf, br = nge.evaluate(dat, rec, pos + base, vel, clock)
    pose = np.concatenate([pos, [0, 0, 0, 1.0]]); sb = np.concatenate([vel, np.zeros(6)])
    want = [npf.cp_residual(pose, N[i], clock[s_cp[i]], cp[i], base) for i in range(k)]
    want += [npf.pr_residual(pose, clock[s_pr[i]], pr[i], base) for i in range(k)]
    want += [npf.spr_residual(pose, clock[s_spr[i]], spr[i], base) for i in range(k)]
    want += [npf.scp_residual(pose, clock[s_scp[i]], N[i] + 1, scp[i], base) for i in range(k)]
    want += [npf.dop_residual(sb, clock[12], pose, dop[i], base) for i in range(k)]
    want = np.array(want)
    assert (np.abs(r - want) <= 4 * EPS * br * dat[:, 7]).all(), np.abs(r - want) / (EPS * br * dat[:, 7])
    wcp = np.array([1 / np.sqrt(npf.varerr2(cp[i, 5], cp[i, 6], cp[i, 7])) if cp[i, 8] else 1.0 for i in range(k)])
    wpr = np.array([1 / np.sqrt(npf.varerr2(pr[i, 4], pr[i, 5], pr[i, 6])) for i in range(k)])
    assert np.array_equal(dat[:k, 7], wcp) and np.array_equal(dat[k:2 * k, 7], wpr)


def test_inputs_are_decisive():
    """By the longdouble referee: no step magnitude of any test input lies in [step_tol / 10, 10 step_tol]; every well-posed epoch has its
    smallest relative pivot >= 1e-5 and every deficient one <= 1e-12; and the inputs cover what the issue lists."""
    seen = set()
    todo = [(label, referee(label)) for label in calls()]
    bp = gg.pack(batch_epochs())
    todo.append(("batch", referee_call(bp, 20, LD)))
    for label, ref in todo:
        steps = [s for ep in ref["steps"] for s in ep]
        close = [s for s in steps if STEP_TOL / 10 <= s <= 10 * STEP_TOL]
        piv = ref["pivot"]
        print("%s: steps %s, relative pivots %s" % (label, " ".join("%.1e" % s for s in steps[:12]), " ".join("%.1e" % p for p in piv[:10])))
        assert not close, (label, close)
        for e, st in enumerate(ref["status"]):
            if st == nge.RANK_DEFICIENT:
                assert piv[e] <= 1e-12, (label, e, piv[e])
            else:
                assert piv[e] >= 1e-5, (label, e, piv[e])
            seen.add(int(st))
    assert seen == {nge.CONVERGED, nge.MAX_ITER, nge.RANK_DEFICIENT}
    b = {label: referee(label) for label, _e, _it in branch_epochs()}
    assert b["deficient"]["status"][0] == nge.RANK_DEFICIENT and b["max_iter = 1"]["status"][0] == nge.MAX_ITER
    q = b["a clock whose rows are all absorbed"]
    assert q["clk_rows"][0, 4] == 0 and q["status"][0] == nge.CONVERGED
    assert b["w = 0 rows"]["clk_rows"][0, 8] == 0 and b["w = 0 rows"]["status"][0] == nge.CONVERGED
    for label in ("every ambiguity free", "no ambiguity free", "constant clocks, first fix", "FREE_VEL without FREE_POS", "Doppler rows only"):
        assert b[label]["status"][0] == nge.CONVERGED, label
    for preset in ("seed", "first_fix"):
        ref = referee("sizes, " + preset)
        assert (ref["status"][3:] == nge.CONVERGED).all(), preset
    assert (referee("sizes, first_fix")["iters"][3:] >= 3).all()


def test_tolerance_is_measured_on_the_cpu():
    """Prints the measured float64 unit and the tolerance of every call; the unit of pos and clock stays below 1e-6 m (it is ~1e-8)."""
    for label in calls():
        tol, unit = tolerance(label)
        print("%s: unit %s | tol %s" % (label, " ".join("%s %.2e" % (k, unit[k].max() if unit[k].size else 0) for k in FLOAT_KEYS),
                                       " ".join("%s %.2e" % (k, tol[k].max() if tol[k].size else 0) for k in FLOAT_KEYS)))
        fl = floors(calls()[label][0], referee(label))
        for k in FLOAT_KEYS:
            assert np.isfinite(tol[k]).all() and (tol[k] >= fl[k]).all(), (label, k)
        assert (unit["pos"] < 1e-6).all() and (unit["clock"] < 1e-6).all(), label


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def run_host(packed, max_iter):
    return solver.gnss_epoch_solve_batch(*packed, max_iter=max_iter, step_tol=STEP_TOL, eps_rank=EPS_RANK)


OUT_SPEC = (("pos", 3, np.float64, "E"), ("vel", 3, np.float64, "E"), ("clock", 13, np.float64, "E"), ("N", 1, np.float64, "n"),
            ("r", 1, np.float64, "n"), ("cost", 1, np.float64, "E"), ("iters", 1, np.int32, "E"), ("status", 1, np.int32, "E"),
            ("clk_rows", 13, np.int32, "E"), ("info", 36, np.float64, "E"))
IN_WIDTH = (1, 3, 3, 3, 13, 1, 1, 10, 4)


def make_outs(E, n, fill=-7):
    return {k: np.full(max(E if per == "E" else n, 1) * w, fill, t) for k, w, t, per in OUT_SPEC}


def shape_outs(o, E, n):
    out = {}
    for k, w, _t, per in OUT_SPEC:
        cnt = E if per == "E" else n
        v = o[k][:cnt * w]
        out[k] = v.reshape(cnt, 6, 6) if k == "info" else v.reshape(cnt, w) if w > 1 else v
    return out


def raw_call(packed, max_iter=20, step_tol=STEP_TOL, eps_rank=EPS_RANK, outs=None, n_epochs=None, null_outs=()):
    """the C entry point on host memory; returns (code, raw output buffers pre-filled with -7)"""
    arrs = [np.ascontiguousarray(a) if a is not None else None for a in packed]
    E = (arrs[0].size - 1) if n_epochs is None else n_epochs
    n = arrs[7].shape[0] if arrs[7] is not None else 0
    o = outs or make_outs(E, n)
    p = lambda a: None if a is None else a.ctypes.data_as(pd if a.dtype == np.float64 else pi)
    po = lambda k: None if k in null_outs else p(o[k])
    rc = solver.lib().swf_gnss_epoch_solve_batch(C.c_int32(E), *[p(a) for a in arrs], C.c_int32(max_iter), C.c_double(step_tol), C.c_double(eps_rank),
                                                 *[po(k) for k, _w, _t, _per in OUT_SPEC], C.c_int32(0), None)
    return rc, o


def _hip(call, *args):
    """a HIP runtime call of the runtime libswf_hip.so itself is linked against (its symbols resolve through the library's handle)"""
    rc = getattr(solver.lib(), call)(*args)
    assert rc == 0, (call, rc)


def run_device(packed, max_iter, fill=-7):
    """on_device = 1 over hipMalloc'ed buffers on the null stream; the device output buffers pre-filled with `fill`"""
    first = packed[0]
    E, n = first.size - 1, packed[7].shape[0]
    host_in = [np.ascontiguousarray(a).reshape(-1) if a.size else np.zeros(w, a.dtype) for a, w in zip(packed, IN_WIDTH)]
    host_out = make_outs(E, n, fill)
    bufs = []

    def up(a):
        d = C.c_void_p()
        _hip("hipMalloc", C.byref(d), C.c_size_t(a.nbytes))
        bufs.append(d)
        _hip("hipMemcpy", d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1))          # hipMemcpyHostToDevice
        return d
    try:
        ins = [up(a) for a in host_in]
        o = {k: up(v) for k, v in host_out.items()}
        ty = lambda a: pd if a.dtype == np.float64 else pi
        rc = solver.lib().swf_gnss_epoch_solve_batch(C.c_int32(E), *[C.cast(d, ty(a)) for d, a in zip(ins, host_in)], C.c_int32(max_iter),
                                                     C.c_double(STEP_TOL), C.c_double(EPS_RANK),
                                                     *[C.cast(o[k], ty(host_out[k])) for k, _w, _t, _per in OUT_SPEC], C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in host_out.items():
            _hip("hipMemcpy", C.c_void_p(v.ctypes.data), o[k], C.c_size_t(v.nbytes), C.c_int(2))   # hipMemcpyDeviceToHost
    finally:
        for d in bufs:
            solver.lib().hipFree(d)
    return shape_outs(host_out, E, n)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["seed", "first_fix"])
def test_epoch_sizes_match_referee(preset):
    """Epochs of 0, 1, 2, 63, 64, 65, 129 and 512 records in one call, under both presets."""
    label = "sizes, " + preset
    packed, it = calls()[label]
    worst = assert_matches_referee(label, run_host(packed, it))
    print("largest device deviation in units of the tolerance: %.3f" % max(worst.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(10))
def test_branches_match_referee(case):
    label, e, it = branch_epochs()[case]
    packed = gg.pack([e])
    got = run_host(packed, it)
    assert_matches_referee(label, got)
    ref = referee(label)
    if label == "a clock whose rows are all absorbed":
        assert got["clk_rows"][0, 4] == 0 and got["clock"][0, 4] == e["clock"][4]                   # unchanged, to the bit
        m = e["rec"][:, 1] == 4
        want = nge.evaluate(e["dat"], e["rec"], e["pos"] + e["base"], e["vel"], e["clock"], LD)[2][m]   # N from the input clock
        assert (np.abs(got["N"][m] - want.astype(np.float64)) <= tolerance(label)[0]["N"][0]).all()
        assert not got["r"][m].any()
    if label.startswith("constant clock") or label == "a constant clock, seed":
        for s in range(13):
            if (e["clk_const"] >> s) & 1:
                assert got["clock"][0, s] == e["clock"][s]
    if label == "w = 0 rows":
        assert got["clk_rows"][0, 8] == 0 and got["clock"][0, 8] == e["clock"][8]
    if label == "max_iter = 1":
        assert got["status"][0] == nge.MAX_ITER and got["iters"][0] == 1
    if label == "deficient":
        assert got["status"][0] == nge.RANK_DEFICIENT
        assert np.array_equal(got["pos"][0], e["pos"]) and np.array_equal(got["vel"][0], e["vel"]) and np.array_equal(got["clock"][0], e["clock"])
    if label in ("FREE_VEL without FREE_POS", "Doppler rows only"):
        assert np.array_equal(got["pos"][0], e["pos"]) and not got["info"][0][:3].any() and not got["info"][0][:, :3].any()
        assert ref["status"][0] == nge.CONVERGED


@pytest.mark.gpu
def test_batch_equals_single_epoch_calls_bit_for_bit():
    """A 37-epoch call of mixed sizes and presets, then every epoch alone; then the same with a 65-record epoch appended, which moves the
    call to the streaming instance: an epoch's bits depend neither on its neighbours nor on the instance."""
    eps = batch_epochs()
    packed = gg.pack(eps)
    got = run_host(packed, 20)
    ref = referee_call(packed, 20, LD)
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["iters"], ref["iters"]) and np.array_equal(got["clk_rows"], ref["clk_rows"])
    padded = gg.pack(eps + [gg.gen_epoch(2999, 65, "first_fix")])
    got2 = run_host(padded, 20)
    for e, ep in enumerate(eps):
        one = run_host(gg.pack([ep]), 20)
        alone = epoch_slice(one, np.array([0, ep["dat"].shape[0]]), 0)
        assert bitwise_equal(epoch_slice(got, packed[0], e), alone), e
        assert bitwise_equal(epoch_slice(got2, padded[0], e), alone), ("streaming instance", e)


@pytest.mark.gpu
def test_host_and_device_memory_agree_bit_for_bit():
    label = "sizes, first_fix"
    packed, it = calls()[label]
    host = run_host(packed, it)
    dev = run_device(packed, it)
    assert bitwise_equal(host, dev)
    small = gg.pack(batch_epochs()[:8])
    assert bitwise_equal(run_host(small, 20), run_device(small, 20))
    # NULL outputs are accepted
    E, n = small[0].size - 1, small[7].shape[0]
    rc, o = raw_call(small, null_outs=("pos", "N", "info", "clk_rows", "cost"))
    assert rc == 0
    full = run_host(small, 20)
    got = shape_outs(o, E, n)
    for k in ("vel", "clock", "r", "iters", "status"):
        assert np.array_equal(bits(got[k]), bits(full[k])), k
    assert (o["pos"] == -7).all() and (o["N"] == -7).all()
    rc, o = raw_call(small, null_outs=tuple(k for k, *_ in OUT_SPEC))
    assert rc == 0


def _bad_inputs():
    """(good, [(label, packed, max_iter, code)])"""
    n0, n1 = 45, 50
    good = gg.pack([gg.gen_epoch(3000, n0, "first_fix"), gg.gen_epoch(3001, n1, "first_fix")])
    bad = []

    def variant(label, code=E_INVALID, max_iter=20, **edit):
        p = [a.copy() for a in good]
        for k, fn in edit.items():
            fn(p[int(k[1:])])
        bad.append((label, tuple(p), max_iter, code))
    row = n0 + 5                                                   # a record of the second epoch
    phase_row = int(np.nonzero((good[8][:, 0] == nge.RTK_PHASE) & (np.arange(n0 + n1) >= n0))[0][0])
    code_row = int(np.nonzero((good[8][:, 0] == nge.RTK_CODE) & (np.arange(n0 + n1) >= n0))[0][0])

    def set_(i, j, v):
        def f(a):
            a[i, j] = v
        return f
    variant("first[0] != 0", a0=lambda a: a.__setitem__(0, 1))
    variant("decreasing first", a0=lambda a: a.__setitem__(1, n0 + n1 + 1))
    variant("kind 5", a8=set_(row, 0, 5))
    variant("kind -1", a8=set_(row, 0, -1))
    variant("slot 13", a8=set_(row, 1, 13))
    variant("state bit 2", a8=set_(row, 2, 2))
    variant("AMB_FREE on a code row", a8=set_(code_row, 2, 1))
    variant("NaN in a record", a7=set_(row, 1, np.nan))
    variant("inf obs", a7=set_(row, 6, np.inf))
    variant("inf pos", a1=set_(1, 0, np.inf))
    variant("NaN clock", a4=set_(1, 3, np.nan))
    variant("w < 0", a7=set_(row, 7, -1.0))
    variant("lam = 0 on a phase row", a7=set_(phase_row, 8, 0.0))
    variant("mode bit 4", a5=lambda a: a.__setitem__(1, 4))
    variant("max_iter 0", max_iter=0)
    big = gg.pack([gg.gen_epoch(3000, n0, "first_fix"), gg.gen_epoch(3002, 513, "first_fix")])
    bad.append(("513 records", big, 20, E_UNSUPPORTED))
    return good, bad


@pytest.mark.gpu
def test_rejections_return_their_code_and_launch_nothing():
    good, bad = _bad_inputs()
    rc, _o = raw_call(good)
    assert rc == 0
    for label, packed, it, code in bad:
        rc, o = raw_call(packed, max_iter=it)
        assert rc == code, (label, rc)
        assert solver.lib().swf_last_error(), label
        for k, v in o.items():
            assert (v == -7).all(), (label, k)                                                       # nothing was written
    for label, kw in (("step_tol NaN", dict(step_tol=np.nan)), ("eps_rank inf", dict(eps_rank=np.inf))):
        rc, o = raw_call(good, **kw)
        assert rc == E_INVALID and (o["status"] == -7).all(), label
    for k in range(9):                                                                               # null input pointers
        p = list(good); p[k] = None
        E, n = good[0].size - 1, good[7].shape[0]
        rc, o = raw_call(p, outs=make_outs(E, n), n_epochs=E)
        assert rc == E_INVALID and (o["status"] == -7).all(), k
    rc, o = raw_call(good, n_epochs=-1)
    assert rc == E_INVALID
    rc, o = raw_call(good, n_epochs=0)
    assert rc == 0 and (o["status"] == -7).all()
    with pytest.raises(solver.SwfError):
        solver.gnss_epoch_solve_batch(*bad[2][1])


@pytest.mark.gpu
def test_device_memory_bad_epoch_reports_minus_one():
    """With device memory the host cannot look: the kernel reports status = -1 for the epoch it finds invalid, writes nothing else of it,
    and its neighbour is what it is alone."""
    good, bad = _bad_inputs()
    ref = run_device(good, 20)
    want = referee_call(good, 20, LD)
    assert np.array_equal(ref["status"], want["status"]) and np.array_equal(ref["iters"], want["iters"])
    for label, packed, it, code in bad:
        if label in ("first[0] != 0", "decreasing first", "max_iter 0"):
            continue                                       # (the first two move every run of records; the last is a by-value argument)
        got = run_device(packed, it)
        first = packed[0]
        s = epoch_slice(got, first, 1)
        assert s["status"] == -1, label
        for k in ALL_KEYS:
            if k != "status":
                assert (np.atleast_1d(s[k]) == -7).all(), (label, k)
        assert bitwise_equal(epoch_slice(got, first, 0), epoch_slice(ref, good[0], 0)), label


def _parse_run(out, tag):
    fl = lambda key: [[float(v) for v in m.group(1).split()] for m in re.finditer(r"^%s %s (.*)$" % (key, tag), out, re.M)]
    st = fl("in")[0]
    recs = fl("rec")
    dat = np.array([r[6:] for r in recs]); rec = np.array([[r[2], r[4], r[5], 0] for r in recs], np.int32)
    src = [(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in recs]
    o = fl("out")[0]
    rows = np.array(fl("row"))
    packed = (np.array([0, len(recs)], np.int32), np.array([st[0:3]]), np.array([st[3:6]]), np.array([st[6:9]]), np.array(fl("clk")),
              np.array([0 if tag == "seed" else 3], np.int32), np.array([0], np.int32), dat, rec)
    got = dict(pos=np.array([o[0:3]]), vel=np.array([o[3:6]]), cost=np.array([o[6]]), iters=np.array([int(o[7])]), status=np.array([int(o[8])]),
               clock=np.array(fl("oclk")), N=rows[:, 1], r=rows[:, 2])
    return packed, got, src


@pytest.mark.gpu
def test_gnss_epoch_adapter_run_matches_referee(tmp_path):
    exe = compile_shim(tmp_path, "shim_gnss_epoch")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    obs = {int(m.group(1)): [float(v) for v in m.group(2).split()] for m in re.finditer(r"^obs (\d+) (.*)$", out.stdout, re.M)}
    for tag, it in (("seed", 2), ("fix", 20)):
        packed, got, src = _parse_run(out.stdout, tag)
        ref = referee_call(packed, it, LD)
        assert ref["status"][0] == nge.CONVERGED
        # the tolerance of this input, measured as for every other
        variants = [referee_call(packed, it, np.float64, nge.solve_dense)]
        rng = np.random.default_rng(9)
        n = packed[7].shape[0]
        for _ in range(N_ORDERS):
            variants.append(_stack([nge.solve(packed[1][0], packed[2][0], packed[3][0], packed[4][0], int(packed[5][0]), 0, packed[7], packed[8], it,
                                              STEP_TOL, EPS_RANK, np.float64, order=rng.permutation(n))]))
        got["info"] = ref["info"]; got["clk_rows"] = ref["clk_rows"]               # (the shim does not print them)
        unit = {k: np.zeros(1) for k in FLOAT_KEYS}
        for v in variants:
            v["info"] = ref["info"]
            d = deviations(packed, ref, v)
            unit = {k: np.maximum(unit[k], d[k]) for k in FLOAT_KEYS}
        fl = floors(packed, ref)
        tol = {k: np.maximum(8 * unit[k], fl[k]) for k in FLOAT_KEYS}
        assert_matches_referee("shim " + tag, got, packed, ref, tol)
        kinds = [s[2] for s in src]
        if tag == "seed":
            # AddGnssResidual's rows: RTK phase for every ambiguity above the mask (the unhealthy 9 included, 6 has none), RTK code without 3, 5 and 9,
            # no rover-only code (have_base), rover-only phase and Doppler without 3 and 9, correction rows for the odd observations
            assert sorted(s[0] for s in src if s[2] == 0) == [0, 1, 2, 4, 5, 7, 8, 9, 10, 11]
            assert sorted(s[0] for s in src if s[2] == 1) == [0, 1, 2, 4, 6, 7, 8, 10, 11]
            assert kinds.count(2) == 0 and kinds.count(4) == 10
            assert sorted(s[0] for s in src if s[2] == 3 and s[3]) == [1, 5, 7, 11]
            free = {(s[0], s[2]) for s, q in zip(src, packed[8]) if q[2]}
            assert free == {(0, 0), (4, 0), (8, 0), (0, 3), (4, 3), (8, 3)}
            for s, d in zip(src, packed[7]):
                if s[2] == 1:                                                       # the RTK code weight is 1 / sqrt(varerr2)
                    _i, _svh, _sys, el, pstd, dtb = [float(s[0])] + obs[s[0]]
                    assert abs(d[7] * np.sqrt(npf.varerr2(el, dtb, pstd * pstd)) - 1) < 3e-7      # (one float ulp of the sine)
        else:
            assert kinds.count(0) == 0 and kinds.count(1) == 0 and kinds.count(2) == 10 and kinds.count(3) == 10 and kinds.count(4) == 10
            assert all(q[2] == 1 for s, q in zip(src, packed[8]) if s[2] == 3)
