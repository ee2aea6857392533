"""The pre-fit carrier-phase screen on the device (swf_phase_screen_batch / solver.phase_screen_batch / swf_ceres::PhaseScreen): the
residuals, medians, slip flags and compacted reset lists of the first half of SWFOptimization::GnssPreprocess
(R/swf/swf_gnss.cpp:337-499) against the numpy referee of tests/np_phase.py on the inputs of tests/phase_gen.py.

Flags, counts and reset lists are compared exactly: every decision of every input sits >= 1e-4 m from its threshold by the longdouble
referee (test_inputs_are_decisive) while rounding is ~1e-8 m.

Tolerance of r and med.  Per record
    tol = M_TOL * 2^-52 * (|xg| + |sat| + |N lam| + |L_lam| + |dt|)
(for a median: the largest bracket among its set's members).  M_TOL is measured, not chosen
(test_tolerance_constant_is_the_measured_one): the float64 referee in two legitimate operation orders (the factor's left-to-right sum;
the sums regrouped) against the longdouble referee on the inputs below: largest ratio of a deviation to the bracket = 0.77, times the
margin of 8 for the device's fused multiply-adds, rounded up: M_TOL = 7.
Largest device deviation on MI355X, in units of the bracket: not measured; every GPU test prints it (`deviation / bracket`)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import np_phase as nph
import phase_gen as pg
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import build, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
M_TOL = 7.0
E_INVALID, E_UNSUPPORTED = -2, -3
SIZES = [0, 1, 2, 63, 64, 65, 255, 256]
BOTH = nph.GATE_RTK | nph.GATE_SPP
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pu8 = C.POINTER(C.c_uint8)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def size_epochs():
    """One epoch per size of the issue (0 .. 256 records), a few small ones for median sets of 1, 2 and 3, and one with a tie."""
    eps = [pg.gen_epoch(100 + n, n) for n in SIZES]
    eps += [pg.gen_epoch(200 + n, n, p_noamb=0.0, p_stale=0.0, groups=[0, 3]) for n in (3, 5, 7, 9)]
    eps.append(pg.gen_epoch(300, 40, tie=True))
    return eps


@functools.lru_cache(maxsize=None)
def branch_epochs():
    return [("gates off", pg.gen_epoch(400, 70, mode=0)),
            ("RTK gate only", pg.gen_epoch(401, 70, mode=nph.GATE_RTK)),
            ("SPP gate only", pg.gen_epoch(402, 70, mode=nph.GATE_SPP)),
            ("reset all", pg.gen_epoch(403, 70, mode=BOTH | nph.RESET_ALL)),
            ("reset all, gates off", pg.gen_epoch(404, 33, mode=nph.RESET_ALL)),
            ("records without an ambiguity", pg.gen_epoch(405, 90, p_noamb=0.5, p_stale=0.2))]


@functools.lru_cache(maxsize=None)
def batch_epochs():
    """~300 mixed epochs of at most 64 records (so that the call takes the one-slot instance unless a larger epoch is appended)."""
    rng = np.random.default_rng(7)
    sizes = rng.integers(0, 65, 300)
    sizes[:6] = [0, 64, 1, 63, 2, 32]
    modes = rng.choice([BOTH, BOTH, BOTH, nph.GATE_RTK, nph.GATE_SPP, 0, BOTH | nph.RESET_ALL], 300)
    return [pg.gen_epoch(1000 + i, int(sizes[i]), mode=int(modes[i])) for i in range(300)]


@functools.lru_cache(maxsize=None)
def all_inputs():
    """[(label, packed arrays)] of every input the GPU tests run."""
    out = [("size %d" % e["dat"].shape[0], pg.pack([e])) for e in size_epochs()]
    out += [(label, pg.pack([e])) for label, e in branch_epochs()]
    out.append(("batch", pg.pack(batch_epochs())))
    return out


@functools.lru_cache(maxsize=None)
def referee(label):
    return nph.screen(*dict(all_inputs())[label])


def deviation_ratio(packed, ref, got):
    """largest deviation of (r, med) from the referee in units of the bracket 2^-52 (|xg| + |sat| + |N lam| + |L_lam| + |dt|)"""
    first, pos, base, mode, dat, rec = packed
    br = nph.bracket(first, pos, base, dat, rec)
    E = first.size - 1
    ep = np.repeat(np.arange(E), np.diff(first))
    key = ep * 12 + rec[:, 0] * 6 + rec[:, 1]
    brm = np.zeros(E * 12)
    el = (rec[:, 2] & 3) == 3
    np.maximum.at(brm, key[el], br[el])
    with np.errstate(invalid="ignore", divide="ignore"):
        dr = np.abs((got["r"] - ref["r"]).astype(np.float64)) / (EPS * br)
        gm, rm = np.asarray(got["med"], np.float64).ravel(), np.asarray(ref["med"]).astype(np.float64).ravel()
        have = ref["cnt"].ravel() > 0
        dm = np.abs(gm[have] - rm[have]) / (EPS * brm[have])
    assert np.array_equal(np.isnan(gm), ~have), "med is NaN exactly for the empty sets"
    return (float(dr.max()) if dr.size else 0.0), (float(dm.max()) if dm.size else 0.0)


def assert_matches_referee(packed, got, ref=None, label=""):
    """`got` (device) against the float64 referee: flags, counts, reset lists exactly; r and med within tol."""
    ref = nph.screen(*packed) if ref is None else ref
    rr, rm = deviation_ratio(packed, ref, got)
    print("%s: %d epochs, %d records, %d resets, deviation / bracket: r %.3f med %.3f (M_TOL %.0f)"
          % (label, packed[0].size - 1, packed[4].shape[0], int(ref["n_reset"].sum()), rr, rm, M_TOL))
    assert np.array_equal(got["flags"], ref["flags"]), (label, np.nonzero(got["flags"] != ref["flags"])[0])
    assert np.array_equal(got["cnt"], ref["cnt"]), label
    assert np.array_equal(got["n_reset"], ref["n_reset"]), label
    assert np.array_equal(got["reset"], ref["reset"]), label
    assert rr <= M_TOL and rm <= M_TOL, (label, rr, rm)
    return rr, rm


KEYS = ("r", "flags", "med", "cnt", "reset", "n_reset")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def bitwise_equal(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in KEYS)


def epoch_slice(res, first, e):
    lo, hi = int(first[e]), int(first[e + 1])
    return dict(r=res["r"][lo:hi], flags=res["flags"][lo:hi], reset=res["reset"][lo:hi], med=res["med"][e], cnt=res["cnt"][e],
                n_reset=res["n_reset"][e:e + 1])


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_phase_screen_symbols_exported():
    build.build()
    lib = C.CDLL(solver.LIB_PATH)
    assert hasattr(lib, "swf_phase_screen_batch")
    assert "swf_phase_screen_batch" in solver.EXPORTED
    assert callable(solver.phase_screen_batch)
    assert lib.swf_version() >= 110
    hdr = open(os.path.join(ROOT, "include", "swf_solver.h")).read() + open(os.path.join(ROOT, "include", "swf_types.h")).read()
    for s in ("int swf_phase_screen_batch(", "SWF_SCR_DOUBLES = 9", "SWF_SCR_GROUPS = 6", "#define SWF_SCR_NMAX 256", "SWF_SCR_NEW_AMB = 8",
              "SWF_SCR_RESET_ALL = 4", "SWF_SCR_CONTINUING = 2", "SWF_SCR_SPP = 1"):
        assert s in hdr, s
    assert "PhaseScreen(" in open(os.path.join(ROOT, "include", "swf_ceres.hpp")).read()
    assert (solver.SCR_DOUBLES, solver.SCR_GROUPS, solver.SCR_NMAX) == (nph.DOUBLES, nph.GROUPS, nph.NMAX)


def test_inputs_are_decisive():
    """By the longdouble referee every |deviation - threshold| of every test input is >= 1e-4 m (code minus phase: >= 5 m from the
    limit), every elevation >= 1 degree from the mask; and the inputs cover what the issue lists."""
    kinds, groups, cnts, slips, codes, masked = set(), set(), set(), 0, 0, 0
    for label, packed in all_inputs():
        a, b, c = nph.margins(*packed)
        print("%s: closest residual decision %.3g m, closest code decision %.3g m, closest elevation %.3g rad" % (label, a, b, c))
        assert a >= 1e-4 and b >= 5.0 and c >= np.deg2rad(1.0) * 0.999, label
        ref = referee(label)
        kinds |= set(packed[5][:, 0].tolist()); groups |= set(packed[5][:, 1].tolist()); cnts |= set(ref["cnt"].ravel().tolist())
        slips += int(((ref["flags"] & nph.SLIP_RESIDUAL) != 0).sum()); codes += int(((ref["flags"] & nph.SLIP_CODE) != 0).sum())
        masked += int(((ref["flags"] & nph.MASKED) != 0).sum())
    assert kinds == {0, 1} and groups == set(range(6)) and {0, 1, 2, 3} <= cnts
    assert slips >= 20 and codes >= 20 and masked >= 20
    assert sorted(e["dat"].shape[0] for e in size_epochs())[-1] == nph.NMAX and [e["dat"].shape[0] for e in size_epochs()[:len(SIZES)]] == SIZES


def test_generator_slips_are_found_by_the_referee():
    """What the generator injected is what the referee flags (un-masked, gated, continuing records)."""
    for e in size_epochs() + [e for _, e in branch_epochs()][:1] + batch_epochs()[:40]:
        q = nph.screen(*pg.pack([e]), detail=True)
        g = q["gate"]
        assert np.array_equal(((q["flags"] & nph.SLIP_RESIDUAL) != 0)[g], e["slipped"][g])
        gs = g & ~q["rtk"]
        assert np.array_equal(((q["flags"] & nph.SLIP_CODE) != 0)[gs], e["code_slip"][gs])
        assert not (q["flags"][~g] & (nph.SLIP_RESIDUAL | nph.SLIP_CODE)).any()


def test_tie_case_has_a_tie():
    e = size_epochs()[-1]
    q = nph.screen(*pg.pack([e]))
    el = (e["rec"][:, 2] & 3) == 3
    rr = q["r"][el]
    assert np.unique(rr).size < rr.size


def test_tolerance_constant_is_the_measured_one():
    """M_TOL = 8 x the largest ratio, over the test inputs, of |float64 referee (either operation order) - longdouble referee| to the
    bracket, rounded up to the next integer."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    worst = 0.0
    for label, packed in all_inputs():
        first, pos, base, mode, dat, rec = packed
        br = EPS * nph.bracket(first, pos, base, dat, rec)
        ref = nph.residuals(first, pos, base, dat, rec, dtype=np.longdouble)
        for order in ("factor", "alt"):
            r = nph.residuals(first, pos, base, dat, rec, order=order)
            if r.size:
                worst = max(worst, float((np.abs(r - ref) / br).max()))
    print("largest float64 / longdouble deviation in units of the bracket: %.3f" % worst)
    assert 8.0 * worst <= M_TOL
    assert M_TOL <= 8.0 * worst + 1.0          # rounded up to the next integer, not padded


def _one(dat, rec, mode=BOTH, el_min=nph.AZELMIN):
    dat, rec = np.asarray(dat, np.float64).reshape(-1, 9), np.asarray(rec, np.int32).reshape(-1, 4)
    return nph.screen(np.array([0, dat.shape[0]], np.int32), np.zeros((1, 3)), np.array([[6.4e6, 0, 0]]), np.array([mode]), dat, rec, el_min)


def _row(L_off=0.0, lam=0.19, el=1.0, P=None, N=0.0, dt=0.0):
    """a record whose residual is exactly -L_off for the base (6.4e6, 0, 0) and the satellite (2.64e7, 0, 0): distance 2e7"""
    L = 2.0e7 + L_off
    return [2.64e7, 0.0, 0.0, L, lam, el, L if P is None else P, N, dt]


def test_referee_median_is_sorted_n_over_2():
    assert nph.upper_median([5.0]) == 5.0
    assert nph.upper_median([5.0, 1.0]) == 5.0
    assert nph.upper_median([5.0, 1.0, 3.0]) == 3.0
    assert nph.upper_median([5.0, 1.0, 3.0, 4.0]) == 4.0
    assert np.isnan(nph.upper_median([]))
    assert nph.upper_median([np.nan, 1.0]) != nph.upper_median([np.nan, 1.0]) and nph.upper_median([np.nan, 1.0, 2.0]) == 2.0
    assert nph.upper_median([2.0, 2.0, 1.0, 2.0]) == 2.0                                   # ties
    for n, want in ((1, 0.0), (2, 0.0), (3, -1.0), (4, -1.0)):                            # r_i = -i: sorted[n / 2] of {0, -1, .., -(n-1)}
        q = _one([_row(float(i)) for i in range(n)], [[0, 0, 3, -1]] * n, mode=0)
        assert q["cnt"][0, 0, 0] == n and q["med"][0, 0, 0] == want, n
        assert np.isnan(q["med"][0, 1, 0]) and q["cnt"][0, 1, 0] == 0


def test_referee_masked_record_stays_in_the_median():
    """Three members, one below the mask: its phase is zeroed, its residual (2e7 m off) still takes part (R/swf/swf_gnss.cpp:351-362)."""
    q = _one([_row(0.0), _row(0.01), _row(0.02, el=0.1)], [[0, 2, 3, -1]] * 3)
    assert q["cnt"][0, 0, 2] == 3 and q["r"][2] == 2.0e7 and q["med"][0, 0, 2] == 0.0     # sorted: -0.01, 0, 2e7
    assert q["flags"].tolist() == [0, 0, nph.MASKED] and q["n_reset"][0] == 0
    # a masked record alone decides nothing, even with RESET_ALL and without an ambiguity
    q = _one([_row(0.0, el=0.1)], [[0, 0, 0, -1]], mode=BOTH | nph.RESET_ALL)
    assert q["flags"].tolist() == [nph.MASKED] and q["n_reset"][0] == 0


def test_referee_partner_propagation_and_reset_all():
    lam = 0.19
    rtk = [_row(0.0), _row(0.001), _row(0.002), _row(lam)]                     # record 3 slipped by one cycle
    spp = [_row(0.0, N=1.0, dt=lam), _row(0.0, N=1.0, dt=lam), _row(0.0, N=1.0, dt=lam)]   # clean: r = -N lam + dt = 0; code test: |N lam| < 10
    rec = [[0, 0, 3, -1]] * 4 + [[1, 0, 3, 3], [1, 0, 3, 0], [1, 0, 3, -1]]
    q = _one(rtk + spp, rec)
    assert q["flags"].tolist() == [0, 0, 0, nph.SLIP_RESIDUAL | nph.NEW_AMB, nph.NEW_AMB, 0, 0]
    assert q["reset"].tolist() == [3, 4, -1, -1, -1, -1, -1] and q["n_reset"][0] == 2
    # RESET_ALL reaches every un-masked RTK record and no SPP record (:433 against :454)
    q = _one(rtk + spp, rec, mode=BOTH | nph.RESET_ALL)
    assert [f & nph.NEW_AMB for f in q["flags"].tolist()] == [8, 8, 8, 8, 8, 0, 0]
    # gates off: no slip is declared, the partner has nothing to pass on; records without a continuing ambiguity are still new
    rec2 = [list(r) for r in rec]; rec2[1][2] = nph.HAS_AMB; rec2[6][2] = 0
    q = _one(rtk + spp, rec2, mode=0)
    assert q["flags"].tolist() == [0, nph.NEW_AMB, 0, 0, 0, 0, nph.NEW_AMB] and q["r"][6] == 0.0
    # the code-minus-phase test: |(L + N lam) - P| sin^2(el) > 10
    s2 = np.sin(1.0) ** 2
    q = _one([_row(0.0, P=2.0e7 + 9.0 / s2), _row(0.0, P=2.0e7 - 11.0 / s2)], [[1, 4, 3, -1]] * 2)
    assert q["flags"].tolist() == [0, nph.SLIP_CODE | nph.NEW_AMB]


def test_phase_screen_adapter_compiles_as_cxx14(tmp_path):
    """GnssPreprocess's screen binds to swf_ceres::PhaseScreen under the reference's -std=c++14; without a GPU the shim exits non-zero
    with a message."""
    exe = compile_shim(tmp_path, "shim_phase_screen")
    if solver.device_count() == 0:
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode != 0 and "failed" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def run_host(packed, el_min=nph.AZELMIN):
    return solver.phase_screen_batch(*packed, el_min=el_min)


def raw_call(packed, el_min=nph.AZELMIN, outs=None, n_epochs=None):
    """the C entry point on host memory; returns its code"""
    first, pos, base, mode, dat, rec = [np.ascontiguousarray(a) for a in packed]
    n, E = max(dat.shape[0], 1), (first.size - 1 if n_epochs is None else n_epochs)
    o = outs or dict(r=np.zeros(n), flags=np.zeros(n, np.uint8), med=np.zeros(max(E, 1) * 12), cnt=np.zeros(max(E, 1) * 12, np.int32),
                     reset=np.zeros(n, np.int32), n_reset=np.full(max(E, 1), -7, np.int32))
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    rc = solver.lib().swf_phase_screen_batch(C.c_int32(E), p(first, pi), p(pos, pd), p(base, pd), p(mode, pi), C.c_double(el_min), p(dat, pd),
                                             p(rec, pi), p(o["r"], pd), p(o["flags"], pu8), p(o["med"], pd), p(o["cnt"], pi), p(o["reset"], pi),
                                             p(o["n_reset"], pi), C.c_int32(0), None)
    return rc, o


def _hip(call, *args):
    """a HIP runtime call of the runtime libswf_hip.so itself is linked against (its symbols resolve through the library's handle)"""
    rc = getattr(solver.lib(), call)(*args)
    assert rc == 0, (call, rc)


def run_device(packed, el_min=nph.AZELMIN, fill=None):
    """on_device = 1 over hipMalloc'ed buffers on the null stream; returns the outputs as numpy arrays (the device buffers pre-filled with
    `fill`)"""
    first, pos, base, mode, dat, rec = packed
    E, n = first.size - 1, dat.shape[0]
    f = fill if fill is not None else 0
    mk = lambda k, t, v: np.full(max(k, 1), v, t)
    host_in = [np.ascontiguousarray(a).reshape(-1) if a.size else np.zeros(k, a.dtype) for a, k in zip(packed, (1, 3, 3, 1, 9, 4))]
    host_out = dict(r=mk(n, np.float64, float(f)), flags=mk(n, np.uint8, f & 0xff), med=mk(E * 12, np.float64, float(f)), cnt=mk(E * 12, np.int32, f),
                    reset=mk(n, np.int32, f), n_reset=mk(E, np.int32, f))
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
        ptr = lambda d, ty: C.cast(d, ty)
        rc = solver.lib().swf_phase_screen_batch(C.c_int32(E), ptr(ins[0], pi), ptr(ins[1], pd), ptr(ins[2], pd), ptr(ins[3], pi), C.c_double(el_min),
                                                 ptr(ins[4], pd), ptr(ins[5], pi), ptr(o["r"], pd), ptr(o["flags"], pu8), ptr(o["med"], pd),
                                                 ptr(o["cnt"], pi), ptr(o["reset"], pi), ptr(o["n_reset"], pi), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in host_out.items():
            _hip("hipMemcpy", C.c_void_p(v.ctypes.data), o[k], C.c_size_t(v.nbytes), C.c_int(2))   # hipMemcpyDeviceToHost
    finally:
        for d in bufs:
            solver.lib().hipFree(d)
    h = host_out
    return dict(r=h["r"][:n], flags=h["flags"][:n], reset=h["reset"][:n], med=h["med"][:E * 12].reshape(E, 2, 6), cnt=h["cnt"][:E * 12].reshape(E, 2, 6),
                n_reset=h["n_reset"][:E])


@pytest.mark.gpu
def test_epoch_sizes_match_referee():
    """Epochs of 0, 1, 2, 63, 64, 65, 255 and 256 records (and the small and tied ones), each alone, then all in one call."""
    worst = (0.0, 0.0)
    for label, packed in all_inputs():
        if not label.startswith("size"):
            continue
        got = run_host(packed)
        rr, rm = assert_matches_referee(packed, got, referee(label), label)
        worst = (max(worst[0], rr), max(worst[1], rm))
    packed = pg.pack(size_epochs())
    got = run_host(packed)
    rr, rm = assert_matches_referee(packed, got, label="all sizes in one call")
    for e, ep in enumerate(size_epochs()):
        assert bitwise_equal(epoch_slice(got, packed[0], e), epoch_slice(run_host(pg.pack([ep])), np.array([0, ep["dat"].shape[0]]), 0)), e
    print("largest device deviation in units of the bracket: r %.3f med %.3f" % (max(worst[0], rr), max(worst[1], rm)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(6))
def test_branches_match_referee(case):
    label, e = branch_epochs()[case]
    packed = pg.pack([e])
    got = run_host(packed)
    assert_matches_referee(packed, got, referee(label), label)
    if "gates off" in label:
        assert not (got["flags"] & (nph.SLIP_RESIDUAL | nph.SLIP_CODE)).any()
    if label == "reset all":
        rtk = (e["rec"][:, 0] == nph.RTK) & ((got["flags"] & nph.MASKED) == 0)
        assert ((got["flags"][rtk] & nph.NEW_AMB) != 0).all() and rtk.sum() > 10
    if "without" in label:
        noamb = (e["rec"][:, 2] & nph.HAS_AMB) == 0
        assert noamb.sum() > 20 and (got["r"][noamb] == 0.0).all() and np.isnan(e["dat"][noamb, 7]).all()


@pytest.mark.gpu
def test_batch_equals_single_bitwise():
    """~300 mixed epochs in one call against the referee; every epoch equals the epoch run alone, bit for bit — also with the epoch
    order permuted, and with a 65-record epoch appended (which moves the whole call to the 256-record instance)."""
    eps = batch_epochs()
    packed = pg.pack(eps)
    got = run_host(packed)
    assert_matches_referee(packed, got, referee("batch"), "batch of %d" % len(eps))
    alone = [run_host(pg.pack([e])) for e in eps]
    one = lambda i: epoch_slice(alone[i], np.array([0, eps[i]["dat"].shape[0]]), 0)
    for i in range(len(eps)):
        assert bitwise_equal(epoch_slice(got, packed[0], i), one(i)), i
    perm = np.random.default_rng(3).permutation(len(eps))
    pp = pg.pack([eps[i] for i in perm])
    gp = run_host(pp)
    for k, i in enumerate(perm):
        assert bitwise_equal(epoch_slice(gp, pp[0], k), one(i)), (k, i)
    assert int(np.diff(packed[0]).max()) <= 64
    big = pg.pack(eps + [pg.gen_epoch(100 + 65, 65)])
    gb = run_host(big)
    for i in range(len(eps)):
        assert bitwise_equal(epoch_slice(gb, big[0], i), one(i)), i
    assert bitwise_equal(epoch_slice(gb, big[0], len(eps)), epoch_slice(run_host(pg.pack([pg.gen_epoch(100 + 65, 65)])), np.array([0, 65]), 0))


@pytest.mark.gpu
def test_memory_modes_agree_bitwise_and_null_outputs():
    for packed in (pg.pack(size_epochs()), pg.pack(batch_epochs()[:40])):
        host, dev = run_host(packed), run_device(packed)
        assert bitwise_equal(host, dev)
        assert_matches_referee(packed, dev, label="device memory")
    # NULL output pointers, one kind at a time and all at once
    packed = pg.pack(batch_epochs()[:12])
    full = run_host(packed)
    n, E = packed[4].shape[0], packed[0].size - 1
    for drop in KEYS + (None,):
        o = dict(r=np.zeros(n), flags=np.zeros(n, np.uint8), med=np.zeros(E * 12), cnt=np.zeros(E * 12, np.int32), reset=np.zeros(n, np.int32),
                 n_reset=np.zeros(E, np.int32))
        for k in (KEYS if drop is None else (drop,)):
            o[k] = None
        rc, o = raw_call(packed, outs=o)
        assert rc == 0, (drop, solver.lib().swf_last_error())
        for k in KEYS:
            if o[k] is not None:
                assert np.array_equal(bits(o[k]), bits(full[k].ravel())), (drop, k)


def _bad_inputs():
    """[(label, packed, expected code)]: every rejection of the issue, on an otherwise valid two-epoch call"""
    eps = [pg.gen_epoch(500, 20), pg.gen_epoch(501, 24)]
    good = pg.pack(eps)
    n0 = int(good[0][1])
    spps = np.nonzero(good[5][:n0, 0] == nph.SPP)[0]
    assert spps.size >= 2
    spp, spp_other = int(spps[0]), int(spps[1])           # two rover-only records of epoch 0
    out = []

    def mod(label, code, fn):
        p = [a.copy() for a in good]
        fn(p)
        out.append((label, tuple(p), code))
    mod("first[0] != 0", E_INVALID, lambda p: p[0].__setitem__(0, 1))
    mod("decreasing first", E_INVALID, lambda p: p[0].__setitem__(1, p[0][2] + 1))
    mod("kind 2", E_INVALID, lambda p: p[5].__setitem__((3, 0), 2))
    mod("kind -1", E_INVALID, lambda p: p[5].__setitem__((3, 0), -1))
    mod("group 6", E_INVALID, lambda p: p[5].__setitem__((25, 1), 6))
    mod("group -1", E_INVALID, lambda p: p[5].__setitem__((25, 1), -1))
    mod("state bit 4", E_INVALID, lambda p: p[5].__setitem__((7, 2), 7))
    mod("partner out of range", E_INVALID, lambda p: p[5].__setitem__((spp, 3), n0))
    mod("partner -2", E_INVALID, lambda p: p[5].__setitem__((spp, 3), -2))
    mod("partner is the record itself", E_INVALID, lambda p: p[5].__setitem__((spp, 3), spp))
    mod("partner is an SPP record", E_INVALID, lambda p: p[5].__setitem__((spp, 3), spp_other))
    mod("lam = 0", E_INVALID, lambda p: p[4].__setitem__((5, 4), 0.0))
    mod("lam < 0", E_INVALID, lambda p: p[4].__setitem__((5, 4), -0.19))
    mod("lam NaN", E_INVALID, lambda p: p[4].__setitem__((30, 4), np.nan))
    mod("lam inf", E_INVALID, lambda p: p[4].__setitem__((30, 4), np.inf))
    big = pg.pack([eps[0], pg.gen_epoch(502, nph.NMAX + 1)])
    out.append(("257 records", big, E_UNSUPPORTED))
    return good, out, spp


@pytest.mark.gpu
def test_rejections_return_their_code_and_launch_nothing():
    good, bad, _ = _bad_inputs()
    rc, _o = raw_call(good)
    assert rc == 0
    for label, packed, code in bad:
        rc, o = raw_call(packed)
        assert rc == code, (label, rc)
        assert solver.lib().swf_last_error(), label
        assert (o["n_reset"] == -7).all() and not o["r"].any() and not o["flags"].any(), label       # nothing was written
    for label, el in (("el_min NaN", np.nan), ("el_min inf", np.inf)):
        rc, o = raw_call(good, el_min=el)
        assert rc == E_INVALID and (o["n_reset"] == -7).all(), label
    for k in range(6):                                                                               # null input pointers
        p = list(good); p[k] = None
        first = good[0]
        n, E = good[4].shape[0], first.size - 1
        o = dict(r=np.zeros(n), flags=np.zeros(n, np.uint8), med=np.zeros(E * 12), cnt=np.zeros(E * 12, np.int32), reset=np.zeros(n, np.int32),
                 n_reset=np.full(E, -7, np.int32))
        q = lambda a, t: a.ctypes.data_as(t) if a is not None else None
        rc = solver.lib().swf_phase_screen_batch(C.c_int32(E), q(p[0], pi), q(p[1], pd), q(p[2], pd), q(p[3], pi), C.c_double(nph.AZELMIN), q(p[4], pd),
                                                 q(p[5], pi), q(o["r"], pd), q(o["flags"], pu8), q(o["med"], pd), q(o["cnt"], pi), q(o["reset"], pi),
                                                 q(o["n_reset"], pi), C.c_int32(0), None)
        assert rc == E_INVALID and (o["n_reset"] == -7).all(), k
    rc, o = raw_call(good, n_epochs=-1)
    assert rc == E_INVALID
    rc, o = raw_call(good, n_epochs=0)
    assert rc == 0 and (o["n_reset"] == -7).all()
    with pytest.raises(solver.SwfError):
        solver.phase_screen_batch(*bad[2][1])


@pytest.mark.gpu
def test_device_memory_bad_epoch_reports_minus_one():
    """With device memory the host cannot look: the kernel reports n_reset = -1 for the epoch it finds invalid, writes nothing else of
    it, and its neighbours are what they are alone."""
    good, bad, _ = _bad_inputs()
    ref = run_device(good, fill=-7)
    assert_matches_referee(good, ref, label="two good epochs, device memory")
    for label, packed, code in bad:
        if label in ("first[0] != 0", "decreasing first"):
            continue                                       # (these move every run of records: not an epoch-local fault)
        got = run_device(packed, fill=-7)
        first = packed[0]
        if label == "257 records":
            be = 1
        else:
            be = [e for e in range(2) if not bitwise_equal(epoch_slice(got, first, e), epoch_slice(ref, first, e))]
            assert len(be) == 1, (label, be)
            be = be[0]
        s = epoch_slice(got, first, be)
        assert s["n_reset"][0] == -1, label
        assert (s["r"] == -7.0).all() and (s["flags"] == (-7 & 0xff)).all() and (s["reset"] == -7).all() and (s["cnt"] == -7).all() and (s["med"] == -7.0).all(), label
        good_e = 1 - be
        assert bitwise_equal(epoch_slice(got, first, good_e), epoch_slice(ref, good[0], good_e)), label


@pytest.mark.gpu
def test_phase_screen_adapter_run_matches_referee(tmp_path):
    exe = compile_shim(tmp_path, "shim_phase_screen")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    fl = lambda tag: [[float(v) for v in m.group(1).split()] for m in re.finditer(r"^%s (.*)$" % tag, out.stdout, re.M)]
    ep = fl("epoch")[0]
    lams = {(int(a), int(b)): v for a, b, v in fl("lam")}
    dt = {int(k): v for k, v in fl("dt")}
    obs = {int(r[0]): r for r in fl("obs")}
    # the records GnssPreprocess evaluates or decides on, restated from the printed epoch
    dat, rec, where, partner = [], [], [], -1
    for i, f, rtk_L, spp_L, spp_P, rh, rN, rc_, sh, sN, sc in fl("obsf"):
        i, f = int(i), int(f)
        _, svh, sys_, el, sx, sy, sz = obs[i]
        if svh:
            continue
        lam = lams[(int(sys_), f)]
        partner = -1
        for kind, L, P, h, N, c, clk in ((0, rtk_L, 0.0, rh, rN, rc_, dt[int(sys_) * 2 + f]), (1, spp_L, spp_P, sh, sN, sc, dt[6 + int(sys_) * 2])):
            if L == 0 and not h:
                continue
            dat.append([sx, sy, sz, L * lam, lam, el if L != 0 else -1e300, P, N, clk])
            rec.append([kind, int(sys_) * 2 + f, (1 if h else 0) | (2 if c else 0), -1 if kind == 0 else partner])
            where.append((i, f, kind))
            if kind == 0:
                partner = len(where) - 1
    assert len(where) == 18
    packed = (np.array([0, len(where)], np.int32), np.array([ep[0:3]]), np.array([ep[3:6]]), np.array([int(ep[6])], np.int32), np.array(dat),
              np.array(rec, np.int32))
    assert min(nph.margins(*packed, el_min=ep[7])[:2]) >= 1e-4
    ref = nph.screen(*packed, el_min=ep[7])
    got_f = {(int(r[0]), int(r[1])): r for r in fl("flag")}
    tol = M_TOL * EPS * nph.bracket(packed[0], packed[1], packed[2], packed[4], packed[5])
    for k, (i, f, kind) in enumerate(where):
        assert int(got_f[(i, f)][2 + kind]) == ref["flags"][k], (i, f, kind)
        assert abs(got_f[(i, f)][4 + kind] - ref["r"][k]) <= tol[k], (i, f, kind)
    seen = {(i, f) for i, f, _ in where}
    for key, r in got_f.items():
        if key not in seen:
            assert r[2] == 0 and r[3] == 0, key
    reset = [int(v) for v in re.search(r"^reset(.*)$", out.stdout, re.M).group(1).split()]
    assert reset == [(where[k][0] * 2 + where[k][1]) * 2 + where[k][2] for k in ref["reset"][:ref["n_reset"][0]]]
    for kind, g, cnt, med in fl("med"):
        assert int(cnt) == ref["cnt"][0, int(kind), int(g)]
    new = {w for k, w in enumerate(where) if ref["flags"][k] & nph.NEW_AMB}
    assert new == {(1, 0, 1), (2, 0, 0), (2, 0, 1), (4, 0, 1), (6, 0, 0), (7, 0, 0)}
