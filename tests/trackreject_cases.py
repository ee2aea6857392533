"""The inputs of test_track_reject.py and test_track_reject_gpu.py and the referee's results on them, computed once per process."""
import functools

import numpy as np

import np_trackreject as npt
import trackreject_gen as tg

EPS = 2.0 ** -52
SHAPE_N = (7, 8, 9, 63, 64, 65, 200, 1024)
ITERATIONS = (1, 255, 256, 257, 1000)
LONG_ITERATIONS = 1000                  # judged by the scan replay and the masks only
KAPPA_MAX = 1e10
M_HYP, M_LIFT = 43.0, 3.0               # measured: the docstring of test_track_reject.py; test_tolerance_constants_are_the_measured_ones holds them
MOVING = ("general", "forward", "sideways")
E2E_SEED = 20000
TRUTH_ITERATIONS = 1000                 # OpenCV's default: at 40 % outliers one sample in 60 is clean
LOW_NOISE = 0.03                        # a pair of 8 points has one hypothesis, which must hold all 8: less noise than elsewhere


@functools.lru_cache(maxsize=None)
def shape_pairs():
    """every point count of the issue, flag bit 0 both ways.  The pairs without the flag use the camera with the rational terms (the
    flag and the camera are arguments of the call: a call per flag value)."""
    return [tg.gen_pair(300 + 2 * i + fl, n, outliers=0.2 if n >= 33 else 0.0, flags=fl, motion=MOVING[i % 3], fail="few" if n < 8 else None,
                        cam=tg.CAM if fl else tg.CAM_RATIONAL, noise=LOW_NOISE if n == 8 else tg.NOISE) for i, n in enumerate(SHAPE_N) for fl in (0, 1)]


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """257 ragged pairs of 8 to 120 points with the three failure codes mixed in, all with flag bit 0 set; every fourth a pure rotation"""
    rng = np.random.default_rng(29)
    sizes = rng.integers(8, 121, 257)
    sizes[:6] = [8, 9, 120, 64, 65, 16]
    fails = {3: "bad", 17: "few", 19: "nomodel", 20: "bad", 100: "few", 101: "few", 181: "nomodel", 255: "bad", 256: "few"}
    out = []
    for i in range(257):
        fail = fails.get(i)
        n = int(rng.integers(0, 8)) if fail == "few" else int(sizes[i])
        frac = float(rng.uniform(0.05, 0.35)) if n >= 33 else 0.0      # (few points: an all-inlier sample must be likely)
        out.append(tg.gen_pair(7000 + i, n, outliers=frac, flags=1, motion=tg.MOTIONS[i % 4], fail=fail,
                               noise=LOW_NOISE if n == 8 else tg.NOISE))
    return out


@functools.lru_cache(maxsize=None)
def truth_pairs():
    """n >= 33 and at most 40 % outliers, the three motions with a translation, 0.1 px of noise; judged at TRUTH_ITERATIONS"""
    return [tg.gen_pair(1100 + 10 * i + j, n, outliers=frac, motion=MOVING[(i + j) % 3], noise=0.1)
            for i, n in enumerate((33, 50, 100, 150)) for j, frac in enumerate((0.1, 0.25, 0.4))]


@functools.lru_cache(maxsize=None)
def e2e_pairs():
    """The end-to-end set: 48 pairs whose every decision is out of rounding's reach by the margin of undecided().  That margin comes
    from the bracket 2^-52 kappa, which overstates the error of the Householder route by about sqrt(kappa), and it is multiplied by the
    pixel coordinates (up to 752): a pair with outliers, whose contaminated hypotheses spread their errors over every magnitude, or with
    a short baseline (kappa 1e6 and more) is undecided almost surely.  So these pairs have 8 to 13 tracks, no outliers, 0.02 px of noise
    and eight times the baseline of the other sets; their scans end after one to five hypotheses."""
    return [tg.gen_pair(E2E_SEED + i, 8 + i % 6, outliers=0.0, flags=1, motion=MOVING[i % 3], noise=0.02, baseline=8.0) for i in range(48)]


def iteration_pairs():
    """the pairs of the iteration-count tests: 9, 65 and 200 points"""
    return [p for p in shape_pairs() if p["n"] in (9, 65, 200) and p["flags"] == 1]


def pairs_of(which):
    return {"shape": shape_pairs, "batch": batch_pairs, "truth": truth_pairs, "e2e": e2e_pairs}[which]()


def run_referee(p, dtype=np.float64, order=0, iterations=tg.ITERATIONS):
    return npt.pair(p["cur"], p["prev"], p["cam"], p["dt"], tg.COL, tg.ROW, tg.FOCAL, iterations, tg.THRESHOLD, tg.CONFIDENCE, tg.SEED,
                    p["flags"], dtype, order)


@functools.lru_cache(maxsize=None)
def referee(which, dtype_name="float64", order=0):
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return [run_referee(p, dtype, order, TRUTH_ITERATIONS if which == "truth" else tg.ITERATIONS) for p in pairs_of(which)]


@functools.lru_cache(maxsize=None)
def referee_iterations(iterations, dtype_name="float64", order=0):
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return [run_referee(p, dtype, order, iterations) for p in iteration_pairs()]


def expected_code(p):
    return {None: npt.OK, "few": npt.TOO_FEW, "bad": npt.BAD_INPUT, "nomodel": npt.NO_MODEL}[p["fail"]]


def hyp_deviation(hyp, ref):
    """largest entry deviation of the unit-norm, sign-fixed hypotheses [H]"""
    with np.errstate(all="ignore"):
        return np.asarray(np.abs(npt.normalised(np.asarray(hyp).astype(ref.dtype)) - npt.normalised(ref)).max(axis=1), np.float64)


def undecided(r, m_hyp):
    """A pair whose decisions rounding could change.  (i) Some scanned hypothesis k has a point whose e^2 / thr^2 lies within that
    hypothesis's first-order margin of 1: the unit-norm hypothesis may deviate by delta = m_hyp 2^-52 kappa_k in every entry, which moves
    N = m2^T F m1 by at most delta L1 L2 and a, b by at most delta L1 (L = |u| + |v| + 1), so that at the threshold, where |N| = thr
    sqrt(D), d = N^2 / D moves by at most mu d, mu = 2 delta L1 (L2 / thr + sqrt 2) / sqrt(D) (np_trackreject.score's mu1, mu2 per unit
    of delta).  A hypothesis above KAPPA_MAX or invalid makes the pair undecided if it is scanned.  (ii) A stopping-rule quotient within
    1e-9 of a half-integer."""
    if "hyp" not in r:
        return False
    if any(abs(abs(q - np.floor(q)) - 0.5) <= 1e-9 for q in r["ratios"]):
        return True
    k = r["scanned"]
    kap = r["kappa"][:k]
    if not (kap <= KAPPA_MAX).all():
        return True
    delta = (m_hyp * EPS * kap)[:, None]
    thr2 = float(r["thr2"])
    with np.errstate(all="ignore"):
        for d, mu in ((r["d1"], r["mu1"]), (r["d2"], r["mu2"])):
            rel = np.abs(np.asarray(d[:k], np.float64) / thr2 - 1.0)
            if (rel <= delta * mu[:k]).any():
                return True
    return False
