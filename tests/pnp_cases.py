"""The inputs of test_pnp.py and test_pnp_gpu.py and the referee's results on them, computed once per process."""
import functools

import numpy as np

import np_pnp as npp
import pnp_gen as pg

EPS = 2.0 ** -52
SHAPE_N = (3, 4, 5, 6, 8, 63, 64, 65, 200)
ITERATIONS = (1, 63, 64, 65, 100, 128)
COND_MAX = 1e8
M_HYP, M_REF = 2.0, 1.0                 # measured: the docstring of test_pnp.py; test_tolerance_constants_are_the_measured_ones holds them
ARGS = (pg.TIC, pg.RIC, pg.PBG)


@functools.lru_cache(maxsize=None)
def shape_frames():
    """every point count of the issue, flag bit 0 both ways; no outliers below 8 points (a frame of 5 would have no model)"""
    return [pg.gen_frame(300 + 2 * i + fl, n, outliers=0.3 if n >= 8 else 0.0, flags=fl, fail="few" if n < 4 else None)
            for i, n in enumerate(SHAPE_N) for fl in (0, 1)]


@functools.lru_cache(maxsize=None)
def batch_frames():
    """257 ragged frames of 4 to 120 points with the three failure codes mixed in, all with flag bit 0 set (the flag is an argument of
    the call: one call takes them all; the shape frames have it both ways)"""
    rng = np.random.default_rng(23)
    sizes = rng.integers(4, 121, 257)
    sizes[:6] = [4, 5, 120, 64, 65, 8]
    fails = {3: "bad", 17: "few", 19: "nomodel", 20: "bad", 100: "few", 101: "few", 181: "nomodel", 255: "bad", 256: "few"}
    out = []
    for i in range(257):
        fail = fails.get(i)
        n = int(rng.integers(0, 4)) if fail == "few" else max(int(sizes[i]), 12) if fail == "nomodel" else int(sizes[i])
        frac = 0.0 if n < 8 else float(rng.uniform(0.17, 0.45)) if n >= 33 else 0.25     # (few points: an all-inlier sample must be likely)
        out.append(pg.gen_frame(5000 + i, n, outliers=frac, flags=1, fail=fail))
    return out


@functools.lru_cache(maxsize=None)
def truth_frames():
    """n >= 33 and at most 40 % outliers"""
    return [pg.gen_frame(900 + 10 * i + j, n, outliers=frac) for i, n in enumerate((33, 50, 100, 200)) for j, frac in enumerate((0.17, 0.3, 0.4))]


def iteration_frames():
    """the frames of the iteration-count tests: 4, 5, 65 and 200 points"""
    return [f for f in shape_frames() if f["n"] in (4, 5, 65, 200) and f["flags"] == 1]


@functools.lru_cache(maxsize=None)
def referee_iterations(iterations, dtype_name="float64", order=0):
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return [run_referee(f, dtype, order, iterations) for f in iteration_frames()]


def frames_of(which):
    return {"shape": shape_frames, "batch": batch_frames, "truth": truth_frames}[which]()


def run_referee(f, dtype=np.float64, order=0, iterations=pg.ITERATIONS):
    return npp.frame(f["pts_w"], f["pts_uv"], f["Ps_prev"], f["Rs_prev"], *ARGS, iterations, pg.THRESHOLD, pg.CONFIDENCE, pg.SEED, f["flags"], dtype, order)


@functools.lru_cache(maxsize=None)
def referee(which, dtype_name="float64", order=0):
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return [run_referee(f, dtype, order) for f in frames_of(which)]


def expected_code(f):
    return {None: npp.OK, "few": npp.TOO_FEW, "bad": npp.BAD_INPUT, "nomodel": npp.NO_MODEL}[f["fail"]]


def tnorm(t):
    return max(1.0, float(np.linalg.norm(np.asarray(t, np.float64))))


def hyp_bracket(cond, hyp):
    """2^-52 cond(A) max(1, |t|) per hypothesis (inf where the hypothesis is invalid)"""
    t = np.linalg.norm(np.nan_to_num(np.asarray(hyp, np.float64)[:, 9:]), axis=1)
    return EPS * cond * np.maximum(1.0, t)


def undecided(r, rel=1e-6):
    """condition (iii): some squared error within rel of the threshold, or some |z| <= rel, over all hypothesis-point pairs"""
    v = np.isfinite(np.asarray(r["hyp"], np.float64)).all(axis=1)
    e2, z, thr2 = np.asarray(r["e2"], np.float64)[v], np.asarray(r["z"], np.float64)[v], float(r["thr2"])
    return bool((np.abs(e2 - thr2) <= rel * thr2).any() or (np.abs(z) <= rel).any())


def near_half(r, tol=1e-9):
    """condition (ii): a rounded quotient of the stopping rule within tol of a half-integer"""
    return any(abs(abs(q - np.floor(q)) - 0.5) <= tol for q in r["ratios"])
