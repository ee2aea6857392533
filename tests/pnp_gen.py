"""Frames for the RANSAC PnP operator: a true pose, landmarks at 3 to 20 m inside the field of view, observation noise of half a pixel,
outliers displaced by at least 50 pixels at shuffled positions, and the previous frame's pose 0.05 to 0.3 m and 0.02 to 0.1 rad off."""
import numpy as np

FOCAL_LENGTH = 1000.0
SIGMA = 0.5 / FOCAL_LENGTH
THRESHOLD = 8.0 / FOCAL_LENGTH
CONFIDENCE = 0.99
ITERATIONS = 100
SEED = 0x5EED0123456789AB
TIC = np.array([0.05, -0.02, 0.03])
PBG = np.array([0.1, 0.2, -0.3])


def rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


RIC = rot([0.01, -0.02, 0.015]) @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def gen_frame(seed, n, outliers=0.3, flags=1, fail=None):
    """one frame of n points.  fail: None, "few" (n is taken as given, < 4), "bad" (one non-finite coordinate) or "nomodel" (the
    observations are unrelated to the landmarks).  Returns a dict; `outlier` marks the displaced observations."""
    rng = np.random.default_rng(seed)
    Rs = rot(_unit(rng) * rng.uniform(0.0, 2.5))
    Ps = rng.uniform(-20.0, 20.0, 3)
    Rc, Pc = Rs @ RIC, Rs @ (TIC - PBG) + Ps
    z = rng.uniform(3.0, 20.0, n)
    xy = rng.uniform(-0.5, 0.5, (n, 2))
    pc = np.concatenate([xy * z[:, None], z[:, None]], axis=1)
    pts_w = pc @ Rc.T + Pc
    uv = xy + SIGMA * rng.standard_normal((n, 2))
    n_out = int(round(outliers * n)) if n >= 5 else 0
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:n_out]] = True
    ang = rng.uniform(0.0, 2 * np.pi, n)
    mag = rng.uniform(50.0, 200.0, n) / FOCAL_LENGTH
    uv[out] += (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[out]
    if fail == "nomodel":
        uv = rng.uniform(-0.5, 0.5, (n, 2))
        out[:] = True
    if fail == "bad":
        which = int(rng.integers(0, 5 * n))
        if which < 3 * n:
            pts_w[which // 3, which % 3] = (np.nan, np.inf, -np.inf)[which % 3]
        else:
            uv[(which - 3 * n) // 2, which % 2] = np.nan
    Ps_prev = Ps + _unit(rng) * rng.uniform(0.05, 0.3)
    Rs_prev = Rs @ rot(_unit(rng) * rng.uniform(0.02, 0.1))
    return dict(n=n, pts_w=pts_w, pts_uv=uv, Ps_prev=Ps_prev, Rs_prev=Rs_prev, Ps_true=Ps, Rs_true=Rs, Rc_true=Rc, Pc_true=Pc,
                outlier=out, flags=flags, fail=fail, seed=seed)


def pack(frames):
    """the arguments of solver.pnp_frame_batch: lists of per-frame arrays, then Ps_prev [n][3], Rs_prev [n][9]"""
    return ([f["pts_w"] for f in frames], [f["pts_uv"] for f in frames], np.array([f["Ps_prev"] for f in frames]).reshape(-1, 3),
            np.array([f["Rs_prev"] for f in frames]).reshape(-1, 9))
