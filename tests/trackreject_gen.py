"""Two-view scenes for the track outlier rejection: points at 3 to 20 m seen by the current camera, moved by a known motion into the
previous camera, both projected forward through the PINHOLE_FULL model into pixels; pixel noise of 0.3 px in both images; a share of
gross outliers whose previous pixel is displaced by 20 to 100 px and lies at least 10 px from its true epipolar line.  Motions:
general, forward, sideways and pure rotation (degenerate for F by construction)."""
import json
import os

import numpy as np

import np_trackreject as npt

HERE = os.path.dirname(os.path.abspath(__file__))
COL, ROW, FOCAL = 752, 480, 1000.0
THRESHOLD = 1.0
CONFIDENCE = 0.99
ITERATIONS = 128
SEED = 0x7AC3E11D5EED0042
NOISE = 0.3
MOTIONS = ("general", "forward", "sideways", "rotation")


def load_cam():
    """fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 from tests/golden/cam0_pinhole_full.json (the reference's cam0 settings; k3 .. k6 are 0)"""
    g = json.load(open(os.path.join(HERE, "golden", "cam0_pinhole_full.json")))
    d, p = g["distortion_parameters"], g["projection_parameters"]
    return np.array([p["fx"], p["fy"], p["cx"], p["cy"], d["k1"], d["k2"], d["p1"], d["p2"], d["k3"], d["k4"], d["k5"], d["k6"]])


CAM = load_cam()
# the same camera with the rational terms switched on, so that every coefficient of the lift takes part
CAM_RATIONAL = np.concatenate([CAM[:8], [0.012, 0.015, -0.008, 0.004]])


def rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def motion_of(kind, rng, baseline=1.0):
    """(R, t): P_prev = R P_cur + t; baseline scales the translation"""
    R = rot(_unit(rng) * rng.uniform(0.01, 0.05))
    if kind == "general":
        return R, _unit(rng) * rng.uniform(0.15, 0.4) * baseline
    if kind == "forward":
        return R, np.array([0.02, -0.01, 1.0]) * rng.uniform(0.2, 0.5) * baseline
    if kind == "sideways":
        return R, np.array([1.0, 0.05, 0.02]) * rng.uniform(0.15, 0.4) * baseline
    return rot(_unit(rng) * rng.uniform(0.03, 0.08)), np.zeros(3)


def true_F(R, t):
    """in the virtual camera's pixels: m_prev^T F m_cur = 0"""
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    Ki = np.linalg.inv(np.array([[FOCAL, 0, COL / 2.0], [0, FOCAL, ROW / 2.0], [0, 0, 1.0]]))
    return Ki.T @ E @ Ki


def gen_pair(seed, n, outliers=0.25, flags=1, motion="general", fail=None, cam=None, noise=NOISE, baseline=1.0):
    """one pair of n tracks.  fail: None, "few" (n is taken as given, < 8), "bad" (a non-finite pixel, or dt not positive) or "nomodel"
    (every current pixel the same: no sample can be normalised).  Returns a dict; `outlier` marks the displaced tracks, cur0 / prev0 are
    the noise-free pixels, F_true the fundamental matrix of the motion in the virtual camera (None for a pure rotation)."""
    cam = CAM if cam is None else cam
    rng = np.random.default_rng(seed)
    R, t = motion_of(motion, rng, baseline)
    cur0, prev0 = np.zeros((n, 2)), np.zeros((n, 2))
    k = 0
    while k < n:                                          # tracks visible in both images
        m = max(2 * (n - k), 16)
        px = np.stack([rng.uniform(15, COL - 15, m), rng.uniform(15, ROW - 15, m)], axis=1)
        xy, _ = npt.lift(cam, px)
        P = np.concatenate([xy, np.ones((m, 1))], axis=1) * rng.uniform(3.0, 20.0, m)[:, None]
        Q = P @ R.T + t
        c, p = npt.distort(cam, P[:, :2] / P[:, 2:3]), npt.distort(cam, Q[:, :2] / Q[:, 2:3])
        ok = (Q[:, 2] > 1.0) & (p[:, 0] > 15) & (p[:, 0] < COL - 15) & (p[:, 1] > 15) & (p[:, 1] < ROW - 15)
        take = min(int(ok.sum()), n - k)
        cur0[k:k + take], prev0[k:k + take] = c[ok][:take], p[ok][:take]
        k += take
    d_cur, d_prev = noise * rng.standard_normal((n, 2)), noise * rng.standard_normal((n, 2))
    cur, prev = cur0 + d_cur, prev0 + d_prev
    n_out = int(round(outliers * n)) if n >= 9 else 0
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:n_out]] = True
    F = None if motion == "rotation" else true_F(R, t)
    for i in np.flatnonzero(out):
        for _ in range(200):
            a, mag = rng.uniform(0, 2 * np.pi), rng.uniform(20.0, 100.0)
            q = prev0[i] + mag * np.array([np.cos(a), np.sin(a)])
            if not (15 < q[0] < COL - 15 and 15 < q[1] < ROW - 15):
                continue
            if F is not None and epipolar_px(F, cam, cur[i:i + 1], q[None])[0] < 10.0:
                continue
            prev[i] = q
            break
        else:
            out[i] = False
    dt = float(rng.uniform(0.03, 0.12))
    if fail == "nomodel":
        cur = np.tile(cur[:1], (n, 1))
        out[:] = True
    if fail == "bad":
        which = int(rng.integers(0, 4 * n + 1))
        if which == 4 * n:
            dt = (0.0, -0.05, np.nan)[seed % 3]
        elif which < 2 * n:
            cur[which // 2, which % 2] = (np.nan, np.inf)[which % 2]
        else:
            prev[(which - 2 * n) // 2, which % 2] = (-np.inf, np.nan)[which % 2]
    return dict(n=n, cur=cur, prev=prev, cur0=cur0, prev0=prev0, d_cur=d_cur, d_prev=d_prev, dt=dt, outlier=out, flags=flags, fail=fail,
                seed=seed, motion=motion, cam=cam, R=R, t=t, F_true=F)


def epipolar_px(F, cam, cur, prev):
    """sqrt of the symmetric epipolar distance, in virtual-camera pixels, of pixel pairs under F (float64, unrounded)"""
    xc, _ = npt.lift(cam, cur)
    xp, _ = npt.lift(cam, prev)
    virt = npt.virtual_of(xc, xp, COL, ROW, FOCAL, 0)
    sc = npt.score(virt, np.asarray(F, np.float64).reshape(1, 9), THRESHOLD)
    return np.sqrt(np.asarray(sc["e2"][0], np.float64))


def pack(pairs):
    """the leading arguments of solver.track_reject_batch: lists of per-pair arrays, then the camera and dt"""
    assert all(p["cam"] is pairs[0]["cam"] for p in pairs)
    return [p["cur"] for p in pairs], [p["prev"] for p in pairs], pairs[0]["cam"], np.array([p["dt"] for p in pairs])
