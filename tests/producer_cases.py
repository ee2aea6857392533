"""Seeded inputs of tests/test_producers.py, shared by its CPU and GPU tests: intervals for k_preintegrate, scenes for k_triangulate,
factors for k_eval_idepth.  Small on purpose: the longdouble referees of np_producers.py run over all of them in a few seconds."""
import functools

import numpy as np

import np_producers as npp

NOISE = (0.05, 0.005, 0.0005, 0.00005)                   # ACC_N, GYR_N, ACC_W, GYR_W (R/parameter/parameters.cpp:24-27)
PBG = np.array([-0.0051302024, 0.0091942546, 0.308739733])
SQRT_INFO = 1000.0 / 1.5                                  # FOCAL_LENGTH / FEATUREWEIGHTINVERSE
INIT_DEPTH = 5.0


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def _rotvec(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _quat(v):
    """unit quaternion (x, y, z, w) of the rotation vector v"""
    th = np.linalg.norm(v)
    q = np.concatenate([np.sin(th / 2) * v / th if th else np.zeros(3), [np.cos(th / 2)]])
    return q / np.linalg.norm(q)


# ------------------------------------------------------------------------------------------------------------ pre-integration
def imu_samples(rng, n, dt=0.0025, jitter=True, rate=0.3, acc_sigma=1.0):
    """a plausible IMU stream: gravity-ish specific force, a rotation rate of `rate` rad/s, per-sample dt jitter"""
    t = np.cumsum(np.full(n, dt))
    s = np.zeros((n, 7))
    s[:, 0] = dt * (1 + (rng.uniform(-0.2, 0.2, n) if jitter else 0))
    w0 = rng.normal(0, 1, 3)
    w0 *= rate / np.linalg.norm(w0)
    a0 = rng.normal(0, acc_sigma, 3) + np.array([0, 0, 9.8])
    s[:, 1:4] = a0 + 0.5 * np.sin(np.outer(t, rng.uniform(1, 20, 3))) + rng.normal(0, 0.05, (n, 3))
    s[:, 4:7] = w0 + 0.2 * np.cos(np.outer(t, rng.uniform(1, 20, 3))) + rng.normal(0, 0.005, (n, 3))
    return s


# the fixed lengths, ordered so that the four intervals of one wavefront differ widely, then a dozen random ones
FIXED_LENGTHS = (400, 1, 3, 41, 161, 2, 17, 64, 100, 4, 40, 5)


@functools.lru_cache(maxsize=None)
def preint_cases():
    """list of dict(name, samples [n][7], bias [6]): the length sweep, then the edge intervals"""
    rng = np.random.default_rng(20240611)
    lens = list(FIXED_LENGTHS) + [int(v) for v in rng.integers(2, 81, 12)]
    out = []
    for i, n in enumerate(lens):
        out.append(dict(name="len%d" % n, samples=imu_samples(rng, n, jitter=(i % 3 != 0)),
                        bias=np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)])))
    small = lambda: np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)])
    s = imu_samples(rng, 12)
    s[6, 0] = 0.0                                         # a duplicate timestamp
    out.append(dict(name="dt0_row", samples=s, bias=small()))
    out.append(dict(name="dt_0.1", samples=imu_samples(rng, 10, dt=0.1), bias=small()))
    out.append(dict(name="rate_10", samples=imu_samples(rng, 20, dt=0.01, rate=10.0), bias=small()))
    out.append(dict(name="rate_10_dt_0.1", samples=imu_samples(rng, 6, dt=0.1, rate=10.0), bias=small()))
    b = np.concatenate([rng.choice([-1.0, 1.0], 3) * 1.0, rng.choice([-1.0, 1.0], 3) * 0.2])
    out.append(dict(name="large_bias", samples=imu_samples(rng, 15), bias=b))
    out.append(dict(name="one_sample", samples=imu_samples(rng, 1), bias=small()))
    out.append(dict(name="one_push_back", samples=imu_samples(rng, 2), bias=small()))
    out.append(dict(name="one_push_back_b", samples=imu_samples(rng, 2, dt=0.01), bias=small()))
    s = imu_samples(rng, 3)
    s[2, 0] = 0.0                                         # the second push_back adds nothing: the covariance keeps rank 12
    out.append(dict(name="push_back_then_dt0", samples=s, bias=small()))
    return out


@functools.lru_cache(maxsize=None)
def one_push_back_cases():
    """96 intervals of one push_back each (two samples): the covariance V Q V^T has rank 12 whatever the samples are, so whether its
    factorisation is refused must not hang on the sign of a rounding residue; dt cycles through 2.5, 5 and 10 ms, with jitter"""
    rng = np.random.default_rng(626)
    return [dict(name="pb1_%d" % i, samples=imu_samples(rng, 2, dt=(0.0025, 0.005, 0.01)[i % 3]),
                 bias=np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)])) for i in range(96)]


PREINT_SUBBATCHES = (1, 3, 4, 5)                          # intervals per call: partial wavefronts


@functools.lru_cache(maxsize=None)
def preint_runs_case():
    """a two-run gather per interval out of one resident sample array: (samples [N][7], runs, rows per interval, biases)"""
    rng = np.random.default_rng(515)
    pool = imu_samples(rng, 120)
    runs = [[(10, 7), (40, 9)], [(0, 1), (100, 20)], [(60, 3), (5, 2)], [(30, 30), (90, 11)], [(70, 2), (20, 1)]]
    rows = [np.concatenate([pool[o:o + c] for o, c in r]) for r in runs]
    bias = np.concatenate([rng.normal(0, 0.05, (len(runs), 3)), rng.normal(0, 0.005, (len(runs), 3))], axis=1)
    return pool, runs, rows, bias


# ------------------------------------------------------------------------------------------------------------ triangulation
TRI_COUNTS = (1, 255, 256, 257, 600)                      # 256 lanes per block


def _project(Ps, Rs, tic, ric, f, Xw):
    q = ric.T @ (Rs[f].T @ (Xw - Ps[f]) - tic)
    return q[:2] / q[2]


@functools.lru_cache(maxsize=None)
def tri_scene():
    """40 frames along a gently curving path; 600 features, the first 65 the special ones: 0-4 identical observations, 5-9 behind the
    camera, 10-11 out-of-range starts, 12-16 on the pure-rotation pair, 17-19 on the baseline, 20-39 about 0.2 m deep, 40-59 about 300 m,
    60-64 starting in the last valid frame.  Returns dict(Ps, Rs, tic, ric, pbg, start, pt0, pt1, tag [n]).  tag: "" = not degenerate
    by construction; the others name the case."""
    rng = np.random.default_rng(907)
    nfr, n = 40, 600
    Ps = np.cumsum(rng.normal([0.6, 0.05, 0.0], 0.05, (nfr, 3)), axis=0)
    Rs = np.stack([_rotvec(rng.normal(0, 0.05, 3) + np.array([0, 0, 0.02 * k])) for k in range(nfr)])
    ric = _rot(2, -1.55) @ _rot(1, 0.02) @ _rot(0, -1.5)
    tic = np.array([0.05, -0.02, 0.1])
    Ps[6] = Ps[5] + Rs[5] @ tic - Rs[6] @ tic             # frames 5, 6: one camera centre, two orientations (pure rotation)
    start = rng.integers(0, nfr - 1, n).astype(np.int32)
    start[(start == 5)] = 7                               # the pure-rotation pair is for features 12-16 alone
    tag = np.array([""] * n, dtype=object)
    depth = rng.uniform(3, 40, n)
    depth[20:40], depth[40:60] = rng.uniform(0.15, 0.25, 20), rng.uniform(250, 350, 20)
    start[12:17] = 5
    start[60:65] = nfr - 2
    pt0, pt1 = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(n):
        f = int(start[i])
        pc = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0]) * depth[i]
        Xw = Rs[f] @ (ric @ pc + tic) + Ps[f]
        if 17 <= i < 20:                                  # on the baseline, ahead of both cameras
            c0, c1 = Ps[f] + Rs[f] @ tic, Ps[f + 1] + Rs[f + 1] @ tic
            Xw = c0 + (3.0 + i) * (c1 - c0)
        pt0[i], pt1[i] = _project(Ps, Rs, tic, ric, f, Xw), _project(Ps, Rs, tic, ric, f + 1, Xw)
    pt0 += rng.normal(0, 1e-3, pt0.shape)
    pt1 += rng.normal(0, 1e-3, pt1.shape)
    pt1[0:5] = pt0[0:5]
    tag[0:5] = "identical"
    pt0[5:10] = -3 * pt0[5:10] + 1.0
    pt1[5:10] = -2.0
    tag[5:10] = "behind"
    start[10], start[11] = nfr - 1, -1
    tag[10:12] = "out_of_range"
    tag[12:17] = "pure_rotation"
    tag[17:20] = "on_baseline"
    return dict(Ps=Ps, Rs=Rs, tic=tic, ric=ric, pbg=np.array([0.1, -0.3, 0.2]), start=start, pt0=pt0, pt1=pt1, tag=tag)


@functools.lru_cache(maxsize=None)
def tri_two_frames():
    """n_frames = 2: start = 0 = n_frames - 2 is the only valid start; 1 and -1 are out of range"""
    rng = np.random.default_rng(908)
    sc = tri_scene()
    Ps, Rs = sc["Ps"][8:10].copy(), sc["Rs"][8:10].copy()
    n = 24
    start = np.zeros(n, np.int32)
    start[20], start[21] = 1, -1
    pt0, pt1 = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(n):
        pc = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0]) * rng.uniform(3, 40)
        Xw = Rs[0] @ (sc["ric"] @ pc + sc["tic"]) + Ps[0]
        pt0[i], pt1[i] = _project(Ps, Rs, sc["tic"], sc["ric"], 0, Xw), _project(Ps, Rs, sc["tic"], sc["ric"], 1, Xw)
    pt0 += rng.normal(0, 1e-3, pt0.shape)
    pt1 += rng.normal(0, 1e-3, pt1.shape)
    tag = np.array([""] * n, dtype=object)
    tag[20:22] = "out_of_range"
    return dict(Ps=Ps, Rs=Rs, tic=sc["tic"], ric=sc["ric"], pbg=sc["pbg"], start=start, pt0=pt0, pt1=pt1, tag=tag)


def tri_args(sc, n=None):
    n = len(sc["start"]) if n is None else n
    return (sc["Ps"], sc["Rs"], sc["tic"], sc["ric"], sc["pbg"], sc["start"][:n], sc["pt0"][:n], sc["pt1"][:n])


# ------------------------------------------------------------------------------------------------------------ inverse depth
IDEPTH_COUNTS = (1, 127, 128, 129, 300)                   # 128 lanes per block
LAMBDAS = (1e-3, 0.03, 0.3, 5.0)
Z_NEAR = 0.05


@functools.lru_cache(maxsize=None)
def idepth_factors():
    """300 factors, kinds cycling 0, 1, 2 and lambda cycling LAMBDAS; factors 30 .. 41 have the point Z_NEAR in front of the projecting
    camera.  Returns dict(kind [n], idx [n][5], poses [4 n][7], lam [n], pts [n][6]): factor q owns poses 4 q .. 4 q + 3 = pose_i,
    pose_j, ex, ex2 and lambda q; idx is -1 where the kind has no such block."""
    rng = np.random.default_rng(31337)
    n = 300
    Rbc = _rot(2, -1.57) @ _rot(1, 0.01) @ _rot(0, -1.56)
    # (x, y, z, w) of Rbc through a rotation vector: log of the matrix
    ang = np.arccos((np.trace(Rbc) - 1) / 2)
    ax = np.array([Rbc[2, 1] - Rbc[1, 2], Rbc[0, 2] - Rbc[2, 0], Rbc[1, 0] - Rbc[0, 1]]) / (2 * np.sin(ang))
    qic = _quat(ax * ang)
    kind, idx, poses, lam, pts = [], [], [], [], []
    for q in range(n):
        k = q % 3
        Pi = np.concatenate([rng.normal(0, 5, 3), _quat(rng.normal(0, 0.3, 3))])
        Pj = npp.pose_plus(Pi, np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.05, 3)]))
        ex = np.concatenate([[0.013, 0.057, -0.015], qic])
        ex2 = npp.pose_plus(ex, np.array([0.12, 0.0, 0.0, 0.01, -0.02, 0.005]))
        L = LAMBDAS[(q // 3) % 4]
        pts_i = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0])
        cam = ex if k == 0 else ex2
        if 30 <= q < 42:
            # move the projecting camera along its own axis until the point is Z_NEAR in front of it
            L = 0.3
            _, pcj = npp.idepth_residual(k, Pi, Pj, ex, cam, L, pts_i, np.zeros(3), SQRT_INFO, PBG)
            pts_i = pts_i * np.array([0.02, 0.02, 1.0])   # near the axis, so that it stays in view
            _, pcj = npp.idepth_residual(k, Pi, Pj, ex, cam, L, pts_i, np.zeros(3), SQRT_INFO, PBG)
            shift = npp.q2R(cam[3:]) @ np.array([0, 0, pcj[2] - Z_NEAR])
            if k == 2:
                ex2 = np.concatenate([ex2[:3] + shift, ex2[3:]])
            else:
                Pj = np.concatenate([Pj[:3] + npp.q2R(Pj[3:]) @ shift, Pj[3:]])
            cam = ex if k == 0 else ex2
        r0, _ = npp.idepth_residual(k, Pi, Pj, ex, cam, L, pts_i, np.zeros(3), SQRT_INFO, PBG)
        pj = r0 / SQRT_INFO + rng.normal(0, 1e-3, 2)
        b = 4 * q
        poses += [Pi, Pj, ex, ex2]
        lam.append(L)
        kind.append(k)
        idx.append([b if k != 2 else -1, b + 1 if k != 2 else -1, b + 2, b + 3 if k != 0 else -1, q])
        pts.append(np.concatenate([pts_i, [pj[0], pj[1], 1.0]]))
    return dict(kind=np.array(kind, np.int32), idx=np.array(idx, np.int32), poses=np.array(poses), lam=np.array(lam), pts=np.array(pts))
