"""Inputs for the IMU frame front (tests/test_imu_frame.py, tests/perf/bench_imu_frame.py): frames as tests/np_imu_frame.py takes them,
with the raw samples GetImuInterval (R/swf/swf_imu.cpp:82-106) would return: every sample with t0 < t < t1, then one with t >= t1.

Decisive by construction: every time stamp is a multiple of Q = 2^-20 s and t1 is either a sample's own stamp or at least 2 Q ~ 1.9e-6 s
away from every sample; sums and differences of the stamps are exact in float64."""
import numpy as np

Q = 2.0 ** -20                      # the time grid
PBG = np.array([0.12, -0.31, 0.07])
G_W = np.array([0.0, 0.0, 9.8])
NOISE = (0.08, 0.004, 0.00004, 2.0e-6)


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def gen_frame(seed, n_raw, last="beyond", flag=0, fail=None, rate=400.0):
    """One frame with n_raw raw samples.  last: "beyond" (the last sample lies beyond t1 and is blended) or "at" (it sits exactly on t1).
    fail: None, "empty", "no_inner" (the first sample is already beyond t1), "order" (an inner stamp steps back) or "order0" (the first
    stamp lies before t0)."""
    rng = np.random.default_rng(seed)
    t0 = np.round(rng.uniform(100.0, 5000.0) / Q) * Q
    if fail == "empty":
        n_raw = 0
    if fail == "no_inner":
        n_raw = max(n_raw, 1)
    step = np.round((1.0 / rate) * (1 + rng.uniform(-0.2, 0.2, max(n_raw, 1))) / Q) * Q
    t = t0 + np.cumsum(step)                                              # t0 < t_0 < t_1 < ...
    if n_raw == 0:
        t1 = t0 + 0.05
    elif fail == "no_inner":
        t1 = t[0] - max(2, int(rng.integers(2, int(step[0] / Q) - 2))) * Q
    elif last == "at":
        t1 = t[n_raw - 1]
    else:
        t1 = t[n_raw - 1] - max(2, int(rng.integers(2, int(step[n_raw - 1] / Q) - 2))) * Q     # inside the last step, >= 2 Q from both ends
    t = t[:n_raw]
    if fail == "order":
        assert n_raw >= 3
        k = int(rng.integers(1, n_raw - 1))
        t[k] = t[k - 1] - 3 * Q
    if fail == "order0":
        t[0] = t0 - 5 * Q
    tt = t - t0
    w0 = rng.normal(0, 0.3, 3); a0 = rng.normal(0, 1.0, 3) + np.array([0, 0, 9.8])
    raw = np.zeros((n_raw, 7))
    raw[:, 0] = t
    raw[:, 1:4] = a0 + 0.5 * np.sin(np.outer(tt, rng.uniform(1, 20, 3))) + rng.normal(0, 0.05, (n_raw, 3))
    raw[:, 4:7] = w0 + 0.2 * np.cos(np.outer(tt, rng.uniform(1, 20, 3))) + rng.normal(0, 0.005, (n_raw, 3))
    state = np.concatenate([rng.normal(0, 100.0, 3), _rot(rng).ravel(), rng.normal(0, 3.0, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)])
    return dict(raw=raw, t01=np.array([t0, t1]), seed=np.concatenate([a0 + rng.normal(0, 0.05, 3), w0 + rng.normal(0, 0.005, 3)]),
                state=state, gyrj_prev=w0 + rng.normal(0, 0.01, 3), flag=int(flag), fail=fail)


def pack(frames):
    """the arguments of solver.imu_frame_batch up to pbg: raw list, t01, seed, state, gyrj_prev, flags"""
    n = len(frames)
    return ([f["raw"] for f in frames], np.array([f["t01"] for f in frames]).reshape(n, 2), np.array([f["seed"] for f in frames]).reshape(n, 6),
            np.array([f["state"] for f in frames]).reshape(n, 21), np.array([f["gyrj_prev"] for f in frames]).reshape(n, 3),
            np.array([f["flag"] for f in frames], np.int32))
