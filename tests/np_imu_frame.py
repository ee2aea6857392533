"""numpy referee of the IMU frame front: SWFOptimization::ImuIntegrate and IMUProcess (R/swf/swf_imu.cpp:117-213) and the sample push
of SlideWindowFrame (R/swf/swf.cpp:241-247), restated.  Parameterised by dtype (float64, longdouble); order="alt" regroups the sums
of the float64 arithmetic (a second legitimate operation order, for measuring the tolerance constant).

A frame is a dict: raw [n][7] (t, acc, gyr), t01 (t0, t1), seed [6] (acc_0, gyr_0), state [21] (P, R row-major, V, ba, bg),
gyrj_prev [3], flag (bit 0: velocity lever arm)."""
import numpy as np

OK, EMPTY, NO_INNER, TIME_ORDER = 0, 1, 2, 3
EPS = 2.0 ** -52


def cut(raw, t0, t1, dtype=np.float64):
    """(code, rows): rows [m][7] = the (dt, acc, gyr) of every IMUProcess call of the frame (without the seed row).  A sample with
    t <= t1 is used as it is; the one beyond is blended onto t1 with the raw sample before it and is the last one used."""
    raw = np.asarray(raw, np.float64).reshape(-1, 7)
    if raw.shape[0] == 0:
        return EMPTY, None
    if not raw[0, 0] <= t1:
        return NO_INNER, None
    r = raw.astype(dtype)
    t0, t1 = dtype(t0), dtype(t1)
    rows, cur, prev = [], t0, np.zeros(6, dtype)
    for i in range(r.shape[0]):
        t = r[i, 0]
        if t <= t1:
            dt = t - cur
            if dt < 0:
                return TIME_ORDER, None
            cur = t
            prev = r[i, 1:]
            rows.append(np.concatenate([[dt], prev]))
        else:
            dt_1, dt_2 = t1 - cur, t - t1
            w1, w2 = dt_2 / (dt_1 + dt_2), dt_1 / (dt_1 + dt_2)
            rows.append(np.concatenate([[dt_1], w1 * prev + w2 * r[i, 1:]]))
            break
    return OK, np.array(rows, dtype).reshape(-1, 7)


def M_theta(theta, dtype=np.float64):
    """What the reference multiplies R by: Eigen's toRotationMatrix applied to the UNNORMALISED quaternion (w, v) = (1, theta / 2)
    that Utility::deltaQ returns.  Not a rotation: M - I = (1 + |v|^2) (Rn - I) with Rn the rotation of the normalised quaternion."""
    x, y, z = [dtype(v) / dtype(2) for v in theta]
    w = dtype(1)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype)


def rotation_of(theta):
    """the orthonormal rotation of the normalised quaternion (1, theta / 2) / |.| (what a "corrected" restatement would form)"""
    v = np.asarray(theta, np.float64) / 2
    s = float(v @ v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + (2 * K + 2 * (np.outer(v, v) - s * np.eye(3))) / (1 + s)


def _mv(R, v, alt):
    if alt:
        return np.array([R[a, 2] * v[2] + (R[a, 1] * v[1] + R[a, 0] * v[0]) for a in range(3)], R.dtype)
    return np.array([R[a, 0] * v[0] + R[a, 1] * v[1] + R[a, 2] * v[2] for a in range(3)], R.dtype)


def _mm(A, B, alt):
    if alt:
        return np.array([[A[i, 2] * B[2, j] + (A[i, 1] * B[1, j] + A[i, 0] * B[0, j]) for j in range(3)] for i in range(3)], A.dtype)
    return np.array([[A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)], A.dtype)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def predict(rows, seed, state, gyrj_prev, flag, pbg, g_w, dtype=np.float64, order="reference"):
    """(pred [15], scales): P, R, V after the lever arm came off, the mid-point steps ran and the lever arm went back on.  scales =
    (max |P| + |V| T + |un_acc| T^2, max |V| + |un_acc| T, max |R|) over the steps, T the frame's span: what the brackets are made of."""
    alt = order == "alt"
    c = lambda v: np.asarray(v, np.float64).astype(dtype)
    rows, seed, state, gyrj_prev, pbg, g_w = c(rows), c(seed), c(state), c(gyrj_prev), c(pbg), c(g_w)
    P, R, V, ba, bg = state[0:3].copy(), state[3:12].reshape(3, 3).copy(), state[12:15].copy(), state[15:18], state[18:21]
    acc_0, gyr_0 = seed[:3], seed[3:]
    half, two = dtype(0.5), dtype(2)
    P = P - _mv(R, pbg, alt)
    if flag & 1:
        V = V - _mv(R, _cross(gyrj_prev - bg, pbg), alt)
    T = rows[:, 0].sum()
    nrm = lambda v: float(np.sqrt((v.astype(np.float64) ** 2).sum()))
    sP = sV = sR = 0.0
    for k in range(rows.shape[0]):
        dt, acc, gyr = rows[k, 0], rows[k, 1:4], rows[k, 4:7]
        un_acc_0 = _mv(R, acc_0 - ba, alt) - g_w
        un_gyr = half * (gyr_0 + gyr) - bg
        R = _mm(R, M_theta(un_gyr * dt, dtype), alt)
        un_acc_1 = _mv(R, acc - ba, alt) - g_w
        if alt:
            un_acc = half * un_acc_0 + half * un_acc_1
            P = P + dt * (V + (half * dt) * un_acc)
        else:
            un_acc = half * (un_acc_0 + un_acc_1)
            P = P + (dt * V + half * dt * dt * un_acc)
        V = V + dt * un_acc
        acc_0, gyr_0 = acc, gyr
        sP = max(sP, nrm(P) + nrm(V) * float(T) + nrm(un_acc) * float(T) ** 2)
        sV = max(sV, nrm(V) + nrm(un_acc) * float(T))
        sR = max(sR, float(np.abs(R).max()))
    P = P + _mv(R, pbg, alt)
    if flag & 1:
        V = V + _mv(R, _cross(gyr_0 - bg, pbg), alt)
    sP, sV = max(sP, nrm(P)), max(sV, nrm(V))
    return np.concatenate([P, R.ravel(), V]), (sP, sV, sR)


def frame(f, pbg, g_w, dtype=np.float64, order="reference"):
    """One frame: dict(code, cut [m + 1][7] with the seed row first, pred [15], bracket [15]) (code only for a failed frame)."""
    code, rows = cut(f["raw"], f["t01"][0], f["t01"][1], dtype)
    if code != OK:
        return dict(code=code)
    pred, (sP, sV, sR) = predict(rows, f["seed"], f["state"], f["gyrj_prev"], f["flag"], pbg, g_w, dtype, order)
    n = rows.shape[0]
    br = EPS * n * np.concatenate([np.full(3, sP), np.full(9, sR), np.full(3, sV)])
    seed_row = np.concatenate([[0.0], np.asarray(f["seed"], np.float64)]).astype(dtype)
    return dict(code=code, cut=np.vstack([seed_row, rows]), pred=pred, bracket=br)


def merged_rows(cut_k, cut_k1):
    """SlideWindowFrame (R/swf/swf.cpp:241-247): interval k+1's samples pushed onto interval k's pre-integration: the rows of k, then the
    rows of k+1 without its seed row."""
    return np.vstack([cut_k, cut_k1[1:]])
