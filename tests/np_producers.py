"""numpy referees of the three stand-alone producer kernels of csrc/swf_producers.hip, written from the reference's lines:
  preintegrate   IntegrationBase::{ctor, push_back, propagate, midPointIntegration, get_sqrtinfo}   R/factor/integration_base.cpp:5-142
  triangulate    FeatureManager::triangulate (two-view branch) and triangulatePoint                 R/feature/feature_manager.cpp:148-161, 285-316
  eval_idepth    ProjectionTwoFrameOneCam / TwoFrameTwoCam / OneFrameTwoCam ::Evaluate                R/factor/projection_factor.cpp:77-329
Every function takes dtype = np.float64 | np.longdouble; nothing here calls LAPACK in longdouble (Cholesky, LU, triangular solves and the
one-sided Jacobi are written out), and nothing comes from oracle/ or synth.py.  order="alt" is a second legitimate float64 operation
order (regrouped sums, F (cov F^T) for (F cov) F^T, LAPACK's SVD for the Jacobi): it exists to measure the tolerance constant M.

Each referee returns, next to its values, a BRACKET per compared quantity: a float64 magnitude such that a correct float64 evaluation
lies within a small multiple of 2^-52 * bracket of the exact value.  The brackets are derived (docstrings below), never fitted."""
import numpy as np

EPS = 2.0 ** -52
# record layout (include/swf_types.h)
DP, DQ, DV, LBA, LBG, DP_DBA, DP_DBG, DQ_DBG, DV_DBA, DV_DBG, SUMDT, GYRI, GYRJ, SQRTINFO, PRE_DOUBLES = 0, 3, 7, 10, 13, 16, 25, 34, 43, 52, 61, 62, 65, 68, 293
# (name, record slice, rows, columns of the 15x15 jacobian)
JAC_BLOCKS = (("dp_dba", DP_DBA, 0, 9), ("dp_dbg", DP_DBG, 0, 12), ("dq_dbg", DQ_DBG, 3, 12), ("dv_dba", DV_DBA, 6, 9), ("dv_dbg", DV_DBG, 6, 12))
# a pivot of the reverse Cholesky below this share of its own diagonal entry means a rank-deficient covariance: a regular one has a
# scaled condition number of 13 .. 28 on every input of producer_cases.py, a singular one leaves rounding noise (2^-52), so 2^-20
# has four orders of magnitude to one side and nine to the other; the kernel's PI_RANK_TOL is the same number
RANK_TOL = 2.0 ** -20


def _c(v, dtype):
    return np.asarray(v, np.float64).astype(dtype)


def _f(v):
    return np.asarray(v).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ small algebra
def q2R(q):
    """Eigen's Quaternion::toRotationMatrix for q = (x, y, z, w), NOT normalised first"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], q.dtype)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def qrot(q, v):
    """Eigen's Quaternion * Vector3 (v + 2 w (u x v) + 2 u x (u x v)): the unit-quaternion formula applied to whatever q is"""
    uv = _cross(q[:3], v)
    uv = uv + uv
    return v + q[3] * uv + _cross(q[:3], uv)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def qinv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2], q.dtype)


def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def _mm(A, B, alt=False):
    """a 3-term (or longer) product written out, so that float64 and longdouble run the same sums; alt sums from the other end"""
    if alt:
        return _mm_rev(A, B)
    out = np.zeros((A.shape[0], B.shape[1]), A.dtype)
    for k in range(A.shape[1]):
        out = out + A[:, k:k + 1] * B[k:k + 1, :]
    return out


def _mm_rev(A, B):
    out = np.zeros((A.shape[0], B.shape[1]), A.dtype)
    for k in range(A.shape[1] - 1, -1, -1):
        out = out + A[:, k:k + 1] * B[k:k + 1, :]
    return out


# ------------------------------------------------------------------------------------------------------------ pre-integration
def chol_reverse_inverse(cov):
    """route (a), the device's: cov = R R^T with R upper triangular, built from the last column backwards; returns (R^-1, regular).
    R^-1 is upper triangular with a positive diagonal and (R^-1)^T R^-1 = cov^-1."""
    dt = cov.dtype
    n = cov.shape[0]
    A = cov.copy()
    R = np.zeros((n, n), dt)
    d0 = _f(np.diag(cov))
    for j in range(n - 1, -1, -1):
        if not (_f(A[j, j]) > RANK_TOL * d0[j]) or not np.isfinite(_f(A[j, j])):
            return np.zeros((n, n), dt), False
        R[j, j] = np.sqrt(A[j, j])
        R[:j, j] = A[:j, j] / R[j, j]
        A[:j, :j] = A[:j, :j] - np.outer(R[:j, j], R[:j, j])
    U = np.zeros((n, n), dt)
    for c in range(n):                                     # R u = e_c, backwards
        U[c, c] = 1 / R[c, c]
        for i in range(c - 1, -1, -1):
            U[i, c] = -(R[i, i + 1:c + 1] * U[i + 1:c + 1, c]).sum() / R[i, i]
    return U, True


def inverse_then_llt(cov):
    """route (b), the reference's (integration_base.cpp:109): an explicit inverse (LU with partial pivoting, as Eigen's inverse() of a
    15x15 takes), then the lower Cholesky factor of it, transposed."""
    dt = cov.dtype
    n = cov.shape[0]
    A = np.concatenate([cov.copy(), np.eye(n, dtype=dt)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
        A[k] = A[k] / A[k, k]
        for i in range(n):
            if i != k:
                A[i] = A[i] - A[i, k] * A[k]
    inv = A[:, n:]
    inv = (inv + inv.T) / 2
    L = np.zeros((n, n), dt)
    for j in range(n):
        d = inv[j, j] - (L[j, :j] * L[j, :j]).sum()
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (inv[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L.T


def scaled_condition(cov):
    """2-norm condition number of D cov D, D = diag(cov)^-1/2, in float64 (a magnitude, not a compared value)"""
    c = _f(cov)
    d = 1 / np.sqrt(np.diag(c))
    return float(np.linalg.cond(c * np.outer(d, d)))


def preintegrate(samples, ba, bg, noise, dtype=np.float64, order="reference"):
    """IntegrationBase over samples [n][7] = (dt, acc, gyr), the first row seeding acc_0 / gyr_0, every further row a push_back.
    noise = (ACC_N, GYR_N, ACC_W, GYR_W).  The quaternion the step forms, delta_q * (1, w dt / 2), is used UNNORMALISED for the second
    rotation q * v and for toRotationMatrix (:40-41, :66-91) and normalised only at the end of propagate (:137).

    Returns dict(record [293], bracket, regular, cond, jacobian, covariance, sqrt_info_b, n_pb).  bracket maps each compared quantity to a
    float64 magnitude; with n_pb push_backs and T = sum dt, maxima over the steps:
      dp      n_pb max(|dp| + |dv| T + |un_acc| T^2)      dv   n_pb max(|dv| + |un_acc| T)       (np_imu_frame.predict's form)
      dq      n_pb max(|delta_q| (x) |(w dt / 2, 1)|)  (the products of the quaternion multiplication, magnitudes summed)
      sum_dt  n_pb sum dt
      each bias-Jacobian block: n_pb max((|F| |jacobian|) over the block): the sums jacobian = F jacobian forms, magnitudes summed
      sqrt_info row i: n_pb * cond * max_j |sqrt_info[i][j]|, cond = the scaled condition number of the covariance: the recursion
              leaves the covariance with a scaled relative error of n_pb roundings, which the factor's inverse magnifies by cond.
    A rank-deficient covariance (no push_back, one push_back: rows 0-2 of V are dt / 2 times rows 6-8; all-zero noise) has no
    sqrt_info: zeros, as the device and the oracle write."""
    alt = order == "alt"
    s = _c(samples, dtype).reshape(-1, 7)
    ba, bg = _c(ba, dtype), _c(bg, dtype)
    an2, gn2, aw2, gw2 = [dtype(float(v)) * dtype(float(v)) for v in noise]
    n = s.shape[0]
    half, quarter, one = dtype(0.5), dtype(0.25), dtype(1)
    I3 = np.eye(3, dtype=dtype)
    dp, dv, dq = np.zeros(3, dtype), np.zeros(3, dtype), np.array([0, 0, 0, 1], dtype)
    J, P = np.eye(15, dtype=dtype), np.zeros((15, 15), dtype)
    Q = np.zeros((18, 18), dtype)
    for b, v in enumerate((an2, gn2, an2, gn2, aw2, gw2)):
        Q[3 * b:3 * b + 3, 3 * b:3 * b + 3] = v * I3
    acc0, gyr0 = s[0, 1:4].copy(), s[0, 4:7].copy()
    gyri = gyr0.copy()
    sum_dt = dtype(0)
    T = float(_f(s[1:, 0]).sum())
    m_dp = m_dv = m_dq = 0.0
    nrm = lambda v: float(np.abs(_f(v)).max())
    m_blk = {name: 0.0 for name, _, _, _ in JAC_BLOCKS}
    for k in range(1, n):
        dt, acc1, gyr1 = s[k, 0], s[k, 1:4], s[k, 4:7]
        a0, a1 = acc0 - ba, acc1 - ba
        w = half * (gyr0 + gyr1) - bg
        un0 = qrot(dq, a0)
        hq = np.array([w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, one], dtype)
        rq = qmul(dq, hq)
        un1 = qrot(rq, a1)
        un = half * (un0 + un1) if not alt else half * un0 + half * un1
        if alt:
            rp = dp + dt * (dv + (half * dt) * un)
        else:
            rp = dp + dv * dt + half * un * dt * dt
        rv = dv + un * dt
        R0, R1 = q2R(dq), q2R(rq)
        Rw, Ra0, Ra1 = skew(w), skew(a0), skew(a1)
        ImRw = I3 - Rw * dt
        F = np.zeros((15, 15), dtype)
        V = np.zeros((15, 18), dtype)
        if alt:                                            # the grouping the device takes: M0 + M2, R0 + R1 first
            M1 = _mm(R1, Ra1)
            Ms = _mm(R0, Ra0) + _mm(M1, ImRw)
            Rs_ = R0 + R1
            F[0:3, 3:6] = (-quarter * dt * dt) * Ms
            F[0:3, 9:12] = (-quarter * dt * dt) * Rs_
            F[0:3, 12:15] = (quarter * dt * dt * dt) * M1
            F[6:9, 3:6] = (-half * dt) * Ms
            F[6:9, 9:12] = (-half * dt) * Rs_
            F[6:9, 12:15] = (half * dt * dt) * M1
        else:
            M1 = _mm(R1, Ra1)
            F[0:3, 3:6] = -quarter * _mm(R0, Ra0) * dt * dt + -quarter * _mm(M1, ImRw) * dt * dt
            F[0:3, 9:12] = -quarter * (R0 + R1) * dt * dt
            F[0:3, 12:15] = -quarter * M1 * dt * dt * -dt
            F[6:9, 3:6] = -half * _mm(R0, Ra0) * dt + -half * _mm(M1, ImRw) * dt
            F[6:9, 9:12] = -half * (R0 + R1) * dt
            F[6:9, 12:15] = -half * M1 * dt * -dt
        F[0:3, 0:3] = I3
        F[0:3, 6:9] = I3 * dt
        F[3:6, 3:6] = ImRw
        F[3:6, 12:15] = -I3 * dt
        F[6:9, 6:9] = I3
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V[0:3, 0:3] = quarter * R0 * dt * dt
        V[0:3, 3:6] = quarter * -M1 * dt * dt * half * dt
        V[0:3, 6:9] = quarter * R1 * dt * dt
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = half * I3 * dt
        V[3:6, 9:12] = half * I3 * dt
        V[6:9, 0:3] = half * R0 * dt
        V[6:9, 3:6] = half * -M1 * dt * half * dt
        V[6:9, 6:9] = half * R1 * dt
        V[6:9, 9:12] = V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        terms = np.abs(_f(F)) @ np.abs(_f(J))
        for name, _, r0, c0 in JAC_BLOCKS:
            m_blk[name] = max(m_blk[name], float(terms[r0:r0 + 3, c0:c0 + 3].max()))
        if alt:
            J = _mm_rev(F, J)
            P = _mm_rev(F, _mm_rev(P, F.T)) + _mm_rev(V, _mm_rev(Q, V.T))
        else:
            J = _mm(F, J)
            P = _mm(_mm(F, P), F.T) + _mm(_mm(V, Q), V.T)
        m_dq = max(m_dq, float((np.abs(_f(dq)).sum()) * nrm(hq)))
        dp, dv = rp, rv
        dq = rq / np.sqrt((rq * rq).sum())
        sum_dt = sum_dt + dt
        acc0, gyr0 = acc1, gyr1
        m_dp = max(m_dp, nrm(dp) + nrm(dv) * T + nrm(un) * T * T)
        m_dv = max(m_dv, nrm(dv) + nrm(un) * T)
    n_pb = n - 1
    U, regular = chol_reverse_inverse(P) if n_pb > 0 else (np.zeros((15, 15), dtype), False)
    rec = np.zeros(PRE_DOUBLES, dtype)
    rec[DP:DP + 3], rec[DQ:DQ + 4], rec[DV:DV + 3], rec[LBA:LBA + 3], rec[LBG:LBG + 3] = dp, dq, dv, ba, bg
    for name, off, r0, c0 in JAC_BLOCKS:
        rec[off:off + 9] = J[r0:r0 + 3, c0:c0 + 3].ravel()
    rec[SUMDT] = sum_dt
    rec[GYRI:GYRI + 3], rec[GYRJ:GYRJ + 3] = gyri, gyr0
    rec[SQRTINFO:] = U.ravel()
    cond = scaled_condition(P) if regular else float("inf")
    br = dict(dp=n_pb * m_dp, dq=n_pb * m_dq, dv=n_pb * m_dv, sum_dt=n_pb * float(_f(sum_dt)))
    for name in m_blk:
        br[name] = n_pb * m_blk[name]
    br["sqrt_info"] = n_pb * cond * np.abs(_f(U)).max(axis=1) if regular else np.zeros(15)
    return dict(record=rec, bracket=br, regular=regular, cond=cond, jacobian=J, covariance=P, n_pb=n_pb,
                sqrt_info_b=inverse_then_llt(P) if regular else np.zeros((15, 15), dtype))


def record_quantities(rec):
    """the compared quantities of a 293-double record: name -> array (sqrt_info as [15][15], one row per quantity)"""
    out = dict(dp=rec[DP:DP + 3], dq=rec[DQ:DQ + 4], dv=rec[DV:DV + 3], sum_dt=rec[SUMDT:SUMDT + 1])
    for name, off, _, _ in JAC_BLOCKS:
        out[name] = rec[off:off + 9]
    out["sqrt_info"] = rec[SQRTINFO:].reshape(15, 15)
    return out


def record_ratios(rec, ref):
    """name -> |rec - ref's record| / ref's bracket (the largest over the quantity; sqrt_info: over its rows).  0 / 0 counts as 0."""
    q, e, br = record_quantities(rec), record_quantities(ref["record"]), ref["bracket"]
    out = {}
    for name in q:
        d = _f(np.abs(q[name].astype(np.longdouble) - e[name].astype(np.longdouble)))
        b = np.asarray(br[name], np.float64)
        if name == "sqrt_info":
            d = d.max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0, 0.0, d / b)
        out[name] = float(np.max(r))
    return out


# ------------------------------------------------------------------------------------------------------------ triangulation
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def jacobi_right_vectors(D):
    """One-sided (Hestenes) Jacobi on the columns of D [n][4][4], run to convergence in D's dtype (a pair is rotated while its cosine
    exceeds the dtype's eps).  Returns (sigma [n][4] descending, V [n][4][4] with the right singular vectors as columns, same order)."""
    dt = D.dtype
    n = D.shape[0]
    D = D.copy()
    V = np.broadcast_to(np.eye(4, dtype=dt), (n, 4, 4)).copy()
    thr = dt.type(np.finfo(dt).eps) ** 2
    for sweep in range(80):
        rot = False
        for p, q in _PAIRS:
            a, b = D[:, :, p], D[:, :, q]
            al, be, ga = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
            m = (ga != 0) & (ga * ga > thr * (al * be))
            if not m.any():
                continue
            rot = True
            g = np.where(m, ga, dt.type(1))
            zeta = (be - al) / (2 * g)
            t = np.where(zeta >= 0, dt.type(1), dt.type(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            c = 1 / np.sqrt(1 + t * t)
            sn = c * t
            c, sn = np.where(m, c, dt.type(1))[:, None], np.where(m, sn, dt.type(0))[:, None]
            D[:, :, p], D[:, :, q] = c * a - sn * b, sn * a + c * b
            va, vb = V[:, :, p], V[:, :, q]
            V[:, :, p], V[:, :, q] = c * va - sn * vb, sn * va + c * vb
        if not rot:
            break
    sig = np.sqrt((D * D).sum(1))
    o = np.argsort(-_f(sig), axis=1, kind="stable")
    return np.take_along_axis(sig, o, 1), np.take_along_axis(V, o[:, None, :], 2)


def triangulate(Ps, Rs, tic, ric, pbg, start, pt0, pt1, init_depth=5.0, dtype=np.float64, order="reference"):
    """Two-view DLT for n features: frames start[i], start[i] + 1.  Returns dict(depth [n], world [n][3], raw_depth [n] (before the
    depth > 0 branch), positive [n], in_range [n], sigma [n][4], bracket_depth [n], bracket_world [n][3], gap [n]).

    bracket_depth, first order: depth = row . (v[:3] / v[3]) + m0z with v the right singular vector of the smallest singular value of
    the design matrix D and row = the third row of R0^T.  g = d depth / d v = (row / v3, -(row . X) / v3).  A perturbation dD of D moves v
    by sum_k v_k (...) / (sigma_k^2 - sigma_4^2) with a numerator of at most |dD| (sigma_k + sigma_4), and |dD| is sigma_1 roundings:
        bracket_depth = sigma_1 sum_{k<4} |g . v_k| / (sigma_k - sigma_4)  +  (|row| . |X| + |m0z|)
    the second term being the sum depth itself is.  bracket_world = bracket_depth (|Rs| |ric| |(u0, v0, 1)|) + |Rs| (|ric| |depth (u0,
    v0, 1)| + |tic| + |pbg|) + |Ps|, without the first term where the depth is INIT_DEPTH.
    gap = (sigma_3 - sigma_4) / sigma_1: where it is not far above the rounding level the first-order bracket does not apply."""
    Ps, Rs = _c(Ps, dtype).reshape(-1, 3), _c(Rs, dtype).reshape(-1, 3, 3)
    tic, ric, pbg = _c(tic, dtype), _c(ric, dtype).reshape(3, 3), _c(pbg, dtype)
    pt0, pt1 = _c(pt0, dtype).reshape(-1, 2), _c(pt1, dtype).reshape(-1, 2)
    start = np.asarray(start, np.int64).ravel()
    nfr, n = Ps.shape[0], start.size
    # camera poses of all frames (:288-298): t = Ps + Rs tic, R = Rs ric; pose = [R^T | -R^T t]
    t = Ps + np.stack([_mm(Rs[f], tic[:, None])[:, 0] for f in range(nfr)]) if nfr else Ps
    Rt = np.stack([_mm(Rs[f], ric).T for f in range(nfr)]) if nfr else Rs
    mt = np.stack([-_mm(Rt[f], t[f][:, None])[:, 0] for f in range(nfr)]) if nfr else Ps
    pose = np.concatenate([Rt, mt[:, :, None]], axis=2) if nfr else np.zeros((0, 3, 4), dtype)
    in_range = (start >= 0) & (start + 1 < nfr)
    f0 = np.where(in_range, start, 0)
    f1 = np.where(in_range, start + 1, 0)
    out = dict(depth=np.full(n, -1.0, dtype), world=np.zeros((n, 3), dtype), raw_depth=np.full(n, np.nan, dtype), in_range=in_range,
               positive=np.zeros(n, bool), sigma=np.zeros((n, 4), dtype), bracket_depth=np.full(n, np.inf), bracket_world=np.full((n, 3), np.inf),
               gap=np.zeros(n))
    if nfr < 2 or not in_range.any():
        return out
    P0, P1 = pose[f0], pose[f1]
    D = np.stack([pt0[:, 0:1] * P0[:, 2] - P0[:, 0], pt0[:, 1:2] * P0[:, 2] - P0[:, 1],
                  pt1[:, 0:1] * P1[:, 2] - P1[:, 0], pt1[:, 1:2] * P1[:, 2] - P1[:, 1]], axis=1)
    sig, V = jacobi_right_vectors(D)
    v = V[:, :, 3]
    if order == "alt":
        if dtype != np.float64:
            raise ValueError("order='alt' is LAPACK's SVD: float64 only")
        v = np.linalg.svd(D)[2][:, 3, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v[:, :3] / v[:, 3:4]
        row, m0z = P0[:, 2, :3], P0[:, 2, 3]
        raw = (row * X).sum(1) + m0z
        pos = _f(raw) > 0
        depth = np.where(pos, raw, dtype(init_depth))
        # first-order bracket, float64 magnitudes
        g = np.concatenate([_f(row) / _f(v[:, 3:4]), -(_f(row) * _f(X)).sum(1, keepdims=True) / _f(v[:, 3:4])], axis=1)
        s, Vf = _f(sig), _f(V)
        gv = np.abs(np.einsum("nr,nrk->nk", g, Vf))[:, :3]
        bd = s[:, 0] * (gv / (s[:, :3] - s[:, 3:4])).sum(1) + (np.abs(_f(row)) * np.abs(_f(X))).sum(1) + np.abs(_f(m0z))
        bd = np.where(np.isfinite(bd), bd, np.inf)
    uv1 = np.concatenate([pt0, np.ones((n, 1), dtype)], axis=1)
    pc = uv1 * depth[:, None]
    R0, Pf = Rs[f0], Ps[f0]
    pb = np.einsum("ij,nj->ni", ric, pc) + tic - pbg
    W = np.einsum("nij,nj->ni", R0, pb) + Pf
    aR, aric = np.abs(_f(R0)), np.abs(_f(ric))
    dirn = np.einsum("nij,nj->ni", aR, np.abs(_f(uv1)) @ aric.T)
    bw = np.einsum("nij,nj->ni", aR, np.abs(_f(pc)) @ aric.T + np.abs(_f(tic)) + np.abs(_f(pbg))) + np.abs(_f(Pf))
    with np.errstate(invalid="ignore"):
        bw = bw + np.where(pos, bd, 0.0)[:, None] * dirn
    ir = in_range
    out["depth"][ir], out["world"][ir], out["raw_depth"][ir], out["positive"][ir] = depth[ir], W[ir], raw[ir], pos[ir]
    out["sigma"][ir], out["bracket_depth"][ir], out["bracket_world"][ir] = sig[ir], bd[ir], bw[ir]
    out["gap"][ir] = ((s[:, 2] - s[:, 3]) / s[:, 0])[ir]
    return out


# ------------------------------------------------------------------------------------------------------------ inverse depth
class _E:
    """A value in the working dtype with its running bracket e (float64, same shape): the magnitudes of all terms that entered the
    value, each counted once per rounding.  A correct float64 evaluation lies within a small multiple of 2^-52 e of the exact value."""
    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros(np.shape(v)) if e is None else e

    @property
    def a(self):
        return np.abs(_f(self.v))

    @property
    def T(self):
        return _E(self.v.T, self.e.T)

    def __neg__(self):
        return _E(-self.v, self.e)

    def __add__(self, o):
        return _E(self.v + o.v, self.e + o.e + self.a + o.a)

    def __sub__(self, o):
        return _E(self.v - o.v, self.e + o.e + self.a + o.a)

    def __matmul__(self, o):
        return _E(_mm(self.v, o.v), self.a @ o.e + self.e @ o.a + self.a @ o.a)

    def times(self, s):
        """by a scalar _E"""
        v = self.v * s.v
        return _E(v, self.e * s.a + self.a * s.e + np.abs(_f(v)))

    def over(self, s):
        """divided by a scalar _E: the 1 / z factors of the projection enter here"""
        v = self.v / s.v
        return _E(v, self.e / s.a + self.a * s.e / (s.a * s.a) + np.abs(_f(v)))

    def __getitem__(self, k):
        return _E(self.v[k], self.e[k])


def _rotE(q):
    """toRotationMatrix with the bracket of its entries: each is a sum of three products of at most 2 |q_a| |q_b| (or 1)"""
    a = np.abs(_f(q))
    x, y, z, w = a
    e = np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 + 2 * (x * x + z * z), 2 * (y * z + x * w)],
                  [2 * (x * z + y * w), 2 * (y * z + x * w), 1 + 2 * (x * x + y * y)]])
    return _E(q2R(q), e)


def _skewE(v):
    z0 = np.zeros(())
    e = v.e
    return _E(skew(v.v[:, 0]), np.array([[z0, e[2, 0], e[1, 0]], [e[2, 0], z0, e[0, 0]], [e[1, 0], e[0, 0], z0]], np.float64))


def _col(v):
    return _E(v.reshape(3, 1))


def idepth_residual(kind, Pi, Pj, ex, e2, lam, pts_i, pts_j, si, pbg):
    """the residual alone, in the dtype of its arguments, with the reference's operations (q * v, q.inverse() * v): (r [2], pcj [3])"""
    lever = pbg if kind != 2 else np.zeros(3, pbg.dtype)
    pci = pts_i / lam
    pimu_i = qrot(ex[3:], pci) + ex[:3] - lever
    if kind == 2:
        pimu_j = pimu_i
    else:
        pimu_j = qrot(qinv(Pj[3:]), qrot(Pi[3:], pimu_i) + (Pi[:3] - Pj[:3]))
    cam = ex if kind == 0 else e2
    pcj = qrot(qinv(cam[3:]), pimu_j + lever - cam[:3])
    dep = pcj[2]
    return np.array([si * (pcj[0] / dep - pts_j[0]), si * (pcj[1] / dep - pts_j[1])], pcj.dtype), pcj


def pose_plus(x, d):
    """PoseLocalParameterization::Plus: p + dp, q * (d_theta / 2, 1) normalised"""
    one = x.dtype.type(1)
    q = qmul(x[3:], np.array([d[3] / 2, d[4] / 2, d[5] / 2, one], x.dtype))
    return np.concatenate([x[:3] + d[:3], q / np.sqrt((q * q).sum())])


def eval_idepth(kind, Pi, Pj, ex, ex2, lam, pts_i, pts_j, sqrt_info, pbg, dtype=np.float64, fd=False):
    """One inverse-depth projection factor: kind 0 TwoFrameOneCam (:179-256), 1 TwoFrameTwoCam (:77-166), 2 OneFrameTwoCam (:269-329,
    no lever arm, Pi = Pj = identity).  Returns dict(r [2], J = (J_pose_i, J_pose_j, J_ex, J_ex2 [2][6] each, J_lambda [2]), the same
    shapes under br_r / br_J, z = the camera-frame depth) and, with fd=True (longdouble), J_fd: every block by central differences on
    the manifold (PoseLocalParameterization::Plus) of idepth_residual, and h_rel, the relative step used.

    Brackets: the values are computed from the reference's expressions; next to every intermediate runs the sum of the magnitudes of
    the terms it was formed from (class _E): a sum adds its operands' magnitudes, a product |A| |B|, and the two divisions by the
    camera-frame depth z carry 1 / z and |x| / z^2.  q * v is bracketed as the matrix-vector product with toRotationMatrix(q)."""
    c = lambda v: _c(v, dtype)
    Pi, Pj, ex, ex2, pts_i, pts_j, pbg = c(Pi), c(Pj), c(ex), c(ex2), c(pts_i), c(pts_j), c(pbg)
    lam, si = dtype(float(lam)), dtype(float(sqrt_info))
    if kind == 2:
        Pi = Pj = np.array([0, 0, 0, 0, 0, 0, 1], dtype)
    cam = ex if kind == 0 else ex2
    lever = pbg if kind != 2 else np.zeros(3, dtype)
    r, pcj_v = idepth_residual(kind, Pi, Pj, ex, cam, lam, pts_i, pts_j, si, pbg)
    # the same chain with brackets
    S = lambda v: _E(np.asarray(v, dtype).reshape(()))
    ric, ric2, Ri, Rj = _rotE(ex[3:]), _rotE(cam[3:]), _rotE(Pi[3:]), _rotE(Pj[3:])
    pci = _col(pts_i).over(S(lam))
    pimu_i = (ric @ pci + _col(ex[:3])) - _col(lever) if kind != 2 else ric @ pci + _col(ex[:3])
    pimu_j = pimu_i if kind == 2 else Rj.T @ (Ri @ pimu_i + (_col(Pi[:3]) - _col(Pj[:3])))
    pcj = ric2.T @ ((pimu_j + _col(lever)) - _col(cam[:3])) if kind != 2 else ric2.T @ (pimu_j - _col(cam[:3]))
    pcj = _E(pcj_v.reshape(3, 1), pcj.e)                  # the value the reference's quaternion products give, the bracket of the chain
    dep = pcj[2, 0]
    sE = S(si)
    res = [(pcj[k, 0].over(dep) - S(pts_j[k])).times(sE) for k in range(2)]
    br_r = np.array([float(res[0].e), float(res[1].e)])
    inv_d = S(dtype(1)).over(dep)
    red = _E(np.zeros((2, 3), dtype), np.zeros((2, 3)))
    for k in range(2):
        a = inv_d.times(sE)
        b = (-pcj[k, 0]).over(dep.times(dep)).times(sE)
        red.v[k, k], red.e[k, k] = a.v, a.e
        red.v[k, 2], red.e[k, 2] = b.v, b.e
    Am = ric2.T @ Rj.T
    Bm = Am @ Ri
    Cm = Bm @ ric
    Z = _E(np.zeros((2, 6), dtype), np.zeros((2, 6)))
    cat = lambda L, Rr: _E(np.concatenate([L.v, Rr.v], axis=1), np.concatenate([L.e, Rr.e], axis=1))
    Ji = Jj = Jex2 = Z
    if kind != 2:
        Ji = cat(red @ Am, -(red @ (Bm @ _skewE(pimu_i))))
        Jj = cat(-(red @ Am), red @ (ric2.T @ _skewE(pimu_j)))
    if kind == 0:
        T1 = Bm - ric2.T
        tmp = Cm @ pci
        u = Rj.T @ (Ri @ (_col(ex[:3]) - _col(pbg)) + (_col(Pi[:3]) - _col(Pj[:3]))) + _col(pbg) - _col(ex[:3])
        M = (-(Cm @ _skewE(pci)) + _skewE(tmp)) + _skewE(ric2.T @ u)
        Jex = cat(red @ T1, red @ M)
    else:
        Jex = cat(red @ Bm, -(red @ (Cm @ _skewE(pci))))
        Jex2 = cat(-(red @ ric2.T), red @ _skewE(pcj))
    Jl = (red @ (Cm @ _col(pts_i))).times(S(dtype(-1)).over(S(lam).times(S(lam))))
    Jl = _E(Jl.v[:, 0], Jl.e[:, 0])
    blocks = (Ji, Jj, Jex, Jex2, Jl)
    out = dict(r=r, br_r=br_r, J=tuple(b.v for b in blocks), br_J=tuple(b.e for b in blocks), z=float(_f(pcj_v[2])))
    if fd:
        # central differences: the residual varies on the scale of z / (lever of the perturbed block), so the step is relative to the
        # smallest length in play; truncation h_rel^2, rounding eps / h_rel
        z = min(abs(out["z"]), abs(float(_f(pts_i[2] / lam))), 1.0)
        h_rel = 1e-6
        h = dtype(h_rel * z)
        blocks_x = [Pi, Pj, ex, ex2]
        f = lambda xs, L: idepth_residual(kind, xs[0], xs[1], xs[2], xs[2] if kind == 0 else xs[3], L, pts_i, pts_j, si, pbg)[0]
        Jfd = []
        for b in range(4):
            Jb = np.zeros((2, 6), dtype)
            has = (kind != 2) if b < 2 else (kind != 0 if b == 3 else True)
            for k in range(6 if has else 0):
                d = np.zeros(6, dtype)
                d[k] = h
                xp, xm = list(blocks_x), list(blocks_x)
                xp[b], xm[b] = pose_plus(blocks_x[b], d), pose_plus(blocks_x[b], -d)
                Jb[:, k] = (f(xp, lam) - f(xm, lam)) / (2 * h)
            Jfd.append(Jb)
        hl = dtype(h_rel) * lam * dtype(min(1.0, abs(out["z"]) * abs(float(_f(lam)))))
        Jfd.append((f(blocks_x, lam + hl) - f(blocks_x, lam - hl)) / (2 * hl))
        out["J_fd"], out["h_rel"] = tuple(Jfd), h_rel
    return out
