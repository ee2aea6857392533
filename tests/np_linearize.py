"""A longdouble referee of the factor LINEARISATION (residual rows and analytic Jacobian blocks, in the row and column order of
swf_batch_export_jacobian) with one bracket per compared entry — TEST INFRASTRUCTURE.  Written from the reference's lines:
  IMUFactor::Evaluate, IntegrationBase::evaluate          R/factor/imu_factor.cpp:5-101, R/factor/integration_base.cpp:144-174
  Utility::deltaQ / Qleft / Qright                          R/utility/utility.h:11-49
  projection_factor::Evaluate                               R/factor/projection_factor.cpp:13-65
  the loss corrector (CauchyLoss: rho'' < 0 => alpha = 0)   R/factor/marginalization_factor.cpp:23-45
  ProjectionTwoFrameOneCam / TwoFrameTwoCam / OneFrameTwoCam  np_producers.eval_idepth (R/factor/projection_factor.cpp:77-329), reused
  RTKCarrierPhase / RTKPseudorange / SppPseudorange / SppCarrierPhase / FixedInteger / SppDoppler, varerr2
                                                            R/factor/gnss_factor.cpp:9-212, distance / velecitydistance
                                                            R/gnss/src/common_function.cpp:126-134, 411-421
  InitialBlackFactor                                        R/factor/initial_factor.cpp:81-87
  MarginalizationFactor::Evaluate                           R/factor/marginalization_factor.cpp:410-446
Nothing comes from oracle/, the kernels or tests/np_factors.py (rotation-matrix algebra and finite differences: the third opinion).
dtype = np.float64 | np.longdouble; no LAPACK.  order="alt" is a second legitimate float64 operation order (every sum of products
taken from the other end): it exists to measure the tolerance constants.

BRACKETS.  Every value is carried as a pair (v, e) (class V): v in the working dtype, e a float64 magnitude, the running first-order
bound of the referee's own arithmetic.  Inputs are exact (e = 0) and
    x +- y      e = e_x + e_y + |x +- y|
    x y         e = |x| e_y + |y| e_x + |x y|            (matrix products: the same with |A| |B|, magnitudes summed)
    x / y       e = e_x / |y| + |x| e_y / y^2 + |x / y|
    sqrt x      e = e_x / (2 sqrt x) + |sqrt x|
    log x       e = e_x / |x| + |log x|
so that a correct float64 evaluation, in any operation order, lies within a small multiple of 2^-52 e of the exact value.  The whitened
IMU quantities come out as |SI| (B_U + |U|) per entry; a GNSS residual gets a bracket of the size of weight x range (its own
conditioning, not slack).  An entry whose bracket is exactly zero is an exact value: a structural zero (rotation columns of the GNSS
factors, the blocks of SI U that are empty because SI is upper triangular, columns of blocks a factor does not touch), a copied input
(the prior's J), or +-1.  A quaternion q enters rotations as toRotationMatrix(q) / q * v of whatever q is (not normalised), and
q.inverse() is conj / |q|^2: the two are the same polynomial in q, so the longdouble value does not depend on which is written.

Composite IMU-GNSS rows are a square root, unique only up to an orthogonal factor: they stay with np_dense.composite_dense.  Their rows
are the LAST rows of the export; the referee marks them family "comp" with value NaN and every comparison skips them by position.

varerr2 takes sinf(el): the float32 sine of the float32 elevation (correctly rounded on both sides).  In longdouble: the
sine of float32(el) in longdouble, rounded ONCE to float32.  Caveat: rounding a 64-bit-significand sine to 24 bits is not the correctly
rounded float32 sine when the longdouble sine lies within its own error of a float32 tie (double rounding); sine_is_safe() states that
it is not within 2^-40 relative of a tie, and test_case_reaches_its_branch asserts it for every elevation of every case."""
import numpy as np

import np_producers as npp
from np_producers import EPS

CLIGHT, OMGE = 299792458.0, 7.2921151467E-5
FAMILIES = ("proj", "imu", "cp", "pr", "dop", "sp", "spr", "scp", "fix", "idp", "prior", "comp")
# what the constants are measured per: the issue's families
GROUP = dict(proj="proj", imu="imu", cp="gnss", pr="gnss", dop="gnss", sp="gnss", spr="gnss", scp="gnss", fix="gnss", idp="idp", prior="prior")
GROUPS = ("imu", "proj", "idp", "gnss", "prior")
_ALT = [False]


def _f(v):
    return np.asarray(v).astype(np.float64)


def _mm(A, B):
    return npp._mm(A, B, _ALT[0])


class V:
    """value (working dtype) and running bracket (float64), same shape"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros(np.shape(v)) if e is None else e

    @property
    def a(self):
        return np.abs(_f(self.v))

    @property
    def T(self):
        return V(self.v.T, self.e.T)

    def __neg__(self):
        return V(-self.v, self.e)

    def __add__(self, o):
        v = self.v + o.v
        return V(v, self.e + o.e + np.abs(_f(v)))

    def __sub__(self, o):
        v = self.v - o.v
        return V(v, self.e + o.e + np.abs(_f(v)))

    def __mul__(self, o):
        """elementwise (broadcasting)"""
        v = self.v * o.v
        return V(v, self.a * o.e + o.a * self.e + np.abs(_f(v)))

    def __truediv__(self, o):
        v = self.v / o.v
        return V(v, self.e / o.a + self.a * o.e / (o.a * o.a) + np.abs(_f(v)))

    def __matmul__(self, o):
        return V(_mm(self.v, o.v), self.a @ o.e + self.e @ o.a + self.a @ o.a)

    def __getitem__(self, k):
        return V(self.v[k], self.e[k])

    def sqrt(self):
        v = np.sqrt(self.v)
        return V(v, self.e / (2 * np.abs(_f(v))) + np.abs(_f(v)))

    def log(self):
        v = np.log(self.v)
        return V(v, self.e / self.a + np.abs(_f(v)))

    def sum(self):
        """all entries, one after the other (alt: from the other end)"""
        it = list(np.ndindex(*np.shape(self.v)))
        it = it[::-1] if _ALT[0] else it
        s = self[it[0]]
        for k in it[1:]:
            s = s + self[k]
        return s


def cat(rows):
    """block matrix of V from a list of lists of V"""
    return V(np.block([[b.v for b in r] for r in rows]), np.block([[b.e for b in r] for r in rows]))


def col(v, dtype):
    return V(np.asarray(v, np.float64).astype(dtype).reshape(-1, 1))


def sc(v, dtype):
    return V(np.asarray(float(v), np.float64).astype(dtype).reshape(()))


def eye3(dtype):
    return V(np.eye(3, dtype=dtype))


def rot(q):
    """toRotationMatrix of the quaternion q (V [4][1], x y z w), not normalised: 1 - 2 (yy + zz), 2 (xy - wz), ..."""
    x, y, z, w = (q[k, 0] for k in range(4))
    two, one = sc(2, q.v.dtype), sc(1, q.v.dtype)
    d = lambda a, b: one - two * (a * a + b * b)
    p = lambda a, b, c, dd: two * (a * b + c * dd)
    m = lambda a, b, c, dd: two * (a * b - c * dd)
    g = [[d(y, z), m(x, y, z, w), p(x, z, y, w)], [p(x, y, z, w), d(x, z), m(y, z, x, w)], [m(x, z, y, w), p(y, z, x, w), d(x, y)]]
    return V(np.array([[c.v for c in r] for r in g], q.v.dtype), np.array([[c.e for c in r] for r in g], np.float64))


def qinv(q):
    """Eigen's Quaternion::inverse: conj / |q|^2"""
    n2 = (q * q).sum()
    sgn = V(np.array([[-1], [-1], [-1], [1]], q.v.dtype))
    return (q * sgn) / n2


def skew(v):
    """Utility::skewSymmetric of V [3][1]"""
    z = np.zeros((), v.v.dtype)
    a, e = v.v[:, 0], v.e[:, 0]
    return V(np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], v.v.dtype),
             np.array([[0, e[2], e[1]], [e[2], 0, e[0]], [e[1], e[0], 0]], np.float64))


def qleft4(a):
    """the matrix L(a) with a * b = L(a) b, both quaternions as (x, y, z, w) columns"""
    x, y, z, w = a.v[:, 0]
    ex, ey, ez, ew = a.e[:, 0]
    return V(np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]], a.v.dtype),
             np.array([[ew, ez, ey, ex], [ez, ew, ex, ey], [ey, ex, ew, ez], [ex, ey, ez, ew]], np.float64))


def qmul(a, b):
    return qleft4(a) @ b


def qleft_br(q):
    """Utility::Qleft(q).bottomRightCorner<3, 3>() = w I + skew(vec)"""
    w = q[3, 0]
    return eye3(q.v.dtype) * w + skew(q[:3])


def qright_br(q):
    """Utility::Qright(q).bottomRightCorner<3, 3>() = w I - skew(vec)"""
    w = q[3, 0]
    return eye3(q.v.dtype) * w - skew(q[:3])


def zeros(r, c, dtype):
    return V(np.zeros((r, c), dtype))


# ---------------------------------------------------------------------------------------------------------------- the loss
def loss(r, J, a, dtype):
    """The corrector of R/factor/marginalization_factor.cpp:23-45 for CauchyLoss(a), rho = a^2 log(1 + s / a^2): rho' = 1 / (1 + s / a^2),
    rho'' < 0, hence residual_scaling = sqrt(rho'), alpha = 0: r and J are scaled by sr = sqrt(1 / (1 + s / a^2)).  a <= 0: the trivial
    loss.  r: V [n][1], J: V [n][m].  Returns (r, J, cost = 1/2 rho(s), sr as float)."""
    s = (r * r).sum()
    half = sc(0.5, dtype)
    if not a > 0:
        return r, J, half * s, 1.0
    b = sc(a, dtype) * sc(a, dtype)
    one = sc(1, dtype)
    arg = one + s / b
    sr = (one / arg).sqrt()
    return r * sr, J * sr, half * (b * arg.log()), float(_f(sr.v))


# ---------------------------------------------------------------------------------------------------------------- IMU
def imu_unwhitened(Pi, Bi, Pj, Bj, pre, pbg, gw, dtype):
    """(raw [15][1], U [15][30], SI [15][15]) as V: the residual of IntegrationBase::evaluate and the un-whitened Jacobian of
    IMUFactor::Evaluate, columns [pose_i 6 | speed-bias_i 9 | pose_j 6 | speed-bias_j 9], rows O_P 0, O_R 3, O_V 6, O_BA 9, O_BG 12.
    The reference's quirk is restated: d r_theta / d bg_i uses the UNCORRECTED delta_q (imu_factor.cpp:67), the residual and the two
    pose blocks the corrected one (:52, :81, integration_base.cpp:164)."""
    c = lambda v: col(v, dtype)
    m3 = lambda o: V(np.asarray(pre[o:o + 9], np.float64).astype(dtype).reshape(3, 3))
    pi, qi, pj, qj = c(Pi[:3]), c(Pi[3:]), c(Pj[:3]), c(Pj[3:])
    vi, bai, bgi, vj, baj, bgj = c(Bi[:3]), c(Bi[3:6]), c(Bi[6:9]), c(Bj[:3]), c(Bj[3:6]), c(Bj[6:9])
    dp, dq, dv, lba, lbg = c(pre[0:3]), c(pre[3:7]), c(pre[7:10]), c(pre[10:13]), c(pre[13:16])
    dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg = m3(16), m3(25), m3(34), m3(43), m3(52)
    T, gyri, gyrj = sc(pre[61], dtype), c(pre[62:65]), c(pre[65:68])
    SI = V(np.asarray(pre[68:293], np.float64).astype(dtype).reshape(15, 15))
    pbg, g = c(pbg), c(gw)
    half, two, one = sc(0.5, dtype), sc(2, dtype), sc(1, dtype)
    I3 = eye3(dtype)
    dba, dbg = bai - lba, bgi - lbg
    th = dq_dbg @ dbg
    dtheta = cat([[th / two], [V(np.ones((1, 1), dtype))]])                   # Utility::deltaQ: (theta / 2, 1), not normalised
    cq = qmul(dq, dtheta)
    cv = dv + dv_dba @ dba + dv_dbg @ dbg
    cp = dp + dp_dba @ dba + dp_dbg @ dbg
    qi_inv, qj_inv = qinv(qi), qinv(qj)
    Ri_inv, Rj = rot(qi_inv), rot(qj)
    wi, wj = skew(gyri - bgi) @ pbg, skew(gyrj - bgj) @ pbg
    in_p = Ri_inv @ (half * g * T * T + ((pj - pi) - Rj @ pbg) - vi * T)
    in_v = Ri_inv @ (g * T + (vj - Rj @ wj) - vi)
    qij = qmul(qi_inv, qj)
    raw = cat([[in_p - cp + pbg + wi * T], [(two * qmul(qinv(cq), qij))[:3]], [in_v - cv + wi], [baj - bai], [bgj - bgi]])
    Z = lambda r_, c_: zeros(r_, c_, dtype)
    RiRj = Ri_inv @ Rj
    # pose_i (imu_factor.cpp:50-54)
    qji = qmul(qj_inv, qi)
    a_, b_ = qji, cq                                                          # (Qleft(a) Qright(b)).bottomRightCorner<3, 3>
    lr = a_[:3] @ (-(b_[:3].T)) + qleft_br(a_) @ qright_br(b_)
    Jpi = cat([[-Ri_inv, skew(in_p)], [Z(3, 3), -lr], [Z(3, 3), skew(in_v)], [Z(6, 3), Z(6, 3)]])
    # speed-bias_i (:64-72)
    Jbi = cat([[-(Ri_inv * T), -dp_dba, -dp_dbg + skew(pbg) * T],
               [Z(3, 3), Z(3, 3), -(qleft_br(qmul(qji, dq)) @ dq_dbg)],
               [-Ri_inv, -dv_dba, -dv_dbg + skew(pbg)],
               [Z(3, 3), -I3, Z(3, 3)], [Z(3, 3), Z(3, 3), -I3]])
    # pose_j (:79-83)
    Jpj = cat([[Ri_inv, RiRj @ skew(pbg)], [Z(3, 3), qleft_br(qmul(qmul(qinv(cq), qi_inv), qj))], [Z(3, 3), RiRj @ skew(wj)], [Z(6, 3), Z(6, 3)]])
    # speed-bias_j (:90-93)
    Jbj = cat([[Z(3, 9)], [Z(3, 9)], [Ri_inv, Z(3, 3), RiRj @ (-skew(pbg))], [Z(3, 3), I3, Z(3, 3)], [Z(3, 3), Z(3, 3), I3]])
    return raw, cat([[Jpi, Jbi, Jpj, Jbj]]), SI


def eval_imu(Pi, Bi, Pj, Bj, pre, pbg, gw, dtype):
    """r = SI raw, J = SI U; blocks (6, 9, 6, 9); scale = |SI| |raw|, the rows' un-cancelled size"""
    raw, U, SI = imu_unwhitened(Pi, Bi, Pj, Bj, pre, pbg, gw, dtype)
    r, J = SI @ raw, SI @ U
    return r, [J[:, 0:6], J[:, 6:15], J[:, 15:21], J[:, 21:30]], (SI.a @ raw.a)[:, 0], dict(raw=raw, U=U)


# ---------------------------------------------------------------------------------------------------------------- projection
def eval_proj(P, E, X, uv, si, pbg, dtype):
    """projection_factor::Evaluate before the loss: r [2][1], blocks (pose 2x6, extrinsic 2x6, landmark 2x3)"""
    c = lambda v: col(v, dtype)
    pj, qj, tic, qic, x, pbg = c(P[:3]), c(P[3:]), c(E[:3]), c(E[3:]), c(X), c(pbg)
    siV, one = sc(si, dtype), sc(1, dtype)
    pts_imu = rot(qinv(qj)) @ (x - pj)
    pc = rot(qinv(qic)) @ (pts_imu + pbg - tic)
    dep = pc[2, 0]
    r = (pc[:2] / dep - c(uv)) * siV
    Rj, ric = rot(qj), rot(qic)
    z = V(np.zeros((), dtype))
    inv, d2 = one / dep, dep * dep
    g = [[inv, z, -pc[0, 0] / d2], [z, inv, -pc[1, 0] / d2]]
    red = V(np.array([[e_.v for e_ in r_] for r_ in g], dtype), np.array([[e_.e for e_ in r_] for r_ in g], np.float64)) * siV
    ricT = ric.T
    Jp = red @ cat([[ricT @ (-(Rj.T)), ricT @ skew(pts_imu)]])
    Je = red @ cat([[-ricT, skew(pc)]])
    Jl = (red @ ricT) @ Rj.T
    scale = float(_f(si)) * (np.abs(_f(pc.v[:2, 0] / pc.v[2, 0])) + np.abs(np.asarray(uv, np.float64)))
    return r, [Jp, Je, Jl], scale


# ---------------------------------------------------------------------------------------------------------------- GNSS
def sine_f32(el):
    """sinf(el) as DESIGN.md §4 states it: the correctly rounded float32 sine of float32(el).  (value as float64, relative distance of the
    longdouble sine from the nearest float32 rounding tie)"""
    x = np.longdouble(np.float64(np.float32(el)))
    s = np.sin(x)
    f = np.float32(s)
    nb = np.nextafter(f, np.float32(np.inf) if np.longdouble(f) < s else np.float32(-np.inf))
    tie = (np.longdouble(f) + np.longdouble(nb)) / 2
    return float(f), float(abs(s - tie) / abs(s))


def sine_is_safe(el):
    return sine_f32(el)[1] > 2.0 ** -40


def gnss_weight(el, dt, mv, dtype):
    """1 / sqrt(varerr2(el, dt, mea_var)) (gnss_factor.cpp:98-103, :117, :149)"""
    s = sc(sine_f32(el)[0], dtype)
    b = sc(CLIGHT, dtype) * sc(5e-12, dtype) * sc(dt, dtype)
    return sc(1, dtype) / (sc(mv, dtype) / s / s + b * b).sqrt()


def gnss_range(p, base, sat, dtype):
    """distance() of common_function.cpp:126-134 at xyz + base: (range with the Sagnac term, unit vector e [3][1], geometric r, xg)"""
    xg = col(p, dtype) + col(base, dtype)
    rs = col(sat, dtype)
    e = xg - rs
    r = (e * e).sum().sqrt()
    sag = sc(OMGE, dtype) * (rs[0, 0] * xg[1, 0] - rs[1, 0] * xg[0, 0]) / sc(CLIGHT, dtype)
    return r + sag, e / r, r, xg


def eval_range_factor(kind, P, scalars, d, base, dtype):
    """cp / pr / spr / scp: r [1][1], blocks (pose 1x6, then one 1x1 per scalar in the factor's own order), scale = weight x range.
    The Sagnac term is in the range and NOT in the Jacobians; the rotation columns are exact zeros."""
    rng, e, _, _ = gnss_range(P[:3], base, d[:3], dtype)
    s = [sc(v, dtype) for v in scalars]
    one = sc(1, dtype)
    if kind == "cp":          # sat[3] L1_lam lam el dt_br mea_var use_istd; blocks pose, ambiguity, clock
        w = gnss_weight(d[5], d[6], d[7], dtype) if d[8] != 0 else one
        res = w * (rng - s[0] * sc(d[4], dtype) - sc(d[3], dtype) + s[1])
        Js = [-(w * sc(d[4], dtype)), w]
    elif kind == "pr":        # sat[3] P1 el dt_br mea_var; blocks pose, clock
        w = gnss_weight(d[4], d[5], d[6], dtype)
        res = w * (rng - sc(d[3], dtype) + s[0])
        Js = [w]
    elif kind == "spr":       # sat[3] P1 istd; blocks pose, clock
        w = sc(d[4], dtype)
        res = w * (rng + s[0] - sc(d[3], dtype))
        Js = [w * one]
    else:                     # scp: sat[3] L1_lam istd lam; blocks pose, clock, ambiguity
        w = sc(d[4], dtype)
        res = w * (rng + s[0] - s[1] * sc(d[5], dtype) - sc(d[3], dtype))
        Js = [w * one, -(w * sc(d[5], dtype))]
    Jp = cat([[(e * w).T, zeros(1, 3, dtype)]])
    m11 = lambda x: V(x.v.reshape(1, 1), x.e.reshape(1, 1))
    return m11(res), [Jp] + [m11(j) for j in Js], np.array([float(_f(w.v)) * float(_f(rng.v))])


def eval_dop(B, drift, P, d, base, dtype):
    """SppDopplerFactor (gnss_factor.cpp:174-212): blocks (speed-bias 1x9, drift 1x1, pose 1x6); dat = sat[3] satvel[3] D1_lam istd"""
    _, e, r, xg = gnss_range(P[:3], base, d[:3], dtype)
    rs, vs, vr = col(d[:3], dtype), col(d[3:6], dtype), col(B[:3], dtype)
    ev = vr - vs
    w = sc(d[7], dtype)
    sag = sc(OMGE, dtype) / sc(CLIGHT, dtype) * (vs[1, 0] * xg[0, 0] + rs[1, 0] * vr[0, 0] - vs[0, 0] * xg[1, 0] - rs[0, 0] * vr[1, 0])
    rate = (ev * e).sum() + sag
    res = w * (rate + sc(drift, dtype) + sc(d[6], dtype))
    Jb = cat([[(e * w).T, zeros(1, 6, dtype)]])
    proj = eye3(dtype) - e @ e.T
    Jp = cat([[((ev.T * w) @ proj) / r, zeros(1, 3, dtype)]])
    m11 = lambda x: V(x.v.reshape(1, 1), x.e.reshape(1, 1))
    scale = float(_f(w.v)) * (float((ev.a * e.a).sum()) + abs(float(drift)) + abs(float(d[6])))
    return m11(res), [Jb, m11(w * sc(1, dtype)), Jp], np.array([scale])


# ---------------------------------------------------------------------------------------------------------------- prior
def prior_dx(x, x0, dtype):
    """one kept block's increment (marginalization_factor.cpp:418-428): x - x0, or [p - p0, +-2 vec(q0^-1 q)] with the sign of w.
    Returns (dx, its un-cancelled size: |x| + |x0|, and 2 |L(q0^-1)| |q| for the rotation part)."""
    a = lambda v: np.abs(np.asarray(v, np.float64)).reshape(-1, 1)
    if len(x) != 7:
        return col(x, dtype) - col(x0, dtype), a(x) + a(x0)
    q0i = qinv(col(x0[3:], dtype))
    dq = qmul(q0i, col(x[3:], dtype))
    v = sc(2, dtype) * dq[:3]
    size = np.concatenate([a(x[:3]) + a(x0[:3]), 2 * (qleft4(q0i).a @ a(x[3:]))[:3]])
    return cat([[col(x[:3], dtype) - col(x0[:3], dtype)], [v if _f(dq.v[3, 0]) >= 0 else -v]]), size


def eval_prior(xs, x0s, J, r0, dtype):
    """r = r0 + J dx; the Jacobian IS the input J (bracket zero: it must come back bit for bit).  scale = |r0| + |J| (un-cancelled
    size of dx): the differences x - x0 and the quaternion product cancel before J multiplies them."""
    parts = [prior_dx(x, x0, dtype) for x, x0 in zip(xs, x0s)]
    dx, size = cat([[p[0]] for p in parts]), np.concatenate([p[1] for p in parts])
    Jv = V(np.asarray(J, np.float64).astype(dtype))
    r = col(r0, dtype) + Jv @ dx
    blocks, o = [], 0
    for x in xs:
        l = 6 if len(x) == 7 else len(x)
        blocks.append(Jv[:, o:o + l])
        o += l
    return r, blocks, np.abs(np.asarray(r0, np.float64)) + (Jv.a @ size)[:, 0], dx


# ---------------------------------------------------------------------------------------------------------------- the window
def local_layout(w):
    """(column offset per global block or -1, n_loc): the local vector in elimination order.  (Restated here, like factors() below, so
    that the referee imports neither np_dense nor, through it, np_factors.)"""
    _, l = w.block_sizes()
    loc = -np.ones(w.n_blocks, np.int64)
    o = 0
    for b in w.a["order_block"]:
        loc[b] = o
        o += l[b]
    return loc, o


def factors(w):
    """every factor in the row order of swf_batch_export_jacobian: (family, nres, global block ids, record)"""
    a = w.a
    out = []
    for ix, uv in zip(a["proj_idx"].reshape(-1, 3), a["proj_uv"].reshape(-1, 2)):
        out.append(("proj", 2, [w.bid_pose(ix[0]), w.bid_pose(ix[1]), w.bid_lm(ix[2])], uv))
    for ix, pre in zip(a["imu_idx"].reshape(-1, 4), a["imu_pre"].reshape(-1, 293)):
        out.append(("imu", 15, [w.bid_pose(ix[0]), w.bid_sb(ix[1]), w.bid_pose(ix[2]), w.bid_sb(ix[3])], pre))
    for ix, d in zip(a["cp_idx"].reshape(-1, 3), a["cp_dat"].reshape(-1, 9)):
        out.append(("cp", 1, [w.bid_pose(ix[0]), w.bid_sc(ix[1]), w.bid_sc(ix[2])], d))
    for ix, d in zip(a["pr_idx"].reshape(-1, 2), a["pr_dat"].reshape(-1, 7)):
        out.append(("pr", 1, [w.bid_pose(ix[0]), w.bid_sc(ix[1])], d))
    for ix, d in zip(a["dop_idx"].reshape(-1, 3), a["dop_dat"].reshape(-1, 8)):
        out.append(("dop", 1, [w.bid_sb(ix[0]), w.bid_sc(ix[1]), w.bid_pose(ix[2])], d))
    for i, wv in zip(a["sp_idx"], a["sp_w"]):
        out.append(("sp", 1, [w.bid_sc(i)], wv))
    for ix, d in zip(a["spr_idx"].reshape(-1, 2), a["spr_dat"].reshape(-1, 5)):
        out.append(("spr", 1, [w.bid_pose(ix[0]), w.bid_sc(ix[1])], d))
    for ix, d in zip(a["scp_idx"].reshape(-1, 3), a["scp_dat"].reshape(-1, 6)):
        out.append(("scp", 1, [w.bid_pose(ix[0]), w.bid_sc(ix[1]), w.bid_sc(ix[2])], d))
    for ix, d in zip(a["fix_idx"].reshape(-1, 2), a["fix_dat"].reshape(-1, 2)):
        out.append(("fix", 1, [w.bid_sc(ix[0]), w.bid_sc(ix[1])], d))
    for kd, ix, pt in zip(a["idp_kind"], a["idp_idx"].reshape(-1, 5), a["idp_pts"].reshape(-1, 6)):
        kd = int(kd)
        blocks = ([w.bid_pose(ix[0]), w.bid_pose(ix[1])] if kd != 2 else []) + [w.bid_pose(ix[2])] + ([w.bid_pose(ix[3])] if kd != 0 else []) + [w.bid_sc(ix[4])]
        out.append(("idp", 2, blocks, (kd, pt)))
    g, _ = w.block_sizes()
    bo = jo = ro = xo = 0
    for nb, dim in zip(a["prior_nblk"], a["prior_dim"]):
        nb, dim = int(nb), int(dim)
        ids = [int(b) for b in a["prior_blk"][bo:bo + nb]]
        x0s = []
        for b in ids:
            x0s.append(a["prior_x0"][xo:xo + g[b]])
            xo += g[b]
        out.append(("prior", dim, ids, (a["prior_J"][jo:jo + dim * dim].reshape(dim, dim), a["prior_r0"][ro:ro + dim], x0s)))
        bo += nb; jo += dim * dim; ro += dim
    for N in a["comp_N"]:
        out.append(("comp", 30 + int(N), [], None))
    return out


def block_values(w):
    a = w.a
    return ([a["pose"].reshape(-1, 7)[i] for i in range(w.n_pose)] + [a["sb"].reshape(-1, 9)[i] for i in range(w.n_sb)]
            + [a["lm"].reshape(-1, 3)[i] for i in range(w.n_lm)] + [a["sc"][i:i + 1] for i in range(w.n_sc)])


def eval_factor(w, fam, ids, rec, dtype):
    """(r V [n][1], blocks list of V [n][l_b], scale [n], cost V scalar, sr) of one factor at the window's state, loss applied"""
    x = [block_values(w)[b] for b in ids] if ids else []
    a_loss = 0.0
    if fam == "proj":
        r, B, scale = eval_proj(x[0], x[1], x[2], rec, w.proj_sqrt_info, w.pbg, dtype)
        a_loss = w.proj_loss_a
    elif fam == "imu":
        r, B, scale, _ = eval_imu(x[0], x[1], x[2], x[3], rec, w.pbg, w.gw, dtype)
    elif fam in ("cp", "pr", "spr", "scp"):
        r, B, scale = eval_range_factor(fam, x[0], [v[0] for v in x[1:]], rec, w.base, dtype)
    elif fam == "dop":
        r, B, scale = eval_dop(x[0], x[1][0], x[2], rec, w.base, dtype)
    elif fam == "sp":
        wv, xv = sc(rec, dtype), sc(x[0][0], dtype)
        m11 = lambda q: V(q.v.reshape(1, 1), q.e.reshape(1, 1))
        r, B, scale = m11(xv * wv), [m11(sc(1, dtype) * wv)], np.array([abs(float(rec) * float(x[0][0]))])
    elif fam == "fix":
        wv = sc(rec[1], dtype)
        m11 = lambda q: V(q.v.reshape(1, 1), q.e.reshape(1, 1))
        r = m11(wv * ((sc(x[1][0], dtype) - sc(x[0][0], dtype)) - sc(rec[0], dtype)))
        B, scale = [m11(-wv), m11(wv)], np.array([abs(float(rec[1])) * (abs(float(x[0][0])) + abs(float(x[1][0])) + abs(float(rec[0])))])
    elif fam == "idp":
        kd, pt = rec
        one7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
        xx = list(x)
        Pi, Pj = (xx.pop(0), xx.pop(0)) if kd != 2 else (one7, one7)
        ex = xx.pop(0)
        ex2 = xx.pop(0) if kd != 0 else ex
        o = npp.eval_idepth(kd, Pi, Pj, ex, ex2, xx[0][0], pt[:3], pt[3:], w.proj_sqrt_info, w.pbg, dtype=dtype)
        r = V(o["r"].reshape(2, 1), o["br_r"].reshape(2, 1))
        allb = [V(o["J"][k].reshape(2, -1), o["br_J"][k].reshape(2, -1)) for k in range(5)]
        B = ([allb[0], allb[1]] if kd != 2 else []) + [allb[2]] + ([allb[3]] if kd != 0 else []) + [allb[4]]
        uvj = np.asarray(pt[3:5], np.float64)                                 # |pc / z| + |pts_j|, times sqrt_info
        scale = w.proj_sqrt_info * (np.abs(_f(o["r"]) / w.proj_sqrt_info + uvj) + np.abs(uvj))
        a_loss = w.proj_loss_a
    elif fam == "prior":
        J, r0, x0s = rec
        r, B, scale, _ = eval_prior(x, x0s, J, r0, dtype)
    else:
        raise KeyError(fam)
    n = [b.v.shape[1] for b in B]
    Jall = cat([B])
    r, Jall, cost, sr = loss(r, Jall, a_loss, dtype)
    o, out = 0, []
    for k in n:
        out.append(Jall[:, o:o + k])
        o += k
    return r, out, np.asarray(scale, np.float64) * sr, cost, sr


def linearize(w, dtype=np.longdouble, order="reference"):
    """The whole window.  dict(r [n_res], J [n_res][n_loc] in dtype; b_r, b_J float64 brackets; scale [n_res] the rows' un-cancelled
    size; fam [n_res] index into FAMILIES; fac [n_res] factor number; cost, b_cost (without composite factors: None when the window has
    any); n_comp_rows).  Composite rows: NaN, family "comp"."""
    _ALT[0] = order == "alt"
    try:
        loc, n_loc = local_layout(w)
        _, l = w.block_sizes()
        fl = factors(w)
        n_res = sum(f[1] for f in fl)
        r, J = np.zeros(n_res, dtype), np.zeros((n_res, n_loc), dtype)
        b_r, b_J, scale = np.zeros(n_res), np.zeros((n_res, n_loc)), np.zeros(n_res)
        fam, fac = np.zeros(n_res, np.int64), np.zeros(n_res, np.int64)
        costs, row, n_comp = [], 0, 0
        for k, (name, nres, ids, rec) in enumerate(fl):
            fam[row:row + nres], fac[row:row + nres] = FAMILIES.index(name), k
            if name == "comp":
                r[row:row + nres], J[row:row + nres] = np.nan, np.nan
                n_comp += nres
                row += nres
                continue
            rv, B, sc_, cost, _ = eval_factor(w, name, ids, rec, dtype)
            r[row:row + nres], b_r[row:row + nres], scale[row:row + nres] = rv.v[:, 0], rv.e[:, 0], sc_
            for b, blk in zip(ids, B):
                if loc[b] >= 0:
                    J[row:row + nres, loc[b]:loc[b] + l[b]] += blk.v          # (a block may enter a factor twice only in no factor here)
                    b_J[row:row + nres, loc[b]:loc[b] + l[b]] += blk.e
            costs.append(cost)
            row += nres
        cost = b_cost = None
        if not n_comp:
            cv = np.array([c.v for c in costs], dtype)
            cost = cv[::-1].sum() if _ALT[0] else cv.sum()
            b_cost = float(sum(float(c.e) for c in costs) + np.abs(_f(cv)).sum())
        return dict(r=r, J=J, b_r=b_r, b_J=b_J, scale=scale, fam=fam, fac=fac, cost=cost, b_cost=b_cost, n_comp_rows=n_comp)
    finally:
        _ALT[0] = False


# ---------------------------------------------------------------------------------------------------------------- comparison
def ratio(dev, ref, bracket):
    """|dev - ref| / (2^-52 bracket) entry by entry: 0 where the deviation is zero, inf where the bracket is zero and the value differs"""
    d = np.abs(np.asarray(dev).astype(np.longdouble) - np.asarray(ref).astype(np.longdouble)).astype(np.float64)
    br = np.asarray(bracket, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, np.where(br > 0, d / (EPS * br), np.inf))


def family_ratios(r, J, ref):
    """{group: (largest ratio of r, largest ratio of J)} over the rows of each family group, composite rows skipped by position"""
    qr, qJ = ratio(r, ref["r"], ref["b_r"]), ratio(J, ref["J"], ref["b_J"])
    out = {}
    for g in GROUPS:
        m = np.array([GROUP.get(FAMILIES[f]) == g for f in ref["fam"]], bool)
        if m.any():
            out[g] = (float(qr[m].max()), float(qJ[m].max()))
    return out


def weakest_entry(ref, group):
    """(row, column) of the smallest non-zero |J| with a non-zero bracket among the group's rows"""
    m = np.array([GROUP.get(FAMILIES[f]) == group for f in ref["fam"]], bool)
    v = np.abs(_f(ref["J"]))
    v = np.where(m[:, None] & (ref["b_J"] > 0) & (v > 0), v, np.inf)
    i, j = np.unravel_index(np.argmin(v), v.shape)
    return (int(i), int(j)) if np.isfinite(v[i, j]) else None
