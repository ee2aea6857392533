"""numpy referee of the batched track outlier rejection (swf_track_reject_batch), one entry point per stage, each taking the
previous stage's output as an argument:

    stage_pixels -> lift_stage (un_cur, un_prev, velocity, virtual pixels) -> sample_table -> minimal_solves -> score -> scan -> mask

(pair() chains them).  Written from R/feature/feature_tracker.cpp:265-294, :334-376, PinholeFullCamera::liftProjective
(C/src/camera_models/PinholeFullCamera.cc:535-607) and the specification at swf_track_reject_batch in include/swf_solver.h.  dtype is
np.float64 or np.longdouble; nothing here calls LAPACK on the working dtype (the condition number kappa is a float64 magnitude, not a
compared value).  order 0 takes a sample's points in the order drawn; order 1 reversed: the centroid and mean-distance sums run the
other way and the design matrix's rows enter the Householder reduction in the opposite order."""
import numpy as np

import np_pnp as npp

OK, TOO_FEW, NO_MODEL, BAD_INPUT = 0, 1, 2, 3
NMAX, HMAX = 1024, 1024
DRAWS = 64
LIFT_STEPS = 9
SWEEPS = 6
M_POINTS = 8
EPS = 2.0 ** -52
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- sampler
def sample_table(n, iterations, seed):
    """(samples [H][8] int32, rejected draws): H = iterations for n > 8, one row 0 .. 7 for n == 8.  A sample that is not complete
    after 64 draws keeps -1 in its open places (an invalid hypothesis)."""
    if n == 8:
        return np.arange(8, dtype=np.int32)[None], 0
    out = np.full((iterations, 8), -1, np.int32)
    rejected = 0
    for k in range(iterations):
        got = []
        for j in range(DRAWS):
            x = npp.splitmix64((seed + 64 * k + j) & M64)
            idx = ((x >> 32) * n) >> 32
            if idx in got:
                rejected += 1
                continue
            got.append(idx)
            if len(got) == 8:
                break
        out[k, :len(got)] = got
    return out, rejected


# ---------------------------------------------------------------------------------------------------------------- camera
class _E:
    """A value in the working dtype with its running bracket e (float64): the magnitudes of all terms that entered the value, each
    counted once per rounding (the inverse-depth item of DESIGN 3c).  A correct float64 evaluation lies within a small multiple of
    2^-52 e of the exact value."""
    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros(np.shape(v)) if e is None else e

    @property
    def a(self):
        return np.abs(np.asarray(self.v, np.float64))

    def __add__(self, o):
        return _E(self.v + o.v, self.e + o.e + self.a + o.a)

    def __sub__(self, o):
        return _E(self.v - o.v, self.e + o.e + self.a + o.a)

    def __mul__(self, o):
        v = self.v * o.v
        return _E(v, self.e * o.a + self.a * o.e + np.abs(np.asarray(v, np.float64)))

    def __truediv__(self, o):
        v = self.v / o.v
        return _E(v, self.e / o.a + self.a * o.e / (o.a * o.a) + np.abs(np.asarray(v, np.float64)))


def lift(cam, px, dtype=np.float64):
    """liftProjective for px [N][2] (already in float64): x0 = p.x / fx - cx / fx, then exactly nine steps in the order of :574-581.
    Nine is what the reference executes: `int min_error = 0.01` is 0 and the error it tests is a square root, never below 0, so the
    loop ends only by j > 8.  Returns (xy [N][2] in dtype, bracket [N][2] float64)."""
    c = [_E(dtype(v)) for v in np.asarray(cam, np.float64).reshape(12)]
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = c
    one, two = _E(dtype(1)), _E(dtype(2))
    p = np.asarray(px, np.float64).astype(dtype)
    x0 = _E(p[:, 0]) / fx - cx / fx
    y0 = _E(p[:, 1]) / fy - cy / fy
    x, y = x0, y0
    with np.errstate(all="ignore"):
        for _ in range(LIFT_STEPS):
            r2 = x * x + y * y
            icdist = (one + ((k6 * r2 + k5) * r2 + k4) * r2) / (one + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = two * p1 * x * y + p2 * (r2 + two * x * x)
            dy = p1 * (r2 + two * y * y) + two * p2 * x * y
            x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x.v, y.v], axis=1), np.stack([x.e, y.e], axis=1)


def distort(cam, xy):
    """the forward model (spaceToPlane with the rational distortion): normalised xy [N][2] -> pixels, float64.  The generator's way
    into pixels and the lift's round trip."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in np.asarray(cam, np.float64).reshape(12))
    x, y = np.asarray(xy, np.float64)[:, 0], np.asarray(xy, np.float64)[:, 1]
    r2 = x * x + y * y
    cd = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def f32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def stage_pixels(cur_px, prev_px, flags):
    """flag bit 0: the pixels pass through float, as cv::Point2f"""
    c, p = np.asarray(cur_px, np.float64).reshape(-1, 2), np.asarray(prev_px, np.float64).reshape(-1, 2)
    return (f32(c), f32(p)) if flags & 1 else (c, p)


def velocity_of(un_cur, un_prev, dt, flags, dtype=np.float64):
    """ptsVelocity (:361-363) from the lift's outputs: with the flag the difference is a float's, the quotient a double's, the result
    a float's (un_* are then floats already); without it (un_cur - un_prev) / dt in dtype"""
    if flags & 1:
        d = (np.asarray(un_cur, np.float64).astype(np.float32) - np.asarray(un_prev, np.float64).astype(np.float32)).astype(np.float64)
        return f32(d / np.float64(dt))
    return (np.asarray(un_cur).astype(dtype) - np.asarray(un_prev).astype(dtype)) / dtype(dt)


def virtual_of(xy_cur, xy_prev, col, row, focal, flags, dtype=np.float64):
    """[n][4] = u1 v1 (cur) u2 v2 (prev) of the virtual camera, from the unrounded lift: u = focal x + col / 2"""
    h = np.array([col / 2.0, row / 2.0] * 2).astype(dtype)
    v = dtype(focal) * np.concatenate([xy_cur, xy_prev], axis=1).astype(dtype) + h
    return f32(v).astype(dtype) if flags & 1 else v


def lift_stage(cur_px, prev_px, cam, dt, col, row, focal, flags, dtype=np.float64):
    """stage 1 and 2 on staged pixels.  Returns dict(un_cur, un_prev, velocity (rounded through float with the flag), raw_cur, raw_prev
    (unrounded, dtype), e_cur, e_prev, e_vel (float64 brackets of the unrounded values), virt [n][4])"""
    xc, ec = lift(cam, cur_px, dtype)
    xp, ep = lift(cam, prev_px, dtype)
    fl = flags & 1
    un_c, un_p = (f32(xc), f32(xp)) if fl else (xc, xp)
    with np.errstate(all="ignore"):
        dv = _E(xc, ec) - _E(xp, ep)
        e_vel = (dv / _E(dtype(dt))).e
        vel = velocity_of(un_c, un_p, dt, flags, dtype)
    return dict(un_cur=un_c, un_prev=un_p, velocity=vel, raw_cur=xc, raw_prev=xp, e_cur=ec, e_prev=ep, e_vel=e_vel,
                virt=virtual_of(xc, xp, col, row, focal, flags, dtype))


# ---------------------------------------------------------------------------------------------------------------- 8-point algorithm
def _acc(C):
    """sum over axis 1, one term after the other"""
    return np.add.accumulate(C, axis=1)[:, -1]


def design(virt, samples, dtype=np.float64, order=0):
    """the normalised samples: dict(A [H][8][9], c [H][4], s1, s2 [H], ok [H]); rows in the sample's order (reversed for order 1)"""
    complete = (samples >= 0).all(axis=1)
    s = np.where(samples >= 0, samples, 0)
    if order:
        s = s[:, ::-1]
    P = np.asarray(virt).astype(dtype)[s]                                      # [H][8][4]
    c = _acc(P) * dtype(0.125)
    d = P - c[:, None, :]
    m1 = _acc(np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1])[:, :, None])[:, 0] * dtype(0.125)
    m2 = _acc(np.sqrt(d[:, :, 2] * d[:, :, 2] + d[:, :, 3] * d[:, :, 3])[:, :, None])[:, 0] * dtype(0.125)
    ok = complete & (m1 >= 2.0 ** -23) & (m2 >= 2.0 ** -23)
    root2 = np.sqrt(dtype(2))
    s1, s2 = root2 / np.where(ok, m1, dtype(1)), root2 / np.where(ok, m2, dtype(1))
    x1, y1, x2, y2 = d[:, :, 0] * s1[:, None], d[:, :, 1] * s1[:, None], d[:, :, 2] * s2[:, None], d[:, :, 3] * s2[:, None]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=2)
    return dict(A=A, c=c, s1=s1, s2=s2, ok=ok)


def null_vector(A):
    """the unit right null vector of A [H][8][9]: Householder QR of A^T, row by row; q = H_0 .. H_7 e_8"""
    H = A.shape[0]
    dtype = A.dtype
    hv, hb = [], []
    for j in range(8):
        a = A[:, j, :].copy()
        for i in range(j):
            d = np.zeros(H, dtype)
            for r in range(i, 9):
                d = d + hv[i][:, r - i] * a[:, r]
            d = d * hb[i]
            for r in range(i, 9):
                a[:, r] = a[:, r] - d * hv[i][:, r - i]
        s = np.zeros(H, dtype)
        for r in range(j, 9):
            s = s + a[:, r] * a[:, r]
        nrm = np.sqrt(s)
        v = a[:, j:].copy()
        v[:, 0] = np.where(a[:, j] >= 0, a[:, j] + nrm, a[:, j] - nrm)
        hv.append(v)
        hb.append(dtype.type(1) / (nrm * (nrm + np.abs(a[:, j]))))
    g = np.zeros((H, 9), dtype)
    g[:, 8] = 1
    for i in range(7, -1, -1):
        d = np.zeros(H, dtype)
        for r in range(i, 9):
            d = d + hv[i][:, r - i] * g[:, r]
        d = d * hb[i]
        for r in range(i, 9):
            g[:, r] = g[:, r] - d * hv[i][:, r - i]
    return g


def rank2(g):
    """g [H][9] row-major 3 x 3: one-sided Jacobi on the columns (G V = U S, six sweeps over (0,1), (0,2), (1,2)), the column of the
    smallest norm (the lowest index on a tie) dropped: F0 = sum over the others of g_p v_p^T"""
    dtype = g.dtype
    H = g.shape[0]
    G = g.reshape(H, 3, 3).copy()
    V = np.broadcast_to(np.eye(3, dtype=dtype), (H, 3, 3)).copy()
    dot = lambda p, q: G[:, 0, p] * G[:, 0, q] + G[:, 1, p] * G[:, 1, q] + G[:, 2, p] * G[:, 2, q]
    one = dtype.type(1)
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            aa, bb, cc = dot(p, p), dot(q, q), dot(p, q)
            zeta = (bb - aa) / (dtype.type(2) * cc)
            t = np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
            t = np.where((cc == 0) | np.isnan(t), dtype.type(0), t)
            cs = one / np.sqrt(one + t * t)
            sn = cs * t
            for M in (G, V):
                mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                M[:, :, p] = cs[:, None] * mp - sn[:, None] * mq
                M[:, :, q] = sn[:, None] * mp + cs[:, None] * mq
    nn = np.stack([dot(p, p) for p in range(3)], axis=1)
    drop = np.argmin(np.where(np.isnan(nn), np.inf, nn), axis=1)
    w = (np.arange(3)[None, :] != drop[:, None]).astype(dtype)
    F0 = np.zeros((H, 3, 3), dtype)
    for i in range(3):
        for j in range(3):
            F0[:, i, j] = w[:, 0] * (G[:, i, 0] * V[:, j, 0]) + w[:, 1] * (G[:, i, 1] * V[:, j, 1]) + w[:, 2] * (G[:, i, 2] * V[:, j, 2])
    return F0


def denormalise(F0, c, s1, s2):
    """F = T2^T F0 T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]; [H][9] row-major"""
    tx1, ty1, tx2, ty2 = -(c[:, 0] * s1), -(c[:, 1] * s1), -(c[:, 2] * s2), -(c[:, 3] * s2)
    M = np.zeros_like(F0)
    M[:, :, 0], M[:, :, 1] = F0[:, :, 0] * s1[:, None], F0[:, :, 1] * s1[:, None]
    M[:, :, 2] = F0[:, :, 0] * tx1[:, None] + F0[:, :, 1] * ty1[:, None] + F0[:, :, 2]
    F = np.zeros_like(F0)
    F[:, 0, :], F[:, 1, :] = s2[:, None] * M[:, 0, :], s2[:, None] * M[:, 1, :]
    F[:, 2, :] = tx2[:, None] * M[:, 0, :] + ty2[:, None] * M[:, 1, :] + M[:, 2, :]
    return F.reshape(-1, 9)


def kappa_of(A, ok):
    """(sigma_1 / sigma_8)^2 of the normalised design matrix, float64 (inf where the hypothesis is invalid)"""
    k = np.full(A.shape[0], np.inf)
    A64 = np.asarray(A, np.float64)
    good = ok & np.isfinite(A64).all(axis=(1, 2))
    if good.any():
        sv = np.linalg.svd(A64[good], compute_uv=False)
        with np.errstate(all="ignore"):
            k[good] = (sv[:, 0] / sv[:, 7]) ** 2
    return np.where(np.isnan(k), np.inf, k)


def minimal_solves(virt, samples, dtype=np.float64, order=0):
    """the 8-point algorithm per sample.  Returns dict(hyp [H][9] (NaN rows where invalid), valid [H], kappa [H])"""
    with np.errstate(all="ignore"):
        D = design(virt, samples, dtype, order)
        F = denormalise(rank2(null_vector(D["A"])), D["c"], D["s1"], D["s2"])
        ok = D["ok"] & np.isfinite(F).all(axis=1)
    F[~ok] = np.nan
    return dict(hyp=F, valid=ok, kappa=kappa_of(D["A"], ok))


def normalised(hyp):
    """unit Frobenius norm, the entry of the largest magnitude positive (float64 picks the entry)"""
    h = np.asarray(hyp)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((h * h).sum(axis=1))
        k = np.argmax(np.abs(np.nan_to_num(np.asarray(h, np.float64))), axis=1)
        sg = np.where(h[np.arange(h.shape[0]), k] < 0, -1, 1).astype(h.dtype)
        return h * (sg / nrm)[:, None]


def hyp_bracket(kappa):
    return EPS * np.asarray(kappa, np.float64)


# ---------------------------------------------------------------------------------------------------------------- scoring, scan
def score(virt, hyp, threshold, dtype=np.float64):
    """OpenCV's symmetric epipolar distance of every hypothesis against every point.  Returns dict(count [H], mask [H][n], e2 [H][n]
    = max(d1, d2), valid, thr2, margin_unit [H][n]: the first-order bound of |delta e2| / e2 at the threshold per unit of the largest
    entry deviation of the unit-norm hypothesis, see undecided())"""
    hyp = np.asarray(hyp).astype(dtype)
    valid = np.isfinite(hyp).all(axis=1)
    F = np.where(valid[:, None], hyp, dtype(0))
    v = np.asarray(virt).astype(dtype)
    u1, v1, u2, v2 = v[None, :, 0], v[None, :, 1], v[None, :, 2], v[None, :, 3]
    f = [F[:, i, None] for i in range(9)]
    thr2 = dtype(np.float64(threshold) * np.float64(threshold))
    with np.errstate(all="ignore"):
        a, b, c = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        D2 = a * a + b * b
        d2 = (u2 * a + v2 * b + c) ** 2 / D2
        at, bt, ct = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        D1 = at * at + bt * bt
        d1 = (u1 * at + v1 * bt + ct) ** 2 / D1
        mask = valid[:, None] & (d1 <= thr2) & (d2 <= thr2)
        e2 = np.where(np.isnan(d1) | np.isnan(d2), dtype(np.inf), np.maximum(d1, d2))
        # sensitivity: with |delta F_ij| <= delta |F|_F, |delta N| <= delta L1 L2 |F|_F and |delta a|, |delta b| <= delta L1 |F|_F
        # (L = |u| + |v| + 1); at the threshold |N| = thr sqrt(D): |delta d| / d <= 2 delta |F|_F L1 (L2 / thr + sqrt 2) / sqrt D
        nF = np.sqrt(np.asarray((F * F).sum(axis=1), np.float64))[:, None]
        L1, L2 = np.asarray(np.abs(u1) + np.abs(v1) + 1, np.float64), np.asarray(np.abs(u2) + np.abs(v2) + 1, np.float64)
        thr = float(np.sqrt(np.float64(thr2)))
        mu2 = 2 * nF * L1 * (L2 / thr + np.sqrt(2.0)) / np.sqrt(np.asarray(D2, np.float64))
        mu1 = 2 * nF * L2 * (L1 / thr + np.sqrt(2.0)) / np.sqrt(np.asarray(D1, np.float64))
    return dict(count=mask.sum(axis=1).astype(np.int32), mask=mask, e2=e2, d1=d1, d2=d2, valid=valid, thr2=thr2, mu1=mu1, mu2=mu2)


def scan(count, n, iterations, confidence):
    """k = 0, 1, .. while k < n_iters: a count > max(best count, 7) becomes the best and updates n_iters (RANSACUpdateNumIters with 8
    model points, np_pnp's function).  Returns dict(best, n_iters, best_count, ratios, scanned)"""
    best, best_count, n_iters, ratios = -1, 0, min(iterations, len(count)), []
    k = 0
    while k < n_iters:
        if count[k] > max(best_count, M_POINTS - 1):
            best, best_count = k, int(count[k])
            n_iters, q = npp.update_num_iters(confidence, best_count, n, M_POINTS, n_iters)
            if q is not None:
                ratios.append(q)
        k += 1
    return dict(best=best, n_iters=n_iters, best_count=best_count, ratios=ratios, scanned=k)


def classify(cur, prev, dt):
    """BAD_INPUT (on the staged pixels; tested first), TOO_FEW or OK"""
    if not (np.isfinite(cur).all() and np.isfinite(prev).all() and np.isfinite(dt) and dt > 0):
        return BAD_INPUT
    return TOO_FEW if cur.shape[0] < 8 else OK


def pair(cur_px, prev_px, cam, dt, col, row, focal, iterations, threshold, confidence, seed, flags, dtype=np.float64, order=0):
    """the whole operator for one pair; every stage's result is in the returned dict"""
    cur, prev = stage_pixels(cur_px, prev_px, flags)
    n = cur.shape[0]
    out = dict(info=classify(cur, prev, dt), n=n)
    if out["info"] == BAD_INPUT:
        return out
    out.update(lift_stage(cur, prev, cam, dt, col, row, focal, flags, dtype))
    if out["info"] == TOO_FEW:
        return out
    samples, _ = sample_table(n, iterations, seed)
    ms = minimal_solves(out["virt"], samples, dtype, order)
    sc = score(out["virt"], ms["hyp"], threshold, dtype)
    sn = scan(sc["count"], n, iterations, confidence)
    out.update(samples=samples, hyp=ms["hyp"], kappa=ms["kappa"], count=sc["count"], e2=sc["e2"], d1=sc["d1"], d2=sc["d2"], mu1=sc["mu1"],
               mu2=sc["mu2"], thr2=sc["thr2"], best=sn["best"], n_iters=sn["n_iters"], ratios=sn["ratios"], scanned=sn["scanned"])
    if sn["best"] < 0:
        out["info"] = NO_MODEL
        return out
    status = sc["mask"][sn["best"]]
    keep = np.full(n, -1, np.int32)
    idx = np.flatnonzero(status)
    keep[:idx.size] = idx
    out.update(status=status, keep_idx=keep, n_inliers=sn["best_count"], F=ms["hyp"][sn["best"]])
    return out
