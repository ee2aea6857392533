"""numpy referee of the batched RANSAC PnP operator (swf_pnp_frame_batch), one entry point per stage, each taking the
previous stage's output as an argument:

    stage_points -> sample_table -> guess -> minimal_solves -> score -> scan -> refine -> to_imu          (frame() chains them)

dtype is np.float64 or np.longdouble.  order 0 adds the normal equations point by point in ascending order; order 1 is a second
legitimate order: the sample's points reversed in the minimal solve, and 128 strided partial sums combined by a halving tree in the
refinement (the shape of the device's sum)."""
import numpy as np

OK, TOO_FEW, NO_MODEL, UNREFINED, BAD_INPUT = 0, 1, 2, 3, 4
NMAX, HMAX = 1024, 128
K_MIN, K_REF = 6, 10
DRAWS = 64
Z_MIN = 1e-12
TH_MIN = 1e-12
DBL_MIN = np.finfo(np.float64).tiny
M64 = (1 << 64) - 1
TRI = [(i, j) for i in range(6) for j in range(i + 1)]


# ---------------------------------------------------------------------------------------------------------------- sampler
def splitmix64(x):
    """the output function of splitmix64 at state x + 0x9E3779B97F4A7C15 (mod 2^64)"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_table(n, iterations, seed):
    """(samples [H][5] int32, rejected draws): H = iterations for n >= 5, one row 0 1 2 3 -1 for n == 4.  A sample that is not complete
    after 64 draws keeps -1 in its open places (an invalid hypothesis)."""
    if n == 4:
        return np.array([[0, 1, 2, 3, -1]], np.int32), 0
    out = np.full((iterations, 5), -1, np.int32)
    rejected = 0
    for k in range(iterations):
        got = []
        for j in range(DRAWS):
            x = splitmix64((seed + 64 * k + j) & M64)
            idx = ((x >> 32) * n) >> 32
            if idx in got:
                rejected += 1
                continue
            got.append(idx)
            if len(got) == 5:
                break
        out[k, :len(got)] = got
    return out, rejected


# ---------------------------------------------------------------------------------------------------------------- small algebra
def stage_points(pts_w, pts_uv, flags):
    """flag bit 0: the points pass through float, as cv::Point3f / Point2f"""
    pw, uv = np.asarray(pts_w, np.float64).reshape(-1, 3), np.asarray(pts_uv, np.float64).reshape(-1, 2)
    if flags & 1:
        with np.errstate(over="ignore"):
            pw, uv = pw.astype(np.float32).astype(np.float64), uv.astype(np.float32).astype(np.float64)
    return pw, uv


def guess(Ps_prev, Rs_prev, tic, ric, pbg, dtype=np.float64):
    """cam_T_w of the previous frame: RCam = Rs ric, PCam = Rs (tic - pbg) + Ps; R0 = RCam^T, t0 = -(R0 PCam)"""
    Ps, Rs, tic, ric, pbg = (np.asarray(v, np.float64).astype(dtype) for v in (Ps_prev, Rs_prev, tic, ric, pbg))
    Rs, ric = Rs.reshape(3, 3), ric.reshape(3, 3)
    RCam = _mm(Rs, ric)
    PCam = _mv(Rs, tic - pbg) + Ps
    R0 = RCam.T.copy()
    return R0, -_mv(R0, PCam)


def to_imu(R, t, tic, ric, pbg, dtype=np.float64):
    """cam_T_w -> Ps, Rs of the IMU frame: RCam = R^T, PCam = RCam (-t); Rs = RCam ric^T, Ps = PCam - Rs (tic - pbg)"""
    R, t, tic, ric, pbg = (np.asarray(v).astype(dtype) for v in (R, t, tic, ric, pbg))
    ric = ric.reshape(3, 3)
    RCam = R.reshape(3, 3).T
    PCam = _mv(RCam, -t)
    Rs = _mm(RCam, ric.T)
    return PCam - _mv(Rs, tic - pbg), Rs


def _mm(A, B):
    """3 x 3 product, terms added left to right (no BLAS: also for longdouble)"""
    return A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :] + A[..., :, 2, None] * B[..., None, 2, :]


def _mv(A, v):
    return A[..., :, 0] * v[..., None, 0] + A[..., :, 1] * v[..., None, 1] + A[..., :, 2] * v[..., None, 2]


def exp_so3(w):
    """Rodrigues' formula for w [B][3]; I + [w]_x below |w| = 1e-12"""
    dtype = w.dtype
    B = w.shape[0]
    th2 = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    th = np.sqrt(th2)
    small = ~(th >= TH_MIN)
    ths = np.where(small, dtype.type(1), th)
    a = np.where(small, dtype.type(1), np.sin(ths) / ths)
    c = np.where(small, dtype.type(0), (dtype.type(1) - np.cos(ths)) / (ths * ths))
    K = np.zeros((B, 3, 3), dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    K2 = w[:, :, None] * w[:, None, :] - th2[:, None, None] * np.eye(3, dtype=dtype)
    return np.eye(3, dtype=dtype) + a[:, None, None] * K + c[:, None, None] * K2


def chol_solve6(A, b):
    """unpivoted Cholesky of A [B][6][6] (lower triangle read), solve A x = -b.  Returns x, ok: ok is False where a pivot is not > 0."""
    dtype = A.dtype
    B = A.shape[0]
    L = np.zeros((B, 6, 6), dtype)
    ok = np.ones(B, bool)
    for j in range(6):
        d = A[:, j, j].copy()
        for k in range(j):
            d = d - L[:, j, k] * L[:, j, k]
        ok &= d > 0
        d = np.sqrt(np.where(d > 0, d, dtype.type(1)))
        L[:, j, j] = d
        for i in range(j + 1, 6):
            s = A[:, i, j].copy()
            for k in range(j):
                s = s - L[:, i, k] * L[:, j, k]
            L[:, i, j] = s / d
    y = np.zeros((B, 6), dtype)
    for i in range(6):
        s = -b[:, i]
        for k in range(i):
            s = s - L[:, i, k] * y[:, k]
        y[:, i] = s / L[:, i, i]
    x = np.zeros((B, 6), dtype)
    for i in range(5, -1, -1):
        s = y[:, i].copy()
        for k in range(i + 1, 6):
            s = s - L[:, k, i] * x[:, k]
        x[:, i] = s / L[:, i, i]
    return x, ok


def residuals(R, t, P, U):
    """R [B][3][3], t [B][3], P [B][m][3], U [B][m][2] -> q = R p, z, e2 = |r|^2, r [B][m][2], iz"""
    q = R[:, None, :, 0] * P[:, :, None, 0] + R[:, None, :, 1] * P[:, :, None, 1] + R[:, None, :, 2] * P[:, :, None, 2]
    pc = q + t[:, None, :]
    z = pc[:, :, 2]
    iz = 1 / np.where(z == 0, z.dtype.type(1), z)
    r = np.stack([pc[:, :, 0] * iz - U[:, :, 0], pc[:, :, 1] * iz - U[:, :, 1]], axis=2)
    return q, pc, z, iz, r


def _sum(C, order, idx=None, nthreads=128):
    """C [B][N][K] -> [B][K]; order 0: ascending, one term after the other; order 1: descending, or (with the points' indices idx
    [N / 2]; two rows per point) strided partial sums per thread and a halving tree"""
    if order == 0:
        return np.add.accumulate(C, axis=1)[:, -1]
    if idx is None:
        return np.add.accumulate(C[:, ::-1], axis=1)[:, -1]
    B, N, K = C.shape
    top = (int(idx.max()) // nthreads + 1) * nthreads if idx.size else nthreads
    full = np.zeros((B, top, 2, K), C.dtype)
    full[:, idx] = C.reshape(B, N // 2, 2, K)
    part = full.reshape(B, top // nthreads, nthreads, 2, K).transpose(0, 2, 1, 3, 4).reshape(B, nthreads, -1, K)
    p = np.add.accumulate(part, axis=2)[:, :, -1]
    s = nthreads // 2
    while s:
        p = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0]


def gauss_newton(R, t, P, U, steps, order=0, idx=None):
    """steps Gauss-Newton steps on r = (x/z - u, y/z - v), p_c = R p_w + t, from R [B][3][3], t [B][3] over P [B][m][3], U [B][m][2]:
    J = [-J_p [R p_w]_x | J_p], unpivoted Cholesky of J^T J, R <- Exp(dtheta) R, t <- t + dt.
    Returns R, t, ok [B] (False from the step on that met |z| < 1e-12, a pivot <= 0 or a non-finite value; R, t of such a row are
    not to be used), cond [B] (largest condition number of J^T J over the steps, inf where not ok)."""
    dtype = R.dtype
    B, m = P.shape[0], P.shape[1]
    R, t = R.copy(), t.copy()
    ok = np.ones(B, bool)
    cond = np.zeros(B)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            q, pc, z, iz, r = residuals(R, t, P, U)
            ok &= (np.abs(z) >= Z_MIN).all(axis=1)
            jx2, jy2 = -(pc[:, :, 0] * iz * iz), -(pc[:, :, 1] * iz * iz)
            zero = np.zeros_like(iz)
            G = np.stack([np.stack([jx2 * q[:, :, 1], iz * q[:, :, 2] - jx2 * q[:, :, 0], -(iz * q[:, :, 1]), iz, zero, jx2], axis=2),
                          np.stack([jy2 * q[:, :, 1] - iz * q[:, :, 2], -(jy2 * q[:, :, 0]), iz * q[:, :, 0], zero, iz, jy2], axis=2)], axis=2)
            G = G.reshape(B, 2 * m, 6)
            rr = r.reshape(B, 2 * m)
            C = np.concatenate([np.stack([G[:, :, i] * G[:, :, j] for i, j in TRI], axis=2), G * rr[:, :, None]], axis=2)
            S = _sum(C, order, idx)
            A = np.zeros((B, 6, 6), dtype)
            for k, (i, j) in enumerate(TRI):
                A[:, i, j] = S[:, k]
                A[:, j, i] = S[:, k]
            b = S[:, 21:]
            x, pos = chol_solve6(A, b)
            ok &= pos & np.isfinite(x).all(axis=1)
            A64 = np.where(np.isfinite(A), A, 0).astype(np.float64)
            c = np.full(B, np.inf)
            good = ok & (np.abs(A64).max(axis=(1, 2)) > 0)
            if good.any():
                c[good] = np.linalg.cond(A64[good])
            cond = np.maximum(cond, c)
            x = np.where(ok[:, None], x, dtype.type(0))
            R = np.where(ok[:, None, None], _mm(exp_so3(x[:, :3]), R), R)
            t = t + x[:, 3:]
    return R, t, ok, cond


# ---------------------------------------------------------------------------------------------------------------- stages
def minimal_solves(pw, uv, samples, R0, t0, dtype=np.float64, order=0):
    """K_MIN steps per sample from the guess.  Returns dict(hyp [H][12] (R row-major, t; NaN rows where invalid), valid [H], cond [H])"""
    H = samples.shape[0]
    m = 5 if pw.shape[0] >= 5 else 4
    complete = (samples[:, :m] >= 0).all(axis=1)
    s = np.where(samples[:, :m] >= 0, samples[:, :m], 0)
    P, U = pw.astype(dtype)[s], uv.astype(dtype)[s]
    R, t, ok, cond = gauss_newton(np.broadcast_to(R0.astype(dtype), (H, 3, 3)), np.broadcast_to(t0.astype(dtype), (H, 3)), P, U, K_MIN, order)
    ok &= complete
    hyp = np.concatenate([R.reshape(H, 9), t], axis=1)
    hyp[~ok] = np.nan
    cond[~ok] = np.inf
    return dict(hyp=hyp, valid=ok, cond=cond)


def score(pw, uv, hyp, threshold, dtype=np.float64):
    """every hypothesis against every point: inlier iff z > 0 and |r|^2 <= thr^2.  Returns dict(count [H], mask [H][n], e2, z)"""
    hyp = np.asarray(hyp).astype(dtype)
    H, n = hyp.shape[0], pw.shape[0]
    valid = np.isfinite(hyp).all(axis=1)
    hz = np.where(valid[:, None], hyp, dtype(0))
    with np.errstate(all="ignore"):
        _, _, z, _, r = residuals(hz[:, :9].reshape(H, 3, 3), hz[:, 9:], np.broadcast_to(pw.astype(dtype), (H, n, 3)), np.broadcast_to(uv.astype(dtype), (H, n, 2)))
        e2 = r[:, :, 0] * r[:, :, 0] + r[:, :, 1] * r[:, :, 1]
        thr2 = dtype(np.float64(threshold) * np.float64(threshold))
        mask = valid[:, None] & (z > 0) & (e2 <= thr2)
    return dict(count=mask.sum(axis=1).astype(np.int32), mask=mask, e2=e2, z=z, thr2=thr2, valid=valid)


def update_num_iters(confidence, count, n, m, n_iters):
    """OpenCV's RANSACUpdateNumIters with ep = (n - count) / n.  Returns (n_iters, ratio): ratio is the quotient that was rounded, or
    None where none was"""
    p = min(max(float(confidence), 0.0), 1.0)
    ep = min(max((n - count) / float(n), 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    w = 1.0 - ep
    wm = w
    for _ in range(m - 1):
        wm = wm * w
    d = 1.0 - wm
    if d < DBL_MIN:
        return 0, None
    num, den = float(np.log(num)), float(np.log(d))
    if den >= 0 or -num >= n_iters * -den:
        return n_iters, (None if den >= 0 else num / den)
    q = num / den
    return int(np.rint(q)), q


def scan(count, n, m, iterations, confidence):
    """k = 0, 1, .. while k < n_iters: a hypothesis with count > max(best_count, m - 1) becomes the best and updates n_iters.
    Returns dict(best, n_iters, best_count, ratios)"""
    best, best_count, n_iters, ratios = -1, 0, min(iterations, len(count)), []
    k = 0
    while k < n_iters:
        if count[k] > max(best_count, m - 1):
            best, best_count = k, int(count[k])
            n_iters, q = update_num_iters(confidence, best_count, n, m, n_iters)
            if q is not None:
                ratios.append(q)
        k += 1
    return dict(best=best, n_iters=n_iters, best_count=best_count, ratios=ratios)


def refine(pw, uv, hyp_best, mask, dtype=np.float64, order=0):
    """K_REF steps from the best hypothesis over its inliers.  Returns dict(R, t, ok, cond); R, t are the unrefined ones where not ok"""
    idx = np.flatnonzero(mask)
    h = np.asarray(hyp_best).astype(dtype)
    R0, t0 = h[:9].reshape(1, 3, 3), h[9:].reshape(1, 3)
    R, t, ok, cond = gauss_newton(R0, t0, pw.astype(dtype)[idx][None], uv.astype(dtype)[idx][None], K_REF, order, idx if order else None)
    if not ok[0] or not (np.isfinite(R).all() and np.isfinite(t).all()):
        return dict(R=R0[0], t=t0[0], ok=False, cond=np.inf)
    return dict(R=R[0], t=t[0], ok=True, cond=float(cond[0]))


def classify(pw, uv, Ps_prev, Rs_prev):
    """TOO_FEW, BAD_INPUT (on the staged points) or OK"""
    if pw.shape[0] < 4:
        return TOO_FEW
    if not (np.isfinite(pw).all() and np.isfinite(uv).all() and np.isfinite(np.asarray(Ps_prev, np.float64)).all()
            and np.isfinite(np.asarray(Rs_prev, np.float64)).all()):
        return BAD_INPUT
    return OK


def frame(pts_w, pts_uv, Ps_prev, Rs_prev, tic, ric, pbg, iterations, threshold, confidence, seed, flags, dtype=np.float64, order=0):
    """the whole operator for one frame; every stage's result is in the returned dict"""
    pw, uv = stage_points(pts_w, pts_uv, flags)
    n = pw.shape[0]
    out = dict(info=classify(pw, uv, Ps_prev, Rs_prev), n=n)
    if out["info"] != OK:
        return out
    m = 5 if n >= 5 else 4
    samples, _ = sample_table(n, iterations, seed)
    R0, t0 = guess(Ps_prev, Rs_prev, tic, ric, pbg, dtype)
    ms = minimal_solves(pw, uv, samples, R0, t0, dtype, order)
    sc = score(pw, uv, ms["hyp"], threshold, dtype)
    sn = scan(sc["count"], n, m, iterations, confidence)
    out.update(m=m, samples=samples, hyp=ms["hyp"], hyp_cond=ms["cond"], count=sc["count"], e2=sc["e2"], z=sc["z"], thr2=sc["thr2"],
               best=sn["best"], n_iters=sn["n_iters"], ratios=sn["ratios"])
    if sn["best"] < 0:
        out["info"] = NO_MODEL
        return out
    mask = sc["mask"][sn["best"]]
    rf = refine(pw, uv, ms["hyp"][sn["best"]], mask, dtype, order)
    Ps, Rs = to_imu(rf["R"], rf["t"], tic, ric, pbg, dtype)
    out.update(info=OK if rf["ok"] else UNREFINED, inlier=mask, n_inliers=sn["best_count"], R=rf["R"], t=rf["t"], ref_cond=rf["cond"], Ps=Ps, Rs=Rs)
    return out
