"""numpy referee of the post-solve feature check (swf_batch_check_features): the depth-sign test of SWFOptimization::Double2Vector
(R/swf/swf.cpp:214-229) and the mean reprojection error of OutliersRejection (R/swf/swf_image.cpp:255-308), restated from their
formulas and evaluated in the reference's operation order, in float64 or np.longdouble.

    P_j = p_j - R_j pbg,  R from the normalised quaternion
    world point X:      pc = R_e^T (R_j^T (X - P_j) - t_e),  err = |pc.xy / pc.z - uv|,  depth = pc.z of the first factor
    inverse depth lam:  X = R_i (R_ex (pts_i / lam) + t_ex - pbg) + p_i, the anchor's own observation first, depth = 1 / lam
    mean_err = (sum err) / n_obs, summed left to right;  OUTLIER iff mean_err * proj_sqrt_info > threshold;  NEG_DEPTH iff depth < 0
    (lam < 0);  UNOBSERVED for a landmark without factors.

order="factor" evaluates the camera point the way the projection factor does, R_j^T (X - p_j) + pbg - t_e: the second legitimate
operation order, used to measure how far two correct evaluations may differ (tests/test_feature_check.py)."""
import numpy as np

OUTLIER, NEG_DEPTH, UNOBSERVED = 1, 2, 4


def table(w):
    """The observation table of a FlatWindow: features = landmarks in pool order, then the distinct inverse depths ascending; a
    feature's observations in the caller's factor order.  Pose index -1 = the identity (a lam only kind-2 factors name).
    Raises ValueError when the factors of one inverse depth disagree on (pose_i, pts_i)."""
    a = w.a
    pidx = a["proj_idx"].reshape(-1, 3); puv = a["proj_uv"].reshape(-1, 2)
    kind = a["idp_kind"].ravel(); iidx = a["idp_idx"].reshape(-1, 5); ipts = a["idp_pts"].reshape(-1, 6)
    n_lm = w.n_lm
    pj, pe, ft, pi, pa, uv, fid, obs0, is_idp, pts_i = [], [], [], [], [], [], [], [0], [], []
    order = np.argsort(pidx[:, 2], kind="stable") if pidx.size else np.zeros(0, int)
    cnt = np.bincount(pidx[:, 2], minlength=n_lm) if pidx.size else np.zeros(n_lm, int)
    pos = 0
    for l in range(n_lm):
        for i in order[pos:pos + cnt[l]]:
            pj.append(pidx[i, 0]); pe.append(pidx[i, 1]); ft.append(l); pi.append(-1); pa.append(-1); uv.append(puv[i]); fid.append(l)
        pos += cnt[l]
        obs0.append(len(pj)); is_idp.append(False); pts_i.append(np.zeros(3))
    lams = sorted(set(int(c) for c in iidx[:, 4])) if iidx.size else []
    for k, c in enumerate(lams):
        f = n_lm + k
        fac = np.nonzero(iidx[:, 4] == c)[0]
        p0 = ipts[fac[0], :3]
        anchor = next((int(iidx[i, 0]) for i in fac if kind[i] != 2), -1)
        for i in fac:
            if not np.array_equal(ipts[i, :3], p0) or (kind[i] != 2 and iidx[i, 0] != anchor):
                raise ValueError("the factors of inverse depth %d disagree on the anchor" % c)
        ex0 = int(iidx[fac[0], 2])
        pj.append(anchor); pe.append(ex0); ft.append(c); pi.append(anchor); pa.append(ex0); uv.append(p0[:2]); fid.append(f)
        for i in fac:
            kd = kind[i]
            pj.append(anchor if kd == 2 else iidx[i, 1]); pe.append(iidx[i, 2] if kd == 0 else iidx[i, 3])
            ft.append(c); pi.append(anchor); pa.append(iidx[i, 2]); uv.append(ipts[i, 3:5]); fid.append(f)
        obs0.append(len(pj)); is_idp.append(True); pts_i.append(p0)
    I = lambda v: np.array(v, dtype=np.int64).reshape(-1)
    return dict(pj=I(pj), pe=I(pe), ft=I(ft), pi=I(pi), pa=I(pa), uv=np.array(uv, dtype=np.float64).reshape(-1, 2), fid=I(fid),
                obs0=I(obs0), is_idp=np.array(is_idp, dtype=bool).reshape(-1), pts_i=np.array(pts_i, dtype=np.float64).reshape(-1, 3),
                n_lm=n_lm, lams=I(lams))


def _rot(q, one):
    """rows of Quaterniond(w, x, y, z).normalized().toRotationMatrix() for q [n][4] = (x, y, z, w): R[r][c] as a dict of arrays"""
    nn = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    x, y, z, w = q[:, 0] / nn, q[:, 1] / nn, q[:, 2] / nn, q[:, 3] / nn
    two = one + one
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]


def _mul(R, v):
    return [R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] for r in range(3)]


def _mulT(R, v):
    return [R[0][r] * v[0] + R[1][r] * v[1] + R[2][r] * v[2] for r in range(3)]


def check(w, threshold=2.0, dtype=np.float64, order="reference", tab=None):
    """The feature check of FlatWindow `w` at its current state.  Returns dict(mean_err, depth, n_obs, flags, rejected, n_feat,
    whitened = mean_err * proj_sqrt_info, cond = per feature max_k (|X| + |p_j| + |pbg| + |t_e|) / |pc.z|), values in `dtype`."""
    T = tab if tab is not None else table(w)
    a = w.a
    one = dtype(1)
    pose = np.vstack([a["pose"].reshape(-1, 7), [[0, 0, 0, 0, 0, 0, 1]]]).astype(dtype)         # row -1 = the identity
    lm = a["lm"].reshape(-1, 3).astype(dtype); sc = a["sc"].ravel().astype(dtype)
    pbg = [dtype(v) for v in np.asarray(w.pbg, dtype=np.float64)]
    n_feat = T["obs0"].size - 1
    n_obs = np.diff(T["obs0"]).astype(np.int32)
    fid = T["fid"]; idp = T["is_idp"][fid] if fid.size else np.zeros(0, bool)
    Pj, Pe = pose[T["pj"]], pose[T["pe"]]
    # the world point of every observation
    X = [np.zeros(fid.size, dtype) for _ in range(3)]
    wp = ~idp
    for k in range(3):
        X[k][wp] = lm[T["ft"][wp], k] if n_feat and lm.size else 0
    lam_o = np.ones(fid.size, dtype)
    if idp.any():
        sel = np.nonzero(idp)[0]
        lam = sc[T["ft"][sel]]; lam_o[sel] = lam
        Pi, Pa = pose[T["pi"][sel]], pose[T["pa"][sel]]
        pts = T["pts_i"][fid[sel]].astype(dtype)
        v = _mul(_rot(Pa[:, 3:], one), [pts[:, k] / lam for k in range(3)])
        v = [v[k] + Pa[:, k] - pbg[k] for k in range(3)]
        u = _mul(_rot(Pi[:, 3:], one), v)
        for k in range(3):
            X[k][sel] = u[k] + Pi[:, k]
    Rj, Re = _rot(Pj[:, 3:], one), _rot(Pe[:, 3:], one)
    if order == "reference":         # OutliersRejection: P_j first
        t = _mul(Rj, pbg)
        d = [X[k] - (Pj[:, k] - t[k]) for k in range(3)]
        b = _mulT(Rj, d)
        b = [b[k] - Pe[:, k] for k in range(3)]
    else:                            # the projection factor: R_j^T (X - p_j) + pbg - t_e
        b = _mulT(Rj, [X[k] - Pj[:, k] for k in range(3)])
        b = [b[k] + pbg[k] - Pe[:, k] for k in range(3)]
    pc = _mulT(Re, b)
    uv = T["uv"].astype(dtype)
    rx, ry = pc[0] / pc[2] - uv[:, 0], pc[1] / pc[2] - uv[:, 1]
    err = np.sqrt(rx * rx + ry * ry)
    nrm = lambda c: np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    cond_o = (nrm(X) + nrm([Pj[:, k] for k in range(3)]) + nrm([np.full(fid.size, pbg[k]) for k in range(3)]) + nrm([Pe[:, k] for k in range(3)])) / np.abs(pc[2])
    # per feature: left-to-right sum of its run
    acc = np.zeros(n_feat, dtype); cond = np.zeros(n_feat, dtype)
    o0 = T["obs0"][:-1]
    for k in range(int(n_obs.max()) if n_feat else 0):
        m = n_obs > k
        acc[m] = acc[m] + err[o0[m] + k]
        cond[m] = np.maximum(cond[m], cond_o[o0[m] + k])
    seen = n_obs > 0
    mean = np.zeros(n_feat, dtype); depth = np.zeros(n_feat, dtype); zsign = np.zeros(n_feat, dtype)
    mean[seen] = acc[seen] / n_obs[seen].astype(dtype)
    first = o0[seen]
    fi = T["is_idp"][seen] if n_feat else np.zeros(0, bool)
    zsign[seen] = np.where(fi, lam_o[first], pc[2][first])
    depth[seen] = np.where(fi, one / lam_o[first], pc[2][first])
    whitened = mean * dtype(w.proj_sqrt_info)
    flags = np.zeros(n_feat, np.uint8)
    with np.errstate(invalid="ignore"):
        flags[seen & (whitened > dtype(threshold))] |= OUTLIER
        flags[seen & (zsign < 0)] |= NEG_DEPTH
    flags[~seen] = UNOBSERVED
    rejected = np.nonzero(flags & (OUTLIER | NEG_DEPTH))[0].astype(np.int32)
    return dict(mean_err=mean, depth=depth, n_obs=n_obs, flags=flags, rejected=rejected, n_feat=n_feat, whitened=whitened, cond=cond)


def inject(w, rng, n_bad):
    """Displace every observation of n_bad landmarks by 0.020 .. 0.060 (normalised image units) in a random direction; per landmark,
    the angles of all its observations are drawn first, then all their magnitudes.  Returns the landmark indices."""
    bad = rng.choice(w.n_lm, n_bad, replace=False)
    pidx = w.a["proj_idx"].reshape(-1, 3); puv = w.a["proj_uv"].reshape(-1, 2)
    for l in bad:
        obs = np.nonzero(pidx[:, 2] == l)[0]
        ang = rng.uniform(0, 2 * np.pi, obs.size)
        mag = rng.uniform(20, 60, obs.size) / 1000
        puv[obs] += mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return bad
