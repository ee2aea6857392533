"""A hand-built window with a second camera — TEST INFRASTRUCTURE (tests/test_feature_check.py, tests/linearize_cases.py)."""
import numpy as np

import idepth_gen
from rtk_visual_inertial_navigation_amd import synth
from rtk_visual_inertial_navigation_amd.flat import FlatWindow
from rtk_visual_inertial_navigation_amd.ordering import my_ordering


def _project(pose, ex, X, pbg):
    R, Re = synth.q_to_R(pose[3:]), synth.q_to_R(ex[3:])
    pc = Re.T @ (R.T @ (X - pose[:3]) + pbg - ex[:3])
    return pc[:2] / pc[2]


def stereo_window(seed=31):
    """A hand-built window: a small synthetic window whose short tracks are inverse depths (kind 0), with a second camera's
    extrinsic appended to the pose pool (variable, so the factors that name it take the generic path), stereo world-point factors
    for three landmarks, kind-1 and kind-2 inverse-depth factors, one inverse depth that only a kind-2 factor names (constant),
    and one landmark without any factor (constant).  Meant to be checked at the uploaded state."""
    base = idepth_gen.convert_short_tracks(synth.make_window(3, K=6, F=30, S=5, seed=seed), max_track=3)
    a = base.a
    rng = np.random.default_rng(seed)
    nP, nS, nL, nC = base.n_pose, base.n_sb, base.n_lm, base.n_sc
    K = base.meta["K"]                                   # the first camera's extrinsic is pose K
    pose = a["pose"].reshape(-1, 7)
    ex2 = pose[K].copy(); ex2[:3] += synth.q_to_R(ex2[3:]) @ np.array([0.11, 0.0, 0.0])
    pose2 = np.vstack([pose, ex2]); e2 = nP
    sh = lambda b: int(b) if b < nP else int(b) + 1      # global block ids behind the pose pool move up by one
    pidx = a["proj_idx"].reshape(-1, 3).copy(); puv = a["proj_uv"].reshape(-1, 2).copy()
    lm = a["lm"].reshape(-1, 3)
    # an unobserved landmark: landmark 0 loses its factors and is held constant
    keep = pidx[:, 2] != 0
    pidx, puv = pidx[keep], puv[keep]
    add_i, add_uv = [], []
    for l in (1, 2, 3):
        for p, e, _ in pidx[pidx[:, 2] == l]:
            add_i.append([p, e2, l]); add_uv.append(_project(pose2[p], ex2, lm[l], base.pbg) + rng.normal(0, 1e-3, 2))
    pidx = np.vstack([pidx, np.array(add_i, np.int32)]); puv = np.vstack([puv, np.array(add_uv)])
    kind = list(a["idp_kind"]); iidx = [list(r) for r in a["idp_idx"].reshape(-1, 5)]; ipts = [r.copy() for r in a["idp_pts"].reshape(-1, 6)]
    sc = list(a["sc"])
    lams = sorted(set(r[4] for r in iidx))
    for c in lams[:4]:
        first = next(i for i, r in enumerate(iidx) if r[4] == c)
        fi, fj, ex = iidx[first][0], iidx[first][1], iidx[first][2]
        pts_i = ipts[first][:3]
        Xa = synth.q_to_R(pose2[ex][3:]) @ (pts_i / sc[c]) + pose2[ex][:3] - base.pbg
        Xw = synth.q_to_R(pose2[fi][3:]) @ Xa + pose2[fi][:3]
        uvr_j = _project(pose2[fj], ex2, Xw, base.pbg) + rng.normal(0, 1e-3, 2)
        uvr_i = _project(pose2[fi], ex2, Xw, base.pbg) + rng.normal(0, 1e-3, 2)
        kind.append(1); iidx.append([fi, fj, ex, e2, c]); ipts.append(np.concatenate([pts_i, uvr_j, [1.0]]))
        kind.append(2); iidx.append([-1, -1, ex, e2, c]); ipts.append(np.concatenate([pts_i, uvr_i, [1.0]]))
    lone = len(sc); sc.append(0.2)                       # an inverse depth only a kind-2 factor names: 5 m along pts_i
    pts_l = np.array([0.05, -0.02, 1.0])
    Xb = synth.q_to_R(pose2[K][3:]) @ (pts_l / 0.2) + pose2[K][:3] - base.pbg
    kind.append(2); iidx.append([-1, -1, K, e2, lone])
    ipts.append(np.concatenate([pts_l, _project(np.array([0, 0, 0, 0, 0, 0, 1.0]), ex2, Xb, base.pbg) + 2e-3, [1.0]]))
    is_const = np.concatenate([a["is_const"][:nP], [0], a["is_const"][nP:], [1]]).astype(np.uint8)
    is_const[nP + 1 + nS + 0] = 1
    roles = {}
    for k, v in base.meta["roles"].items():
        roles[k] = [sh(b) for b in v] if isinstance(v, (list, tuple, np.ndarray)) else (sh(v) if v is not None else None)
    roles["extrinsics"] = list(roles["extrinsics"]) + [e2]
    o_b, o_g, nt = my_ordering(roles, is_const)
    kw = {k: v for k, v in a.items() if k not in ("pose", "sc", "is_const", "order_block", "order_group", "proj_idx", "proj_uv",
                                                   "idp_kind", "idp_idx", "idp_pts", "prior_blk")}
    w = FlatWindow(pose=pose2, sc=np.array(sc), is_const=is_const, order_block=o_b, order_group=o_g, n_tail=int(nt),
                   proj_idx=pidx, proj_uv=puv, idp_kind=np.array(kind, np.int32), idp_idx=np.array(iidx, np.int32), idp_pts=np.array(ipts),
                   prior_blk=np.array([sh(b) for b in a["prior_blk"]], np.int32), proj_sqrt_info=base.proj_sqrt_info,
                   proj_loss_a=base.proj_loss_a, pbg=base.pbg, gw=base.gw, base=base.base, meta=dict(base.meta, roles=roles), **kw)
    assert w.n_blocks == is_const.size
    return w, lone
