"""Small scenes that tests/test_oracle.py pins the oracle on and tests/test_gpu_parity.py runs the device on — TEST INFRASTRUCTURE."""
import numpy as np

import np_factors as nf
from rtk_visual_inertial_navigation_amd import synth


def idepth_scene(rng):
    """Two body poses a short step apart, two camera extrinsics (stereo pair), a point a few metres ahead."""
    q = lambda s: (lambda v: v / np.linalg.norm(v))(np.concatenate([rng.normal(0, s, 3) / 2, [1.0]]))
    Pi = np.concatenate([rng.normal(0, 5, 3), q(0.3)]); Pj = nf.pose_plus(Pi, np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.05, 3)]))
    qic = synth.R_to_q(synth.BODY_T_CAM0[:3, :3])
    ex = np.concatenate([synth.BODY_T_CAM0[:3, 3], qic]); ex2 = nf.pose_plus(ex, np.array([0.12, 0.0, 0.0, 0.01, -0.02, 0.005]))
    pts_i = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0]); inv_dep = 1.0 / rng.uniform(3, 25)
    return Pi, Pj, ex, ex2, pts_i, inv_dep


def triangulation_scene(rng, n_frames=12, n_feat=200, pbg=None):
    """Frames along a gently curving path, features in front of consecutive frame pairs; noise-free normalised observations."""
    from scipy.spatial.transform import Rotation
    Ps = np.cumsum(rng.normal([0.6, 0.05, 0.0], 0.05, (n_frames, 3)), axis=0) + np.array([3e6, -1e6, 2e6]) * 0   # local frame
    Rs = np.stack([Rotation.from_rotvec(rng.normal(0, 0.05, 3) + np.array([0, 0, 0.02 * k])).as_matrix() for k in range(n_frames)])
    ric = Rotation.from_euler("xyz", [-1.5, 0.02, -1.55]).as_matrix()
    tic = np.array([0.05, -0.02, 0.1])
    pbg = np.zeros(3) if pbg is None else pbg
    start = rng.integers(0, n_frames - 1, n_feat).astype(np.int32)
    Xw, pt0, pt1 = np.zeros((n_feat, 3)), np.zeros((n_feat, 2)), np.zeros((n_feat, 2))
    for i, f in enumerate(start):
        pc = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0]) * rng.uniform(3, 40)
        Xw[i] = Rs[f] @ (ric @ pc + tic) + Ps[f]
        for pts, ff in ((pt0, f), (pt1, f + 1)):
            q = ric.T @ (Rs[ff].T @ (Xw[i] - Ps[ff]) - tic)
            pts[i] = q[:2] / q[2]
    return Ps, Rs, tic, ric, pbg, start, pt0, pt1, Xw
