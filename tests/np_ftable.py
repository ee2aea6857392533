"""The referee of the resident feature table (swf_ftable_*): the specification at swf_ftable_add_frame in
include/swf_solver.h restated in plain Python, one list of features per stream, scalar float64 arithmetic in the written order, no
np.dot.  Python floats are IEEE doubles, every operation below rounds once and math.sqrt is correctly rounded, so a device kernel
that keeps the order (contraction off) gives the same bits.

The one thing that is not restated is the two-view triangulation itself: the table is specified to be bit-identical to
swf_triangulate_batch, whose kernel is compiled with contraction on and cannot be followed bit for bit by scalar Python.  So
triangulate() gathers start / pt0 / pt1 as the specification says and takes depth and world from a function `tri` with the signature
of solver.triangulate_batch: the GPU tests pass that operator itself (which has its own referees elsewhere), the CPU tests use
dlt_triangulate below, a numpy SVD that is good to rounding and serves only to reach the branches."""
import math

import numpy as np

WINDOW_FULL, TABLE_FULL, BAD_FRAME, STALE_LIST, BAD_SLIDE = 1, 2, 4, 8, 16
FEAT_OUTLIER, FEAT_NEG_DEPTH = 1, 2
COUNTS = ("keyframe", "last_track", "long_track", "new", "erased", "info", "parallax_num", "n_listed", "n_proj", "n_pnp")
KEYFRAME, LAST_TRACK, LONG_TRACK, NEW, ERASED, INFO, PARALLAX_NUM, N_LISTED, N_PROJ, N_PNP = range(10)
DEFAULTS = dict(window=11, feat_cap=4096, frame_cap=350, feature_continue=2, min_track=20, min_long=40, long_len=4,
                new_ratio=0.5, min_parallax=10.0 / 1000.0, focal=1000.0, init_depth=5.0)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def dlt_triangulate(Ps, Rs, tic, ric, pbg, start_frame, pt0, pt1, init_depth=5.0):
    """triangulate's two-view branch (:285-316) with numpy; the stand-in for swf_triangulate_batch where there is no device"""
    Ps, Rs = np.asarray(Ps, np.float64).reshape(-1, 3), np.asarray(Rs, np.float64).reshape(-1, 3, 3)
    tic, ric, pbg = np.asarray(tic, np.float64).reshape(3), np.asarray(ric, np.float64).reshape(3, 3), np.asarray(pbg, np.float64).reshape(3)
    n = len(start_frame)
    depth, world = np.zeros(n), np.zeros((n, 3))
    for i in range(n):
        f = int(start_frame[i])
        if f < 0 or f + 1 >= Ps.shape[0]:
            depth[i] = -1.0
            continue
        poses = []
        for g in (f, f + 1):
            Rc = Rs[g] @ ric
            poses.append(np.hstack([Rc.T, (-Rc.T @ (Ps[g] + Rs[g] @ tic))[:, None]]))
        (u0, v0), (u1, v1) = pt0[i], pt1[i]
        A = np.stack([u0 * poses[0][2] - poses[0][0], v0 * poses[0][2] - poses[0][1], u1 * poses[1][2] - poses[1][0], v1 * poses[1][2] - poses[1][1]])
        x = np.linalg.svd(A)[2][3]
        d = (poses[0][:, :3] @ (x[:3] / x[3]) + poses[0][:, 3])[2]
        if not d > 0:
            d = init_depth
        depth[i] = d
        world[i] = Rs[f] @ (ric @ (np.array([u0, v0, 1.0]) * d) + tic - pbg) + Ps[f]
    return depth, world


def depth_z(w, P, R, tic, ric, pbg):
    """z of ric^T (R^T (w - P) + pbg - tic); R, ric are 3 x 3 nested, row-major"""
    d = [float(w[k]) - float(P[k]) for k in range(3)]
    b = []
    for r in range(3):
        a = (float(R[0][r]) * d[0] + float(R[1][r]) * d[1]) + float(R[2][r]) * d[2]
        b.append((a + float(pbg[r])) - float(tic[r]))
    return (float(ric[0][2]) * b[0] + float(ric[1][2]) * b[1]) + float(ric[2][2]) * b[2]


def inverse(z):
    z = float(z)
    if z == 0.0:
        return math.copysign(math.inf, z)
    return 1.0 / z


class Table:
    """one stream's FeatureManager"""

    def __init__(self, **opt):
        self.o = options(**opt)
        self.n_frames, self.feat, self.n_listed = 0, [], 0
        self.counts, self.parallax = [0] * len(COUNTS), 0.0
        self.reached = {}                                   # branch counters, for the tests that show a case gets there

    def _hit(self, what, n=1):
        self.reached[what] = self.reached.get(what, 0) + n

    @staticmethod
    def end_frame(f):
        return f["start"] + len(f["obs"]) - 1

    # 1 ---------------------------------------------------------------------------------------------------------------------------
    def add_frame(self, ids, obs):
        o, c = self.o, self.counts
        ids = [int(v) for v in np.asarray(ids).reshape(-1)]
        obs = np.asarray(obs, np.float64).reshape(-1, 7)
        bad = len(ids) > o["frame_cap"] or len(set(ids)) != len(ids) or not np.isfinite(obs[:min(len(ids), o["frame_cap"] + 1)]).all()
        full = self.n_frames >= o["window"]
        c[KEYFRAME] = c[LAST_TRACK] = c[LONG_TRACK] = c[NEW] = c[ERASED] = 0
        c[INFO] = BAD_FRAME if bad else WINDOW_FULL if full else 0
        if bad or full:
            self._hit("bad_frame" if bad else "window_full")
            return
        image_index, n0 = self.n_frames, len(self.feat)
        where = {f["id"]: f for f in self.feat}
        assert len(where) == n0
        last = lng = new = dropped = 0
        for i in sorted(range(len(ids)), key=lambda j: ids[j]):          # the reference iterates a std::map: ascending id
            row = [float(v) for v in obs[i]]
            f = where.get(ids[i])
            if f is None:
                if n0 + new + dropped < o["feat_cap"]:
                    self.feat.append(dict(id=ids[i], start=image_index, obs=[row], inp=[False], valid=0, flag=0, idepth=0.0, world=[0.0, 0.0, 0.0]))
                    new += 1
                    if self.feat[-2:-1] and self.feat[-2]["id"] > ids[i]:
                        self._hit("out_of_id_order")
                else:
                    dropped += 1
            else:
                assert len(f["obs"]) < o["window"]
                f["obs"].append(row)
                f["inp"].append(False)
                last += 1
                if len(f["obs"]) >= o["long_len"]:
                    lng += 1
        if dropped:
            c[INFO] |= TABLE_FULL
            self._hit("table_full")
        key = image_index < 2 or last < o["min_track"] or lng < o["min_long"] or float(new) > o["new_ratio"] * float(last)
        self._hit("keyframe" if key else "no_keyframe")
        self.n_frames += 1
        before = len(self.feat)
        self.feat = [f for f in self.feat if not (self.end_frame(f) != self.n_frames - 1 and len(f["obs"]) < o["feature_continue"])]
        c[KEYFRAME], c[LAST_TRACK], c[LONG_TRACK], c[NEW], c[ERASED] = int(key), last, lng, new, before - len(self.feat)
        if c[ERASED]:
            self._hit("remove_out", c[ERASED])

    # 2 ---------------------------------------------------------------------------------------------------------------------------
    def pnp_points(self):
        w, uv = [], []
        cnt = self.n_frames - 1
        if self.n_frames >= 2:
            for f in self.feat:
                idx = cnt - f["start"]
                if f["valid"] and len(f["obs"]) >= idx + 1:
                    w.append(list(f["world"]))
                    uv.append(f["obs"][idx][:2])
        self.counts[N_PNP] = len(w)
        return np.array(w, np.float64).reshape(-1, 3), np.array(uv, np.float64).reshape(-1, 2)

    # 3 ---------------------------------------------------------------------------------------------------------------------------
    def tri_inputs(self):
        """start (frame index within the stream, -1: not to be triangulated), pt0, pt1 for every live feature"""
        start, pt0, pt1 = [], [], []
        for f in self.feat:
            go = not f["valid"] and len(f["obs"]) > 1
            start.append(f["start"] if go else -1)
            pt0.append(f["obs"][0][:2] if go else [0.0, 0.0])
            pt1.append(f["obs"][1][:2] if go else [0.0, 0.0])
        return np.array(start, np.int32), np.array(pt0, np.float64).reshape(-1, 2), np.array(pt1, np.float64).reshape(-1, 2)

    def triangulate(self, Ps, Rs, tic, ric, pbg, tri=dlt_triangulate):
        start, pt0, pt1 = self.tri_inputs()
        if not len(start):
            return
        depth, world = tri(Ps, Rs, tic, ric, pbg, start, pt0, pt1, self.o["init_depth"])
        for f, st, d, w in zip(self.feat, start, depth, world):
            if st < 0 or d == -1.0:
                continue
            if d == self.o["init_depth"]:
                self._hit("init_depth")
            f["idepth"], f["world"], f["valid"] = inverse(d), [float(v) for v in w], 1
            self._hit("triangulated")

    # 4 ---------------------------------------------------------------------------------------------------------------------------
    def listed(self):
        return [f for f in self.feat if len(f["obs"]) >= self.o["feature_continue"]]

    def list(self):
        lm = dict(lm_id=[], lm_world=[], lm_start=[], lm_nobs=[], lm_valid=[])
        pr = dict(proj_frame=[], proj_lm=[], proj_uv=[], proj_new=[])
        for j, f in enumerate(self.listed()):
            lm["lm_id"].append(f["id"]); lm["lm_world"].append(list(f["world"])); lm["lm_start"].append(f["start"])
            lm["lm_nobs"].append(len(f["obs"])); lm["lm_valid"].append(f["valid"])
            for k, row in enumerate(f["obs"]):
                pr["proj_frame"].append(f["start"] + k); pr["proj_lm"].append(j); pr["proj_uv"].append(row[:2])
                pr["proj_new"].append(0 if f["inp"][k] else 1)
                self._hit("proj_old" if f["inp"][k] else "proj_new")
                f["inp"][k] = True
        self.n_listed = len(lm["lm_id"])
        self.counts[N_LISTED], self.counts[N_PROJ] = self.n_listed, len(pr["proj_frame"])
        out = {k: np.array(v, np.int32) for k, v in list(lm.items()) + list(pr.items()) if k not in ("lm_world", "proj_uv")}
        out["lm_world"] = np.array(lm["lm_world"], np.float64).reshape(-1, 3)
        out["proj_uv"] = np.array(pr["proj_uv"], np.float64).reshape(-1, 2)
        return out

    # 5 ---------------------------------------------------------------------------------------------------------------------------
    def set_solved(self, lm_world, flags, Ps, Rs, tic, ric, pbg):
        lm_world = np.asarray(lm_world, np.float64).reshape(-1, 3)
        feats = self.listed()
        if len(feats) != len(lm_world) or len(feats) != self.n_listed:
            self.counts[INFO] = STALE_LIST
            self._hit("stale_list")
            return
        self.counts[INFO] = 0
        for j, f in enumerate(feats):
            f["world"] = [float(v) for v in lm_world[j]]
            f["idepth"] = inverse(depth_z(f["world"], Ps[f["start"]], Rs[f["start"]], tic, ric, pbg))
            f["flag"] = 2 if f["idepth"] < 0.0 else 1
            if f["flag"] == 2:
                self._hit("negative_depth")
            if flags is not None and int(flags[j]) & (FEAT_OUTLIER | FEAT_NEG_DEPTH):
                f["flag"] = 2
                self._hit("flagged")

    # 6 ---------------------------------------------------------------------------------------------------------------------------
    def remove_failures(self):
        gone = [f["id"] for f in self.feat if f["flag"] == 2]
        self.feat = [f for f in self.feat if f["flag"] != 2]
        self.counts[ERASED] = len(gone)
        self._hit("failures_removed", len(gone))
        return np.array(gone, np.int32)

    # 7 ---------------------------------------------------------------------------------------------------------------------------
    def parallax_terms(self):
        idx, terms = self.n_frames - 1, []
        for f in self.feat:
            if f["start"] <= idx - 2 and self.end_frame(f) >= idx - 1:
                oi, oj = f["obs"][idx - 2 - f["start"]], f["obs"][idx - 1 - f["start"]]
                u, v = oi[0] / oi[2], oi[1] / oi[2]
                du, dv = u - oj[0], v - oj[1]
                terms.append(math.sqrt(du * du + dv * dv))
        return terms

    def parallax_mean(self):
        terms = self.parallax_terms()
        total = 0.0
        for t in terms:                                     # sequentially, in list order
            total = total + t
        return (total / float(len(terms)) if terms else None), len(terms)

    def check_parallax(self):
        mean, num = self.parallax_mean()
        self.counts[PARALLAX_NUM] = num
        if num == 0:
            self.counts[KEYFRAME], self.parallax = 1, 0.0
            self._hit("parallax_none")
        else:
            self.parallax = mean * self.o["focal"]
            self.counts[KEYFRAME] = int(mean >= self.o["min_parallax"])
            self._hit("parallax_key" if self.counts[KEYFRAME] else "parallax_no_key")

    # 8 ---------------------------------------------------------------------------------------------------------------------------
    def slide(self, mode, P1, R1, tic, ric, pbg):
        bad = mode not in (0, 1, 2) or (mode != 0 and self.n_frames < 2)
        self.counts[INFO], self.counts[ERASED] = (BAD_SLIDE if bad else 0), 0
        if bad or mode == 0:
            if bad:
                self._hit("bad_slide")
            return
        front, before = self.n_frames - 1, len(self.feat)
        for f in self.feat:
            if mode == 1:
                if f["start"] != 0:
                    f["start"] -= 1
                else:
                    f["idepth"] = inverse(depth_z(f["world"], P1, R1, tic, ric, pbg))
                    del f["obs"][0], f["inp"][0]
                    self._hit("back_erased_obs")
                    if len(f["obs"]) == 1:
                        self._hit("back_left_with_one")
            else:
                if f["start"] == front:
                    f["start"] -= 1
                    self._hit("front_moved")
                elif self.end_frame(f) >= front - 1:
                    j = front - 1 - f["start"]
                    del f["obs"][j], f["inp"][j]
                    self._hit("front_j0" if j == 0 else "front_erased_obs")
        self.feat = [f for f in self.feat if f["obs"]]
        self.counts[ERASED] = before - len(self.feat)
        if self.counts[ERASED]:
            self._hit("slide_erased_feature", self.counts[ERASED])
        self.n_frames -= 1
        for f in self.feat:                                 # removeOut2, world-point effect
            if len(f["obs"]) < self.o["feature_continue"]:
                if any(f["inp"]):
                    self._hit("in_problem_cleared")
                f["inp"] = [False] * len(f["obs"])

    def clear(self):
        self.n_frames, self.feat, self.n_listed = 0, [], 0

    # the state in the layout of solver.FeatureTable.state() ---------------------------------------------------------------------
    def state(self):
        W, n = self.o["window"], len(self.feat)
        obs, inp = np.zeros((n, W, 7)), np.zeros((n, W), np.int32)
        for i, f in enumerate(self.feat):
            obs[i, :len(f["obs"])] = np.array(f["obs"], np.float64).reshape(-1, 7)
            inp[i, :len(f["obs"])] = [int(v) for v in f["inp"]]
        i32 = lambda key: np.array([f[key] for f in self.feat], np.int32)
        return dict(n_frames=self.n_frames, id=i32("id"), start_frame=i32("start"), n_obs=np.array([len(f["obs"]) for f in self.feat], np.int32),
                    valid=i32("valid"), solve_flag=i32("flag"), idepth=np.array([f["idepth"] for f in self.feat], np.float64),
                    world=np.array([f["world"] for f in self.feat], np.float64).reshape(-1, 3), obs=obs, in_problem=inp)

    def check_invariants(self, after_add=False):
        """the list-order invariants: unique ids, every feature inside the window, flags in range; after an add_frame no short
        track that has ended is left"""
        ids = [f["id"] for f in self.feat]
        assert len(set(ids)) == len(ids) <= self.o["feat_cap"]
        assert 0 <= self.n_frames <= self.o["window"]
        for f in self.feat:
            assert 1 <= len(f["obs"]) == len(f["inp"]) <= self.o["window"]
            assert 0 <= f["start"] and self.end_frame(f) <= self.n_frames - 1, (f["id"], f["start"], len(f["obs"]), self.n_frames)
            assert f["valid"] in (0, 1) and f["flag"] in (0, 1, 2)
            assert not (after_add and len(f["obs"]) < self.o["feature_continue"] and self.end_frame(f) != self.n_frames - 1)
