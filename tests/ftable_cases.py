"""Synthetic sequences for the resident feature table.  No images: a seeded cloud of points in front of a smoothly moving
camera, projected with the table's own extrinsic formula, ids handed out as the tracker would (ascending by first frame) and shuffled
within each frame.  window = 5, frame_cap = 40, feature_continue = 2, min_track = 3, min_long = 2, long_len = 3 everywhere;
feat_cap = 300 in the main cases and 24 in `overflow`.

A window of 5 frames of at most 40 points cannot hold more than 120 features (a feature that stays needs two of the 200 observation
slots, the 40 of the newest frame one), so the main cases cross the 64-lane wave but not the 256-thread chunk; `wide` is added for
that with frame_cap = 128 and nothing else changed: two-frame tracks bring its list to 270 of its 300 slots.

play() drives anything with solver.FeatureTable's methods through a script and records the whole state, the counters and every
output after every step; Referee gives tests/np_ftable.py that interface for several streams."""
import functools
import math

import numpy as np

import np_ftable as nf

WINDOW, FRAME_CAP = 5, 40
BASE = dict(window=WINDOW, frame_cap=FRAME_CAP, feature_continue=2, feat_cap=300, min_track=3, min_long=2, long_len=3)
N_FRAMES = 8
DT = 0.05
TIC = np.array([0.05, -0.02, 0.03])
PBG = np.array([0.01, 0.02, -0.015])


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, np.float64)


RIC = rot(2, 0.02) @ rot(0, -0.015)

# the script every case runs; ("slide", key) takes the case's mode of that name
SCRIPT = ([("add", k) for k in range(5)] + [("pnp",), ("tri",), ("list",), ("solved", 0), ("remove",), ("parallax",), ("slide", "s1"),
          ("add", 5), ("pnp",), ("tri",), ("list",), ("solved", 1), ("remove",), ("parallax",), ("slide", "s2"),
          ("add", 6), ("tri",), ("list",), ("parallax",), ("slide", "s3"), ("slide", "s3"), ("add", 7), ("list",)])


def camera_point(w, P, R):
    return RIC.T @ (R.T @ (w - P) + PBG - TIC)


def make(name, seed, step, n_points, modes, p_keep=0.8, behind=True, n_frames=N_FRAMES, **opt):
    """one case: n_frames (8) frames of at most n_points points; the camera moves by `step` per frame"""
    o = dict(BASE)
    o.update(opt)
    rng = np.random.default_rng(seed)
    Ps = np.array([[k * step, 0.1 * k * step, 0.02 * k * step] for k in range(n_frames)])
    Rs = np.array([rot(1, 0.004 * k) @ rot(0, 0.002 * k) for k in range(n_frames)])
    truth, alive, frames, next_id, prev = {}, [], [], 0, {}
    for k in range(n_frames):
        p = p_keep(k) if callable(p_keep) else p_keep
        pair = frames[0]["pair"] if frames else set()         # two tracks live for exactly the frames 0 and 1: removeBack leaves
        alive = [i for i in alive if not (k == 2 and i in pair) and ((k == 1 and i in pair) or rng.random() < p)]   # them one observation
        while len(alive) < n_points:
            w = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.8, 1.8), rng.uniform(4.0, 9.0)]) + Ps[k]
            if behind and k == 0 and next_id == 3:
                w = np.array([0.4, -0.3, -6.0])                 # one landmark behind the cameras: init_depth, then solve_flag 2
            truth[next_id] = w
            alive.append(next_id)
            next_id += 1
        ids = np.array(alive, np.int32)
        rng.shuffle(ids)
        obs, now = np.zeros((ids.size, 7)), {}
        for r, i in enumerate(ids):
            pc = camera_point(truth[int(i)], Ps[k], Rs[k])
            x, y = pc[0] / pc[2], pc[1] / pc[2]
            vx, vy = ((x - prev[int(i)][0]) / DT, (y - prev[int(i)][1]) / DT) if int(i) in prev else (0.0, 0.0)
            obs[r] = [x, y, 1.0, 460.0 * x + 376.0, 460.0 * y + 240.0, vx, vy]
            now[int(i)] = (x, y)
        prev = now
        frames.append(dict(ids=ids, obs=obs, pair=set(int(i) for i in alive[:2]) if k == 0 else set()))
    return dict(name=name, opt=nf.options(**o), frames=frames, Ps=Ps, Rs=Rs, truth=truth, modes=modes)


@functools.lru_cache(maxsize=None)
def cases():
    return [make("back", 1, 0.30, 40, dict(s1=1, s2=1, s3=1), p_keep=lambda k: 0.9 if k % 2 else 0.4),
            make("front", 2, 0.012, 40, dict(s1=2, s2=2, s3=2)),
            make("mixed", 3, 0.09, 37, dict(s1=1, s2=2, s3=1), p_keep=lambda k: 0.95 if k % 2 else 0.3),
            make("sparse", 4, 0.05, 5, dict(s1=0, s2=1, s3=2), p_keep=0.6, behind=False),
            make("overflow", 5, 0.20, 20, dict(s1=1, s2=1, s3=2), p_keep=0.5, feat_cap=24),
            make("wide", 6, 0.15, 90, dict(s1=1, s2=2, s3=1), p_keep=lambda k: float(k % 2), frame_cap=128)]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


MAIN = ("back", "front", "mixed", "sparse")


def solved_world(c, ids, rnd):
    """what a solve would hand back for the listed ids: the truth, moved a little"""
    out = np.zeros((len(ids), 3))
    for j, i in enumerate(ids):
        out[j] = c["truth"][int(i)] + 0.01 * np.array([math.sin(i + rnd), math.cos(2 * i + rnd), math.sin(3 * i - rnd)])
    return out


def solved_flags(ids, rnd):
    """the feature check's verdict: every eleventh id an outlier, one with the depth bit, the rest clean or merely unobserved"""
    return np.array([1 if (int(i) + rnd) % 11 == 5 else 2 if (int(i) + rnd) % 23 == 7 else 4 if int(i) % 5 == 0 else 0 for i in ids], np.uint8)


class Referee:
    """tests/np_ftable.py behind the interface of solver.FeatureTable, one Table per stream"""

    def __init__(self, n_streams, tri=nf.dlt_triangulate, **opt):
        self.n_streams, self.opt, self.tri = n_streams, nf.options(**opt), tri
        self.T = [nf.Table(**opt) for _ in range(n_streams)]

    def close(self):
        pass

    def add_frame(self, ids, obs):
        for t, i, o in zip(self.T, ids, obs):
            t.add_frame(i, o)

    def pnp_points(self):
        return [t.pnp_points() for t in self.T]

    def triangulate(self, Ps, Rs, tic, ric, pbg):
        for s, t in enumerate(self.T):
            t.triangulate(np.asarray(Ps)[s], np.asarray(Rs)[s], tic, ric, pbg, self.tri)

    def list(self):
        return [t.list() for t in self.T]

    def set_solved(self, lm_world, flags, Ps, Rs, tic, ric, pbg):
        for s, t in enumerate(self.T):
            t.set_solved(lm_world[s], None if flags is None else flags[s], np.asarray(Ps)[s], np.asarray(Rs)[s], tic, ric, pbg)

    def remove_failures(self):
        return [t.remove_failures() for t in self.T]

    def check_parallax(self):
        for t in self.T:
            t.check_parallax()

    def slide(self, mode, P1, R1, tic, ric, pbg):
        for s, t in enumerate(self.T):
            t.slide(int(mode[s]), np.asarray(P1)[s], np.asarray(R1)[s], tic, ric, pbg)

    def clear(self):
        for t in self.T:
            t.clear()

    def counts(self):
        return np.array([t.counts for t in self.T], np.int32).reshape(self.n_streams, len(nf.COUNTS)), np.array([t.parallax for t in self.T], np.float64)

    def state(self):
        return [t.state() for t in self.T]


def window_poses(streams, wins):
    Ps, Rs = np.zeros((len(streams), WINDOW, 3)), np.tile(np.eye(3), (len(streams), WINDOW, 1, 1))
    for s, (c, win) in enumerate(zip(streams, wins)):
        for w, k in enumerate(win):
            Ps[s, w], Rs[s, w] = c["Ps"][k], c["Rs"][k]
    return Ps, Rs


def play(T, streams, script=SCRIPT, each=None):
    """runs the script over the cases `streams` as the streams of T.  -> one record per step: dict(step, out, state, counts, parallax).
    each(T): called after every step, before the state is read (the CPU tests check the invariants there)."""
    wins = [[] for _ in streams]
    ext = (TIC, RIC, PBG)
    records = []
    for step in script:
        op, out = step[0], None
        if op == "add":
            frames = [c["frames"][step[1]] for c in streams]
            T.add_frame([f["ids"] for f in frames], [f["obs"] for f in frames])
            for win, f in zip(wins, frames):
                if len(win) < WINDOW and not f.get("bad"):
                    win.append(step[1])
        elif op == "pnp":
            out = T.pnp_points()
        elif op == "tri":
            T.triangulate(*window_poses(streams, wins), *ext)
        elif op == "list":
            out = T.list()
            listing = out
        elif op == "solved":
            world = [solved_world(c, l["lm_id"], step[1]) for c, l in zip(streams, listing)]
            flags = [solved_flags(l["lm_id"], step[1]) for l in listing]
            T.set_solved(world, flags, *window_poses(streams, wins), *ext)
        elif op == "remove":
            out = T.remove_failures()
        elif op == "parallax":
            T.check_parallax()
        elif op == "slide":
            mode = [c["modes"][step[1]] if isinstance(step[1], str) else step[1] for c in streams]
            P1 = np.array([c["Ps"][win[1]] if len(win) > 1 else np.zeros(3) for c, win in zip(streams, wins)])
            R1 = np.array([c["Rs"][win[1]] if len(win) > 1 else np.eye(3) for c, win in zip(streams, wins)])
            T.slide(mode, P1, R1, *ext)
            for win, m in zip(wins, mode):
                if len(win) >= 2 and m in (1, 2):
                    win.pop(0 if m == 1 else -2)
        else:
            raise ValueError(op)
        if each is not None:
            each(T, op)
        counts, parallax = T.counts()
        records.append(dict(step=step, out=out, state=T.state(), counts=np.array(counts), parallax=np.array(parallax)))
    return records
