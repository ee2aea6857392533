"""Short synthetic sequences for the resident tracker: the texture of tests/klt_gen.py at 96 x 128, the smallest size at
which every stage still does real work (two pyramid levels get built), moving by (3.3, -2.6) px per frame.  Each case steers the
bookkeeping of trackImage into one of its branches; tests/test_tracker.py asserts on the CPU that the branch is reached."""
import functools
import json
import os

import numpy as np

import klt_gen as kg
import np_tracker as ntk

H, W = 96, 128
SHIFT = (3.3, -2.6)
SMALL = dict(min_dist=10, max_cnt=60, cand_cap=4096, f_iterations=128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def camera():
    """tests/golden/cam0_pinhole_full.json as fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6"""
    c = json.load(open(os.path.join(ROOT, "tests", "golden", "cam0_pinhole_full.json")))
    p, d = c["projection_parameters"], c["distortion_parameters"]
    return np.array([p["fx"], p["fy"], p["cx"], p["cy"], d["k1"], d["k2"], d["p1"], d["p2"], d["k3"], d["k4"], d["k5"], d["k6"]])


def moving(n, seed, shift=SHIFT):
    """n frames of one texture, frame k shifted by k * shift"""
    return [kg.tex(H, W, -k * shift[0], -k * shift[1], seed) for k in range(n)]


def noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def case(name, imgs, masks=None, remove=None, **opt):
    o = dict(SMALL)
    o.update(opt)
    n = len(imgs)
    return dict(name=name, imgs=[np.ascontiguousarray(i) for i in imgs], times=[1.0 + 0.05 * k for k in range(n)], masks=masks,
                seeds=[100 + k for k in range(n)], remove=remove or {}, opt=ntk.options(**o))


@functools.lru_cache(maxsize=None)
def cases():
    out = [case("plain", moving(5, 11))]
    # (b) a block that moves across the motion of the rest: its tracks leave the epipolar lines of the others
    base, other = moving(4, 12), moving(4, 13, (2.6, 3.3))
    imgs = []
    for a, b in zip(base, other):
        a = a.copy()
        a[30:72, 44:100] = b[30:72, 44:100]
        imgs.append(a)
    out.append(case("block", imgs))
    # (c) the second frame is unrelated noise: every track is lost and the stream restarts from detection
    m = moving(4, 14)
    out.append(case("restart", [m[0], noise(3), m[2], m[3]]))
    # (d) a budget that is used up: the first frame's mask keeps the ten points in the interior, so all of them survive the motion and
    # the later frames have nothing to detect; on the second frame setMask drops one of them and one is added
    inner, full = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    inner[34:70, 24:84] = 255
    out.append(case("budget", moving(4, 15), masks=[inner, full, full, full], max_cnt=10))
    # (e) never eight points: the F gate does not run
    out.append(case("too_few", moving(4, 16), max_cnt=6))
    # (f) cand_cap 64 on noise images (and on the texture, which has more corners than that as well): nothing is ever added
    m = moving(4, 17)
    out.append(case("too_many", [noise(7), noise(8), m[2], m[3]], cand_cap=64))
    # (g) the caller's mask blocks a rectangle, the same on every frame
    mk = np.full((H, W), 255, np.uint8)
    mk[20:60, 30:90] = 0
    out.append(case("mask", moving(4, 18), masks=[mk] * 4))
    # (h) removeOutliers between the frames, an id that is not there among them
    out.append(case("remove", moving(5, 19), remove={2: [3, 25, 9999, 40], 3: [], 4: [45, 7]}))
    # (f') more candidates than cand_cap on a frame whose right half is noise: what setMask keeps of the left half's tracks stays
    m = moving(4, 17)
    half = m[2].copy()
    half[:, 64:] = noise(6)[:, 64:]
    out.append(case("too_many_keeps", [m[0], m[1], half, m[3]], cand_cap=300))
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
