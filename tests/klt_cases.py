"""The inputs of the KLT tests and their referee results, built once per process.  A case is one image pair with its points and the
arguments of the call: dict(name, prev, cur, pts, guess, args)."""
import functools

import numpy as np

import klt_gen as kg
import np_klt as nk

H, W = 96, 128                                      # the size of everything but the truth and pyramid cases
SHIFT = (3.3, -2.6)


def case(name, prev, cur, pts, guess=None, **args):
    a = dict(nk.DEFAULTS)
    a.update(args)
    return dict(name=name, prev=prev, cur=cur, pts=np.asarray(pts, np.float64).reshape(-1, 2), guess=guess, args=a)


@functools.lru_cache(maxsize=None)
def truth_cases():
    """the four truth cases of the issue at the reference defaults, 64 points each"""
    out = []
    for k, (h, w, sh, margin, levels) in enumerate(kg.TRUTH):
        prev, cur = kg.pair(h, w, sh, 100 + k)
        out.append(case("truth%d" % k, prev, cur, kg.points(h, w, 64, margin, 100 + k)))
        out[-1].update(shift=sh, levels=levels)
    return out


@functools.lru_cache(maxsize=None)
def count_cases():
    """1, 63, 65 and 257 points: below, at and above a workgroup's four waves and a wave's 64 lanes"""
    prev, cur = kg.pair(H, W, SHIFT, 7)
    return [case("count%d" % n, prev, cur, kg.points(H, W, n, 16, 200 + n)) for n in (1, 63, 65, 257)]


@functools.lru_cache(maxsize=None)
def pyramid_cases():
    """odd sizes, one level that is just built (23 x 24 at win 21) and levels that are not (24 x 31 at win 5 stops after two of four)"""
    out = []
    for k, (h, w, win, lv) in enumerate(((45, 47, 21, 3), (96, 128, 21, 3), (177, 201, 21, 3), (24, 31, 5, 4))):
        prev, cur = kg.pair(h, w, (1.2, -0.7), 300 + k)
        out.append(case("pyr%dx%d" % (h, w), prev, cur, kg.points(h, w, 5, win // 2 + 1, 300 + k), win=win, max_level=lv))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    prev, cur = kg.pair(H, W, SHIFT, 11)
    border = [(0, 0), (W - 1, H - 1), (0, 50), (64, 0), (W - 1, 40), (30, H - 1),                  # on the border
              (5, 5), (W - 7, H - 6), (12.5, 60.25), (70, 9.75), (W - 15, 30), (50, H - 20),      # within win of it
              (-5, 40), (W + 4, 40), (60, -5), (60, H + 4), (-5, -5),                             # outside by 5 px
              (-40, 40), (W + 39, 50), (60, -40), (60, H + 39), (-40, -40)]                       # outside by 40 px
    out = [case("border", prev, cur, border)]
    p30, c30 = kg.pair(H, W, (30.0, 0.0), 12)
    out.append(case("shift30", p30, c30, kg.points(H, W, 64, 12, 12)))
    pm, cm = kg.pair(H, W, (-2.0, 1.5), 17)          # a small flow towards the left and lower borders: tracked onto the border rows
    rng = np.random.default_rng(17)
    onto = np.concatenate([np.column_stack([rng.uniform(1.6, 3.2, 10), rng.uniform(20, 70, 10)]),
                           np.column_stack([rng.uniform(20, 100, 10), rng.uniform(H - 4.2, H - 2.6, 10)])])
    out.append(case("onto_border", pm, cm, onto))
    pf, cf = prev.copy(), cur.copy()
    pf[30:70, 50:90] = 128
    cf[30:70, 50:90] = 128
    rng = np.random.default_rng(13)
    inside = np.column_stack([rng.uniform(61, 79, 12), rng.uniform(41, 59, 12)])
    out.append(case("flat", pf, cf, np.concatenate([inside, kg.points(H, W, 28, 12, 13)])))
    cr = cur.copy()                                  # flat in cur only: the reverse pass meets it
    cr[20:76, 40:100] = 90
    out.append(case("flat_cur", prev, cr, kg.points(H, W, 64, 12, 14)))
    other = kg.tex(H, W, 0.0, 0.0, 999)
    out.append(case("unrelated", prev, other, kg.points(H, W, 64, 12, 15)))
    out.append(case("unrelated_border", prev, other, kg.points(H, W, 64, 0, 16)))
    return out


@functools.lru_cache(maxsize=None)
def option_cases():
    prev, cur = kg.pair(H, W, SHIFT, 21)
    pts = kg.points(H, W, 40, 16, 21)
    return [case("guess", prev, cur, pts, guess=pts + np.array(SHIFT) + 1.5, max_level=1, flags=7),
            case("no_back", prev, cur, pts, flags=1),
            case("win5", prev, cur, pts, win=5),
            case("win11", prev, cur, pts, win=11),
            case("count1", prev, cur, pts, max_count=1),
            case("back0", prev, cur, pts, back_level=0),
            case("back_above", prev, cur, pts, max_level=0, back_level=2)]


RAGGED_N = (0, 1, 7, 64, 65, 130, 3, 64)


@functools.lru_cache(maxsize=None)
def ragged_cases():
    """nine pairs of one call: the point counts of the issue and one BAD_INPUT pair (a NaN coordinate) in the middle"""
    out = []
    for k, n in enumerate(RAGGED_N):
        sh = (1.0 + 0.6 * k, -2.0 + 0.5 * k)
        prev, cur = kg.pair(H, W, sh, 400 + k)
        out.append(case("ragged%d" % k, prev, cur, kg.points(H, W, n, 14, 400 + k)))
    prev, cur = kg.pair(H, W, (1.0, 1.0), 450)
    bad = kg.points(H, W, 9, 14, 450)
    bad[4, 1] = np.nan
    out.insert(4, case("ragged_bad", prev, cur, bad))
    return out


def referee_of(c, flags=None, pyr_fill=0):
    a = dict(c["args"])
    if flags is not None:
        a["flags"] = flags
    return nk.track_pair(c["prev"], c["cur"], c["pts"], c["guess"], pyr_fill=pyr_fill, **a)


@functools.lru_cache(maxsize=None)
def referee(group, flags=None):
    """the referee's results of a group of cases ('truth', 'count', 'pyramid', 'edge', 'option', 'ragged'), in order"""
    cases = dict(truth=truth_cases, count=count_cases, pyramid=pyramid_cases, edge=edge_cases, option=option_cases, ragged=ragged_cases)[group]()
    return [referee_of(c, flags) for c in cases]
