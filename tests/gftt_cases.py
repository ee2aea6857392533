"""The inputs of the corner-detection tests and their referee results, built once per process.  A case is one frame with its tracked
points and the arguments of the call: dict(name, img, mask, px, tc, args).  Everything is 96 x 128 or smaller: seconds on the GPU."""
import functools

import numpy as np

import np_gftt as ng

H, W = 96, 128
SMALL = dict(max_cnt=1000, min_dist=10, quality=0.01, disc_halfwidth=None, cand_cap=4096, flags=1)
NONE = np.zeros((0, 2))


def case(name, img, px=NONE, tc=None, mask=None, **args):
    a = dict(SMALL)
    a.update(args)
    px = np.asarray(px, np.float64).reshape(-1, 2)
    tc = np.ones(px.shape[0], np.int32) if tc is None else np.asarray(tc, np.int32).reshape(-1)
    return dict(name=name, img=np.ascontiguousarray(img, dtype=np.uint8), mask=mask, px=px, tc=tc, args=a)


def noise(h=H, w=W, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def grid(h, w):
    return np.mgrid[0:h, 0:w]


def checkerboard():
    yy, xx = grid(H, W)
    return (((yy // 8) + (xx // 8)) % 2 * 255).astype(np.uint8)


def sinusoid():
    yy, xx = grid(H, W)
    return np.rint((127.5 + 200.0 * np.sin(xx * 0.21 + 0.3) * np.sin(yy * 0.17 + 1.0)).clip(0, 255)).astype(np.uint8)     # clipped: plateaus


def spread_points(step, x0=6, y0=6):
    """a lattice of points `step` apart: none inside another's disc for min_dist < step"""
    return np.array([(x, y) for y in range(y0, H - 2, step) for x in range(x0, W - 2, step)], np.float64)


@functools.lru_cache(maxsize=None)
def image_cases():
    yy, xx = grid(H, W)
    out = [case("noise_all", noise())]                                           # budget 1000: the list is exhausted
    out += [case("noise_budget%d" % b, noise(), max_cnt=b) for b in (40, 63, 64, 65)]     # the chunk edges of the walk
    out.append(case("checkerboard", checkerboard()))                             # every candidate ties: the index decides
    out.append(case("sinusoid", sinusoid()))
    out.append(case("constant", np.full((H, W), 93, np.uint8)))                  # m = 0
    out.append(case("lattice1", ((yy + xx) % 2 * 255)))                          # one-pixel lattice: the central differences vanish
    out.append(case("stripes2", ((xx % 4 < 2) * 255)))                           # |Ix| = 1020, Iy = 0: rank-deficient everywhere, m = 0
    out.append(case("odd51x67", noise(51, 67, 6)))
    out.append(case("tiny8x8", noise(8, 8, 7)))
    e = ng.eig_image(noise())
    y, x = np.unravel_index(np.argmax(e), e.shape)
    m = np.full((H, W), 255, np.uint8)
    m[max(y - 9, 0):y + 10, max(x - 12, 0):x + 13] = 0                           # the global maximum is blocked
    out.append(case("mask_rect", noise(), mask=m))
    out.append(case("mask_zero", noise(), mask=np.zeros((H, W), np.uint8)))
    pair = np.zeros((H, W), np.uint8)
    for x, y in ((20, 20), (25, 20), (60, 50), (63, 54)):                        # two pairs of corners exactly r = 5 apart: all kept
        pair[y, x] = 255
    out.append(case("exactly_r", pair, min_dist=5))
    # more candidates than one round of the selection holds (4096): the list is exhausted over two rounds, and the budget is met in
    # the second one
    big = case("two_rounds", noise(256, 320, 8), max_cnt=1024, min_dist=12, cand_cap=8192)
    full = referee_of(big)
    assert full["n_cand"] > 4096 + 64 and full["n_new"] < 1024
    out += [big, case("second_round_budget", noise(256, 320, 8), max_cnt=full["n_new"] - 2, min_dist=12, cand_cap=8192)]
    return out


@functools.lru_cache(maxsize=None)
def point_cases():
    """the tracked-point cases, all on the noise image"""
    img = noise()
    rng = np.random.default_rng(11)
    rand = np.column_stack([rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40)])
    out = [case("skipped", img, spread_points(24), max_cnt=12),                  # 20 kept >= max_cnt: stages B to D do not run
           case("skipped_equal", img, spread_points(24), max_cnt=20),            # budget exactly 0
           case("budget_one", img, spread_points(24), max_cnt=21),
           case("equal_counts", img, rand, tc=np.full(40, 3)),                   # ties go by index
           case("counts", img, rand, tc=rng.integers(1, 6, 40)),
           case("nested", img, [(50, 40), (52, 41), (49, 44), (58, 40), (61, 40), (70, 70), (70.4, 70.4)], tc=[2, 9, 9, 1, 5, 7, 7]),
           # r = 5: (43, 34) is at offset (3, 4) from (40, 30), on the rim, blocked under <=; (46, 30) at offset (6, 0) is not
           case("rim", img, [(40, 30), (43, 34), (46, 30), (40, 35), (40, 36)], tc=[5, 4, 3, 2, 1], min_dist=5),
           case("outside", img, [(-1, 10), (10, -0.6), (W - 0.5, 20), (W - 0.51, 21), (30, H - 0.5), (30, H), (-0.5, -0.5), (1e12, 5), (64, 48)]),
           # 21.499999999 is 21.5 as a float and then 22 (rint to even) instead of 21; 20.5 -> 20, 23.5 -> 24 either way
           case("half_float", img, [(21.499999999, 30.5), (20.5, 60), (23.5, 61.5), (34, 30.5)], flags=1, min_dist=12),
           case("half_double", img, [(21.499999999, 30.5), (20.5, 60), (23.5, 61.5), (34, 30.5)], flags=0, min_dist=12),
           # OpenCV's midpoint raster of radius 10 is wider than the Euclidean disc in four rows
           case("user_table", img, rand, tc=np.full(40, 3), disc_halfwidth=[10, 10, 10, 10, 9, 9, 8, 7, 6, 5, 3]),
           case("square_table", img, rand, tc=np.full(40, 3), disc_halfwidth=[10] * 11),
           case("full_house", img, spread_points(11, 3, 3)[:60], max_cnt=70)]     # many old points, few free pixels
    return out


@functools.lru_cache(maxsize=None)
def option_cases():
    bad = np.array([(20.0, 20.0), (np.nan, 30.0), (40.0, 40.0)])
    return [case("too_many", noise(), cand_cap=64),
            case("bad_nan", noise(), bad),
            case("bad_inf_as_float", noise(), [(1e39, 20.0)], flags=1),           # finite as a double, infinite as a float
            case("bad_count", noise(), [(20.0, 20.0), (50.0, 50.0)], tc=[3, -1])]


RAGGED = dict(max_cnt=45, min_dist=10, cand_cap=600)


@functools.lru_cache(maxsize=None)
def ragged_cases():
    """nine frames of one call: no points, points, every candidate tied, a flat image, a BAD_INPUT frame, a blocked rectangle, nothing
    free, the detector skipped, and more candidates than cand_cap"""
    rng = np.random.default_rng(23)
    full = np.full((H, W), 255, np.uint8)
    rect = full.copy()
    rect[30:70, 20:90] = 0
    pts = lambda n: np.column_stack([rng.uniform(-3, W + 2, n), rng.uniform(-3, H + 2, n)])
    bad = pts(9)
    bad[4, 1] = np.inf
    out = [case("r_none", sinusoid(), mask=full, **RAGGED),
           case("r_points", noise(H, W, 32), pts(30), tc=rng.integers(1, 9, 30), mask=full, **RAGGED),
           case("r_checker", checkerboard(), pts(7), mask=full, **RAGGED),
           case("r_constant", np.full((H, W), 200, np.uint8), pts(3), mask=full, **RAGGED),
           case("r_bad", noise(H, W, 33), bad, mask=full, **RAGGED),
           case("r_rect", noise(H, W, 34), pts(65), tc=rng.integers(1, 4, 65), mask=rect, **RAGGED),
           case("r_blocked", noise(H, W, 35), pts(5), mask=np.zeros((H, W), np.uint8), **RAGGED),
           case("r_skipped", noise(H, W, 36), spread_points(12), mask=full, **RAGGED),
           case("r_too_many", noise(H, W, 37), mask=full, **RAGGED)]
    return out


def referee_of(c, **over):
    a = dict(c["args"])
    a.update(over)
    return ng.detect_frame(c["img"], c["px"], c["tc"], mask=c["mask"], **a)


@functools.lru_cache(maxsize=None)
def referee(group):
    """the referee's results of a group of cases ('image', 'point', 'option', 'ragged'), in order"""
    cases = dict(image=image_cases, point=point_cases, option=option_cases, ragged=ragged_cases)[group]()
    return [referee_of(c) for c in cases]
