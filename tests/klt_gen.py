"""Inputs of the KLT tests: a smooth synthetic texture evaluated at shifted coordinates, so that the true flow between the two images
of a pair is one known vector everywhere, and points drawn in the interior."""
import numpy as np

N_WAVES = 24


def tex(h, w, dx, dy, seed):
    """A sum of 24 sinusoids (|frequency| 0.02 .. 0.35 rad/px per axis with random sign, amplitude 0.3 .. 1, random phase) evaluated
    at (x + dx, y + dy).  The grey scale is fixed by the amplitudes alone (three standard deviations of the sum map to 0 and 255,
    what lies beyond is clipped), so every shift of one seed has the same brightness.  uint8 [h][w]."""
    rng = np.random.default_rng(seed)
    fx = rng.uniform(0.02, 0.35, N_WAVES) * rng.choice([-1.0, 1.0], N_WAVES)
    fy = rng.uniform(0.02, 0.35, N_WAVES) * rng.choice([-1.0, 1.0], N_WAVES)
    amp = rng.uniform(0.3, 1.0, N_WAVES)
    ph = rng.uniform(0.0, 2.0 * np.pi, N_WAVES)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    s = np.zeros((h, w))
    for k in range(N_WAVES):
        s += amp[k] * np.sin(fx[k] * (x + dx) + fy[k] * (y + dy) + ph[k])
    sigma = np.sqrt(0.5 * (amp * amp).sum())
    return np.rint(np.clip(127.5 + 127.5 * s / (3.0 * sigma), 0.0, 255.0)).astype(np.uint8)


def pair(h, w, shift, seed):
    """(prev, cur) with the true flow `shift` = (sx, sy) from prev to cur"""
    return tex(h, w, 0.0, 0.0, seed), tex(h, w, -shift[0], -shift[1], seed)


def points(h, w, n, margin, seed):
    """n points (x, y), uniform in the interior with a margin"""
    rng = np.random.default_rng(seed + 7919)
    return np.column_stack([rng.uniform(margin, w - 1 - margin, n), rng.uniform(margin, h - 1 - margin, n)])


# the truth cases of the issue: rows, cols, shift, margin, max_level
TRUTH = [(176, 200, (13.7, -9.2), 26, 3), (96, 128, (3.3, -2.6), 16, 2), (48, 64, (1.6, -1.2), 14, 1), (176, 200, (0.0, 0.0), 12, 3)]
