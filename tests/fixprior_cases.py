"""Inputs of the stand-alone fix-and-hold tests (tests/test_fix_prior.py) and of the derivation of their tolerances: random linear
priors with fixed-integer constraint rows, dimension 7 to 140, one to six groups, up to 64 rows.  Deterministic (seeded)."""
import numpy as np

DIMS = (7, 23, 45, 64, 97, 140)
EPS = 1e-8
ISTD = 1.0 / 0.03


def make_problem(n, seed, n_groups=None, s_min=1e-1, s_max=1e3, null_dirs=0):
    """J = U diag(s) V^T with singular values log-uniform in [s_min, s_max] (information s^2), r ~ N(0, 1); the last min(n - 6, 64)
    coordinates (n - 3 below ten dimensions) are the one-dimensional blocks, a random subset of them carries the rows (every group at least two).  null_dirs > 0
    projects that many directions of the first six coordinates out of J: directions nobody measured (and no row touches)."""
    rng = np.random.default_rng(1000 * n + seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.exp(rng.uniform(np.log(s_min), np.log(s_max), n))
    J = (U * s) @ V.T
    for k in range(null_dirs):
        u = np.zeros(n); u[:6] = rng.standard_normal(6)
        if k:
            u[k - 1] = 0.0
        u /= np.linalg.norm(u)
        J = J - np.outer(J @ u, u)
    r = rng.standard_normal(n)
    n_sc = min(n - 6, 64) if n >= 10 else n - 3
    G = n_groups if n_groups is not None else int(rng.integers(1, 7))
    G = max(1, min(G, n_sc // 2))
    nrows = int(rng.integers(2 * G, n_sc + 1))
    coords = (n - n_sc) + rng.permutation(n_sc)[:nrows]
    grp = np.concatenate([np.repeat(np.arange(G), 2), rng.integers(0, G, nrows - 2 * G)])
    rows, seen = [], set()
    for c, g in zip(coords, grp):
        v = 0.0 if g not in seen else float(rng.integers(-50, 51))
        seen.add(g)
        rows.append((int(c), 100 + int(g), v))          # (arbitrary group labels)
    return J, r, rows


def healthy_cases():
    out = []
    for n in DIMS:
        for seed in (0, 1):
            out.append(("n%d_s%d" % (n, seed), make_problem(n, seed)))
    # a weak direction (information 1e-4) next to istd^2 ~ 1.1e3 and 1e6
    out.append(("n64_weak", make_problem(64, 7, n_groups=3, s_min=1e-2)))
    out.append(("n140_g6", make_problem(140, 9, n_groups=6)))
    return out


def deficient_cases():
    return [("n23_null1", make_problem(23, 3, null_dirs=1)), ("n64_null2", make_problem(64, 4, null_dirs=2)),
            ("n140_null1", make_problem(140, 5, null_dirs=1))]
