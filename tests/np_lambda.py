"""Referees for the integer least-squares (LAMBDA) search, tests only.

lambda_np   a numpy restatement of the published method: the LtDL factorisation Q = L^T diag(d) L, the LAMBDA reduction
            (integer Gauss transforms and permutations, Teunissen 1995; de Jonge & Tiberius 1996) and the MLAMBDA search
            (Chang, Yang & Zhou 2005) for the m best integer vectors.  It carries Z^-1 and z = Z^T a through the reduction, counts
            search iterations as RTKLIB's lambda() does (a limit of 10000), and rounds every product and sum separately.
brute_force an exhaustive enumerator for small n: every integer point of the box |z_i - a_i| <= sqrt(r^2 Q_ii), where r^2 is the
            distance of the m-th best point among round(a) + {-1, 0, 1}^n (a point within r^2 lies in that box by Cauchy-Schwarz).
ratio_test  the ratio test of SWFOptimization::LambdaSearch on (F, s, Qb, bf).
"""
import itertools
import math

import numpy as np

OK, NOT_PD, LOOP_LIMIT, NO_INPUT = 0, 1, 2, 3
LOOPMAX = 10000
PERMMAX = 10 * LOOPMAX          # permutations of the reduction before it is given up (LOOP_LIMIT)


def _round(x):
    return float(math.floor(x + 0.5))


def _sgn(x):
    return -1.0 if x <= 0.0 else 1.0


def ltdl(Q):
    """Q = L^T diag(d) L (L unit lower triangular), from the last row upwards; only the lower triangle of Q is read.
    Returns (L, d), or None when a pivot is not positive."""
    n = Q.shape[0]
    A = np.tril(np.array(Q, dtype=np.float64))
    L = np.zeros((n, n))
    d = np.zeros(n)
    for i in range(n - 1, -1, -1):
        di = A[i, i]
        if not di > 0.0:
            return None
        d[i] = di
        sa = np.sqrt(di)
        t = A[i, :i + 1] / sa
        A[:i, :i] -= np.tril(np.outer(t[:i], t[:i]))
        L[i, :i + 1] = t / (di / sa)
    return L, d


def reduction(L, d, a):
    """Decorrelation: unimodular Z with Z^T Q Z = L^T diag(d) L reduced.  Returns (L, d, Zi = Z^-1, z = Z^T a), or None after
    PERMMAX permutations."""
    L, d, z = L.copy(), d.copy(), np.array(a, dtype=np.float64).copy()
    n = d.size
    Zi = np.eye(n)
    j = k = n - 2
    nperm = 0
    while j >= 0:
        if j <= k:
            for i in range(j + 1, n):
                mu = _round(L[i, j])
                if mu != 0.0:
                    L[i:, j] -= mu * L[i:, i]
                    Zi[i, :] += mu * Zi[j, :]
                    z[j] -= mu * z[i]
        lj = L[j + 1, j]
        delta = d[j] + lj * lj * d[j + 1]
        if delta + 1e-6 < d[j + 1]:
            eta, lam = d[j] / delta, d[j + 1] * lj / delta
            d[j], d[j + 1] = eta * d[j + 1], delta
            a0, a1 = L[j, :j].copy(), L[j + 1, :j].copy()
            L[j, :j] = -lj * a0 + a1
            L[j + 1, :j] = eta * a0 + lam * a1
            L[j + 1, j] = lam
            L[j + 2:, [j, j + 1]] = L[j + 2:, [j + 1, j]]
            Zi[[j, j + 1], :] = Zi[[j + 1, j], :]
            z[j], z[j + 1] = z[j + 1], z[j]
            k, j = j, n - 2
            nperm += 1
            if nperm >= PERMMAX:
                return None
        else:
            j -= 1
    return L, d, Zi, z


def search(L, d, zs, m):
    """Schnorr-Euchner enumeration on the reduced problem, the radius shrunk once m leaves are known.
    Returns (E [m][n], s [m], iterations)."""
    n = d.size
    Lr = [list(map(float, L[r])) for r in range(n)]
    dd = list(map(float, d))
    zs = list(map(float, zs))
    S = [[0.0] * n for _ in range(n)]
    dist, zb, z, step = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n
    k = n - 1
    zb[k] = zs[k]
    z[k] = _round(zb[k])
    y = zb[k] - z[k]
    step[k] = _sgn(y)
    maxdist, nn, imax = 1e99, 0, 0
    E, s = [[0.0] * n for _ in range(m)], [0.0] * m
    c = 0
    while c < LOOPMAX:
        newdist = dist[k] + y * y / dd[k]
        if newdist < maxdist:
            if k != 0:
                k -= 1
                dist[k] = newdist
                dz = z[k + 1] - zb[k + 1]
                Sk, Sk1, Lk1 = S[k], S[k + 1], Lr[k + 1]
                for i in range(k + 1):
                    Sk[i] = Sk1[i] + dz * Lk1[i]
                zb[k] = zs[k] + Sk[k]
                z[k] = _round(zb[k])
                y = zb[k] - z[k]
                step[k] = _sgn(y)
            else:
                if nn < m:
                    if nn == 0 or newdist > s[imax]:
                        imax = nn
                    E[nn] = list(z)
                    s[nn] = newdist
                    nn += 1
                else:
                    if newdist < s[imax]:
                        E[imax] = list(z)
                        s[imax] = newdist
                        imax = 0 if m == 1 or not s[0] < s[1] else 1
                    maxdist = s[imax]
                z[0] += step[0]
                y = zb[0] - z[0]
                step[0] = -step[0] - _sgn(step[0])
        else:
            if k == n - 1:
                break
            k += 1
            z[k] += step[k]
            y = zb[k] - z[k]
            step[k] = -step[k] - _sgn(step[k])
        c += 1
    if m > 1 and not s[0] < s[1]:
        s[0], s[1] = s[1], s[0]
        E[0], E[1] = E[1], E[0]
    return np.array(E), np.array(s), c


def lambda_np(a, Q, m=2):
    """(F [m][n], s [m], info, iterations) for float solution a with covariance Q (info: OK, NOT_PD, LOOP_LIMIT; F, s = 0 unless OK)."""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    if n < 1:
        return np.zeros((m, 0)), np.zeros(m), NO_INPUT, 0
    fac = ltdl(np.asarray(Q, dtype=np.float64))
    if fac is None:
        return np.zeros((m, n)), np.zeros(m), NOT_PD, 0
    red = reduction(fac[0], fac[1], a)
    if red is None:
        return np.zeros((m, n)), np.zeros(m), LOOP_LIMIT, 0
    L, d, Zi, z = red
    E, s, c = search(L, d, z, m)
    if c >= LOOPMAX:
        return np.zeros((m, n)), np.zeros(m), LOOP_LIMIT, c
    F = (Zi.T @ E.T).T            # F = Z^-T E: integer products, exact
    return F, s, OK, c


def brute_force(a, Q, m=2, max_points=400000):
    """The m best integer vectors by exhaustive enumeration of a box that must contain them.  Returns (F [m][n], s [m]),
    or None when the box holds more than max_points points."""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    Qi = np.linalg.inv(Q)
    Qi = 0.5 * (Qi + Qi.T)

    def dist(Z):
        e = a[None, :] - Z
        return np.einsum("ij,jk,ik->i", e, Qi, e)
    base = np.floor(a + 0.5)
    nb = base[None, :] + np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=n)))
    r2 = np.sort(dist(nb))[m - 1] * (1 + 1e-9)
    half = np.sqrt(r2 * np.diag(Q))
    lo, hi = np.ceil(a - half), np.floor(a + half)
    sizes = (hi - lo + 1).astype(np.int64)
    if np.prod(sizes.astype(float)) > max_points:
        return None
    grids = np.meshgrid(*[np.arange(lo[i], hi[i] + 1) for i in range(n)], indexing="ij")
    Z = np.stack([g.ravel() for g in grids], axis=1)
    ds = dist(Z)
    order = np.argsort(ds, kind="stable")[:m]
    return Z[order], ds[order]


def ratio_test(F, s, Qb, bf, thr=2.0):
    """SWFOptimization::LambdaSearch's acceptance test (R/swf/swf_lambda.cpp:208-253): returns (ratio [2], fixed)."""
    F1, F2 = F[0], F[1]
    same = np.abs(F1 - F2) < 1e-2
    e = (F1 - bf)[same]
    same_cost = float(e @ np.linalg.solve(Qb[np.ix_(same, same)], e)) if same.any() else 0.0
    s1 = s[1] - same_cost
    s0 = s[0] - same_cost
    if abs(s0) < 1e-3:
        s0 = 1e-3
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.array([s[1] / s[0], s1 / s0])
    return r, bool(s[0] <= 0 or r[0] >= thr or r[1] >= thr)
