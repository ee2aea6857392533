"""A longdouble referee for the SQUARE ROOT of the marginal prior, with one bracket per compared entry — TEST INFRASTRUCTURE.

swf_batch_marginalize (csrc/swf_kernels3.h, csrc/swf_rootdev.h) and the fix-and-hold operator (csrc/swf_fixprior.hip) turn a marginal
(A, b) into the prior the next window consumes: J, r0, eig, rank with J^T J = A, J^T r0 = b — the eigen form (rows = sqrt(lambda_k) v_k^T
by ascending eigenvalue, eigenvalues <= thr dropped: null row, null r0) or the Cholesky form (J upper triangular).  The input of every
rule here is the implementation's own A, b, J, r0, eig, bit for bit (A and b are judged by tests/np_schur.py); plain numpy, longdouble
where marked, nothing imported from the package.

Why componentwise.  The device rotates the columns of G (G G^T = A) from the right, which is backward stable ROW BY ROW; row i of G has
norm sqrt(A_ii), hence |J^T J - A|_ij <~ c n 2^-52 sqrt(A_ii A_jj), for the Cholesky factor and the diagonally pivoted one alike.  A rule
relative to max|A| (1e-12 max|A| in tests/test_gpu_parity.py) allows 1e-2 absolute in every entry at max|A| = 1e10, where the tails
carry informations down to 1e-7: it does not see the weakest row of J deleted.

The rules (quantities): name -> (value, referee, bracket, cut); a value passes when |value - referee| <= cut + M 2^-52 bracket in EVERY
entry, and must equal the referee exactly where bracket and cut are zero.  Products in longdouble.

    JtJ    J^T J (both forms)       A at full rank, else A - sum_{lambda <= thr} lambda v v^T (jacobi_ld)      n sqrt(A_ii A_jj)
    JJt    J J^T off the diagonal   0                                                     (eigen form)       n sqrt(eig_k eig_l)
    eig    eig_k                    the longdouble J_k . J_k of a kept row                                     eig_k
    lam    eig_k                    lambda_k of jacobi_ld(A), kept eigenvalues (n <= 141)                       n (sum_i sqrt(A_ii) |v_ki|)^2
    r0     r0_k (eigen form)        (J_k . b) / (J_k . J_k); exactly 0 on a dropped row                        n (|J_k| . |b|) / eig_k
    Jtr    J^T r0 at full rank      b                       eigen: n |J|^T Lambda^-1 |J| |b|;  Cholesky: n |J|^T |r0|
    chd    eig_k (Cholesky form)    diag(J)_k^2                                                                eig_k
    exact: rank = #(lambda > thr); eig ascending; dropped rows null with null r0; J upper triangular in the Cholesky form.

`lam`'s bracket is the first-order image of JtJ's: d lambda_k = v_k^T dA v_k.  A dropped eigenvalue is held by the rank and by its null
row, not by `lam` (what the implementation reports there is whatever its factorisation left of a direction the specification discards).
The cut is what the specification grants a factorisation that stops early, on rank-deficient inputs only (declared_cut); it is absolute,
never multiplied by M 2^-52."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
THR = 1e-8            # the reference's eigenvalue threshold (absolute)
JACOBI_MAX_N = 141


def _ld(a):
    return np.asarray(a).astype(LD)


# ---------------------------------------------------------------------------------------------------------------- the referee
def chol_factor_ld(A):
    """G (n x n, longdouble) with G G^T = A for the symmetric float64 matrix A, its bits taken as exact: the lower Cholesky factor; on a
    semi-definite input the diagonally pivoted one (rows in the original order, columns in pivot order), which stops at pivots
    <= 2^-60 of the index's own original diagonal entry — the remaining columns are zero.  Returns (G, number of columns)."""
    A = _ld(A)
    n = A.shape[0]
    d0 = np.diag(A).copy()
    cut = d0 * LD(2.0) ** -60
    G = np.zeros((n, n), LD)
    ok = True
    for j in range(n):                                  # unpivoted first
        v = A[j:, j] - G[j:, :j] @ G[j, :j]
        if not v[0] > cut[j]:
            ok = False
            break
        G[j, j] = np.sqrt(v[0])
        G[j + 1:, j] = v[1:] / G[j, j]
    if ok:
        return G, n
    G[:] = 0
    d = d0.copy()
    live = d > np.maximum(cut, 0)
    r = 0
    while live.any():
        p = int(np.argmax(np.where(live, d, -np.inf)))
        v = A[:, p] - G[:, :r] @ G[p, :r]
        piv = v[p]
        if not piv > cut[p]:
            live[p] = False
            continue
        v = np.where(live, v, 0) / np.sqrt(piv)
        G[:, r] = v
        d = d - v * v
        live[p] = False
        live &= d > np.maximum(cut, 0)
        r += 1
    return G, r


def _round_robin(ne):
    """the n - 1 steps of the circle method over ne (even) players: arrays (p, q), p < q, every pair exactly once"""
    out = []
    for st in range(ne - 1):
        pr = np.arange(1, ne // 2)
        p = np.concatenate([[ne - 1], (st + pr) % (ne - 1)])
        q = np.concatenate([[st], (st - pr) % (ne - 1)])
        out.append((np.minimum(p, q), np.maximum(p, q)))
    return out


def jacobi_ld(A):
    """(lambda ascending, V with orthonormal columns) of the symmetric float64 matrix A to longdouble accuracy RELATIVE TO EACH EIGENVALUE
    as far as A's scaling allows: a one-sided cyclic Jacobi in longdouble on chol_factor_ld(A) (columns rotated from the right, the
    round-robin order: every pair once per sweep, the disjoint pairs of a step rotated at once), until every pair's cos^2 <= 1e-36.
    Eigenvalues of the directions the factor dropped are exactly 0, their vectors an orthonormal completion."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    assert n <= JACOBI_MAX_N and np.array_equal(A, A.T)
    G, r = chol_factor_ld(A)
    C = np.ascontiguousarray(G.T[:r])                   # row c = column c of G
    if r > 1:
        steps = _round_robin((r + 1) & ~1)
        for sweep in range(60):
            worst = LD(0)
            for p, q in steps:
                k = q < r
                p, q = p[k], q[k]
                a, b = C[p], C[q]
                al, be, ga = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
                c2 = ga * ga / (al * be)
                worst = max(worst, c2.max())
                go = c2 > LD(1e-36)
                if not go.any():
                    continue
                gs = np.where(go, ga, 1)
                zeta = (be - al) / (2 * gs)
                t = np.where(zeta >= 0, 1, -1) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                c, s = np.where(go, c, 1)[:, None], np.where(go, c * t, 0)[:, None]
                C[p], C[q] = c * a - s * b, s * a + c * b
            if worst <= LD(1e-36):
                break
        else:
            raise RuntimeError("jacobi_ld did not converge")
    lam = np.zeros(n, LD)
    V = np.zeros((n, n), LD)
    lam[:r] = (C * C).sum(1)
    V[:, :r] = (C / np.sqrt(lam[:r])[:, None]).T
    k = r
    for e in range(n):                                  # (the completion: unit vectors, orthogonalised twice)
        if k == n:
            break
        v = np.zeros(n, LD); v[e] = 1
        for _ in range(2):
            v -= V[:, :k] @ (V[:, :k].T @ v)
        nv = np.sqrt(v @ v)
        if nv > 0.5 ** 20:
            V[:, k] = v / nv
            k += 1
    assert k == n
    o = np.argsort(lam, kind="stable")
    return lam[o], V[:, o]


def referee(A, thr=THR):
    """dict(lam, V, rank, tie) of jacobi_ld(A): rank = #(lambda > thr); tie = some eigenvalue lies in [thr / 4, 4 thr] (a case must not)"""
    lam, V = jacobi_ld(A)
    return dict(lam=lam, V=V, rank=int((lam > thr).sum()), tie=bool(np.any((lam >= thr / 4) & (lam <= 4 * thr))))


# ---------------------------------------------------------------------------------------------------------------- float64 routes
def pivoted_chol64(A, eps=THR, precond_cut="now"):
    """The device's preconditioner restated (csrc/swf_rootdev.h, d_pivoted_chol with drop_abs = eps / (16 n)): diagonally pivoted
    Cholesky of A in float64, G[:, r] = v_r with sum_r v_r v_r^T = A up to the pivots it drops; it stops at a largest running diagonal
    entry <= min(1e-14 d0, eps / (16 n)), d0 the largest diagonal entry.  precond_cut = "r4": the historical rule, 1e-14 d0 alone."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    d = A.diagonal().copy()
    d0 = d.max()
    thr = 1e-14 * d0 if precond_cut == "r4" else min(1e-14 * d0, eps / (16.0 * n))
    assert precond_cut in ("r4", "now")
    G = np.zeros((n, n))
    live = np.ones(n, bool)
    for r in range(n):
        p = int(np.argmax(np.where(live, d, -np.inf)))
        if not (live[p] and d[p] > thr and d[p] > 0):
            break
        v = A[:, p] - G[:, :r] @ G[p, :r]
        v = np.where(live, v, 0.0) / np.sqrt(d[p])
        G[:, r] = v
        d = d - v * v
        live[p] = False
    return G


def hestenes64(G, order):
    """One-sided Jacobi in float64 on the columns of G (n x n, G G^T = A), returned rotated (G W, columns mutually orthogonal).
    order = "cyclic": the row-cyclic order (p < q in lexicographic order) until a sweep rotates nothing; the textbook statement.
    order = "device": d_jacobi_sweeps restated — the round-robin pairing of the circle method (a bye for odd n), the disjoint pairs of a
    step at once, its two rotation tests (1e-30, 1e-140), at most 40 sweeps, and its early exit n^2 max cos^2 max sin^2 <= 1e-30."""
    C = np.ascontiguousarray(np.asarray(G, np.float64).T)      # row c = column c
    n = C.shape[0]

    def rot(a, b):
        al, be, ga = (a * a).sum(-1), (b * b).sum(-1), (a * b).sum(-1)
        go = (ga * ga > 1e-30 * (al * be)) & (np.abs(ga) > 1e-140 * (al + be))
        gs = np.where(go, ga, 1.0)
        zeta = (be - al) * (0.5 / gs)
        t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
        c = 1.0 / np.sqrt(1.0 + t * t)
        with np.errstate(divide="ignore", invalid="ignore"):
            c2 = np.where(go, ga * ga / (al * be), 0.0)
        return go, np.where(go, c, 1.0), np.where(go, c * t, 0.0), c2

    if order == "cyclic":
        for sweep in range(60):
            nrot = 0
            for p in range(n - 1):
                for q in range(p + 1, n):
                    a, b = C[p], C[q]
                    go, c, s, _ = rot(a, b)
                    if go:
                        C[p], C[q] = c * a - s * b, s * a + c * b
                        nrot += 1
            if nrot == 0:
                break
        return C.T.copy()
    assert order == "device"
    steps = _round_robin((n + 1) & ~1)
    for sweep in range(40):
        nrot, mc2, ms2 = 0, 0.0, 0.0
        for p, q in steps:
            k = q < n
            p, q = p[k], q[k]
            a, b = C[p], C[q]
            go, c, s, c2 = rot(a, b)
            nrot += int(go.sum())
            if go.any():
                mc2, ms2 = max(mc2, float(c2.max())), max(ms2, float((s * s).max()))
                C[p], C[q] = c[:, None] * a - s[:, None] * b, s[:, None] * a + c[:, None] * b
        if nrot == 0 or float(n) * float(n) * mc2 * ms2 <= 1e-30:
            break
    return C.T.copy()


def eigen_root_out64(G, b, eps=THR):
    """d_eigen_root_out restated: eigenvalues = squared column norms, J = the columns as rows by ascending eigenvalue (ties: the lower
    column first), r0 = (column . b) / lambda, eigenvalues <= eps dropped (null row, null r0; eig keeps the norm).  dict(J, r0, eig, rank)."""
    G = np.asarray(G, np.float64)
    lam = (G * G).sum(0)
    o = np.argsort(lam, kind="stable")
    keep = lam[o] > eps
    J = np.where(keep[:, None], G.T[o], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = np.where(keep, (G.T[o] @ np.asarray(b, np.float64)) / lam[o], 0.0)
    return dict(J=J, r0=r0, eig=lam[o].copy(), rank=int(keep.sum()))


def eigen_route64(A, b, route, eps=THR, precond_cut="now"):
    """route "cyclic": hestenes64 on the unpivoted Cholesky factor of A (L_nn); route "device": on pivoted_chol64(A)"""
    G = np.linalg.cholesky(A) if route == "cyclic" else pivoted_chol64(A, eps, precond_cut)
    out = eigen_root_out64(hestenes64(G, route), b, eps)
    out.update(A=np.asarray(A, np.float64), b=np.asarray(b, np.float64))
    return out


def chol_route64(A, b):
    """the Cholesky form in float64: J = L^T, r0 = L^-1 b, eig = diag(L)^2"""
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(A)
    return dict(A=np.asarray(A, np.float64), b=np.asarray(b, np.float64), J=L.T.copy(), r0=solve_triangular(L, b, lower=True),
                eig=L.diagonal() ** 2, rank=A.shape[0])


def marginal64(S, rhs, n):
    """(A, b) onto the trailing n coordinates in float64 the way the device forms them (csrc/swf_kernels3.h): S = L L^T,
    A = L_nn L_nn^T, b = L_nn (L_nn^T y_n), y = S^-1 rhs"""
    from scipy.linalg import solve_triangular
    m = S.shape[0] - n
    L = np.linalg.cholesky(S)
    y = solve_triangular(L, solve_triangular(L, rhs, lower=True), lower=True, trans=1)
    Ln = L[m:, m:]
    A = Ln @ Ln.T
    return 0.5 * (A + A.T), Ln @ (Ln.T @ y[m:])


# ---------------------------------------------------------------------------------------------------------------- the rules
def declared_cut(A, n_dropped, path, eps=THR):
    """What the specification grants a factorisation that stops early, per entry of J^T J, on a rank-deficient input (n_dropped > 0), as
    csrc/swf_rootdev.h states its stopping rules.  path "healthy": (n - r) min(1e-14 d0, eps / (16 n)), the largest pivot left behind
    bounds every entry of the remainder.  path "rescue": an index is dropped at a running diagonal <= 1e-14 of its OWN A_ii, the
    remainder is positive semi-definite: (n - r) 1e-14 sqrt(A_ii A_jj)."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    if n_dropped <= 0:
        return np.zeros((n, n))
    d = np.abs(A.diagonal())
    if path == "healthy":
        return np.full((n, n), n_dropped * min(1e-14 * d.max(), eps / (16.0 * n)))
    assert path == "rescue"
    return n_dropped * 1e-14 * np.sqrt(np.outer(d, d))


def quantities(out, form, ref=None, thr=THR, path="healthy"):
    """name -> (value, referee, bracket, cut) of one implementation's dict(A, b, J, r0, eig, rank); form 0 = eigen, 1 = Cholesky;
    ref = referee(A) or None (n > 141: the product rules only, and the prior must then be of full rank)."""
    A, b = np.asarray(out["A"], np.float64), np.asarray(out["b"], np.float64)
    J, r0, eig = np.asarray(out["J"], np.float64), np.asarray(out["r0"], np.float64), np.asarray(out["eig"], np.float64)
    n = A.shape[0]
    Jl, bl = _ld(J), _ld(b)
    dA = np.sqrt(np.abs(A.diagonal()))
    q = {}
    rank = ref["rank"] if ref is not None else n
    Aref, cut = _ld(A), 0.0
    if rank < n:
        for k in np.flatnonzero(np.asarray(ref["lam"] <= thr)):
            Aref = Aref - ref["lam"][k] * np.outer(ref["V"][:, k], ref["V"][:, k])
        cut = declared_cut(A, n - rank, path, thr)
    q["JtJ"] = (Jl.T @ Jl, Aref, n * np.outer(dA, dA), cut)
    if form == 1:
        q["chd"] = (eig, _ld(J.diagonal()) ** 2, eig.copy(), 0.0)
        q["Jtr"] = (Jl.T @ _ld(r0), bl, n * (np.abs(J).T @ np.abs(r0)), 0.0)
        return q
    keep = eig > thr
    se = np.sqrt(eig)
    off = ~np.eye(n, dtype=bool)
    q["JJt"] = (np.where(off, Jl @ Jl.T, 0), np.zeros((n, n), LD), np.where(off, n * np.outer(se, se), 0.0), 0.0)
    rn = (Jl * Jl).sum(1)
    q["eig"] = (np.where(keep, eig, 0.0), np.where(keep, rn, 0), np.where(keep, eig, 0.0), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q["r0"] = (r0, np.where(keep, (Jl @ bl) / np.where(keep, rn, 1), 0), np.where(keep, n * (np.abs(J) @ np.abs(b)) / eig, 0.0), 0.0)
        if rank == n:
            Ja = np.abs(J)
            q["Jtr"] = (Jl.T @ _ld(r0), bl, n * (Ja.T @ ((Ja @ np.abs(b)) / eig)), 0.0)
    if ref is not None:
        kl = np.asarray(ref["lam"] > thr)
        img = n * (np.abs(np.asarray(ref["V"], np.float64)).T @ dA) ** 2
        q["lam"] = (np.where(kl, eig, 0.0), np.where(kl, ref["lam"], 0), np.where(kl, img, 0.0), 0.0)
    return q


def ratio(value, referee_, bracket, cut=0.0):
    """max(|value - referee| - cut, 0) / (2^-52 bracket), entry by entry and over EVERY entry: 0 where nothing is left, inf where the
    bracket is zero and something is."""
    d = np.maximum(np.abs(_ld(value) - _ld(referee_)).astype(np.float64) - cut, 0.0)
    br = np.broadcast_to(np.asarray(bracket, np.float64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, np.where(br > 0, d / (EPS * br), np.inf))


def ratios(q):
    return {k: ratio(*v) for k, v in q.items()}


def exact_rules(out, form, ref=None, thr=THR):
    """list of the exact rules that do NOT hold (empty = all hold)"""
    J, r0, eig = np.asarray(out["J"]), np.asarray(out["r0"]), np.asarray(out["eig"])
    n = J.shape[0]
    bad = []
    if out["rank"] != (ref["rank"] if ref is not None else n):
        bad.append("rank %d, referee %d" % (out["rank"], ref["rank"] if ref is not None else n))
    if form == 1:
        if np.tril(J, -1).any():
            bad.append("J is not upper triangular")
        return bad
    if not np.all(np.diff(eig) >= 0):
        bad.append("eig is not ascending")
    drop = eig <= thr
    if int((~drop).sum()) != out["rank"]:
        bad.append("rank is not the number of eig > thr")
    if J[drop].any() or r0[drop].any():
        bad.append("a dropped row is not null")
    return bad


def weakest(ref, bracket):
    """flat index of the entry with the smallest |referee| among those with a non-zero bracket (where a loose rule is blind)"""
    v = np.abs(np.asarray(ref, np.float64)).ravel()
    v = np.where(np.broadcast_to(np.asarray(bracket, np.float64), np.shape(ref)).ravel() > 0, v, np.inf)
    return int(np.argmin(v))


def old_rule(out):
    """the one-number-per-array rule of tests/test_gpu_parity.py: (|J^T J - A|max / max|A|, |J^T r0 - b|max / max|b|); it passes at
    (<= 1e-12, <= 1e-10)"""
    J = np.asarray(out["J"], np.float64)
    return (float(np.abs(J.T @ J - out["A"]).max() / np.abs(out["A"]).max()),
            float(np.abs(J.T @ np.asarray(out["r0"], np.float64) - out["b"]).max() / np.abs(out["b"]).max()))
