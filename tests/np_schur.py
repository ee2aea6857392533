"""A longdouble referee for the assembly and elimination path, with one bracket per compared entry — TEST INFRASTRUCTURE.

Input: (r, J, n_e), r and J exactly as export_jacobian returned them (the device's BatchSolver.export_jacobian or the oracle's
oracle_binding.export_jacobian): their float64 bits ARE the problem, loss-corrected rows and composite-factor rows as they stand.
mu = 0 (ASSEMBLE_ELIMINATE_ONLY).  Everything that is compared is computed in np.longdouble, without LAPACK:

    H = J^T J,  g = J^T r,  diag = diag(H),
    S = H_ff - H_fe H_ee^-1 H_ef,  rhs = g_f - H_fe H_ee^-1 g_e          (e = the leading n_e coordinates, elimination group 0)

H_ee is block diagonal (landmarks, inverse depths, speed-bias cliques with whatever scalars join them): the blocks are the connected
components of the coupling pattern |J|^T |J| restricted to e, found here from the export itself, and each is factored on its own by a
longdouble Cholesky of its few rows.  Cost: the longdouble work is O(sum of rows x (columns touched)^2), not O(n^3).

Brackets (float64 is enough for them), the first-order componentwise bounds of the operation itself:

    B_H = |J|^T |J|,  B_g = |J|^T |r|
    X = |H_ee^-1 H_ef|,  x = |H_ee^-1 g_e|
    E = B_H, with |L_e| |L_e|^T added on the ee block (L_e = chol(H_ee), block by block)
    grad: B_g        diag: diag(B_H)
    S:    E_ff + E_fe X + X^T E_ef + X^T E_ee X
    rhs:  B_g,f + X^T B_g,e + E_fe x + X^T E_ee x

A quantity q of an implementation passes when |q - referee| <= M 2^-52 bracket in EVERY entry; where the bracket is exactly zero (a
structural zero: no row of J touches both coordinates, directly or through an eliminated block) the entry must be exactly zero.
The exported Cholesky factor is judged by its own backward error, |L L^T - S_dev| <= M_L 2^-52 |L| |L|^T, the product in longdouble
from the implementation's own L and S (factor_ratio).

The marginal prior (swf_batch_marginalize, Cholesky form) is the same operation one level on: A, b = the Schur complement of
(S, rhs) onto the trailing n_tail coordinates.  marginal() reduces the referee's own S and rhs in longdouble and propagates the
bracket by the same formula, E = bracket(S) with |L_m| |L_m|^T on the eliminated block; two derived terms state how the device forms
its result (csrc/swf_kernels3.h: A = L_nn L_nn^T from the factor of ALL of S, b = L_nn (L_nn^T y_n) with y = S^-1 rhs, no
regularisation and no threshold in this form): the product's own rounding |L_nn| |L_nn|^T for A, and |L_nn| |L_nn|^T |y_n| for b
(y_n is recovered by a back-substitution through L_nn^T and multiplied back)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def _ld(a):
    return np.asarray(a).astype(LD)


def chol_ld(A):
    """lower Cholesky factor of a (small) symmetric positive definite longdouble matrix; column by column, no LAPACK"""
    d = A.shape[0]
    L = np.zeros((d, d), LD)
    for j in range(d):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("eliminated block is not positive definite (pivot %d of %d)" % (j, d))
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def chol_solve_ld(L, B):
    """(L L^T)^-1 B, B with any number of columns, longdouble"""
    d = L.shape[0]
    Y = np.array(B, LD)
    for j in range(d):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(d - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


def gram_ld(r, J):
    """(H, g) = (J^T J, J^T r) in longdouble.  Consecutive rows with the same non-zero columns (the rows of one factor) are multiplied
    as one small dense block, so the cost follows the number of non-zeros and not n_res x n_loc^2."""
    n_res, n = J.shape
    H, g = np.zeros((n, n), LD), np.zeros(n, LD)
    nz = J != 0
    cut = np.flatnonzero(np.any(nz[1:] != nz[:-1], axis=1)) + 1 if n_res > 1 else np.zeros(0, np.int64)
    for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [n_res]])):
        c = np.flatnonzero(nz[a])
        if c.size == 0:
            continue
        Jb = _ld(J[a:b][:, c])
        H[np.ix_(c, c)] += Jb.T @ Jb
        g[c] += Jb.T @ _ld(r[a:b])
    return H, g


def components(P):
    """connected components of a symmetric boolean coupling pattern: list of index arrays, each ascending, ordered by first index"""
    n = P.shape[0]
    lab = -np.ones(n, np.int64)
    out = []
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = len(out)
        todo, comp = [s], [s]
        while todo:
            nb = np.flatnonzero(P[todo.pop()] & (lab < 0))
            lab[nb] = len(out)
            todo.extend(nb.tolist()); comp.extend(nb.tolist())
        out.append(np.array(sorted(comp), np.int64))
    return out


def _eliminate(H, g, E, Bg, n_e, blocks):
    """Schur complement of the leading n_e coordinates of (H, g) in longdouble, `blocks` = the index sets H_ee is block diagonal over,
    and its bracket from E (ee block still without the factor's term) and Bg.  Returns S, rhs, bracket of S, bracket of rhs."""
    n = H.shape[0]
    nf = n - n_e
    S, rhs = H[n_e:, n_e:].copy(), g[n_e:].copy()
    X, x = np.zeros((n_e, nf)), np.zeros(n_e)
    Eee = E[:n_e, :n_e].copy()
    for c in blocks:
        f = np.flatnonzero(E[c][:, n_e:].any(axis=0))            # the reduced coordinates this block couples to
        L = chol_ld(H[np.ix_(c, c)])
        Hcf = H[np.ix_(c, n_e + f)]
        Y = chol_solve_ld(L, np.column_stack([Hcf, g[c]]))
        S[np.ix_(f, f)] -= Hcf.T @ Y[:, :-1]
        rhs[f] -= Hcf.T @ Y[:, -1]
        X[np.ix_(c, f)] = np.abs(Y[:, :-1]).astype(np.float64)
        x[c] = np.abs(Y[:, -1]).astype(np.float64)
        La = np.abs(L).astype(np.float64)
        Eee[np.ix_(c, c)] += La @ La.T
    Efe = E[n_e:, :n_e]
    EX = Efe @ X
    bS = E[n_e:, n_e:] + EX + EX.T + X.T @ (Eee @ X)
    brhs = Bg[n_e:] + X.T @ Bg[:n_e] + Efe @ x + X.T @ (Eee @ x)
    return S, rhs, bS, brhs


def referee(r, J, n_e):
    """dict(g, diag, S, rhs: longdouble referees; b_g, b_diag, b_S, b_rhs: float64 brackets; n_blocks, max_block: the block
    structure found in H_ee) from the exported (r, J) and the number of eliminated coordinates."""
    r, J = np.asarray(r, np.float64), np.asarray(J, np.float64)
    n_e = int(n_e)
    H, g = gram_ld(r, J)
    Ja = np.abs(J)
    BH, Bg = Ja.T @ Ja, Ja.T @ np.abs(r)
    blocks = components(BH[:n_e, :n_e] > 0)
    S, rhs, bS, brhs = _eliminate(H, g, BH, Bg, n_e, blocks)
    S = (S + S.T) / 2                                            # (exactly symmetric already up to the order of two sums)
    assert not S[bS == 0].any() and not rhs[brhs == 0].any() and not g[Bg == 0].any()
    return dict(g=g, diag=np.diag(H).copy(), S=S, rhs=rhs, b_g=Bg, b_diag=np.diag(BH).copy(), b_S=bS, b_rhs=brhs,
                n_blocks=len(blocks), max_block=max([c.size for c in blocks], default=0))


def marginal(ref, n_tail):
    """dict(A, b: longdouble; b_A, b_b: brackets) — the referee's own (S, rhs) reduced onto the trailing n_tail coordinates, the bracket
    propagated by the same formula plus the two derived terms of the module docstring."""
    S, rhs, n_tail = ref["S"], ref["rhs"], int(n_tail)
    m = S.shape[0] - n_tail
    A, b, bA, bb = _eliminate(S, rhs, ref["b_S"], ref["b_rhs"], m, [np.arange(m)])
    A = (A + A.T) / 2
    Ln = chol_ld(A)
    y = np.abs(chol_solve_ld(Ln, b[:, None])[:, 0]).astype(np.float64)
    La = np.abs(Ln).astype(np.float64)
    LLt = La @ La.T
    return dict(A=A, b=b, b_A=bA + LLt, b_b=bb + LLt @ y)


def ratio(dev, ref, bracket):
    """|dev - ref| / (2^-52 bracket), entry by entry and over EVERY entry: 0 where the deviation is zero, inf where the bracket is zero
    and the value is not (a structural zero that is not one)."""
    d = np.abs(_ld(dev) - _ld(ref)).astype(np.float64)
    br = np.asarray(bracket, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, np.where(br > 0, d / (EPS * br), np.inf))


def factor_ratio(L, S):
    """backward error of an exported factor against the SAME implementation's S: |L L^T - S| / (2^-52 |L| |L|^T) entry by entry, the
    product in longdouble.  L must be lower triangular."""
    L, S = np.asarray(L, np.float64), np.asarray(S, np.float64)
    assert not np.triu(L, 1).any(), "the exported factor is not lower triangular"
    Ll = _ld(L)
    La = np.abs(L)
    return ratio(Ll @ Ll.T, S, La @ La.T)


def weakest(ref, bracket):
    """flat index of the entry with the smallest |value| among those with a non-zero bracket (where a loose rule is blind)"""
    v = np.abs(np.asarray(ref, np.float64)).ravel()
    v = np.where(np.asarray(bracket).ravel() > 0, v, np.inf)
    return int(np.argmin(v))
