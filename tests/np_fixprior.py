"""Referee of the fix-and-hold operator (swf_prior_fix_batch): the literal thing in numpy.

The second half of SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:254-343) stacks the window prior's rows with one
FixedIntegerFactor row istd ((x_c - tf_g) - v) per constraint, each on a hidden offset tf_g, and eliminates the tf columns the way
MarginalizationInfo::marginalize does: A = H_kk - H_km pinv(H_mm) H_mk, b = g_k - H_km pinv(H_mm) g_m with the eigen pseudo-inverse
(eigenvalues <= eps dropped).  `explicit` does exactly that; `closed_form` is the definition the kernel implements.  Both run in
float64 and in np.longdouble; the tests derive their tolerances from the distance between the two precisions.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -52


def _groups(rows):
    gs = []
    for (_, g, _) in rows:
        if g not in gs:
            gs.append(g)
    return gs


def closed_form(J, r, rows, istd, dtype=np.float64):
    """A' and b' by the closed form: per group with members c_1..c_k, A'[c_a, c_b] += istd^2 (delta_ab - 1/k),
    b'[c_a] -= istd^2 (v_a - mean(v))."""
    J = np.asarray(J, dtype); r = np.asarray(r, dtype)
    w2 = dtype(istd) * dtype(istd)
    A = J.T @ J
    b = J.T @ r
    for g in _groups(rows):
        mem = [(c, dtype(v)) for (c, gg, v) in rows if gg == g]
        k = dtype(len(mem))
        mean = sum(v for _, v in mem) / k
        for a, (ca, va) in enumerate(mem):
            for bb, (cb, _) in enumerate(mem):
                A[ca, cb] += w2 * ((dtype(1) if a == bb else dtype(0)) - dtype(1) / k)
            b[ca] -= w2 * (va - mean)
    return A, b


def explicit(J, r, rows, istd, dtype=np.float64, eps=1e-8):
    """A' and b' by explicit elimination: prior rows plus fixed-integer rows with tf columns, the tf block pseudo-inverted through its
    eigen-decomposition as MarginalizationInfo::marginalize does.  The tf are mutually independent, so that block is diagonal: in
    float64 numpy's eigh is applied to it literally; in longdouble (no eigh) its eigen-decomposition is read off the diagonal."""
    J = np.asarray(J, dtype); r = np.asarray(r, dtype)
    n = J.shape[0]
    gs = _groups(rows)
    G, m = len(gs), len(rows)
    Js = np.zeros((n + m, G + n), dtype)          # columns: tf (marginalised, first, as marginalize orders them) | kept
    rs = np.zeros(n + m, dtype)
    Js[:n, G:] = J; rs[:n] = r
    for i, (c, g, v) in enumerate(rows):
        Js[n + i, G + c] = dtype(istd); Js[n + i, gs.index(g)] = -dtype(istd)
        rs[n + i] = dtype(istd) * (dtype(0) - dtype(0) - dtype(v))      # x_c = tf = 0 at the linearisation point
    H = Js.T @ Js
    g_ = Js.T @ rs
    Hmm = 0.5 * (H[:G, :G] + H[:G, :G].T)
    if dtype is np.float64:
        lam, V = np.linalg.eigh(Hmm)
        inv = np.where(lam > eps, 1.0 / np.where(lam > eps, lam, 1.0), 0.0)
        Hmm_inv = V @ np.diag(inv) @ V.T
    else:
        assert np.all(Hmm - np.diag(np.diag(Hmm)) == 0), "the tf block is diagonal"
        d = np.diag(Hmm)
        Hmm_inv = np.diag(np.where(d > eps, dtype(1) / np.where(d > eps, d, dtype(1)), dtype(0)))
    Hkm = H[G:, :G]
    A = H[G:, G:] - Hkm @ Hmm_inv @ Hkm.T
    b = g_[G:] - Hkm @ Hmm_inv @ g_[:G]
    return A, b


def eigen_root(A, b, eps=1e-8):
    """setmarginalizeinfo's square root in float64: J = sqrt(lam+) V^T (ascending), r0 = lam+^-1/2 V^T b, eigenvalues <= eps dropped."""
    A = np.asarray(A, np.float64)
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = lam > eps
    s = np.sqrt(np.where(keep, lam, 0.0))
    si = np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)
    Jn = (V * s).T
    r0 = si * (V.T @ np.asarray(b, np.float64))
    return Jn, r0, lam, int(keep.sum())


def chol_root(A, b):
    """The Cholesky form in float64: J = L^T, r0 = L^-1 b, eig = diag(L)^2."""
    L = np.linalg.cholesky(np.asarray(A, np.float64))
    r0 = np.linalg.solve(L, np.asarray(b, np.float64))
    return L.T.copy(), r0, np.diag(L) ** 2, A.shape[0]


def chol_ld(A):
    """Lower Cholesky factor in longdouble (no LAPACK there): right-looking, a column at a time."""
    A = np.array(A, LD)
    n = A.shape[0]
    for k in range(n):
        A[k, k] = np.sqrt(A[k, k])
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return np.tril(A)


def eig_ld(A):
    """Eigenvalues (ascending) and orthonormal eigenvectors of a symmetric longdouble matrix to longdouble accuracy: float64 eigh,
    the vectors re-orthonormalised in longdouble (modified Gram-Schmidt, twice), eigenvalues as longdouble Rayleigh quotients — the
    quotient's error is quadratic in the vector's."""
    A = np.asarray(A, LD)
    _, V = np.linalg.eigh(np.asarray(0.5 * (A + A.T), np.float64))
    V = np.array(V, LD)
    n = A.shape[0]
    for _ in range(2):
        for k in range(n):
            if k:
                V[:, k] -= V[:, :k] @ (V[:, :k].T @ V[:, k])
            V[:, k] /= np.sqrt(V[:, k] @ V[:, k])
    lam = np.einsum("ik,ik->k", V, A @ V)
    o = np.argsort(lam, kind="stable")
    return lam[o], V[:, o]


def brackets(J, r, rows, istd, A_ld, b_ld, lam_ld, eps):
    """The norm brackets of DESIGN.md 3k (float64 numbers): a compared quantity's bound is M * 2^-52 * its bracket.
      A    n max_c |J[:, c]|^2 + istd^2          (a length-n dot product of two columns, plus the one update of an entry)
      b    n max_c |J[:, c]| |r| + istd^2 (1 + max |v|)
      JtJ  n |A'|_2                              (a backward-stable root reproduces A' to n u |A'|_2)
      Jtr  n |b'| sqrt(|A'|_2 / lam_min kept)    (b' passes through a root of that condition and back)
      eig  n |A'|_2                              (Weyl: an eigenvalue moves by at most the perturbation's norm)"""
    J = np.asarray(J, np.float64); r = np.asarray(r, np.float64)
    n = J.shape[0]
    cmax = float(np.sqrt((J * J).sum(0)).max())
    vmax = max([abs(float(v)) for (_, _, v) in rows] + [0.0])
    lmax = float(lam_ld[-1])
    kept = [float(x) for x in lam_ld if x > eps]
    return dict(A=n * cmax * cmax + istd * istd,
                b=n * cmax * float(np.linalg.norm(r)) + istd * istd * (1.0 + vmax),
                JtJ=n * lmax, eig=n * lmax,
                Jtr=n * float(np.linalg.norm(np.asarray(b_ld, np.float64))) * float(np.sqrt(lmax / min(kept))) if kept else 1.0)


def deviations(out, ref, form):
    """Deviation of one result dict(A, b, J, r0, eig, rank) from the longdouble reference `ref` (reference()), per compared quantity,
    in units of 2^-52 * bracket.  Nothing compares rows of J: the eigen form leaves eigenvector signs undefined."""
    br = ref["br"]
    A, b = np.asarray(out["A"], LD), np.asarray(out["b"], LD)
    Jn, r0 = np.asarray(out["J"], LD), np.asarray(out["r0"], LD)
    d = dict(A=float(np.abs(A - ref["A"]).max()) / (U * br["A"]),
             b=float(np.abs(b - ref["b"]).max()) / (U * br["b"]),
             JtJ=float(np.abs(Jn.T @ Jn - ref["A_kept"]).max()) / (U * br["JtJ"]),
             Jtr=float(np.abs(Jn.T @ r0 - ref["b_kept"]).max()) / (U * br["Jtr"]))
    e_ref = ref["lam"] if form == 0 else ref["chol_d2"]
    d["eig"] = float(np.abs(np.asarray(out["eig"], LD) - e_ref).max()) / (U * br["eig"]) if e_ref is not None else 0.0
    return d


def reference(J, r, rows, istd, eps=1e-8):
    """The longdouble reference of one problem: A', b' (explicit elimination), eigenvalues, rank, A' and b' restricted to the kept range
    (the dropped directions carry no information by definition: eigenvalues <= eps), the squared Cholesky diagonal where A' is definite."""
    A, b = explicit(J, r, rows, istd, LD, eps)
    lam, V = eig_ld(A)
    keep = lam > eps
    Vk = V[:, keep]
    ref = dict(A=A, b=b, lam=lam, rank=int(keep.sum()), A_kept=(Vk * lam[keep]) @ Vk.T, b_kept=Vk @ (Vk.T @ b))
    ref["chol_d2"] = np.diag(chol_ld(A)) ** 2 if bool(np.all(keep)) else None
    ref["br"] = brackets(J, r, rows, istd, A, b, lam, eps)
    return ref


def float64_referees(J, r, rows, istd, form, eps=1e-8):
    """The float64 referee in its two legitimate orders (closed form; explicit elimination), each with numpy's own root."""
    outs = []
    for fn in (closed_form, explicit):
        A, b = fn(J, r, rows, istd, np.float64)
        Jn, r0, eig, rank = eigen_root(A, b, eps) if form == 0 else chol_root(A, b)
        outs.append(dict(A=A, b=b, J=Jn, r0=r0, eig=eig, rank=rank))
    return outs


def prior_dx(x, x0, sizes):
    """dx of MarginalizationFactor::Evaluate over the kept blocks (global sizes; 7 = pose: p - p0, +-2 vec(q0^-1 q))."""
    out, o = [], 0
    for s in sizes:
        a, a0 = np.asarray(x[o:o + s], np.float64), np.asarray(x0[o:o + s], np.float64)
        if s != 7:
            out.append(a - a0)
        else:
            q0, q = a0[3:], a[3:]
            qi = np.array([-q0[0], -q0[1], -q0[2], q0[3]]) / (q0 @ q0)
            ax, ay, az, aw = qi; bx, by, bz, bw = q
            dq = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                           aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
            out.append(np.concatenate([a[:3] - a0[:3], (2.0 if dq[3] >= 0 else -2.0) * dq[:3]]))
        o += s
    return np.concatenate(out)
