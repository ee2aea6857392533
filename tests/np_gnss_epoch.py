"""numpy referee of the single-epoch GNSS solve (swf_gnss_epoch_solve_batch), in two forms and two precisions.

solve()        the structured definition of include/swf_solver.h: rows with a free ambiguity dropped, the clocks eliminated as scalars,
               Cholesky on what is left of [pos, vel], the ambiguities absorbed after the last iteration.
solve_dense()  a second opinion that knows none of that: Gauss-Newton by least squares (Householder QR) on the full whitened Jacobian of
               every row, the free ambiguities as ordinary columns ordered first, then the clocks, then [pos, vel].  The trailing block
               of its R factor is the Cholesky factor of the reduced system, so it takes the rank decision from its own numbers.
Both run in float64 or in longdouble (dtype=), and solve() takes `order`, a permutation of the records in which the sums run.
TEST INFRASTRUCTURE."""
import numpy as np

CLIGHT, OMGE = 299792458.0, 7.2921151467E-5
DOUBLES, CLOCKS, NMAX = 10, 13, 512
RTK_PHASE, RTK_CODE, SPP_CODE, SPP_PHASE, DOPPLER = 0, 1, 2, 3, 4
AMB_FREE = 1
FREE_POS, FREE_VEL = 1, 2
CONVERGED, MAX_ITER, RANK_DEFICIENT = 0, 1, 2
SEED = dict(mode=0, max_iter=2)                                # GnssPreprocess, R/swf/swf_gnss.cpp:534-575
FIRST_FIX = dict(mode=FREE_POS | FREE_VEL, max_iter=20)        # GnssProcess, :203-215


def evaluate(dat, rec, xg, vel, clock, T=np.float64):
    """r (weighted, with the records' own N), J [n][6] on [pos, vel], nfree (the N that zeroes a phase row), bracket |xg|+|sat|+|obs|+|clk|."""
    d = np.asarray(dat).astype(T).reshape(-1, DOUBLES)
    kind, slot = rec[:, 0], rec[:, 1]
    n = d.shape[0]
    sat, sv, obs, w, lam, N = d[:, 0:3], d[:, 3:6], d[:, 6], d[:, 7], d[:, 8], d[:, 9]
    clk = np.asarray(clock).astype(T)[slot]
    e = xg[None, :] - sat
    rr = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    e = e / rr[:, None]
    rho = rr + T(OMGE) * (sat[:, 0] * xg[1] - sat[:, 1] * xg[0]) / T(CLIGHT)
    rtk = (kind == RTK_PHASE) | (kind == RTK_CODE)
    phase = (kind == RTK_PHASE) | (kind == SPP_PHASE)
    a = np.where(rtk, rho, rho + clk)
    b = a.copy()
    a = np.where(phase, a - N * lam, a)
    a = a - obs; b = b - obs
    a = np.where(rtk, a + clk, a); b = np.where(rtk, b + clk, b)
    ev = vel[None, :] - sv
    ee = ev[:, 0] * e[:, 0] + ev[:, 1] * e[:, 1] + ev[:, 2] * e[:, 2]
    rate = ee + T(OMGE) / T(CLIGHT) * (sv[:, 1] * xg[0] + sat[:, 1] * vel[0] - sv[:, 0] * xg[1] - sat[:, 0] * vel[1])
    dop = kind == DOPPLER
    r = np.where(dop, w * (rate + clk + obs), w * a)
    J = np.zeros((n, 6), T)
    J[:, 0:3] = np.where(dop[:, None], w[:, None] * (ev - ee[:, None] * e) / rr[:, None], w[:, None] * e)
    J[:, 3:6] = np.where(dop[:, None], w[:, None] * e, T(0))
    nfree = np.where(phase, b / lam, N)
    norm = lambda v: np.sqrt((v * v).sum(-1))
    bracket = norm(xg) + norm(sat) + np.abs(obs) + np.abs(clk)
    return r, J, nfree, bracket


def _finish(out, dat, rec, base, pos, vel, clock, T):
    free = (rec[:, 2] & AMB_FREE) != 0
    r, _J, nfree, br = evaluate(dat, rec, pos + base, vel, clock, T)
    out["r"] = np.where(free, T(0), r)
    out["N"] = np.where(free, nfree, np.asarray(dat).astype(T).reshape(-1, DOUBLES)[:, 9])
    out["cost"] = T(0.5) * (out["r"] * out["r"]).sum()
    out["pos"], out["vel"], out["clock"] = pos, vel, clock
    out["bracket"] = br
    return out


def solve(pos, vel, base, clock, mode, clk_const, dat, rec, max_iter=20, step_tol=1e-4, eps_rank=1e-8, dtype=np.float64, order=None):
    """One epoch by the structured definition.  Returns dict(pos, vel, clock, N, r, cost, iters, status, clk_rows, info [6][6]) plus the
    diagnostics steps (largest |entry| of every step taken), pivot (smallest relative pivot met; inf without a [pos, vel] unknown) and
    bracket [n]."""
    T = dtype
    dat = np.asarray(dat, np.float64).reshape(-1, DOUBLES); rec = np.asarray(rec).reshape(-1, 4)
    if order is not None:
        inv = np.argsort(order)
        out = solve(pos, vel, base, clock, mode, clk_const, dat[order], rec[order], max_iter, step_tol, eps_rank, dtype)
        for k in ("N", "r", "bracket"):
            out[k] = out[k][inv]
        return out
    pos0, vel0, base, clock0 = (np.asarray(v).astype(T) for v in (pos, vel, base, clock))
    free = (rec[:, 2] & AMB_FREE) != 0
    inc = ~free
    slot = rec[:, 1]
    w = dat[:, 7]
    clk_rows = np.array([int((inc & (w > 0) & (slot == s)).sum()) for s in range(CLOCKS)], np.int32)
    act_c = [s for s in range(CLOCKS) if not (clk_const >> s) & 1 and clk_rows[s] > 0]
    act = np.array([bool(mode & FREE_POS)] * 3 + [bool(mode & FREE_VEL)] * 3)
    pos, vel, clock = pos0.copy(), vel0.copy(), clock0.copy()
    out = dict(clk_rows=clk_rows, info=np.zeros((6, 6), T), steps=[], pivot=np.inf)
    status, it = MAX_ITER, 0
    while it < max_iter:
        it += 1
        r, J, _nf, _br = evaluate(dat, rec, pos + base, vel, clock, T)
        r = np.where(inc, r, T(0)); jc = np.where(inc, dat[:, 7].astype(T), T(0))
        J = np.where(inc[:, None] & act[None, :], J, T(0))
        step_c = np.zeros(CLOCKS, T)
        dx = np.zeros(6, T)
        if act.any():
            S = J.T @ J
            rhs = -(J.T @ r)
            hd = np.diag(S).copy()
            cl = {}
            for s in act_c:
                m = slot == s
                hcc, gc, hpc = (jc[m] * jc[m]).sum(), (jc[m] * r[m]).sum(), (J[m] * jc[m, None]).sum(0)
                u = hpc / hcc
                S = S - np.outer(u, hpc); rhs = rhs + u * gc
                cl[s] = (hcc, gc, hpc)
            out["info"] = S.copy()
            ix = np.nonzero(act)[0]
            Sa = S[np.ix_(ix, ix)]
            L = np.zeros_like(Sa)
            deficient = False
            for i in range(ix.size):
                dg = Sa[i, i] - (L[i, :i] * L[i, :i]).sum()
                with np.errstate(all="ignore"):
                    rel = min(Sa[i, i] / hd[ix[i]] if hd[ix[i]] > 0 else T(0), dg / Sa[i, i] if Sa[i, i] > 0 else T(0))
                out["pivot"] = min(out["pivot"], float(rel))
                if not Sa[i, i] > T(eps_rank) * hd[ix[i]] or not dg > T(eps_rank) * Sa[i, i]:
                    deficient = True
                    break
                L[i, i] = np.sqrt(dg)
                for j in range(i + 1, ix.size):
                    L[j, i] = (Sa[i, j] - (L[i, :i] * L[j, :i]).sum()) / L[i, i]
            if deficient:
                status = RANK_DEFICIENT
                break
            y = np.zeros(ix.size, T)
            for i in range(ix.size):
                y[i] = (rhs[ix[i]] - (L[i, :i] * y[:i]).sum()) / L[i, i]
            x = np.zeros(ix.size, T)
            for i in range(ix.size - 1, -1, -1):
                x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
            dx[ix] = x
            for s in act_c:
                hcc, gc, hpc = cl[s]
                step_c[s] = (-gc - (hpc * dx).sum()) / hcc
        else:
            for s in act_c:
                m = slot == s
                step_c[s] = -(jc[m] * r[m]).sum() / (jc[m] * jc[m]).sum()
        pos, vel, clock = pos + dx[:3], vel + dx[3:], clock + step_c
        mag = max([0.0] + [float(abs(v)) for v in dx[act]] + [float(abs(step_c[s])) for s in act_c])
        out["steps"].append(mag)
        if not mag > step_tol:
            status = CONVERGED
            break
    if status == RANK_DEFICIENT:
        pos, vel, clock = pos0, vel0, clock0
    out["iters"], out["status"] = it, status
    return _finish(out, dat, rec, base, pos, vel, clock, T)


def _qr_lstsq(A, b):
    """min |A x - b| by Householder QR without pivoting, in A's precision.  Returns (R, Q^T b) of the leading columns."""
    A = A.copy(); b = b.copy()
    m, k = A.shape
    T = A.dtype.type
    for j in range(min(m, k)):
        x = A[j:, j]
        nx = np.sqrt((x * x).sum())
        if nx == 0:
            continue
        v = x.copy()
        v[0] = v[0] + (nx if x[0] >= 0 else -nx)
        vv = (v * v).sum()
        A[j:, j:] = A[j:, j:] - np.outer(v, (T(2) / vv) * (v @ A[j:, j:]))
        b[j:] = b[j:] - v * ((T(2) / vv) * (v @ b[j:]))
    return np.triu(A[:k, :k]) if m >= k else None, b[:k]


def solve_dense(pos, vel, base, clock, mode, clk_const, dat, rec, max_iter=20, step_tol=1e-4, eps_rank=1e-8, dtype=np.float64):
    """One epoch by Gauss-Newton on the full whitened Jacobian: columns = free ambiguities, unknown clocks, free [pos, vel]."""
    T = dtype
    dat = np.asarray(dat, np.float64).reshape(-1, DOUBLES).copy(); rec = np.asarray(rec).reshape(-1, 4)
    n = dat.shape[0]
    pos0, vel0, base, clock0 = (np.asarray(v).astype(T) for v in (pos, vel, base, clock))
    free = (rec[:, 2] & AMB_FREE) != 0
    slot = rec[:, 1]
    # a row with a free ambiguity is met exactly whatever its scale: one with w = 0 is taken with w = 1 so that its column is not zero
    unweighted = free & (dat[:, 7] == 0)
    dat[unweighted, 7] = 1.0
    w, lam = dat[:, 7].astype(T), dat[:, 8].astype(T)
    clk_rows = np.array([int((~free & (dat[:, 7] > 0) & (slot == s)).sum()) for s in range(CLOCKS)], np.int32)
    act_c = [s for s in range(CLOCKS) if not (clk_const >> s) & 1 and clk_rows[s] > 0]
    act = np.array([bool(mode & FREE_POS)] * 3 + [bool(mode & FREE_VEL)] * 3)
    ix = np.nonzero(act)[0]
    amb = np.nonzero(free)[0]
    na, nc, npv = amb.size, len(act_c), ix.size
    pos, vel, clock = pos0.copy(), vel0.copy(), clock0.copy()
    N = dat[:, 9].astype(T)
    out = dict(clk_rows=clk_rows, steps=[], pivot=np.inf)
    status, it = MAX_ITER, 0

    def residual(N):
        dd = dat.astype(T); dd[:, 9] = N
        return evaluate(dd, rec, pos + base, vel, clock, T)

    while it < max_iter:
        it += 1
        r, J, _nf, _br = residual(N)
        A = np.zeros((n, na + nc + npv), T)
        A[amb, np.arange(na)] = -w[amb] * lam[amb]
        for c, s in enumerate(act_c):
            A[slot == s, na + c] = w[slot == s]
        A[:, na + nc:] = J[:, ix]
        if n < A.shape[1]:
            A = np.vstack([A, np.zeros((A.shape[1] - n, A.shape[1]), T)]); r = np.concatenate([r, np.zeros(A.shape[0] - n, T)])
        R, qb = _qr_lstsq(A, -r)
        deficient = False
        for i in range(npv):
            col = R[:, na + nc + i]
            dg = col[na + nc + i] ** 2
            sii = (col[na + nc:na + nc + i + 1] ** 2).sum()
            hd = sii + (col[na:na + nc] ** 2).sum()
            with np.errstate(all="ignore"):
                out["pivot"] = min(out["pivot"], float(min(sii / hd if hd > 0 else T(0), dg / sii if sii > 0 else T(0))))
            if not sii > T(eps_rank) * hd or not dg > T(eps_rank) * sii:
                deficient = True
                break
        if deficient:
            status = RANK_DEFICIENT
            break
        k = A.shape[1]
        x = np.zeros(k, T)
        for i in range(k - 1, -1, -1):
            x[i] = (qb[i] - (R[i, i + 1:] * x[i + 1:]).sum()) / R[i, i] if R[i, i] != 0 else T(0)
        N[amb] = N[amb] + x[:na]
        for c, s in enumerate(act_c):
            clock[s] = clock[s] + x[na + c]
        dx = np.zeros(6, T); dx[ix] = x[na + nc:]
        pos, vel = pos + dx[:3], vel + dx[3:]
        mag = max([0.0] + [float(abs(v)) for v in x[na:]])
        out["steps"].append(mag)
        if not mag > step_tol:
            status = CONVERGED
            break
    if status == RANK_DEFICIENT:
        pos, vel, clock = pos0, vel0, clock0
    # the ambiguities alone at the final state: one column each, least squares again
    r, _J, _nf, br = residual(N)
    if na:
        A = np.zeros((n, na), T)
        A[amb, np.arange(na)] = -w[amb] * lam[amb]
        R, qb = _qr_lstsq(A, -r)
        N[amb] = N[amb] + qb / np.diag(R)
    r, _J, _nf, br = residual(N)
    r = np.where(unweighted, T(0), r)
    out.update(iters=it, status=status, pos=pos, vel=vel, clock=clock, N=N, r=r, cost=T(0.5) * (r * r).sum(), bracket=br)
    return out


def solve_batch(first, pos, vel, base, clock, mode, clk_const, dat, rec, max_iter=20, step_tol=1e-4, eps_rank=1e-8, dtype=np.float64,
                form=solve, **kw):
    """Every epoch of a packed call; returns the per-epoch results concatenated as solver.gnss_epoch_solve_batch returns them."""
    E = first.size - 1
    res = [form(pos[e], vel[e], base[e], clock[e], int(mode[e]), int(clk_const[e]), dat[first[e]:first[e + 1]], rec[first[e]:first[e + 1]],
                max_iter, step_tol, eps_rank, dtype, **kw) for e in range(E)]
    cat = lambda k: np.concatenate([np.atleast_1d(q[k]) for q in res]) if res else np.zeros(0, dtype)
    stack = lambda k: np.array([q[k] for q in res])
    out = dict(N=cat("N"), r=cat("r"), bracket=cat("bracket"))
    for k in ("pos", "vel", "clock", "cost", "iters", "status", "clk_rows"):
        out[k] = stack(k)
    if "info" in res[0] if res else False:
        out["info"] = stack("info")
    out["steps"] = [q["steps"] for q in res]
    out["pivot"] = np.array([q["pivot"] for q in res])
    return out
