"""A longdouble referee for everything BEHIND the reduced system of one trust-region iteration — the reduced solve, the back-substitution,
the dogleg (or Levenberg-Marquardt) step, the model cost change, the step norm and the retraction — with one bracket per compared
entry.  TEST INFRASTRUCTURE; the sibling of np_schur.py (whose elimination, Cholesky and ratio it reuses) and of np_linearize.py (whose
running (value, bracket) pairs V it reuses: x + y -> e_x + e_y + |x + y|, x y -> |x| e_y + |y| e_x + |x y|, ...; a sum of n terms is
taken as ONE operation of bracket sum e_i + sum |t_i|, in np_schur's manner, so that the bound does not depend on the summation order).

The damped system is (H + mu D) y = g with H = J^T J, g = J^T r from the exported (r, J), D = damping(diag) — clamp(diag) or, with Jacobi
scaling (Levenberg-Marquardt only), D_eff_i = clamp(diag_i s_i^2) / s_i^2, s_i = 1 / (1 + sqrt(diag_i)) — and mu the strategy's value
from the OPTIONS (dogleg: min_mu; Levenberg-Marquardt: 1 / radius, the float64 quotient), never from an export.  All arithmetic in
np.longdouble, without LAPACK; brackets in float64.

1. y_f is judged by the componentwise residual of the two triangular solves, not by its forward error (that one is the conditioning of S):
       with the implementation's complete factor L:      |L (L^T y_f) - rhs| <= M_Y 2^-52 |L| (|L^T| |y_f|)                     (solve_ratio)
       without it (the factor stayed in registers):      |S y_f - rhs| <= (M_Y + M_L) 2^-52 |Lh| (|Lh^T| |y_f|),  Lh = chol_ld(S)  (system_ratio)
2. y_e from the implementation's own y_f: (H_ee + mu D_e) y_e = g_e - H_ef y_f block by block over the connected components of H_ee;
   bracket |Ht_ee^-1| (B_g,e + E_ef |y_f| + E_ee |y_e|) in np_schur's notation (E = |J|^T |J| + mu D, |L_e| |L_e|^T added on ee).      (backsub)
3. the step from the implementation's own g, diag and y: ComputeTraditionalDoglegStep restated with V — alpha = |g / sqrt D|^2 / |J v|^2,
   v = g / D, |J v|^2 from J; the three branches; beta; step = (c1 g / sqrt d + c2 sqrt d y) / sqrt d.  Levenberg-Marquardt: -y, bracket 0. (step)
4. the model cost change, (a) by the identity H y = g - mu D y restated with V from the same vectors, (b) the true value
   -(J s).(r + J s / 2) with the derived terms of the gap (model_cost): the identity's own, 2 |c1 c2| |v|^T |rho| + c2^2 |y|^T |rho| with
   rho = g - (H + mu D) y from the implementation's own y, and the gradient's, |s|^T B_g (the implementation's g against J^T r).
   The step norm |x - Plus(x, step)| of the implementation's own step (step_norm).
5. the new state from the implementation's own step: fl(x + step) bit for bit on vector blocks, PoseLocalParameterization::Plus restated
   with V on pose blocks (retract)."""
import numpy as np

import np_linearize as nl
import np_schur as ns
from np_linearize import V

LD = np.longdouble
EPS = ns.EPS
DOGLEG, LM = 0, 1
GN, CAUCHY, INTERP = 0, 1, 2
BRANCH = ("gauss-newton", "cauchy", "interpolated")


def _ld(a):
    return np.asarray(a, np.float64).astype(LD)


def _f(a):
    return np.asarray(a).astype(np.float64)


def vsum(t):
    """sum of the entries of a V as ONE operation: bracket = sum of the terms' brackets + sum of their magnitudes"""
    return V(np.sum(t.v), np.asarray(np.sum(t.e) + np.sum(np.abs(_f(t.v)))))


def const(x):
    return V(np.asarray(x, np.float64).astype(LD))


def strategy_mu(opt):
    """the damping factor of the FIRST iteration as the kernels use it"""
    return float(np.float64(1.0) / np.float64(opt.initial_trust_region_radius)) if opt.trust_region_strategy == LM else float(opt.min_mu)


def damping(diag, opt, dtype=LD):
    """the diagonal the damping multiplies (damp_diag): clamp(diag), or with Jacobi scaling clamp(diag / q) q, q = (1 + sqrt(diag))^2"""
    d = np.asarray(diag, np.float64).astype(dtype)
    lo, hi = dtype(opt.min_diagonal), dtype(opt.max_diagonal)
    if opt.trust_region_strategy == LM and opt.jacobi_scaling:
        q = (1 + np.sqrt(np.maximum(d, 0))) ** 2
        return np.clip(d / q, lo, hi) * q
    return np.clip(d, lo, hi)


# ---------------------------------------------------------------------------------------------------------------- the damped system
def system(r, J, n_e, D, mu):
    """H, g (longdouble) of the export, the damped Hd = H + mu D, the brackets B_H, B_g, E = B_H + mu D and the blocks of H_ee"""
    r, J = np.asarray(r, np.float64), np.asarray(J, np.float64)
    H, g = ns.gram_ld(r, J)
    Ja = np.abs(J)
    BH, Bg = Ja.T @ Ja, Ja.T @ np.abs(r)
    md = LD(mu) * _ld(D)
    Hd = H.copy()
    Hd[np.diag_indices_from(Hd)] += md
    E = BH.copy()
    E[np.diag_indices_from(E)] += _f(md)
    return dict(r=r, J=J, n_e=int(n_e), H=H, g=g, Hd=Hd, BH=BH, Bg=Bg, E=E, md=md, blocks=ns.components(BH[:n_e, :n_e] > 0))


def reduced(sy):
    """referee and brackets of the DAMPED reduced system (S, rhs) of a system(): np_schur's elimination with Hd and E"""
    S, rhs, bS, brhs = ns._eliminate(sy["Hd"], sy["g"], sy["E"], sy["Bg"], sy["n_e"], sy["blocks"])
    return dict(S=(S + S.T) / 2, rhs=rhs, b_S=bS, b_rhs=brhs)


# ---------------------------------------------------------------------------------------------------------------- 1. y_f
def solve_ratio(L, rhs, yf):
    """|L (L^T y_f) - rhs| / (2^-52 |L| (|L^T| |y_f|)) entry by entry; L the implementation's complete lower factor"""
    L, yf = np.asarray(L, np.float64), np.asarray(yf, np.float64)
    assert not np.triu(L, 1).any(), "the exported factor is not lower triangular"
    Ll, La = _ld(L), np.abs(L)
    return ns.ratio(Ll @ (Ll.T @ _ld(yf)), rhs, La @ (La.T @ np.abs(yf))), La @ (La.T @ np.abs(yf))


def system_ratio(S, rhs, yf):
    """|S y_f - rhs| / (2^-52 |Lh| (|Lh^T| |y_f|)), Lh the referee's own longdouble Cholesky factor of the implementation's S"""
    S, yf = np.asarray(S, np.float64), np.asarray(yf, np.float64)
    La = np.abs(_f(ns.chol_ld(_ld(S))))
    return ns.ratio(_ld(S) @ _ld(yf), rhs, La @ (La.T @ np.abs(yf))), La @ (La.T @ np.abs(yf))


# ---------------------------------------------------------------------------------------------------------------- 2. y_e
def backsub(sy, yf):
    """(y_e longdouble, bracket float64) from the implementation's y_f"""
    n_e, Hd, E, g, Bg = sy["n_e"], sy["Hd"], sy["E"], sy["g"], sy["Bg"]
    yf = np.asarray(yf, np.float64)
    ye, br = np.zeros(n_e, LD), np.zeros(n_e)
    for c in sy["blocks"]:
        f = np.flatnonzero(E[c][:, n_e:].any(axis=0))
        L = ns.chol_ld(Hd[np.ix_(c, c)])
        t = g[c] - Hd[np.ix_(c, n_e + f)] @ _ld(yf[f])
        sol = ns.chol_solve_ld(L, np.column_stack([t, np.eye(c.size, dtype=LD)]))
        ye[c] = sol[:, 0]
        La = np.abs(_f(L))
        Eee = E[np.ix_(c, c)] + La @ La.T
        br[c] = np.abs(_f(sol[:, 1:])) @ (Bg[c] + E[np.ix_(c, n_e + f)] @ np.abs(yf[f]) + Eee @ np.abs(_f(sol[:, 0])))
    assert not ye[br == 0].any()
    return ye, br


# ---------------------------------------------------------------------------------------------------------------- 3. the step
def step(sy, g, diag, y, opt):
    """The step of the first iteration from the implementation's own g, diag, y (float64, exact inputs).  Returns dict(step: V [n];
    branch; ties: the relative distances of the branch conditions from equality; c1, c2, alpha, gsq, ynn, gy, jg_sq: V scalars; v, sd)"""
    g, diag, y = (V(_ld(a)) for a in (g, diag, y))
    n = g.v.size
    lm = opt.trust_region_strategy == LM
    radius = const(opt.initial_trust_region_radius)
    D = V(damping(diag.v, opt))                       # clamping is exact; D_eff carries the roundings of its own formula below
    if lm and opt.jacobi_scaling:
        one = const(1.0)
        q = (one + V(np.maximum(diag.v, 0)).sqrt())
        q = q * q
        lo, hi = LD(opt.min_diagonal), LD(opt.max_diagonal)
        c = diag / q
        D = V(np.clip(c.v, lo, hi), np.where((c.v > lo) & (c.v < hi), c.e, 0.0)) * q
    sd = D.sqrt()
    gs = g / sd
    gsq, ynn, gy = vsum(gs * gs), vsum(D * y * y), vsum(g * y)
    v = g / D
    Jv = V(_ld(sy["J"])) @ V(v.v.reshape(-1, 1), v.e.reshape(-1, 1))
    jg_sq = vsum(Jv * Jv)
    out = dict(gsq=gsq, ynn=ynn, gy=gy, jg_sq=jg_sq, v=v, sd=sd, D=D, ties=[])
    if lm:
        out.update(branch=GN, c1=const(0.0), c2=const(-1.0), step=V(-y.v, np.zeros(n)), alpha=gsq / jg_sq)
        return out
    gnorm, gnn, alpha = gsq.sqrt(), ynn.sqrt(), gsq / jg_sq
    ca = gnorm * alpha
    rel = lambda a: abs(float(a.v / radius.v) - 1.0)
    out["ties"].append(rel(gnn))
    if gnn.v <= radius.v:
        branch, c1, c2 = GN, const(0.0), const(-1.0)
    else:
        out["ties"].append(rel(ca))
        if ca.v >= radius.v:
            branch, c1, c2 = CAUCHY, -(radius / gnorm), const(0.0)
        else:
            b_dot_a = alpha * gy                      # -alpha * gdot, gdot = -g.y
            a_sq = ca * ca
            bma_sq = a_sq - const(2.0) * b_dot_a + gnn * gnn
            cc = b_dot_a - a_sq
            rr = radius * radius - a_sq
            dd = (cc * cc + bma_sq * rr).sqrt()
            beta = (dd - cc) / bma_sq if cc.v <= 0 else rr / (dd + cc)
            branch, c1, c2 = INTERP, -(alpha * (const(1.0) - beta)), -beta
            out.update(beta=beta, cc=cc, dd=dd, bma_sq=bma_sq)
    out.update(branch=branch, c1=c1, c2=c2, alpha=alpha, step=(c1 * gs + c2 * (sd * y)) / sd)
    return out


# ---------------------------------------------------------------------------------------------------------------- 4. scalars
def model_cost(sy, st, g, y, mu, s_impl):
    """(identity: V, true: longdouble, derived: float64) — the model cost change by the identity from the referee's scalars; its true value
    -(J s).(r + J s / 2) at the implementation's own step; and the derived bound of the gap between the two beyond rounding"""
    c1, c2, gsq, ynn, gy, jg_sq = (st[k] for k in ("c1", "c2", "gsq", "ynn", "gy", "jg_sq"))
    m, two, half = const(mu), const(2.0), const(0.5)
    sHs = c1 * c1 * jg_sq + two * c1 * c2 * (gsq - m * gy) + c2 * c2 * (gy - m * ynn)
    ident = -(c1 * gsq + c2 * gy + half * sHs)
    s = _ld(s_impl)
    Js = _ld(sy["J"]) @ s
    true = -(Js @ (_ld(sy["r"]) + Js / 2))
    rho = np.abs(_f(_ld(g) - (sy["Hd"] @ _ld(y))))
    a1, a2 = abs(float(c1.v * c2.v)), float(c2.v) ** 2
    derived = 2 * a1 * float(np.abs(_f(st["v"].v)) @ rho) + a2 * float(np.abs(np.asarray(y, np.float64)) @ rho)
    grad_term = float(np.abs(np.asarray(s_impl, np.float64)) @ sy["Bg"])
    return ident, true, derived, grad_term


def pose_plus(x, d):
    """PoseLocalParameterization::Plus with V: x [7] exact, d [6] exact -> V [7]"""
    x, d = V(_ld(x)), V(_ld(d))
    p = x[:3] + d[:3]
    half = d[3:] / const(2.0)
    dq = V(np.concatenate([half.v, [LD(1)]]).reshape(4, 1), np.concatenate([half.e, [0.0]]).reshape(4, 1))
    q = nl.qmul(V(x.v[3:].reshape(4, 1), x.e[3:].reshape(4, 1)), dq)
    q = q / vsum(q * q).sqrt()
    return V(np.concatenate([p.v, q.v[:, 0]]), np.concatenate([p.e, q.e[:, 0]]))


def retract(blocks, loc, s_impl):
    """Per variable block (in block order): (local offset, x_new as V [size]) from the implementation's own step.  Vector blocks:
    fl(x + step), bracket zero.  blocks: the state BEFORE the step; loc: local offset per block or -1."""
    out = []
    s = np.asarray(s_impl, np.float64)
    for b, x in enumerate(blocks):
        if loc[b] < 0:
            continue
        if x.size == 7:
            out.append((b, pose_plus(x, s[loc[b]:loc[b] + 6])))
        else:
            out.append((b, V(_ld(np.asarray(x, np.float64) + s[loc[b]:loc[b] + x.size]))))
    return out


def step_norm(blocks, new):
    """|x - x_new| over the variable blocks (ambient coordinates) as a V scalar; new = retract(...)"""
    d = [V(_ld(blocks[b])) - xn if np.any(xn.e) else V(_ld(blocks[b]) - xn.v) for b, xn in new]
    d = V(np.concatenate([t.v for t in d]), np.concatenate([t.e for t in d]))
    return vsum(d * d).sqrt()


def scalar_ratio(impl, ref):
    return float(ns.ratio(np.asarray(impl), ref.v, ref.e))
