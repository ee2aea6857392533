"""The solve step — the reduced solve, the back-substitution (k_post_chol: d_backsub_lm, d_backsub_clique), the dogleg / Levenberg-
Marquardt step, the model cost change, the step norm (d_dogleg) and the retraction to the new state — held to a longdouble referee ENTRY BY
ENTRY.  Referee and brackets: tests/np_step.py; cases: tests/step_cases.py.  The sibling of test_schur_componentwise.py, one stage on.

One case is two solves of the same window.  Run A, step_mode = 1: (r, J), grad, diag, S, rhs, the complete L and y_f at the uploaded
state, mu = 0.  Run B, max_num_iterations = 1 with the case's strategy and radius: the damped S, rhs, y, the step, iteration row 1 and the
downloaded state; its step must be valid and successful.  That the two describe the same linearisation is asserted through the referee:
run B's S and rhs must be the DAMPED reduction of run A's (r, J) under the Schur test's own rule and constants (M_S, M_R), mu taken from
the options.  (mu damps H_ee as well, so run B's rhs and the off-diagonal of its S are NOT run A's bits)

Every judged quantity q must satisfy |q - referee| <= M 2^-52 bracket(q) in every entry, no mask; a zero bracket admits the exact value
only (Levenberg-Marquardt's step = -y, the vector blocks of the new state = fl(x + step), structural zeros).

    quantity                    input                                   rule / constant
    y_f, run A                  the implementation's L, rhs             |L (L^T y_f) - rhs| <= M_Y 2^-52 |L| |L^T| |y_f|
    y_f, run B                  its damped S, rhs                       |S y_f - rhs| <= (M_Y + M_L) 2^-52 |Lh| |Lh^T| |y_f|, Lh = chol_ld(S)
    y_e                         (r, J) of run A, y_f of run B           M_E
    step                        g, diag of run A, y of run B, J         M_T, the branch the referee's, no branch condition within 1e-6 of a tie
    model cost change (a)       the same vectors, the identity          M_C
    model cost change (b)       J, r, the implementation's step         M_C bracket + M_G |s|^T B_g + 2 |c1 c2| |v|^T |rho| + c2^2 |y|^T |rho|
    step_norm                   the implementation's step, x            M_N
    new state                   the implementation's step, x            vector blocks exact, pose blocks M_P

The constants are measured on the CPU, never on the device: M = ceil(8 x the largest ratio either of two float64 routes shows over every
case); route 1 the oracle (its own (r, J), y, step, rows, end state; the identity of (a) evaluated in float64 from its vectors), route 2
plain numpy (np_dense.dense_system's normal equations, LAPACK solves, the dogleg of np_dense.trust_region restated on vectors).
test_constants_are_the_measured_ones prints every ratio with its route and case.

Largest device ratios on MI355X (every GPU test prints its own; per case in DESIGN.md §4): y_f 3.96 (run A, idepth_long) and 6.27 (run B,
n_red_550), y_e 1.29 (n_red_256), step 0.40 (n_loc_over_4096), model cost change 0.05, step_norm 0.48 (ragged-lm), pose 0.49 (tiny_rtk);
the model cost change lies at most 4.6e-16 of its value from -(J s).(r + J s / 2) (composite_landmarks).  The knob and batch variants give
the single window's bits.  Found and fixed with this file: Levenberg-Marquardt's step went through the scaled space and was -y only to the
roundings of rsqrt_nr; d_dogleg now stores -y itself."""
import functools
import math

import numpy as np
import pytest

import np_dense as nd
import np_schur as ns
import np_step as st
import oracle_binding as ob
import step_cases as sp
from bitwise import multi_processor_count
from plan_cases import plan_check
from schur_cases import M_G, M_L, M_R, M_S, VACUOUS
from rtk_visual_inertial_navigation_amd.flat import default_options

EPS = ns.EPS
# name = ceil(8 x largest CPU ratio); the ratio, the route and the case it came from
M_Y = 48.0      # y_f         5.989  oracle, n_red_550 (run A; run B, judged at M_Y + M_L, shows at most 8.45: oracle, n_red_550)
M_E = 16.0      # y_e         1.910  oracle, n_red_256
M_T = 3.0       # step        0.318  oracle, n_red_550 (clipped Cauchy step)
M_C = 1.0       # model cost change by the identity  0.087  numpy, idepth_long
M_N = 6.0       # step_norm   0.649  oracle, doppler
M_P = 4.0       # pose blocks of the new state  0.492  numpy, ragged-lm
M = dict(Y=M_Y, E=M_E, T=M_T, C=M_C, N=M_N, P=M_P)
FLOOR = 2.0 ** -26       # entries of y_e and step at least this share of their block's largest are held to VACUOUS
SHARE = 0.25             # at most this share of a family's non-zero entries may lie below the floor
TIE = 1e-6
OLD = dict(berr=1e-12, step_norm=1e-9, relative_decrease=1e-7)

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps,
                                      reason="np.longdouble is no wider than float64 on this platform")
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the rule
def passes(q, limit):
    return bool(np.all(np.asarray(q) <= limit))


def layout(w):
    """(blocks: views of the window's state, loc: local offset per block or -1, sizes: local size per block)"""
    loc, _, _ = nd.local_layout(w)
    _, l = w.block_sizes()
    return nd.blocks_of(w), loc, l


def vacuity(w, ref, bracket, limit, n0=0):
    """(largest M 2^-52 bracket / |value| over the entries at or above the floor of their block, largest share of a family's non-zero entries
    below it) of a local vector starting at local offset n0; family = blocks of one size (poses, speed-bias, landmarks, scalars)"""
    _, loc, l = layout(w)
    v, br = np.abs(np.asarray(ref, np.float64)), np.asarray(bracket, np.float64)
    worst, below, count = 0.0, {}, {}
    for b in range(len(loc)):
        a = loc[b] - n0
        if loc[b] < 0 or a < 0 or a >= v.size:
            continue
        vb, bb = v[a:a + l[b]], br[a:a + l[b]]
        top = vb.max()
        if top == 0:
            continue
        keep = vb >= FLOOR * top
        worst = max(worst, float((limit * EPS * bb[keep] / vb[keep]).max()))
        nz = vb > 0
        below[l[b]] = below.get(l[b], 0) + int((nz & ~keep).sum())
        count[l[b]] = count.get(l[b], 0) + int(nz.sum())
    return worst, max([below[k] / count[k] for k in count], default=0.0)


def blind(impl, ref, bracket, limit):
    """True if the rule does NOT see 2 M brackets added to the weakest expected entry (smallest |value| among those with a bracket)"""
    br = np.asarray(bracket, np.float64).ravel()
    if not (br > 0).any():
        return False
    i = ns.weakest(ref, br)
    e = np.array(ref, np.longdouble).ravel()
    e[i] += 2 * limit * EPS * br[i]
    return passes(ns.ratio(np.asarray(impl).ravel(), e, br), limit)


def judge(label, w, opt, A, B, want_branch=None, constants=M, check=True):
    """The whole rule on one implementation.  A: dict(r, J, n_e, g, diag, rhs, L, y) of run A; B: dict(S, rhs, y, step, mcc, step_norm,
    valid, successful, blocks: the state after the step) of run B; w: the window BEFORE the step.  Returns dict(name -> largest ratio, plus
    the evidence figures).  check = False only measures (the constants test)."""
    n_e = int(A["n_e"])
    mu = st.strategy_mu(opt)
    D = st.damping(A["diag"], opt)
    sy = st.system(A["r"], A["J"], n_e, D, mu)
    out = {}
    if check:
        assert B["valid"] and B["successful"], (label, "the step of run B was not valid and successful")
        red = st.reduced(sy)
        out["S_B"], out["rhs_B"] = float(ns.ratio(B["S"], red["S"], red["b_S"]).max()), float(ns.ratio(B["rhs"], red["rhs"], red["b_rhs"]).max())
        assert out["S_B"] <= M_S and out["rhs_B"] <= M_R, (label, "run B's reduced system is not the damped reduction of run A's linearisation", out)
        assert np.array_equal(np.asarray(B["S"]), np.asarray(B["S"]).T)
    # 1. y_f
    qa, ba = st.solve_ratio(A["L"], A["rhs"], A["y"][n_e:])
    qb, bb = st.system_ratio(B["S"], B["rhs"], B["y"][n_e:])
    out["Y"], out["Y_B"] = float(qa.max()), float(qb.max())
    # 2. y_e
    ye, bye = st.backsub(sy, B["y"][n_e:])
    qe = ns.ratio(B["y"][:n_e], ye, bye)
    out["E"] = float(qe.max()) if n_e else 0.0
    # 3. the step
    s = st.step(sy, A["g"], A["diag"], B["y"], opt)
    qt = ns.ratio(B["step"], s["step"].v, s["step"].e)
    out["T"] = float(qt.max())
    out["branch"], out["ties"] = s["branch"], s["ties"]
    # 4. the scalars
    ident, true, derived, grad_term = st.model_cost(sy, s, A["g"], B["y"], mu, B["step"])
    out["C"] = st.scalar_ratio(B["mcc"], ident)
    gap = abs(float(np.longdouble(B["mcc"]) - true))
    bound = constants["C"] * EPS * float(ident.e) + M_G * EPS * grad_term + derived
    out["gap"], out["gap_bound"], out["gap_rel"], out["derived_rel"] = gap, bound, gap / abs(float(true)), derived / abs(float(true))
    blocks, loc, _ = layout(w)
    new = st.retract(blocks, loc, B["step"])
    sn = st.step_norm(blocks, new)
    out["N"] = st.scalar_ratio(B["step_norm"], sn)
    # 5. the new state
    qp, exact = [0.0], True
    for b, xn in new:
        if np.any(xn.e):
            qp.append(float(ns.ratio(B["blocks"][b], xn.v, xn.e).max()))
        else:
            exact &= np.array_equal(np.asarray(B["blocks"][b], np.float64), xn.v.astype(np.float64))
    out["P"], out["exact"] = max(qp), exact
    print("%-44s y_f %.2f (run B %.2f)  y_e %.2f  step %.2f [%s]  mcc %.2f  step_norm %.2f  pose %.2f | mcc identity gap %.1e of mcc (derived bound %.1e)"
          % (label, out["Y"], out["Y_B"], out["E"], out["T"], st.BRANCH[s["branch"]], out["C"], out["N"], out["P"], out["gap_rel"], out["derived_rel"]))
    if not check:
        return out
    c = constants
    assert all(t > TIE for t in s["ties"]), (label, "a branch condition lies within 1e-6 of a tie: not a case", s["ties"])
    if want_branch is not None:
        assert s["branch"] == want_branch, (label, "the case does not reach its branch", st.BRANCH[s["branch"]])
    assert passes(qa, c["Y"]), (label, "y_f of run A", out["Y"], int(np.argmax(qa)))
    assert passes(qb, c["Y"] + M_L), (label, "y_f of run B", out["Y_B"], int(np.argmax(qb)))
    assert passes(qe, c["E"]), (label, "y_e", out["E"], int(np.argmax(qe)))
    assert passes(qt, c["T"]), (label, "step", out["T"], int(np.argmax(qt)), st.BRANCH[s["branch"]])
    assert out["C"] <= c["C"], (label, "model cost change against the identity", out["C"])
    assert gap <= bound, (label, "model cost change against -(J s).(r + J s / 2)", gap, bound)
    assert out["N"] <= c["N"], (label, "step_norm", out["N"])
    assert exact, (label, "a vector block of the new state is not fl(x + step)")
    assert out["P"] <= c["P"], (label, "pose block of the new state", out["P"])
    # not vacuous: M 2^-52 bracket <= VACUOUS |value| at or above the floor; at most SHARE of a family's non-zeros below it
    for name, ref, br, lim, n0 in (("y_e", ye, bye, c["E"], 0), ("step", s["step"].v, s["step"].e, c["T"], 0)):
        if np.size(ref) and (opt.trust_region_strategy != st.LM or name != "step"):
            vac, share = vacuity(w, ref, br, lim, n0)
            out["vac_" + name], out["share_" + name] = vac, share
            assert vac <= VACUOUS and share <= SHARE, (label, name, "vacuous", vac, share)
    # sensitive: 2 M brackets on the weakest expected entry of each quantity must fail
    assert not blind(_apply(A["L"], A["y"][n_e:]), A["rhs"], ba, c["Y"]), (label, "y_f (run A) blind to 2 M brackets")
    assert not blind(_apply_S(B["S"], B["y"][n_e:]), B["rhs"], bb, c["Y"] + M_L), (label, "y_f (run B) blind to 2 M brackets")
    assert not blind(B["y"][:n_e], ye, bye, c["E"]), (label, "y_e blind to 2 M brackets")
    assert not blind(B["step"], s["step"].v, s["step"].e, c["T"]), (label, "step blind to 2 M brackets")
    assert not blind([B["mcc"]], [ident.v], [ident.e], c["C"]) and not blind([B["step_norm"]], [sn.v], [sn.e], c["N"]), (label, "scalars blind")
    for b, xn in new:
        if np.any(xn.e):
            assert not blind(B["blocks"][b], xn.v, xn.e, c["P"]), (label, "pose blind to 2 M brackets")
    return out


def _apply(L, y):
    Ll = np.asarray(L, np.float64).astype(np.longdouble)
    return Ll @ (Ll.T @ np.asarray(y, np.float64).astype(np.longdouble))


def _apply_S(S, y):
    return np.asarray(S, np.float64).astype(np.longdouble) @ np.asarray(y, np.float64).astype(np.longdouble)


# ---------------------------------------------------------------------------------------------------------------- CPU routes
def dogleg_f64(r, J, g, diag, y, opt, faults=()):
    """d_dogleg restated on vectors in float64 (np_dense.trust_region's dogleg, the model cost change by the identity): dict(step, mcc, branch)"""
    D = st.damping(diag, opt, np.float64)
    mu = st.strategy_mu(opt)
    sd = np.sqrt(D)
    gs = g / sd
    gsq, ynn, gy = gs @ gs, (D * y) @ y, g @ y
    v = g / D
    Jv = J @ v
    if "papart" in faults:       # one block of (up to 256) projection observations left out of |J v|^2
        Jv = Jv[2 * min(256, faults["papart"]):]
    jg_sq = Jv @ Jv
    radius = opt.initial_trust_region_radius
    if opt.trust_region_strategy == st.LM:
        c1, c2, branch, step = 0.0, -1.0, st.GN, -y
    else:
        gnorm, gnn, alpha = np.sqrt(gsq), np.sqrt(ynn), gsq / jg_sq
        if gnn <= radius:
            c1, c2, branch = 0.0, -1.0, st.GN
        elif gnorm * alpha >= radius:
            c1, c2, branch = -(radius / gnorm), 0.0, st.CAUCHY
        else:
            b_dot_a = alpha * gy
            a_sq = (alpha * gnorm) ** 2
            bma_sq = a_sq - 2 * b_dot_a + gnn ** 2
            cc = b_dot_a - a_sq
            dd = np.sqrt(cc * cc + bma_sq * (radius ** 2 - a_sq))
            beta = (dd - cc) / bma_sq if cc <= 0 else (radius ** 2 - a_sq) / (dd + cc)
            if "beta" in faults:   # the other root of the quadratic
                beta = (-dd - cc) / bma_sq
            c1, c2, branch = -alpha * (1 - beta), -beta, st.INTERP
        step = (c1 * gs + c2 * (sd * y)) / sd
    sHs = c1 * c1 * jg_sq + 2 * c1 * c2 * (gsq - mu * gy) + c2 * c2 * (gy - mu * ynn)
    return dict(step=step, mcc=-(c1 * gsq + c2 * gy + 0.5 * sHs), branch=branch)


def after_step(w, step):
    """(state blocks after Plus(x, step), step_norm, cost at the new state) in float64, on a copy"""
    w2 = w.copy()
    x0 = nd.variable_state(w2)
    nd.plus(w2, step)
    return [b.copy() for b in nd.blocks_of(w2)], float(np.linalg.norm(nd.variable_state(w2) - x0)), w2


def oracle_route(w, opt):
    """route 1: the oracle's own (r, J), exports, step, rows and end state; the identity of the model cost change in float64 from its vectors"""
    _, ea = ob.solve(w.copy(), default_options(step_mode=1))
    r, J = ob.export_jacobian(w)
    wb = w.copy()
    sm, eb = ob.solve(wb, opt)
    row = sm.trace[1]
    A = dict(r=r, J=J, n_e=ea["n_e"], g=ea["grad"], diag=ea["diag"], rhs=ea["rhs"], L=ea["L"], y=ea["y"], S=ea["S"])
    B = dict(S=eb["S"], rhs=eb["rhs"], y=eb["y"], step=eb["step"], mcc=dogleg_f64(r, J, ea["grad"], ea["diag"], eb["y"], opt)["mcc"],
             mcc_true=row.model_cost_change, step_norm=row.step_norm, valid=row.step_is_valid, successful=row.step_is_successful,
             blocks=[b.copy() for b in nd.blocks_of(wb)], relative_decrease=row.relative_decrease)
    return A, B


def numpy_route(w, r, J, n_e, opt, faults=None):
    """route 2: plain numpy from (r, J).  faults (the mutation controls): dict with any of ypose, obs, strip, papart, beta"""
    from scipy.linalg import solve_triangular
    faults = faults or {}
    d0 = nd.dense_system(r, J, n_e)
    g, diag = d0["g"], d0["diag"]
    y0 = solve_triangular(d0["L"], solve_triangular(d0["L"], d0["rhs"], lower=True), lower=True, trans=1)
    A = dict(r=r, J=J, n_e=n_e, g=g, diag=diag, rhs=d0["rhs"], L=d0["L"], y=np.concatenate([np.zeros(n_e), y0]), S=d0["S"])
    mu, D = st.strategy_mu(opt), st.damping(diag, opt, np.float64)
    Hd = d0["H"] + np.diag(mu * D)
    Hee, Hef = Hd[:n_e, :n_e], Hd[:n_e, n_e:]
    X = np.linalg.solve(Hee, np.column_stack([Hef, g[:n_e]])) if n_e else np.zeros((0, Hd.shape[0] - n_e + 1))
    S = Hd[n_e:, n_e:] - Hef.T @ X[:, :-1]
    S = 0.5 * (S + S.T)
    rhs = g[n_e:] - Hef.T @ X[:, -1]
    L = np.linalg.cholesky(S)
    yf = solve_triangular(L, solve_triangular(L, rhs, lower=True), lower=True, trans=1)
    # back-substitution from the stored Jacobians, block by block: y_c = Hd_cc^-1 J_c^T (r - J_f y_f) over the rows that touch the block
    ye = np.zeros(n_e)
    nz = J != 0
    blocks = ns.components((np.abs(J[:, :n_e]).T @ np.abs(J[:, :n_e])) > 0) if n_e else []
    lm = [k for k, c in enumerate(blocks) if c.size == 3]
    cl = [k for k, c in enumerate(blocks) if c.size > 3] or list(range(len(blocks)))
    for k, c in enumerate(blocks):
        rows = np.flatnonzero(nz[:, c].any(axis=1))
        y_use = yf.copy()
        f = np.flatnonzero(nz[rows][:, n_e:].any(axis=0))
        if "ypose" in faults and f.size:                     # one entry of y_f scaled by 1 + 1e-9 ahead of every back-substitution that reads it
            y_use[faults["ypose"]] *= 1.0 + 1e-9
        if "strip" in faults and k == cl[len(cl) // 2]:      # one strip column of this clique's H_ef y_f skipped
            y_use[f[np.argmax(np.abs(J[rows][:, n_e + f]).sum(0) * np.abs(yf[f]))]] = 0.0
        if "obs" in faults and lm and k == lm[len(lm) // 2]:   # one observation (its two rows) left out of this track's sum
            rows = rows[2:]
        ye[c] = np.linalg.solve(Hd[np.ix_(c, c)], J[rows][:, c].T @ (r[rows] - J[rows][:, n_e:] @ y_use))
    y = np.concatenate([ye, yf])
    dl = dogleg_f64(r, J, g, diag, y, opt, faults)
    blocks_new, sn, w2 = after_step(w, dl["step"])
    Js = J @ dl["step"]
    B = dict(S=S, rhs=rhs, y=y, step=dl["step"], mcc=dl["mcc"], mcc_true=-Js @ (r + Js / 2), step_norm=sn, valid=True, successful=True,
             blocks=blocks_new, Hd=Hd, g=g, w_new=w2)
    return A, B


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    wn, kw, branch = sp.CASES[name]
    w = sp.window(wn)
    opt = sp.options(**kw)
    Ao, Bo = oracle_route(w, opt)
    An, Bn = numpy_route(w, Ao["r"], Ao["J"], Ao["n_e"], opt)
    return dict(w=w, opt=opt, branch=branch, oracle=(Ao, Bo), numpy=(An, Bn))


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@needs_longdouble
def test_constants_are_the_measured_ones():
    """Both float64 routes over every case: every ratio printed with its route and case, every one within its constant, and no constant
    padded (the largest ratio within a factor of two of M / 8)."""
    top = {k: (0.0, "") for k in M}
    for name in sp.CASES:
        c = cpu_case(name)
        for route in ("oracle", "numpy"):
            A, B = c[route]
            o = judge("%s, %s:" % (name, route), c["w"], c["opt"], A, B, check=False)
            for k in M:
                v = max(o[k], o["Y_B"] - M_L) if k == "Y" else o[k]
                if v > top[k][0]:
                    top[k] = (v, "%s, %s" % (name, route))
    for k, (v, where) in top.items():
        print("M_%s: largest ratio %.3f (%s) -> ceil(8 x) = %d, constant %d" % (k, v, where, math.ceil(8 * v), M[k]))
    for k, (v, where) in top.items():
        assert v <= M[k], (k, v, where)
        assert v >= M[k] / 16, (k, v, where, "the constant is padded")


@needs_longdouble
@pytest.mark.parametrize("name", list(sp.CASES))
def test_oracle_and_numpy_pass_the_componentwise_rule(name):
    """the CPU tier proper: both float64 routes within the constants in every entry, zero brackets exact, nothing vacuous, the rule sensitive
    to 2 M brackets on the weakest entry of every quantity, the branch the case names, no branch condition near a tie"""
    c = cpu_case(name)
    for route in ("oracle", "numpy"):
        A, B = c[route]
        o = judge("%s, %s:" % (name, route), c["w"], c["opt"], A, B, want_branch=c["branch"])
        print("%-44s vacuity: y_e %.1e (share below the floor %.2f)  step %.1e (%.2f); run B against the damped referee: S %.2f rhs %.2f"
              % ("", o.get("vac_y_e", 0), o.get("share_y_e", 0), o.get("vac_step", 0), o.get("share_step", 0), o["S_B"], o["rhs_B"]))
    # the oracle's own model cost change is the true one, -(J s).(r + J s / 2): the identity's gap against it, for the record
    A, B = c["oracle"]
    print("%-44s the oracle's -(J s).(r + J s / 2) %.17g, the identity from its vectors %.17g" % ("", B["mcc_true"], B["mcc"]))


@needs_longdouble
def test_case_reaches_its_branch():
    """each window reaches what step_cases.py says: the eliminated-block structure, the observation counts, the reduced dimensions"""
    import schur_cases as sc
    for name, n_red in sc.FACTOR_N_RED.items():
        if name in sp.CASES:
            assert cpu_case(name)["oracle"][0]["rhs"].size == n_red
    w = sp.window("constant_landmark")
    assert int(w.a["is_const"][w.n_pose + w.n_sb:w.n_pose + w.n_sb + w.n_lm].sum()) == 1
    lm_obs = w.a["proj_idx"].reshape(-1, 3)[:, 2]
    assert (w.a["is_const"][w.n_pose + w.n_sb + lm_obs] == 1).sum() >= 2
    assert sp.window("obs_over_256").a["proj_idx"].size // 3 > 256
    w = sp.window("constant_pose")
    assert w.a["is_const"][2] == 1 and nd.local_layout(w)[0][2] < 0          # pose 2 has no local columns (lp < 0 for its observations)
    assert (w.a["proj_idx"].reshape(-1, 3)[:, :2] == 2).any()
    assert nd.local_layout(sp.window("n_loc_over_1024"))[1] > 1024 and nd.local_layout(sp.window("n_loc_over_4096"))[1] > 4096
    # launch shapes, from the host-only plan (swf_debug_plan_check): one window takes the latency path (k_post_chol<0>, the fused step or
    # k_dogleg<16, 4>), SWF_NO_LAT_FUSE (flag 1) and the batches the batch path (k_dogleg<4, 2>); 256 = the MI355X's CU count
    for wins, flags, lat in (([sp.window("ragged")], 0, 1), ([sp.window("ragged")], 1, 0), (_batch(sp.BATCH_N)[0], 0, 0), (_batch(260)[0], 0, 0),
                             ([sp.window("n_loc_over_1024")], 1, 0), ([sp.window("n_loc_over_4096")], 0, 1), ([sp.window("n_loc_over_4096")], 1, 0)):
        rc, msg, info = plan_check(wins, 256, flags=flags)
        assert rc == 0 and info["lat_fuse"] == lat, (len(wins), flags, msg, info)
    for name, (wn, kw, branch) in sp.CASES.items():
        if branch is not None and kw.get("strategy", 0) == sp.DOGLEG:
            c = cpu_case(name)
            A, B = c["oracle"]
            s = st.step(st.system(A["r"], A["J"], A["n_e"], st.damping(A["diag"], c["opt"]), st.strategy_mu(c["opt"])), A["g"], A["diag"], B["y"], c["opt"])
            gnn, ca = float(np.sqrt(s["ynn"].v)), float(np.sqrt(s["gsq"].v) * s["alpha"].v)
            print("%-24s radius %.4g  Gauss-Newton norm %.6g  Cauchy length %.6g -> %s" % (name, c["opt"].initial_trust_region_radius, gnn, ca, st.BRANCH[s["branch"]]))
            assert s["branch"] == branch and all(t > 0.2 for t in s["ties"]), (name, s["ties"])


def _old_rules(c, Bn, Bm):
    """readings of the rules this file replaces, mutated route against the clean one: normwise backward error of y, step_norm, relative decrease"""
    cost0 = nd.window_cost(c["w"])
    rd = lambda B: (cost0 - nd.window_cost(B["w_new"])) / B["mcc_true"]
    return dict(berr=nd.backward_error(Bm["Hd"], Bm["y"], Bm["g"]), step_norm=abs(Bm["step_norm"] - Bn["step_norm"]) / Bn["step_norm"],
                relative_decrease=abs(rd(Bm) - rd(Bn)) / abs(rd(Bn)))


@needs_longdouble
@pytest.mark.parametrize("pair", sp.CONTROL, ids=[p[0].split("-")[0] for p in sp.CONTROL])
def test_mutation_controls_fail_the_new_rule(pair):
    """Copies of the numpy float64 route, not the device, each with ONE fault: the new rule must fail on the quantity the fault touches (the
    margin is printed: ratio / constant), and the readings of the old rules (backward error of y 1e-12, step_norm 1e-9, relative decrease
    1e-7; y_f itself is untouched by every control, so its old rule at 1e-14 cond + 1e-9 reads 0) are printed next to it."""
    for case, faults, key in ((pair[0], ("ypose",), "E"), (pair[0], ("obs",), "E"), (pair[0], ("strip",), "E"), (pair[1], ("papart",), "T"), (pair[1], ("beta",), "T")):
        c = cpu_case(case)
        A, Bn = c["numpy"]
        n_e = A["n_e"]
        f = {}
        for k in faults:
            # ypose: the reduced coordinate that most landmark rows read; papart: the number of projection observations
            f[k] = {"ypose": int(np.argmax((A["J"][:, n_e:] != 0).sum(0))), "papart": c["w"].a["proj_idx"].size // 3}.get(k, True)
        _, Bm = numpy_route(c["w"], A["r"], A["J"], n_e, c["opt"], f)
        o = judge("%s, %s:" % (case, faults[0]), c["w"], c["opt"], A, Bm, check=False)
        old = _old_rules(c, Bn, Bm)
        caught = [k for k, v in old.items() if v > OLD[k]]
        print("%-44s fails the new rule on %s by %.3g x the constant; old rules: %s -> %s"
              % ("", dict(E="y_e", T="step")[key], o[key] / M[key], "  ".join("%s %.1e" % kv for kv in old.items()),
                 "caught by " + ", ".join(caught) if caught else "none of them sees it"))
        assert o[key] > M[key], (case, faults, o[key])
        if key == "T":
            assert o["C"] > M_C or faults[0] == "beta", (case, faults, "the model cost change carries the wrong |J v|^2 as well")


def test_library_exports_the_step():
    """swf_batch_export_step is exported, bound and documented; the SWF_EXPORT_L sentence (nothing ever read the variable) is gone"""
    import os
    from rtk_visual_inertial_navigation_amd import build, solver
    build.build()
    assert "swf_batch_export_step" in solver.EXPORTED and hasattr(solver.lib(), "swf_batch_export_step") and hasattr(solver.BatchSolver, "export_step")
    assert solver.lib().swf_version() == 113
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "swf_solver.h")).read()
    assert "int swf_batch_export_step(swf_batch* b, int32_t w, double* step);" in hdr and "113: no layout change" in hdr
    for f in (hdr, open(os.path.join(root, "INTEGRATION.md")).read()):
        assert "SWF_EXPORT_L" not in f


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def device_runs(ws, opt):
    """runs A and B of a batch of windows -> list of (A, B) per window"""
    from rtk_visual_inertial_navigation_amd import solver
    out = []
    bs = solver.BatchSolver([w.copy() for w in ws])
    try:
        sms = bs.solve(default_options(step_mode=1), download=False)
        assert all(s.termination == 7 for s in sms)
        with pytest.raises(RuntimeError):
            bs.export_step(0)                       # SWF_E_STATE before any optimising solve
        for i in range(len(ws)):
            r, J = bs.export_jacobian(i)
            g, dg, y = bs.export_vectors(i)
            S, rhs, L = bs.export_reduced(i)
            out.append([dict(r=r, J=J, n_e=bs.dims(i)["n_e"], g=g, diag=dg, rhs=rhs, L=L, y=y, S=S)])
    finally:
        bs.close()
    wb = [w.copy() for w in ws]
    bs = solver.BatchSolver(wb)
    try:
        sms = bs.solve(opt, download=True)
        for i in range(len(ws)):
            row = sms[i].trace[1]
            _, _, y = bs.export_vectors(i)
            S, rhs, _ = bs.export_reduced(i)
            out[i].append(dict(S=S, rhs=rhs, y=y, step=bs.export_step(i), mcc=row.model_cost_change, step_norm=row.step_norm, valid=row.step_is_valid,
                               successful=row.step_is_successful, blocks=[b.copy() for b in nd.blocks_of(wb[i])], cost=row.cost,
                               relative_decrease=row.relative_decrease, radius=row.trust_region_radius))
    finally:
        bs.close()
    return out


def same_bits(B1, B2):
    for k in ("S", "rhs", "y", "step", "mcc", "step_norm", "cost", "relative_decrease", "radius"):
        assert np.array_equal(np.asarray(B1[k]), np.asarray(B2[k])), k
    for a, b in zip(B1["blocks"], B2["blocks"]):
        assert np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def device_case(name):
    wn, kw, branch = sp.CASES[name]
    w = sp.window(wn)
    return (w,) + tuple(device_runs([w], sp.options(**kw))[0])


@gpu
@needs_longdouble
@pytest.mark.parametrize("name", list(sp.CASES))
def test_device_step_componentwise(name):
    """one window alone (the fused k_step_eval, k_post_chol<0>): the whole rule, consistency of the two runs and sensitivity included"""
    wn, kw, branch = sp.CASES[name]
    w, A, B = device_case(name)
    judge("device, %s:" % name, w, sp.options(**kw), A, B, want_branch=branch)


@gpu
@needs_longdouble
@pytest.mark.parametrize("env", sp.KNOBS, ids=[list(e)[0] for e in sp.KNOBS])
def test_device_knobs_componentwise_and_bit_identical(env, monkeypatch):
    """the separate k_dogleg launch, the two-pass flow and the batch kernels forced on one window (the knobs are read when the batch is
    created): the rule, and the bits of the default launch"""
    for k in ("SWF_NO_STEP_FUSE", "SWF_NO_SPEC_EVAL", "SWF_NO_LAT_FUSE"):
        monkeypatch.delenv(k, raising=False)
    ref = {n: device_case(n) for n in sp.KNOB_CASES}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n in sp.KNOB_CASES:
        wn, kw, branch = sp.CASES[n]
        w = sp.window(wn)
        A, B = device_runs([w], sp.options(**kw))[0]
        judge("device, %s, %s:" % (n, env), w, sp.options(**kw), A, B, want_branch=branch)
        same_bits(B, ref[n][2])


def _batch(n):
    ws = [sp.window(k) for k in sp.BATCH_HEAD]
    return [ws[i % len(ws)] for i in range(n)], [sp.BATCH_HEAD[i % len(ws)] for i in range(n)]


@gpu
@needs_longdouble
def test_device_batch_33_componentwise_and_bit_identical():
    """33 windows in one batch (the batch path): every distinct window and the last judged, each with the bits of the window solved alone"""
    ws, names = _batch(sp.BATCH_N)
    runs = device_runs(ws, sp.options())
    alone = {n: device_runs([sp.window(n)], sp.options())[0] for n in sp.BATCH_HEAD}
    for i in list(range(len(sp.BATCH_HEAD))) + [sp.BATCH_N - 1]:
        judge("device, batch of 33, window %d (%s):" % (i, names[i]), ws[i], sp.options(), *runs[i])
        same_bits(runs[i][1], alone[names[i]][1])


@gpu
@needs_longdouble
def test_device_batch_beyond_the_cu_count_componentwise_and_bit_identical():
    """(CU count + 4) windows: k_post_chol<1> and <2> run only when n_win >= n_cu.  Eight sampled windows plus the first and the last."""
    n = multi_processor_count() + 4
    ws, names = _batch(n)
    runs = device_runs(ws, sp.options())
    alone = {k: device_runs([sp.window(k)], sp.options())[0] for k in sp.BATCH_HEAD}
    pick = sorted(set([0, n - 1] + [int(i) for i in np.random.default_rng(5).choice(np.arange(1, n - 1), 8, replace=False)]))
    for i in pick:
        judge("device, batch of %d, window %d (%s):" % (n, i, names[i]), ws[i], sp.options(), *runs[i])
        same_bits(runs[i][1], alone[names[i]][1])


@gpu
@needs_longdouble
@pytest.mark.parametrize("name", ["n_loc_over_1024", "n_loc_over_4096"])
def test_device_large_window_strided_loops(name, monkeypatch):
    """n_loc > 1024 under SWF_NO_LAT_FUSE: the strided tail loops of k_dogleg<4, 2> (4 x 256 local dimensions in registers).  n_loc > 4096
    (x_n beyond the fused step kernel's LDS candidate, so the plan routes the window alone to a k_dogleg<16, 4> launch): its tail loop
    without the knob, <4, 2>'s with it.  The knob's run is judged; the default launch must give the same bits."""
    monkeypatch.setenv("SWF_NO_LAT_FUSE", "1")
    w = sp.window(name)
    A, B = device_runs([w], sp.options())[0]
    assert A["g"].size > (1024 if name == "n_loc_over_1024" else 4096)
    judge("device, %s, SWF_NO_LAT_FUSE:" % name, w, sp.options(), A, B)
    monkeypatch.delenv("SWF_NO_LAT_FUSE")
    same_bits(B, device_runs([w], sp.options())[0][1])
