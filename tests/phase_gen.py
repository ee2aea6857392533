"""Inputs for the pre-fit carrier-phase screen whose decisions are decisive by construction.

Geometry: satellites at 2.0-2.6e7 m, |base| ~ 6.4e6 m, |pos| <= 1e3 m; lam in {0.1903, 0.1920, 0.2548}.  A clean residual is a per-set
offset plus noise of sigma = 3 mm (clipped at 10 mm).  What is injected:
  - phase slips of k whole cycles, |k| >= 1 (RTK) or >= 2 (SPP), never half-integers: a slipped record sits >= lam - 20 mm (RTK) or
    >= 2 lam - 20 mm (SPP) from a clean median, against thresholds of lam / 2 and lam; a clean one <= 20 mm;
  - code-minus-phase offsets, after the sin^2(el) factor, of < 5 m or > 20 m against the limit of 10 m;
  - masked records (el < 25 deg; every el is >= 1 deg away from the mask);
  - at most floor((cnt - 1) / 2) slipped or masked members per median set, so the median is a clean member whatever side they fall on.
Records without HAS_AMB carry NaN in N and dt (the operator must not use them)."""
import numpy as np

import np_phase as nph

LAMS = (0.1903, 0.1920, 0.2548)


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def gen_epoch(seed, n, mode=nph.GATE_RTK | nph.GATE_SPP, p_noamb=0.08, p_stale=0.08, p_spp=0.45, p_bad=0.35, p_code=0.2, tie=False,
              groups=None):
    """One epoch of n records: dict(pos [3], base [3], mode, dat [n][9], rec [n][4], slipped [n], code_slip [n])."""
    rng = np.random.default_rng(seed)
    base = _unit(rng, 1)[0] * 6.4e6
    pos = rng.uniform(-500.0, 500.0, 3)
    xg = pos + base
    kind = (rng.random(n) < p_spp).astype(np.int64)
    grp = rng.integers(0, nph.GROUPS, n) if groups is None else rng.choice(np.asarray(groups), n)
    u = rng.random(n)
    st = np.where(u < p_noamb, 0, np.where(u < p_noamb + p_stale, nph.HAS_AMB, nph.HAS_AMB | nph.CONTINUING))
    st = np.where(rng.random(n) < 0.03, st & nph.CONTINUING, st)          # a few with the CONTINUING bit alone (no ambiguity)
    has, elig = (st & nph.HAS_AMB) != 0, st == (nph.HAS_AMB | nph.CONTINUING)
    sat = _unit(rng, n) * rng.uniform(2.0e7, 2.6e7, (n, 1))
    lam = np.array(LAMS)[grp // 2]
    el = np.deg2rad(rng.uniform(30.0, 85.0, n))
    N = np.round(rng.uniform(-2000.0, 2000.0, n))
    set_id = kind * nph.GROUPS + grp
    dt_set = rng.uniform(-100.0, 100.0, 2 * nph.GROUPS)
    off_set = rng.uniform(-5.0, 5.0, 2 * nph.GROUPS)
    dt = dt_set[set_id]
    noise = np.clip(rng.normal(0.0, 3e-3, n), -1e-2, 1e-2)
    e = xg - sat
    dist = np.sqrt((e * e).sum(1)) + nph.OMGE * (sat[:, 0] * xg[1] - sat[:, 1] * xg[0]) / nph.CLIGHT
    Nv, dtv = np.where(has, N, 0.0), np.where(has, dt, 0.0)
    L = dist - Nv * lam + dtv - (off_set[set_id] + noise)                # clean: r = offset of the set + noise
    # ---- slips and masks, within the budget of every median set
    slipped, masked = np.zeros(n, bool), np.zeros(n, bool)
    for s in range(2 * nph.GROUPS):
        mem = np.nonzero(elig & (set_id == s))[0]
        budget = (mem.size - 1) // 2 if mem.size else 0
        bad = rng.permutation(mem)[:rng.binomial(budget, p_bad) if budget else 0]
        for i in bad:
            if rng.random() < 0.3:
                masked[i] = True
            else:
                slipped[i] = True
    masked |= ~elig & (rng.random(n) < 0.1)                               # outside the median sets: freely
    k = rng.integers(1, 4, n) * rng.choice([-1, 1], n)
    k = np.where(kind == nph.SPP, np.sign(k) * (np.abs(k) + 1), k)        # |k| >= 2 for SPP
    L = L + np.where(slipped, k * lam, 0.0)
    el = np.where(masked, np.deg2rad(rng.uniform(5.0, 24.0, n)), el)
    # ---- code minus phase: P = (L + N lam) + offset / sin^2(el)
    code_slip = (kind == nph.SPP) & (rng.random(n) < p_code)
    c_off = np.where(code_slip, rng.uniform(20.5, 40.0, n), rng.uniform(0.0, 4.5, n)) * rng.choice([-1, 1], n)
    P = (L + Nv * lam) + c_off / np.sin(el) ** 2
    # ---- partners: an SPP record names an RTK record of its group (if the epoch has one), most of the time
    pt = np.full(n, -1, np.int64)
    for i in np.nonzero(kind == nph.SPP)[0]:
        cand = np.nonzero((kind == nph.RTK) & (grp == grp[i]))[0]
        if cand.size and rng.random() < 0.8:
            pt[i] = rng.choice(cand)
    dat = np.column_stack([sat, L, lam, el, P, np.where(has, N, np.nan), np.where(has, dt, np.nan)]) if n else np.zeros((0, nph.DOUBLES))
    rec = np.column_stack([kind, grp, st, pt]).astype(np.int32) if n else np.zeros((0, 4), np.int32)
    if tie and n >= 2:                                                    # two members of one set with bit-identical inputs
        mem = np.nonzero(elig & ~masked & ~slipped)[0]
        pairs = [(a, b) for a in mem for b in mem if a < b and set_id[a] == set_id[b]]
        assert pairs, "no set with two clean members to tie"
        a, b = pairs[0]
        dat[b] = dat[a]
        rec[b, 3] = rec[a, 3]
        code_slip[b] = code_slip[a]
    return dict(pos=pos, base=base, mode=int(mode), dat=np.ascontiguousarray(dat), rec=np.ascontiguousarray(rec),
                slipped=slipped, code_slip=code_slip)


def pack(epochs):
    """(first, pos, base, mode, dat, rec) of a list of epochs, as swf_phase_screen_batch takes them."""
    first = np.zeros(len(epochs) + 1, np.int32)
    first[1:] = np.cumsum([e["dat"].shape[0] for e in epochs])
    cat = lambda k, w, t: np.ascontiguousarray(np.concatenate([e[k].reshape(-1, w) for e in epochs]) if epochs else np.zeros((0, w)), t)
    return (first, cat("pos", 3, np.float64), cat("base", 3, np.float64), np.array([e["mode"] for e in epochs], np.int32),
            cat("dat", nph.DOUBLES, np.float64), cat("rec", 4, np.int32))
