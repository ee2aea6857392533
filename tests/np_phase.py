"""numpy referee of the pre-fit carrier-phase screen (swf_phase_screen_batch): an independent restatement of the first half of
SWFOptimization::GnssPreprocess (R/swf/swf_gnss.cpp:337-499) over the operator's flat records, vectorised over all epochs of a call.

  residuals(...)   the un-weighted RTKCarrierPhaseFactor at the predicted pose, in float64 or longdouble, in two legitimate
                   operation orders ("factor": as the factor adds, left to right; "alt": the sums regrouped)
  screen(...)      residuals, medians (sorted[size / 2], ties by record index, NaN last), flags and the compacted reset list
  margins(...)     how far every decision of an input sits from its threshold"""
import numpy as np

CLIGHT = 299792458.0
OMGE = 7.2921151467E-5
DOUBLES, GROUPS, NMAX = 9, 6, 256
RTK, SPP = 0, 1
HAS_AMB, CONTINUING = 1, 2
GATE_RTK, GATE_SPP, RESET_ALL = 1, 2, 4
MASKED, SLIP_RESIDUAL, SLIP_CODE, NEW_AMB = 1, 2, 4, 8
AZELMIN = 25.0 * np.pi / 180.0
CODE_LIMIT = 10.0


def _layout(first, rec):
    first = np.asarray(first, np.int64)
    E = first.size - 1
    ep = np.repeat(np.arange(E), np.diff(first))
    rec = np.asarray(rec, np.int64).reshape(-1, 4)
    return first, E, ep, rec


def residuals(first, pos, base, dat, rec, el_min=AZELMIN, dtype=np.float64, order="factor"):
    """r [n]: distance(pos + base, sat) - N lam - L + dt for a record with HAS_AMB (L = 0 when masked), 0 without."""
    first, E, ep, rec = _layout(first, rec)
    d = np.asarray(dat, np.float64).reshape(-1, DOUBLES)
    has = (rec[:, 2] & HAS_AMB) != 0
    T = dtype
    xg = (np.asarray(pos, np.float64).reshape(-1, 3).astype(T) + np.asarray(base, np.float64).reshape(-1, 3).astype(T))[ep]
    sat = d[:, 0:3].astype(T)
    L = np.where(d[:, 5] < el_min, 0.0, d[:, 3]).astype(T)
    lam = d[:, 4].astype(T)
    N = np.where(has, d[:, 7], 0.0).astype(T)
    dt = np.where(has, d[:, 8], 0.0).astype(T)
    e = xg - sat
    if order == "factor":
        rho = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        dist = rho + T(OMGE) * (sat[:, 0] * xg[:, 1] - sat[:, 1] * xg[:, 0]) / T(CLIGHT)
        r = dist - N * lam - L + dt
    elif order == "alt":
        rho = np.sqrt(e[:, 2] * e[:, 2] + (e[:, 1] * e[:, 1] + e[:, 0] * e[:, 0]))
        sag = (T(OMGE) / T(CLIGHT)) * (sat[:, 0] * xg[:, 1]) - (T(OMGE) / T(CLIGHT)) * (sat[:, 1] * xg[:, 0])
        r = (rho + dt) - (L + N * lam) + sag
    else:
        raise ValueError(order)
    return np.where(has, r, T(0.0))


def bracket(first, pos, base, dat, rec):
    """|xg| + |sat| + |N lam| + |L_lam| + |dt| per record: what 2^-52 multiplies in the tolerance of r and med."""
    first, E, ep, rec = _layout(first, rec)
    d = np.asarray(dat, np.float64).reshape(-1, DOUBLES)
    has = (rec[:, 2] & HAS_AMB) != 0
    xg = (np.asarray(pos, np.float64).reshape(-1, 3) + np.asarray(base, np.float64).reshape(-1, 3))[ep]
    return (np.linalg.norm(xg, axis=1) + np.linalg.norm(d[:, 0:3], axis=1) + np.abs(np.where(has, d[:, 7], 0.0) * d[:, 4])
            + np.abs(d[:, 3]) + np.abs(np.where(has, d[:, 8], 0.0)))


def upper_median(values):
    """sorted[size / 2] with a NaN last (one set; NaN for an empty one)."""
    v = np.asarray(values)
    if v.size == 0:
        return np.nan
    o = np.lexsort((np.arange(v.size), np.where(np.isnan(v), 0.0, v), np.isnan(v)))
    return v[o[v.size // 2]]


def screen(first, pos, base, mode, dat, rec, el_min=AZELMIN, dtype=np.float64, order="factor", detail=False):
    first, E, ep, rec = _layout(first, rec)
    d = np.asarray(dat, np.float64).reshape(-1, DOUBLES)
    n = d.shape[0]
    mode = np.asarray(mode, np.int64).ravel()
    kind, grp, st, pt = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    has, cont = (st & HAS_AMB) != 0, (st & CONTINUING) != 0
    masked = d[:, 5] < el_min
    r = residuals(first, pos, base, d, rec, el_min, dtype, order)
    elig = has & cont
    # ---- medians: sort the members by (epoch, set, NaN last, value, record index); the element of rank cnt / 2 of every run
    key = ep * (2 * GROUPS) + kind * GROUPS + grp
    sel = np.nonzero(elig)[0]
    rs = r[sel]
    isn = np.isnan(rs)
    o = np.lexsort((sel, np.where(isn, 0.0, rs), isn, key[sel]))
    cnt = np.bincount(key[sel], minlength=E * 2 * GROUPS).astype(np.int64)
    start = np.cumsum(cnt) - cnt
    med = np.full(E * 2 * GROUPS, np.nan, dtype)
    nz = cnt > 0
    med[nz] = rs[o][start[nz] + cnt[nz] // 2]
    # ---- decisions
    lam = d[:, 4].astype(dtype)
    rtk = kind == RTK
    m_e = mode[ep] if n else np.zeros(0, np.int64)
    gate = elig & ~masked & np.where(rtk, (m_e & GATE_RTK) != 0, (m_e & GATE_SPP) != 0)
    with np.errstate(invalid="ignore"):
        dev = np.abs(r - med[key])
        thr = np.where(rtk, lam / 2, lam)
        slipr = gate & (dev > thr)
        s = np.sin(d[:, 5].astype(dtype))
        codev = np.abs((d[:, 3].astype(dtype) + np.where(has, d[:, 7], 0.0).astype(dtype) * lam) - d[:, 6].astype(dtype)) * s * s
        slipc = gate & ~rtk & (codev > CODE_LIMIT)
    c3 = rtk & slipr
    pc3 = np.zeros(n, bool)
    hp = ~rtk & (pt >= 0)
    pc3[hp] = c3[first[ep[hp]] + pt[hp]]
    new = ~masked & (~elig | np.where(rtk, slipr | ((m_e & RESET_ALL) != 0), pc3 | slipc | slipr))
    flags = np.where(masked, MASKED, slipr * SLIP_RESIDUAL | slipc * SLIP_CODE | new * NEW_AMB).astype(np.uint8)
    # ---- the reset list: within-epoch indices of the NEW_AMB records, ascending, from first[e]; -1 behind them
    reset = np.full(n, -1, np.int32)
    n_reset = np.bincount(ep[new], minlength=E).astype(np.int32) if n else np.zeros(E, np.int32)
    if n:
        c = np.cumsum(new)
        before = np.concatenate([[0], c])[first[:-1]]            # NEW_AMB records ahead of each epoch
        w = np.nonzero(new)[0]
        reset[first[ep[w]] + (c[w] - 1 - before[ep[w]])] = (w - first[ep[w]]).astype(np.int32)
    out = dict(r=r, flags=flags, med=med.reshape(E, 2, GROUPS), cnt=cnt.astype(np.int32).reshape(E, 2, GROUPS), reset=reset, n_reset=n_reset)
    if detail:
        out.update(gate=gate, dev=dev, thr=thr, codev=codev, rtk=rtk, masked=masked, elig=elig)
    return out


def margins(first, pos, base, mode, dat, rec, el_min=AZELMIN):
    """(smallest | |r - med| - threshold | over the gated records, smallest | code - 10 | over the gated SPP records, smallest
    |el - el_min|), by the longdouble referee; inf where there is no such record."""
    q = screen(first, pos, base, mode, dat, rec, el_min, dtype=np.longdouble, detail=True)
    g = q["gate"]
    a = np.abs(q["dev"][g] - q["thr"][g])
    gs = g & ~q["rtk"]
    b = np.abs(q["codev"][gs] - CODE_LIMIT)
    el = np.abs(np.asarray(dat, np.float64).reshape(-1, DOUBLES)[:, 5] - el_min)
    f = lambda v: float(v.min()) if v.size else float("inf")
    return f(a), f(b), f(el)
