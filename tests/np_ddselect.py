"""Referee of the double-difference pair selection (swf_dd_select_batch): FindReferenceSatellites and the D3 loop of
SWFOptimization::LambdaSearch (R/swf/swf_lambda.cpp:8-53, 118-188) in plain Python floats, one statement per line of the
reference's logic.  Every operation is a subtraction, a round, a fabs, an addition or a comparison, all exact or correctly rounded
in IEEE double: the device's results are compared with these for equality."""
import math

OK, TOO_FEW, OVERFLOW, NONFINITE = 0, 1, 2, 3
SKIPPED, REFERENCE, PAIRED, GATED_OUT, NO_REFERENCE = 0, 1, 2, 3, 4
NMAX_PAIRS = 64


def c_round(x):
    """C round(): halves away from zero (not numpy.round, not floor(x + 0.5)).  x - trunc(x) is exact."""
    r = float(math.trunc(x))
    if abs(x - r) >= 0.5:
        r += math.copysign(1.0, x)
    return r


def frac(d):
    return abs(d - c_round(d))


def select(epochs, y, gate):
    """epochs: newest first, each a list of (class, t) in observation order; y: the tail's float values; gate: the window's gate.
    Returns dict(pairs, n_pairs, last_count, last_ref_count, info, refs [epochs][6], cost [observations], role [observations]) with
    cost / role concatenated over the epochs in order."""
    y = [float(v) for v in y]
    tail = len(y)
    n_obs = sum(len(e) for e in epochs)
    if any(not math.isfinite(y[t]) for e in epochs for _, t in e):
        # every ambiguity is a candidate where it first appears; the reference would sort NaN costs: nothing is reported
        return dict(pairs=[], n_pairs=0, last_count=0, last_ref_count=0, info=NONFINITE, refs=[[-1] * 6 for _ in epochs],
                    cost=[-1.0] * n_obs, role=[SKIPPED] * n_obs)
    used = set()
    pairs = []
    last_count = last_ref_count = 0
    refs, cost, role = [], [], []
    for ei, e in enumerate(epochs):
        ref = [-1] * 6
        ecost = [-1.0] * len(e)
        for c in range(6):                                             # FindReferenceSatellites
            cand = [k for k, (ck, t) in enumerate(e) if ck == c and t not in used]
            if not cand:
                continue
            for j in cand:
                acc = 0.0
                for i in cand:
                    s = y[e[i][1]] - y[e[j][1]]
                    acc += abs(s - c_round(s))
                ecost[j] = acc
            lo = min(ecost[j] for j in cand)
            for j in cand:                                             # :41-46: every equal entry overwrites, the last one stays
                if ecost[j] == lo:
                    ref[c] = j
        if ei == 0:
            last_ref_count = sum(1 for r in ref if r >= 0)
        for k, (c, t) in enumerate(e):
            if ref[c] < 0:
                role.append(NO_REFERENCE)
                continue
            if t in used:
                role.append(SKIPPED)
                continue
            if k == ref[c]:
                role.append(REFERENCE)
                continue
            used.add(t)                                                # before the gate
            d = y[t] - y[e[ref[c]][1]]
            if frac(d) < gate:
                pairs.append((t, e[ref[c]][1]))
                role.append(PAIRED)
                if ei == 0:
                    last_count += 1
            else:
                role.append(GATED_OUT)
        refs.append(ref)
        cost.extend(ecost)
    if len(pairs) > NMAX_PAIRS:
        info, rep = OVERFLOW, []
    else:
        go = tail >= 6 and last_count + last_ref_count >= 6 and last_count >= 4 and len(pairs) >= 4
        info, rep = (OK if go else TOO_FEW), pairs
    return dict(pairs=rep, n_pairs=len(rep), last_count=last_count, last_ref_count=last_ref_count, info=info, refs=refs, cost=cost, role=role)
