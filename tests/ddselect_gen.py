"""Inputs for the double-difference pair selection (swf_dd_select_batch): windows of epochs (newest first) of (class, tail
coordinate) observations over a tail of float ambiguities drawn as integer + fraction, so that the gate passes some differences
and rejects others and both SWF_DDSEL_OK and SWF_DDSEL_TOO_FEW occur."""
import numpy as np

import np_ddselect as nd

SIZES = (0, 1, 2, 63, 64, 65, 130, 256)          # observations per epoch: the 64-record chunks and the strided j change here
EPOCHS = (0, 1, 2, 5)
CLASS_MODES = ("one", "six", "single")           # one class only; all six; all six, one of them with a single ambiguity


def _classes(rng, T, mode):
    if mode == "one":
        return np.full(T, int(rng.integers(0, 6)))
    cls = rng.integers(0, 6, T)
    if mode == "single":
        lone = int(rng.integers(0, 6))
        cls[cls == lone] = (lone + 1) % 6
        cls[int(rng.integers(0, T))] = lone
    return cls


def make_window(rng, sizes, mode, gate, noise=0.05, outliers=0.15, spread=40, extra=6):
    """A window whose epoch k has sizes[k] observations.  y = integer + a per-class fraction + noise; `outliers` of the ambiguities
    get a uniform fraction instead."""
    T = max([6] + [int(s) for s in sizes]) + extra
    cls = _classes(rng, T, mode)
    base = rng.uniform(-0.5, 0.5, 6)
    y = rng.integers(-spread, spread + 1, T) + base[cls] + noise * rng.standard_normal(T)
    out = rng.random(T) < outliers
    y[out] = rng.integers(-spread, spread + 1, int(out.sum())) + rng.uniform(-0.5, 0.5, int(out.sum()))
    epochs = []
    for n in sizes:
        ts = rng.permutation(T)[:int(n)]
        epochs.append([(int(cls[t]), int(t)) for t in ts])
    return dict(epochs=epochs, y=y.astype(np.float64), gate=float(gate))


def _specials(rng):
    out = {}
    # every candidate of the second epoch is already used: it repeats the first epoch's paired and gated-out observations
    w = make_window(rng, [24], "six", 0.2)
    r = nd.select(w["epochs"], w["y"], w["gate"])
    w["epochs"].append([o for o, rl in zip(w["epochs"][0], r["role"]) if rl in (nd.PAIRED, nd.GATED_OUT)])
    out["second_epoch_all_used"] = w
    # a deliberate tie: three ambiguities of one class with the same value (and the two-candidate class, which always ties)
    w = make_window(rng, [12, 9], "six", 1.4)
    c0 = int(np.bincount([c for c, _ in w["epochs"][0]]).argmax())
    same = [t for c, t in w["epochs"][0] if c == c0][:3]
    w["y"][same] = w["y"][same[0]]
    out["tie"] = w
    # gate 0.2, fractional parts at 0.2 +- 1e-3 around integers of a few hundred: ulp(y) ~ 1e-13, so is the rounding of a difference
    T = 40
    cls = np.arange(T) % 2
    frac = np.array([0.0, 0.0, 0.2 - 1e-3, 0.2 + 1e-3, -0.2 + 1e-3, -0.2 - 1e-3, 0.4 - 2e-3, 0.4 + 2e-3])[rng.integers(0, 8, T)]
    y = rng.integers(-900, 901, T).astype(np.float64) + frac
    ep = [[(int(cls[t]), int(t)) for t in rng.permutation(T)[:n]] for n in (30, 22)]
    out["gate_edge"] = dict(epochs=ep, y=y, gate=0.2)
    # exactly 64 pairs, and 65
    for name, n in (("pairs64", 65), ("pairs65", 66)):
        yy = rng.integers(-50, 51, n + 3) + 0.01 * rng.standard_normal(n + 3)
        out[name] = dict(epochs=[[(2, t) for t in range(n)]], y=yy, gate=1.4)
    w = make_window(rng, [20, 10], "six", 1.4)
    w["y"][w["epochs"][1][3][1]] = np.nan
    out["nan"] = w
    yy = rng.integers(-9, 10, 5) + 0.01 * rng.standard_normal(5)
    out["tail5"] = dict(epochs=[[(1, t) for t in range(5)]], y=yy, gate=1.4)
    return out


def mixed_batch(seed=2024):
    """About 300 windows: SIZES x EPOCHS x CLASS_MODES three times over (the first epoch has the size, the older ones any of SIZES),
    gates of 1.4 and 0.2, and the special windows.  Returns (windows, {special name: index})."""
    rng = np.random.default_rng(seed)
    ws = []
    for n in SIZES:
        for ne in EPOCHS:
            for mode in CLASS_MODES:
                for rep in range(3):
                    sizes = [n] + [int(rng.choice(SIZES)) for _ in range(ne - 1)] if ne else []
                    ws.append(make_window(rng, sizes, mode, 0.2 if (len(ws) % 3 == 0) else 1.4))
    # five epochs at the largest sizes
    ws.append(make_window(rng, [256, 130, 256, 65, 256], "six", 1.4))
    ws.append(make_window(rng, [130, 256, 64, 130, 2], "single", 0.2))
    sp = _specials(rng)
    idx = {}
    for k, w in sp.items():
        idx[k] = len(ws)
        ws.append(w)
    return ws, idx
