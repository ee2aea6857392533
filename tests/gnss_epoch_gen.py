"""Inputs for the single-epoch GNSS solve (swf_gnss_epoch_solve_batch) whose decisions are decisive by construction.

Geometry: a base on the WGS84 ellipsoid, the rover within 1 km of it, satellites 2.2e7 m away at elevations of 25 to 85 degrees over
three systems.  Receiver clocks up to +-3e5 m, the drift up to +-300 m/s.  A satellite gives up to five records: RTK phase and code (clock
slot sys * 2), rover-only code and phase (slot 6 + sys * 2) and Doppler (slot 12), shuffled; an epoch of n records keeps the first n.
Observations are the model at the truth plus noise of one sigma = 1 / w (clipped at 3 sigma), so weighted residuals are of order one.
A free ambiguity carries a wrong N (the operator must not use it); a constant one carries the truth.
Presets: `seed` starts at the true pose with clocks up to 30 m off and holds [pos, vel] constant, two iterations; `first_fix` starts
4 km off with zero velocity and zero clocks and frees everything, twenty iterations.  (The Sagnac term is not differentiated, so the
iteration contracts by ~6e-6 per step once it is close: from 4 km the steps are ~1e5 (clocks), ~0.4 and ~2e-6 m, clear of step_tol =
1e-4 by more than a factor of ten on either side; from 10 km the third step is ~1.4e-5 and is not.)  Epochs of fewer than 8 satellites are deficient
for the first fix by design (0, 1 and 2 records), and `deficient=True` gives 4 satellites over three systems without Doppler rows."""
import numpy as np

import np_gnss_epoch as nge

LAMS = (0.1903, 0.1920, 0.2548)
A_WGS, E2_WGS = 6378137.0, 6.69437999014e-3


def _ecef(lat, lon):
    nu = A_WGS / np.sqrt(1 - E2_WGS * np.sin(lat) ** 2)
    return np.array([nu * np.cos(lat) * np.cos(lon), nu * np.cos(lat) * np.sin(lon), nu * (1 - E2_WGS) * np.sin(lat)])


def _enu(lat, lon):
    return np.array([[-np.sin(lon), np.cos(lon), 0.0],
                     [-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)],
                     [np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)]])


def gen_epoch(seed, n, preset="seed", p_free=0.3, kinds=(0, 1, 2, 3, 4), deficient=False, n_sat=None, all_free=False, none_free=False):
    """One epoch of n records: dict(pos, vel, base, clock [13], mode, clk_const, dat [n][10], rec [n][4], truth=(pos, vel, clock))."""
    rng = np.random.default_rng(seed)
    lat, lon = rng.uniform(-1.2, 1.2), rng.uniform(-np.pi, np.pi)
    base = _ecef(lat, lon)
    pos_t, vel_t = rng.uniform(-500.0, 500.0, 3), rng.uniform(-15.0, 15.0, 3)
    clock_t = np.concatenate([rng.uniform(-3e5, 3e5, 12), rng.uniform(-300.0, 300.0, 1)])
    ns = n_sat if n_sat is not None else (4 if deficient else max((n + len(kinds) - 1) // len(kinds), 0))
    az, el = rng.uniform(0, 2 * np.pi, ns), np.deg2rad(rng.uniform(25.0, 85.0, ns))
    if ns >= 4:                                                           # spread in azimuth and elevation: a healthy geometry
        az = (np.arange(ns) * 2 * np.pi / ns + rng.uniform(0, 0.3, ns)) % (2 * np.pi)
        el = np.deg2rad(np.where(np.arange(ns) % 2 == 0, rng.uniform(25.0, 45.0, ns), rng.uniform(55.0, 85.0, ns)))
    u = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], 1) @ _enu(lat, lon)
    sat = base[None, :] + 2.2e7 * u
    satvel = rng.normal(0.0, 2.0e3, (ns, 3))
    sys_ = np.arange(ns) % 3 if not deficient else np.array([0, 0, 1, 2])
    rows = []
    for i in range(ns):
        s2 = np.sin(el[i]) ** 2
        for k in kinds:
            slot = (sys_[i] * 2, sys_[i] * 2, 6 + sys_[i] * 2, 6 + sys_[i] * 2, 12)[k]
            w = (s2 / 0.004, s2 / 0.4, s2 / 0.9, s2 / 0.006, s2 / 0.06)[k] * rng.uniform(0.7, 1.4)
            rows.append((i, k, slot, w))
    rows = [rows[j] for j in rng.permutation(len(rows))][:n]
    assert len(rows) == n, "not enough satellites for n records"
    dat, rec = np.zeros((n, nge.DOUBLES)), np.zeros((n, 4), np.int32)
    xg = pos_t + base
    for j, (i, k, slot, w) in enumerate(rows):
        lam = LAMS[sys_[i]]
        N = float(np.round(rng.uniform(-2000.0, 2000.0)))
        phase = k in (nge.RTK_PHASE, nge.SPP_PHASE)
        free = phase and not none_free and (all_free or rng.random() < p_free)
        d = np.concatenate([sat[i], satvel[i], [0.0, w, lam if phase else 1.0, N if phase else 0.0]])
        q = np.array([[k, slot, 0, 0]], np.int32)
        r0 = nge.evaluate(d[None, :], q, xg, vel_t, clock_t)[0][0] / w             # the model at the truth with obs = 0
        noise = float(np.clip(rng.normal(), -3, 3)) / w
        d[6] = (-r0 + noise) if k == nge.DOPPLER else (r0 - noise)                 # Doppler enters with +obs, the ranges with -obs
        if free:
            d[9] = N + float(np.round(rng.uniform(-5e4, 5e4)))
        dat[j], rec[j] = d, (k, slot, nge.AMB_FREE if free else 0, 0)
    if preset == "seed":
        pos0, vel0 = pos_t + rng.uniform(-0.02, 0.02, 3), vel_t + rng.uniform(-0.01, 0.01, 3)
        clock0 = clock_t + rng.uniform(5.0, 30.0, 13) * rng.choice([-1, 1], 13)
        mode = 0
    else:
        v = rng.normal(size=3)
        pos0, vel0, clock0 = pos_t + 4.0e3 * v / np.linalg.norm(v), np.zeros(3), np.zeros(13)
        mode = nge.FREE_POS | nge.FREE_VEL
    return dict(pos=pos0, vel=vel0, base=base, clock=clock0, mode=int(mode), clk_const=0, dat=dat, rec=rec, truth=(pos_t, vel_t, clock_t))


def pack(epochs):
    """(first, pos, vel, base, clock, mode, clk_const, dat, rec) of a list of epochs, as swf_gnss_epoch_solve_batch takes them."""
    first = np.zeros(len(epochs) + 1, np.int32)
    first[1:] = np.cumsum([e["dat"].shape[0] for e in epochs])
    cat = lambda k, w, t: np.ascontiguousarray(np.concatenate([np.asarray(e[k]).reshape(-1, w) for e in epochs]) if epochs else np.zeros((0, w)), t)
    return (first, cat("pos", 3, np.float64), cat("vel", 3, np.float64), cat("base", 3, np.float64), cat("clock", nge.CLOCKS, np.float64),
            np.array([e["mode"] for e in epochs], np.int32), np.array([e["clk_const"] for e in epochs], np.int32),
            cat("dat", nge.DOUBLES, np.float64), cat("rec", 4, np.int32))
