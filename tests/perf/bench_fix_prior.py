"""Time fix and hold on the device (swf_batch_fix_prior, swf_batch_install_fixed_prior) against what the library offered before for
the same result, for 1, 64 and 512 RTK windows whose prior keeps the ambiguities (tests/fixprior_gen.py: K = 5, F = 24, S = 12:
a 27-dimension prior, 11 double differences).
   python tests/perf/bench_fix_prior.py [reps]
Per batch size (warm, median of `reps`):
  fix_ms            HIP events on the batch stream around swf_batch_fix_prior (host-side row checks, the table upload, k_fix_prior)
  fix_install_ms    the same around swf_batch_fix_prior + swf_batch_install_fixed_prior
  fetch_ms          swf_batch_get_fixed_prior for every window after a fix (one bulk copy per array, then host reads)
and the path a caller had before:
  get_fix_ms        swf_batch_get_ambiguity_fix for every window
  referee_ms        the numpy closed form + eigen root per window (tests/np_fixprior.py)
  rebuild_ms        swf_batch_destroy + swf_batch_create with the new priors
  old_path_ms       their sum
Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fixprior_gen as fg
import np_fixprior as nf
from rtk_visual_inertial_navigation_amd import solver
from rtk_visual_inertial_navigation_amd.flat import default_options

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
S, DISTINCT = 12, 8
lib = solver.lib()
PAIRS = [(i, 0) for i in range(1, S)]


def device_ms(fn, reps):
    ts = []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1))
    return float(np.median(ts))


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


out = dict(reps=REPS, S=S, prior_dim=15 + S)
base = [fg.make_fix_window(K=5, F=24, S=S, seed=300 + i) for i in range(DISTINCT)]
for W in (1, 64, 512):
    ws = [base[i % DISTINCT].copy() for i in range(W)]
    bs = solver.BatchSolver(ws)                      # the default stream: torch's events bracket its work
    bs.solve(default_options())
    bs.tail_covariance()
    res = bs.ambiguity_search([PAIRS] * W)
    bs.sync()
    h = bs._h

    def fix():
        assert lib.swf_batch_fix_prior(h, None, None, None, 1, 1, C.c_double(fg.ISTD), C.c_double(1e-8), 0) == 0, lib.swf_last_error()

    def fix_install():
        fix()
        assert lib.swf_batch_install_fixed_prior(h) == 0

    fix_ms = device_ms(fix, REPS)

    def fetch():
        fix(); bs.sync()
        t0 = time.perf_counter()
        r = [bs.get_fixed_prior(w) for w in range(W)]
        return (time.perf_counter() - t0) * 1e3, r
    fetch_ms, fixed = fetch()
    # install rewrites the priors: time it last, on a state whose search results stay valid (an install does not invalidate them)
    fix_install_ms = device_ms(fix_install, REPS)

    # ---- the path a caller had before
    def get_fix():
        F, s_, r_, fx = np.zeros(2 * (S - 1)), np.zeros(2), np.zeros(2), C.c_int32()
        _pd = C.POINTER(C.c_double)
        for w in range(W):
            assert lib.swf_batch_get_ambiguity_fix(h, C.c_int32(w), F.ctypes.data_as(_pd), s_.ctypes.data_as(_pd), r_.ctypes.data_as(_pd),
                                                   C.byref(fx), None, None, None, None) == 0
    get_fix_ms = host_ms(get_fix, max(3, REPS // 10))
    sizes = [7, 9] + [1] * S

    def referee():
        for w in range(W):
            win = ws[w]
            dim = 15 + S
            J = win.a["prior_J"].reshape(dim, dim)
            x = np.concatenate([win.a["pose"].reshape(-1, 7)[0], win.a["sb"].reshape(-1, 9)[0], np.zeros(S)])
            r = win.a["prior_r0"] + J @ nf.prior_dx(x, win.a["prior_x0"], sizes)
            rows = [(15, 0, 0.0)] + [(15 + a, 0, float(np.floor(res[w]["F"][0][i] + 0.5))) for i, (a, _) in enumerate(PAIRS)]
            A, b = nf.closed_form(J, r, rows, fg.ISTD)
            nf.eigen_root(A, b)
    referee_ms = host_ms(referee, 3)
    new_ws = [fg.with_prior(w, f["J"], f["r0"], f["x0"]) if f["applied"] else w for w, f in zip(ws, fixed)]
    bs.close()

    def rebuild():
        b2 = solver.BatchSolver(new_ws)
        b2.sync()
        b2.close()
    rebuild_ms = host_ms(rebuild, max(3, REPS // 10))
    out["w%d" % W] = dict(fix_ms=round(fix_ms, 4), fix_install_ms=round(fix_install_ms, 4), fetch_ms=round(fetch_ms, 3),
                          get_fix_ms=round(get_fix_ms, 3), referee_ms=round(referee_ms, 3), rebuild_ms=round(rebuild_ms, 3),
                          old_path_ms=round(get_fix_ms + referee_ms + rebuild_ms, 3), applied=int(sum(f["applied"] for f in fixed)))
print(json.dumps(out))
