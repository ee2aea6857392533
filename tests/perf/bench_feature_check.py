"""Time the post-solve feature check on the device (swf_batch_check_features + the result fetch of every window) beside what the
library offered for the same answer before it: swf_batch_download_state + the vectorised numpy referee (tests/np_features.py, its
observation table prebuilt), for 1, 64 and 512 cfg3 windows.
   python tests/perf/bench_feature_check.py [reps]
Per batch size (warm, median of `reps` >= 50 calls; the numpy leg: 5):
  check_ms             HIP events on the batch stream around swf_batch_check_features (k_feature_err + k_feature_compact)
  check_fetch_ms       host clock around the check and swf_batch_get_feature_check for every window (ends in a synchronise)
  download_state_ms    host clock around swf_batch_download_state
  download_numpy_ms    download_state + the numpy referee over every window
  n_obs, n_feat, rejected   observations / features / rejected features of the batch
The kernels alone: `rocprofv3 --kernel-trace --stats -- python tests/perf/bench_feature_check.py profile [windows]` (one solve and 20
checks of one batch, nothing else).  Prints one JSON line."""
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
import np_features as nf
from rtk_visual_inertial_navigation_amd import solver, synth
from rtk_visual_inertial_navigation_amd.flat import default_options

PROFILE = len(sys.argv) > 1 and sys.argv[1] == "profile"
REPS = max(50, int(sys.argv[1])) if len(sys.argv) > 1 and not PROFILE else 50
DISTINCT = 8
lib = solver.lib()
pi = C.POINTER(C.c_int32)
_pd = C.POINTER(C.c_double)


def median_host_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def median_device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t))


base = [synth.make_window(3, seed=900 + i) for i in range(DISTINCT)]
for i, w in enumerate(base):
    nf.inject(w, np.random.default_rng(1000 + i), 24)
if PROFILE:
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    bs = solver.BatchSolver([base[i % DISTINCT].copy() for i in range(W)])
    bs.solve(default_options(), download=False)
    for _ in range(20):
        assert lib.swf_batch_check_features(bs._h, C.c_double(2.0)) == 0, lib.swf_last_error()
    bs.sync()
    print(json.dumps(dict(profile_windows=W, checks=20, rejected=int(sum(r["rejected"].size for r in bs.check_features(2.0))))))
    bs.close()
    sys.exit(0)
out = dict(reps=REPS)
for W in (1, 64, 512):
    ws = [base[i % DISTINCT].copy() for i in range(W)]
    bs = solver.BatchSolver(ws)                     # the default stream: torch's events bracket its work
    bs.solve(default_options())
    h = bs._h
    nfeat = max(w.n_lm for w in ws)
    m, d = np.zeros(nfeat), np.zeros(nfeat)
    no, rj, fl = np.zeros(nfeat, np.int32), np.zeros(nfeat, np.int32), np.zeros(nfeat, np.uint8)
    nr, nfo = C.c_int32(), C.c_int32()

    def check():
        assert lib.swf_batch_check_features(h, C.c_double(2.0)) == 0, lib.swf_last_error()

    def check_fetch():
        check()
        tot = 0
        for w in range(W):
            assert lib.swf_batch_get_feature_check(h, C.c_int32(w), m.ctypes.data_as(_pd), d.ctypes.data_as(_pd), no.ctypes.data_as(pi),
                                                   fl.ctypes.data_as(C.POINTER(C.c_uint8)), rj.ctypes.data_as(pi), C.byref(nr), C.byref(nfo)) == 0
            tot += nr.value
        return tot

    tabs = [nf.table(w) for w in ws]

    def download():
        assert lib.swf_batch_download_state(h) == 0

    def download_numpy():
        download()
        return sum(nf.check(w, tab=t)["rejected"].size for w, t in zip(ws, tabs))

    rejected = check_fetch()
    assert rejected == download_numpy(), (rejected, download_numpy())
    out["windows_%d" % W] = dict(check_ms=round(median_device_ms(check, REPS), 4), check_fetch_ms=round(median_host_ms(check_fetch, REPS), 4),
                                 download_state_ms=round(median_host_ms(download, REPS), 4),
                                 download_numpy_ms=round(median_host_ms(download_numpy, 5), 2),
                                 n_obs=int(sum(w.a["proj_idx"].shape[0] for w in ws)), n_feat=int(sum(w.n_lm for w in ws)), rejected=int(rejected))
    bs.close()
print(json.dumps(out))
