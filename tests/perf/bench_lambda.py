"""Time the device ambiguity search (swf_batch_ambiguity_search: D Qy D^T gather, LAMBDA with m = 2, ratio test) against what the
host hand-off needs just to deliver Qy (one swf_batch_get_tail_covariance per window), for 512 cfg3-size windows.
   python tests/perf/bench_lambda.py [windows] [reps]
n_b = S - 1 pairs per window (every ambiguity against the first).  Per n_b:
  call_ms        HIP events on the batch stream around the whole call (host-side pair validation, the pair upload, k_lambda);
                 the kernel alone: run under `rocprofv3 --kernel-trace --stats`
  fetch_ms       swf_batch_get_ambiguity_fix for every window after a search (one bulk copy, then host reads)
  qy_delivery_ms one swf_batch_get_tail_covariance per window: the floor of a host-side search before it has searched
  info_counts    windows per SWF_LAMBDA_* code (OK, NOT_PD, LOOP_LIMIT, NO_INPUT), fixed = windows that pass the ratio test
With a library built with -DSWF_PROFILE_LAMBDA (SWF_LIB=...), also the in-kernel split: mean / max microseconds per phase over the
windows (operands, LtDL, reduction, search, outputs, ratio test), search iterations and permutations.
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
from rtk_visual_inertial_navigation_amd import solver, synth
from rtk_visual_inertial_navigation_amd.flat import default_options

W = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
DISTINCT = 8
pi = C.POINTER(C.c_int32)
_pd = C.POINTER(C.c_double)
lib = solver.lib()


def pair_arrays(S, nw):
    P = [(i, 0) for i in range(1, S)]
    first = (np.arange(nw + 1) * len(P)).astype(np.int32)
    return first, np.ascontiguousarray(np.array(P * nw, np.int32).reshape(-1, 2))


def device_ms(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


out = dict(windows=W, reps=REPS)
for S in (9, 21, 41):
    base = [synth.make_window(3, S=S, seed=900 + i, head="ambiguities") for i in range(DISTINCT)]
    ws = [base[i % DISTINCT].copy() for i in range(W)]
    bs = solver.BatchSolver(ws)                     # the default stream: torch's events bracket its work
    bs.solve(default_options(), download=False)
    bs.tail_covariance()
    bs.sync()
    first, pairs = pair_arrays(S, W)
    h = bs._h

    def search(h=h, first=first, pairs=pairs):
        r = lib.swf_batch_ambiguity_search(h, first.ctypes.data_as(pi), pairs.ctypes.data_as(pi), C.c_double(2.0))
        assert r == 0, lib.swf_last_error()
    ms = device_ms(search, REPS)
    prof = None
    if hasattr(lib, "swf_debug_lambda_stamps"):
        search()
        st = np.zeros((min(W, 4096), 16), np.uint64)
        assert lib.swf_debug_lambda_stamps(st.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(W)) == 0
        rt = st[:, 8:15].astype(np.float64) / 100.0          # s_memrealtime: 100 MHz
        ph = np.diff(rt, axis=1)
        names = ["operands", "ltdl", "reduction", "search", "outputs", "ratio"]
        prof = dict(phase_us_mean={k: round(float(v), 3) for k, v in zip(names, ph.mean(0))},
                    phase_us_max={k: round(float(v), 3) for k, v in zip(names, ph.max(0))},
                    kernel_span_us=round(float(rt[:, 6].max() - rt[:, 0].min()), 2),
                    search_iterations_mean=round(float(st[:, 7].astype(float).mean()), 1), search_iterations_max=int(st[:, 7].max()),
                    permutations_mean=round(float(st[:, 15].astype(float).mean()), 1), permutations_max=int(st[:, 15].max()),
                    us_per_search_iteration=round(float((ph[:, 3] / np.maximum(st[:, 7].astype(float), 1)).mean()), 4))
    res = bs.ambiguity_search([[(i, 0) for i in range(1, S)]] * W)
    info = np.bincount([r["info"] for r in res], minlength=4).tolist()
    fixed = int(sum(r["fixed"] for r in res))
    # the results of every window: the first getter copies all records at once
    search()
    bs.sync()
    Fo, so, ro, fo = np.zeros(2 * (S - 1)), np.zeros(2), np.zeros(2), C.c_int32()
    t0 = time.perf_counter()
    for w in range(W):
        assert lib.swf_batch_get_ambiguity_fix(h, C.c_int32(w), Fo.ctypes.data_as(_pd), so.ctypes.data_as(_pd), ro.ctypes.data_as(_pd),
                                               C.byref(fo), None, None, None, None) == 0
    fetch_ms = (time.perf_counter() - t0) * 1e3
    # the host hand-off's floor: deliver Qy of every window (each call synchronises and copies n^2 doubles)
    Q = np.zeros((S, S))
    n = C.c_int32()
    t0 = time.perf_counter()
    for w in range(W):
        assert lib.swf_batch_get_tail_covariance(h, C.c_int32(w), None, Q.ctypes.data_as(_pd), C.byref(n)) == 0
    qy_ms = (time.perf_counter() - t0) * 1e3
    bs.close()
    one = solver.BatchSolver([base[0].copy()])
    one.solve(default_options(), download=False)
    one.tail_covariance()
    one.sync()
    f1, p1 = pair_arrays(S, 1)
    h1 = one._h

    def search1(h1=h1, f1=f1, p1=p1):
        assert lib.swf_batch_ambiguity_search(h1, f1.ctypes.data_as(pi), p1.ctypes.data_as(pi), C.c_double(2.0)) == 0
    one_ms = device_ms(search1, REPS)
    one.close()
    out["n_b%d" % (S - 1)] = dict(call_ms=round(ms, 4), fetch_ms=round(fetch_ms, 3), one_window_call_ms=round(one_ms, 4),
                                  qy_delivery_ms=round(qy_ms, 3), info_counts=info, fixed=fixed)
    if prof:
        out["n_b%d" % (S - 1)]["profile"] = prof
print(json.dumps(out))
