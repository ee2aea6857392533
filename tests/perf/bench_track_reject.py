"""Time the batched track outlier rejection (swf_track_reject_batch) for 1, 64 and 4 864 pairs of 150 points, up to 1000
hypotheses, 25 % outliers; every timed path is warmed with 5 calls of the same shape first (1 for the host paths at 4 864 pairs);
median of 50.
   python tests/perf/bench_track_reject.py [reps]
Per pair count:
  device_ms      HIP events around the call with on_device = 1 (every array resident: the kernel and its launch)
  host_ms        the call on host memory (allocation, copies in, kernel, copies out, synchronisation), wall clock
  host_loop_ms   the same algorithm as a compiled host loop (tests/perf/track_reject_host.cpp, g++ -O3), which stops drawing hypotheses
                 where the scan stops; wall clock
The device's codes and lifted points are compared with the host loop's, and its inlier counts where the host loop (which rounds
differently) takes the same decisions, before anything is timed.  Prints one JSON line."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import trackreject_gen as tg
from rtk_visual_inertial_navigation_amd import solver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
POINTS, DISTINCT, H, WARM = 150, 64, 1000, 5
pi, pd, pb = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "track_reject_host.so")
subprocess.check_call(["g++", "-O3", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "track_reject_host.cpp")])
hostlib = C.CDLL(so)
cam = (C.c_double * 12)(*tg.CAM)
base = [tg.gen_pair(8000 + i, POINTS, outliers=0.25, motion=tg.MOTIONS[i % 3]) for i in range(DISTINCT)]
out = dict(points_per_pair=POINTS, hypotheses=H, reps=REPS)
for E in (1, 64, 4864):
    pairs = [base[i % DISTINCT] for i in range(E)]
    cur, prev, _, dt = tg.pack(pairs)
    first = (np.arange(E + 1) * POINTS).astype(np.int32)
    fc, fp = np.ascontiguousarray(np.concatenate(cur)), np.ascontiguousarray(np.concatenate(prev))
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in (first, fc, fp, dt)]
    z = lambda n, t=torch.float64: torch.zeros(n, dtype=t, device="cuda")
    o = dict(status=z(E * POINTS, torch.uint8), keep=z(E * POINTS, torch.int32), ni=z(E, torch.int32), best=z(E, torch.int32), nit=z(E, torch.int32),
             info=z(E, torch.int32), F=z(E * 9), uc=z(E * POINTS * 2), up=z(E * POINTS * 2), vel=z(E * POINTS * 2))
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def device_call():
        rc = lib.swf_track_reject_batch(C.c_int32(E), p(dev[0], pi), p(dev[1], pd), p(dev[2], pd), cam, C.c_int32(tg.COL), C.c_int32(tg.ROW),
                                        C.c_double(tg.FOCAL), p(dev[3], pd), C.c_int32(H), C.c_double(tg.THRESHOLD), C.c_double(tg.CONFIDENCE),
                                        C.c_uint64(tg.SEED), C.c_int32(1), p(o["status"], pb), p(o["keep"], pi), p(o["ni"], pi), p(o["best"], pi),
                                        p(o["nit"], pi), p(o["info"], pi), p(o["F"], pd), p(o["uc"], pd), p(o["up"], pd), p(o["vel"], pd),
                                        None, None, None, C.c_int32(1), stream)
        assert rc == 0, lib.swf_last_error()

    def host_call():
        return solver.track_reject_batch(cur, prev, tg.CAM, dt, col=tg.COL, row=tg.ROW, focal=tg.FOCAL, iterations=H, threshold=tg.THRESHOLD,
                                         confidence=tg.CONFIDENCE, seed=tg.SEED, flags=1)

    h_st, h_ni, h_info = np.zeros(E * POINTS, np.uint8), np.zeros(E, np.int32), np.zeros(E, np.int32)
    h_uc, h_vel = np.zeros((E * POINTS, 2)), np.zeros((E * POINTS, 2))

    def host_loop():
        hostlib.track_reject_host(C.c_int32(E), first.ctypes.data_as(pi), fc.ctypes.data_as(pd), fp.ctypes.data_as(pd), cam, C.c_int32(tg.COL),
                                  C.c_int32(tg.ROW), C.c_double(tg.FOCAL), np.ascontiguousarray(dt).ctypes.data_as(pd), C.c_int32(H),
                                  C.c_double(tg.THRESHOLD), C.c_double(tg.CONFIDENCE), C.c_uint64(tg.SEED), C.c_int32(1), h_st.ctypes.data_as(pb),
                                  h_ni.ctypes.data_as(pi), h_info.ctypes.data_as(pi), h_uc.ctypes.data_as(pd), h_vel.ctypes.data_as(pd))

    device_call(); torch.cuda.synchronize()
    host = host_call(); host_loop()
    d_ni, d_st = o["ni"].cpu().numpy(), o["status"].cpu().numpy()
    assert (o["info"].cpu().numpy() == 0).all() and (host["info"] == 0).all() and (h_info == 0).all()
    assert np.array_equal(d_ni, host["n_inliers"]) and np.array_equal(d_st, host["status"])
    assert np.array_equal(o["uc"].cpu().numpy().view(np.uint64), host["un_cur"].reshape(-1).view(np.uint64))
    assert np.abs(h_uc - host["un_cur"]).max() <= 1e-6 and np.abs(h_vel - host["velocity"]).max() <= 1e-4
    same = float((h_ni == d_ni).mean())
    assert same >= 0.5 and abs(int(h_ni.sum()) - int(d_ni.sum())) <= 0.1 * d_ni.sum()

    def events(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4)

    def wall(fn, reps):
        for _ in range(WARM if E < 1000 else 1):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    out["pairs%d" % E] = dict(points=int(fc.shape[0]), device_ms=events(device_call), host_ms=wall(host_call, REPS if E < 1000 else max(5, REPS // 5)),
                              host_loop_ms=wall(host_loop, REPS if E < 1000 else max(5, REPS // 10)), host_loop_same_counts=round(same, 3),
                              mean_n_iters=round(float(o["nit"].cpu().numpy().mean()), 1))
print(json.dumps(out))
