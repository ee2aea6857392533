"""Time the batched pyramidal Lucas-Kanade tracking (swf_klt_track_batch) for 1, 8 and 64 pairs of 480 x 752 images with
150 points each at the reference's arguments (21 x 21, 3 levels forward, 1 level back, 30 iterations); every timed path is warmed with
5 calls of the same shape first; median of 30.
   python tests/perf/bench_klt.py [reps]
Per pair count:
  device_ms      HIP events around the call with on_device = 1 (every array resident: the kernels and their launches)
  host_ms        the call on host memory (allocation, image copies in, kernels, copies out, synchronisation), wall clock
  host_loop_ms   the same specification as a compiled host loop (tests/perf/klt_host.cpp, g++ -O3, one thread), wall clock
The device's cur_px, back_px, status and why are compared with the host loop's bit for bit before anything is timed.  Prints one JSON
line."""
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
import klt_gen as kg
from rtk_visual_inertial_navigation_amd import solver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
ROWS, COLS, POINTS, DISTINCT, WARM = 480, 752, 150, 8, 5
ARGS = dict(win=21, max_level=3, back_level=1, max_count=30, eps=0.01, min_eig=1e-4, back_dist=0.5, flags=5)
pi, pd, pb = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "klt_host.so")
subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "klt_host.cpp")])
hostlib = C.CDLL(so)
base = []
for i in range(DISTINCT):
    shift = (4.0 + 1.5 * i, -3.0 + 1.1 * i)
    prev, cur = kg.pair(ROWS, COLS, shift, 9000 + i)
    base.append((prev, cur, kg.points(ROWS, COLS, POINTS, 30, 9000 + i)))
nb = solver.klt_pyramid_bytes(ROWS, COLS, 3)
out = dict(rows=ROWS, cols=COLS, points_per_pair=POINTS, reps=REPS)
for E in (1, 8, 64):
    prev = np.stack([base[i % DISTINCT][0] for i in range(E)])
    cur = np.stack([base[i % DISTINCT][1] for i in range(E)])
    pts = [base[i % DISTINCT][2] for i in range(E)]
    fp = np.ascontiguousarray(np.concatenate(pts))
    first = (np.arange(E + 1) * POINTS).astype(np.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in (prev, cur, first, fp)]
    z = lambda n, t=torch.float64: torch.zeros(n, dtype=t, device="cuda")
    o = dict(cur=z(E * POINTS * 2), back=z(E * POINTS * 2), status=z(E * POINTS, torch.uint8), why=z(E * POINTS, torch.int32),
             keep=z(E * POINTS, torch.int32), nk=z(E, torch.int32), info=z(E, torch.int32), pyr=z(E * nb, torch.uint8))
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def device_call():
        rc = lib.swf_klt_track_batch(C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), p(dev[0], pb), p(dev[1], pb), p(dev[2], pi), p(dev[3], pd), None,
                                     C.c_int32(ARGS["win"]), C.c_int32(ARGS["max_level"]), C.c_int32(ARGS["back_level"]), C.c_int32(ARGS["max_count"]),
                                     C.c_double(ARGS["eps"]), C.c_double(ARGS["min_eig"]), C.c_double(ARGS["back_dist"]), C.c_int32(ARGS["flags"]),
                                     p(o["cur"], pd), p(o["back"], pd), p(o["status"], pb), p(o["why"], pi), p(o["keep"], pi), p(o["nk"], pi),
                                     p(o["info"], pi), None, None, p(o["pyr"], pb), C.c_int32(1), stream)
        assert rc == 0, lib.swf_last_error()

    def host_call():
        return solver.klt_track_batch(prev, cur, pts, **ARGS)

    h_cur, h_back = np.zeros((E * POINTS, 2)), np.zeros((E * POINTS, 2))
    h_st, h_why, h_nk, h_info = np.zeros(E * POINTS, np.uint8), np.zeros(E * POINTS, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)

    def host_loop():
        hostlib.klt_host(C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), prev.ctypes.data_as(pb), cur.ctypes.data_as(pb), first.ctypes.data_as(pi),
                         fp.ctypes.data_as(pd), None, C.c_int32(ARGS["win"]), C.c_int32(ARGS["max_level"]), C.c_int32(ARGS["back_level"]),
                         C.c_int32(ARGS["max_count"]), C.c_double(ARGS["eps"]), C.c_double(ARGS["min_eig"]), C.c_double(ARGS["back_dist"]),
                         C.c_int32(ARGS["flags"]), h_cur.ctypes.data_as(pd), h_back.ctypes.data_as(pd), h_st.ctypes.data_as(pb), h_why.ctypes.data_as(pi),
                         h_nk.ctypes.data_as(pi), h_info.ctypes.data_as(pi))

    device_call(); torch.cuda.synchronize()
    host = host_call(); host_loop()
    u64 = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint64)
    assert (o["info"].cpu().numpy() == 0).all() and (host["info"] == 0).all() and (h_info == 0).all()
    for got in (o["cur"].cpu().numpy(), host["cur_px"]):
        assert np.array_equal(u64(got), u64(h_cur))
    for got in (o["back"].cpu().numpy(), host["back_px"]):
        assert np.array_equal(u64(got), u64(h_back))
    assert np.array_equal(o["why"].cpu().numpy(), h_why) and np.array_equal(host["why"], h_why) and np.array_equal(o["nk"].cpu().numpy(), h_nk)

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
        for _ in range(WARM if E < 64 else 1):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    out["pairs%d" % E] = dict(points=int(fp.shape[0]), kept=int(h_nk.sum()), device_ms=events(device_call), host_ms=wall(host_call, REPS),
                              host_loop_ms=wall(host_loop, REPS if E < 64 else max(3, REPS // 10)))
print(json.dumps(out))
