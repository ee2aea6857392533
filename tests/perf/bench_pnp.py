"""Time the batched RANSAC PnP (swf_pnp_frame_batch) for 1, 64 and 4 864 frames of 150 points, 100 hypotheses, 30 %
outliers; every timed path is warmed with 5 calls of the same shape first (1 for the host paths at 4 864 frames); median of 50.
   python tests/perf/bench_pnp.py [reps]
Per frame count:
  device_ms      HIP events around the call with on_device = 1 (every array resident: the kernel and its launch)
  host_ms        the call on host memory (allocation, copies in, kernel, copies out, synchronisation), wall clock
  host_loop_ms   the same algorithm as a compiled host loop (tests/perf/pnp_host.cpp, g++ -O3), which stops drawing hypotheses where the
                 scan stops; wall clock
The device's codes and inlier counts are compared with the host loop's and its poses to 1e-9 before anything is timed.  Prints one
JSON line."""
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
import pnp_gen as pg
from rtk_visual_inertial_navigation_amd import solver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
POINTS, DISTINCT, H, WARM = 150, 64, 100, 5
pi, pd, pb = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "pnp_host.so")
subprocess.check_call(["g++", "-O3", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "pnp_host.cpp")])
hostlib = C.CDLL(so)
vec = lambda v, k: (C.c_double * k)(*np.asarray(v, np.float64).reshape(k))
base = [pg.gen_frame(8000 + i, POINTS, outliers=0.3) for i in range(DISTINCT)]
out = dict(points_per_frame=POINTS, hypotheses=H, reps=REPS)
for E in (1, 64, 4864):
    frames = [base[i % DISTINCT] for i in range(E)]
    pw, uv, pp, rp = pg.pack(frames)
    first = (np.arange(E + 1) * POINTS).astype(np.int32)
    fw, fu = np.ascontiguousarray(np.concatenate(pw)), np.ascontiguousarray(np.concatenate(uv))
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in (first, fw, fu, pp, rp)]
    z = lambda n, t=torch.float64: torch.zeros(n, dtype=t, device="cuda")
    o = dict(Ps=z(E * 3), Rs=z(E * 9), ni=z(E, torch.int32), inl=z(E * POINTS, torch.uint8), best=z(E, torch.int32), nit=z(E, torch.int32),
             info=z(E, torch.int32))
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def device_call():
        rc = lib.swf_pnp_frame_batch(C.c_int32(E), p(dev[0], pi), p(dev[1], pd), p(dev[2], pd), p(dev[3], pd), p(dev[4], pd), vec(pg.TIC, 3), vec(pg.RIC, 9),
                                     vec(pg.PBG, 3), C.c_int32(H), C.c_double(pg.THRESHOLD), C.c_double(pg.CONFIDENCE), C.c_uint64(pg.SEED), C.c_int32(1),
                                     p(o["Ps"], pd), p(o["Rs"], pd), p(o["ni"], pi), p(o["inl"], pb), p(o["best"], pi), p(o["nit"], pi), p(o["info"], pi),
                                     None, None, None, C.c_int32(1), stream)
        assert rc == 0, lib.swf_last_error()

    def host_call():
        return solver.pnp_frame_batch(pw, uv, pp, rp, pg.TIC, pg.RIC, pg.PBG, iterations=H, threshold=pg.THRESHOLD, confidence=pg.CONFIDENCE,
                                      seed=pg.SEED, flags=1)

    h_Ps, h_Rs, h_ni, h_info = np.zeros((E, 3)), np.zeros((E, 9)), np.zeros(E, np.int32), np.zeros(E, np.int32)

    def host_loop():
        hostlib.pnp_host(C.c_int32(E), first.ctypes.data_as(pi), fw.ctypes.data_as(pd), fu.ctypes.data_as(pd), pp.ctypes.data_as(pd), rp.ctypes.data_as(pd),
                         vec(pg.TIC, 3), vec(pg.RIC, 9), vec(pg.PBG, 3), C.c_int32(H), C.c_double(pg.THRESHOLD), C.c_double(pg.CONFIDENCE),
                         C.c_uint64(pg.SEED), C.c_int32(1), h_Ps.ctypes.data_as(pd), h_Rs.ctypes.data_as(pd), h_ni.ctypes.data_as(pi),
                         h_info.ctypes.data_as(pi))

    device_call(); torch.cuda.synchronize()
    host = host_call(); host_loop()
    d_Ps, d_Rs = o["Ps"].cpu().numpy().reshape(E, 3), o["Rs"].cpu().numpy().reshape(E, 9)
    assert (o["info"].cpu().numpy() == 0).all() and (host["info"] == 0).all() and (h_info == 0).all()
    assert np.array_equal(d_Ps.view(np.uint64), host["Ps"].view(np.uint64)) and np.array_equal(d_Rs.view(np.uint64), host["Rs"].view(np.uint64))
    assert np.array_equal(o["ni"].cpu().numpy(), h_ni)
    assert np.abs(h_Ps - d_Ps).max() <= 1e-9 * max(1.0, np.abs(d_Ps).max()) and np.abs(h_Rs - d_Rs).max() <= 1e-9

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

    out["frames%d" % E] = dict(points=int(fw.shape[0]), device_ms=events(device_call), host_ms=wall(host_call, REPS if E < 1000 else max(5, REPS // 5)),
                               host_loop_ms=wall(host_loop, REPS if E < 1000 else max(5, REPS // 10)))
print(json.dumps(out))
