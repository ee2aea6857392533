"""Time the IMU frame front (swf_imu_frame_batch) for 1, 64 and 4 864 frames of 40 raw samples, warm, median of 50.
   python tests/perf/bench_imu_frame.py [reps]
Per frame count:
  device_ms        HIP events around the call with on_device = 1 (every array resident: the kernel and its launch)
  host_ms          the call on host memory (allocation, copies in, kernel, copies out, synchronisation), wall clock
  host_loop_ms     the same work as a compiled host loop (tests/perf/imu_frame_host.cpp, g++ -O3): cut, prediction, pre-integration with
                   dense 15x15 Jacobian and covariance updates, without the final square-root information; wall clock
  preint_ms        swf_preintegrate_batch alone, on_device = 1, on the cut samples the fused call wrote (HIP events)
  preint_parent_ms the same from the library named by SWF_PARENT_LIB (a build of the parent commit), when that is set
The fused call's pre is compared bit for bit with swf_preintegrate_batch on its cut rows, its pred with the host loop (1e-9), and the
host loop's covariance with the device's square-root information, before anything is timed.  Prints one JSON line."""
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
import imu_frame_gen as ig
from rtk_visual_inertial_navigation_amd import solver, synth

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SAMPLES, DISTINCT = 40, 64
NOISE = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
lib = solver.lib()
parent = None
if os.environ.get("SWF_PARENT_LIB"):
    parent = C.CDLL(os.environ["SWF_PARENT_LIB"])
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "imu_frame_host.so")
subprocess.check_call(["g++", "-O3", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "imu_frame_host.cpp")])
hostlib = C.CDLL(so)
v3 = lambda v: (C.c_double * 3)(*v)
nz = (C.c_double * 4)(*NOISE)
base = [ig.gen_frame(7000 + i, SAMPLES, "beyond", flag=i & 1) for i in range(DISTINCT)]
out = dict(samples_per_frame=SAMPLES, reps=REPS)
for E in (1, 64, 4864):
    frames = [base[i % DISTINCT] for i in range(E)]
    raw, t01, seed, state, gp, flags = ig.pack(frames)
    first = (np.arange(E + 1) * SAMPLES).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate(raw))
    cfirst = (np.arange(E + 1) * (SAMPLES + 1)).astype(np.int32)
    bias = np.ascontiguousarray(state[:, 15:21])
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in (flat, first, t01, seed, state, gp, flags, cfirst, bias)]
    z = lambda n, t=torch.float64: torch.zeros(n, dtype=t, device="cuda")
    o = dict(cut=z((E * (SAMPLES + 1)) * 7), pre=z(E * 293), pred=z(E * 15), info=z(E, torch.int32), pre2=z(E * 293))
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        rc = lib.swf_imu_frame_batch(p(dev[0], pd), p(dev[1], pi), C.c_int32(E), p(dev[2], pd), p(dev[3], pd), p(dev[4], pd), p(dev[5], pd),
                                     p(dev[6], pi), v3(ig.PBG), v3(ig.G_W), nz, p(o["cut"], pd), p(o["pre"], pd), p(o["pred"], pd), p(o["info"], pi),
                                     C.c_int32(1), stream)
        assert rc == 0, lib.swf_last_error()

    def preint(l=lib):
        rc = l.swf_preintegrate_batch(p(o["cut"], pd), p(dev[7], pi), C.c_int32(E), p(dev[8], pd), nz, p(o["pre2"], pd), C.c_int32(1), stream)
        assert rc == 0

    def host_call():
        return solver.imu_frame_batch(raw, t01, seed, state, gp, flags, ig.PBG, ig.G_W, NOISE)

    h_pred, h_dc = np.zeros((E, 15)), np.zeros((E, 236))

    def host_loop():
        hostlib.imu_frame_host(C.c_int32(E), flat.ctypes.data_as(pd), first.ctypes.data_as(pi), t01.ctypes.data_as(pd), seed.ctypes.data_as(pd),
                               state.ctypes.data_as(pd), gp.ctypes.data_as(pd), flags.ctypes.data_as(pi), v3(ig.PBG), v3(ig.G_W), nz,
                               h_pred.ctypes.data_as(pd), h_dc.ctypes.data_as(pd))

    fused(); preint(); torch.cuda.synchronize()
    host = host_call(); host_loop()
    d_pre, d_pred = o["pre"].cpu().numpy().reshape(E, 293), o["pred"].cpu().numpy().reshape(E, 15)
    assert (o["info"].cpu().numpy() == 0).all() and (host["info"] == 0).all()
    assert np.array_equal(d_pre.view(np.uint64), o["pre2"].cpu().numpy().reshape(E, 293).view(np.uint64))
    assert np.array_equal(d_pre.view(np.uint64), host["pre"].view(np.uint64)) and np.array_equal(d_pred.view(np.uint64), host["pred"].view(np.uint64))
    assert np.abs(h_pred - d_pred).max() <= 1e-9 * np.abs(d_pred).max()
    assert np.abs(h_dc[:, :11] - np.concatenate([d_pre[:, :10], d_pre[:, 61:62]], axis=1)).max() <= 1e-11
    for k in range(min(E, 4)):
        U = d_pre[k, 68:].reshape(15, 15)
        assert np.abs(U @ h_dc[k, 11:].reshape(15, 15) @ U.T - np.eye(15)).max() <= 1e-6
    if parent is not None:
        preint(parent); torch.cuda.synchronize()
        assert np.array_equal(d_pre.view(np.uint64), o["pre2"].cpu().numpy().reshape(E, 293).view(np.uint64))

    def events(fn):
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4)

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    r = dict(samples=int(flat.shape[0]), device_ms=events(fused), preint_ms=events(preint), host_ms=wall(host_call, REPS),
             host_loop_ms=wall(host_loop, REPS if E < 1000 else max(5, REPS // 10)))
    if parent is not None:
        r["preint_parent_ms"] = events(lambda: preint(parent))
    out["frames%d" % E] = r
print(json.dumps(out))
