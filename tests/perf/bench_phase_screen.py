"""Time the pre-fit carrier-phase screen (swf_phase_screen_batch) for 1, 64 and 4 864 epochs of 32 records, warm, median of 50.
   python tests/perf/bench_phase_screen.py [reps]
Per epoch count:
  device_ms     HIP events around the call with on_device = 1 (every array resident: the kernel and its launch)
  host_ms       the call on host memory (allocation, copies in, kernel, copies out, synchronisation), wall clock
  numpy_ms      the vectorised numpy referee (tests/np_phase.py) on the same arrays, wall clock
The results of the two memory modes are compared bit for bit and against the referee's flags before anything is timed.
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
import np_phase as nph
import phase_gen as pg
from rtk_visual_inertial_navigation_amd import solver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
RECORDS, DISTINCT = 32, 64
pi, pd, pu8 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
base = [pg.gen_epoch(5000 + i, RECORDS) for i in range(DISTINCT)]
out = dict(records_per_epoch=RECORDS, reps=REPS)
for E in (1, 64, 4864):
    packed = pg.pack([base[i % DISTINCT] for i in range(E)])
    first, pos, bas, mode, dat, rec = packed
    n = dat.shape[0]
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in packed]
    o = dict(r=torch.zeros(n, dtype=torch.float64, device="cuda"), flags=torch.zeros(n, dtype=torch.uint8, device="cuda"),
             med=torch.zeros(E * 12, dtype=torch.float64, device="cuda"), cnt=torch.zeros(E * 12, dtype=torch.int32, device="cuda"),
             reset=torch.zeros(n, dtype=torch.int32, device="cuda"), n_reset=torch.zeros(E, dtype=torch.int32, device="cuda"))
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def on_device():
        rc = lib.swf_phase_screen_batch(C.c_int32(E), p(dev[0], pi), p(dev[1], pd), p(dev[2], pd), p(dev[3], pi), C.c_double(nph.AZELMIN),
                                        p(dev[4], pd), p(dev[5], pi), p(o["r"], pd), p(o["flags"], pu8), p(o["med"], pd), p(o["cnt"], pi),
                                        p(o["reset"], pi), p(o["n_reset"], pi), C.c_int32(1), stream)
        assert rc == 0, lib.swf_last_error()

    on_device()
    torch.cuda.synchronize()
    host = solver.phase_screen_batch(*packed)
    ref = nph.screen(*packed)
    assert np.array_equal(o["flags"].cpu().numpy(), host["flags"]) and np.array_equal(host["flags"], ref["flags"])
    assert np.array_equal(o["r"].cpu().numpy().view(np.uint64), host["r"].view(np.uint64))
    assert np.array_equal(o["reset"].cpu().numpy(), ref["reset"]) and np.array_equal(host["n_reset"], ref["n_reset"])
    t_dev, t_host, t_np = [], [], []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); on_device(); e1.record()
        torch.cuda.synchronize()
        t_dev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter(); solver.phase_screen_batch(*packed); t_host.append((time.perf_counter() - t0) * 1e3)
    for _ in range(max(3, REPS // 10)):
        t0 = time.perf_counter(); nph.screen(*packed); t_np.append((time.perf_counter() - t0) * 1e3)
    out["epochs%d" % E] = dict(records=int(n), device_ms=round(float(np.median(t_dev)), 4), host_ms=round(float(np.median(t_host)), 4),
                               numpy_ms=round(float(np.median(t_np)), 4), resets=int(ref["n_reset"].sum()))
print(json.dumps(out))
