"""Time the single-epoch GNSS solve (swf_gnss_epoch_solve_batch) for 1, 64 and 4 864 epochs of 40 records under the seed preset (pose and
speed-bias constant, 2 iterations) and the first-fix preset (everything free, 20 allowed, 3 taken), warm, median of 50.
   python tests/perf/bench_gnss_epoch.py [reps]
Per preset and epoch count:
  device_ms             HIP events around the call with on_device = 1 (every array resident: the kernel and its launch)
  host_ms               the call on host memory (allocation, copies in, kernel, copies out, synchronisation), wall clock
  numpy_ms_per_epoch    the float64 numpy referee (tests/np_gnss_epoch.py, a host loop over the epochs), wall clock per epoch, measured on
                        at most 64 epochs
The results of the two memory modes are compared bit for bit and status / iterations against the referee before anything is timed.
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
import np_gnss_epoch as nge
import gnss_epoch_gen as gg
from rtk_visual_inertial_navigation_amd import solver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
RECORDS, DISTINCT = 40, 64
pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
lib = solver.lib()
out = dict(records_per_epoch=RECORDS, reps=REPS)
for preset, max_iter in (("seed", 2), ("first_fix", 20)):
    base = [gg.gen_epoch(7000 + i, RECORDS, preset) for i in range(DISTINCT)]
    for E in (1, 64, 4864):
        packed = gg.pack([base[i % DISTINCT] for i in range(E)])
        n = packed[7].shape[0]
        dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in packed]
        f64 = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")
        o = [f64(3 * E), f64(3 * E), f64(13 * E), f64(n), f64(n), f64(E), i32(E), i32(E), i32(13 * E), f64(36 * E)]
        p = lambda t: C.cast(t.data_ptr(), pd if t.dtype == torch.float64 else pi)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def on_device():
            rc = lib.swf_gnss_epoch_solve_batch(C.c_int32(E), *[p(t) for t in dev], C.c_int32(max_iter), C.c_double(1e-4), C.c_double(1e-8),
                                                *[p(t) for t in o], C.c_int32(1), stream)
            assert rc == 0, lib.swf_last_error()

        on_device()
        torch.cuda.synchronize()
        host = solver.gnss_epoch_solve_batch(*packed, max_iter=max_iter)
        k = min(E, DISTINCT)
        sub = gg.pack([base[i % DISTINCT] for i in range(k)])
        ref = nge.solve_batch(*sub, max_iter=max_iter)
        assert np.array_equal(host["status"][:k], ref["status"]) and np.array_equal(host["iters"][:k], ref["iters"])
        for t, key in zip(o, ("pos", "vel", "clock", "N", "r", "cost", "iters", "status", "clk_rows", "info")):
            a, b = t.cpu().numpy().reshape(-1), np.ascontiguousarray(host[key]).reshape(-1)
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), key
        t_dev, t_host, t_np = [], [], []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); on_device(); e1.record()
            torch.cuda.synchronize()
            t_dev.append(e0.elapsed_time(e1))
            t0 = time.perf_counter(); solver.gnss_epoch_solve_batch(*packed, max_iter=max_iter); t_host.append((time.perf_counter() - t0) * 1e3)
        for _ in range(3):
            t0 = time.perf_counter(); nge.solve_batch(*sub, max_iter=max_iter); t_np.append((time.perf_counter() - t0) * 1e3 / k)
        out["%s_epochs%d" % (preset, E)] = dict(records=int(n), iters=int(host["iters"].max()), device_ms=round(float(np.median(t_dev)), 4),
                                                host_ms=round(float(np.median(t_host)), 4), numpy_ms_per_epoch=round(float(np.median(t_np)), 4))
print(json.dumps(out))
