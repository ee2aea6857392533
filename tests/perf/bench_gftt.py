"""Time the batched corner detection (swf_gftt_detect_batch) for 1, 8 and 64 frames of 480 x 752 with 150 tracked points
each at the reference's arguments (MAX_CNT 350, MIN_DIST 30, quality 0.01), on a natural-looking texture, on uniform noise, and on
uniform noise without tracked points (noise_start: about 24 000 free candidates per frame, the worst case of the selection); every
timed path is warmed with 5 calls of the same shape first; median of 30.
   python tests/perf/bench_gftt.py [reps]
   rocprofv3 --kernel-trace --stats -d DIR -- python tests/perf/bench_gftt.py --kernels texture|noise|noise_start FRAMES     (20 device calls, nothing timed)
Per image kind and frame count:
  device_ms      HIP events around the call with on_device = 1 (every array resident: the six kernels and their launches)
  host_ms        the call on host memory (allocation, image copies in, kernels, copies out, synchronisation), wall clock
  host_loop_ms   the same specification as a compiled host loop (tests/perf/gftt_host.cpp, g++ -O3, one thread), wall clock
The device's order, why, new_px, n_new, n_cand and max_eig are compared with the host loop's bit for bit before anything is timed.
Prints one JSON line."""
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

KERNELS = sys.argv[1] == "--kernels" if len(sys.argv) > 1 else False
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and not KERNELS else 30
ROWS, COLS, DISTINCT, WARM = 480, 752, 8, 5
ARGS = dict(max_cnt=350, min_dist=30, quality=0.01, cand_cap=1 << 15, flags=1)
pi, pd, pb = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "gftt_host.so")
subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "gftt_host.cpp")])
hostlib = C.CDLL(so)
wb = solver.gftt_workspace_bytes(ROWS, COLS, ARGS["cand_cap"])


def images(kind, i):
    if kind.startswith("noise"):
        return np.random.default_rng(7000 + i).integers(0, 256, (ROWS, COLS), dtype=np.uint8)
    return kg.tex(ROWS, COLS, 0.0, 0.0, 9000 + i)


out = dict(rows=ROWS, cols=COLS, points_per_frame=150, reps=REPS)
for kind in (sys.argv[2],) if KERNELS else ("texture", "noise", "noise_start"):
    POINTS = 0 if kind == "noise_start" else 150         # noise_start: no tracked points yet, every candidate free: the worst case of stage D
    base = [(images(kind, i), kg.points(ROWS, COLS, POINTS, 0, 9000 + i), np.random.default_rng(i).integers(1, 30, POINTS).astype(np.int32)) for i in range(DISTINCT)]
    for E in (int(sys.argv[3]),) if KERNELS else (1, 8, 64):
        img = np.stack([base[i % DISTINCT][0] for i in range(E)])
        pts = [base[i % DISTINCT][1] for i in range(E)]
        tcs = [base[i % DISTINCT][2] for i in range(E)]
        fp = np.ascontiguousarray(np.concatenate(pts + [np.zeros((1, 2))]))              # one spare element: never an empty array
        ft = np.ascontiguousarray(np.concatenate(tcs + [np.zeros(1, np.int32)]))
        first = (np.arange(E + 1) * POINTS).astype(np.int32)
        mc, tot = ARGS["max_cnt"], E * POINTS
        dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in (img, first, fp, ft)]
        z = lambda n, t=torch.float64: torch.zeros(n, dtype=t, device="cuda")
        I = torch.int32
        o = dict(order=z(tot + 1, I), why=z(tot + 1, I), n_old=z(E, I), new_px=z(E * mc * 2), n_new=z(E, I), n_cand=z(E, I), max_eig=z(E), pack_first=z(E + 1, I),
                 pack_px=z((tot + E * mc) * 2), pack_src=z(tot + E * mc, I), info=z(E, I), work=z(E * wb, torch.uint8))
        p = lambda t, ty: C.cast(t.data_ptr(), ty)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def device_call():
            rc = lib.swf_gftt_detect_batch(C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), p(dev[0], pb), None, p(dev[1], pi), p(dev[2], pd), p(dev[3], pi),
                                           C.c_int32(mc), C.c_int32(ARGS["min_dist"]), C.c_double(ARGS["quality"]), None, C.c_int32(ARGS["cand_cap"]),
                                           C.c_int32(ARGS["flags"]), p(o["order"], pi), p(o["why"], pi), p(o["n_old"], pi), p(o["new_px"], pd), p(o["n_new"], pi),
                                           p(o["n_cand"], pi), p(o["max_eig"], pd), p(o["pack_first"], pi), p(o["pack_px"], pd), p(o["pack_src"], pi),
                                           p(o["info"], pi), p(o["work"], pb), C.c_int32(1), stream)
            assert rc == 0, lib.swf_last_error()

        if KERNELS:
            for _ in range(20):
                device_call()
            torch.cuda.synchronize()
            continue

        def host_call():
            return solver.gftt_detect_batch(img, pts, tcs, **ARGS)

        h = dict(order=np.zeros(tot + 1, np.int32), why=np.zeros(tot + 1, np.int32), n_old=np.zeros(E, np.int32), new_px=np.zeros((E, mc, 2)), n_new=np.zeros(E, np.int32),
                 n_cand=np.zeros(E, np.int32), max_eig=np.zeros(E), pack_first=np.zeros(E + 1, np.int32), pack_px=np.zeros((tot + E * mc, 2)),
                 pack_src=np.zeros(tot + E * mc, np.int32), info=np.zeros(E, np.int32))
        kind_of = dict(order=pi, why=pi, n_old=pi, new_px=pd, n_new=pi, n_cand=pi, max_eig=pd, pack_first=pi, pack_px=pd, pack_src=pi, info=pi)

        def host_loop():
            hostlib.gftt_host(C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), img.ctypes.data_as(pb), None, first.ctypes.data_as(pi), fp.ctypes.data_as(pd),
                              ft.ctypes.data_as(pi), C.c_int32(mc), C.c_int32(ARGS["min_dist"]), C.c_double(ARGS["quality"]), None, C.c_int32(ARGS["cand_cap"]),
                              C.c_int32(ARGS["flags"]), *[h[k].ctypes.data_as(kind_of[k]) for k in kind_of], None)

        device_call(); torch.cuda.synchronize()
        host = host_call(); host_loop()
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)
        assert (o["info"].cpu().numpy() == 0).all() and (host["info"] == 0).all() and (h["info"] == 0).all()
        for key in ("order", "why", "n_old", "n_new", "n_cand", "pack_first"):
            cut = tot if key in ("order", "why") else None
            assert np.array_equal(o[key].cpu().numpy()[:cut], h[key][:cut]) and np.array_equal(host[key], h[key][:cut]), key
        assert np.array_equal(u64(o["max_eig"].cpu().numpy()), u64(h["max_eig"])) and np.array_equal(u64(host["max_eig"]), u64(h["max_eig"]))
        d_new = o["new_px"].cpu().numpy().reshape(E, mc, 2)
        for k in range(E):
            n = int(h["n_new"][k])
            assert np.array_equal(u64(d_new[k, :n]), u64(h["new_px"][k, :n])) and np.array_equal(u64(host["new_px"][k, :n]), u64(h["new_px"][k, :n])), k
        used = int(h["pack_first"][E])
        assert np.array_equal(u64(o["pack_px"].cpu().numpy()[:used * 2]), u64(h["pack_px"][:used])) and np.array_equal(o["pack_src"].cpu().numpy()[:used], h["pack_src"][:used])

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

        out["%s_frames%d" % (kind, E)] = dict(kept=int(h["n_old"].sum()), new=int(h["n_new"].sum()), candidates=int(h["n_cand"].sum()),
                                              device_ms=events(device_call), host_ms=wall(host_call, REPS if E < 64 else max(5, REPS // 3)),
                                              host_loop_ms=wall(host_loop, REPS if E < 64 else max(3, REPS // 10)))
if not KERNELS:
    print(json.dumps(out))
