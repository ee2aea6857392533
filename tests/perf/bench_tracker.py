"""Time the resident feature tracker (swf_tracker_track) per frame in steady state (from frame 3 on) for 1, 8 and 64
streams of 480 x 752 with MAX_CNT 150 and otherwise the reference's options, on a textured sequence that moves by (3.3, -2.6) px per
frame; median over the timed frames.
   python tests/perf/bench_tracker.py [timed frames]
Per stream count, all in the same run:
  fused_host_ms       wall clock of swf_tracker_track + swf_tracker_sync with the images in host memory (the upload included)
  fused_resident_ms   the same with the images in device memory already (img_on_device = 1; a device-to-device copy remains)
  upload_ms           fused_host_ms - fused_resident_ms
  chain_host_ms       (i) what a caller does without the tracker: the three operators through host memory, one call each for all
                      streams, and trackImage's bookkeeping in numpy between them (reduceVector, n++, ids, the final lift and velocity)
  operators_device_ms (ii) the three operators alone, called on device-resident arrays of a steady-state frame, HIP events, summed
  bookkeeping_ms      fused_resident_ms - operators_device_ms: the three bookkeeping kernels, the image copy and the launches
(iii) a compiled host loop of the whole chain was not built: the three tests/perf/*_host.cpp loops have no common driver.
The ids and pixels of the last frame of the chain and of the tracker are compared before anything is reported.  Prints one JSON line."""
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
import klt_gen as kg
import np_trackreject as nt
import tracker_cases as tcs
from rtk_visual_inertial_navigation_amd import solver

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 12
ROWS, COLS, DISTINCT, SKIP = 480, 752, 4, 3
FRAMES = SKIP + TIMED
OPT = dict(max_cnt=150)
KLT = dict(win=21, max_level=3, back_level=1, max_count=30, eps=0.01, min_eig=1e-4, back_dist=0.5, flags=5)
TRK = dict(col=COLS, row=ROWS, focal=1000.0, iterations=1000, threshold=1.0, confidence=0.99, flags=1)
GFTT = dict(max_cnt=150, min_dist=30, quality=0.01, cand_cap=1 << 15, flags=1)
CAM = tcs.camera()
pi, pd, pb = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lib = solver.lib()
SEQ = [[kg.tex(ROWS, COLS, -k * tcs.SHIFT[0], -k * tcs.SHIFT[1], 9100 + i) for k in range(FRAMES)] for i in range(DISTINCT)]
times_of = lambda k, E: [1.0 + 0.05 * k] * E
f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def frames_of(E, k):
    return np.stack([SEQ[s % DISTINCT][k] for s in range(E)])


class Chain:
    """(i): the three host-memory operators, batched over the streams, with trackImage's bookkeeping in numpy"""

    def __init__(self, E):
        self.E, self.prev_img, self.prev_time = E, None, None
        self.px = [np.zeros((0, 2))] * E
        self.ids = [np.zeros(0, np.int32)] * E
        self.tc = [np.zeros(0, np.int32)] * E
        self.un = [None] * E
        self.n_id = [0] * E
        self.captured = None

    def track(self, t, imgs, seed):
        E = self.E
        cur, prev, ids, tc = self.px, self.px, self.ids, self.tc
        if self.prev_img is not None:
            r = solver.klt_track_batch(self.prev_img, imgs, self.px, **KLT)
            klt_in = (self.prev_img, imgs, [p.copy() for p in self.px])
            keep = [r["keep_idx"][r["first"][s]:r["first"][s + 1]][:r["n_keep"][s]] for s in range(E)]
            cur = [r["cur_px"][r["first"][s]:r["first"][s + 1]][keep[s]] for s in range(E)]
            prev, ids, tc = [self.px[s][keep[s]] for s in range(E)], [ids[s][keep[s]] for s in range(E)], [tc[s][keep[s]] + 1 for s in range(E)]
            dt = t - self.prev_time
            r = solver.track_reject_batch(cur, prev, CAM, [dt] * E, seed=seed, **TRK)
            trk_in = (cur, prev, dt)
            for s in range(E):
                if r["info"][s] == solver.TRK_OK:
                    k = r["keep_idx"][r["first"][s]:r["first"][s + 1]]
                    k = k[k >= 0]
                    cur[s], ids[s], tc[s] = cur[s][k], ids[s][k], tc[s][k]
            self.captured = (klt_in, trk_in, (imgs, [c.copy() for c in cur], [c.copy() for c in tc]))
        r = solver.gftt_detect_batch(imgs, cur, tc, **GFTT)
        obs = []
        for s in range(E):
            lo, hi = r["pack_first"][s], r["pack_first"][s + 1]
            src, px = r["pack_src"][lo:hi], r["pack_px"][lo:hi]
            old = src >= 0
            n_new = int((~old).sum())
            new_ids = np.concatenate([ids[s][src[old]], np.arange(self.n_id[s], self.n_id[s] + n_new, dtype=np.int32)]).astype(np.int32)
            new_tc = np.concatenate([tc[s][src[old]], np.ones(n_new, np.int32)]).astype(np.int32)
            self.n_id[s] += n_new
            un = f32(nt.lift(CAM, px)[0])
            vel = np.zeros_like(un)
            if self.un[s] is not None and len(self.un[s][0]) and int(old.sum()):      # ptsVelocity: the ids of the previous frame's final list
                p_ids, p_un = self.un[s]
                order = np.argsort(p_ids)
                at = np.minimum(np.searchsorted(p_ids[order], new_ids[:int(old.sum())]), len(p_ids) - 1)
                hit = p_ids[order][at] == new_ids[:int(old.sum())]
                rows = np.flatnonzero(hit)
                vel[rows] = nt.velocity_of(un[rows], p_un[order][at[hit]], t - self.prev_time, 1)
            self.un[s] = (new_ids, un)
            self.px[s], self.ids[s], self.tc[s] = px, new_ids, new_tc
            obs.append(np.column_stack([un, np.ones(len(px)), px, vel]))
        self.prev_img, self.prev_time = imgs, t
        return obs


def events(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def operators_device(E, captured):
    """(ii): each operator on device-resident arrays of a steady-state frame"""
    (pimg, cimg, kpx), (tcur, tprev, dt), (gimg, gpx, gtc) = captured
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    z = lambda n, t=torch.float64: torch.zeros(max(n, 1), dtype=t, device="cuda")
    p = lambda t, ty: C.cast(t.data_ptr(), ty)
    I, stream = torch.int32, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    first_of = lambda lst: np.concatenate([[0], np.cumsum([len(a) for a in lst])]).astype(np.int32)
    flat = lambda lst, w: np.concatenate(list(lst) + [np.zeros((1, w)) if w else np.zeros(1, np.int32)])
    out = {}
    kf, n = first_of(kpx), int(first_of(kpx)[-1])
    d = [dev(pimg), dev(cimg), dev(kf), dev(flat(kpx, 2))]
    o = [z(n * 2), z(n, torch.uint8), z(n, I), z(E, I), z(E, I), z(E * solver.klt_pyramid_bytes(ROWS, COLS, 3), torch.uint8)]
    out["klt"] = events(lambda: lib.swf_klt_track_batch(
        C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), p(d[0], pb), p(d[1], pb), p(d[2], pi), p(d[3], pd), None, C.c_int32(KLT["win"]),
        C.c_int32(KLT["max_level"]), C.c_int32(KLT["back_level"]), C.c_int32(KLT["max_count"]), C.c_double(KLT["eps"]), C.c_double(KLT["min_eig"]),
        C.c_double(KLT["back_dist"]), C.c_int32(KLT["flags"]), p(o[0], pd), None, p(o[1], pb), None, p(o[2], pi), p(o[3], pi), p(o[4], pi), None, None,
        p(o[5], pb), C.c_int32(1), stream))
    tf, n = first_of(tcur), int(first_of(tcur)[-1])
    d = [dev(tf), dev(flat(tcur, 2)), dev(flat(tprev, 2)), dev(np.full(E, dt))]
    o = [z(n, I), z(E, I), z(E, I), z(n * 2), z(n * 2), z(n * 2)]
    cm = (C.c_double * 12)(*[float(v) for v in CAM])
    out["track_reject"] = events(lambda: lib.swf_track_reject_batch(
        C.c_int32(E), p(d[0], pi), p(d[1], pd), p(d[2], pd), cm, C.c_int32(COLS), C.c_int32(ROWS), C.c_double(TRK["focal"]), p(d[3], pd),
        C.c_int32(TRK["iterations"]), C.c_double(TRK["threshold"]), C.c_double(TRK["confidence"]), C.c_uint64(7), C.c_int32(1), None, p(o[0], pi), p(o[1], pi),
        None, None, p(o[2], pi), None, p(o[3], pd), p(o[4], pd), p(o[5], pd), None, None, None, C.c_int32(1), stream))
    gf, n = first_of(gpx), int(first_of(gpx)[-1])
    mc = GFTT["max_cnt"]
    d = [dev(gimg), dev(gf), dev(flat(gpx, 2)), dev(flat(gtc, 0).astype(np.int32))]
    o = [z(E, I), z(E, I), z(E, I), z(E + 1, I), z((n + E * mc) * 2), z(n + E * mc, I), z(E, I), z(E * solver.gftt_workspace_bytes(ROWS, COLS, GFTT["cand_cap"]), torch.uint8)]
    out["gftt"] = events(lambda: lib.swf_gftt_detect_batch(
        C.c_int32(E), C.c_int32(ROWS), C.c_int32(COLS), p(d[0], pb), None, p(d[1], pi), p(d[2], pd), p(d[3], pi), C.c_int32(mc), C.c_int32(GFTT["min_dist"]),
        C.c_double(GFTT["quality"]), None, C.c_int32(GFTT["cand_cap"]), C.c_int32(1), None, None, p(o[0], pi), None, p(o[1], pi), p(o[2], pi), None,
        p(o[3], pi), p(o[4], pd), p(o[5], pi), p(o[6], pi), p(o[7], pb), C.c_int32(1), stream))
    return out


def fused(E, on_device):
    T = solver.Tracker(E, ROWS, COLS, CAM, **OPT)
    ts, last = [], None
    try:
        for k in range(FRAMES):
            imgs = frames_of(E, k)
            d = torch.from_numpy(imgs.reshape(-1)).cuda() if on_device else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if on_device:
                T.track_device(times_of(k, E), d.data_ptr(), None, 100 + k)
            else:
                T.track(times_of(k, E), imgs, None, 100 + k)
            T.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        last = T.frame()
    finally:
        T.close()
    return float(np.median(ts[SKIP:])), last


out = dict(rows=ROWS, cols=COLS, max_cnt=OPT["max_cnt"], timed_frames=TIMED, first_timed_frame=SKIP)
for E in (1, 8, 64):
    fused(E, False)                                         # warm: the first calls of every kernel
    host_ms, last = fused(E, False)
    res_ms, last_dev = fused(E, True)
    ch, ts = Chain(E), []
    for k in range(FRAMES):
        imgs = frames_of(E, k)
        t0 = time.perf_counter()
        obs = ch.track(times_of(k, E)[0], imgs, 100 + k)
        ts.append((time.perf_counter() - t0) * 1e3)
    for s in range(E):                                      # the chain and the tracker agree on the last frame
        assert np.array_equal(ch.ids[s], last["ids"][s]) and np.array_equal(ch.ids[s], last_dev["ids"][s]), s
        assert np.array_equal(obs[s][:, 3:5], last["obs"][s][:, 3:5]), s
    ops = operators_device(E, ch.captured)
    ops_sum = sum(ops.values())
    out["streams%d" % E] = dict(points=int(sum(len(i) for i in last["ids"])), fused_host_ms=round(host_ms, 4), fused_resident_ms=round(res_ms, 4),
                                upload_ms=round(host_ms - res_ms, 4), chain_host_ms=round(float(np.median(ts[SKIP:])), 4),
                                operators_device_ms=round(ops_sum, 4), operators={k: round(v, 4) for k, v in ops.items()},
                                bookkeeping_ms=round(res_ms - ops_sum, 4), below_chain=bool(host_ms < float(np.median(ts[SKIP:]))))
print(json.dumps(out))
