"""Time one steady-state cycle of the resident feature table (swf_ftable_*): add_frame, triangulate, list,
check_parallax, slide (removeBack) on a full window, for 1, 8 and 64 streams of 150 points a frame with the reference's options
(window 11, feat_cap 4096, frame_cap 350); median over the timed cycles.
   python tests/perf/bench_ftable.py [timed cycles]
Per stream count, all in the same run:
  resident_ms   wall clock of the five enqueues + swf_ftable_sync with the frame and the poses in device memory already (on_device = 1)
  host_ms       the same with the frame and the poses in host memory (the hipMemcpyAsync uploads included)
  host_loop_ms  the same specification as a compiled host loop (tests/perf/ftable_host.cpp, g++ -O3), one stream after the other
  share         each operation's part of a cycle, from a pass that synchronises after every operation (device-resident inputs)
The table and the host loop are compared on n_frames, the list lengths and the listing's sizes before anything is reported.
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
import ftable_cases as fc
from rtk_visual_inertial_navigation_amd import solver

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 20
POINTS, DISTINCT, WARM = 150, 4, 3
OPT = solver.ftable_options()
W = OPT.window
CYCLES = WARM + TIMED
N_FRAMES = W - 1 + CYCLES
pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
lib = solver.lib()
SEQ = [fc.make("bench%d" % i, 900 + i, 0.12, POINTS, {}, p_keep=0.85, behind=False, n_frames=N_FRAMES, window=W, frame_cap=OPT.frame_cap,
               feat_cap=OPT.feat_cap) for i in range(DISTINCT)]
EXT = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (fc.TIC, fc.RIC, fc.PBG)]
ext = [a.ctypes.data_as(pd) for a in EXT]

tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "ftable_host.so")
subprocess.check_call(["g++", "-O3", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "ftable_host.cpp")])
hostlib = C.CDLL(so)
hostlib.fth_create.restype = C.c_void_p


def frame_of(E, k):
    """frame k of E streams, packed: first, ids, obs"""
    fr = [SEQ[s % DISTINCT]["frames"][k] for s in range(E)]
    first = np.concatenate([[0], np.cumsum([f["ids"].size for f in fr])]).astype(np.int32)
    return first, np.ascontiguousarray(np.concatenate([f["ids"] for f in fr]), np.int32), np.ascontiguousarray(np.concatenate([f["obs"] for f in fr]))


def poses_of(E, k):
    """the window's poses when frame k is its newest, and the pose of the frame that becomes the oldest"""
    lo = k - (W - 1)
    Ps = np.ascontiguousarray(np.stack([SEQ[s % DISTINCT]["Ps"][lo:k + 1] for s in range(E)]))
    Rs = np.ascontiguousarray(np.stack([SEQ[s % DISTINCT]["Rs"][lo:k + 1] for s in range(E)]).reshape(E, W, 9))
    return Ps, Rs, np.ascontiguousarray(Ps[:, 1]), np.ascontiguousarray(Rs[:, 1])


class Device:
    def __init__(self, E, resident):
        self.E, self.resident = E, resident
        self.T = solver.FeatureTable(E)
        self.h = self.T._h
        self.mode = np.ones(E, np.int32)
        self.keep = []

    def args(self, arrays):
        """the arrays as the call wants them: device tensors, uploaded ahead of the timed region, or the host arrays themselves"""
        held = arrays if not self.resident else [torch.from_numpy(a.reshape(-1)).cuda() for a in arrays]
        self.keep.extend(held)                              # alive until the next cycle's are made
        return [C.c_void_p(a.data_ptr() if self.resident else a.ctypes.data) for a in held]

    def ops(self, k):
        dev = C.c_int32(1 if self.resident else 0)
        self.keep = []
        f = self.args(list(frame_of(self.E, k)))
        Ps, Rs, P1, R1 = self.args(list(poses_of(self.E, k)))
        listing = solver.FtableListingC()
        torch.cuda.synchronize()
        return [("add_frame", lambda: lib.swf_ftable_add_frame(self.h, f[0], f[1], f[2], dev)),
                ("triangulate", lambda: lib.swf_ftable_triangulate(self.h, Ps, Rs, ext[0], ext[1], ext[2], dev)),
                ("list", lambda: lib.swf_ftable_list(self.h, C.byref(listing))),
                ("check_parallax", lambda: lib.swf_ftable_check_parallax(self.h)),
                ("slide", lambda: lib.swf_ftable_slide(self.h, self.mode.ctypes.data_as(pi), None, None, P1, R1, ext[0], ext[1], ext[2], dev))]

    def fill(self):
        for k in range(W - 1):
            first, ids, obs = frame_of(self.E, k)
            assert lib.swf_ftable_add_frame(self.h, first.ctypes.data_as(pi), ids.ctypes.data_as(pi), obs.ctypes.data_as(pd), C.c_int32(0)) == 0
        self.T.sync()

    def run(self, each_op):
        """-> (cycle times, {operation: times}) in ms"""
        self.fill()
        total, per = [], {}
        for c in range(CYCLES):
            ops = self.ops(W - 1 + c)
            t0 = time.perf_counter()
            for name, fn in ops:
                t1 = time.perf_counter()
                assert fn() == 0, (name, lib.swf_last_error())
                if each_op:
                    self.T.sync()
                    per.setdefault(name, []).append((time.perf_counter() - t1) * 1e3)
            self.T.sync()
            total.append((time.perf_counter() - t0) * 1e3)
        return total, per

    def sizes(self):
        nf, n = np.zeros(self.E, np.int32), np.zeros(self.E, np.int32)
        assert lib.swf_ftable_download(self.h, nf.ctypes.data_as(pi), n.ctypes.data_as(pi), *[None] * 9) == 0
        c, _ = self.T.counts()
        return nf, n, c[:, 7].copy(), c[:, 8].copy()        # n_listed, n_proj of the last listing


def host_loop(E):
    h = C.c_void_p(hostlib.fth_create(C.c_int32(E), C.c_int32(W), C.c_int32(OPT.feature_continue), C.c_int32(OPT.min_track), C.c_int32(OPT.min_long),
                                      C.c_int32(OPT.long_len), C.c_double(OPT.new_ratio), C.c_double(OPT.min_parallax), C.c_double(OPT.focal),
                                      C.c_double(OPT.init_depth)))
    key, par, mode = np.zeros(E, np.int32), np.zeros(E), np.ones(E, np.int32)
    cap = E * OPT.frame_cap * (W + 2)
    lf, pf = np.zeros(E + 1, np.int32), np.zeros(E + 1, np.int32)
    li = [np.zeros(cap, np.int32) for _ in range(4)]
    lw, pu = np.zeros(cap * 3), np.zeros(cap * W * 2)
    pj = [np.zeros(cap * W, np.int32) for _ in range(3)]
    p_ = lambda a: a.ctypes.data_as(pd if a.dtype == np.float64 else pi)
    for k in range(W - 1):
        first, ids, obs = frame_of(E, k)
        hostlib.fth_add(h, p_(first), p_(ids), p_(obs), p_(key))
    ts = []
    for c in range(CYCLES):
        k = W - 1 + c
        first, ids, obs = frame_of(E, k)
        Ps, Rs, P1, R1 = poses_of(E, k)
        t0 = time.perf_counter()
        hostlib.fth_add(h, p_(first), p_(ids), p_(obs), p_(key))
        hostlib.fth_triangulate(h, p_(Ps), p_(Rs), *ext)
        hostlib.fth_list(h, p_(lf), p_(pf), p_(li[0]), p_(lw), p_(li[1]), p_(li[2]), p_(li[3]), p_(pj[0]), p_(pj[1]), p_(pu), p_(pj[2]))
        hostlib.fth_parallax(h, p_(key), p_(par))
        hostlib.fth_slide(h, p_(mode), p_(P1), p_(R1), *ext)
        ts.append((time.perf_counter() - t0) * 1e3)
    nf, n = np.zeros(E, np.int32), np.zeros(E, np.int32)
    hostlib.fth_state(h, p_(nf), p_(n))
    hostlib.fth_destroy(h)
    return ts, (nf, n, np.diff(lf), np.diff(pf))


med = lambda v: float(np.median(v[WARM:]))
out = dict(points=POINTS, window=W, feat_cap=OPT.feat_cap, timed_cycles=TIMED, warm_cycles=WARM)
for E in (1, 8, 64):
    res = {}
    for resident in (True, False):
        D = Device(E, resident)
        try:
            total, _ = D.run(False)
            res["resident_ms" if resident else "host_ms"] = round(med(total), 4)
            sizes = D.sizes()
        finally:
            D.T.close()
    D = Device(E, True)
    try:
        _, per = D.run(True)
    finally:
        D.T.close()
    ts, host_sizes = host_loop(E)
    for a, b in zip(sizes, host_sizes):                     # the table and the host loop agree on where the cycles end
        assert np.array_equal(a, b), (E, a, b)
    each = {k: med(v) for k, v in per.items()}
    res.update(host_loop_ms=round(med(ts), 4), features=int(sizes[1].sum()), listed=int(sizes[2].sum()), projections=int(sizes[3].sum()),
               share={k: round(v / sum(each.values()), 3) for k, v in each.items()}, per_op_synced_ms={k: round(v, 4) for k, v in each.items()},
               below_host_loop=bool(res["resident_ms"] < med(ts)))
    out["streams%d" % E] = res
print(json.dumps(out))
