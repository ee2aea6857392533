"""Time the device chain of the ambiguity search's pair selection (swf_batch_select_ambiguity_pairs +
swf_batch_ambiguity_search_selected) against the path it replaces, for 1, 64 and 512 RTK windows
(synth.make_window(3, K=4, F=16, S=16, head="ambiguities"): 16 ambiguities as 3 epochs over 4 classes).
   python tests/perf/bench_dd_select.py [reps]
Per batch size (warm, median of `reps`, host clock from the first call to the end of swf_batch_sync):
  device_chain_ms   select + selected search + sync
  select_ms         swf_batch_select_ambiguity_pairs alone + sync (host checks, one upload, k_dd_select)
  host_path_ms      swf_batch_download_state, the tail values gathered from the windows, the selection as a compiled host loop
                    (tests/perf/dd_select_host.cpp, g++ -O2), swf_batch_ambiguity_search with the pairs (upload + search) + sync
  host_select_ms    the compiled host loop alone
The two paths' pairs are compared before anything is timed.  Prints one JSON line."""
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
from rtk_visual_inertial_navigation_amd import solver, synth
from rtk_visual_inertial_navigation_amd.flat import default_options

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
S, DISTINCT, GATE = 16, 8, 1.4
lib = solver.lib()
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "dd_select_host.so")
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perf", "dd_select_host.cpp")])
host = C.CDLL(so)
pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
LAYOUT = [[(t % 4, t) for t in range(S) if (t + e) % 4 != 0] for e in range(3)]


def host_ms(fn, reps):
    ts = []
    fn()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


out = dict(reps=REPS, S=S, epochs=3)
base = [synth.make_window(3, K=4, F=16, S=S, seed=900 + i, head="ambiguities") for i in range(DISTINCT)]
for W in (1, 64, 512):
    ws = [base[i % DISTINCT].copy() for i in range(W)]
    bs = solver.BatchSolver(ws)
    bs.solve(default_options())
    bs.tail_covariance()
    bs.sync()
    h = bs._h
    ef, of, obs = solver._dd_flatten([LAYOUT] * W)
    gate = np.full(W, GATE)
    yf = (np.arange(W + 1) * S).astype(np.int32)
    off = ws[0].n_pose + ws[0].n_sb + ws[0].n_lm
    tail_idx = [np.asarray(w.a["order_block"][-S:]) - off for w in ws]
    pairs, counts = np.zeros((W, 64, 2), np.int32), np.zeros((W, 4), np.int32)
    first = np.zeros(W + 1, np.int32)

    def device_chain():
        assert lib.swf_batch_select_ambiguity_pairs(h, ef.ctypes.data_as(pi), of.ctypes.data_as(pi), obs.ctypes.data_as(pi), gate.ctypes.data_as(pd)) == 0, lib.swf_last_error()
        assert lib.swf_batch_ambiguity_search_selected(h, C.c_double(2.0)) == 0, lib.swf_last_error()
        bs.sync()

    def select_only():
        assert lib.swf_batch_select_ambiguity_pairs(h, ef.ctypes.data_as(pi), of.ctypes.data_as(pi), obs.ctypes.data_as(pi), gate.ctypes.data_as(pd)) == 0
        bs.sync()

    def host_select(y):
        host.dd_select_host(C.c_int32(W), ef.ctypes.data_as(pi), of.ctypes.data_as(pi), obs.ctypes.data_as(pi), yf.ctypes.data_as(pi),
                            y.ctypes.data_as(pd), gate.ctypes.data_as(pd), pairs.ctypes.data_as(pi), counts.ctypes.data_as(pi))

    def host_path():
        bs.download_state()
        y = np.concatenate([w.a["sc"][ix] for w, ix in zip(ws, tail_idx)])
        host_select(y)
        n = np.where(counts[:, 3] == 0, counts[:, 0], 0)
        first[1:] = np.cumsum(n)
        flat = np.ascontiguousarray(np.concatenate([pairs[w, :n[w]] for w in range(W)] + [np.zeros((1, 2), np.int32)]))
        assert lib.swf_batch_ambiguity_search(h, first.ctypes.data_as(pi), flat.ctypes.data_as(pi), C.c_double(2.0)) == 0, lib.swf_last_error()
        bs.sync()

    # the two paths choose the same pairs
    host_path()
    hp, hc = pairs.copy(), counts.copy()
    device_chain()
    for w in range(W):
        d = bs.ambiguity_pairs(w)
        assert [d["n_pairs"], d["last_count"], d["last_ref_count"], d["info"]] == list(hc[w]) and np.array_equal(d["pairs"], hp[w, :d["n_pairs"]]), w
    y0 = np.concatenate([w.a["sc"][ix] for w, ix in zip(ws, tail_idx)])
    out["w%d" % W] = dict(device_chain_ms=round(host_ms(device_chain, REPS), 4), select_ms=round(host_ms(select_only, REPS), 4),
                          host_path_ms=round(host_ms(host_path, REPS), 4), host_select_ms=round(host_ms(lambda: host_select(y0), REPS), 4),
                          ok=int((hc[:, 3] == 0).sum()))
    bs.close()
print(json.dumps(out))
