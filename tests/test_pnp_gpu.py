"""Batched RANSAC PnP on the device (swf_pnp_frame_batch) against the numpy referee of tests/np_pnp.py, stage by stage: each
stage is checked against the referee fed with the device's own previous stage, so one flipped decision can neither cascade into a
false failure nor hide a real one.

  samples            equal the referee's table, exactly
  hyp                within M_HYP x bracket of the longdouble minimal solves on the same samples, for the hypotheses whose 6 x 6 systems
                     stay below a condition number of 1e8 (for the others validity may differ)
  count, inlier      recomputed in longdouble from the device's hyp: equal outside the margin of 1e-9 (relative, on the squared error
                     against the threshold; absolute on z); sure count <= count <= sure count + borderline points
  best, n_iters      equal a replay of the scan on the device's own count
  Ps_out, Rs_out     within M_REF x bracket of the longdouble refinement from the device's hyp[best] over the device's mask
  end to end         the decided frames (pnp_cases.undecided) equal the pure referee in info, best, n_iters, n_inliers and the mask

bracket = 2^-52 cond(A) max(1, |t|); M_HYP = 2, M_REF = 1 are derived in tests/test_pnp.py.  Every test prints the largest
`deviation / bracket`.  Largest on MI355X: hyp 0.142, refinement 0.0150 (the 257-frame call)."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import np_pnp as npp
import pnp_cases as pc
import pnp_gen as pg
from pnp_cases import M_HYP, M_REF
from shim import compile_shim
from rtk_visual_inertial_navigation_amd import solver

SENTINEL = -7.0
MARGIN = 1e-9
pi = C.POINTER(C.c_int32)
pd = C.POINTER(C.c_double)
pb = C.POINTER(C.c_uint8)
KEYS = ("Ps", "Rs", "n_inliers", "best", "n_iters", "info", "samples", "hyp", "count")


def _flag(frames):
    """flag bit 0 is an argument of the call: its frames agree on it"""
    assert len({f["flags"] for f in frames}) == 1
    return frames[0]["flags"]


def run(frames, iterations=pg.ITERATIONS):
    return solver.pnp_frame_batch(*pg.pack(frames), *pc.ARGS, iterations=iterations, threshold=pg.THRESHOLD, confidence=pg.CONFIDENCE,
                                  seed=pg.SEED, flags=_flag(frames), fill=SENTINEL, stages=True)


def run_mixed(frames, iterations=pg.ITERATIONS):
    """flag bit 0 is an argument of the call: frames of both kinds go in two calls, merged into one result in the frames' order"""
    out = None
    for fl in (0, 1):
        idx = [k for k, f in enumerate(frames) if f["flags"] == fl]
        if not idx:
            continue
        part = run([frames[k] for k in idx], iterations)
        if out is None:
            sizes = np.array([f["n"] for f in frames])
            first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            out = {k: np.full((len(frames),) + part[k].shape[1:], SENTINEL if part[k].dtype == np.float64 else int(SENTINEL), part[k].dtype) for k in KEYS}
            out["first"], out["inlier"] = first, np.full(int(first[-1]), 255, np.uint8)
        for j, k in enumerate(idx):
            for key in KEYS:
                out[key][k] = part[key][j]
            out["inlier"][out["first"][k]:out["first"][k + 1]] = part["inlier"][part["first"][j]:part["first"][j + 1]]
    return out


@functools.lru_cache(maxsize=None)
def device(which):
    """the shape frames carry both flag values: two calls; the 257 batch frames share one: a single call"""
    return run_mixed(pc.frames_of(which)) if which == "shape" else run(pc.frames_of(which))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b, ka, kb):
    """every output of frame ka of result a equals frame kb of result b"""
    ok = all(np.array_equal(bits(a[key][ka]), bits(b[key][kb])) for key in KEYS)
    return ok and np.array_equal(a["inlier"][a["first"][ka]:a["first"][ka + 1]], b["inlier"][b["first"][kb]:b["first"][kb + 1]])


def frame_untouched(res, k):
    lo, hi = int(res["first"][k]), int(res["first"][k + 1])
    return (all((res[key][k] == (SENTINEL if res[key].dtype == np.float64 else int(SENTINEL))).all() for key in KEYS if key != "info")
            and (res["inlier"][lo:hi] == 255).all())


def check_stages(frames, res, iterations, pure, label):
    """the six stage checks and the sentinel check for one result; returns the largest deviation / bracket of hyp and of the pose"""
    worst_h = worst_r = 0.0
    decided = 0
    for k, f in enumerate(frames):
        code = pc.expected_code(f)
        tag = (label, k, f["seed"])
        if code != npp.OK:
            assert res["info"][k] == code and frame_untouched(res, k), tag
            continue
        assert res["info"][k] == npp.OK, tag
        pw, uv = npp.stage_points(f["pts_w"], f["pts_uv"], f["flags"])
        n, m = f["n"], 5 if f["n"] >= 5 else 4
        lo, hi = int(res["first"][k]), int(res["first"][k + 1])
        # 1: the samples
        samples, _ = npp.sample_table(n, iterations, pg.SEED)
        H = samples.shape[0]
        assert np.array_equal(res["samples"][k][:H], samples), tag
        for key in ("samples", "hyp", "count"):                              # a frame of 4 points owns one row: the tail keeps the sentinel
            assert (res[key][k][H:] == int(SENTINEL)).all(), tag
        hyp, count = res["hyp"][k][:H], res["count"][k][:H]
        # 2: the minimal solves
        R0, t0 = npp.guess(f["Ps_prev"], f["Rs_prev"], *pc.ARGS, np.longdouble)
        ms = npp.minimal_solves(pw, uv, samples, R0, t0, np.longdouble)
        use = ms["cond"] <= pc.COND_MAX
        valid = np.isfinite(hyp).all(axis=1)
        assert (np.isnan(hyp).all(axis=1) == ~valid).all(), tag            # a row is whole or NaN
        assert valid[use].all(), tag
        if use.any():
            ratio = np.abs(hyp[use] - ms["hyp"][use]).astype(np.float64).max(axis=1) / pc.hyp_bracket(ms["cond"], ms["hyp"])[use]
            worst_h = max(worst_h, float(ratio.max()))
            assert ratio.max() <= M_HYP, tag + (float(ratio.max()),)
        # 3: the counts and the mask, from the device's own hypotheses
        sc = npp.score(pw, uv, hyp, pg.THRESHOLD, np.longdouble)
        thr2 = np.longdouble(sc["thr2"])
        border = sc["valid"][:, None] & ((np.abs(sc["e2"] - thr2) <= MARGIN * thr2) | (np.abs(sc["z"]) <= MARGIN))
        sure = (sc["mask"] & ~border).sum(axis=1)
        assert (count[~valid] == 0).all(), tag
        assert ((sure <= count) & (count <= sure + border.sum(axis=1))).all(), tag
        # 4: the scan, on the device's own counts
        sn = npp.scan(count, n, m, iterations, pg.CONFIDENCE)
        assert (res["best"][k], res["n_iters"][k], res["n_inliers"][k]) == (sn["best"], sn["n_iters"], sn["best_count"]), tag
        b = sn["best"]
        mask = res["inlier"][lo:hi]
        assert set(mask.tolist()) <= {0, 1} and mask.sum() == count[b], tag
        free = ~border[b]
        assert np.array_equal(mask.astype(bool)[free], sc["mask"][b][free]), tag
        # 5: the refinement from the device's hypothesis over the device's mask
        rf = npp.refine(pw, uv, hyp[b], mask.astype(bool), np.longdouble)
        assert rf["ok"], tag
        Ps, Rs = npp.to_imu(rf["R"], rf["t"], *pc.ARGS, np.longdouble)
        br = pc.EPS * rf["cond"] * pc.tnorm(rf["t"])
        ratio = float(max(np.abs(res["Ps"][k] - Ps).max(), np.abs(res["Rs"][k].reshape(3, 3) - Rs).max())) / br
        worst_r = max(worst_r, ratio)
        assert ratio <= M_REF, tag + (ratio,)
        # 6: end to end against the pure referee, where no decision is within reach of rounding
        r = pure[k]
        if not pc.undecided(r):
            decided += 1
            assert (res["info"][k], res["best"][k], res["n_iters"][k], res["n_inliers"][k]) == (r["info"], r["best"], r["n_iters"], r["n_inliers"]), tag
            assert np.array_equal(mask.astype(bool), r["inlier"]), tag
    print("%s: %d frames (%d decided), deviation / bracket: hyp %.3f (M_HYP %.0f), pose %.4f (M_REF %.0f)" %
          (label, len(frames), decided, worst_h, M_HYP, worst_r, M_REF))
    return worst_h, worst_r


@pytest.mark.gpu
def test_point_counts_match_referee():
    """3, 4, 5, 6, 8, 63, 64, 65 and 200 points, flag bit 0 both ways (a call per flag value), and each frame alone, bit for bit"""
    frames = pc.shape_frames()
    res = device("shape")
    check_stages(frames, res, pg.ITERATIONS, pc.referee("shape"), "all point counts")
    for k, f in enumerate(frames):
        one = run([f])
        assert same_bits(one, res, 0, k), (f["n"], f["flags"])
    a, b = [f for f in frames if f["n"] == 200]
    assert a["flags"] != b["flags"]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", pc.ITERATIONS)
def test_iteration_counts(iterations):
    """1, 63, 64, 65, 100 and 128 hypotheses (one lane each: one and two wavefronts) on 4, 5, 65 and 200 points"""
    frames = pc.iteration_frames()
    res = run(frames, iterations)
    pure = pc.referee_iterations(iterations)
    for k, r in enumerate(pure):                      # with few hypotheses a frame may have no model: the referee says which
        if not pc.undecided(r):
            assert res["info"][k] == r["info"], (iterations, k)
        if res["info"][k] == npp.NO_MODEL:
            assert frame_untouched(res, k), (iterations, k)
    keep = [k for k, r in enumerate(pure) if r["info"] == npp.OK and res["info"][k] == npp.OK]
    assert keep or iterations == 1
    sub = {key: res[key][keep] for key in KEYS}
    sizes = [frames[k]["n"] for k in keep]
    sub["first"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sub["inlier"] = np.concatenate([res["inlier"][res["first"][k]:res["first"][k + 1]] for k in keep] + [np.zeros(0, np.uint8)])
    check_stages([frames[k] for k in keep], sub, iterations, [pure[k] for k in keep], "%d iterations" % iterations)


@pytest.mark.gpu
def test_ragged_batch_with_failures():
    """one call of 257 frames of 4 to 120 points with TOO_FEW, BAD_INPUT and NO_MODEL frames mixed in: the stages, and the sentinel in
    everything a failed frame owns"""
    frames = pc.batch_frames()
    res = device("batch")
    assert res["info"].shape == (257,)
    check_stages(frames, res, pg.ITERATIONS, pc.referee("batch"), "257 frames")
    assert sorted(set(res["info"].tolist())) == [npp.OK, npp.TOO_FEW, npp.NO_MODEL, npp.BAD_INPUT]


def _hip(call, *args):
    rc = getattr(solver.lib(), call)(*args)
    assert rc == 0, (call, rc)


class DeviceArrays:
    def __init__(self):
        self.bufs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = C.c_void_p()
        _hip("hipMalloc", C.byref(d), C.c_size_t(max(a.nbytes, 8)))
        self.bufs.append(d)
        if a.nbytes:
            _hip("hipMemcpy", d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1))
        return d

    def down(self, d, a):
        if a.nbytes:
            _hip("hipMemcpy", C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), C.c_int(2))

    def free(self):
        for d in self.bufs:
            solver.lib().hipFree(d)


def _device_memory_call(frames, iterations=pg.ITERATIONS):
    """on_device = 1 over hipMalloc'ed buffers pre-filled with the sentinel; returns the result in run()'s layout"""
    pw, uv, pp, rp = pg.pack(frames)
    nf = len(frames)
    first = np.concatenate([[0], np.cumsum([p.shape[0] for p in pw])]).astype(np.int32)
    tot = int(first[-1])
    out = dict(Ps=np.full((nf, 3), SENTINEL), Rs=np.full((nf, 9), SENTINEL), n_inliers=np.full(nf, int(SENTINEL), np.int32),
               inlier=np.full(tot, 255, np.uint8), best=np.full(nf, int(SENTINEL), np.int32), n_iters=np.full(nf, int(SENTINEL), np.int32),
               info=np.full(nf, -1, np.int32), samples=np.full((nf, iterations, 5), int(SENTINEL), np.int32),
               hyp=np.full((nf, iterations, 12), SENTINEL), count=np.full((nf, iterations), int(SENTINEL), np.int32))
    D = DeviceArrays()
    vec = lambda v, k: (C.c_double * k)(*np.asarray(v, np.float64).reshape(k))
    try:
        ins = [D.up(a) for a in (first, np.concatenate(pw), np.concatenate(uv), pp, rp)]
        o = {k: D.up(v) for k, v in out.items()}
        rc = solver.lib().swf_pnp_frame_batch(C.c_int32(nf), C.cast(ins[0], pi), C.cast(ins[1], pd), C.cast(ins[2], pd), C.cast(ins[3], pd), C.cast(ins[4], pd),
                                              vec(pg.TIC, 3), vec(pg.RIC, 9), vec(pg.PBG, 3), C.c_int32(iterations), C.c_double(pg.THRESHOLD),
                                              C.c_double(pg.CONFIDENCE), C.c_uint64(pg.SEED), C.c_int32(_flag(frames)),
                                              C.cast(o["Ps"], pd), C.cast(o["Rs"], pd), C.cast(o["n_inliers"], pi), C.cast(o["inlier"], pb),
                                              C.cast(o["best"], pi), C.cast(o["n_iters"], pi), C.cast(o["info"], pi), C.cast(o["samples"], pi),
                                              C.cast(o["hyp"], pd), C.cast(o["count"], pi), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        for k, v in out.items():
            D.down(o[k], v)
    finally:
        D.free()
    out["first"] = first
    return out


@pytest.mark.gpu
def test_alone_in_the_batch_host_and_device_memory_bitwise():
    """the one call of 257 frames from host memory, the same call again, the same call from device memory, and frames of it run alone:
    the same bits in every output; failed frames stay untouched in device memory too"""
    frames = pc.batch_frames()
    assert len(frames) == 257 and {f["fail"] for f in frames} == {None, "few", "bad", "nomodel"}
    full = device("batch")
    assert full["info"].shape == (257,)
    again = run(frames)
    dev = _device_memory_call(frames)
    for k, f in enumerate(frames):
        assert same_bits(again, full, k, k), k
        assert same_bits(dev, full, k, k), k
        if f["fail"] is not None:
            assert frame_untouched(dev, k), k
    for k in (0, 1, 2, 4, 17, 19, 20, 40, 254, 256):
        one = run([frames[k]])
        assert same_bits(one, full, 0, k), k
        alone = _device_memory_call([frames[k]])
        assert same_bits(alone, full, 0, k), k


@pytest.mark.gpu
def test_chained_with_triangulation_on_device_memory():
    """Ps_out / Rs_out written into the slot of a frame array on the device that swf_triangulate_batch then reads: the depths equal
    those from the same pose passed through the host, bit for bit"""
    f = pc.shape_frames()[2 * pc.SHAPE_N.index(65) + 1]
    host = run([f])
    assert host["info"][0] == npp.OK
    slot, nfr = 3, 5
    Ps = np.tile(f["Ps_prev"], (nfr, 1)); Rs = np.tile(f["Rs_prev"].reshape(9), (nfr, 1))
    # features first seen in frame slot - 1 (the previous frame) and observed again in the new frame: its true inliers
    keep = np.flatnonzero(~f["outlier"])[:24]
    Rc_prev, Pc_prev = f["Rs_prev"] @ pg.RIC, f["Rs_prev"] @ (pg.TIC - pg.PBG) + f["Ps_prev"]
    pcam = (f["pts_w"][keep] - Pc_prev) @ Rc_prev
    pt0 = np.ascontiguousarray(pcam[:, :2] / pcam[:, 2:3]); pt1 = np.ascontiguousarray(f["pts_uv"][keep])
    start = np.full(keep.size, slot - 1, np.int32)
    Ps_h, Rs_h = Ps.copy(), Rs.copy()
    Ps_h[slot], Rs_h[slot] = host["Ps"][0], host["Rs"][0]
    depth_h, world_h = solver.triangulate_batch(Ps_h, Rs_h.reshape(nfr, 3, 3), pg.TIC, pg.RIC, pg.PBG, start, pt0, pt1)
    D = DeviceArrays()
    vec = lambda v, k: (C.c_double * k)(*np.asarray(v, np.float64).reshape(k))
    depth_d, world_d = np.zeros(keep.size), np.zeros((keep.size, 3))
    sink_i, sink_b = np.zeros(4, np.int32), np.zeros(f["n"], np.uint8)
    try:
        first = np.array([0, f["n"]], np.int32)
        d_first, d_pw, d_uv, d_pp, d_rp = (D.up(a) for a in (first, f["pts_w"], f["pts_uv"], f["Ps_prev"], f["Rs_prev"]))
        d_Ps, d_Rs, d_int, d_in = D.up(Ps), D.up(Rs), D.up(sink_i), D.up(sink_b)
        d_start, d_pt0, d_pt1, d_depth, d_world = D.up(start), D.up(pt0), D.up(pt1), D.up(depth_d), D.up(world_d)
        at = lambda d, off: C.c_void_p(d.value + off)
        rc = solver.lib().swf_pnp_frame_batch(C.c_int32(1), C.cast(d_first, pi), C.cast(d_pw, pd), C.cast(d_uv, pd), C.cast(d_pp, pd), C.cast(d_rp, pd),
                                              vec(pg.TIC, 3), vec(pg.RIC, 9), vec(pg.PBG, 3), C.c_int32(pg.ITERATIONS), C.c_double(pg.THRESHOLD),
                                              C.c_double(pg.CONFIDENCE), C.c_uint64(pg.SEED), C.c_int32(f["flags"]),
                                              C.cast(at(d_Ps, slot * 24), pd), C.cast(at(d_Rs, slot * 72), pd), C.cast(d_int, pi), C.cast(d_in, pb),
                                              C.cast(at(d_int, 4), pi), C.cast(at(d_int, 8), pi), C.cast(at(d_int, 12), pi), None, None, None,
                                              C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        rc = solver.lib().swf_triangulate_batch(C.cast(d_Ps, pd), C.cast(d_Rs, pd), C.c_int32(nfr), vec(pg.TIC, 3), vec(pg.RIC, 9), vec(pg.PBG, 3),
                                                C.cast(d_start, pi), C.cast(d_pt0, pd), C.cast(d_pt1, pd), C.c_int32(keep.size), C.c_double(5.0),
                                                C.cast(d_depth, pd), C.cast(d_world, pd), C.c_int32(1), None)
        assert rc == 0, solver.lib().swf_last_error()
        _hip("hipDeviceSynchronize")
        D.down(d_depth, depth_d); D.down(d_world, world_d); D.down(d_int, sink_i)
        got_Ps = np.zeros((nfr, 3)); D.down(d_Ps, got_Ps)
    finally:
        D.free()
    assert sink_i[3] == npp.OK and np.array_equal(bits(got_Ps[slot]), bits(host["Ps"][0])) and np.array_equal(got_Ps[slot - 1], Ps[slot - 1])
    assert np.array_equal(bits(depth_d), bits(depth_h)) and np.array_equal(bits(world_d), bits(world_h))
    assert (depth_d > 0).all() and (depth_d != 5.0).any()


@pytest.mark.gpu
def test_pnp_adapter_runs(tmp_path):
    exe = compile_shim(tmp_path, "shim_pnp")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "pnp ok" in out.stdout, out.stdout
