"""Bit-identity comparisons of the solver's launch paths — TEST INFRASTRUCTURE, every name defined once.

Window edits:   with_constant holds blocks constant and re-issues the elimination ordering.
In process:     a batch against the same windows solved alone (solve_alone, solve_batch, assert_batch_equals_singles, ...).  The
                batch is created under SWF_NO_LAT_FUSE=1 (`no_lat_fuse=True`: a handful of small windows takes the batch kernels)
                or with the environment as it stands (`no_lat_fuse=False`); every caller says which.
Child process:  a path against the one behind an SWF_* knob.  The knobs are read when a batch is created, so each side of a
                comparison is a fresh `python tests/bitwise.py MODULE CASE PATH`: it imports the test module MODULE, calls its
                child(CASE) -> dict of arrays (composed from dump_solve / dump_elimination) and saves the dict as PATH (.npz).
                solve_in_child starts it with every knob the library reads scrubbed from the environment, and loads the file;
                assert_same_bytes compares two of them."""
import ctypes
import ctypes.util
import importlib
import os
import subprocess
import sys
from contextlib import contextmanager, nullcontext

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pose", "sb", "lm", "sc")
ELIMINATE_ONLY = 1                # step_mode SWF_ASSEMBLE_ELIMINATE_ONLY: linearise, eliminate, assemble, factor — no step
SUMMARY_FIELDS = ("initial_cost", "final_cost", "minimizer_time_in_seconds", "num_successful_steps", "num_unsuccessful_steps",
                  "num_iterations", "termination", "reduced_dim", "tail_dim")
TRACE_FIELDS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius",
                "model_cost_change", "step_is_successful", "step_is_valid")
# every environment variable csrc/ reads (tests/test_bitwise_support.py holds this list to the source)
ENV_KNOBS = ("SWF_NO_COMP_FUSE", "SWF_NO_SPEC_EVAL", "SWF_NO_STEP_FUSE", "SWF_NO_DECIDE_FUSE", "SWF_FULL_FINAL_ELIM", "SWF_NO_CLIQUE_PACK",
             "SWF_NO_CLIQUE_MFMA", "SWF_FORCE_MARG_RESCUE", "SWF_NO_LAT_FUSE", "SWF_NO_CHOL_COL", "SWF_LS_VARIANT", "SWF_LS_QPB",
             "SWF_LS_GRAD_QPB", "SWF_TRACE_REBUILD")


# ---------------------------------------------------------------------------------------------------------------- window edits
def with_constant(win, blocks, store_roles=False):
    """A copy of the window with the given global blocks held constant (pose p is block p, landmark l is win.bid_lm(l)) and the
    elimination ordering re-issued for the new set of variable blocks.  store_roles: the copy's meta["roles"] becomes the
    normalised dict the ordering was issued from (tests/linearize_cases.py edits it further); otherwise it stays the input's."""
    from rtk_visual_inertial_navigation_amd.ordering import my_ordering
    w = win.copy()
    roles = {k: (list(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in w.meta["roles"].items()}
    is_const = w.a["is_const"].copy()
    is_const[list(blocks)] = 1
    o_b, o_g, nt = my_ordering(roles, is_const)
    w.a["is_const"] = np.ascontiguousarray(is_const, np.uint8)
    w.a["order_block"], w.a["order_group"], w.n_tail = o_b, o_g, int(nt)
    if store_roles:
        w.meta["roles"] = roles
    return w


def with_constant_pose_and_landmark(win, pose=2, landmark=3):
    """One pose block and one landmark block held constant: their observations then carry no pose / no landmark Jacobian."""
    return with_constant(win, [pose, win.bid_lm(landmark)])


# ------------------------------------------------------------------------------------------------- in process: batch == single
def rel(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@contextmanager
def batch_kernels():
    """SWF_NO_LAT_FUSE=1 while a batch is created and solved (the knob is read when the plan is built)."""
    old = os.environ.get("SWF_NO_LAT_FUSE")
    os.environ["SWF_NO_LAT_FUSE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["SWF_NO_LAT_FUSE"]
        else:
            os.environ["SWF_NO_LAT_FUSE"] = old


def multi_processor_count():
    """hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount) of the current device, from the HIP runtime the library links."""
    from rtk_visual_inertial_navigation_amd import solver
    solver.lib()
    hip = ctypes.CDLL(ctypes.util.find_library("amdhip64") or "libamdhip64.so")
    n, dev = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.hipGetDevice(ctypes.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), 63, dev) == 0          # 63: hipDeviceAttributeMultiprocessorCount
    assert 1 <= n.value <= 1024, n.value
    return n.value


def solve_alone(w, opt, batch_shapes=False):
    """One window by itself: on the latency path (other launches, the same sums under dogleg), or, batch_shapes, through the batch
    kernels.  -> (solved copy, iterations, cost column, step_is_successful column, termination)"""
    from rtk_visual_inertial_navigation_amd import solver
    c = w.copy()
    with (batch_kernels() if batch_shapes else nullcontext()):
        bs = solver.BatchSolver([c])
        sm = bs.solve(opt)[0]
    out = (c, sm.num_iterations, [r["cost"] for r in sm.rows()], [r["step_is_successful"] for r in sm.rows()], sm.termination)
    bs.close()
    return out


def solve_batch(ws, opt, *, no_lat_fuse):
    """Copies of the windows solved as one batch.  -> (solved copies, summaries)"""
    from rtk_visual_inertial_navigation_amd import solver
    batch = [w.copy() for w in ws]
    with (batch_kernels() if no_lat_fuse else nullcontext()):
        bs = solver.BatchSolver(batch)
        sms = bs.solve(opt)
        bs.close()
    return batch, sms


def assert_window_equal(i, single, wb, sm):
    """Window i of a batch (wb, its summary sm) ended on the bytes of its solve_alone: iterations, both trace columns, the state."""
    c, nit, costs, ok, _ = single
    assert sm.num_iterations == nit, i
    assert [r["cost"] for r in sm.rows()] == costs, i
    assert [r["step_is_successful"] for r in sm.rows()] == ok, i
    for k in KEYS:
        assert np.array_equal(c.a[k], wb.a[k]), (i, k)


def assert_batch_equals_singles(ws, opt, *, no_lat_fuse, batch_shapes=False):
    singles = [solve_alone(w, opt, batch_shapes) for w in ws]
    batch, sms = solve_batch(ws, opt, no_lat_fuse=no_lat_fuse)
    for i, (single, wb, sm) in enumerate(zip(singles, batch, sms)):
        assert_window_equal(i, single, wb, sm)
    return singles, sms


def assert_reduced_system_matches_oracle_and_single(ws):
    """ELIMINATE_ONLY through the batch (the environment as it stands): every window's exported reduced system equals, bit for
    bit, what the window alone exports, and matches the CPU oracle's at the tolerances of tests/test_gpu_parity.py."""
    import oracle_binding as ob
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    opt = default_options(step_mode=ELIMINATE_ONLY)
    alone = []
    for w in ws:
        bs = solver.BatchSolver([w.copy()])
        bs.solve(opt)
        alone.append((bs.export_reduced(0), bs.export_vectors(0)))
        bs.close()
    bs = solver.BatchSolver([w.copy() for w in ws])
    bs.solve(opt)
    for i, w in enumerate(ws):
        S, rhs, L = bs.export_reduced(i)
        g, dg, y = bs.export_vectors(i)
        (S1, rhs1, L1), (g1, dg1, y1) = alone[i]
        assert np.array_equal(S, S1) and np.array_equal(rhs, rhs1) and np.array_equal(L, L1), i
        assert np.array_equal(g, g1) and np.array_equal(dg, dg1) and np.array_equal(y, y1), i
        _, eo = ob.solve(w.copy(), opt)
        assert rel(S, eo["S"]) < 1e-11 and np.abs(S - S.T).max() == 0, i
        assert rel(rhs, eo["rhs"]) < 1e-10, i
        assert rel(g, eo["grad"]) < 1e-11 and rel(dg, eo["diag"]) < 1e-11, i
    bs.close()


# ------------------------------------------------------------------------------------------------------- child process: A / B
def dump_solve(ws, sms):
    """The solved windows' states, every summary field and the whole iteration trace, keyed w%d_state_* / _summary_* / _trace_*."""
    out = {}
    for i, (w, sm) in enumerate(zip(ws, sms)):
        for k, v in w.state().items():
            out["w%d_state_%s" % (i, k)] = v
        for f in SUMMARY_FIELDS:
            out["w%d_summary_%s" % (i, f)] = np.array(getattr(sm, f))
        rows = sm.rows()
        for f in TRACE_FIELDS:
            out["w%d_trace_%s" % (i, f)] = np.array([r[f] for r in rows])
    return out


def dump_elimination(ws):
    """The linearisation at the uploaded state alone (a step_mode = 1 solve of a batch of its own): the reduced system and the
    local vectors the eliminations wrote, keyed w%d_elim_S / _rhs / _g / _diag."""
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    out = {}
    bs = solver.BatchSolver(ws)
    bs.solve(default_options(step_mode=ELIMINATE_ONLY), download=False)
    for i in range(len(ws)):
        S, rhs, _ = bs.export_reduced(i)
        g, d, _ = bs.export_vectors(i)
        out["w%d_elim_S" % i] = S; out["w%d_elim_rhs" % i] = rhs; out["w%d_elim_g" % i] = g; out["w%d_elim_diag" % i] = d
    bs.close()
    return out


def solve_in_child(module, case, path, env, *, batch_kernels):
    """child(case) of the test module, in a fresh process whose environment holds none of ENV_KNOBS but SWF_NO_LAT_FUSE=1 where
    batch_kernels is set, and then `env`.  -> the dict the child saved"""
    e = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    if batch_kernels:
        e["SWF_NO_LAT_FUSE"] = "1"
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), module, case, path], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def assert_same_bytes(a, b, keys=None, nan_equal=True):
    """The two dicts have the same keys and, under `keys` (default: all), arrays of one dtype, shape and byte string.  nan_equal=False:
    the arrays compare equal as numbers too, so a NaN anywhere fails."""
    assert sorted(a) == sorted(b)
    for k in sorted(a) if keys is None else keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert nan_equal or np.array_equal(a[k], b[k]), k


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    np.savez(sys.argv[3], **importlib.import_module(sys.argv[1]).child(sys.argv[2]))
