"""Host-side mirror of the C-ABI in include/swf_solver.h (ctypes over libswf_hip.so).

Plumbing only: numpy arrays <-> C structs.  All arithmetic of a solve runs in the HIP
kernels; if the library or a GPU is missing every call raises — there is no CPU fallback.
"""
import ctypes as C
import os
import numpy as np

from .flat import FlatWindowC, OptionsC, SummaryC, default_options

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWF_LIB", os.path.join(_HERE, "libswf_hip.so"))   # SWF_LIB: A/B builds for tuning
_pd = C.POINTER(C.c_double)
_lib = None


class SwfError(RuntimeError):
    pass


K_NAMES = ["total", "eval_ps", "eval_imu", "frame_sums", "eval_prior", "lm_schur", "clique_elim", "lm_elim",
           "assemble", "chol_solve", "post_chol", "post_dogleg", "dogleg", "cand_eval", "decide", "unused"]


class TimingC(C.Structure):
    _fields_ = [("ms", C.c_double * 16), ("calls", C.c_int32 * 16), ("jacobian_bytes", C.c_int64),
                ("proj_bytes", C.c_int64), ("chol_flops", C.c_int64), ("lm_schur_flops", C.c_int64), ("n_obs", C.c_int64),
                ("n_linearizations", C.c_int32), ("reserved", C.c_int32),
                ("lm_schur_flops_sym", C.c_int64), ("lm_schur_mfma", C.c_int64)]


EXPORTED = [
    "swf_version", "swf_device_count", "swf_set_device", "swf_last_error",
    "swf_batch_create", "swf_batch_destroy", "swf_batch_upload_state", "swf_batch_reset_state",
    "swf_batch_solve", "swf_batch_sync", "swf_batch_download_state", "swf_batch_summaries",
    "swf_batch_export_reduced", "swf_batch_export_vectors", "swf_batch_export_step", "swf_batch_dims",
    "swf_batch_enable_timing", "swf_batch_timing",
    "swf_problem_create", "swf_problem_destroy", "swf_add_parameter_block", "swf_has_parameter_block",
    "swf_remove_parameter_block", "swf_set_parameter_block_constant", "swf_set_parameter_block_variable",
    "swf_is_parameter_block_constant", "swf_parameter_block_size", "swf_num_parameter_blocks",
    "swf_num_residual_blocks", "swf_add_projection", "swf_add_imu", "swf_add_rtk_carrier_phase",
    "swf_add_rtk_pseudorange", "swf_add_doppler", "swf_add_scalar_prior", "swf_add_linear_prior",
    "swf_remove_factor", "swf_factor_set_enabled", "swf_set_constants", "swf_set_ordering",
    "swf_set_export_tail", "swf_problem_solve", "swf_get_reduced", "swf_problem_marginalize",
    "swf_batch_marginalize", "swf_batch_get_prior",
    "swf_add_spp_pseudorange", "swf_add_spp_carrier_phase", "swf_add_fixed_integer",
    "swf_preintegrate_batch", "swf_triangulate_batch",
    "swf_batch_tail_covariance", "swf_batch_get_tail_covariance", "swf_problem_tail_covariance",
    "swf_composite_create", "swf_composite_evaluate", "swf_composite_hidden", "swf_composite_destroy", "swf_add_imu_gnss",
    "swf_eval_inverse_depth_batch", "swf_add_projection_inverse_depth",
    "swf_factor_is_enabled", "swf_get_residual_blocks", "swf_get_residual_blocks_for_parameter_block",
    "swf_get_parameter_blocks", "swf_get_parameter_blocks_for_residual_block", "swf_batch_export_jacobian",
    "swf_batch_marginal_priors", "swf_composite_assemble",
    "swf_composite_set_mid_links", "swf_composite_add_mid_prior", "swf_set_imu_gnss_mid_link", "swf_composite_set_root",
    "swf_batch_create_on", "swf_batch_create_sharded", "swf_solve_batches", "swf_batch_device", "swf_default_options", "swf_shard_partition",
    "swf_prior_reset_linearization_point",
    "swf_lambda_batch", "swf_batch_ambiguity_search", "swf_batch_get_ambiguity_fix",
    "swf_batch_check_features", "swf_batch_get_feature_check",
    "swf_problem_check_features", "swf_problem_get_feature_check", "swf_problem_rejected_features",
    "swf_prior_fix_batch", "swf_batch_fix_prior", "swf_batch_get_fixed_prior", "swf_batch_install_fixed_prior", "swf_problem_fix_prior",
    "swf_phase_screen_batch",
    "swf_gnss_epoch_solve_batch",
    "swf_dd_select_batch", "swf_batch_select_ambiguity_pairs", "swf_batch_ambiguity_search_selected", "swf_batch_get_ambiguity_pairs",
    "swf_imu_frame_batch", "swf_preintegrate_runs_batch",
    "swf_pnp_frame_batch",
    "swf_track_reject_batch",
    "swf_klt_track_batch", "swf_klt_pyramid_bytes",
    "swf_gftt_detect_batch", "swf_gftt_workspace_bytes",
    "swf_tracker_default_options", "swf_tracker_create", "swf_tracker_track", "swf_tracker_remove_ids", "swf_tracker_download",
    "swf_tracker_device_frame", "swf_tracker_sync", "swf_tracker_destroy",
    "swf_ftable_default_options", "swf_ftable_create", "swf_ftable_add_frame", "swf_ftable_pnp_points", "swf_ftable_triangulate",
    "swf_ftable_list", "swf_ftable_set_solved", "swf_ftable_remove_failures", "swf_ftable_removed", "swf_ftable_check_parallax",
    "swf_ftable_slide", "swf_ftable_download", "swf_ftable_counts", "swf_ftable_fetch", "swf_ftable_sync", "swf_ftable_clear",
    "swf_ftable_destroy",
]


def lib():
    """Load libswf_hip.so (must have been built by build.py / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SwfError("libswf_hip.so not built: run `python -m rtk_visual_inertial_navigation_amd.build` "
                           "(no CPU fallback exists)")
        _lib = C.CDLL(LIB_PATH)
        _lib.swf_last_error.restype = C.c_char_p
    return _lib


def _chk(rc, what):
    if rc != 0:
        raise SwfError("%s failed (%d): %s" % (what, rc, lib().swf_last_error().decode()))


def device_count():
    n = C.c_int32()
    rc = lib().swf_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def set_device(d):
    _chk(lib().swf_set_device(C.c_int32(d)), "swf_set_device")


class BatchSolver:
    """A batch of flat windows resident on the current HIP device (swf_batch_*), or on `device` (swf_batch_create_on)."""

    def __init__(self, windows, stream=None, device=None, _handle=None):
        self.windows = list(windows)
        self.n = len(self.windows)
        if _handle is not None:                      # adopted from swf_batch_create_sharded
            self._structs = None
            self._h = _handle
            return
        self._structs = [w.c_struct() for w in self.windows]
        arr = (C.POINTER(FlatWindowC) * len(self._structs))(*[C.pointer(s) for s in self._structs])
        self._h = C.c_void_p()
        if device is None:
            _chk(lib().swf_batch_create(arr, C.c_int32(len(self._structs)), C.c_void_p(stream or 0), C.byref(self._h)), "swf_batch_create")
        else:
            _chk(lib().swf_batch_create_on(C.c_int32(device), arr, C.c_int32(len(self._structs)), C.c_void_p(stream or 0), C.byref(self._h)),
                 "swf_batch_create_on")

    def device(self):
        d = C.c_int32(-1)
        _chk(lib().swf_batch_device(self._h, C.byref(d)), "swf_batch_device")
        return d.value

    def close(self):
        if self._h:
            lib().swf_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_state(self):
        _chk(lib().swf_batch_upload_state(self._h), "swf_batch_upload_state")

    def reset_state(self):
        _chk(lib().swf_batch_reset_state(self._h), "swf_batch_reset_state")

    def solve_async(self, opt=None):
        self._opt = opt if opt is not None else default_options()
        _chk(lib().swf_batch_solve(self._h, C.byref(self._opt)), "swf_batch_solve")

    def sync(self):
        _chk(lib().swf_batch_sync(self._h), "swf_batch_sync")

    def solve(self, opt=None, download=True):
        self.solve_async(opt)
        self.sync()
        if download:
            self.download_state()
        return self.summaries()

    def download_state(self):
        _chk(lib().swf_batch_download_state(self._h), "swf_batch_download_state")

    def summaries(self):
        out = (SummaryC * self.n)()
        _chk(lib().swf_batch_summaries(self._h, out), "swf_batch_summaries")
        return list(out)

    def dims(self, w=0):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().swf_batch_dims(self._h, C.c_int32(w), C.byref(a), C.byref(b), C.byref(c)), "swf_batch_dims")
        return dict(n_loc=a.value, n_e=b.value, n_red=c.value)

    def export_reduced(self, w=0):
        n = self.dims(w)["n_red"]
        S, rhs, L = np.zeros((n, n)), np.zeros(n), np.zeros((n, n))
        _chk(lib().swf_batch_export_reduced(self._h, C.c_int32(w), S.ctypes.data_as(_pd), rhs.ctypes.data_as(_pd),
                                            L.ctypes.data_as(_pd)), "swf_batch_export_reduced")
        return S, rhs, L

    def export_vectors(self, w=0):
        n = self.dims(w)["n_loc"]
        g, d, y = np.zeros(n), np.zeros(n), np.zeros(n)
        _chk(lib().swf_batch_export_vectors(self._h, C.c_int32(w), g.ctypes.data_as(_pd), d.ctypes.data_as(_pd),
                                            y.ctypes.data_as(_pd)), "swf_batch_export_vectors")
        return g, d, y

    def export_step(self, w=0):
        """the step of window w's last proposed candidate, n_loc doubles in elimination order (swf_batch_export_step)"""
        step = np.zeros(self.dims(w)["n_loc"])
        _chk(lib().swf_batch_export_step(self._h, C.c_int32(w), step.ctypes.data_as(_pd)), "swf_batch_export_step")
        return step

    def export_jacobian(self, w=0):
        """(r [n_res], J [n_res][n_loc]) of window w's last linearisation as the device holds it (swf_batch_export_jacobian)."""
        nr, nl = C.c_int32(), C.c_int32()
        _chk(lib().swf_batch_export_jacobian(self._h, C.c_int32(w), None, None, C.byref(nr), C.byref(nl)), "swf_batch_export_jacobian")
        r, J = np.zeros(nr.value), np.zeros((nr.value, nl.value))
        _chk(lib().swf_batch_export_jacobian(self._h, C.c_int32(w), r.ctypes.data_as(_pd), J.ctypes.data_as(_pd), C.byref(nr), C.byref(nl)),
             "swf_batch_export_jacobian")
        return r, J

    PRIOR_EIGEN, PRIOR_CHOLESKY = 0, 1

    def marginalize(self, eps=1e-8, form=0):
        """UpdateSchur + setmarginalizeinfo(Sqrt=true) for every window, on the device, from the last
        ASSEMBLE_ELIMINATE_ONLY solve (R/swf/swf_gnss.cpp:25-61, R/factor/marginalization_factor.cpp:449-488)."""
        _chk(lib().swf_batch_marginalize(self._h, C.c_double(eps), C.c_int32(form)), "swf_batch_marginalize")

    def get_prior(self, w=0):
        n, rank = C.c_int32(0), C.c_int32(0)
        _chk(lib().swf_batch_get_prior(self._h, C.c_int32(w), None, None, None, None, None, C.byref(n), C.byref(rank)), "swf_batch_get_prior")
        k = n.value
        A, J, b, r0, eig = np.zeros((k, k)), np.zeros((k, k)), np.zeros(k), np.zeros(k), np.zeros(k)
        _chk(lib().swf_batch_get_prior(self._h, C.c_int32(w), A.ctypes.data_as(_pd), b.ctypes.data_as(_pd), J.ctypes.data_as(_pd),
                                       r0.ctypes.data_as(_pd), eig.ctypes.data_as(_pd), C.byref(n), C.byref(rank)), "swf_batch_get_prior")
        return dict(A=A, b=b, J=J, r0=r0, eig=eig, n=k, rank=rank.value)

    def tail_covariance(self, w=None):
        """UpdateSchurHessianOnly + LambdaSearch's covariance (R/swf/swf_gnss.cpp:65-94, swf_lambda.cpp:94-99): information A and
        covariance Qy = A^-1 of the parameter_head states of every window, from the factor of the last linear solve.
        w = None: list over windows; else one window's dict(A, Qy, n)."""
        _chk(lib().swf_batch_tail_covariance(self._h), "swf_batch_tail_covariance")

        def one(i):
            n = C.c_int32(0)
            _chk(lib().swf_batch_get_tail_covariance(self._h, C.c_int32(i), None, None, C.byref(n)), "swf_batch_get_tail_covariance")
            k = n.value
            A, Q = np.zeros((k, k)), np.zeros((k, k))
            _chk(lib().swf_batch_get_tail_covariance(self._h, C.c_int32(i), A.ctypes.data_as(_pd), Q.ctypes.data_as(_pd), C.byref(n)),
                 "swf_batch_get_tail_covariance")
            return dict(A=A, Qy=Q, n=k)
        return [one(i) for i in range(self.n)] if w is None else one(w)

    def ambiguity_search(self, pairs_per_window, ratio_threshold=2.0):
        """LambdaSearch's numeric core for every window (R/swf/swf_lambda.cpp:82-365), on the device after tail_covariance():
        pairs_per_window[w] = [(tail coordinate of an ambiguity, tail coordinate of its reference ambiguity), ...].  Returns one
        dict per window: F [2][n_b], s [2], ratio [2], fixed, Qb = D Qy D^T, bf = D y, n_b, info (SWF_LAMBDA_*)."""
        first = np.zeros(self.n + 1, np.int32)
        for w, pw in enumerate(pairs_per_window):
            first[w + 1] = first[w] + len(pw)
        flat = np.ascontiguousarray(np.array([q for pw in pairs_per_window for q in pw], np.int32).reshape(-1, 2)) if first[-1] else np.zeros((1, 2), np.int32)
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_batch_ambiguity_search(self._h, first.ctypes.data_as(pi), flat.ctypes.data_as(pi), C.c_double(ratio_threshold)),
             "swf_batch_ambiguity_search")
        out = []
        for w in range(self.n):
            k = len(pairs_per_window[w])
            F, sv, r, Qb, bf = np.zeros((2, k)), np.zeros(2), np.zeros(2), np.zeros((k, k)), np.zeros(k)
            fx, nb, info = C.c_int32(), C.c_int32(), C.c_int32()
            _chk(lib().swf_batch_get_ambiguity_fix(self._h, C.c_int32(w), F.ctypes.data_as(_pd), sv.ctypes.data_as(_pd), r.ctypes.data_as(_pd),
                                                   C.byref(fx), Qb.ctypes.data_as(_pd), bf.ctypes.data_as(_pd), C.byref(nb), C.byref(info)),
                 "swf_batch_get_ambiguity_fix")
            out.append(dict(F=F, s=sv, ratio=r, fixed=bool(fx.value), Qb=Qb, bf=bf, n_b=nb.value, info=info.value))
        return out

    def _ambiguity_fix(self, w, k):
        F, sv, r, Qb, bf = np.zeros((2, k)), np.zeros(2), np.zeros(2), np.zeros((k, k)), np.zeros(k)
        fx, nb, info = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().swf_batch_get_ambiguity_fix(self._h, C.c_int32(w), F.ctypes.data_as(_pd), sv.ctypes.data_as(_pd), r.ctypes.data_as(_pd),
                                               C.byref(fx), Qb.ctypes.data_as(_pd), bf.ctypes.data_as(_pd), C.byref(nb), C.byref(info)),
             "swf_batch_get_ambiguity_fix")
        return dict(F=F, s=sv, ratio=r, fixed=bool(fx.value), Qb=Qb, bf=bf, n_b=nb.value, info=info.value)

    def select_ambiguity_pairs(self, epochs_per_window, gate):
        """The double-difference pairs of the search chosen on the device (FindReferenceSatellites and LambdaSearch's D3 loop,
        R/swf/swf_lambda.cpp:8-53, 118-188) from the device state, after a solve; asynchronous.  epochs_per_window[w] = the window's
        epochs NEWEST FIRST, each a list of (class = sys * 2 + f, tail coordinate) in the reference's observation order; gate: one
        value or one per window (the reference: 0.2 after a fix, 1.4 otherwise).  Read the result with ambiguity_pairs(w)."""
        if len(epochs_per_window) != self.n:
            raise ValueError("select_ambiguity_pairs: one epoch list per window")
        ef, of, obs = _dd_flatten(epochs_per_window)
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gate, np.float64), (self.n,)))
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_batch_select_ambiguity_pairs(self._h, ef.ctypes.data_as(pi), of.ctypes.data_as(pi), obs.ctypes.data_as(pi), g.ctypes.data_as(_pd)),
             "swf_batch_select_ambiguity_pairs")
        self._dd_shape = [(len(ep), sum(len(e) for e in ep)) for ep in epochs_per_window]

    def ambiguity_pairs(self, w=0):
        """Window w's selection (synchronises): dict(pairs [n_pairs][2], raw_pairs [64][2] with -1 behind the pairs, n_pairs,
        last_count, last_ref_count, info (DDSEL_*), refs [epochs][6], cost [observations], role [observations])."""
        ne, no = self._dd_shape[w] if getattr(self, "_dd_shape", None) else (0, 0)
        pairs, counts = np.zeros((LAMBDA_NMAX, 2), np.int32), np.zeros(4, np.int32)
        refs, cost, role = np.zeros((max(ne, 1), 6), np.int32), np.zeros(max(no, 1)), np.zeros(max(no, 1), np.uint8)
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_batch_get_ambiguity_pairs(self._h, C.c_int32(w), pairs.ctypes.data_as(pi), counts.ctypes.data_as(pi), refs.ctypes.data_as(pi),
                                                 cost.ctypes.data_as(_pd), role.ctypes.data_as(C.POINTER(C.c_uint8))), "swf_batch_get_ambiguity_pairs")
        return _dd_result(pairs, counts, refs[:ne], cost[:no], role[:no])

    def ambiguity_search_selected(self, ratio_threshold=2.0, fetch=True):
        """ambiguity_search() on the pairs select_ambiguity_pairs() chose, without leaving the device: needs a selection and a
        tail_covariance() after the last solve.  A window whose selection is not DDSEL_OK reports LAMBDA_NO_INPUT.  fetch = False only
        enqueues; otherwise one dict per window as ambiguity_search() returns."""
        _chk(lib().swf_batch_ambiguity_search_selected(self._h, C.c_double(ratio_threshold)), "swf_batch_ambiguity_search_selected")
        if not fetch:
            return None
        out = []
        for w in range(self.n):
            nb = C.c_int32()
            _chk(lib().swf_batch_get_ambiguity_fix(self._h, C.c_int32(w), None, None, None, None, None, None, C.byref(nb), None), "swf_batch_get_ambiguity_fix")
            out.append(self._ambiguity_fix(w, nb.value))
        return out

    def fix_prior(self, prior_sel=None, n_use=None, enable=None, ignore_ratio=False, scalars_at_zero=True, istd=1.0 / 0.03, eps=1e-8, form=0):
        """Fix and hold (the second half of LambdaSearch, R/swf/swf_lambda.cpp:249-355) for every window, on the device after
        ambiguity_search(): the accepted integers of the search folded into linear prior prior_sel[w] (default 0) of each window.
        n_use[w] = take the first n_use[w] pairs (default all), enable[w] = 0 leaves a window alone.  Asynchronous; read-only until
        install_fixed_prior()."""
        pi, pb = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        ps = None if prior_sel is None else np.ascontiguousarray(prior_sel, np.int32)
        nu = None if n_use is None else np.ascontiguousarray(n_use, np.int32)
        en = None if enable is None else np.ascontiguousarray(enable, np.uint8)
        for a in (ps, nu, en):
            if a is not None and a.size != self.n:
                raise ValueError("fix_prior: one entry per window")
        _chk(lib().swf_batch_fix_prior(self._h, None if ps is None else ps.ctypes.data_as(pi), None if nu is None else nu.ctypes.data_as(pi),
                                       None if en is None else en.ctypes.data_as(pb), C.c_int32(1 if ignore_ratio else 0),
                                       C.c_int32(1 if scalars_at_zero else 0), C.c_double(istd), C.c_double(eps), C.c_int32(form)),
             "swf_batch_fix_prior")
        self._fix_sel = np.zeros(self.n, np.int32) if ps is None else ps.copy()

    def _prior_x0_size(self, w, k):
        """Doubles of the linearisation point of linear prior k of window w (global sizes of its kept blocks)."""
        win = self.windows[w]
        nblk = np.asarray(win.a["prior_nblk"]).ravel()
        b0 = int(nblk[:k].sum())
        ids = np.asarray(win.a["prior_blk"]).ravel()[b0:b0 + int(nblk[k])]
        return int(sum(7 if i < win.n_pose else 9 if i < win.n_pose + win.n_sb else 3 if i < win.n_pose + win.n_sb + win.n_lm else 1 for i in ids))

    def get_fixed_prior(self, w=0):
        """Results of fix_prior() for window w: dict(applied, rank, n, and — when applied — A, b, J, r0, x0, eig)."""
        n, rank, ap = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _chk(lib().swf_batch_get_fixed_prior(self._h, C.c_int32(w), None, None, None, None, None, None, C.byref(n), C.byref(rank), C.byref(ap)),
             "swf_batch_get_fixed_prior")
        out = dict(applied=bool(ap.value), rank=rank.value, n=n.value)
        if not ap.value:
            return out
        k = n.value
        A, J, b, r0, eig, x0 = np.zeros((k, k)), np.zeros((k, k)), np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(self._prior_x0_size(w, int(self._fix_sel[w])))
        _chk(lib().swf_batch_get_fixed_prior(self._h, C.c_int32(w), A.ctypes.data_as(_pd), b.ctypes.data_as(_pd), J.ctypes.data_as(_pd),
                                             r0.ctypes.data_as(_pd), x0.ctypes.data_as(_pd), eig.ctypes.data_as(_pd), C.byref(n), C.byref(rank),
                                             C.byref(ap)), "swf_batch_get_fixed_prior")
        out.update(A=A, b=b, J=J, r0=r0, eig=eig, x0=x0)
        return out

    def install_fixed_prior(self):
        """Write (J', r0', x0') of every applied window into the batch's own prior record (and the clique data derived from it): the
        next solve runs with the fix-and-hold prior, without a rebuild.  upload_state() / reset_state() do not undo it."""
        _chk(lib().swf_batch_install_fixed_prior(self._h), "swf_batch_install_fixed_prior")

    def check_features(self, threshold=2.0):
        """The post-solve feature check of every window on the device (swf_batch_check_features: OutliersRejection's mean
        reprojection error, R/swf/swf_image.cpp:255-308, and Double2Vector's depth sign, R/swf/swf.cpp:214-229) at the state
        download_state() would return.  Features: the window's landmarks in pool order, then its inverse depths ascending.
        Returns one dict per window: mean_err, depth, n_obs, flags (FEAT_* bits), rejected (ascending feature indices), n_feat."""
        _chk(lib().swf_batch_check_features(self._h, C.c_double(threshold)), "swf_batch_check_features")
        return [self.get_feature_check(w) for w in range(self.n)]

    def get_feature_check(self, w=0):
        pi = C.POINTER(C.c_int32)
        nf, nr = C.c_int32(), C.c_int32()
        _chk(lib().swf_batch_get_feature_check(self._h, C.c_int32(w), None, None, None, None, None, None, C.byref(nf)), "swf_batch_get_feature_check")
        k = nf.value
        m, d = np.zeros(k), np.zeros(k)
        no, rj, fl = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.uint8)
        _chk(lib().swf_batch_get_feature_check(self._h, C.c_int32(w), m.ctypes.data_as(_pd), d.ctypes.data_as(_pd), no.ctypes.data_as(pi),
                                               fl.ctypes.data_as(C.POINTER(C.c_uint8)), rj.ctypes.data_as(pi), C.byref(nr), C.byref(nf)),
             "swf_batch_get_feature_check")
        return dict(mean_err=m, depth=d, n_obs=no, flags=fl, rejected=rj[:nr.value].copy(), n_feat=k)

    def enable_timing(self, mask=1):
        """mask: bit k brackets kernel K_NAMES[k] with a HIP event pair per launch (bit 0 = whole solve);
        True = everything."""
        if mask is True:
            mask = 0xffff
        _chk(lib().swf_batch_enable_timing(self._h, C.c_int32(int(mask))), "swf_batch_enable_timing")

    def timing(self):
        t = TimingC()
        _chk(lib().swf_batch_timing(self._h, C.byref(t)), "swf_batch_timing")
        d = dict(jacobian_bytes=t.jacobian_bytes, proj_bytes=t.proj_bytes, chol_flops=t.chol_flops,
                 lm_schur_flops=t.lm_schur_flops, lm_schur_flops_sym=t.lm_schur_flops_sym, lm_schur_mfma=t.lm_schur_mfma, n_obs=t.n_obs,
                 n_linearizations=t.n_linearizations, total_ms=t.ms[0])
        d["kernels"] = {K_NAMES[k]: dict(ms=t.ms[k], calls=t.calls[k]) for k in range(16) if t.calls[k]}
        return d


class ShardedBatchSolver:
    """Windows sharded over the GPUs of one node from ONE process (swf_batch_create_sharded + swf_solve_batches): contiguous, near-equal
    blocks per device of `device_mask` (0 = every visible device), no data-path collective, one host thread driving every device."""

    def __init__(self, windows, device_mask=0):
        self.windows = list(windows)
        self._structs = [w.c_struct() for w in self.windows]
        n = len(self._structs)
        arr = (C.POINTER(FlatWindowC) * n)(*[C.pointer(s) for s in self._structs])
        cap = max(1, device_count())
        hs = (C.c_void_p * cap)(); first = (C.c_int32 * cap)(); count = (C.c_int32 * cap)(); nb = C.c_int32(0)
        _chk(lib().swf_batch_create_sharded(arr, C.c_int32(n), C.c_uint32(device_mask), hs, first, count, C.byref(nb)), "swf_batch_create_sharded")
        self.parts = [(first[k], count[k]) for k in range(nb.value)]
        self.batches = [BatchSolver(self.windows[first[k]:first[k] + count[k]], _handle=C.c_void_p(hs[k])) for k in range(nb.value)]

    def solve(self, opt=None, download=True):
        self._opt = opt if opt is not None else default_options()
        hs = (C.c_void_p * len(self.batches))(*[b._h for b in self.batches])
        _chk(lib().swf_solve_batches(hs, C.c_int32(len(self.batches)), C.byref(self._opt)), "swf_solve_batches")
        out = []
        for b in self.batches:
            if download:
                b.download_state()
            out += b.summaries()
        return out

    def close(self):
        for b in self.batches:
            b.close()
        self.batches = []


class Problem:
    """ceres::Problem-shaped host mirror (swf_problem_*).  Parameter blocks are numpy float64
    arrays owned by the caller and identified by address, as in Ceres; Solve() reads them and
    writes the result back in place.  Method names follow the ceres::Problem members the
    reference uses."""

    def __init__(self):
        self._h = C.c_void_p()
        _chk(lib().swf_problem_create(C.byref(self._h)), "swf_problem_create")
        self._keep = {}          # address -> array (keeps caller arrays alive)

    def close(self):
        if self._h:
            lib().swf_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _p(self, arr):
        assert isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"]
        self._keep[arr.ctypes.data] = arr
        return arr.ctypes.data_as(_pd)

    @staticmethod
    def _d(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(_pd)

    # --- ceres::Problem members
    def AddParameterBlock(self, arr, size, pose_manifold=False):
        _chk(lib().swf_add_parameter_block(self._h, self._p(arr), C.c_int32(size), C.c_int32(1 if pose_manifold else 0)), "AddParameterBlock")

    def HasParameterBlock(self, arr):
        return bool(lib().swf_has_parameter_block(self._h, arr.ctypes.data_as(_pd)))

    def RemoveParameterBlock(self, arr):
        _chk(lib().swf_remove_parameter_block(self._h, arr.ctypes.data_as(_pd)), "RemoveParameterBlock")

    def SetParameterBlockConstant(self, arr):
        _chk(lib().swf_set_parameter_block_constant(self._h, arr.ctypes.data_as(_pd)), "SetParameterBlockConstant")

    def SetParameterBlockVariable(self, arr):
        _chk(lib().swf_set_parameter_block_variable(self._h, arr.ctypes.data_as(_pd)), "SetParameterBlockVariable")

    def IsParameterBlockConstant(self, arr):
        return bool(lib().swf_is_parameter_block_constant(self._h, arr.ctypes.data_as(_pd)))

    def ParameterBlockSize(self, arr):
        return lib().swf_parameter_block_size(self._h, arr.ctypes.data_as(_pd))

    def NumParameterBlocks(self):
        return lib().swf_num_parameter_blocks(self._h)

    def NumResidualBlocks(self):
        return lib().swf_num_residual_blocks(self._h)

    def RemoveResidualBlock(self, fid):
        _chk(lib().swf_remove_factor(self._h, C.c_int32(fid)), "RemoveResidualBlock")

    def SetResidualBlockUsed(self, fid, on):          # ResidualBlock::is_use of the modified Ceres
        _chk(lib().swf_factor_set_enabled(self._h, C.c_int32(fid), C.c_int32(1 if on else 0)), "is_use")

    def IsResidualBlockUsed(self, fid):
        rc = lib().swf_factor_is_enabled(self._h, C.c_int32(fid))
        if rc < 0:
            raise SwfError("is_use: unknown residual block %d" % fid)
        return bool(rc)

    # --- the query surface (GlobalMarge, R/swf/swf_image.cpp:350-367)
    def _ids(self, fn, what, *head):
        n = C.c_int32(0)
        _chk(fn(self._h, *head, None, C.c_int32(0), C.byref(n)), what)
        buf = (C.c_int32 * max(1, n.value))()
        _chk(fn(self._h, *head, buf, C.c_int32(n.value), C.byref(n)), what)
        return [int(buf[i]) for i in range(n.value)]

    def _blocks(self, fn, what, *head):
        n = C.c_int32(0)
        _chk(fn(self._h, *head, None, C.c_int32(0), C.byref(n)), what)
        buf = (_pd * max(1, n.value))()
        _chk(fn(self._h, *head, buf, C.c_int32(n.value), C.byref(n)), what)
        return [self._keep[C.cast(buf[i], C.c_void_p).value] for i in range(n.value)]

    def GetResidualBlocks(self):
        return self._ids(lib().swf_get_residual_blocks, "GetResidualBlocks")

    def GetResidualBlocksForParameterBlock(self, arr):
        return self._ids(lib().swf_get_residual_blocks_for_parameter_block, "GetResidualBlocksForParameterBlock", arr.ctypes.data_as(_pd))

    def GetParameterBlocks(self):
        return self._blocks(lib().swf_get_parameter_blocks, "GetParameterBlocks")

    def GetParameterBlocksForResidualBlock(self, fid):
        return self._blocks(lib().swf_get_parameter_blocks_for_residual_block, "GetParameterBlocksForResidualBlock", C.c_int32(fid))

    # --- typed AddResidualBlock()s
    def _fid(self, rc, what):
        if rc < 0:
            raise SwfError("%s failed (%d): %s" % (what, rc, lib().swf_last_error().decode()))
        return rc

    def AddProjection(self, pose, ex, point, uv, sqrt_info=1000.0 / 1.5, cauchy_a=1.0):
        a, pa = self._d(uv)
        return self._fid(lib().swf_add_projection(self._h, self._p(pose), self._p(ex), self._p(point), pa,
                                                  C.c_double(sqrt_info), C.c_double(cauchy_a)), "AddProjection")

    def AddImu(self, pose_i, sb_i, pose_j, sb_j, pre):
        a, pa = self._d(pre)
        return self._fid(lib().swf_add_imu(self._h, self._p(pose_i), self._p(sb_i), self._p(pose_j), self._p(sb_j), pa), "AddImu")

    def AddRtkCarrierPhase(self, pose, amb, clk, dat):
        a, pa = self._d(dat)
        return self._fid(lib().swf_add_rtk_carrier_phase(self._h, self._p(pose), self._p(amb), self._p(clk), pa), "AddRtkCarrierPhase")

    def AddRtkPseudorange(self, pose, clk, dat):
        a, pa = self._d(dat)
        return self._fid(lib().swf_add_rtk_pseudorange(self._h, self._p(pose), self._p(clk), pa), "AddRtkPseudorange")

    def AddDoppler(self, sb, drift, pose, dat):
        a, pa = self._d(dat)
        return self._fid(lib().swf_add_doppler(self._h, self._p(sb), self._p(drift), self._p(pose), pa), "AddDoppler")

    def AddSppPseudorange(self, pose, clk, dat):
        a, pa = self._d(dat)
        return self._fid(lib().swf_add_spp_pseudorange(self._h, self._p(pose), self._p(clk), pa), "AddSppPseudorange")

    def AddSppCarrierPhase(self, pose, clk, amb, dat):
        a, pa = self._d(dat)
        return self._fid(lib().swf_add_spp_carrier_phase(self._h, self._p(pose), self._p(clk), self._p(amb), pa), "AddSppCarrierPhase")

    def AddFixedInteger(self, n_a, n_b, N21, istd):
        return self._fid(lib().swf_add_fixed_integer(self._h, self._p(n_a), self._p(n_b), C.c_double(N21), C.c_double(istd)), "AddFixedInteger")

    def AddProjectionInverseDepth(self, kind, pose_i, pose_j, ex, ex2, inv_depth, pts_i, pts_j, sqrt_info, loss_a):
        pi = (C.c_double * 3)(*[float(v) for v in pts_i]); pj = (C.c_double * 3)(*[float(v) for v in pts_j])
        pp = lambda a: self._p(a) if a is not None else None
        return self._fid(lib().swf_add_projection_inverse_depth(self._h, C.c_int32(kind), pp(pose_i), pp(pose_j), pp(ex), pp(ex2), self._p(inv_depth), pi, pj,
                                                                 C.c_double(sqrt_info), C.c_double(loss_a)), "AddProjectionInverseDepth")

    def AddImuGnss(self, pose_i, sb_i, pose_j, sb_j, ambiguities, hidden_pose, hidden_sb, pose_lin, sb_lin, Hpp, HpN, rhs_p, HNN, rhsN, pre):
        """IMUGNSSFactor: hidden_pose [M][7] / hidden_sb [M][9] are caller-owned numpy arrays the solve updates in place."""
        N, M = len(ambiguities), int(np.asarray(hidden_pose).reshape(-1, 7).shape[0])
        assert hidden_pose.dtype == np.float64 and hidden_pose.flags["C_CONTIGUOUS"] and hidden_sb.dtype == np.float64 and hidden_sb.flags["C_CONTIGUOUS"]
        self._keep[hidden_pose.ctypes.data] = hidden_pose; self._keep[hidden_sb.ctypes.data] = hidden_sb
        keys = (_pd * max(1, N))(*[self._p(a) for a in ambiguities])
        arrs = [self._d(x) for x in (pose_lin, sb_lin, Hpp, HpN if N else np.zeros(1), rhs_p, HNN if N else np.zeros(1), rhsN if N else np.zeros(1), pre)]
        return self._fid(lib().swf_add_imu_gnss(self._h, self._p(pose_i), self._p(sb_i), self._p(pose_j), self._p(sb_j), keys, C.c_int32(N), C.c_int32(M),
                                                 hidden_pose.ctypes.data_as(_pd), hidden_sb.ctypes.data_as(_pd), *[a[1] for a in arrs]), "AddImuGnss")

    def SetImuGnssMidLink(self, fid, k, H12):
        """IMUGNSSBase::AddMidMargInfo's product: link k (1..M-1) of composite factor `fid` carries the cross block H12 (15x15); k = 0 clears."""
        a, pa = self._d(H12 if k else np.zeros(225))
        _chk(lib().swf_set_imu_gnss_mid_link(self._h, C.c_int32(fid), C.c_int32(k), pa), "SetImuGnssMidLink")

    def AddScalarPrior(self, scalar, w):
        return self._fid(lib().swf_add_scalar_prior(self._h, self._p(scalar), C.c_double(w)), "AddScalarPrior")

    def AddLinearPrior(self, blocks, J, r0, x0):
        keys = (_pd * len(blocks))(*[self._p(b) for b in blocks])
        aJ, pJ = self._d(J); ar, pr = self._d(r0); ax, px = self._d(x0)
        return self._fid(lib().swf_add_linear_prior(self._h, keys, C.c_int32(len(blocks)), pJ, pr, px), "AddLinearPrior")

    # --- window constants, ordering, parameter_head
    def SetConstants(self, pbg, gw, base):
        a, pa = self._d(pbg); b, pb = self._d(gw); c, pc = self._d(base)
        _chk(lib().swf_set_constants(self._h, pa, pb, pc), "SetConstants")

    def SetOrdering(self, blocks, groups):
        """blocks = [] asks for the automatic ordering (a null linear_solver_ordering)."""
        keys = (_pd * max(1, len(blocks)))(*[b.ctypes.data_as(_pd) for b in blocks])
        g = np.ascontiguousarray(groups, dtype=np.int32)
        _chk(lib().swf_set_ordering(self._h, keys, g.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(len(blocks))), "SetOrdering")

    def SetParameterHead(self, blocks):
        keys = (_pd * max(len(blocks), 1))(*[b.ctypes.data_as(_pd) for b in blocks])
        _chk(lib().swf_set_export_tail(self._h, keys, C.c_int32(len(blocks))), "SetParameterHead")

    # --- ceres::Solve
    def Solve(self, opt=None):
        opt = opt if opt is not None else default_options()
        sm = SummaryC()
        _chk(lib().swf_problem_solve(self._h, C.byref(opt), C.byref(sm)), "Solve")
        return sm

    def Marginalize(self, eps=1e-8, form=0):
        """UpdateSchur + setmarginalizeinfo(Sqrt=true) over the parameter_head blocks, after Solve with
        step_mode = ASSEMBLE_ELIMINATE_ONLY (R/swf/swf_image.cpp:404-418).  Returns dict(J, r0, A, b, n, rank)."""
        J, r0, A, b, n, rk = _pd(), _pd(), _pd(), _pd(), C.c_int32(), C.c_int32()
        _chk(lib().swf_problem_marginalize(self._h, C.c_double(eps), C.c_int32(form), C.byref(J), C.byref(r0), C.byref(A), C.byref(b),
                                           C.byref(n), C.byref(rk)), "Marginalize")
        n = n.value
        return dict(J=np.ctypeslib.as_array(J, (n, n)).copy(), r0=np.ctypeslib.as_array(r0, (n,)).copy(),
                    A=np.ctypeslib.as_array(A, (n, n)).copy(), b=np.ctypeslib.as_array(b, (n,)).copy(), n=n, rank=rk.value)

    def TailCovariance(self):
        """UpdateSchurHessianOnly (R/swf/swf_gnss.cpp:65-94) + Qy = A^-1 (R/swf/swf_lambda.cpp:94-99) after Solve."""
        A, Q, n = _pd(), _pd(), C.c_int32()
        _chk(lib().swf_problem_tail_covariance(self._h, C.byref(A), C.byref(Q), C.byref(n)), "TailCovariance")
        n = n.value
        return dict(A=np.ctypeslib.as_array(A, (n, n)).copy(), Qy=np.ctypeslib.as_array(Q, (n, n)).copy(), n=n)

    def CheckFeatures(self, threshold=2.0):
        """SWFOptimization::OutliersRejection + the depth sign of Double2Vector after Solve (swf_problem_check_features).  Returns
        (get, rejected): get(block) -> dict(mean_err, depth, n_obs, flags) by parameter block, rejected = the addresses of the
        blocks FeatureManager::removeFailures would remove, in feature order."""
        _chk(lib().swf_problem_check_features(self._h, C.c_double(threshold)), "CheckFeatures")
        n = C.c_int32()
        _chk(lib().swf_problem_rejected_features(self._h, None, C.c_int32(0), C.byref(n)), "CheckFeatures")
        keys = (_pd * max(n.value, 1))()
        _chk(lib().swf_problem_rejected_features(self._h, keys, n, C.byref(n)), "CheckFeatures")
        rejected = [C.cast(keys[i], C.c_void_p).value for i in range(n.value)]

        def get(arr):
            m, d, no, fl = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
            _chk(lib().swf_problem_get_feature_check(self._h, arr.ctypes.data_as(_pd), C.byref(m), C.byref(d), C.byref(no), C.byref(fl)),
                 "swf_problem_get_feature_check")
            return dict(mean_err=m.value, depth=d.value, n_obs=no.value, flags=fl.value)
        return get, rejected

    def FixPrior(self, fid, amb, ref, N21, scalars_at_zero=True, istd=1.0 / 0.03, eps=1e-8, form=0):
        """Fix and hold for this problem (swf_problem_fix_prior): fold *amb[i] - *ref[i] = N21[i] into linear prior `fid`, evaluated at
        the blocks' current values.  Returns dict(J, r0, x0, n, rank); then RemoveResidualBlock(fid) + AddLinearPrior(...) as the
        reference does (R/swf/swf_lambda.cpp:344-354)."""
        n = len(amb)
        ka = (_pd * max(n, 1))(*[self._p(a) for a in amb]); kr = (_pd * max(n, 1))(*[self._p(a) for a in ref])
        v = np.ascontiguousarray(N21, np.float64)
        J, r0, x0, dim, rk = _pd(), _pd(), _pd(), C.c_int32(), C.c_int32()
        _chk(lib().swf_problem_fix_prior(self._h, C.c_int32(fid), ka, kr, v.ctypes.data_as(_pd), C.c_int32(n), C.c_int32(1 if scalars_at_zero else 0),
                                         C.c_double(istd), C.c_double(eps), C.c_int32(form), C.byref(J), C.byref(r0), C.byref(x0), C.byref(dim),
                                         C.byref(rk)), "FixPrior")
        d = dim.value
        gs = sum(self.ParameterBlockSize(k) for k in self.GetParameterBlocksForResidualBlock(fid))
        return dict(J=np.ctypeslib.as_array(J, (d, d)).copy(), r0=np.ctypeslib.as_array(r0, (d,)).copy(),
                    x0=np.ctypeslib.as_array(x0, (gs,)).copy(), n=d, rank=rk.value)

    def GetReduced(self):
        S, r, L, n = _pd(), _pd(), _pd(), C.c_int32()
        _chk(lib().swf_get_reduced(self._h, C.byref(S), C.byref(r), C.byref(L), C.byref(n)), "GetReduced")
        n = n.value
        return (np.ctypeslib.as_array(S, (n, n)).copy(), np.ctypeslib.as_array(r, (n,)).copy(),
                np.ctypeslib.as_array(L, (n, n)).copy())


class CompositeBatch:
    """n composite IMU-GNSS factors (IMUGNSSBase, R/factor/gnss_imu_factor.cpp) evaluated together on the device.
    `factors`: list of dicts with pose [M][7], sb [M][9], pose_lin, sb_lin, Hpp [M][15][15], HpN [M][15][N], rhs_p [M][15],
    HNN [N][N], rhsN [N], pre [M+1][PRE_DOUBLES]; pbg, gw shared."""

    def __init__(self, factors, pbg, gw):
        cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(f[k], np.float64).ravel() for f in factors]) if factors else np.zeros(0))
        self.M = np.array([np.asarray(f["pose"]).reshape(-1, 7).shape[0] for f in factors], np.int32)
        self.N = np.array([np.asarray(f["rhsN"]).size for f in factors], np.int32)
        self.n = len(factors)
        arrs = [cat(k) for k in ("pose", "sb", "pose_lin", "sb_lin", "Hpp", "HpN", "rhs_p", "HNN", "rhsN", "pre")]
        arrs = [a if a.size else np.zeros(1) for a in arrs]
        pb, g = np.ascontiguousarray(pbg, np.float64), np.ascontiguousarray(gw, np.float64)
        self._h = C.c_void_p()
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_composite_create(C.c_int32(self.n), self.M.ctypes.data_as(pi), self.N.ctypes.data_as(pi),
                                        *[a.ctypes.data_as(_pd) for a in arrs], pb.ctypes.data_as(_pd), g.ctypes.data_as(_pd), None,
                                        C.byref(self._h)), "swf_composite_create")
        self.G = 30 + self.N
        self.g_off = np.concatenate([[0], np.cumsum(self.G)]); self.g2_off = np.concatenate([[0], np.cumsum(self.G.astype(np.int64) ** 2)])

    def evaluate(self, outer, Nv, want_jac):
        """outer [n][32] (pose_i sb_i pose_j sb_j), Nv: list of per-factor ambiguity vectors.  Returns per-factor lists
        (residual, J, H, rhs, status) — J is None for a cost-only call."""
        o = np.ascontiguousarray(np.asarray(outer, np.float64).reshape(self.n, 32))
        nv = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).ravel() for v in Nv]) if int(self.N.sum()) else np.zeros(1))
        res = np.zeros(int(self.g_off[-1])); jac = np.zeros(int(self.g2_off[-1])); Hd = np.zeros_like(jac); rd = np.zeros_like(res)
        st = np.zeros(self.n, np.int32)
        _chk(lib().swf_composite_evaluate(self._h, o.ctypes.data_as(_pd), nv.ctypes.data_as(_pd), C.c_int32(1 if want_jac else 0),
                                          res.ctypes.data_as(_pd), jac.ctypes.data_as(_pd), Hd.ctypes.data_as(_pd), rd.ctypes.data_as(_pd),
                                          st.ctypes.data_as(C.POINTER(C.c_int32))), "swf_composite_evaluate")
        out = []
        for f in range(self.n):
            G = int(self.G[f]); a, b = int(self.g_off[f]), int(self.g2_off[f])
            out.append(dict(r=res[a:a + G].copy(), J=jac[b:b + G * G].reshape(G, G).copy() if want_jac else None,
                            H=Hd[b:b + G * G].reshape(G, G).copy(), rhs=rd[a:a + G].copy(), status=int(st[f])))
        return out

    ROOT_PIVOTED_CHOLESKY, ROOT_EIGEN = 0, 1

    def set_root(self, form):
        """ROOT_EIGEN: the reference's eigen square root (rows in ascending eigenvalue order); default: pivoted Cholesky rows."""
        _chk(lib().swf_composite_set_root(self._h, C.c_int32(form)), "swf_composite_set_root")

    def set_mid_links(self, mid, H12):
        """IMUGNSSBase::AddMidMargInfo's product per factor: mid[f] = link 1..M-1 carrying the cross block H12[f] (15x15), 0 = none."""
        m = np.ascontiguousarray(mid, np.int32); h = np.ascontiguousarray(np.asarray(H12, np.float64).reshape(self.n, 225))
        _chk(lib().swf_composite_set_mid_links(self._h, m.ctypes.data_as(C.POINTER(C.c_int32)), h.ctypes.data_as(_pd)), "swf_composite_set_mid_links")

    def hidden(self):
        m = int(self.M.sum())
        pose, sb = np.zeros((m, 7)), np.zeros((m, 9))
        _chk(lib().swf_composite_hidden(self._h, pose.ctypes.data_as(_pd), sb.ctypes.data_as(_pd)), "swf_composite_hidden")
        e = np.concatenate([[0], np.cumsum(self.M)])
        return [(pose[e[f]:e[f + 1]], sb[e[f]:e[f + 1]]) for f in range(self.n)]

    def close(self):
        if self._h:
            lib().swf_composite_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def marginal_priors(windows, eps=1e-8, form=0, timing=None, allow_failed=False):
    """swf_batch_marginal_priors: the linear prior over each window's parameter_head tail with everything else eliminated
    (GnssPreprocess's per-epoch marginalize, R/swf/swf_gnss.cpp:504-532), for all windows in one batch on the device.
    Returns a list of dict(n, rank, A, b, J, r0).  A window whose marginal could not be formed comes back with rank -1 and zeros:
    that raises here unless allow_failed (such a prior must not be filed into a composite factor)."""
    structs = [w.c_struct() for w in windows]
    arr = (C.POINTER(FlatWindowC) * len(structs))(*[C.pointer(s) for s in structs])
    n = len(structs)
    dims = np.zeros(n, np.int32)
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_batch_marginal_priors(arr, C.c_int32(n), C.c_double(eps), C.c_int32(form), dims.ctypes.data_as(pi), None, None, None, None, None, None),
         "swf_batch_marginal_priors")
    n2, n1 = int((dims.astype(np.int64) ** 2).sum()), int(dims.sum())
    A, J, b, r0, ranks = np.zeros(max(n2, 1)), np.zeros(max(n2, 1)), np.zeros(max(n1, 1)), np.zeros(max(n1, 1)), np.zeros(n, np.int32)
    import time as _time
    t0 = _time.perf_counter()
    _chk(lib().swf_batch_marginal_priors(arr, C.c_int32(n), C.c_double(eps), C.c_int32(form), dims.ctypes.data_as(pi), ranks.ctypes.data_as(pi),
                                         A.ctypes.data_as(_pd), b.ctypes.data_as(_pd), J.ctypes.data_as(_pd), r0.ctypes.data_as(_pd), None), "swf_batch_marginal_priors")
    if timing is not None:
        timing["c_abi_call_s"] = _time.perf_counter() - t0          # the C-ABI call alone (structure upload, solve, consumer, download), without this wrapper's marshalling
    if not allow_failed and (ranks < 0).any():
        raise SwfError("swf_batch_marginal_priors: no marginal for window(s) %s (rank -1: failed elimination)" % np.nonzero(ranks < 0)[0].tolist())
    out, o2, o1 = [], 0, 0
    for i in range(n):
        d = int(dims[i])
        out.append(dict(n=d, rank=int(ranks[i]), A=A[o2:o2 + d * d].reshape(d, d).copy(), b=b[o1:o1 + d].copy(),
                        J=J[o2:o2 + d * d].reshape(d, d).copy(), r0=r0[o1:o1 + d].copy()))
        o2 += d * d; o1 += d
    return out


def composite_assemble(epochs):
    """swf_composite_assemble: IMUGNSSBase::AddMargInfo (R/factor/gnss_imu_factor.cpp:245-352) for a chain of epochs.
    epochs: list of dict(kept = [(size, key)] in prior order — key = the numpy array of a scalar block, anything for poses /
    speed-biases —, A, b).  Returns dict(N, keys (the scalar blocks in first-seen order), Hpp [M][15][15], HpN [M][15][N],
    rhs_p [M][15], HNN [N][N], rhsN [N])."""
    M = len(epochs)
    n_kept = np.array([len(e["kept"]) for e in epochs], np.int32)
    sizes = np.array([s for e in epochs for (s, _) in e["kept"]], np.int32)
    keep_alive, ptrs = {}, []
    for e in epochs:
        for (s, k) in e["kept"]:
            if s == 1:
                assert isinstance(k, np.ndarray) and k.dtype == np.float64
                keep_alive[k.ctypes.data] = k; ptrs.append(k.ctypes.data_as(_pd))
            else:
                ptrs.append(_pd())
    keys = (_pd * max(1, len(ptrs)))(*ptrs)
    A = np.ascontiguousarray(np.concatenate([np.asarray(e["A"], np.float64).ravel() for e in epochs]))
    b = np.ascontiguousarray(np.concatenate([np.asarray(e["b"], np.float64).ravel() for e in epochs]))
    pi = C.POINTER(C.c_int32)
    N = C.c_int32(0)
    _chk(lib().swf_composite_assemble(C.c_int32(M), n_kept.ctypes.data_as(pi), sizes.ctypes.data_as(pi), keys, A.ctypes.data_as(_pd), b.ctypes.data_as(_pd),
                                      C.c_int32(0), None, C.byref(N), None, None, None, None, None), "swf_composite_assemble")
    n = N.value
    Hpp, HpN, rhs_p, HNN, rhsN = np.zeros((M, 15, 15)), np.zeros((M, 15, max(n, 1))), np.zeros((M, 15)), np.zeros((max(n, 1), max(n, 1))), np.zeros(max(n, 1))
    HpN_buf = np.zeros(M * 15 * max(n, 1))
    nk = (_pd * max(1, n))()
    _chk(lib().swf_composite_assemble(C.c_int32(M), n_kept.ctypes.data_as(pi), sizes.ctypes.data_as(pi), keys, A.ctypes.data_as(_pd), b.ctypes.data_as(_pd),
                                      C.c_int32(n), nk, C.byref(N), Hpp.ctypes.data_as(_pd), HpN_buf.ctypes.data_as(_pd), rhs_p.ctypes.data_as(_pd),
                                      HNN.ctypes.data_as(_pd), rhsN.ctypes.data_as(_pd)), "swf_composite_assemble")
    HpN = HpN_buf[:M * 15 * n].reshape(M, 15, n) if n else np.zeros((M, 15, 0))
    return dict(N=n, keys=[keep_alive[C.cast(nk[i], C.c_void_p).value] for i in range(n)], Hpp=Hpp, HpN=HpN, rhs_p=rhs_p,
                HNN=HNN[:n, :n].copy(), rhsN=rhsN[:n].copy())


def prior_reset_linearization_point(blocks, sizes, J, A, r0, b, x0):
    """swf_prior_reset_linearization_point: MarginalizationInfo::ResetLinearizationPoint (R/factor/marginalization_factor.cpp:232-258).
    blocks = the kept blocks' current values (numpy arrays, kept order), sizes = their global sizes; J / A dim x dim or None.
    Returns the shifted (r0, b, x0) as new arrays (None where the pair was not given)."""
    sizes = np.ascontiguousarray(sizes, np.int32)
    arrs = [np.ascontiguousarray(np.asarray(x, np.float64).ravel()) for x in blocks]
    ptrs = (_pd * max(1, len(arrs)))(*[a.ctypes.data_as(_pd) for a in arrs])
    dim = int(sum(6 if sz == 7 else sz for sz in sizes))
    Jc = None if J is None else np.ascontiguousarray(J, np.float64); Ac = None if A is None else np.ascontiguousarray(A, np.float64)
    r = None if r0 is None else np.array(r0, np.float64); bb = None if b is None else np.array(b, np.float64)
    x = np.array(x0, np.float64)
    pn = lambda a: a.ctypes.data_as(_pd) if a is not None else None
    _chk(lib().swf_prior_reset_linearization_point(C.c_int32(len(arrs)), sizes.ctypes.data_as(C.POINTER(C.c_int32)), ptrs, C.c_int32(dim),
                                                   pn(Jc), pn(Ac), pn(r), pn(bb), pn(x)), "swf_prior_reset_linearization_point")
    return r, bb, x


def composite_add_mid_prior(fac, k, kept, A, b):
    """swf_composite_add_mid_prior: IMUGNSSBase::AddMidMargInfo (R/factor/gnss_imu_factor.cpp:121-240).  `fac` = what composite_assemble
    returned (N, keys, Hpp, HpN, rhs_p, HNN, rhsN); kept = [(size, epoch or key)] of the marginalised stretch's prior (A, b): poses (7) and
    speed-biases (9) carry the epoch index k-1 or k, scalars (1) their numpy block.  Returns the updated dict plus mid = k and H12."""
    M = fac["Hpp"].shape[0]; N0 = int(fac["N"])
    n_new = sum(1 for (sz, _) in kept if sz == 1)
    cap = N0 + n_new
    sizes = np.array([sz for (sz, _) in kept], np.int32)
    epochs = np.array([int(e) if sz != 1 else -1 for (sz, e) in kept], np.int32)
    keep_alive = {kk.ctypes.data: kk for kk in fac["keys"]}
    ptrs = []
    for (sz, kk) in kept:
        if sz == 1:
            assert isinstance(kk, np.ndarray) and kk.dtype == np.float64
            keep_alive[kk.ctypes.data] = kk; ptrs.append(kk.ctypes.data_as(_pd))
        else:
            ptrs.append(_pd())
    keys = (_pd * max(1, len(ptrs)))(*ptrs)
    nk = (_pd * max(1, cap))(*[kk.ctypes.data_as(_pd) for kk in fac["keys"]])
    Hpp = np.ascontiguousarray(fac["Hpp"], np.float64).copy(); rhs_p = np.ascontiguousarray(fac["rhs_p"], np.float64).copy()
    HpN = np.zeros((M, 15, max(cap, 1))); HpN[:, :, :N0] = fac["HpN"]
    HNN = np.zeros((max(cap, 1), max(cap, 1))); HNN[:N0, :N0] = fac["HNN"]
    rhsN = np.zeros(max(cap, 1)); rhsN[:N0] = fac["rhsN"]
    H12 = np.zeros((15, 15))
    A_ = np.ascontiguousarray(A, np.float64); b_ = np.ascontiguousarray(b, np.float64)
    N = C.c_int32(N0)
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_composite_add_mid_prior(C.c_int32(M), C.c_int32(k), C.c_int32(len(kept)), sizes.ctypes.data_as(pi), epochs.ctypes.data_as(pi), keys,
                                           A_.ctypes.data_as(_pd), b_.ctypes.data_as(_pd), C.c_int32(cap), nk, C.byref(N), Hpp.ctypes.data_as(_pd),
                                           HpN.ctypes.data_as(_pd), rhs_p.ctypes.data_as(_pd), HNN.ctypes.data_as(_pd), rhsN.ctypes.data_as(_pd),
                                           H12.ctypes.data_as(_pd)), "swf_composite_add_mid_prior")
    n = N.value
    return dict(N=n, keys=[keep_alive[C.cast(nk[i], C.c_void_p).value] for i in range(n)], Hpp=Hpp, HpN=HpN[:, :, :n].copy(), rhs_p=rhs_p,
                HNN=HNN[:n, :n].copy(), rhsN=rhsN[:n].copy(), mid=k, H12=H12)


def eval_inverse_depth_batch(kind, idx, poses, lam, pts, sqrt_info, pbg):
    """Inverse-depth projection factors (R/factor/projection_factor.cpp:77-329) for a batch on the device.
    kind [n] (0 TwoFrameOneCam, 1 TwoFrameTwoCam, 2 OneFrameTwoCam), idx [n][5] = pose_i, pose_j, ex, ex2, lambda rows,
    poses [P][7], lam [L], pts [n][6].  Returns r [n][2], J [n][50] (pose_i | pose_j | ex | ex2 | lambda)."""
    k = np.ascontiguousarray(kind, np.int32); ix = np.ascontiguousarray(idx, np.int32).reshape(-1, 5)
    ps = np.ascontiguousarray(poses, np.float64).reshape(-1, 7); lm = np.ascontiguousarray(lam, np.float64).ravel()
    pt = np.ascontiguousarray(pts, np.float64).reshape(-1, 6); pb = np.ascontiguousarray(pbg, np.float64)
    n = k.size
    r, J = np.zeros((n, 2)), np.zeros((n, 50))
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_eval_inverse_depth_batch(k.ctypes.data_as(pi), ix.ctypes.data_as(pi), C.c_int32(n), ps.ctypes.data_as(_pd), C.c_int32(ps.shape[0]),
                                            lm.ctypes.data_as(_pd), C.c_int32(lm.size), pt.ctypes.data_as(_pd), C.c_double(sqrt_info), pb.ctypes.data_as(_pd),
                                            r.ctypes.data_as(_pd), J.ctypes.data_as(_pd), C.c_int32(0), None), "eval_inverse_depth_batch")
    return r, J


def preintegrate_batch(samples, biases, noise):
    """IntegrationBase for a batch of keyframe intervals on the device (R/factor/integration_base.cpp:5-142).
    samples: list of [n_i][7] arrays (dt, acc, gyr; the first row seeds acc_0 / gyr_0); biases [n][6] (ba, bg);
    noise = (ACC_N, GYR_N, ACC_W, GYR_W).  Returns the [n][PRE_DOUBLES] records AddImu / imu_pre take."""
    n = len(samples)
    first = np.zeros(n + 1, np.int32)
    for i, s_ in enumerate(samples):
        first[i + 1] = first[i] + np.asarray(s_).reshape(-1, 7).shape[0]
    flat = (np.ascontiguousarray(np.concatenate([np.asarray(s_, np.float64).reshape(-1, 7) for s_ in samples]))
            if n and first[n] else np.zeros((1, 7)))
    b = np.ascontiguousarray(np.asarray(biases, np.float64).reshape(n, 6))
    nz = (C.c_double * 4)(*[float(v) for v in noise])
    out = np.zeros((n, 293))
    _chk(lib().swf_preintegrate_batch(flat.ctypes.data_as(_pd), first.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(n),
                                      b.ctypes.data_as(_pd), nz, out.ctypes.data_as(_pd), C.c_int32(0), None), "preintegrate_batch")
    return out


def preintegrate_runs_batch(samples, runs, biases, noise):
    """swf_preintegrate_batch over a gather list (swf_preintegrate_runs_batch): samples [N][7] is one resident array, runs a list, per
    interval, of (offset, count) pairs into it.  The first row of an interval's first non-empty run seeds acc_0 / gyr_0, every
    further row is a push_back.  Returns the [n][PRE_DOUBLES] records, bit-identical to preintegrate_batch on the concatenated rows."""
    n = len(runs)
    s = np.ascontiguousarray(np.asarray(samples, np.float64).reshape(-1, 7))
    run_first = np.zeros(n + 1, np.int32)
    for i, r in enumerate(runs):
        run_first[i + 1] = run_first[i] + np.asarray(r, np.int64).reshape(-1, 2).shape[0]
    rr = [np.asarray(r, np.int32).reshape(-1, 2) for r in runs]
    flat = np.ascontiguousarray(np.concatenate(rr)) if n and run_first[n] else np.zeros((1, 2), np.int32)
    b = np.ascontiguousarray(np.asarray(biases, np.float64).reshape(n, 6))
    nz = (C.c_double * 4)(*[float(v) for v in noise])
    out = np.zeros((n, 293))
    pi = C.POINTER(C.c_int32)
    sp = s if s.size else np.zeros((1, 7))
    _chk(lib().swf_preintegrate_runs_batch(sp.ctypes.data_as(_pd), C.c_int32(s.shape[0]), flat.ctypes.data_as(pi), run_first.ctypes.data_as(pi),
                                           C.c_int32(n), b.ctypes.data_as(_pd), nz, out.ctypes.data_as(_pd), C.c_int32(0), None),
         "preintegrate_runs_batch")
    return out


IMUF_OK, IMUF_EMPTY, IMUF_NO_INNER, IMUF_TIME_ORDER = 0, 1, 2, 3


def imu_frame_batch(raw, t01, seed, state, gyrj_prev, flags, pbg, g_w, noise, fill=0.0):
    """SWFOptimization::ImuIntegrate + IMUProcess (R/swf/swf_imu.cpp:117-213) for a batch of frames on the device
    (swf_imu_frame_batch).  raw: list of [n_f][7] arrays (t, acc, gyr: what GetImuInterval returns); t01 [n][2]; seed [n][6] (acc_0,
    gyr_0 on entry); state [n][21] (P, R row-major, V, ba, bg); gyrj_prev [n][3]; flags [n] (bit 0: velocity lever arm); pbg, g_w [3];
    noise = (ACC_N, GYR_N, ACC_W, GYR_W).  Returns dict(cut, first, pre, pred, info): cut [sum n_f + n][7] in preintegrate_batch's
    layout, frame f owning rows first[f] + f .. first[f + 1] + f; a frame whose info is not IMUF_OK leaves its rows at `fill`."""
    n = len(raw)
    rr = [np.asarray(r, np.float64).reshape(-1, 7) for r in raw]
    first = np.zeros(n + 1, np.int32)
    for i, r in enumerate(rr):
        first[i + 1] = first[i] + r.shape[0]
    flat = np.ascontiguousarray(np.concatenate(rr)) if n and first[n] else np.zeros((1, 7))
    a = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(n, k)) for v, k in ((t01, 2), (seed, 6), (state, 21), (gyrj_prev, 3))]
    fl = np.ascontiguousarray(np.asarray(flags, np.int32).reshape(n))
    v3 = lambda v: (C.c_double * 3)(*[float(x) for x in np.asarray(v, np.float64).reshape(3)])
    nz = (C.c_double * 4)(*[float(v) for v in noise])
    cut = np.full((int(first[n]) + n, 7), float(fill)); pre = np.full((n, 293), float(fill)); pred = np.full((n, 15), float(fill))
    info = np.full(n, -1, np.int32)
    pi = C.POINTER(C.c_int32)
    if n:
        _chk(lib().swf_imu_frame_batch(flat.ctypes.data_as(_pd), first.ctypes.data_as(pi), C.c_int32(n), a[0].ctypes.data_as(_pd),
                                       a[1].ctypes.data_as(_pd), a[2].ctypes.data_as(_pd), a[3].ctypes.data_as(_pd), fl.ctypes.data_as(pi),
                                       v3(pbg), v3(g_w), nz, cut.ctypes.data_as(_pd), pre.ctypes.data_as(_pd), pred.ctypes.data_as(_pd),
                                       info.ctypes.data_as(pi), C.c_int32(0), None), "imu_frame_batch")
    return dict(cut=cut, first=first, pre=pre, pred=pred, info=info)


PNP_OK, PNP_TOO_FEW, PNP_NO_MODEL, PNP_UNREFINED, PNP_BAD_INPUT = 0, 1, 2, 3, 4
PNP_NMAX, PNP_HMAX = 1024, 128


def pnp_frame_batch(pts_w, pts_uv, Ps_prev, Rs_prev, tic, ric, pbg, iterations=100, threshold=8.0 / 1000.0, confidence=0.99, seed=0,
                    flags=1, fill=0.0, stages=False):
    """FeatureManager::initFramePoseByPnP + solvePoseByPnP (R/feature/feature_manager.cpp:164-243) for a batch of frames on the device
    (swf_pnp_frame_batch).  pts_w: list of [n_f][3] world points; pts_uv: list of [n_f][2] normalised observations; Ps_prev [n][3],
    Rs_prev [n][9] (row-major) the previous frame's pose; tic, ric, pbg the extrinsic and the lever arm; flags bit 0: the points pass
    through float.  Returns dict(Ps, Rs, n_inliers, inlier, first, best, n_iters, info) and, with stages=True, samples [n][H][5],
    hyp [n][H][12], count [n][H]; inlier is [first[n]], frame f owning first[f] .. first[f + 1].  A frame whose info is PNP_TOO_FEW,
    PNP_BAD_INPUT or PNP_NO_MODEL leaves its outputs at `fill` (the integer outputs at int(fill), inlier at 255)."""
    n = len(pts_w)
    pw = [np.asarray(p, np.float64).reshape(-1, 3) for p in pts_w]
    uv = [np.asarray(p, np.float64).reshape(-1, 2) for p in pts_uv]
    first = np.zeros(n + 1, np.int32)
    for i in range(n):
        if pw[i].shape[0] != uv[i].shape[0]:
            raise SwfError("pnp_frame_batch: frame %d has %d world points and %d observations" % (i, pw[i].shape[0], uv[i].shape[0]))
        first[i + 1] = first[i] + pw[i].shape[0]
    tot = int(first[n])
    fw = np.ascontiguousarray(np.concatenate(pw + [np.zeros((1, 3))]))
    fu = np.ascontiguousarray(np.concatenate(uv + [np.zeros((1, 2))]))
    pp = np.ascontiguousarray(np.asarray(Ps_prev, np.float64).reshape(n, 3))
    rp = np.ascontiguousarray(np.asarray(Rs_prev, np.float64).reshape(n, 9))
    vec = lambda v, k: (C.c_double * k)(*[float(x) for x in np.asarray(v, np.float64).reshape(k)])
    H = int(iterations)
    out = dict(Ps=np.full((n, 3), float(fill)), Rs=np.full((n, 9), float(fill)), n_inliers=np.full(n, int(fill), np.int32),
               inlier=np.full(tot, 255, np.uint8), first=first, best=np.full(n, int(fill), np.int32), n_iters=np.full(n, int(fill), np.int32),
               info=np.full(n, -1, np.int32))
    pi = C.POINTER(C.c_int32)
    ex = [None, None, None]
    if stages:
        Hs = max(H, 0)
        out.update(samples=np.full((n, Hs, 5), int(fill), np.int32), hyp=np.full((n, Hs, 12), float(fill)), count=np.full((n, Hs), int(fill), np.int32))
        ex = [out["samples"].ctypes.data_as(pi), out["hyp"].ctypes.data_as(_pd), out["count"].ctypes.data_as(pi)]
    inl = out["inlier"] if tot else np.zeros(1, np.uint8)
    _chk(lib().swf_pnp_frame_batch(C.c_int32(n), first.ctypes.data_as(pi), fw.ctypes.data_as(_pd), fu.ctypes.data_as(_pd), pp.ctypes.data_as(_pd),
                                   rp.ctypes.data_as(_pd), vec(tic, 3), vec(ric, 9), vec(pbg, 3), C.c_int32(H), C.c_double(threshold),
                                   C.c_double(confidence), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_int32(flags),
                                   out["Ps"].ctypes.data_as(_pd), out["Rs"].ctypes.data_as(_pd), out["n_inliers"].ctypes.data_as(pi),
                                   inl.ctypes.data_as(C.POINTER(C.c_uint8)), out["best"].ctypes.data_as(pi), out["n_iters"].ctypes.data_as(pi),
                                   out["info"].ctypes.data_as(pi), ex[0], ex[1], ex[2], C.c_int32(0), None), "pnp_frame_batch")
    return out


TRK_OK, TRK_TOO_FEW, TRK_NO_MODEL, TRK_BAD_INPUT = 0, 1, 2, 3
TRK_NMAX, TRK_HMAX = 1024, 1024


def track_reject_batch(cur_px, prev_px, cam, dt, col=752, row=480, focal=1000.0, iterations=1000, threshold=1.0, confidence=0.99, seed=0,
                       flags=1, fill=0.0, stages=False):
    """FeatureTracker::rejectWithF with undistortedPts and ptsVelocity (R/feature/feature_tracker.cpp:265-294, :334-376) for a batch of
    frame pairs on the device (swf_track_reject_batch).  cur_px, prev_px: lists of [n_k][2] pixel positions of the same tracks in the
    current and the previous frame; cam [12] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6; dt [n] = cur_time - prev_time; flags bit 0: round
    through float wherever the reference holds a cv::Point2f.  Returns dict(status, keep_idx, first, n_inliers, best, n_iters, info, F,
    un_cur, un_prev, velocity) and, with stages=True, samples [n][H][8], hyp [n][H][9], count [n][H]; the per-point arrays are
    [first[n]], pair k owning first[k] .. first[k + 1].  A pair whose info is TRK_BAD_INPUT leaves its outputs at `fill` (the integer
    outputs at int(fill), status at 255); TRK_TOO_FEW and TRK_NO_MODEL write un_cur, un_prev and velocity only."""
    n = len(cur_px)
    cp = [np.asarray(p, np.float64).reshape(-1, 2) for p in cur_px]
    pp = [np.asarray(p, np.float64).reshape(-1, 2) for p in prev_px]
    if len(pp) != n:
        raise SwfError("track_reject_batch: %d current and %d previous frames" % (n, len(pp)))
    first = np.zeros(n + 1, np.int32)
    for i in range(n):
        if cp[i].shape[0] != pp[i].shape[0]:
            raise SwfError("track_reject_batch: pair %d has %d current and %d previous points" % (i, cp[i].shape[0], pp[i].shape[0]))
        first[i + 1] = first[i] + cp[i].shape[0]
    tot = int(first[n])
    fc = np.ascontiguousarray(np.concatenate(cp + [np.zeros((1, 2))]))
    fp = np.ascontiguousarray(np.concatenate(pp + [np.zeros((1, 2))]))
    dts = np.ascontiguousarray(np.asarray(dt, np.float64).reshape(n)) if n else np.zeros(1)
    cm = (C.c_double * 12)(*[float(x) for x in np.asarray(cam, np.float64).reshape(12)])
    H = int(iterations)
    pts = max(tot, 1)
    out = dict(status=np.full(pts, 255, np.uint8), keep_idx=np.full(pts, int(fill), np.int32), first=first,
               n_inliers=np.full(n, int(fill), np.int32), best=np.full(n, int(fill), np.int32), n_iters=np.full(n, int(fill), np.int32),
               info=np.full(n, -1, np.int32), F=np.full((n, 9), float(fill)), un_cur=np.full((pts, 2), float(fill)),
               un_prev=np.full((pts, 2), float(fill)), velocity=np.full((pts, 2), float(fill)))
    pi = C.POINTER(C.c_int32)
    ex = [None, None, None]
    if stages:
        Hs = max(H, 0)
        out.update(samples=np.full((n, Hs, 8), int(fill), np.int32), hyp=np.full((n, Hs, 9), float(fill)), count=np.full((n, Hs), int(fill), np.int32))
        ex = [out["samples"].ctypes.data_as(pi), out["hyp"].ctypes.data_as(_pd), out["count"].ctypes.data_as(pi)]
    _chk(lib().swf_track_reject_batch(C.c_int32(n), first.ctypes.data_as(pi), fc.ctypes.data_as(_pd), fp.ctypes.data_as(_pd), cm, C.c_int32(col),
                                      C.c_int32(row), C.c_double(focal), dts.ctypes.data_as(_pd), C.c_int32(H), C.c_double(threshold),
                                      C.c_double(confidence), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_int32(flags),
                                      out["status"].ctypes.data_as(C.POINTER(C.c_uint8)), out["keep_idx"].ctypes.data_as(pi),
                                      out["n_inliers"].ctypes.data_as(pi), out["best"].ctypes.data_as(pi), out["n_iters"].ctypes.data_as(pi),
                                      out["info"].ctypes.data_as(pi), out["F"].ctypes.data_as(_pd), out["un_cur"].ctypes.data_as(_pd),
                                      out["un_prev"].ctypes.data_as(_pd), out["velocity"].ctypes.data_as(_pd), ex[0], ex[1], ex[2],
                                      C.c_int32(0), None), "track_reject_batch")
    for key in ("status", "keep_idx", "un_cur", "un_prev", "velocity"):
        out[key] = out[key][:tot]
    return out


KLT_OK, KLT_BAD_INPUT = 0, 1
KLT_TRACKED, KLT_FWD_LOST, KLT_FWD_FLAT, KLT_BACK_LOST, KLT_BACK_FLAT, KLT_BACK_FAR, KLT_BORDER = 0, 1, 2, 3, 4, 5, 6
KLT_WMAX, KLT_LMAX, KLT_NMAX = 21, 4, 4096


def klt_pyramid_bytes(rows, cols, max_level):
    """swf_klt_pyramid_bytes: the pyramid workspace of one pair (both images, levels 1 .. max_level)"""
    fn = lib().swf_klt_pyramid_bytes
    fn.restype = C.c_size_t
    return int(fn(C.c_int32(rows), C.c_int32(cols), C.c_int32(max_level)))


def klt_track_batch(prev_img, cur_img, prev_px, guess_px=None, win=21, max_level=3, back_level=1, max_count=30, eps=0.01, min_eig=1e-4,
                    back_dist=0.5, flags=5, fill=0.0, stages=False):
    """The sparse optical flow of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:98-141) for a batch of image pairs on the
    device (swf_klt_track_batch): forward pyramidal Lucas-Kanade, the reverse pass, the forward-backward gate and inBorder.  prev_img,
    cur_img: [n][rows][cols] uint8; prev_px (and guess_px, with flag bit 1): lists of [n_k][2] pixel positions (x, y); flags bit 0:
    round through float where the reference holds a cv::Point2f, bit 1: guess_px is the initial flow, bit 2: the reverse pass and its
    gate.  Returns dict(cur_px, back_px, status, why, keep_idx, first, n_keep, info) and, with stages=True, trace_iters [..][2][5],
    trace_px [..][2][5][2] and pyr [n][klt_pyramid_bytes(rows, cols, max(max_level, back_level))]; the per-point arrays are
    [first[n]], pair k owning first[k] .. first[k + 1].  A pair whose info is KLT_BAD_INPUT leaves its outputs at `fill` (the integer
    outputs at int(fill), status at 255, pyr at 0)."""
    pimg = np.ascontiguousarray(prev_img, dtype=np.uint8)
    cimg = np.ascontiguousarray(cur_img, dtype=np.uint8)
    if pimg.ndim != 3 or pimg.shape != cimg.shape:
        raise SwfError("klt_track_batch: the images must be two [n][rows][cols] arrays of one shape")
    n, rows, cols = pimg.shape
    pp = [np.asarray(p, np.float64).reshape(-1, 2) for p in prev_px]
    if len(pp) != n:
        raise SwfError("klt_track_batch: %d image pairs and %d point sets" % (n, len(pp)))
    first = np.zeros(n + 1, np.int32)
    for i in range(n):
        first[i + 1] = first[i] + pp[i].shape[0]
    tot = int(first[n])
    fp = np.ascontiguousarray(np.concatenate(pp + [np.zeros((1, 2))]))
    fg = None
    if guess_px is not None:
        gp = [np.asarray(p, np.float64).reshape(-1, 2) for p in guess_px]
        if [g.shape for g in gp] != [p.shape for p in pp]:
            raise SwfError("klt_track_batch: guess_px does not match prev_px")
        fg = np.ascontiguousarray(np.concatenate(gp + [np.zeros((1, 2))]))
    pts = max(tot, 1)
    T = KLT_LMAX + 1
    out = dict(cur_px=np.full((pts, 2), float(fill)), back_px=np.full((pts, 2), float(fill)), status=np.full(pts, 255, np.uint8),
               why=np.full(pts, int(fill), np.int32), keep_idx=np.full(pts, int(fill), np.int32), first=first,
               n_keep=np.full(n, int(fill), np.int32), info=np.full(n, -1, np.int32))
    pi, pb = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    ex = [None, None, None]
    if stages:
        nb = klt_pyramid_bytes(rows, cols, max(min(max(max_level, back_level), KLT_LMAX), 0))
        out.update(trace_iters=np.full((pts, 2, T), int(fill), np.int32), trace_px=np.full((pts, 2, T, 2), float(fill)),
                   pyr=np.zeros((n, max(nb, 1)), np.uint8))
        ex = [out["trace_iters"].ctypes.data_as(pi), out["trace_px"].ctypes.data_as(_pd), out["pyr"].ctypes.data_as(pb)]
    _chk(lib().swf_klt_track_batch(C.c_int32(n), C.c_int32(rows), C.c_int32(cols), pimg.ctypes.data_as(pb), cimg.ctypes.data_as(pb),
                                   first.ctypes.data_as(pi), fp.ctypes.data_as(_pd), fg.ctypes.data_as(_pd) if fg is not None else None,
                                   C.c_int32(win), C.c_int32(max_level), C.c_int32(back_level), C.c_int32(max_count), C.c_double(eps),
                                   C.c_double(min_eig), C.c_double(back_dist), C.c_int32(flags), out["cur_px"].ctypes.data_as(_pd),
                                   out["back_px"].ctypes.data_as(_pd), out["status"].ctypes.data_as(pb), out["why"].ctypes.data_as(pi),
                                   out["keep_idx"].ctypes.data_as(pi), out["n_keep"].ctypes.data_as(pi), out["info"].ctypes.data_as(pi),
                                   ex[0], ex[1], ex[2], C.c_int32(0), None), "klt_track_batch")
    for key in ("cur_px", "back_px", "status", "why", "keep_idx") + (("trace_iters", "trace_px") if stages else ()):
        out[key] = out[key][:tot]
    if stages:
        out["pyr"] = out["pyr"][:, :nb]
    return out


GFTT_OK, GFTT_BAD_INPUT, GFTT_TOO_MANY = 0, 1, 2
GFTT_KEPT, GFTT_OUTSIDE, GFTT_CROWDED = 0, 1, 2
GFTT_NMAX = 1024


def gftt_workspace_bytes(rows, cols, cand_cap):
    """swf_gftt_workspace_bytes: the workspace of one frame (eig first); 0 outside the limits"""
    fn = lib().swf_gftt_workspace_bytes
    fn.restype = C.c_size_t
    return int(fn(C.c_int32(rows), C.c_int32(cols), C.c_int32(cand_cap)))


def gftt_detect_batch(img, px, track_cnt, mask=None, max_cnt=350, min_dist=30, quality=0.01, disc_halfwidth=None, cand_cap=1 << 15, flags=1,
                      fill=0.0, stages=False):
    """setMask, cv::goodFeaturesToTrack and addPoints of FeatureTracker::trackImage (R/feature/feature_tracker.cpp:148-165) for a batch
    of frames on the device (swf_gftt_detect_batch).  img (and mask, 0 = blocked): [n][rows][cols] uint8; px, track_cnt: lists of the
    frames' tracked points [n_k][2] (x, y) and their counts [n_k]; disc_halfwidth: [min_dist + 1] row half-widths of the blocked disc
    (None: the Euclidean disc); flags bit 0: px through float.  Returns dict(order, why, first, n_old, new_px [n][max_cnt][2], n_new,
    n_cand, max_eig, pack_first, pack_px, pack_src, info) and, with stages=True, eig [n][rows][cols]; order and why are [first[n]],
    frame k owning first[k] .. first[k + 1]; pack_px and pack_src are cut to pack_first[n].  What a frame does not write stays at
    `fill` (the integer outputs at int(fill))."""
    im = np.ascontiguousarray(img, dtype=np.uint8)
    if im.ndim != 3:
        raise SwfError("gftt_detect_batch: the images must be one [n][rows][cols] array")
    n, rows, cols = im.shape
    mk = None
    if mask is not None:
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        if mk.shape != im.shape:
            raise SwfError("gftt_detect_batch: the mask does not match the images")
    pp = [np.asarray(p, np.float64).reshape(-1, 2) for p in px]
    tc = [np.asarray(t, np.int32).reshape(-1) for t in track_cnt]
    if len(pp) != n or [p.shape[0] for p in pp] != [t.size for t in tc]:
        raise SwfError("gftt_detect_batch: %d frames, %d point sets and %d count sets, or sets of different lengths" % (n, len(pp), len(tc)))
    first = np.zeros(n + 1, np.int32)
    for i in range(n):
        first[i + 1] = first[i] + pp[i].shape[0]
    tot = int(first[n])
    fp = np.ascontiguousarray(np.concatenate(pp + [np.zeros((1, 2))]))
    ft = np.ascontiguousarray(np.concatenate(tc + [np.zeros(1, np.int32)]))
    hw = None if disc_halfwidth is None else np.ascontiguousarray(disc_halfwidth, dtype=np.int32)
    if hw is not None and hw.size != min_dist + 1:
        raise SwfError("gftt_detect_batch: disc_halfwidth needs min_dist + 1 entries")
    pts, mc, ifill = max(tot, 1), max(int(max_cnt), 1), int(fill)
    npack = tot + n * mc + 1
    out = dict(order=np.full(pts, ifill, np.int32), why=np.full(pts, ifill, np.int32), first=first, n_old=np.full(n, ifill, np.int32),
               new_px=np.full((n, mc, 2), float(fill)), n_new=np.full(n, ifill, np.int32), n_cand=np.full(n, ifill, np.int32),
               max_eig=np.full(n, float(fill)), pack_first=np.full(n + 1, ifill, np.int32), pack_px=np.full((npack, 2), float(fill)),
               pack_src=np.full(npack, ifill, np.int32), info=np.full(n, -1, np.int32))
    pi, pb = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    work = None
    if stages:
        wb = gftt_workspace_bytes(rows, cols, cand_cap)
        work = np.zeros((n, max(wb, rows * cols * 8)), np.uint8)
        work[:, :rows * cols * 8].view(np.float64)[...] = float(fill)
    _chk(lib().swf_gftt_detect_batch(C.c_int32(n), C.c_int32(rows), C.c_int32(cols), im.ctypes.data_as(pb), mk.ctypes.data_as(pb) if mk is not None else None,
                                     first.ctypes.data_as(pi), fp.ctypes.data_as(_pd), ft.ctypes.data_as(pi), C.c_int32(max_cnt), C.c_int32(min_dist),
                                     C.c_double(quality), hw.ctypes.data_as(pi) if hw is not None else None, C.c_int32(cand_cap), C.c_int32(flags),
                                     out["order"].ctypes.data_as(pi), out["why"].ctypes.data_as(pi), out["n_old"].ctypes.data_as(pi),
                                     out["new_px"].ctypes.data_as(_pd), out["n_new"].ctypes.data_as(pi), out["n_cand"].ctypes.data_as(pi),
                                     out["max_eig"].ctypes.data_as(_pd), out["pack_first"].ctypes.data_as(pi), out["pack_px"].ctypes.data_as(_pd),
                                     out["pack_src"].ctypes.data_as(pi), out["info"].ctypes.data_as(pi),
                                     work.ctypes.data_as(pb) if work is not None else None, C.c_int32(0), None), "gftt_detect_batch")
    for key in ("order", "why"):
        out[key] = out[key][:tot]
    used = int(out["pack_first"][n]) if out["pack_first"][n] >= 0 and (out["info"] != GFTT_BAD_INPUT).any() else 0
    out["pack_px"], out["pack_src"] = out["pack_px"][:used], out["pack_src"][:used]
    if stages:
        out["eig"] = work[:, :rows * cols * 8].view(np.float64).reshape(n, rows, cols)
    return out


TRACKER_NO_MODEL, TRACKER_TOO_MANY, TRACKER_STAGE_FAILED = 1, 2, 4
TRACKER_NCOUNT = 10
TRACKER_COUNTS = ("in", "klt", "f", "mask", "new", "cand", "final", "klt_info", "trk_info", "gftt_info")


class TrackerOptionsC(C.Structure):
    """swf_tracker_options of include/swf_solver.h"""
    _fields_ = [("max_cnt", C.c_int32), ("min_dist", C.c_int32), ("quality", C.c_double), ("cand_cap", C.c_int32),
                ("win", C.c_int32), ("max_level", C.c_int32), ("back_level", C.c_int32), ("max_count", C.c_int32),
                ("eps", C.c_double), ("min_eig", C.c_double), ("back_dist", C.c_double), ("flow_back", C.c_int32),
                ("f_iterations", C.c_int32), ("f_threshold", C.c_double), ("f_confidence", C.c_double), ("focal", C.c_double),
                ("virt_col", C.c_int32), ("virt_row", C.c_int32)]


def tracker_options(**options):
    """the reference's options (swf_tracker_default_options) with the given fields replaced"""
    o = TrackerOptionsC()
    lib().swf_tracker_default_options(C.byref(o))
    names = {f[0] for f in TrackerOptionsC._fields_}
    for k, v in options.items():
        if k not in names:
            raise SwfError("Tracker: unknown option %r" % k)
        setattr(o, k, v)
    return o


class Tracker:
    """FeatureTracker::trackImage and removeOutliers for n_streams image sequences whose state stays on the device (swf_tracker_*).
    cam [12] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6; the options are the fields of swf_tracker_options.  track() enqueues one frame
    of every stream and returns at once; frame() waits and returns the frame the last track() produced."""

    def __init__(self, n_streams, rows, cols, cam, stream=None, **options):
        self._h = C.c_void_p()
        self.n_streams, self.rows, self.cols = int(n_streams), int(rows), int(cols)
        self.opt = tracker_options(**options)
        cm = (C.c_double * 12)(*[float(x) for x in np.asarray(cam, np.float64).reshape(12)])
        _chk(lib().swf_tracker_create(C.c_int32(n_streams), C.c_int32(rows), C.c_int32(cols), cm, C.byref(self.opt),
                                      C.c_void_p(stream), C.byref(self._h)), "swf_tracker_create")

    def close(self):
        if self._h:
            lib().swf_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def track(self, times, imgs, mask=None, seed=0):
        """times [n_streams]; imgs (and mask, 0 = blocked) [n_streams][rows][cols] uint8 in host memory"""
        shape = (self.n_streams, self.rows, self.cols)
        t = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
        im = np.ascontiguousarray(imgs, dtype=np.uint8)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if t.size != self.n_streams or im.shape != shape or (mk is not None and mk.shape != shape):
            raise SwfError("Tracker.track: times, imgs and mask must be [%d], [%d][%d][%d]" % ((self.n_streams,) + shape))
        pb = C.POINTER(C.c_uint8)
        _chk(lib().swf_tracker_track(self._h, t.ctypes.data_as(_pd), im.ctypes.data_as(pb), mk.ctypes.data_as(pb) if mk is not None else None,
                                     C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_int32(0)), "swf_tracker_track")

    def track_device(self, times, d_imgs, d_mask=None, seed=0):
        """track() for images (and mask) that are device memory already: d_imgs, d_mask are device addresses"""
        t = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
        if t.size != self.n_streams:
            raise SwfError("Tracker.track_device: times must be [%d]" % self.n_streams)
        _chk(lib().swf_tracker_track(self._h, t.ctypes.data_as(_pd), C.c_void_p(d_imgs), C.c_void_p(d_mask) if d_mask else None,
                                     C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_int32(1)), "swf_tracker_track")

    def remove_ids(self, ids):
        """removeOutliers: ids is a list of one id array per stream"""
        per = [np.asarray(a, np.int32).reshape(-1) for a in ids]
        if len(per) != self.n_streams:
            raise SwfError("Tracker.remove_ids: %d id arrays for %d streams" % (len(per), self.n_streams))
        first = np.concatenate([[0], np.cumsum([a.size for a in per])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(per + [np.zeros(1, np.int32)]))
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_tracker_remove_ids(self._h, first.ctypes.data_as(pi), flat.ctypes.data_as(pi)), "swf_tracker_remove_ids")

    def sync(self):
        _chk(lib().swf_tracker_sync(self._h), "swf_tracker_sync")

    def frame(self):
        """dict(ids, track_cnt, obs, counts, info): per stream the ids [n], track_cnt [n], obs [n][7] = x y 1 u v vx vy, the
        counts [TRACKER_NCOUNT] (TRACKER_COUNTS names them) and the info bits of the last tracked frame"""
        ns, cap = self.n_streams, self.n_streams * self.opt.max_cnt
        n = np.zeros(ns, np.int32)
        ids, tc, obs = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 7))
        counts, info = np.zeros((ns, TRACKER_NCOUNT), np.int32), np.zeros(ns, np.int32)
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_tracker_download(self._h, n.ctypes.data_as(pi), ids.ctypes.data_as(pi), tc.ctypes.data_as(pi), obs.ctypes.data_as(_pd),
                                        counts.ctypes.data_as(pi), info.ctypes.data_as(pi)), "swf_tracker_download")
        first = np.concatenate([[0], np.cumsum(n)])
        cut = lambda a: [a[first[s]:first[s + 1]].copy() for s in range(ns)]
        return dict(ids=cut(ids), track_cnt=cut(tc), obs=cut(obs), counts=[counts[s].copy() for s in range(ns)], info=[int(v) for v in info])

    def device_frame(self):
        """the device addresses of the last frame's first, ids, track_cnt, px, obs (swf_tracker_device_frame)"""
        p = [C.c_void_p() for _ in range(5)]
        _chk(lib().swf_tracker_device_frame(self._h, *[C.byref(v) for v in p]), "swf_tracker_device_frame")
        return dict(zip(("first", "ids", "track_cnt", "px", "obs"), [v.value for v in p]))


FTABLE_WINDOW_FULL, FTABLE_TABLE_FULL, FTABLE_BAD_FRAME, FTABLE_STALE_LIST, FTABLE_BAD_SLIDE = 1, 2, 4, 8, 16
FTABLE_NCOUNT = 10
FTABLE_COUNTS = ("keyframe", "last_track", "long_track", "new", "erased", "info", "parallax_num", "n_listed", "n_proj", "n_pnp")
FTABLE_LISTING = ("lm_first", "proj_first", "lm_id", "lm_world", "lm_start", "lm_nobs", "lm_valid", "proj_frame", "proj_lm", "proj_uv", "proj_new")


class FtableOptionsC(C.Structure):
    """swf_ftable_options of include/swf_solver.h"""
    _fields_ = [("window", C.c_int32), ("feat_cap", C.c_int32), ("frame_cap", C.c_int32),
                ("feature_continue", C.c_int32), ("min_track", C.c_int32), ("min_long", C.c_int32), ("long_len", C.c_int32),
                ("new_ratio", C.c_double), ("min_parallax", C.c_double), ("focal", C.c_double), ("init_depth", C.c_double)]


class FtableListingC(C.Structure):
    """swf_ftable_listing of include/swf_solver.h: device addresses"""
    _fields_ = [(k, C.c_void_p) for k in FTABLE_LISTING]


def ftable_options(**options):
    """the reference's options (swf_ftable_default_options) with the given fields replaced"""
    o = FtableOptionsC()
    lib().swf_ftable_default_options(C.byref(o))
    names = {f[0] for f in FtableOptionsC._fields_}
    for k, v in options.items():
        if k not in names:
            raise SwfError("FeatureTable: unknown option %r" % k)
        setattr(o, k, v)
    return o


class FeatureTable:
    """FeatureManager for n_streams windows whose track table stays on the device (swf_ftable_*); the options are the
    fields of swf_ftable_options.  Every operation enqueues and returns at once; the methods that return arrays wait for them.
    Poses are Ps [n_streams][window][3], Rs [n_streams][window][3][3] by image frame; tic [3], ric [3][3], pbg [3]."""

    def __init__(self, n_streams, stream=None, **options):
        self._h = C.c_void_p()
        self.n_streams = int(n_streams)
        self.opt = ftable_options(**options)
        _chk(lib().swf_ftable_create(C.c_int32(n_streams), C.byref(self.opt), C.c_void_p(stream), C.byref(self._h)), "swf_ftable_create")

    def close(self):
        if self._h:
            lib().swf_ftable_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _f64(a, shape=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a if shape is None else a.reshape(shape)

    def _ext(self, tic, ric, pbg):
        t, r, p = self._f64(tic, 3), self._f64(ric, 9), self._f64(pbg, 3)
        return t, r, p, (t.ctypes.data_as(_pd), r.ctypes.data_as(_pd), p.ctypes.data_as(_pd))

    def _poses(self, Ps, Rs, per):
        return self._f64(Ps, (self.n_streams * per, 3)), self._f64(Rs, (self.n_streams * per, 9))

    def _pack(self, per, width, dtype, what):
        if len(per) != self.n_streams:
            raise SwfError("FeatureTable.%s: %d arrays for %d streams" % (what, len(per), self.n_streams))
        rows = [np.asarray(a, dtype).reshape((-1,) + width) for a in per]
        first = np.concatenate([[0], np.cumsum([a.shape[0] for a in rows])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(rows + [np.zeros((1,) + width, dtype)]))
        return first, flat

    def _fetch(self, addr, shape, dtype):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            _chk(lib().swf_ftable_fetch(self._h, C.c_void_p(out.ctypes.data), C.c_void_p(addr), C.c_uint64(out.nbytes)), "swf_ftable_fetch")
        return out

    def add_frame(self, ids, obs):
        """addFeatureCheckParallax + removeOut: one id array [n] and one obs array [n][7] per stream, host memory"""
        first, fi = self._pack(ids, (), np.int32, "add_frame")
        first_o, fo = self._pack(obs, (7,), np.float64, "add_frame")
        if not np.array_equal(first, first_o):
            raise SwfError("FeatureTable.add_frame: ids and obs disagree on the number of points")
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_ftable_add_frame(self._h, first.ctypes.data_as(pi), fi.ctypes.data_as(pi), fo.ctypes.data_as(_pd), C.c_int32(0)),
             "swf_ftable_add_frame")

    def add_frame_device(self, d_first, d_ids, d_obs):
        """add_frame for a frame that is device memory already: the first, ids, obs of Tracker.device_frame()"""
        _chk(lib().swf_ftable_add_frame(self._h, C.c_void_p(d_first), C.c_void_p(d_ids), C.c_void_p(d_obs), C.c_int32(1)), "swf_ftable_add_frame")

    def pnp_points_device(self):
        """the device addresses of swf_pnp_frame_batch's first, pts_w, pts_uv"""
        p = [C.c_void_p() for _ in range(3)]
        _chk(lib().swf_ftable_pnp_points(self._h, *[C.byref(v) for v in p]), "swf_ftable_pnp_points")
        return dict(zip(("first", "pts_w", "pts_uv"), [v.value for v in p]))

    def pnp_points(self):
        """per stream (pts_w [n][3], pts_uv [n][2]): the gather of initFramePoseByPnP"""
        d = self.pnp_points_device()
        first = self._fetch(d["first"], self.n_streams + 1, np.int32)
        w, uv = self._fetch(d["pts_w"], (int(first[-1]), 3), np.float64), self._fetch(d["pts_uv"], (int(first[-1]), 2), np.float64)
        return [(w[first[s]:first[s + 1]].copy(), uv[first[s]:first[s + 1]].copy()) for s in range(self.n_streams)]

    def triangulate(self, Ps, Rs, tic, ric, pbg):
        P, R = self._poses(Ps, Rs, self.opt.window)
        _, _, _, e = self._ext(tic, ric, pbg)
        _chk(lib().swf_ftable_triangulate(self._h, P.ctypes.data_as(_pd), R.ctypes.data_as(_pd), e[0], e[1], e[2], C.c_int32(0)), "swf_ftable_triangulate")

    def list_device(self):
        """the device addresses of the listing (FTABLE_LISTING names them)"""
        L = FtableListingC()
        _chk(lib().swf_ftable_list(self._h, C.byref(L)), "swf_ftable_list")
        return {k: getattr(L, k) for k in FTABLE_LISTING}

    def list(self):
        """AddFeature2Problem as data: per stream a dict of lm_id, lm_world [..][3], lm_start, lm_nobs, lm_valid and proj_frame,
        proj_lm, proj_uv [..][2], proj_new"""
        d = self.list_device()
        lf, pf = self._fetch(d["lm_first"], self.n_streams + 1, np.int32), self._fetch(d["proj_first"], self.n_streams + 1, np.int32)
        nl, npj = int(lf[-1]), int(pf[-1])
        a = dict(lm_id=self._fetch(d["lm_id"], nl, np.int32), lm_world=self._fetch(d["lm_world"], (nl, 3), np.float64),
                 lm_start=self._fetch(d["lm_start"], nl, np.int32), lm_nobs=self._fetch(d["lm_nobs"], nl, np.int32),
                 lm_valid=self._fetch(d["lm_valid"], nl, np.int32), proj_frame=self._fetch(d["proj_frame"], npj, np.int32),
                 proj_lm=self._fetch(d["proj_lm"], npj, np.int32), proj_uv=self._fetch(d["proj_uv"], (npj, 2), np.float64),
                 proj_new=self._fetch(d["proj_new"], npj, np.int32))
        return [{k: (v[lf[s]:lf[s + 1]] if k.startswith("lm_") else v[pf[s]:pf[s + 1]]).copy() for k, v in a.items()}
                for s in range(self.n_streams)]

    def set_solved(self, lm_world, flags, Ps, Rs, tic, ric, pbg):
        """the solved world points (one [n][3] array per stream, in the order of the last list()) and, unless None, the feature
        check's flags (one [n] uint8 array per stream)"""
        first, w = self._pack(lm_world, (3,), np.float64, "set_solved")
        fl = None
        if flags is not None:
            first_f, fl = self._pack(flags, (), np.uint8, "set_solved")
            if not np.array_equal(first, first_f):
                raise SwfError("FeatureTable.set_solved: lm_world and flags disagree on the number of landmarks")
        P, R = self._poses(Ps, Rs, self.opt.window)
        _, _, _, e = self._ext(tic, ric, pbg)
        _chk(lib().swf_ftable_set_solved(self._h, first.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(_pd),
                                         fl.ctypes.data_as(C.POINTER(C.c_uint8)) if fl is not None else None,
                                         P.ctypes.data_as(_pd), R.ctypes.data_as(_pd), e[0], e[1], e[2], C.c_int32(0)), "swf_ftable_set_solved")

    def remove_failures(self, fetch=True):
        """removeFailures; -> the erased ids per stream, the argument of Tracker.remove_ids (None without fetch)"""
        _chk(lib().swf_ftable_remove_failures(self._h, None, None), "swf_ftable_remove_failures")
        if not fetch:
            return None
        first, ids = np.zeros(self.n_streams + 1, np.int32), np.zeros(self.n_streams * self.opt.feat_cap, np.int32)
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_ftable_removed(self._h, first.ctypes.data_as(pi), ids.ctypes.data_as(pi)), "swf_ftable_removed")
        return [ids[first[s]:first[s + 1]].copy() for s in range(self.n_streams)]

    def check_parallax(self):
        _chk(lib().swf_ftable_check_parallax(self._h), "swf_ftable_check_parallax")

    def slide(self, mode, P1, R1, tic, ric, pbg):
        """mode [n_streams]: 0 nothing, 1 removeBack with the new oldest frame's P1 [n_streams][3], R1 [n_streams][3][3], 2 removeFront"""
        m = np.ascontiguousarray(np.asarray(mode, np.int32).reshape(self.n_streams))
        P, R = self._poses(P1, R1, 1)
        _, _, _, e = self._ext(tic, ric, pbg)
        _chk(lib().swf_ftable_slide(self._h, m.ctypes.data_as(C.POINTER(C.c_int32)), None, None, P.ctypes.data_as(_pd), R.ctypes.data_as(_pd),
                                    e[0], e[1], e[2], C.c_int32(0)), "swf_ftable_slide")

    def sync(self):
        _chk(lib().swf_ftable_sync(self._h), "swf_ftable_sync")

    def clear(self):
        _chk(lib().swf_ftable_clear(self._h), "swf_ftable_clear")

    def counts(self):
        """(counts [n_streams][FTABLE_NCOUNT] (FTABLE_COUNTS names them), parallax [n_streams])"""
        c, p = np.zeros((self.n_streams, FTABLE_NCOUNT), np.int32), np.zeros(self.n_streams)
        _chk(lib().swf_ftable_counts(self._h, c.ctypes.data_as(C.POINTER(C.c_int32)), p.ctypes.data_as(_pd)), "swf_ftable_counts")
        return c, p

    def state(self):
        """the whole table: per stream a dict of n_frames and, for its features in list order, id, start_frame, n_obs, valid,
        solve_flag, idepth, world [..][3], obs [..][window][7], in_problem [..][window]; the slots past n_obs are zeroed"""
        ns, F, W = self.n_streams, self.opt.feat_cap, self.opt.window
        nf, n = np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        i32 = {k: np.zeros((ns, F), np.int32) for k in ("id", "start_frame", "n_obs", "valid", "solve_flag")}
        idepth, world, obs, inp = np.zeros((ns, F)), np.zeros((ns, F, 3)), np.zeros((ns, F, W, 7)), np.zeros((ns, F, W), np.int32)
        pi = C.POINTER(C.c_int32)
        _chk(lib().swf_ftable_download(self._h, nf.ctypes.data_as(pi), n.ctypes.data_as(pi), i32["id"].ctypes.data_as(pi),
                                       i32["start_frame"].ctypes.data_as(pi), i32["n_obs"].ctypes.data_as(pi), i32["valid"].ctypes.data_as(pi),
                                       i32["solve_flag"].ctypes.data_as(pi), idepth.ctypes.data_as(_pd), world.ctypes.data_as(_pd),
                                       obs.ctypes.data_as(_pd), inp.ctypes.data_as(pi)), "swf_ftable_download")
        out = []
        for s in range(ns):
            m = int(n[s])
            d = {k: v[s, :m].copy() for k, v in i32.items()}
            dead = np.arange(W)[None, :] >= d["n_obs"][:, None]
            o, ip = obs[s, :m].copy(), inp[s, :m].copy()
            o[dead] = 0.0
            ip[dead] = 0
            d.update(n_frames=int(nf[s]), idepth=idepth[s, :m].copy(), world=world[s, :m].copy(), obs=o, in_problem=ip)
            out.append(d)
        return out


def triangulate_batch(Ps, Rs, tic, ric, pbg, start_frame, pt0, pt1, init_depth=5.0):
    """FeatureManager::triangulate (two-view branch, R/feature/feature_manager.cpp:285-316) for a batch of features on
    the device.  Ps [F][3], Rs [F][3][3]; start_frame [n]; pt0 / pt1 [n][2] normalised coordinates in frames i, i + 1.
    Returns (depth [n], pts_world [n][3])."""
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (Ps, Rs, tic, ric, pbg, pt0, pt1)]
    st = np.ascontiguousarray(start_frame, dtype=np.int32)
    n = st.size
    depth, world = np.zeros(n), np.zeros((n, 3))
    _chk(lib().swf_triangulate_batch(a[0].ctypes.data_as(_pd), a[1].ctypes.data_as(_pd), C.c_int32(a[0].size // 3),
                                     a[2].ctypes.data_as(_pd), a[3].ctypes.data_as(_pd), a[4].ctypes.data_as(_pd),
                                     st.ctypes.data_as(C.POINTER(C.c_int32)), a[5].ctypes.data_as(_pd), a[6].ctypes.data_as(_pd),
                                     C.c_int32(n), C.c_double(init_depth), depth.ctypes.data_as(_pd), world.ctypes.data_as(_pd),
                                     C.c_int32(0), None), "triangulate_batch")
    return depth, world


LAMBDA_OK, LAMBDA_NOT_PD, LAMBDA_LOOP_LIMIT, LAMBDA_NO_INPUT = 0, 1, 2, 3
LAMBDA_NMAX = 64
DDSEL_NMAX, DDSEL_TMAX = 256, 2048
DDSEL_OK, DDSEL_TOO_FEW, DDSEL_OVERFLOW, DDSEL_NONFINITE = 0, 1, 2, 3
DDSEL_SKIPPED, DDSEL_REFERENCE, DDSEL_PAIRED, DDSEL_GATED_OUT, DDSEL_NO_REFERENCE = 0, 1, 2, 3, 4
FEAT_OUTLIER, FEAT_NEG_DEPTH, FEAT_UNOBSERVED = 1, 2, 4


def lambda_batch(a_list, Q_list, m=2):
    """RTKLIB's lambda() (R/gnss/src/lambda.cpp:58-235) for a batch of problems on the device (swf_lambda_batch): float solutions
    a_list[p] [n_p] with covariances Q_list[p] [n_p][n_p], n_p <= 64.  Returns one (F [m][n_p], s [m], info) per problem."""
    P = len(a_list)
    ns = np.array([np.asarray(a).size for a in a_list], np.int32)
    ld = max(1, int(ns.max()) if P else 1)
    A = np.zeros((max(P, 1), ld))
    Q = np.zeros((max(P, 1), ld, ld))
    for p in range(P):
        k = ns[p]
        A[p, :k] = np.asarray(a_list[p], np.float64).ravel()
        Q[p, :k, :k] = np.asarray(Q_list[p], np.float64).T          # column-major
    F, s, info = np.zeros((max(P, 1), m, ld)), np.zeros((max(P, 1), m)), np.zeros(max(P, 1), np.int32)
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_lambda_batch(C.c_int32(P), C.c_int32(ld), ns.ctypes.data_as(pi), A.ctypes.data_as(_pd), Q.ctypes.data_as(_pd),
                                C.c_int32(m), F.ctypes.data_as(_pd), s.ctypes.data_as(_pd), info.ctypes.data_as(pi), C.c_int32(0), None),
         "swf_lambda_batch")
    return [(F[p, :, :ns[p]].copy(), s[p].copy(), int(info[p])) for p in range(P)]


def _dd_flatten(epochs_per_window):
    """epoch_first [W + 1], obs_first [E + 1], obs [n][2] of a list (windows) of lists (epochs, newest first) of (class, t)."""
    ef, of, obs = [0], [0], []
    for ep in epochs_per_window:
        for e in ep:
            obs.extend((int(c), int(t)) for c, t in e)
            of.append(len(obs))
        ef.append(len(of) - 1)
    o = np.array(obs, np.int32).reshape(-1, 2) if obs else np.zeros((1, 2), np.int32)
    return np.array(ef, np.int32), np.array(of, np.int32), np.ascontiguousarray(o)


def _dd_result(pairs, counts, refs, cost, role):
    n = int(counts[0])
    return dict(pairs=pairs[:n].copy(), raw_pairs=pairs.copy(), n_pairs=n, last_count=int(counts[1]), last_ref_count=int(counts[2]),
                info=int(counts[3]), refs=refs.copy(), cost=cost.copy(), role=role.copy())


def dd_select_batch(epochs_per_window, y_list, gate):
    """The double-difference pairs of the integer ambiguity search (FindReferenceSatellites and LambdaSearch's D3 loop,
    R/swf/swf_lambda.cpp:8-53, 118-188) for a batch of windows on the device (swf_dd_select_batch, which see).
    epochs_per_window[w] = the window's epochs NEWEST FIRST, each a list of (class = sys * 2 + f, tail coordinate) in the reference's
    observation order; y_list[w] = the float values of the window's tail; gate: one value or one per window.  Returns one dict per
    window as BatchSolver.ambiguity_pairs()."""
    W = len(epochs_per_window)
    if len(y_list) != W:
        raise ValueError("dd_select_batch: one y per window")
    ef, of, obs = _dd_flatten(epochs_per_window)
    ys = [np.asarray(v, np.float64).ravel() for v in y_list]
    yf = np.zeros(W + 1, np.int32)
    yf[1:] = np.cumsum([v.size for v in ys])
    y = np.ascontiguousarray(np.concatenate(ys + [np.zeros(1)]))
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(gate, np.float64), (W,))) if W else np.zeros(1)
    E, n = int(ef[-1]), int(of[-1])
    pairs, counts = np.full((max(W, 1), LAMBDA_NMAX, 2), -2, np.int32), np.full((max(W, 1), 4), -2, np.int32)
    refs, cost, role = np.full((max(E, 1), 6), -2, np.int32), np.full(max(n, 1), -2.0), np.full(max(n, 1), 255, np.uint8)
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_dd_select_batch(C.c_int32(W), ef.ctypes.data_as(pi), of.ctypes.data_as(pi), obs.ctypes.data_as(pi), yf.ctypes.data_as(pi),
                                   y.ctypes.data_as(_pd), g.ctypes.data_as(_pd), pairs.ctypes.data_as(pi), counts.ctypes.data_as(pi),
                                   refs.ctypes.data_as(pi), cost.ctypes.data_as(_pd), role.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   C.c_int32(0), None), "swf_dd_select_batch")
    return [_dd_result(pairs[w], counts[w], refs[ef[w]:ef[w + 1]], cost[of[ef[w]]:of[ef[w + 1]]], role[of[ef[w]]:of[ef[w + 1]]]) for w in range(W)]


FIX_PRIOR_MAXN = 140


def prior_fix_batch(J_list, r_list, rows_list, istd=1.0 / 0.03, eps=1e-8, form=0):
    """The stand-alone fix-and-hold operator (swf_prior_fix_batch) for a batch of linear priors: J_list[p] [n_p][n_p], r_list[p] [n_p]
    (the prior's residual at the new linearisation point), rows_list[p] = [(coordinate, group, value), ...].  Returns one
    dict(A, b, J, r0, eig, rank) per problem."""
    P = len(J_list)
    dims = np.array([np.asarray(r).size for r in r_list], np.int32)
    first = np.zeros(P + 1, np.int32)
    for p, rw in enumerate(rows_list):
        first[p + 1] = first[p] + len(rw)
    rows = np.ascontiguousarray(np.array([(c, g) for rw in rows_list for (c, g, _) in rw], np.int32).reshape(-1, 2)) if first[-1] else np.zeros((1, 2), np.int32)
    vals = np.ascontiguousarray(np.array([v for rw in rows_list for (_, _, v) in rw], np.float64)) if first[-1] else np.zeros(1)
    Jc = np.concatenate([np.asarray(J, np.float64).ravel() for J in J_list]) if P else np.zeros(1)
    rc = np.concatenate([np.asarray(r, np.float64).ravel() for r in r_list]) if P else np.zeros(1)
    t1, t2 = max(int(dims.sum()), 1), max(int((dims.astype(np.int64) ** 2).sum()), 1)
    if Jc.size != (dims.astype(np.int64) ** 2).sum():
        raise ValueError("prior_fix_batch: J must be dim x dim")
    A, Jn, b, r0, eig, rank = np.zeros(t2), np.zeros(t2), np.zeros(t1), np.zeros(t1), np.zeros(t1), np.zeros(max(P, 1), np.int32)
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_prior_fix_batch(C.c_int32(P), dims.ctypes.data_as(pi), Jc.ctypes.data_as(_pd), rc.ctypes.data_as(_pd), first.ctypes.data_as(pi),
                                   rows.ctypes.data_as(pi), vals.ctypes.data_as(_pd), C.c_double(istd), C.c_double(eps), C.c_int32(form),
                                   A.ctypes.data_as(_pd), b.ctypes.data_as(_pd), Jn.ctypes.data_as(_pd), r0.ctypes.data_as(_pd),
                                   eig.ctypes.data_as(_pd), rank.ctypes.data_as(pi), C.c_int32(0), None), "swf_prior_fix_batch")
    out, o1, o2 = [], 0, 0
    for p in range(P):
        n = int(dims[p])
        out.append(dict(A=A[o2:o2 + n * n].reshape(n, n).copy(), b=b[o1:o1 + n].copy(), J=Jn[o2:o2 + n * n].reshape(n, n).copy(),
                        r0=r0[o1:o1 + n].copy(), eig=eig[o1:o1 + n].copy(), rank=int(rank[p])))
        o1 += n; o2 += n * n
    return out


SCR_DOUBLES, SCR_GROUPS, SCR_NMAX = 9, 6, 256
SCR_RTK, SCR_SPP = 0, 1
SCR_HAS_AMB, SCR_CONTINUING = 1, 2
SCR_GATE_RTK, SCR_GATE_SPP, SCR_RESET_ALL = 1, 2, 4
SCR_MASKED, SCR_SLIP_RESIDUAL, SCR_SLIP_CODE, SCR_NEW_AMB = 1, 2, 4, 8
AZELMIN = 25.0 * np.pi / 180.0


def phase_screen_batch(first, pos, base, mode, dat, rec, el_min=AZELMIN):
    """The pre-fit carrier-phase screen of GnssPreprocess (R/swf/swf_gnss.cpp:337-499) for a batch of epochs on the device
    (swf_phase_screen_batch, which see): first [E + 1], pos / base [E][3], mode [E] (SCR_GATE_* | SCR_RESET_ALL), dat [n][9] =
    sat[3] L_lam lam el P N dt, rec [n][4] = kind, group, state bits, partner.  Returns dict(r [n], flags [n], med [E][2][6],
    cnt [E][2][6], reset [n] (an epoch's list starts at first[e], -1 behind it), n_reset [E])."""
    first = np.ascontiguousarray(first, np.int32).ravel()
    E = first.size - 1
    if E < 0:
        raise ValueError("phase_screen_batch: first needs n_epochs + 1 entries")
    pos, base = (np.ascontiguousarray(v, np.float64).reshape(-1) for v in (pos, base))
    mode = np.ascontiguousarray(mode, np.int32).ravel()
    dat = np.ascontiguousarray(dat, np.float64).reshape(-1)
    rec = np.ascontiguousarray(rec, np.int32).reshape(-1)
    n = dat.size // SCR_DOUBLES
    if pos.size != 3 * E or base.size != 3 * E or mode.size != E or dat.size != n * SCR_DOUBLES or rec.size != 4 * n or (E and int(first[-1]) > n):
        raise ValueError("phase_screen_batch: array sizes do not match first")
    pad = lambda a, k, t: a if a.size else np.zeros(k, t)              # (a valid pointer for an empty array)
    pos, base, mode, dat, rec = pad(pos, 3, np.float64), pad(base, 3, np.float64), pad(mode, 1, np.int32), pad(dat, SCR_DOUBLES, np.float64), pad(rec, 4, np.int32)
    out = dict(r=np.zeros(max(n, 1)), flags=np.zeros(max(n, 1), np.uint8), med=np.zeros((max(E, 1), 2, SCR_GROUPS)),
               cnt=np.zeros((max(E, 1), 2, SCR_GROUPS), np.int32), reset=np.full(max(n, 1), -1, np.int32), n_reset=np.zeros(max(E, 1), np.int32))
    pi = C.POINTER(C.c_int32)
    _chk(lib().swf_phase_screen_batch(C.c_int32(E), first.ctypes.data_as(pi), pos.ctypes.data_as(_pd), base.ctypes.data_as(_pd),
                                      mode.ctypes.data_as(pi), C.c_double(el_min), dat.ctypes.data_as(_pd), rec.ctypes.data_as(pi),
                                      out["r"].ctypes.data_as(_pd), out["flags"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                      out["med"].ctypes.data_as(_pd), out["cnt"].ctypes.data_as(pi), out["reset"].ctypes.data_as(pi),
                                      out["n_reset"].ctypes.data_as(pi), C.c_int32(0), None), "swf_phase_screen_batch")
    out["r"], out["flags"], out["reset"] = out["r"][:n], out["flags"][:n], out["reset"][:n]
    out["med"], out["cnt"], out["n_reset"] = out["med"][:E], out["cnt"][:E], out["n_reset"][:E]
    return out


GES_DOUBLES, GES_CLOCKS, GES_NMAX = 10, 13, 512
GES_RTK_PHASE, GES_RTK_CODE, GES_SPP_CODE, GES_SPP_PHASE, GES_DOPPLER = 0, 1, 2, 3, 4
GES_AMB_FREE = 1
GES_FREE_POS, GES_FREE_VEL = 1, 2
GES_CONVERGED, GES_MAX_ITER, GES_RANK_DEFICIENT = 0, 1, 2
_CLIGHT = 299792458.0


def _ges_istd(el, dt, mea_var):
    """1 / sqrt(varerr2) of gnss_factor.cpp:98-103: the reference's float sine, correctly rounded (as tests/np_factors.py has it)"""
    s = np.sin(np.asarray(el, np.float64).astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    b = _CLIGHT * 5e-12 * np.asarray(dt, np.float64)
    return 1.0 / np.sqrt(np.asarray(mea_var, np.float64) / s / s + b * b)


def gnss_epoch_records(cp=None, pr=None, spr=None, scp=None, dop=None):
    """The unified records of swf_gnss_epoch_solve_batch from the factor records of the flat window, in the order cp, pr, spr, scp, dop:
      cp  = (dat [k][SWF_CP_DOUBLES = 9], clock slot [k], N [k], free [k])   RTKCarrierPhaseFactor; w = 1 / sqrt(varerr2) or 1 (use_istd = 0)
      pr  = (dat [k][SWF_PR_DOUBLES = 7], clock slot [k])                    RTKPseudorangeFactor;  w = 1 / sqrt(varerr2)
      spr = (dat [k][SWF_SPR_DOUBLES = 5], clock slot [k])                   SppPseudorangeFactor;  w = istd
      scp = (dat [k][SWF_SCP_DOUBLES = 6], clock slot [k], N [k], free [k])  SppCarrierPhaseFactor; w = istd
      dop = (dat [k][SWF_DOP_DOUBLES = 8], clock slot [k] or None = 12)      SppDopplerFactor;      w = istd
    Returns (dat [n][10] = sat[3] satvel[3] obs w lam N, rec [n][4] = kind, clock slot, state bits, 0)."""
    dats, recs = [], []

    def put(kind, d, width, slot, obs, w, lam=None, N=None, free=None, satvel=None):
        d = np.asarray(d, np.float64).reshape(-1, width)
        k = d.shape[0]
        o = np.zeros((k, GES_DOUBLES))
        o[:, 0:3] = d[:, 0:3]
        if satvel is not None:
            o[:, 3:6] = d[:, satvel:satvel + 3]
        o[:, 6] = d[:, obs]
        o[:, 7] = w(d)
        o[:, 8] = d[:, lam] if lam is not None else 1.0
        o[:, 9] = np.asarray(N, np.float64).reshape(k) if N is not None else 0.0
        q = np.zeros((k, 4), np.int32)
        q[:, 0] = kind
        q[:, 1] = np.asarray(slot, np.int32).reshape(k)
        if free is not None:
            q[:, 2] = np.where(np.asarray(free).reshape(k) != 0, GES_AMB_FREE, 0)
        dats.append(o); recs.append(q)

    if cp is not None:
        put(GES_RTK_PHASE, cp[0], 9, cp[1], 3, lambda d: np.where(d[:, 8] != 0.0, _ges_istd(d[:, 5], d[:, 6], d[:, 7]), 1.0), lam=4, N=cp[2], free=cp[3])
    if pr is not None:
        put(GES_RTK_CODE, pr[0], 7, pr[1], 3, lambda d: _ges_istd(d[:, 4], d[:, 5], d[:, 6]))
    if spr is not None:
        put(GES_SPP_CODE, spr[0], 5, spr[1], 3, lambda d: d[:, 4])
    if scp is not None:
        put(GES_SPP_PHASE, scp[0], 6, scp[1], 3, lambda d: d[:, 4], lam=5, N=scp[2], free=scp[3])
    if dop is not None:
        k = np.asarray(dop[0], np.float64).reshape(-1, 8).shape[0]
        slot = np.full(k, 12, np.int32) if len(dop) < 2 or dop[1] is None else dop[1]
        put(GES_DOPPLER, dop[0], 8, slot, 6, lambda d: d[:, 7], satvel=3)
    if not dats:
        return np.zeros((0, GES_DOUBLES)), np.zeros((0, 4), np.int32)
    return np.ascontiguousarray(np.concatenate(dats)), np.ascontiguousarray(np.concatenate(recs))


def gnss_epoch_solve_batch(first, pos, vel, base, clock, mode, clk_const, dat, rec, max_iter=20, step_tol=1e-4, eps_rank=1e-8):
    """The single-epoch GNSS solve for a batch of epochs on the device (swf_gnss_epoch_solve_batch, which see): the seed mini-solve of
    GnssPreprocess (mode = 0, max_iter = 2) and the first fix of GnssProcess (mode = GES_FREE_POS | GES_FREE_VEL, max_iter = 20).
    first [E + 1], pos / vel / base [E][3], clock [E][13], mode [E], clk_const [E] (bit s: clock s constant), dat [n][10] = sat[3]
    satvel[3] obs w lam N, rec [n][4] = kind, clock slot, state bits, 0 (gnss_epoch_records builds both).  Returns dict(pos, vel [E][3],
    clock [E][13], N [n], r [n], cost [E], iters [E], status [E], clk_rows [E][13], info [E][6][6])."""
    first = np.ascontiguousarray(first, np.int32).ravel()
    E = first.size - 1
    if E < 0:
        raise ValueError("gnss_epoch_solve_batch: first needs n_epochs + 1 entries")
    pos, vel, base, clock = (np.ascontiguousarray(v, np.float64).reshape(-1) for v in (pos, vel, base, clock))
    mode, clk_const = (np.ascontiguousarray(v, np.int32).ravel() for v in (mode, clk_const))
    dat = np.ascontiguousarray(dat, np.float64).reshape(-1)
    rec = np.ascontiguousarray(rec, np.int32).reshape(-1)
    n = dat.size // GES_DOUBLES
    if (pos.size != 3 * E or vel.size != 3 * E or base.size != 3 * E or clock.size != GES_CLOCKS * E or mode.size != E or clk_const.size != E
            or dat.size != n * GES_DOUBLES or rec.size != 4 * n or (E and int(first[-1]) > n)):
        raise ValueError("gnss_epoch_solve_batch: array sizes do not match first")
    pad = lambda a, k, t: a if a.size else np.zeros(k, t)              # (a valid pointer for an empty array)
    pos, vel, base, clock = pad(pos, 3, np.float64), pad(vel, 3, np.float64), pad(base, 3, np.float64), pad(clock, GES_CLOCKS, np.float64)
    mode, clk_const, dat, rec = pad(mode, 1, np.int32), pad(clk_const, 1, np.int32), pad(dat, GES_DOUBLES, np.float64), pad(rec, 4, np.int32)
    E1, n1 = max(E, 1), max(n, 1)
    out = dict(pos=np.zeros((E1, 3)), vel=np.zeros((E1, 3)), clock=np.zeros((E1, GES_CLOCKS)), N=np.zeros(n1), r=np.zeros(n1), cost=np.zeros(E1),
               iters=np.zeros(E1, np.int32), status=np.zeros(E1, np.int32), clk_rows=np.zeros((E1, GES_CLOCKS), np.int32), info=np.zeros((E1, 6, 6)))
    pi = C.POINTER(C.c_int32)
    ptr = lambda a: a.ctypes.data_as(_pd if a.dtype == np.float64 else pi)
    _chk(lib().swf_gnss_epoch_solve_batch(C.c_int32(E), ptr(first), ptr(pos), ptr(vel), ptr(base), ptr(clock), ptr(mode), ptr(clk_const), ptr(dat),
                                          ptr(rec), C.c_int32(max_iter), C.c_double(step_tol), C.c_double(eps_rank), ptr(out["pos"]),
                                          ptr(out["vel"]), ptr(out["clock"]), ptr(out["N"]), ptr(out["r"]), ptr(out["cost"]), ptr(out["iters"]),
                                          ptr(out["status"]), ptr(out["clk_rows"]), ptr(out["info"]), C.c_int32(0), None),
         "swf_gnss_epoch_solve_batch")
    for k in ("N", "r"):
        out[k] = out[k][:n]
    for k in ("pos", "vel", "clock", "cost", "iters", "status", "clk_rows", "info"):
        out[k] = out[k][:E]
    return out


def problem_from_window(w):
    """Build a Problem from a FlatWindow the way the estimator would (AddParameterBlock /
    AddResidualBlock / SetParameterBlockConstant / ordering), returning (problem, blocks) where
    blocks[global_id] is the numpy parameter block."""
    P = Problem()
    a = w.a
    pose = [a["pose"].reshape(-1, 7)[i].copy() for i in range(w.n_pose)]
    sb = [a["sb"].reshape(-1, 9)[i].copy() for i in range(w.n_sb)]
    lm = [a["lm"].reshape(-1, 3)[i].copy() for i in range(w.n_lm)]
    sc = [a["sc"][i:i + 1].copy() for i in range(w.n_sc)]
    blocks = pose + sb + lm + sc
    P.SetConstants(w.pbg, w.gw, w.base)
    for b in pose:
        P.AddParameterBlock(b, 7, True)
    for p_, e_, l_, uv in zip(*a["proj_idx"].reshape(-1, 3).T, a["proj_uv"].reshape(-1, 2)):
        P.AddProjection(pose[p_], pose[e_], lm[l_], uv, w.proj_sqrt_info, w.proj_loss_a)
    for ix, pre in zip(a["imu_idx"].reshape(-1, 4), a["imu_pre"].reshape(-1, 293)):
        P.AddImu(pose[ix[0]], sb[ix[1]], pose[ix[2]], sb[ix[3]], pre)
    for ix, d in zip(a["cp_idx"].reshape(-1, 3), a["cp_dat"].reshape(-1, 9)):
        P.AddRtkCarrierPhase(pose[ix[0]], sc[ix[1]], sc[ix[2]], d)
    for ix, d in zip(a["pr_idx"].reshape(-1, 2), a["pr_dat"].reshape(-1, 7)):
        P.AddRtkPseudorange(pose[ix[0]], sc[ix[1]], d)
    for ix, d in zip(a["dop_idx"].reshape(-1, 3), a["dop_dat"].reshape(-1, 8)):
        P.AddDoppler(sb[ix[0]], sc[ix[1]], pose[ix[2]], d)
    for i, wv in zip(a["sp_idx"], a["sp_w"]):
        P.AddScalarPrior(sc[i], wv)
    for ix, d in zip(a["spr_idx"].reshape(-1, 2), a["spr_dat"].reshape(-1, 5)):
        P.AddSppPseudorange(pose[ix[0]], sc[ix[1]], d)
    for ix, d in zip(a["scp_idx"].reshape(-1, 3), a["scp_dat"].reshape(-1, 6)):
        P.AddSppCarrierPhase(pose[ix[0]], sc[ix[1]], sc[ix[2]], d)
    for ix, d in zip(a["fix_idx"].reshape(-1, 2), a["fix_dat"].reshape(-1, 2)):
        P.AddFixedInteger(sc[ix[0]], sc[ix[1]], d[0], d[1])
    for kd, ix, pt in zip(a["idp_kind"], a["idp_idx"].reshape(-1, 5), a["idp_pts"].reshape(-1, 6)):
        P.AddProjectionInverseDepth(int(kd), pose[ix[0]] if kd != 2 else None, pose[ix[1]] if kd != 2 else None, pose[ix[2]], pose[ix[3]] if kd != 0 else None,
                                    sc[ix[4]], pt[:3], pt[3:], w.proj_sqrt_info, w.proj_loss_a)
    hidden = []
    io = e0 = pn = nn = no = 0
    for k in range(a["comp_M"].size):
        M, N = int(a["comp_M"][k]), int(a["comp_N"][k])
        ix = a["comp_idx"][io:io + 4 + N]
        hp = a["comp_pose"].reshape(-1, 7)[e0:e0 + M].copy(); hs = a["comp_sb"].reshape(-1, 9)[e0:e0 + M].copy()
        hidden.append((hp, hs))
        fid = P.AddImuGnss(pose[ix[0]], sb[ix[1]], pose[ix[2]], sb[ix[3]], [sc[i] for i in ix[4:]], hp, hs,
                     a["comp_pose_lin"].reshape(-1, 7)[e0:e0 + M], a["comp_sb_lin"].reshape(-1, 9)[e0:e0 + M], a["comp_Hpp"].reshape(-1, 225)[e0:e0 + M],
                     a["comp_HpN"][pn:pn + 15 * M * N], a["comp_rhs_p"].reshape(-1, 15)[e0:e0 + M], a["comp_HNN"][nn:nn + N * N], a["comp_rhsN"][no:no + N],
                     a["comp_pre"].reshape(-1, 293)[e0 + k:e0 + k + M + 1])
        if a["comp_mid"].size and a["comp_mid"][k]:
            P.SetImuGnssMidLink(fid, int(a["comp_mid"][k]), a["comp_H12"].reshape(-1, 225)[k])
        io += 4 + N; e0 += M; pn += 15 * M * N; nn += N * N; no += N
    P.hidden = hidden
    bo = jo = ro = xo = 0
    for nb, dim in zip(a["prior_nblk"], a["prior_dim"]):
        ids = a["prior_blk"][bo:bo + nb]
        gs = sum(blocks[i].size for i in ids)
        P.AddLinearPrior([blocks[i] for i in ids], a["prior_J"].ravel()[jo:jo + dim * dim],
                         a["prior_r0"][ro:ro + dim], a["prior_x0"][xo:xo + gs])
        bo += nb; jo += dim * dim; ro += dim; xo += gs
    for i, c in enumerate(a["is_const"]):
        if c:
            P.SetParameterBlockConstant(blocks[i])
    P.SetOrdering([blocks[i] for i in a["order_block"]], a["order_group"])
    n_tail = w.n_tail
    P.SetParameterHead([blocks[i] for i in a["order_block"][len(a["order_block"]) - n_tail:]] if n_tail else [])
    return P, blocks
