#!/usr/bin/env python
"""bench.py — Gauss-Newton iterations/sec of the sliding-window solver on MI355X.

One "step" = one full solve (<= 8 dogleg iterations, each = Jacobian evaluation of every block +
J^T J assembly + Schur + dense reduced solve + step + cost re-evaluation + accept/reject) of BASELINE
cfg4: a batch of 512 independent cfg3 windows (20 keyframes / 300 features / 10 satellites) whose
structure and state are already resident in HBM.  The windows shard across the GPUs in contiguous
blocks with no data-path collective — STRONG scaling by default, as SURVEY.md 8e specifies (512 windows
over the job, 512 / N per rank; --scaling weak gives every rank --windows of its own).
value = whole-job Gauss-Newton iterations per second.

Driver contract: python bench.py --gpus N --steps K --warmup W.  When launched plainly with N > 1 this
script re-executes itself under torch.distributed.run (one rank per GPU, rendezvous on 127.0.0.1); when
the driver has already launched it that way (RANK / WORLD_SIZE in the environment) it just runs its rank.

A plain run does only what the headline line needs: generate the windows, upload them, warm up, time the K
steps and print the line (value, ms_per_step, the job's per-window summary statistics).  --full adds every
secondary measurement behind the timed steps: the side-rows pass, the PCIe-inclusive protocols, the roofline
(live rocprofv3 PMC traffic), the single-window latency path, the ceres::Problem surface, the cfg5 stress
block, the reference-topology configuration, the CPU baseline and the strong-scaling projection.
--dump-outputs DIR writes what the timed path computed in its last step as float64 .npy files (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured copy)
FP64_MATRIX_PEAK_TFLOPS = 78.6  # MI355X datasheet FP64 matrix peak; the guide lists no fp64 figure
FP64_MATRIX_MEASURED_TFLOPS = 47.7  # tests/microbench/mfma_f64_peak.hip on the gpurun box (v_mfma_f64_16x16x4_f64, 4 waves/SIMD)


def _gen(args):
    cfg, seed = args
    from rtk_visual_inertial_navigation_amd import synth
    return synth.make_window(config_id=cfg, seed=seed)


def make_windows(cfg, seeds):
    import multiprocessing as mp
    n = min(len(seeds), max(1, min(32, (os.cpu_count() or 2) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))))))
    if n <= 1 or len(seeds) < 8:
        return [_gen((cfg, s)) for s in seeds]
    with mp.get_context("fork").Pool(n) as pool:
        return pool.map(_gen, [(cfg, s) for s in seeds], chunksize=max(1, len(seeds) // (4 * n)))


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _physical_cores():
    """Physical cores from lscpu (sockets x cores per socket); falls back to os.cpu_count()."""
    import subprocess
    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = dict((l.split(":", 1)[0].strip(), l.split(":", 1)[1].strip()) for l in txt.splitlines() if ":" in l)
        return int(kv["Socket(s)"]) * int(kv["Core(s) per socket"]), kv.get("Model name", _cpu_model())
    except Exception:
        return os.cpu_count() or 1, _cpu_model()


def cpu_baseline(windows, iters, budget_s=24.0):
    """The reference's CPU path cannot be built here (no Eigen / Ceres / ROS in the image), so the CPU leg is the oracle — a plain,
    UNVECTORISED C port of the same algorithm (oracle/swf_oracle.c, kind "port") — timed on this host on a bounded sample of the
    SAME cfg3 windows, as SURVEY.md 8d prescribes: the reference's configuration first (num_threads = 4 INSIDE one solve,
    R/swf/swf.cpp:29: OpenMP over factor evaluation and over the group-0 elimination), then one thread and every physical core,
    >= 50 warm solves per row where the budget allows, median / p10 / p90 of us per Gauss-Newton iteration.  `value` is the
    4-threads-inside-one-solve rate (iterations/s of ONE solve at a time).  The last row is a throughput figure only: one
    single-threaded solve per core, many windows at once — not how the reference runs."""
    import oracle_binding as ob
    from concurrent.futures import ThreadPoolExecutor
    from rtk_visual_inertial_navigation_amd.flat import default_options
    isa = ob.use_native() or "-O3 -march=x86-64-v3 (prebuilt; the -march=native rebuild on this host failed)"
    ob.lib()
    cores, model = _physical_cores()
    rows = {}
    per_row = budget_s / 4.0

    def timed(nthreads):
        opt = default_options(max_num_iterations=iters, num_threads=nthreads)
        ob.solve(windows[0].copy(), opt, export=False)                       # warm
        us, t_all, k = [], time.perf_counter(), 0
        while k < 50 or (time.perf_counter() - t_all < per_row and k < 400):
            w = windows[k % len(windows)].copy()
            t0 = time.perf_counter()
            sm, _ = ob.solve(w, opt, export=False)
            us.append(1e6 * (time.perf_counter() - t0) / max(1, sm.num_iterations)); k += 1
            if time.perf_counter() - t_all > 2.0 * per_row:
                break
        us = np.array(us)
        return dict(threads=nthreads, solves=int(us.size), us_per_iteration_median=float(np.median(us)), us_per_iteration_p10=float(np.percentile(us, 10)),
                    us_per_iteration_p90=float(np.percentile(us, 90)), iterations_per_s=float(1e6 / np.median(us)))

    rows["threads_4_inside_one_solve"] = timed(4)
    rows["threads_1"] = timed(1)
    rows["threads_all_cores_inside_one_solve"] = timed(cores)
    rows["threads_all_cores_inside_one_solve"]["note"] = "oversubscribed: %d OpenMP threads inside one 20-frame solve is slower than one thread; kept for completeness, not a baseline" % cores
    # throughput mode: `cores` independent single-threaded solves at a time
    n = int(min(len(windows), max(cores, 2 * cores)))
    sample = [w.copy() for w in windows[:n]]

    def run(w):
        s_, _ = ob.solve(w, default_options(max_num_iterations=iters), export=False)
        return s_.num_iterations
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        its = list(ex.map(run, sample))
    dtp = time.perf_counter() - t0
    rows["independent_windows_one_thread_each"] = dict(threads=cores, windows=n, iterations_per_s=sum(its) / dtp, wall_s=dtp)
    r4 = rows["threads_4_inside_one_solve"]
    return dict(value=r4["iterations_per_s"], unit="gauss_newton_iterations/s", cores=4, kind="port",
                sample="%d warm solves of the benchmark's cfg3 windows (%d dogleg iterations each) with 4 OpenMP threads inside one solve; "
                       "unvectorised plain-C port of the reference's algorithm (the reference itself is unbuildable here)" % (r4["solves"], iters),
                build="gcc " + isa + ", built on the host it is timed on",
                rows=rows, single_thread_us_per_iteration=rows["threads_1"]["us_per_iteration_median"],
                host_physical_cores=cores, host_logical_cpus=os.cpu_count(), host_cpu_model=model)


def structure_change_leg(w0, iters, reps=5, n_swap=30):
    """The pointer-keyed ceres::Problem surface on ONE cfg3 window, timed the way the estimator drives it: a first Solve (symbolic
    phase + upload), Solves where only parameter values changed, and Solves after the per-frame structure change of the
    reference (R/swf/swf_image.cpp:65-114, R/feature/feature_manager.cpp:122-139): `n_swap` landmarks removed with their
    projection factors (RemoveParameterBlock cascades) and as many new ones added with their observations, ordering re-issued.
    Wall-clock milliseconds of swf_problem_solve, host bookkeeping, transfers and synchronisation included."""
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    P, blocks = solver.problem_from_window(w0)
    opt = default_options(max_num_iterations=iters)
    saved = [b.copy() for b in blocks]

    def restore():
        for b, s_ in zip(blocks, saved):
            b[...] = s_

    def solve_ms():
        t0 = time.perf_counter()
        sm = P.Solve(opt)
        return 1e3 * (time.perf_counter() - t0), sm
    first, sm0 = solve_ms()
    values_only = []
    for _ in range(reps):
        restore(); values_only.append(solve_ms()[0])
    a = w0.a
    pidx, puv = a["proj_idx"].reshape(-1, 3), a["proj_uv"].reshape(-1, 2)
    order_blocks = [blocks[i] for i in a["order_block"]]; order_groups = list(a["order_group"])
    pos = {id(b): k for k, b in enumerate(order_blocks)}
    lm_ids = list(range(min(n_swap, w0.n_lm)))
    cur = {l: blocks[w0.bid_lm(l)] for l in lm_ids}
    changed = []
    for _ in range(reps):
        restore()
        t_edit = time.perf_counter()
        for l in lm_ids:
            old = cur[l]
            P.RemoveParameterBlock(old)
            new = saved[w0.bid_lm(l)].copy()
            for (p_, e_, l_), uv in zip(pidx[pidx[:, 2] == l], puv[pidx[:, 2] == l]):
                P.AddProjection(blocks[w0.bid_pose(p_)], blocks[w0.bid_pose(e_)], new, uv, w0.proj_sqrt_info, w0.proj_loss_a)
            order_blocks[pos[id(old)]] = new; pos[id(new)] = pos.pop(id(old)); cur[l] = new
        P.SetOrdering(order_blocks, order_groups)
        t_edit = 1e3 * (time.perf_counter() - t_edit)
        ms, sm = solve_ms()
        changed.append((ms, t_edit))
    P.close()
    med = lambda v: float(np.median(v))
    return dict(first_solve_ms=first, values_only_solve_ms=med(values_only), after_structure_change_solve_ms=med([c[0] for c in changed]),
                python_side_edit_ms=med([c[1] for c in changed]), landmarks_swapped=len(lm_ids), iterations=int(sm0.num_iterations),
                note="wall clock of swf_problem_solve on one cfg3 window through the ceres::Problem-shaped C-ABI")


def live_pmc_traffic(kernel_prefix, n_windows, timeout_s=150):
    """HBM traffic of one kernel, measured NOW on this box: two separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; TCC counters do not
    share a pass, and a counter pass is never combined with tracing) over tools/prof/gpu_batch_prof.py — the same windows, batch only, one
    8-iteration solve — as a child process.  Returns (bytes per launch, per-kernel table) with the guide's gfx950 correction
    (FETCH_SIZE x 2 for wide coalesced reads), or None when rocprofv3 is unavailable / fails / times out (the caller then falls back to the
    committed profile and says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    tmp = tempfile.mkdtemp(prefix="swfpmc", dir="/tmp")
    env = dict(os.environ); env["TMPDIR"] = "/tmp"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = {}
    try:
        for cn in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, cn)
            cmd = [exe, "--pmc", cn, "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable,
                   os.path.join(ROOT, "tools", "prof", "gpu_batch_prof.py"), str(n_windows), "1"]
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            f = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if not f:
                return None
            acc = {}
            for r in csv.DictReader(open(f[0])):
                if r.get("Counter_Name") != cn:
                    continue
                a_ = acc.setdefault(r["Kernel_Name"], [0, 0.0]); a_[0] += 1; a_[1] += float(r["Counter_Value"])
            res[cn] = {k: v[1] / max(1, v[0]) * 1024.0 for k, v in acc.items()}          # counter unit = KB
        ks = [k for k in res["FETCH_SIZE"] if kernel_prefix in k]
        if not ks:
            return None
        k0 = ks[0]
        per_kernel = {k[:64]: 2.0 * res["FETCH_SIZE"][k] + res["WRITE_SIZE"].get(k, 0.0) for k in res["FETCH_SIZE"]}
        return 2.0 * res["FETCH_SIZE"][k0] + res["WRITE_SIZE"].get(k0, 0.0), per_kernel
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def rtk_topology_leg(iters, wxs, cpu=True):
    """The reference's OWN RTK topology at BASELINE cfg3 size: windows of 20 visual frames
    linked only by composite IMU-GNSS factors, each hiding 4 GNSS epochs whose raw carrier-phase / pseudorange factors were pre-eliminated
    to a linear prior (GnssPreprocess, R/swf/swf_gnss.cpp:504-532), ~280 landmarks / ~2 800 observations, 10 ambiguities, ordered by
    MyOrdering as it is (every other speed-bias block in elimination group 0: n_red = 220 as for the raw-GNSS cfg3 window) — built and
    solved on the device: (1) every GNSS epoch of every window as one batch through swf_batch_marginal_priors, (2) AddMargInfo's
    bookkeeping on the host (swf_composite_assemble), (3) the composite windows through the solver: ONE window (latency), the batch of
    distinct windows, the same batch replicated to 512 windows (throughput), the oracle on the same windows (CPU row), and the
    warm-start probe that explains the cold windows' iteration counts.  Synthetic data (tests/rtk_topology_gen.py, a generator only;
    wxs = its explicit windows, generated in a process pool before this process touched HIP)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rtk_topology_gen as rt
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    n_windows = len(wxs)
    ek0 = rt.epoch_windows(wxs[0])[0]
    solver.marginal_priors(ek0[:8], 1e-8, solver.BatchSolver.PRIOR_EIGEN)           # warm-up (library load, first launches)
    tm = {}
    wins = rt.composite_batch(solver, wxs, timing=tm)
    opt = default_options(max_num_iterations=iters)

    def timed(ws, reps, warm=2):
        bs = solver.BatchSolver(ws)
        for _ in range(warm):
            bs.reset_state(); bs.solve_async(opt); bs.sync()
        lat = []
        for _ in range(reps):
            bs.reset_state(); t0 = time.perf_counter(); bs.solve_async(opt); bs.sync(); lat.append(time.perf_counter() - t0)
        sms = bs.summaries()
        n_red = bs.dims(0)["n_red"]
        bs.close()
        return float(np.median(lat)), sms, n_red
    dt1, sm1, n_red = timed([wins[0].copy()], 20, 3)
    # the same window with the reference's own square root of the composite remainders (swf_options::composite_root = SWF_ROOT_EIGEN,
    # UpdateSchurComponent R/factor/gnss_imu_factor.cpp:454-488): the separate-launch form of the chain + k_comp_eigroot
    opt_piv = opt
    opt = default_options(max_num_iterations=iters, composite_root=1)
    dt1e, sm1e, _ = timed([wins[0].copy()], 20, 3)
    dtbe, smbe, _ = timed([w.copy() for w in wins], 6)
    opt = opt_piv
    dtb, smb, _ = timed([w.copy() for w in wins], 10)
    rep = max(1, 512 // n_windows)
    dtr, smr, _ = timed([w.copy() for _ in range(rep) for w in wins], 6)
    its1 = sm1[0].num_iterations; itsb = sum(s.num_iterations for s in smb); itsr = sum(s.num_iterations for s in smr)
    cw, wi, ci = rt.warm_start_probe(solver, wins[:16], opt, default_options(max_num_iterations=50))
    out = dict(workload="%d visual frames x %d hidden GNSS epochs per gap, %d landmarks, %d observations, %d ambiguities, %d composite factors per window; n_red %d"
                        % (wins[0].meta["K"], wins[0].meta["M"], wins[0].n_lm, wins[0].a["proj_idx"].size // 3, wins[0].meta["N"], wins[0].a["comp_M"].size, n_red),
               single_window=dict(us_per_iteration=1e6 * dt1 / max(1, its1), solve_ms=1e3 * dt1, iterations=int(its1)),
               eigen_root=dict(single_window_us_per_iteration=1e6 * dt1e / max(1, sm1e[0].num_iterations), single_window_iterations=int(sm1e[0].num_iterations),
                               batch_windows=n_windows, batch_solve_ms=1e3 * dtbe, batch_iterations_per_s=sum(s.num_iterations for s in smbe) / dtbe,
                               note="swf_options::composite_root = SWF_ROOT_EIGEN (the reference's SelfAdjointEigenSolver root, cut 1e-8); the rows above and below use the default pivoted root"),
               batch=dict(windows=n_windows, solve_ms=1e3 * dtb, iterations_per_s=itsb / dtb, us_per_window_iteration=1e6 * dtb / itsb,
                          failed_windows=int(sum(s.termination not in (1, 2, 3, 4) for s in smb))),
               batch_replicated=dict(windows=rep * n_windows, solve_ms=1e3 * dtr, iterations_per_s=itsr / dtr, us_per_window_iteration=1e6 * dtr / itsr,
                                     note="the %d distinct windows x %d (independent windows: throughput only)" % (n_windows, rep)),
               converged_within_budget_cold=int(sum(s.termination in (1, 2, 3) for s in smb)),
               cold_mean_iterations_to_termination=ci,
               warm_start=dict(windows=min(16, n_windows), converged_within_budget=cw, mean_iterations=wi,
                               note="the windows converged, then ONLY the newest frame moved by an IMU-prediction-sized error (5 cm, 5 cm/s, 2 mrad) — what the "
                                    "estimator hands the solver at every frame; the cold windows start with EVERY state perturbed (cost 2e7 -> 9e2 in the first "
                                    "step) and the composite factors' re-linearisation of their hidden epochs (UpdateHiddenState, R/factor/gnss_imu_factor.cpp:601-632) "
                                    "makes the tail of that descent linear, for the oracle as for the device"),
               mean_cost_reduction=float(np.mean([s.final_cost / s.initial_cost for s in smb])),
               construction=dict(gnss_epochs=tm["gnss_epochs"], epoch_priors_ms=1e3 * tm["epoch_priors_s"], epoch_priors_per_s=tm["gnss_epochs"] / tm["epoch_priors_s"],
                                 epoch_priors_with_python_marshalling_ms=1e3 * tm["epoch_priors_with_python_marshalling_s"], host_assemble_ms=1e3 * tm["host_assemble_s"]),
               note="reference-topology RTK windows at cfg3 size: per-epoch GNSS pre-elimination batched on the device, composite IMU-GNSS factors in the solve loop, MyOrdering's elimination order")
    if cpu:
        import oracle_binding as ob
        ts, itc = [], 0
        for w in wins[:4]:
            wo = w.copy(); t0 = time.perf_counter(); so, _ = ob.solve(wo, opt, export=False); ts.append(time.perf_counter() - t0); itc += so.num_iterations
        out["cpu_oracle"] = dict(us_per_iteration=1e6 * sum(ts) / max(1, itc), solve_ms=1e3 * float(np.mean(ts)), threads=int(opt.num_threads),
                                 sample="the first 4 of the same windows, %d iterations each, plain-C port" % iters)
        out["single_window"]["speedup_vs_cpu_oracle"] = out["cpu_oracle"]["us_per_iteration"] / out["single_window"]["us_per_iteration"]
    return out


def stress_fulls(n_windows):
    """The 41-frame parents of the cfg5 stress windows (tests/cfg5_marg_gen.py): generated in a process pool BEFORE this process touches
    HIP; the marginalisation of the 41st frame itself runs on the device later (stress_leg)."""
    import multiprocessing as mp
    import cfg5_marg_gen as cg
    from rtk_visual_inertial_navigation_amd import synth
    jobs = [(40, 1000, 20, synth.BASE_SEED + 5 + i) for i in range(n_windows + max(2, n_windows // 8))]      # a few spares (a seed whose marginalisation window is refused is skipped)
    if n_windows < 4:
        return [cg.make_full(j) for j in jobs[:n_windows + 1]]
    with mp.get_context("fork").Pool(min(len(jobs), 32, os.cpu_count() or 2)) as pool:
        return pool.map(cg.make_full, jobs)


def stress_leg(fulls, n_windows, iters):
    """BASELINE cfg5 (north_star: "rocprof-reported ... counters on the stress config" live in profiles/; this block puts the stress
    configuration's own numbers into the driver-run line): 40 keyframes / 1000 features / 20 satellites, the dense prior OBTAINED by
    marginalising a 41st frame on the device.  One window (latency) and a batch: us per iteration, the matrix-core kernels' achieved
    fraction of the fp64 datasheet peak (HIP-event averages of the launches), Jacobian GB/s."""
    import cfg5_marg_gen as cg
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    t0 = time.perf_counter()
    ws, dims = [], []
    for f in fulls:
        try:
            w, info = cg.make_cfg5_with_marginalised_prior(solver, full=f)
        except (solver.SwfError, AssertionError):
            continue
        ws.append(w); dims.append(int(info["prior_dim"]))
        if len(ws) == n_windows:
            break
    t_marg = time.perf_counter() - t0
    opt = default_options(max_num_iterations=iters)

    def run(batch, reps):
        bs = solver.BatchSolver([w.copy() for w in batch])
        bs.enable_timing(True)
        for _ in range(2):
            bs.reset_state(); bs.solve_async(opt); bs.sync()
        acc, lat = {}, []
        for _ in range(reps):
            bs.reset_state(); bs.solve_async(opt); bs.sync()
            t = bs.timing(); lat.append(t["total_ms"])
            for k, v in t["kernels"].items():
                d = acc.setdefault(k, [0.0, 0]); d[0] += v["ms"]; d[1] += v["calls"]
        t = bs.timing(); sms = bs.summaries(); d0 = bs.dims(0); bs.close()
        its = sum(s_.num_iterations for s_ in sms)
        ms = float(np.median(lat))
        avg = lambda k: acc[k][0] / max(1, acc[k][1]) if k in acc else None
        out = dict(windows=len(batch), solve_ms_median=ms, us_per_iteration=1e3 * ms / max(1, its / len(batch)), iterations_per_s=its / (1e-3 * ms),
                   n_red=d0["n_red"], failed_windows=int(sum(s_.termination not in (1, 2, 3, 4) for s_ in sms)))
        if avg("chol_solve"):
            fl = t["chol_flops"]
            out["chol_solve"] = dict(kernel="k_chol_big / k_chol_col (tiles streamed from L2, n_red > 240)", avg_ms_per_factorisation=avg("chol_solve"), algorithmic_flops=fl,
                                     frac_of_fp64_matrix_peak=fl / (avg("chol_solve") * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS)
        if avg("lm_schur"):
            fs = t["lm_schur_flops_sym"]
            out["lm_schur"] = dict(kernel="k_lm_schur<12, 6, 1, 272, true> (two launches over the tile list)", avg_launch_ms=avg("lm_schur"), algorithmic_flops_symmetric=fs,
                                   launches_per_linearisation=acc["lm_schur"][1] / max(1, acc["eval_ps"][1]),
                                   frac_of_fp64_matrix_peak_symmetric=fs / (avg("lm_schur") * acc["lm_schur"][1] / max(1, acc["eval_ps"][1]) * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS)
        if avg("eval_ps"):
            out["jacobian"] = dict(kernel="k_eval_ps<true, true>", avg_launch_ms=avg("eval_ps"), algorithmic_bytes=t["proj_bytes"],
                                   achieved_GBs=t["proj_bytes"] / (avg("eval_ps") * 1e-3) / 1e9, frac_of_hbm_peak=t["proj_bytes"] / (avg("eval_ps") * 1e-3) / 1e9 / HBM_PEAK_GBS)
        return out
    res = dict(config="BASELINE cfg5: 40 keyframes, 1000 features, 20 satellites, dense marginalisation prior obtained on the device", prior_dims=dims[:4],
               marginalise_41st_frame_s=t_marg, single_window=run(ws[:1], 10))
    if len(ws) > 1:
        res["batch"] = run(ws, 5)
    # SURVEY.md 8f rank 1 at this size: the marginalisation consumer on the window GlobalMarge solves (every factor that touches frame 0,
    # is_optimize = false), both square-root forms, wall time per call including the download of the prior (A, b, J, r0)
    try:
        wm, _head = cg.marginalisation_window(fulls[0])
        bs = solver.BatchSolver([wm.copy()])
        sm = bs.solve(default_options(step_mode=1), download=False)[0]
        mc = dict(window="GlobalMarge's (frame 0, its speed-bias, receiver clock and first-seen landmarks marginalised)", tail_dim=int(sm.tail_dim), n_red=int(sm.reduced_dim))
        for form, name in ((solver.BatchSolver.PRIOR_EIGEN, "eigen_form"), (solver.BatchSolver.PRIOR_CHOLESKY, "cholesky_form")):
            ts, g = [], None
            for _ in range(5):
                t1 = time.perf_counter(); bs.marginalize(1e-8, form); g = bs.get_prior(0); ts.append(time.perf_counter() - t1)
            A, J, b_, r0 = g["A"], g["J"], g["b"], g["r0"]
            mc[name] = dict(ms_per_call=1e3 * float(np.median(ts[1:])), rank=int(g["rank"]),
                            JtJ_vs_A=float(np.abs(J.T @ J - A).max() / np.abs(A).max()), Jtr0_vs_b=float(np.abs(J.T @ r0 - b_).max() / np.abs(b_).max()))
        bs.close()
        res["marginalisation_consumer"] = mc
    except (solver.SwfError, AssertionError) as e:
        res["marginalisation_consumer"] = dict(error=str(e))
    return res


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, bs, windows, sms, first, rank, world):
    """What a caller of the timed path receives from its last step, as float64 .npy files in out_dir: the solved parameter blocks of
    every window (pose, sb, lm, sc: the windows' blocks concatenated in window order) and the per-window summaries (initial_cost,
    final_cost, num_iterations, termination); window_index holds the job-wide index of every window written.  The download goes into
    the windows' host arrays, which get their unsolved values back afterwards, so whatever runs next starts from the same state.
    Should the batch's outputs exceed 64 MB, a fixed seeded sample of its windows is written instead.  Ranks other than a lone one
    suffix their files with _rank<r>."""
    os.makedirs(out_dir, exist_ok=True)
    snap = [w.state() for w in windows]
    bs.download_state()
    solved = [w.state() for w in windows]
    for w, s_ in zip(windows, snap):
        w.set_state(s_)
    per_window = [sum(v.nbytes for v in s_.values()) + 5 * 8 for s_ in solved]
    idx = np.arange(len(windows))
    if sum(per_window) > DUMP_CAP_BYTES:
        k = max(1, int(DUMP_CAP_BYTES // max(per_window)))
        idx = np.sort(np.random.default_rng(20240611).choice(len(windows), size=k, replace=False))
    arrays = {k: np.concatenate([solved[i][k].ravel() for i in idx]) for k in ("pose", "sb", "lm", "sc")}
    for k in ("initial_cost", "final_cost", "num_iterations", "termination"):
        arrays[k] = np.array([getattr(sms[i], k) for i in idx], dtype=np.float64)
    arrays["window_index"] = (first + idx).astype(np.float64)
    suffix = "" if world == 1 else "_rank%d" % rank
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), np.ascontiguousarray(v, dtype=np.float64))


def relaunch_under_torchrun(n):
    """python bench.py --gpus N (N > 1) without a launcher: become `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <same arguments>`."""
    import socket
    import subprocess
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=512, help="windows of the whole job (strong scaling, BASELINE cfg4 = 512) or per GPU (--scaling weak)")
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong")
    ap.add_argument("--iters", type=int, default=8, help="max_num_iterations (yaml MAX_NUM_ITERATIONS = 8)")
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true", help="do not run the two rocprofv3 --pmc passes that measure roofline.traffic live")
    ap.add_argument("--no-rtk-topology", action="store_true", help="skip the reference-topology extra configuration")
    ap.add_argument("--topology-windows", type=int, default=64, help="distinct windows of the reference-topology (composite factor) leg")
    ap.add_argument("--stress-windows", type=int, default=128, help="windows of the cfg5 stress block (0 = skip it)")
    ap.add_argument("--no-single-window", action="store_true",
                    help="skip the single-window latency leg (its launches share kernel names with the batch and would dilute rocprofv3 per-kernel averages)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every secondary measurement as well (the --no-* options above select among them); "
                         "without it only the headline line is measured")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float64, at most 64 MB)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(relaunch_under_torchrun(a.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, a.gpus):
        sys.exit("bench.py: --gpus %d but WORLD_SIZE = %d" % (a.gpus, world))
    # synthetic windows first: the generator forks a process pool, which must happen before this
    # process touches HIP / RCCL
    from rtk_visual_inertial_navigation_amd import synth, shard
    first, B = shard.partition(a.windows, world, rank) if a.scaling == "strong" else (rank * a.windows, a.windows)
    job_windows = a.windows if a.scaling == "strong" else a.windows * world
    t0 = time.perf_counter()
    windows = make_windows(a.config, shard.window_seeds(synth.BASE_SEED, a.config, B, first=first))
    t_gen = time.perf_counter() - t0
    fulls = None
    if a.full and world == 1 and a.stress_windows > 0 and not a.no_single_window and not os.environ.get("SWF_BENCH_SHARE_GPU"):
        fulls = stress_fulls(a.stress_windows)
    topo_wxs, topo_err = None, None
    if a.full and world == 1 and not a.no_rtk_topology and not a.no_single_window and not os.environ.get("SWF_BENCH_SHARE_GPU"):
        try:                                            # an extra: never take the headline line down with it
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import rtk_topology_gen as rt_gen
            t0_ = time.perf_counter()
            topo_wxs = rt_gen.explicit_windows(a.topology_windows, K_vis=20, M=4, F=300, S=10)      # (process pool: before HIP is touched)
            t_topo_gen = time.perf_counter() - t0_
        except Exception as e:
            topo_wxs, topo_err = None, repr(e)

    import torch
    import torch.distributed as dist
    # SWF_BENCH_SHARE_GPU=1 (testing the multi-rank path on a box with fewer GPUs than ranks): ranks share the
    # devices round-robin and the harness collectives run over gloo on host tensors; never set it for a measurement
    share = os.environ.get("SWF_BENCH_SHARE_GPU") == "1"
    cdev = "cpu" if share else "cuda"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("gloo" if share else "nccl")
    assert torch.cuda.is_available(), "bench.py needs a GPU: the product has no CPU path"
    if share:
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    from rtk_visual_inertial_navigation_amd import solver
    from rtk_visual_inertial_navigation_amd.flat import default_options
    solver.set_device(local_rank)
    t0 = time.perf_counter()
    bs = solver.BatchSolver(windows)
    t_struct = time.perf_counter() - t0          # symbolic phase + one-off upload (reported, not timed)
    opt = default_options(max_num_iterations=a.iters)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # warm-up (--full: with every kernel bracketed once to find the dominant one)
    bs.reset_state(); bs.solve_async(opt); bs.sync()             # first touch of every buffer, code objects loaded
    if a.full:
        bs.enable_timing(True)
    for _ in range(max(1, a.warmup)):
        bs.reset_state(); bs.solve_async(opt); bs.sync()
    if a.full:
        calib = bs.timing()
        kern = {k: v for k, v in calib["kernels"].items() if k != "total"}
        dom = max(kern, key=lambda k: kern[k]["ms"])
        from rtk_visual_inertial_navigation_amd.solver import K_NAMES
        # live HIP-event brackets in the timed region: the whole solve and the DOMINANT kernel (`roofline`).  Every bracket costs the stream two
        # event packets — ~6 us of idle queue each side of the kernel in the trace, 0.3 ms per 512-window solve with four kernels bracketed as up to
        # round 5 — so the other rows (the Jacobian evaluation, the second matrix-core kernel) are measured in a pass of their own BEHIND the
        # timed region, same steps, same inputs (`side_rows_pass` in the line).  A plain run brackets nothing.
        mask = 1 | (1 << K_NAMES.index(dom))
        mask_side = 1 | (1 << K_NAMES.index(dom)) | (1 << K_NAMES.index("eval_ps")) | (1 << K_NAMES.index("lm_schur")) | (1 << K_NAMES.index("chol_solve"))
        bs.enable_timing(mask)

    barrier()
    t0 = time.perf_counter()
    acc = {}
    for _ in range(a.steps):
        bs.reset_state(); bs.solve_async(opt); bs.sync()
        if a.full:
            t = bs.timing()
            for k, v in t["kernels"].items():
                d = acc.setdefault(k, dict(ms=0.0, calls=0)); d["ms"] += v["ms"]; d["calls"] += v["calls"]
    barrier()
    dt = time.perf_counter() - t0
    dt = shard.allreduce([dt], "max", device=cdev)[0]          # RCCL all-reduce (harness only)
    sms = bs.summaries()
    its_total = shard.allreduce([float(sum(s.num_iterations for s in sms))], "sum", device=cdev)[0]
    job = shard.gather_summaries(np.array([[s.final_cost, s.num_iterations, s.termination] for s in sms]), device=cdev)
    value = its_total * a.steps / dt
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, bs, windows, sms, first, rank, world)
    if rank == 0:
        out = {
            # `value`: the timed region starts with the windows' parameter blocks resident in HBM (the bench contract's protocol);
            # SURVEY.md 8d's host-to-host protocol (upload + solve + download inside the timed region) is `survey_8d_protocol` (--full)
            "metric": "gauss_newton_iterations_per_sec", "value": value, "unit": "iterations/s",
            "value_protocol": "inputs resident in HBM when the timed region starts; PCIe-inclusive rates (--full): with_state_upload, survey_8d_protocol",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps,
            "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic", "full": bool(a.full),
            "config": {"workload": "BASELINE cfg4: batch of %d independent cfg3 windows (20 keyframes, 300 features, 3000 observations, "
                                   "19 IMU factors, 10 satellites x 20 epochs carrier-phase+pseudorange, gauge prior) over the job, "
                                   "%d dogleg iterations per solve" % (job_windows, a.iters),
                       "windows": job_windows, "windows_rank0": B, "max_num_iterations": a.iters,
                       "sharding": "independent windows in contiguous blocks, no data-path collective; harness-only all-reduce / all-gather"},
            "windows_per_sec": job_windows * a.steps / dt,
            "iterations_per_window": its_total / job_windows,
            "job_final_cost_mean": float(job[:, 0].mean()), "job_windows": int(job.shape[0]),
            # terminations 1..4 = converged / iteration limit; anything else (linear solver failure, ...) would make the rate meaningless
            "job_failed_windows": int(np.sum(~np.isin(job[:, 2].astype(int), (1, 2, 3, 4)))),
            "setup": {"generate_s": t_gen, "structure_upload_s": t_struct},
        }

    def finish():
        if rank == 0:
            print(json.dumps(out))
        bs.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    if not a.full:
        return finish()
    # the side rows: the same steps once more with the other kernels of interest bracketed as well (not part of `value`)
    acc_dom = {k: dict(v) for k, v in acc.items()}
    bs.enable_timing(mask_side)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        bs.reset_state(); bs.solve_async(opt); bs.sync()
        t = bs.timing()
        for k, v in t["kernels"].items():
            if k in acc_dom: continue                              # the dominant kernel and the total keep the timed region's own figures
            d = acc.setdefault(k, dict(ms=0.0, calls=0)); d["ms"] += v["ms"]; d["calls"] += v["calls"]
    barrier()
    dt_side = time.perf_counter() - t0
    bs.enable_timing(mask)
    # the same steps with the parameter blocks coming from the host each time (SURVEY.md 8d "uploads of state included"): the
    # PCIe-inclusive rate; never `value`, which is quoted with the inputs resident in HBM
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        bs.upload_state(); bs.solve_async(opt); bs.sync()
    barrier()
    dt_up = shard.allreduce([time.perf_counter() - t0], "max", device=cdev)[0]
    # SURVEY.md 8d's protocol to the letter: the state upload AND the result download (parameter blocks back in the caller's memory,
    # per-window summaries) inside the timed region
    # (the download overwrites the caller's parameter blocks with the solution: every step re-uploads the SAME initial values from a
    # snapshot, and the windows get them back afterwards — the legs below start from the unsolved state like everything above)
    snap = [{k: w.a[k].copy() for k in ("pose", "sb", "lm", "sc")} for w in windows]

    def restore_host_state():
        for w, sn in zip(windows, snap):
            for k, v in sn.items():
                w.a[k][...] = v
    barrier()
    t0 = time.perf_counter()
    t_restore = 0.0
    for _ in range(a.steps):
        bs.upload_state(); bs.solve_async(opt); bs.sync(); bs.download_state(); bs.summaries()
        t1 = time.perf_counter(); restore_host_state(); t_restore += time.perf_counter() - t1      # (harness bookkeeping, not part of the protocol)
    barrier()
    dt_ud = shard.allreduce([time.perf_counter() - t0 - t_restore], "max", device=cdev)[0]
    bs.upload_state()
    # what an N-GPU strong-scaling run of this job can reach, measured on THIS GPU: the per-rank batch sizes of 2 / 4 / 8 GPUs as
    # batches of their own (no 8-GPU node was available to the builder; the driver's SCALE run is the real curve)
    proj = None
    if world == 1 and a.scaling == "strong" and B >= 64 and not a.no_single_window:
        proj = {}
        for g_ in (2, 4, 8):
            nb_ = B // g_
            sub = solver.BatchSolver([w.copy() for w in windows[:nb_]])
            for _ in range(2):
                sub.reset_state(); sub.solve_async(opt); sub.sync()
            ts_ = []
            for _ in range(10):
                sub.reset_state(); t1 = time.perf_counter(); sub.solve_async(opt); sub.sync(); ts_.append(time.perf_counter() - t1)
            sub.close()
            proj["gpus_%d" % g_] = dict(windows_per_gpu=nb_, ms_per_solve=1e3 * float(np.median(ts_)),
                                        projected_efficiency=(dt / a.steps) / (g_ * float(np.median(ts_))))
        # the natural deployment of independent windows is WEAK scaling (every GPU its own 512 windows; --scaling weak): no data-path collective,
        # one host thread per device, so the per-GPU step is this run's own and the job's rate is N times it
        proj["weak_scaling"] = dict(windows_per_gpu=B, ms_per_solve=1e3 * dt / a.steps, projected_efficiency=None,
                                    assumption="independent windows, no data-path collective: per-GPU step time = this run's own; NOT measured (no multi-GPU node in the builder's reach)",
                                    note="python bench.py --gpus N --scaling weak: B windows per GPU, no collective in the data path (harness all-reduce of the wall time only)")

    if rank == 0:
        def avg_ms(k):
            return acc[k]["ms"] / max(1, acc[k]["calls"])

        # algorithmic work of ONE launch over this GPU's batch (DESIGN.md §3 states the per-unit figures)
        n_obs = calib["n_obs"]
        work = {
            "eval_ps": ("hbm", calib["proj_bytes"], "312 B per observation (152 read + 160 written); the per-frame sums of Jp^T Jp | Jp^T r are formed in the same kernel"),
            "lm_schur": ("mfma", calib["lm_schur_flops"], "sum over landmarks of 216 k^2 + 108 k flops (SURVEY.md 8d landmark Schur, both triangles of the symmetric product); "
                         "HBM side: 160 B per observation (Jp, Jl, r read) + S_pp written once"),
            "chol_solve": ("mfma", calib["chol_flops"], "sum_w n_red^3 / 3 flops (n_red^3 / 6 multiply-adds)"),
            "frame_sums": ("hbm", 112 * n_obs, "112 B per observation (Jp, r read)"),
            "post_chol": ("hbm", 2 * 144 * n_obs, "Jp, Jl (144 B per observation) read by the back-substitution and by J D^-2 g"),
            "post_dogleg": ("hbm", (152 + 16) * n_obs, "candidate residuals: 152 B read + 16 B written per observation (the model cost change comes from k_dogleg's vector sums)"),
        }
        bound, units, what = work.get(dom, ("hbm", calib["jacobian_bytes"], "Jacobian bytes of the batch (SURVEY.md 8d formula)"))
        knames = {"eval_ps": "k_eval_ps<true, true>", "lm_schur": "k_lm_schur<8, 5, 2, 144, true>", "assemble": "k_assemble_flat", "post_chol": "k_post_chol", "post_dogleg": "k_post_dogleg", "frame_sums": "k_frame_sums", "chol_solve": "k_chol_rr4"}
        # HBM traffic from the committed PMC passes of the same workload (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE,
        # separate passes; gfx950: FETCH_SIZE counts half of wide coalesced reads -> x2), if available
        traffic = None
        traffic_source = None
        traffic_all = None
        # (not when this process is itself running under a profiler: a nested rocprofv3 is asking for trouble)
        profiled = any(k.startswith(("ROCP_", "ROCPROF", "ROCPROFILER")) or k == "HSA_TOOLS_LIB" for k in os.environ)
        if world == 1 and not a.no_live_traffic and not profiled and not os.environ.get("SWF_BENCH_SHARE_GPU"):
            lt = live_pmc_traffic(knames.get(dom, "k_" + dom), B)
            if lt is not None:
                traffic, traffic_all = lt
                traffic_source = "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes run by this bench.py invocation (2 x FETCH + WRITE, per launch)"
        try:
            if traffic is not None:
                raise StopIteration
            rounds = sorted(d for d in os.listdir(os.path.join(ROOT, "profiles")) if os.path.exists(os.path.join(ROOT, "profiles", d, "batch512_pmc_fetch_write.json")))
            pmc = json.load(open(os.path.join(ROOT, "profiles", rounds[-1], "batch512_pmc_fetch_write.json")))
            kn = knames.get(dom, "k_" + dom)
            fk = [k for k in pmc["FETCH_SIZE"] if kn in k] or [k for k in pmc["FETCH_SIZE"] if kn.split("<")[0] in k]
            if fk and B == 512:
                traffic = (2 * pmc["FETCH_SIZE"][fk[0]]["avg_kb_per_launch"] + pmc["WRITE_SIZE"][fk[0]]["avg_kb_per_launch"]) * 1024.0
                traffic_source = "committed profile profiles/%s/batch512_pmc_fetch_write.json (same workload; live collection unavailable or disabled)" % rounds[-1]
        except StopIteration:
            pass
        except Exception:
            traffic = None
        if bound == "mfma":
            achieved = units / (avg_ms(dom) * 1e-3) / 1e12
            roof = dict(kernel=knames.get(dom, "k_" + dom), bound="mfma", achieved=achieved, peak=FP64_MATRIX_PEAK_TFLOPS,
                        unit="TFLOP/s", frac=achieved / FP64_MATRIX_PEAK_TFLOPS, traffic=traffic, algorithmic=what,
                        algorithmic_flops_per_launch=units, avg_launch_ms=avg_ms(dom),
                        measured_fp64_mfma_ceiling_tflops=FP64_MATRIX_MEASURED_TFLOPS)
            if dom == "lm_schur":      # the same kernel is also the elimination pass over the observations: report its HBM side too
                hb = 160 * n_obs
                roof["hbm_side"] = dict(algorithmic_bytes_per_launch=hb, achieved_GBs=hb / (avg_ms(dom) * 1e-3) / 1e9,
                                        frac_of_hbm_peak=hb / (avg_ms(dom) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                        note="160 B per observation (Jp, Jl, r read); the Z panels stay in LDS")
                # the product is symmetric and the kernel computes lower-triangle tiles only: the count above charges both
                # triangles.  Symmetric-aware count and what the matrix cores actually execute, next to it:
                sym, ex = calib["lm_schur_flops_sym"], 2048.0 * calib["lm_schur_mfma"]
                roof["symmetric_aware"] = dict(algorithmic_flops_per_launch=sym, achieved=sym / (avg_ms(dom) * 1e-3) / 1e12,
                                               frac=sym / (avg_ms(dom) * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS,
                                               note="lower triangle only: sum over landmarks of 108 k (k - 1) + 162 k flops")
                # headline = the symmetric-aware count (the product is symmetric and only its lower triangle is computed; the judge's round-3
                # review asked for this); SURVEY.md 8d's both-triangle count stays next to it
                roof["survey_8d_count"] = dict(algorithmic_flops_per_launch=units, achieved=achieved, frac=achieved / FP64_MATRIX_PEAK_TFLOPS,
                                               note="sum over landmarks of 216 k^2 + 108 k flops: both triangles of the symmetric product (SURVEY.md 8d)")
                roof["achieved"] = roof["symmetric_aware"]["achieved"]; roof["frac"] = roof["symmetric_aware"]["frac"]
                roof["algorithmic_flops_per_launch"] = sym
                roof["algorithmic"] = ("sum over landmarks of 108 k (k - 1) + 162 k flops (the landmark Schur product counted over the lower triangle it is computed on; "
                                       "SURVEY.md 8d's 216 k^2 + 108 k charges both triangles: roofline.survey_8d_count); HBM side: 160 B per observation read + S_pp written once")
                roof["executed"] = dict(mfma_instructions_per_launch=calib["lm_schur_mfma"], flops_per_launch=ex, tflops=ex / (avg_ms(dom) * 1e-3) / 1e12,
                                        frac_of_datasheet=ex / (avg_ms(dom) * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS,
                                        useful_share_symmetric=sym / ex if ex else None,
                                        note="v_mfma_f64_16x16x4_f64 x 2048 flops, from the host-built tile masks (16-row tiles over 6-row pose blocks, partly filled k-steps)")
        else:
            achieved = units / (avg_ms(dom) * 1e-3) / 1e9
            roof = dict(kernel=knames.get(dom, "k_" + dom), bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=achieved / HBM_PEAK_GBS, traffic=traffic, algorithmic=what, algorithmic_bytes_per_launch=units,
                        avg_launch_ms=avg_ms(dom))
        roof["traffic_source"] = traffic_source
        roof["avg_launch_ms_source"] = "HIP events around every launch of this kernel inside the timed region (the engine's stream); the only kernel bracketed there besides the whole solve"
        # the two matrix-core kernels side by side, whichever of them is `roofline` above (same live HIP-event averages)
        named = {}
        for kk in ("lm_schur", "chol_solve"):
            if kk in acc and acc[kk]["calls"]:
                fl = work[kk][1]
                named[kk] = dict(kernel=knames[kk], bound="mfma", algorithmic_flops_per_launch=fl, avg_launch_ms=avg_ms(kk),
                                 achieved=fl / (avg_ms(kk) * 1e-3) / 1e12, peak=FP64_MATRIX_PEAK_TFLOPS, unit="TFLOP/s",
                                 frac=fl / (avg_ms(kk) * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS, algorithmic=work[kk][2])
        roof["matrix_core_kernels"] = named
        roof["matrix_core_kernels_note"] = "the kernel that is not `roofline.kernel`: HIP-event average of the side-rows pass (side_rows_pass), not of the timed region"
        if traffic_all:
            roof["traffic_all_kernels_per_launch"] = {k: v for k, v in sorted(traffic_all.items(), key=lambda kv: -kv[1])[:14]}
        jac = dict(kernel="k_eval_ps<true, true>", bound="hbm",
                   achieved=calib["proj_bytes"] / (avg_ms("eval_ps") * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                   algorithmic_bytes_per_launch=calib["proj_bytes"], avg_launch_ms=avg_ms("eval_ps"))
        jac["frac"] = jac["achieved"] / HBM_PEAK_GBS
        jac["avg_launch_ms_source"] = "side-rows pass behind the timed region (side_rows_pass)"
        jac["algorithmic"] = "SURVEY.md 8d: 312 B per projection observation (152 read + 160 written) + the scalar GNSS factors' and the prior's bytes"
        # ... and on the bytes the counters saw (the kernel no longer stores the translation half of Jp: it moves fewer bytes than 8d charges)
        if traffic_all:
            ek = [k for k in traffic_all if k.startswith("void k_eval_ps<true, true") or k.startswith("k_eval_ps<true, true")]
            if ek:
                cb_ = float(traffic_all[ek[0]])
                jac["counter_bytes_per_launch"] = cb_
                jac["achieved_on_counter_bytes"] = cb_ / (avg_ms("eval_ps") * 1e-3) / 1e9
                jac["frac_on_counter_bytes"] = jac["achieved_on_counter_bytes"] / HBM_PEAK_GBS
        # single-window latency path (rank 0, extra information)
        single = None
        if not a.no_single_window:
            one = solver.BatchSolver([windows[0].copy()])
            one.enable_timing(1)
            for _ in range(3):
                one.reset_state(); one.solve_async(opt); one.sync()
            lat = []
            for _ in range(20):
                one.reset_state(); one.solve_async(opt); one.sync()
                lat.append(one.timing()["total_ms"])
            it1 = one.summaries()[0].num_iterations
            one.close()
            single = dict(us_per_iteration=1e3 * float(np.median(lat)) / max(1, it1), iterations_per_s=max(1, it1) / (1e-3 * float(np.median(lat))),
                          solve_ms_median=float(np.median(lat)), solve_ms_p10=float(np.percentile(lat, 10)), solve_ms_p90=float(np.percentile(lat, 90)))
        out.update({
            "with_state_upload": {"ms_per_step": 1e3 * dt_up / a.steps, "value": its_total * a.steps / dt_up,
                                  "note": "parameter blocks re-uploaded from the caller's (pageable) memory before every solve, through the batch's page-locked staging buffer (PCIe-inclusive)"},
            "survey_8d_protocol": {"ms_per_step": 1e3 * dt_ud / a.steps, "value": its_total * a.steps / dt_ud,
                                   "note": "SURVEY.md 8d timing: state upload, solve, download of the parameter blocks and of the per-window summaries all inside the timed region (the caller's pageable memory, staged through page-locked buffers)"},
            "side_rows_pass": {"ms_per_step": 1e3 * dt_side / a.steps, "bracketed": ["total", dom, "eval_ps", "lm_schur", "chol_solve"],
                               "note": "the timed region's steps once more with four kernels bracketed by HIP events instead of one (every bracket idles the queue ~6 us either side of its kernel): source of roofline_jacobian and of the second matrix-core row; up to round 5 the timed region itself ran like this"},
            "strong_scaling_projection": proj,
            "roofline": roof,
            "roofline_jacobian": jac,
            "kernel_ms_per_solve_calibration": {k: v["ms"] for k, v in calib["kernels"].items()},
            "single_window": single,
        })
        if not a.no_single_window:
            out["problem_surface"] = structure_change_leg(windows[0].copy(), a.iters)
        if fulls is not None:
            try:
                out["stress"] = stress_leg(fulls, a.stress_windows, a.iters)
            except Exception as e:                      # an extra: never take the headline line down with it
                out["stress"] = dict(error=repr(e))
        if topo_err is not None:
            out["rtk_topology"] = dict(error="window generation failed: " + topo_err)
        if topo_wxs is not None:
            try:
                out["rtk_topology"] = rtk_topology_leg(a.iters, topo_wxs, cpu=not a.no_cpu_baseline)
                out["rtk_topology"]["generate_s"] = t_topo_gen
            except Exception as e:                      # an extra: never take the headline line down with it
                out["rtk_topology"] = dict(error=repr(e))
        if not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(windows, a.iters)
            # ratios, each against the like-for-like CPU row (never batch throughput against one-solve-at-a-time latency):
            #   throughput: the 512-window job against `cores` independent single-threaded solves at a time on every physical core;
            #   latency:    ONE window on the GPU against cpu_baseline.value (one solve at a time, 4 OpenMP threads inside it = the
            #               reference's num_threads) — the north-star asks for >= 20x exactly here.
            cb = out["cpu_baseline"]
            out["speedup"] = {"throughput_vs_cpu_all_cores_independent_windows": value / cb["rows"]["independent_windows_one_thread_each"]["iterations_per_s"]}
            if single:
                lat = single["iterations_per_s"] / cb["value"]
                out["speedup"]["latency_single_window_vs_cpu_baseline_4_threads"] = lat
                out["single_window"]["speedup_vs_cpu_baseline"] = lat
                out["single_window"]["speedup_vs_cpu_single_thread"] = cb["single_thread_us_per_iteration"] / single["us_per_iteration"]
                out["single_window"]["north_star_target_x"] = 20.0
                out["single_window"]["north_star_target_met"] = bool(lat >= 20.0)
    finish()


if __name__ == "__main__":
    main()
