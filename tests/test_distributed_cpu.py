"""world_size-2 gloo test of the N>1 path on CPU: disjoint window shards, harness collectives,
and that the gathered per-window records equal what one process computes for the whole job.
(The per-window solves here run through the CPU oracle — test infrastructure — because there is
no GPU in this container; on the GPU box the same sharding code drives libswf_hip.so.)"""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, B, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from rtk_visual_inertial_navigation_amd import synth, shard
    from rtk_visual_inertial_navigation_amd.flat import default_options
    import oracle_binding as ob
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seeds = shard.window_seeds(synth.BASE_SEED, 4, B, rank)
    recs = []
    for s in seeds:
        w = synth.make_window(3, K=4, F=8, S=5, seed=s)
        sm, _ = ob.solve(w, default_options(max_num_iterations=4), export=False)
        recs.append([sm.final_cost, sm.num_iterations, sm.termination])
    allr = shard.gather_summaries(np.array(recs))
    tmax = shard.allreduce([1.0 + rank], "max")[0]
    isum = shard.allreduce([sum(r[1] for r in recs)], "sum")[0]
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.concatenate([allr.ravel(), [tmax, isum], seeds]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_and_gather(tmp_path):
    import torch.multiprocessing as mp
    world, B = 2, 3
    port = _free_port()
    mp.spawn(_worker, args=(world, port, B, str(tmp_path)), nprocs=world, join=True)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from rtk_visual_inertial_navigation_amd import synth, shard
    from rtk_visual_inertial_navigation_amd.flat import default_options
    import oracle_binding as ob
    r0 = np.load(os.path.join(str(tmp_path), "rank0.npy")); r1 = np.load(os.path.join(str(tmp_path), "rank1.npy"))
    n = world * B * 3
    assert np.array_equal(r0[:n + 2], r1[:n + 2])                     # every rank sees the same gathered job
    s0, s1 = r0[n + 2:], r1[n + 2:]
    assert len(set(s0) | set(s1)) == world * B and not (set(s0) & set(s1))   # disjoint shards
    assert r0[n] == 2.0                                               # max over ranks of (1 + rank)
    # single-process reference for the whole job, same seeds in job order
    exp = []
    for rank in range(world):
        for s in shard.window_seeds(synth.BASE_SEED, 4, B, rank):
            w = synth.make_window(3, K=4, F=8, S=5, seed=s)
            sm, _ = ob.solve(w, default_options(max_num_iterations=4), export=False)
            exp.append([sm.final_cost, sm.num_iterations, sm.termination])
    exp = np.array(exp)
    assert np.array_equal(r0[:n].reshape(-1, 3), exp)                  # bit-identical: windows are independent
    assert r0[n + 1] == exp[:, 1].sum()


def test_strong_scaling_partition_covers_the_job_exactly():
    """512 windows over G in {1, 2, 4, 8} GPUs in contiguous blocks (64 per GPU at 8); uneven jobs give the first
    ranks one more; the seeds of the shards tile the job's seed range without gaps or overlaps."""
    from rtk_visual_inertial_navigation_amd import synth, shard
    for n, world in ((512, 1), (512, 2), (512, 4), (512, 8), (10, 4), (3, 8)):
        parts = [shard.partition(n, world, r) for r in range(world)]
        assert parts[0][0] == 0 and sum(c for _, c in parts) == n
        for (f0, c0), (f1, _) in zip(parts, parts[1:]):
            assert f1 == f0 + c0
        assert max(c for _, c in parts) - min(c for _, c in parts) <= 1
        # the C-ABI's in-process sharding (swf_batch_create_sharded) deals the windows by the same rule
        import ctypes
        from rtk_visual_inertial_navigation_amd import solver
        for r in range(world):
            f_, c_ = ctypes.c_int32(-1), ctypes.c_int32(-1)
            assert solver.lib().swf_shard_partition(ctypes.c_int32(n), ctypes.c_int32(world), ctypes.c_int32(r), ctypes.byref(f_), ctypes.byref(c_)) == 0
            assert (f_.value, c_.value) == parts[r]
        seeds = sum((shard.window_seeds(synth.BASE_SEED, 4, c, first=f) for f, c in parts), [])
        assert seeds == [synth.BASE_SEED + 4 + i for i in range(n)]
    assert shard.partition(512, 8, 7) == (448, 64)


def _run_bench(args, env_extra, timeout=900):
    import subprocess
    env = dict(os.environ); env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)


def test_bench_launches_its_own_ranks_and_fails_loudly_without_gpu():
    """`python bench.py --gpus 2` with no launcher around it re-executes itself under torch.distributed.run: both ranks come up
    (and, in this container, both refuse to run without a GPU — the product has no CPU path)."""
    from rtk_visual_inertial_navigation_amd import solver
    if solver.device_count() > 0:
        pytest.skip("a GPU is present (covered by the gpu test)")
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--windows", "4", "--no-cpu-baseline", "--no-single-window"],
                   {"SWF_BENCH_SHARE_GPU": "1"})
    assert r.returncode != 0
    assert r.stderr.count("bench.py needs a GPU") >= 2, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_two_ranks_sharing_one_gpu_reports_the_whole_job():
    """The driver's multi-GPU contract on a 1-GPU box: `python bench.py --gpus 2` (share mode: both ranks on device 0, harness
    collectives over gloo) prints ONE line with n_gpus = 2, strong scaling, and the gathered records of all windows."""
    import json
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--windows", "16", "--no-cpu-baseline", "--no-single-window"],
                   {"SWF_BENCH_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["windows"] == 16 and out["config"]["windows_rank0"] == 8
    assert out["job_windows"] == 16 and out["value"] > 0 and out["steps"] == 2
    # the same job on one rank: identical per-window results (windows are independent units), hence the same mean final cost
    r1 = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--windows", "16", "--no-cpu-baseline", "--no-single-window"], {})
    assert r1.returncode == 0, r1.stderr[-3000:]
    out1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][0])
    assert out1["n_gpus"] == 1 and out1["job_windows"] == 16
    assert out1["job_final_cost_mean"] == out["job_final_cost_mean"]


@pytest.mark.gpu
def test_bench_eight_ranks_sharing_one_gpu_reports_the_whole_job():
    """The 8-GPU launch shape the driver uses (`--gpus 8`: eight ranks, harness collectives, an UNEVEN strong partition — 20 windows as
    3+3+3+3+2+2+2+2) exercised end to end on a 1-GPU box in share mode: one line, n_gpus = 8, every window of the job gathered, and the
    same per-window results as the one-rank job."""
    import json
    args = ["--steps", "2", "--warmup", "1", "--windows", "20", "--no-cpu-baseline", "--no-single-window"]
    r = _run_bench(["--gpus", "8"] + args, {"SWF_BENCH_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["scaling"] == "strong" and out["config"]["windows"] == 20 and out["config"]["windows_rank0"] == 3
    assert out["job_windows"] == 20 and out["job_failed_windows"] == 0 and out["value"] > 0
    r1 = _run_bench(["--gpus", "1"] + args, {})
    assert r1.returncode == 0, r1.stderr[-3000:]
    out1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][0])
    assert out1["job_windows"] == 20 and out1["job_final_cost_mean"] == out["job_final_cost_mean"]


@pytest.mark.gpu
def test_bench_dumps_the_timed_steps_outputs_in_plain_and_full_runs(tmp_path):
    """--dump-outputs DIR: the last timed step's solved blocks and per-window summaries as float64 .npy files.  The same arguments give
    the same inputs, so a plain run and a --full run (whose secondary legs come after the dump) write identical arrays; only --full
    carries the secondary rows."""
    import json
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--windows", "16", "--no-cpu-baseline", "--no-live-traffic",
            "--no-rtk-topology", "--stress-windows", "0"]
    outs, dumps = [], []
    for extra in ([], ["--full"]):
        d = tmp_path / ("full" if extra else "plain")
        r = _run_bench(args + extra + ["--dump-outputs", str(d)], {})
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        outs.append(json.loads(lines[0]))
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    plain, full = outs
    for o in outs:
        assert o["steps"] == 2 and o["ms_per_step"] > 0 and o["value"] > 0 and o["job_windows"] == 16 and o["job_failed_windows"] == 0
    assert "roofline" not in plain and "with_state_upload" not in plain and "single_window" not in plain
    assert "roofline" in full and "with_state_upload" in full and full["single_window"] is not None
    assert plain["job_final_cost_mean"] == full["job_final_cost_mean"]
    names = {"pose", "sb", "lm", "sc", "initial_cost", "final_cost", "num_iterations", "termination", "window_index"}
    assert set(dumps[0]) == names and set(dumps[1]) == names
    assert sum(v.nbytes for v in dumps[0].values()) <= 64 << 20
    for k in names:
        assert dumps[0][k].dtype == np.float64
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k])
    np.testing.assert_array_equal(dumps[0]["window_index"], np.arange(16))
    assert dumps[0]["final_cost"].mean() == pytest.approx(plain["job_final_cost_mean"], rel=1e-14)
    assert dumps[0]["num_iterations"].sum() == plain["iterations_per_window"] * 16


def _uneven_worker(rank, world, port, total, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from rtk_visual_inertial_navigation_amd import shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    first, count = shard.partition(total, world, rank)
    recs = np.array([[100.0 + first + i, first + i, 4.0] for i in range(count)]).reshape(-1, 3)
    np.save(os.path.join(out_dir, "u%d.npy" % rank), shard.gather_summaries(recs))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_of_an_uneven_strong_partition_over_eight_ranks(tmp_path):
    """The 8-way partition of a job that does not divide (21 windows: 3+3+3+3+3+2+2+2): every rank gathers the job's windows in order."""
    import torch.multiprocessing as mp
    from rtk_visual_inertial_navigation_amd import shard
    world, total = 8, 21
    mp.spawn(_uneven_worker, args=(world, _free_port(), total, str(tmp_path)), nprocs=world, join=True)
    g = [np.load(os.path.join(str(tmp_path), "u%d.npy" % r)) for r in range(world)]
    assert all(np.array_equal(g[0], x) for x in g[1:])
    assert g[0].shape == (total, 3) and np.array_equal(g[0][:, 1], np.arange(total))
    counts = [shard.partition(total, world, r)[1] for r in range(world)]
    assert counts == [3, 3, 3, 3, 3, 2, 2, 2] and sum(counts) == total


def test_gather_of_an_uneven_strong_partition(tmp_path):
    """A job that does not divide evenly over the ranks (5 windows on 2 ranks: 3 + 2): the gathered records are the job's windows in order."""
    import torch.multiprocessing as mp
    world, total = 2, 5
    mp.spawn(_uneven_worker, args=(world, _free_port(), total, str(tmp_path)), nprocs=world, join=True)
    g0, g1 = (np.load(os.path.join(str(tmp_path), "u%d.npy" % r)) for r in range(world))
    assert g0.shape == (total, 3) and np.array_equal(g0, g1)
    assert np.array_equal(g0[:, 1], np.arange(total)) and np.array_equal(g0[:, 0], 100.0 + np.arange(total))
