"""bench.py: the pieces that run without a GPU, and (-m gpu) its N > 1 loop end to end on one GPU (gloo, every rank on GPU 0)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_flop_and_core_counts():
    import bench
    assert bench.FLOP_PER_SIM == 134144                            # 2x256 Pendulum
    assert bench.mlp_flops(3, [1024] * 4, 3) == 6303744            # config E
    assert bench.mlp_flops(4, [128, 128], 3) == 34560              # config B, per evaluation
    assert 1 <= bench.physical_cores() <= (os.cpu_count() or 1)


def test_no_profiler_child_passes_under_a_profiler(monkeypatch):
    """bench.py's live PMC passes start rocprofv3 children; when bench.py itself already runs under rocprofv3 the
    tool library is preloaded into every child, and a nested rocprofv3 would re-exec a process whose GPU runtime is initialised.
    live_traffic() must refuse there, and the children's environment must carry nothing a profiler left behind."""
    import bench
    for var, val in (("ROCP_TOOL_LIBRARIES", "/opt/rocm/lib/librocprofiler-sdk-tool.so"), ("ROCPROF_COUNTER_COLLECTION", "1"),
                     ("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")):
        monkeypatch.setenv(var, val)
        assert bench.under_profiler()
        assert bench.live_traffic(16) == (None, "already under a profiler")
        env = bench.clean_child_env()
        assert "LD_PRELOAD" not in env and not [k for k in env if k.startswith("ROCP")] and env["TMPDIR"] == "/tmp"
        monkeypatch.delenv(var)
    assert not bench.under_profiler()


def test_walk_bytes_of_a_widening_search_are_counted_from_the_trees():
    """roofline_hbm of the headline line: L / C / E of SURVEY 8d's byte formula reconstructed from a searched batch (oracle double):
    the children scored are a function of every node's visit count under the widening law; the reconstruction must land on the
    survey's probe values (L 2.64, C 11.45, E 1.0 for 200 rollouts) and on an exact recount for a small case."""
    import bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle_lib as O
    from alphazero_gym_amd import _capi
    e = O.OracleEngine(n_trees=64, n_sims=200, **bench.PENDULUM)
    e.set_weights(_capi.make_desc(3, bench.HIDDEN, 2, "elu"), O.make_weights(34, 3, bench.HIDDEN, 2))
    e.search(e.synthetic_roots())
    per_sim, L, C, E = bench.tree_walk_bytes_continuous(e.dump_tree(), 200, 1.0, 0.5)
    e.close()
    assert E == 1.0 and 2.3 < L < 3.0 and 10.0 < C < 13.0 and 400 < per_sim < 520
    # every node's final child count must equal what the reconstruction's law gives for its visit count (the same walk the formula takes)
    d = None
    e = O.OracleEngine(n_trees=4, n_sims=60, **bench.PENDULUM)
    e.set_weights(_capi.make_desc(3, bench.HIDDEN, 2, "elu"), O.make_weights(34, 3, bench.HIDDEN, 2))
    e.search(e.synthetic_roots())
    d = e.dump_tree()
    e.close()
    import math
    for t in range(4):
        n = int(d["n_records"][t])
        kids = np.bincount(d["parent"][t][1:n], minlength=n)
        for j in range(n):
            K = 1 if j == 0 else 0
            for v in range(int(d["node_n"][t][j])):
                if math.ceil((v + 1) ** 0.5) > K:
                    K += 1
            assert K == kids[j], (t, j, K, kids[j])


def test_dump_outputs_keeps_dtypes_and_samples_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs' writer: float64 stays float64, every other dtype becomes float32; over the budget every array keeps a
    seeded sample of its rows in proportion (the same rows for arrays of the same length, the same rows from run to run)."""
    import numpy as np
    import bench
    arrays = {"Q": np.arange(4000, dtype=np.float64).reshape(1000, 4), "counts": np.arange(1000, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    q, c = np.load(tmp_path / "all" / "Q.npy"), np.load(tmp_path / "all" / "counts.npy")
    assert q.dtype == np.float64 and c.dtype == np.float32
    np.testing.assert_array_equal(q, arrays["Q"])
    np.testing.assert_array_equal(c, arrays["counts"])
    monkeypatch.setattr(bench, "DUMP_BYTES", 9000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    q, c = np.load(tmp_path / "a" / "Q.npy"), np.load(tmp_path / "a" / "counts.npy")
    assert q.nbytes + c.nbytes <= 9000 and q.shape[0] == c.shape[0] > 0
    np.testing.assert_array_equal(q[:, 0] / 4, c)                  # the same rows of both arrays, in order
    assert len(set(c.tolist())) == c.size and np.all(np.diff(c) > 0)
    for f in ("Q.npy", "counts.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env, capture_output=True, text=True)
    assert p.returncode != 0 and "does not match WORLD_SIZE" in (p.stderr + p.stdout)


def test_spawned_ranks_inherit_full(monkeypatch):
    """`bench.py --gpus N` without a launcher starts torch.distributed.run itself: its ranks run --full exactly when it was asked for."""
    import bench
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    for extra, want in (([], False), (["--full"], True)):
        cmds = []
        monkeypatch.setattr(bench.subprocess, "call", lambda cmd: cmds.append(cmd) or 0)
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"] + extra)
        with pytest.raises(SystemExit) as ex:
            bench.main()
        assert ex.value.code == 0 and len(cmds) == 1
        assert ("--full" in cmds[0]) == want, cmds[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 4])
def test_multi_rank_loop_on_one_gpu(ranks):
    """`python bench.py --gpus N` spawns its own ranks; config D's step (self-play step, all-gather of the step's rows, weight
    broadcast + engine re-sync) runs with gloo and every rank on GPU 0: N = 2 and 4 -- four tree_id_base offsets, four engines
    on one device, a four-way gather, followed by the config E leg (4x1024 network, every rank its own shard of trees).  (Eight
    ranks would put nine processes on the one GPU, this test's own included: more than a shared device should carry.  The
    eight-way gather of the same code runs in tests/test_distributed.py over gloo on the CPU.)  With --full the N > 1 line carries the
    CPU baseline, a note about the traffic figure and every rank's host-side timings of the collectives (min /
    median / max over the ranks) with the world size each rank saw."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    trees = "512"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "5", "--warmup", "2", "--trees", trees,
                        "--bcast-every", "2", "--backend", "gloo", "--same-device", "--e-trees", "64", "--e-searches", "2", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == ranks and out["steps"] == 5 and out["scaling"] == "weak"
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] == "port"
    assert "traffic_note" in out["roofline"]
    assert out["value"] > 0 and out["extra"]["search_only"]["sims_per_s"] >= out["value"] * 0.5
    assert "config D" in out["config"]["workload"]
    c = out["extra"]["collectives"]
    assert c["world_size"] == ranks and c["world_size_seen"] == [ranks]
    pr = c["per_rank_ms"]
    assert pr["gathers_timed"] >= 1 and pr["bcasts_timed"] >= 1
    for k in ("gather_ms", "bcast_ms", "step_ms"):
        assert 0 < pr[k]["min"] <= pr[k]["median"] <= pr[k]["max"], (k, pr[k])
    # BASELINE.json configs[4] under N > 1: every rank searched its own shard of the 4x1024 network's trees
    # (64 here; ranks that share one GPU may see their team kernels fall back to the per-layer launches: reported, not an error)
    e = out["extra"]["config_e_nrank"]
    assert f"{ranks * 64} trees = 64 per GPU" in e["config"] and e["searches"] == 2
    assert e["sims_per_s"] > 0 and len(e["team_kernel_fallbacks_per_rank"]) == ranks
    km = e["kernel_ms_per_search"]
    assert 0 < km["min"] <= km["median"] <= km["max"]
    assert all(k.startswith(("ls_team_kernel", "lock-step", "ls_")) for k in e["kernels"]), e["kernels"]
    assert 0 < e["roofline"]["frac"] < 1


@pytest.mark.gpu
def test_a_dead_rank_fails_the_run_instead_of_hanging_it():
    """one of two ranks exits right after the rendezvous (AZG_BENCH_DIE_RANK, a test hook).  The survivor's
    collectives are bounded (--dist-timeout) and torch.distributed.run tears the job down: bench.py exits non-zero, well inside
    the test's own time limit, and prints no JSON line."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["AZG_BENCH_DIE_RANK"] = "1"
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--trees", "256",
                        "--backend", "gloo", "--same-device", "--dist-timeout", "30", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert time.time() - t0 < 300


def _bench_json(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("warmup", [3, 4])
def test_gathered_rows_are_the_previous_steps_rows(warmup):
    """The two-slot replay ring keeps turning across the warm-up, the timed loop and the collective-free loop; the slot that is
    all-gathered while step s searches must be the one step s - 1 wrote, whatever the parity of the warm-up (with an
    odd warm-up the loop used to gather the slot being overwritten).  --verify-gather finds the slot a step wrote by comparing
    the ring before and after it and checks every gathered block against it.  (Rows are gathered in blocks of --gather-every
    steps; the ring holds two blocks.)"""
    out = _bench_json(["--gpus", "2", "--steps", "5", "--warmup", str(warmup), "--trees", "256", "--bcast-every", "2", "--gather-every", "2",
                       "--backend", "gloo", "--same-device", "--verify-gather"])
    c = out["extra"]["collectives"]
    assert c["gathers_verified"] == c["gathers"] >= (warmup + 5 - 1) // 2   # a block of two finished steps per gather, across both runs


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_full_adds_the_rest():
    """A plain `bench.py --gpus 1` run sets up, warms up, times its steps and prints the headline line: no kernel-time pass, no
    roofline, no other run after the timed steps.  --full adds them (here without the profiler passes, the other configurations
    and the CPU baseline, whose own switches keep this test short): the rooflines from a kernel-time pass and the searched trees,
    the PCIe-inclusive rate and config D's step on this one GPU.  The headline fields are the same in both lines."""
    steps, warmup = 3, 1
    plain = _bench_json(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    assert plain["unit"] == "sims/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["n_gpus"] == 1 and plain["steps"] == steps and plain["warmup"] == warmup and "config C" in plain["config"]["workload"]
    sims = 4096 * 200
    assert plain["value"] > 0 and abs(plain["value"] * plain["ms_per_step"] * 1e-3 - sims) < 1e-6 * sims
    assert not {"roofline", "roofline_hbm", "cpu_baseline"} & set(plain) and plain["extra"] == {}
    full = _bench_json(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--full", "--no-extra", "--no-live-traffic",
                        "--no-cpu-baseline"])
    assert set(plain) < set(full) and {"roofline", "roofline_hbm"} <= set(full) and "cpu_baseline" not in full
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert full[k] == plain[k], k
    assert full["roofline"]["kernel_ms"] > 0 and 0 < full["roofline"]["frac"] < 1
    assert full["roofline"]["kernel"].startswith("search_kernel<2, 256"), full["roofline"]["kernel"]
    assert {"pcie_inclusive", "config_d_1rank"} <= set(full["extra"]) and "configs" not in full["extra"]


@pytest.mark.gpu
def test_dump_outputs_are_the_results_of_the_last_timed_search(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` writes return_results of the K-th timed search: search index W + K - 1
    of the headline engine (4096 synthetic fixed-seed roots), so an engine set to that index reproduces them bit for bit."""
    import numpy as np
    import bench
    import oracle_lib as O
    from alphazero_gym_amd import _capi, _native
    steps, warmup = 3, 2
    out = _bench_json(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-extra", "--no-cpu-baseline", "--no-live-traffic",
                       "--dump-outputs", str(tmp_path)])
    assert out["steps"] == steps and out["warmup"] == warmup
    e = _native.HipEngine(n_trees=bench.N_TREES, n_sims=bench.N_SIMS, **bench.PENDULUM)
    e.set_weights(_capi.make_desc(3, bench.HIDDEN, 2, "elu"), O.make_weights(34, 3, bench.HIDDEN, 2))
    e.set_search_index(warmup + steps - 1)
    e.search(e.synthetic_roots())
    want = e.results()
    e.close()
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == (np.float64 if v.dtype == np.float64 else np.float32), k
        np.testing.assert_array_equal(got, v.astype(got.dtype), err_msg=k)
    assert (np.load(tmp_path / "counts.npy").sum(1) == bench.N_SIMS).all()


@pytest.mark.gpu
def test_config_d_loop_over_rccl_with_one_rank(tmp_path):
    """The `nccl` branch on hardware: bench.py --config-d under torch.distributed.run with ONE rank -- all_gather_into_tensor on the
    engine-owned ring (the zero-copy view azg_selfplay_rows_device exports) and the weight broadcast into HBM followed by
    azg_set_weights_device go through RCCL with world size 1.  Proves RCCL accepts engine-owned memory and that the stream
    ordering between the engine's stream and RCCL's holds (every gathered block verified), before a multi-GPU node sees it.
    --dump-outputs: the replay rows of the last timed step and of the last all-gather, every row holding n_sims visits."""
    import numpy as np
    out = _bench_json(["--gpus", "1", "--config-d", "--steps", "6", "--warmup", "3", "--trees", "1024", "--bcast-every", "2", "--gather-every", "2",
                       "--backend", "nccl", "--verify-gather", "--dump-outputs", str(tmp_path)])
    rows, gathered = np.load(tmp_path / "replay_rows.npy"), np.load(tmp_path / "gathered_rows.npy")
    K = (rows.shape[1] - 4) // 3                                   # obs[3] | actions[K] | counts[K] | Q[K] | V
    assert rows.dtype == np.float32 and rows.shape == (1024, 4 + 3 * K) and gathered.shape == (2 * 1024, rows.shape[1])
    for r in (rows, gathered):
        assert (r[:, 3 + K:3 + 2 * K].sum(1) == 200).all()
    assert out["n_gpus"] == 1 and "config D" in out["config"]["workload"]
    c = out["extra"]["collectives"]
    assert c["backend"] == "nccl" and c["world_size"] == 1 and c["gathers_verified"] == c["gathers"] >= 4
    assert c["weight_sync"].startswith("device to device")
    assert out["value"] > 0
