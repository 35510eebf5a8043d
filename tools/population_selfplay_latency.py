#!/usr/bin/env python3
"""Per-step latency of population device self-play (run.PopulationSelfPlay: K nets x T games, one search launch and one self-play
launch per step) against the same games as K single-net DeviceSelfPlay engines stepped one after another, and the weight sync of
K nets: K host uploads against one set_population_policies (one torch.cat per net, one gather launch).
GPU box only:  python tools/population_selfplay_latency.py [--ks 1,8,32,128,256] [--ts 1,16] [--steps 50] [--warmup 5]
Configurations as tools/population_latency.py: Pendulum-v0, 3x128 ELU GMM-2 policy, 25 rollouts; CartPole-v0, 2x128 ReLU, 8
rollouts, epsilon 0.1.  Per (K, T): wall ms per step (host clock around --steps asynchronous steps ended by one sync, after
--warmup steps), the search kernel's ms (azg_last_search_ms, median over synchronised steps), wall ms per step of the K single
engines, and the weight sync ms (medians over --sync-reps).  The policies live on the GPU; the ring runs in FIFO mode."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_gym_amd import run  # noqa: E402
from alphazero_gym_amd.envs import make_game  # noqa: E402

CONFIGS = {
    "pendulum_3x128_gmm2_25": ("continuous", dict(game="Pendulum-v0", policy=dict(num_components=2))),
    "cartpole_2x128_8": ("discrete", dict(game="CartPole-v0")),
}


def _wall_per_step(step_all, sync_all, steps, warmup):
    for _ in range(warmup):
        step_all()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        step_all()
    sync_all()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(kind, over, K, T, steps, warmup, sync_reps):
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, over)
    torch.manual_seed(0)
    env = make_game(cfg["game"])
    cpu = [run.make_agent(kind, cfg, env, tree_id_base=k).nn for k in range(K)]
    gpu = [copy.deepcopy(p).to("cuda:0") for p in cpu]
    m = cfg["mcts"]
    kw = dict(game=cfg["game"], n_rollouts=m["n_rollouts"], c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"],
              c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5), max_episode_length=cfg["max_episode_length"], capacity_steps=64,
              fifo=True)
    pop = run.PopulationSelfPlay(gpu, games_per_net=T, **kw)
    e = pop.engine
    wall_pop = _wall_per_step(e.selfplay_step, e.sync, steps, warmup)
    kern = []
    for _ in range(10):
        e.selfplay_step()
        e.sync()
        kern.append(e.last_search_ms())
    info = e.search_info()
    host, dev = [], []
    for _ in range(sync_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, p in enumerate(cpu):
            e.set_net_policy(k, p)
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.set_population_policies(gpu)
        dev.append((time.perf_counter() - t0) * 1e3)
    pop.close()
    singles = [run.DeviceSelfPlay(p, n_games=T, rank=k, **kw) for k, p in enumerate(gpu)]

    def step_singles():
        for s in singles:
            s.engine.selfplay_step()

    def sync_singles():
        for s in singles:
            s.engine.sync()

    wall_seq = _wall_per_step(step_singles, sync_singles, steps, warmup)
    for s in singles:
        s.engine.close()
    med = lambda x: float(np.median(x))   # noqa: E731
    return dict(K=K, T=T, wall_ms_population_step=round(wall_pop, 3), search_kernel_ms=round(med(kern), 4),
                wall_ms_singles_step=round(wall_seq, 3), speedup_wall=round(wall_seq / wall_pop, 2),
                sync_ms_host_uploads=round(med(host), 3), sync_ms_population_device=round(med(dev), 3),
                kernel=info["kernel_name"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="1,8,32,128,256")
    ap.add_argument("--ts", default="1,16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sync-reps", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    os.environ.setdefault("AZG_QUIET", "1")
    for name in a.configs.split(","):
        kind, over = CONFIGS[name]
        print(f"# {name}: wall ms per step over {a.steps} steps (after {a.warmup} warm-up steps); kernel and sync ms: medians")
        print(f"# {'K':>4} {'T':>3} {'pop step ms':>12} {'search kernel ms':>17} {'K singles step ms':>18} {'speed-up':>9} "
              f"{'sync ms: K host uploads':>24} {'one device call':>16}")
        for T in [int(t) for t in a.ts.split(",")]:
            for K in [int(k) for k in a.ks.split(",")]:
                r = measure(kind, over, K, T, a.steps, a.warmup, a.sync_reps)
                print(f"  {K:4d} {T:3d} {r['wall_ms_population_step']:12.3f} {r['search_kernel_ms']:17.4f} {r['wall_ms_singles_step']:18.3f} "
                      f"{r['speedup_wall']:8.2f}x {r['sync_ms_host_uploads']:24.3f} {r['sync_ms_population_device']:16.3f}")
                print(json.dumps(dict(config=name, **r)), flush=True)


if __name__ == "__main__":
    main()
