#!/usr/bin/env python3
"""Per-act() latency of K agents at the reference defaults: one population step (AgentPopulation.act: all K trees in one launch)
against the same K agents stepped one by one (agent.act: one launch and three ABI round trips each).
GPU box only:  python tools/population_latency.py [--ks 1,3,8,32,128,256] [--steps 20] [--warmup 3]
Configurations: Pendulum-v0, 3x128 ELU GMM-2 policy, 25 rollouts (run_continuous.py with the reference's GMM); CartPole-v0, 2x128
ReLU, 8 rollouts, epsilon 0.1 (run_discrete.py).  Per K: kernel ms per launch (azg_last_search_ms; one-by-one: the mean of the K
single-tree launches, and their sum), wall ms per population step, wall ms of the K one-by-one act() calls, and the speed-up.
Every act searches from the same fresh root (reset_mcts before each step; the envs are not stepped)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_gym_amd import run  # noqa: E402
from alphazero_gym_amd.agent.population import AgentPopulation  # noqa: E402
from alphazero_gym_amd.envs import make_game  # noqa: E402
from alphazero_gym_amd.search.mcts import env_signature  # noqa: E402

CONFIGS = {
    "pendulum_3x128_gmm2_25": ("continuous", dict(game="Pendulum-v0", policy=dict(num_components=2))),
    "cartpole_2x128_8": ("discrete", dict(game="CartPole-v0")),
}


def measure(kind, over, K, steps, warmup):
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, over)
    torch.manual_seed(0)
    envs = []
    for k in range(K):
        env = make_game(cfg["game"])
        env.seed(34 + k)
        env.reset()
        envs.append(env)
    agents = [run.make_agent(kind, cfg, envs[k], tree_id_base=k) for k in range(K)]
    pop = AgentPopulation(agents, seeds=[34 + k for k in range(K)])

    def reset():
        for a in agents:
            a.reset_mcts(root_state=None)   # (return_results then takes the observation from the env)

    wall_pop, kern_pop = [], []
    for i in range(warmup + steps):
        reset()
        t0 = time.perf_counter()
        pop.act(envs)
        t1 = time.perf_counter()
        if i >= warmup:
            wall_pop.append((t1 - t0) * 1e3)
            kern_pop.append(pop.mcts.engine.last_search_ms())
    form = pop.mcts.last_search_info
    pop.close()
    wall_seq, kern_seq = [], []
    for i in range(warmup + steps):
        reset()
        ks = []
        t0 = time.perf_counter()
        for a, env in zip(agents, envs):
            a.act(env)
        t1 = time.perf_counter()
        for a, env in zip(agents, envs):
            ks.append(a.mcts._ensure_engine(env_signature(env)[0], 1).engine.last_search_ms())
        if i >= warmup:
            wall_seq.append((t1 - t0) * 1e3)
            kern_seq.append(ks)
    for a in agents:
        if a.mcts._batched is not None:
            a.mcts._batched.close()
    med = lambda x: float(np.median(x))   # noqa: E731
    ks = np.asarray(kern_seq)
    return dict(K=K, kernel_ms_population=round(med(kern_pop), 4), wall_ms_population_step=round(med(wall_pop), 3),
                kernel_ms_one_by_one_mean=round(float(np.median(ks.mean(1))), 4), kernel_ms_one_by_one_sum=round(float(np.median(ks.sum(1))), 3),
                wall_ms_one_by_one=round(med(wall_seq), 3), speedup_wall=round(med(wall_seq) / med(wall_pop), 2),
                kernel=form["kernel_name"], waves=form.get("waves"), tile_trees=form.get("tile_trees"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="1,3,8,32,128,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    os.environ.setdefault("AZG_QUIET", "1")
    for name in a.configs.split(","):
        kind, over = CONFIGS[name]
        print(f"# {name}: medians over {a.steps} steps (after {a.warmup} warm-up steps)")
        print(f"# {'K':>4} {'kernel ms':>10} {'pop step ms':>12} {'1-by-1 kernel ms (mean / sum)':>30} {'1-by-1 wall ms':>15} {'speed-up':>9}")
        for K in [int(k) for k in a.ks.split(",")]:
            r = measure(kind, over, K, a.steps, a.warmup)
            print(f"  {K:4d} {r['kernel_ms_population']:10.4f} {r['wall_ms_population_step']:12.3f} "
                  f"{r['kernel_ms_one_by_one_mean']:14.4f} / {r['kernel_ms_one_by_one_sum']:11.3f} {r['wall_ms_one_by_one']:15.3f} "
                  f"{r['speedup_wall']:8.2f}x")
            print(json.dumps(dict(config=name, **r)), flush=True)


if __name__ == "__main__":
    main()
