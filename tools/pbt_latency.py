#!/usr/bin/env python3
"""What a population-based-training step costs: ms per PopulationBasedTraining.step beside ms per training iteration of the same run
without PBT (examples/population_selfplay_train.py --trainer device-epoch, --pbt-every 0), the iteration measured both on this tree
and on a checkout of the PARENT commit in the same run on the same box.  GPU box only:
    python tools/pbt_latency.py --parent-tree <checkout of the parent commit, built> [--reps 20] [--out profiles/pbt_latency.txt]
    python tools/pbt_latency.py --learning profiles/pbt_learning_cartpole.jsonl      # the learning record instead

Shapes: 8 and 64 CartPole 2x128 nets and 4 Pendulum 4x1024 nets (the wide trainer), 32 games per net, the example's defaults
otherwise (32 simulations, 20 steps per iteration, 512 training rows per net in minibatches of 128), every net with its own learning
rate (per_net=True in both trees).  An iteration is self-play + the training epoch + the weight hand-off, from the example's own
records, after 3 warm-up iterations.  A step is select + trainer.copy_nets + sp.copy_nets + explore of lr + reload_settings +
upload_flat at fraction 0.25 (2, 16 and 1 nets replaced) on fresh random scores each time, host clock around the call with the device
idle before and after.  Nothing is gated: a record.

The learning record: one run of the example on CartPole with --lrs spread over 1e-5 ... 1e-1 across 8 seeds, without and with
--pbt-every 5 --pbt-explore lr; every iteration's record of both, field "pbt_every" 0 / 5."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WARM = 3
SHAPES = {"cartpole_2x128 x 8 nets": ["--game", "CartPole-v0", "--hidden", "128", "128", "--nets", "8"],
          "cartpole_2x128 x 64 nets": ["--game", "CartPole-v0", "--hidden", "128", "128", "--nets", "64"],
          "pendulum_4x1024 x 4 nets": ["--game", "Pendulum-v0", "--hidden", "1024", "1024", "1024", "1024", "--wide", "--nets", "4"]}
LEARNING = ["--game", "CartPole-v0", "--seeds", "0", "1", "2", "3", "4", "5", "6", "7", "--games-per-seed", "64", "--iters", "40",
            "--trainer", "device-epoch", "--lrs", "1e-5", "3.7e-5", "1.4e-4", "5.2e-4", "1.9e-3", "7.2e-3", "2.7e-2", "1e-1"]


def _example_args(P, shape, iters):
    args = list(shape)
    K = int(args[args.index("--nets") + 1])
    del args[args.index("--nets"):args.index("--nets") + 2]
    lrs = [f"{lr:.3g}" for lr in np.geomspace(1e-4, 1e-2, K)]
    return P.parse_args(args + ["--seeds"] + [str(s) for s in range(K)] + ["--games-per-seed", "32", "--iters", str(iters), "--trainer",
                                                                          "device-epoch", "--device", "cuda", "--lrs"] + lrs)


def child(tree, reps, steps):
    """One tree's measurements as a JSON line {shape: {"iteration": [ms, ...], "step": [ms, ...]}} (``steps``: this tree has the step)."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "examples"))
    import population_selfplay_train as P
    import torch
    res = {}
    for name, shape in SHAPES.items():
        hist = P.train(_example_args(P, shape, WARM + reps), log=None)
        res[name] = {"iteration": [1e3 * (h["selfplay_s"] + h["train_s"] + h["sync_s"]) for h in hist[WARM:]], "step": []}
        if not steps:
            continue
        from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
        from alphazero_gym_amd.pbt import PopulationBasedTraining
        a = _example_args(P, shape, 1)
        agents, _, sp = P.build_population(a)
        tr = PopulationTrainer(agents, max_batch=512, losses="device", optimizers="agents", per_net=True, wide=a.wide)
        driver = PopulationBasedTraining(sp, tr, {"lr": {"factors": [0.8, 1.25], "min": 1e-6, "max": 1.0}}, fraction=0.25, seed=0)
        sp.play(2)
        rng = np.random.default_rng(0)
        for rep in range(WARM + reps):
            scores = rng.normal(size=len(agents))
            sp.engine.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = driver.step(scores)
            sp.engine.sync()
            torch.cuda.synchronize()
            if rep >= WARM:
                res[name]["step"].append(1e3 * (time.perf_counter() - t0))
            assert len(rec["replaced"]) == len(agents) // 4
        tr.close()
        sp.close()
    print("RESULT " + json.dumps(res), flush=True)


def _run_child(tree, reps, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--reps", str(reps)] + (["--steps"] if steps else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900, cwd=tree).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def learning(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import population_selfplay_train as P
    lines = [{"note": "examples/population_selfplay_train.py " + " ".join(LEARNING) + ", without and with --pbt-every 5 --pbt-explore lr (field "
                      "pbt_every: 0 / 5); one run each on one MI355X; a record, no claim: one engine seed, eight nets"}]
    for extra, every in (([], 0), (["--pbt-every", "5", "--pbt-explore", "lr"], 5)):
        for h in P.train(P.parse_args(LEARNING + extra), log=None):
            lines.append(dict({"pbt_every": every}, **{k: v for k, v in h.items() if k not in ("selfplay_s", "train_s", "sync_s", "weight_sync")}))
    with open(out, "w") as f:
        f.write("".join(json.dumps(ln) + "\n" for ln in lines))
    print(f"{len(lines) - 1} records -> {out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--learning", metavar="OUT")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbt_latency.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.tree, a.reps, a.steps)
    if a.learning:
        return learning(a.learning)
    if not a.parent_tree or not os.path.isdir(os.path.join(a.parent_tree, "alphazero_gym_amd")):
        sys.exit("--parent-tree: a built checkout of the parent commit (its training iteration is measured in the same run)")
    if a.reps < 20:
        sys.exit("--reps: medians of at least 20")
    parent = _run_child(os.path.abspath(a.parent_tree), a.reps, False)
    new = _run_child(ROOT, a.reps, True)
    med = statistics.median
    lines = [f"pbt_latency: ms, host clock, medians of {a.reps} (min .. max) after {WARM} warm-up calls; one MI355X, one run, the parent commit's tree",
             "and this tree in a child process each", "",
             "iteration = one iteration of examples/population_selfplay_train.py --trainer device-epoch --lrs ... without PBT (self-play of 20 steps x",
             "32 games per net x 32 simulations + the training epoch over 512 rows per net + upload_flat); step = one",
             "PopulationBasedTraining.step at fraction 0.25 exploring lr (select, both copy_nets, perturb, reload_settings, upload_flat)", ""]
    for name in SHAPES:
        p, n, s = parent[name]["iteration"], new[name]["iteration"], new[name]["step"]
        lines.append(f"  {name:26s} iteration, parent commit {med(p):9.3f} ({min(p):.3f} .. {max(p):.3f})   this tree {med(n):9.3f} ({min(n):.3f} .. {max(n):.3f})   "
                     f"ratio {med(n) / med(p):.3f}")
        lines.append(f"  {'':26s} PBT step {med(s):9.3f} ({min(s):.3f} .. {max(s):.3f})   step / parent iteration {med(s) / med(p):.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
