#!/usr/bin/env python3
"""What feeding the trainer's value errors back as priorities costs: azg_selfplay_priorities_trained under each `unseen` mode beside
azg_selfplay_priorities (value gap) on the same full ring, a self-play step with errors kept beside a plain one, and one
PopulationTrainer.train_epoch_ring(weights="priority", errors=True) against the weighted epoch on the same rows and order -- the
yardstick being the library built from the PARENT commit on the same box in the same run.  GPU box only:
    python tools/priority_feedback_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 3] [--out profiles/priority_feedback_latency.txt]

Ring: CartPole 2x128 ReLU x 4096 games x 100 simulations, a FIFO ring of 64 steps, full (262144 stored rows), as one net of 4096 games
and as 64 nets of 64 games; half of the errors planted as seen.  Priorities: 20 asynchronous calls and one synchronisation, ms per call.
Steps: 20 asynchronous azg_selfplay_step calls and one synchronisation, ms per step: first plain at the same point of the games as in
the parent's child, then, later in the games, with errors not kept and kept alternating repeat by repeat.
Epochs: CartPole 2x128 at 1 / 8 / 64 nets and Pendulum 4x1024 ELU with a mixture of 2 (the wide trainer) at 1 / 4 nets; 32 games per
net, 64 stored steps: 2048 rows per net in minibatches of 256, one permutation per net.  Every round starts one child process per
library (AZG_HIP_LIB), parent and this build alternating; inside a child of this build the weighted epoch and the one that also writes
the errors alternate call by call.  Host clock around the whole call; nothing is gated: a record."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING = (dict(env_id=0, mode=0, n_trees=4096, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34), (4, [128, 128], 2, "relu"), 200)
RING_NETS = (1, 64)
CALLS, CAPACITY = 20, 64
ALPHA, EPS, BETA = 0.6, 1e-3, 0.4
UNSEEN = (("max", "max"), ("value_gap", "value_gap"), ("constant", 1.0))
EPOCHS = {"cartpole_2x128": ("discrete", dict(hidden_dimensions=[128, 128]), dict(), (1, 8, 64)),
          "pendulum_4x1024_gmm2": ("continuous", dict(hidden_dimensions=[1024] * 4, num_components=2), dict(wide=True), (1, 4))}
T, STEPS, BATCH = 32, 64, 256


def _timed(e, call, repeats, calls=CALLS):
    out = []
    for _ in range(repeats):
        e.sync()
        t0 = time.perf_counter()
        for i in range(calls):
            call(i)
        e.sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def _ring_part(repeats, have):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, nd, act), max_len = RING
    res = {}
    for n_nets in RING_NETS:
        e = _native.HipEngine(**kw)
        desc = _capi.make_desc(in_dim, hidden, nd, act)
        if n_nets == 1:
            e.set_weights(desc, make_weights(34, in_dim, hidden, nd))
        else:
            e.set_population(n_nets)
            for k in range(n_nets):
                e.set_net_weights(k, desc, make_weights(34 + k, in_dim, hidden, nd))
        (e.selfplay_begin if n_nets == 1 else e.population_selfplay_begin)(max_len, False, capacity_steps=CAPACITY, fifo=True)
        e.selfplay_keep_transitions(True)
        e.selfplay_keep_priorities(True)
        for _ in range(CAPACITY):
            e.selfplay_step()
        e.selfplay_nstep_targets(5)
        e.selfplay_priorities(ALPHA, EPS)
        res[f"priorities@{n_nets}"] = _timed(e, lambda i: e.selfplay_priorities(ALPHA, EPS), repeats)
        res[f"step@{n_nets}"] = _timed(e, lambda i: e.selfplay_step(), repeats)
        if have:
            e.selfplay_keep_errors(True)
            rng = np.random.default_rng(1)
            err = rng.uniform(0.0, 2.0, CAPACITY * kw["n_trees"]).astype(np.float32)
            err[rng.random(err.shape) < 0.5] = -1.0
            e.selfplay_set_error_values(err)
            for name, unseen in UNSEEN:
                e.selfplay_priorities_trained(ALPHA, EPS, unseen)
                res[f"trained_{name}@{n_nets}"] = _timed(e, lambda i: e.selfplay_priorities_trained(ALPHA, EPS, unseen), repeats)
            # (the games move on and a step's cost with them: errors kept and not kept alternate, repeat by repeat)
            off, on = [], []
            for _ in range(repeats):
                e.selfplay_keep_errors(False)
                off += _timed(e, lambda i: e.selfplay_step(), 1)
                e.selfplay_keep_errors(True)
                on += _timed(e, lambda i: e.selfplay_step(), 1)
            res[f"step_alt_plain@{n_nets}"], res[f"step_kept@{n_nets}"] = off, on
        e.close()
    return res


def _epoch_part(repeats, have):
    import torch
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    from alphazero_gym_amd.envs import make_game
    res = {}
    for name, (kind, policy, flags, net_counts) in EPOCHS.items():
        base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
        cfg = run._merge(base, dict(device="cuda", policy=policy))
        env = make_game(cfg["game"])
        m = cfg["mcts"]
        for K in net_counts:
            torch.manual_seed(0)
            agents = [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]
            prioritized = {"alpha": ALPHA, "eps": EPS, "beta": BETA}
            if have:
                prioritized["feedback"] = "max"
            sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=T, n_rollouts=8, c_uct=m["c_uct"],
                                        gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                        capacity_steps=STEPS, n_step=5, prioritized=prioritized)
            sp.play_device(STEPS)
            n_rows = STEPS * T
            tr = PopulationTrainer(agents, max_batch=2 * BATCH, losses="device", **flags)
            order = np.stack([np.random.RandomState(s).permutation(n_rows) for s in range(K)])
            sp.priorities()
            sp.is_weights()
            weighted, errors = [], []
            for rep in range(2 + repeats):   # (two warm-up pairs)
                t0 = time.perf_counter()
                tr.train_epoch_ring(sp, order, batch_size=BATCH, weights="priority")
                t1 = time.perf_counter()
                if have:
                    tr.train_epoch_ring(sp, order, batch_size=BATCH, weights="priority", errors=True)
                t2 = time.perf_counter()
                if rep >= 2:
                    weighted.append((t1 - t0) * 1e3)
                    errors.append((t2 - t1) * 1e3)
            res[f"{name}@{K}"] = dict(weighted=weighted, errors=errors if have else [])
            tr.close()
            sp.close()
    return res


def child(repeats):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {part: {variant: [ms, ...]}}."""
    from alphazero_gym_amd import _native
    have = "selfplay_priorities_trained" in _native.fns()
    print("RESULT " + json.dumps(dict(ring=_ring_part(repeats, have), epoch=_epoch_part(repeats, have))), flush=True)


def _run_child(lib, repeats):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    else:
        env.pop("AZG_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)], env=env, check=True, capture_output=True,
                         text=True, timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def _against(p_rounds, n_rounds, med):
    """(parent median, its spread over the rounds, this build's median, ratio, verdict)"""
    p, n = med(p_rounds), med(n_rounds)
    spread = (max(p_rounds) - min(p_rounds)) / p
    return p, spread, n, n / p, "within" if abs(n / p - 1) <= spread else "OUTSIDE"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priority_feedback_latency.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.repeats)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the libazgym_hip.so of a build of the parent commit (the yardstick is measured in the same run)")
    parent, new = [], []
    for i in range(a.rounds):
        parent.append(_run_child(os.path.abspath(a.parent_lib), a.repeats))
        new.append(_run_child(None, a.repeats))
        print(f"round {i + 1} of {a.rounds} done", file=sys.stderr, flush=True)
    med = statistics.median
    lines = [f"priority_feedback_latency: ms per call, host clock; {a.rounds} rounds x {a.repeats} repeats per library, parent-commit library and this build in",
             "alternating child processes of one run on one MI355X", "",
             f"azg_selfplay_priorities_trained (alpha {ALPHA}; half of the rows seen) beside azg_selfplay_priorities (value gap): FIFO ring of {CAPACITY} steps x",
             f"4096 CartPole games, full (262144 stored rows); {CALLS} asynchronous calls, one synchronisation"]
    for n_nets in RING_NETS:
        p, spread, n, ratio, verdict = _against([med(r["ring"][f"priorities@{n_nets}"]) for r in parent],
                                                [med(r["ring"][f"priorities@{n_nets}"]) for r in new], med)
        lines.append(f"  {n_nets:2d} net(s) x {4096 // n_nets:4d} games   priorities (value gap): parent library {p:.4f} ms (spread {100 * spread:.1f} %), this build {n:.4f} ms "
                     f"(ratio {ratio:.3f}, {verdict} the parent's spread)")
        for name, _ in UNSEEN:
            rounds = [med(r["ring"][f"trained_{name}@{n_nets}"]) for r in new]
            lines.append(f"      priorities_trained, unseen = {name:9s} {med(rounds):.4f} ms (per-round medians {', '.join(f'{x:.4f}' for x in rounds)})   "
                         f"/ the parent's priorities {med(rounds) / p:.2f}")
    lines += ["", f"azg_selfplay_step on that ring (search of 100 simulations and the step's kernel): {CALLS} asynchronous steps, one synchronisation, ms per step"]
    for n_nets in RING_NETS:
        p_rounds = [med(r["ring"][f"step@{n_nets}"]) for r in parent]
        p, spread, n, ratio, verdict = _against(p_rounds, [med(r["ring"][f"step@{n_nets}"]) for r in new], med)
        a_rounds = [med(r["ring"][f"step_alt_plain@{n_nets}"]) for r in new]
        k_rounds = [med(r["ring"][f"step_kept@{n_nets}"]) for r in new]
        ratios = [k / a for k, a in zip(k_rounds, a_rounds)]
        kverdict = "within" if abs(med(k_rounds) / med(a_rounds) - 1) <= spread else "OUTSIDE"
        lines.append(f"  {n_nets:2d} net(s)   parent {p:.4f} ms (rounds {', '.join(f'{x:.4f}' for x in p_rounds)}; spread {100 * spread:.2f} %)   this build, errors not kept "
                     f"{n:.4f} ms (ratio {ratio:.4f}, {verdict} the parent's spread)")
        lines.append(f"      later in the games, alternating: errors not kept {med(a_rounds):.4f} ms, kept {med(k_rounds):.4f} ms   kept / not kept "
                     f"{med(k_rounds) / med(a_rounds):.4f} (rounds {', '.join(f'{x:.4f}' for x in ratios)}; {kverdict} the parent's spread)")
    lines += ["", f"train_epoch_ring, one epoch of {STEPS * T} rows per net in minibatches of {BATCH} (losses on the device): weights=\"priority\" on the parent's library,",
              "weights=\"priority\" and weights=\"priority\" with errors=True on this build (alternating call by call)"]
    for name, (_, _, _, net_counts) in EPOCHS.items():
        for K in net_counts:
            key = f"{name}@{K}"
            p_rounds = [med(r["epoch"][key]["weighted"]) for r in parent]
            w_rounds = [med(r["epoch"][key]["weighted"]) for r in new]
            e_rounds = [med(r["epoch"][key]["errors"]) for r in new]
            p, spread, w, wratio, _ = _against(p_rounds, w_rounds, med)
            _, _, e, eratio, verdict = _against(p_rounds, e_rounds, med)
            ratios = [er / wr for er, wr in zip(e_rounds, w_rounds)]
            lines.append(f"  {name} x {K:2d} net(s)   parent weighted {p:8.3f} ms (rounds {', '.join(f'{x:.3f}' for x in p_rounds)}; spread {100 * spread:.2f} %)   "
                         f"this build weighted {w:8.3f} ms (ratio to parent {wratio:.4f})   with errors {e:8.3f} ms   errors / weighted "
                         f"{e / w:.4f} (rounds {', '.join(f'{x:.4f}' for x in ratios)})   errors / parent {eratio:.4f} ({verdict} the parent's spread)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
