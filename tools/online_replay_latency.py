#!/usr/bin/env python3
"""What a minibatch of prioritised replay costs when every minibatch is redrawn from refreshed priorities: ms per minibatch of
    (a) PopulationTrainer.train_online_ring -- one native call for M minibatches (azg_trainer_epoch_online), this build;
    (b) the host loop it stands for, per minibatch priorities() / sample_order(batch) / is_weights() /
        train_epoch_ring(weights="priority", errors=True), on the library built from the PARENT commit (and on this build);
    (c) the floor: one fixed-priority train_epoch_ring(weights="priority", errors=True) over M * batch drawn rows, per minibatch, on
        the parent's library (and on this build).
GPU box only:
    python tools/online_replay_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 2] [--out profiles/online_replay_latency.txt]

Ring: 64 steps x 4096 games, full (262144 stored rows), split into K nets of 4096 / K games.  Shapes: CartPole 2x128 ReLU at 1 / 8 /
64 nets, minibatches of 32 and 128 rows per net; Pendulum 4x1024 ELU with a mixture of 2 (the wide trainer) at 1 / 4 nets,
minibatches of 128.  alpha 0.6, beta 0.4, unseen "max" (the five-launch refresh).  Beside them a self-play step on both libraries
(CartPole 2x128 x 4096 games x 100 simulations, transitions, priorities and errors kept: 20 asynchronous steps, one synchronisation).
Every timed window is M = 64 minibatches, host clock around calls that end in a synchronisation; two warm-up windows, then the
repeats, (a) / (b) / (c) alternating window by window.
Every round starts one child process per library (AZG_HIP_LIB), parent and this build alternating, and which of the two goes first
alternates round by round.  Nothing is gated: a record."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole_2x128": ("discrete", dict(hidden_dimensions=[128, 128]), dict(), (1, 8, 64), (32, 128)),
          "pendulum_4x1024_gmm2": ("continuous", dict(hidden_dimensions=[1024] * 4, num_components=2), dict(wide=True), (1, 4), (128,))}
GAMES, STEPS, M = 4096, 64, 64
ALPHA, EPS, BETA = 0.6, 1e-3, 0.4
STEP = (dict(env_id=0, mode=0, n_trees=4096, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34), (4, [128, 128], 2, "relu"), 200)
STEP_CALLS = 20


def _step_part(repeats):
    """ms per azg_selfplay_step with everything the online epoch needs kept, the ring full."""
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, nd, act), max_len = STEP
    e = _native.HipEngine(**kw)
    e.set_weights(_capi.make_desc(in_dim, hidden, nd, act), make_weights(34, in_dim, hidden, nd))
    e.selfplay_begin(max_len, False, capacity_steps=STEPS, fifo=True)
    e.selfplay_keep_transitions(True)
    e.selfplay_keep_priorities(True)
    e.selfplay_keep_errors(True)
    for _ in range(STEPS):
        e.selfplay_step()
    out = []
    for _ in range(repeats):
        e.sync()
        t0 = time.perf_counter()
        for _ in range(STEP_CALLS):
            e.selfplay_step()
        e.sync()
        out.append((time.perf_counter() - t0) * 1e3 / STEP_CALLS)
    e.close()
    return out


def _loop(sp, tr, batch):
    for _ in range(M):
        sp.priorities()
        order = sp.sample_order(batch)
        sp.is_weights()
        tr.train_epoch_ring(sp, order, batch_size=batch, weights="priority", errors=True)


def _fixed(sp, tr, batch):
    """Returns the time of the epoch alone: the draw in front of it is the iteration's, not the minibatch's."""
    sp.priorities()
    order = sp.sample_order(M * batch)
    sp.is_weights()
    sp.engine.sync()
    t0 = time.perf_counter()
    tr.train_epoch_ring(sp, order, batch_size=batch, weights="priority", errors=True)
    return time.perf_counter() - t0


def child(repeats, only):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {shape@K@batch: {variant: [ms per minibatch, ...]}}."""
    import torch
    from alphazero_gym_amd import _native, run
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    from alphazero_gym_amd.envs import make_game
    have = "trainer_epoch_online" in _native.fns()
    res = {"step": _step_part(repeats)}
    for name, (kind, policy, flags, net_counts, batches) in SHAPES.items():
        if only and name not in only:
            continue
        base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
        cfg = run._merge(base, dict(device="cuda", policy=policy))
        env = make_game(cfg["game"])
        m = cfg["mcts"]
        for K in net_counts:
            torch.manual_seed(0)
            agents = [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]
            sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=GAMES // K, n_rollouts=4, c_uct=m["c_uct"],
                                        gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                        capacity_steps=STEPS, n_step=5, prioritized={"alpha": ALPHA, "eps": EPS, "beta": BETA, "feedback": "max"})
            sp.play_device(STEPS)
            tr = PopulationTrainer(agents, max_batch=256, losses="device", **flags)
            for batch in batches:
                out = dict(online=[], loop=[], fixed=[])
                for rep in range(2 + repeats):   # (two warm-up windows of each)
                    t = {}
                    if have:
                        sp.engine.sync()
                        t0 = time.perf_counter()
                        tr.train_online_ring(sp, M, batch_size=batch)
                        t["online"] = time.perf_counter() - t0
                    sp.engine.sync()
                    t0 = time.perf_counter()
                    _loop(sp, tr, batch)
                    t["loop"] = time.perf_counter() - t0
                    t["fixed"] = _fixed(sp, tr, batch)
                    if rep >= 2:
                        for key, val in t.items():
                            out[key].append(val * 1e3 / M)
                res[f"{name}@{K}@{batch}"] = out
            tr.close()
            sp.close()
    print("RESULT " + json.dumps(res), flush=True)


def _run_child(lib, repeats, only):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    else:
        env.pop("AZG_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)] + (["--only"] + only if only else [])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None, help="shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_replay_latency.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.repeats, a.only)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the libazgym_hip.so of a build of the parent commit (the yardstick is measured in the same run)")
    parent, new = [], []
    for i in range(a.rounds):   # (which library goes first alternates round by round: the second child finds a warmer GPU)
        for lib in ((a.parent_lib, None) if i % 2 == 0 else (None, a.parent_lib)):
            (parent if lib else new).append(_run_child(os.path.abspath(lib) if lib else None, a.repeats, a.only))
        print(f"round {i + 1} of {a.rounds} done", file=sys.stderr, flush=True)
    med = statistics.median

    def of(rounds, key, variant):
        per_round = [med(r[key][variant]) for r in rounds]
        return med(per_round), (max(per_round) - min(per_round)) / med(per_round)

    lines = [f"online_replay_latency: ms per minibatch, host clock around windows of {M} minibatches that end in a synchronisation; {a.rounds} rounds x",
             f"{a.repeats} repeats per library, parent-commit library and this build in alternating child processes of one run on one MI355X.",
             f"Ring: {STEPS} steps x {GAMES} games, full ({STEPS * GAMES} stored rows), K nets of {GAMES} / K games; alpha {ALPHA}, beta {BETA}, unseen \"max\".",
             "(a) train_online_ring, this build   (b) the host loop of priorities / sample_order / is_weights / train_epoch_ring per minibatch",
             "(c) the floor: one fixed-priority train_epoch_ring(weights=\"priority\", errors=True), per minibatch.  (spread: of the per-round medians)", ""]
    for key in parent[0]:
        if key == "step":
            continue
        name, K, batch = key.split("@")
        b_p, b_ps = of(parent, key, "loop")
        c_p, c_ps = of(parent, key, "fixed")
        a_n, a_ns = of(new, key, "online")
        b_n, _ = of(new, key, "loop")
        c_n, _ = of(new, key, "fixed")
        lines.append(f"  {name} x {int(K):2d} net(s), batch {int(batch):3d}   (a) {a_n:7.4f} ms (spread {100 * a_ns:4.1f} %)   (b) parent {b_p:7.4f} ms (spread {100 * b_ps:4.1f} %), "
                     f"this build {b_n:7.4f}   (c) parent {c_p:7.4f} ms (spread {100 * c_ps:4.1f} %), this build {c_n:7.4f}   "
                     f"(a) / (b) {a_n / b_p:.3f}   (a) / (c) {a_n / c_p:.3f}   (a) - (c) {a_n - c_p:+.4f} ms")
    p_rounds, n_rounds = [med(r["step"]) for r in parent], [med(r["step"]) for r in new]
    spread = (max(p_rounds) - min(p_rounds)) / med(p_rounds)
    ratio = med(n_rounds) / med(p_rounds)
    lines += ["", f"azg_selfplay_step, CartPole 2x128 x 4096 games x 100 simulations, transitions, priorities and errors kept, the ring full: {STEP_CALLS} asynchronous",
              f"steps, one synchronisation, ms per step: parent {med(p_rounds):.4f} (rounds {', '.join(f'{x:.4f}' for x in p_rounds)}; spread {100 * spread:.2f} %)   this build "
              f"{med(n_rounds):.4f} (rounds {', '.join(f'{x:.4f}' for x in n_rounds)})   ratio {ratio:.4f} ({'within' if abs(ratio - 1) <= spread else 'OUTSIDE'} the parent's spread)"]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
