#!/usr/bin/env python3
"""What the trainer's moving average (include/azgym_train_ema.h) and the engine's target weight set (include/azgym_target.h) cost.
GPU box only:
    python tools/ema_latency.py [--parent-lib <libazgym_hip.so built from the parent commit>] [--reps 20] [--out profiles/ema_latency.txt]

1. train_epoch (1024 rows per net in minibatches of 128: 8 optimiser steps per call) without an average, with one that moves after
   every step and with every=8, on CartPole 2x128 at K = 1, 8, 64, 256 and Pendulum 4x1024 (wide=True) at K = 1, 4, 16; the increment
   per optimiser step, and for the kernel's 12 K P bytes the rate it amounts to beside the 6.29 TB/s of a float4 copy.
2. The same epoch, no average attached, on this tree's library and on --parent-lib's (AZG_HIP_LIB), a child process each; the parent
   twice, which gives its own run-to-run spread.
3. azg_use_weights LIVE -> TARGET -> LIVE around nothing (host time), evaluate(nets="target") beside evaluate(), and what the round
   trip replaces: two upload_flat calls (a gather launch and a synchronisation each).
Host clock around the synchronising calls, medians (min .. max) after 3 warm-up calls.  Nothing is gated: a record."""
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

WARM, ROWS, BATCH = 3, 1024, 128
STEPS = ROWS // BATCH
COPY_RATE = 6.29e12   # bytes / s: the measured float4 copy rate of one MI355X
# name: (kind, state_dim, hidden, policy overrides, trainer keywords, the K to measure)
SHAPES = {"cartpole_2x128": ("discrete", 4, [128, 128], {}, {}, (1, 8, 64, 256)),
          "pendulum_4x1024": ("continuous", 3, [1024] * 4, dict(num_components=2), dict(wide=True), (1, 4, 16))}
EVAL_SHAPES = {"cartpole_2x128 x 8 nets": ("CartPole-v0", "discrete", [128, 128], {}, 8, 32),
               "pendulum_4x1024 x 4 nets": ("Pendulum-v0", "continuous", [1024] * 4, dict(num_components=2), 4, 32)}


def _times(fn, reps):
    import torch
    out = []
    for i in range(WARM + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def _agents(kind, hidden, over, K):
    import torch
    from alphazero_gym_amd import run
    from alphazero_gym_amd.envs import make_game
    base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
    cfg = run._merge(base, dict(device="cuda", policy=dict(over, hidden_dimensions=hidden)))
    env = make_game(cfg["game"])
    torch.manual_seed(0)
    return cfg, [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]


def _rows(kind, K, S, A):
    import torch
    g = torch.Generator().manual_seed(0)
    obs = torch.randn((K, ROWS, S), generator=g)
    actions = torch.arange(A, dtype=torch.float32).repeat(K, ROWS, 1) if kind == "discrete" else torch.rand((K, ROWS, A), generator=g) * 3.6 - 1.8
    counts = torch.randint(1, 9, (K, ROWS, A), generator=g).float()
    return torch.cat([obs, actions, counts, counts, torch.randn((K, ROWS, 1), generator=g)], dim=-1).cuda().contiguous()


def child_epochs(reps, with_ema):
    """{shape: {K: {"P": P, "none": [ms], "every1": [ms], "every8": [ms]}}} (the last two only ``with_ema``)."""
    from alphazero_gym_amd import _capi
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    res = {}
    for name, (kind, S, hidden, over, kw, Ks) in SHAPES.items():
        res[name] = {}
        A = 2 if kind == "discrete" else 8
        for K in Ks:
            _, agents = _agents(kind, hidden, over, K)
            tr = PopulationTrainer(agents, max_batch=2 * BATCH, losses="device", **kw, **({"ema": 0.99} if with_ema else {}))
            rows = _rows(kind, K, S, A)
            order = np.stack([np.random.RandomState(k).permutation(ROWS) for k in range(K)]).astype(np.int32)
            where = _capi.epoch_rows(rows.data_ptr(), S, A, ROWS)
            call = lambda: tr._epoch("train_epoch", where, order, BATCH)   # noqa: E731  (the native call on a prepared order)
            out = {"P": int(tr.flat.shape[1])}
            if with_ema:
                tr.set_ema(None)
            out["none"] = _times(call, reps)
            if with_ema:
                for key, every in (("every1", 1), ("every8", 8)):
                    tr.set_ema(decay=0.99, every=every)
                    out[key] = _times(call, reps)
                    assert tr.ema_updates == (WARM + reps) * STEPS // every
            tr.close()
            res[name][str(K)] = out
    print("RESULT " + json.dumps(res), flush=True)


def child_target(reps):
    """{shape: {"round_trip": [ms], "evaluate": [ms], "evaluate_target": [ms], "two_uploads": [ms]}}"""
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent.population_trainer import bind_flat
    res = {}
    for name, (game, kind, hidden, over, K, G) in EVAL_SHAPES.items():
        cfg, agents = _agents(kind, hidden, over, K)
        m = cfg["mcts"]
        sp = run.PopulationSelfPlay([a.nn for a in agents], game=game, games_per_net=G, n_rollouts=8, c_uct=m["c_uct"], gamma=m["gamma"],
                                    epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5), capacity_steps=2)
        desc, flat = bind_flat([a.nn for a in agents])
        target = (flat * 0.5).contiguous()
        sp.upload_flat(desc, flat)
        sp.upload_target_flat(desc, target)
        e = sp.engine

        def round_trip():
            e.use_weights("target")
            e.use_weights("live")

        def two_uploads():
            sp.upload_flat(desc, target)
            sp.upload_flat(desc, flat)

        res[name] = {"round_trip": _times(round_trip, reps), "evaluate": _times(lambda: sp.evaluate(G), reps),
                     "evaluate_target": _times(lambda: sp.evaluate(G, nets="target"), reps), "two_uploads": _times(two_uploads, reps)}
        sp.close()
    print("RESULT " + json.dumps(res), flush=True)


def _run_child(part, reps, lib=None, no_ema=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--reps", str(reps)] + (["--no-ema"] if no_ema else [])
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("AZG_HIP_LIB", None)
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=1100, cwd=ROOT, env=env).stdout
    print(f"[{part}{' on ' + lib if lib else ''}: done]", file=sys.stderr, flush=True)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def _mmm(x):
    return f"{statistics.median(x):9.3f} ({min(x):.3f} .. {max(x):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["epochs", "target"])
    ap.add_argument("--no-ema", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_latency.txt"))
    a = ap.parse_args()
    if a.child == "epochs":
        return child_epochs(a.reps, not a.no_ema)
    if a.child == "target":
        return child_target(a.reps)
    med = statistics.median
    new = _run_child("epochs", a.reps)
    lines = [f"ema_latency: ms, host clock around the synchronising call, medians of {a.reps} (min .. max) after {WARM} warm-up calls; one MI355X, one run", "",
             f"1. azg_trainer_epoch* of {ROWS} rows per net in minibatches of {BATCH} ({STEPS} optimiser steps per call; the native call on a prepared order,",
             "   losses on the device, fused RMSprop): no average attached | one that moves after every step | every = 8; then the increment per",
             f"   optimiser step in us, (every1 - none) / {STEPS}, the kernel's bytes 12 K P (two loads and a store per element), and the rate that increment",
             "   amounts to as a fraction of the 6.29 TB/s float4 copy rate.  One dependent kernel boundary costs about 1.5-2 us on this device.", ""]
    for name, per_k in new.items():
        lines.append(f"   {name}")
        for K, r in per_k.items():
            inc = (med(r["every1"]) - med(r["none"])) / STEPS * 1e3
            inc8 = (med(r["every8"]) - med(r["none"])) * 1e3
            nbytes = 12 * int(K) * r["P"]
            frac = nbytes / (inc * 1e-6) / COPY_RATE if inc > 0 else float("nan")
            lines.append(f"     K {int(K):4d}  P {r['P']:8d} | none {_mmm(r['none'])} | every 1 {_mmm(r['every1'])} | every 8 {_mmm(r['every8'])} | "
                         f"per step {inc:8.2f} us, {nbytes / 1e6:9.3f} MB, {frac:6.3f} of the copy rate | the one update of every 8: {inc8:8.2f} us")
    if a.parent_lib:
        runs = [_run_child("epochs", a.reps, lib=a.parent_lib, no_ema=True) for _ in range(2)]
        lines += ["", "2. The same call with no average attached: this tree's library against the parent commit's, a process each; the parent twice (its own",
                  "   run-to-run spread: run 2 / run 1).", ""]
        for name, per_k in new.items():
            lines.append(f"   {name}")
            for K, r in per_k.items():
                p1, p2 = runs[0][name][K]["none"], runs[1][name][K]["none"]
                lines.append(f"     K {int(K):4d} | parent run 1 {_mmm(p1)} | parent run 2 {_mmm(p2)} (ratio {med(p2) / med(p1):.4f}) | this tree {_mmm(r['none'])} "
                             f"(to run 1 {med(r['none']) / med(p1):.4f}, to run 2 {med(r['none']) / med(p2):.4f})")
    tgt = _run_child("target", a.reps)
    lines += ["", "3. The engine's target set: azg_use_weights LIVE -> TARGET -> LIVE around nothing (host time only) | evaluate(G episodes per net) live |",
              "   evaluate(nets=\"target\") | what the round trip replaces, two upload_flat calls (a gather launch and a synchronisation each).", ""]
    for name, r in tgt.items():
        lines.append(f"   {name:26s} | round trip {_mmm(r['round_trip'])} | evaluate {_mmm(r['evaluate'])} | nets=target {_mmm(r['evaluate_target'])} | "
                     f"two uploads {_mmm(r['two_uploads'])}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
