#!/usr/bin/env python3
"""What one azg_selfplay_nstep_targets call over a full ring costs, and what keeping the transitions costs a self-play step, against a
library built from the PARENT commit on the same box in the same run.
GPU box only:
    python tools/nstep_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 3] [--out profiles/nstep_latency.txt]

Shapes (tools/reanalyse_latency.py's): Pendulum-v1 2x256 ELU x 4096 games x 200 simulations, CartPole 2x128 ReLU x 4096 x 100,
Pendulum-v1 4x1024 ELU x 1024 x 50; a FIFO ring of 64 steps, full.
Every round starts one child process per library (AZG_HIP_LIB), parent and this build alternating; a child measures, per shape,
    step        selfplay_step, nothing kept (both libraries)
    step+keep   selfplay_step after selfplay_keep_transitions (this build)
    nstep       selfplay_nstep_targets(n_step, the search's gamma) over the full ring, n_step 5 and 1000 (this build)
each as the host clock around 20 calls and ONE stream synchronisation after them, repeated; ms per call.  The table gives medians over
all rounds and repeats, the parent step's spread (max - min of its per-round medians, relative), and the ratios to the parent's step.
Nothing is gated: the figures are a record.

    python tools/nstep_latency.py --lambda-call --parent-lib <parent build's libazgym_hip.so> [--out profiles/lambda_latency.txt]
measures the lambda-return call (include/azgym_lambda.h) instead, on a CartPole 2x128 ReLU population of 8 nets x 512 games whose
full ring holds 64 steps x 4096 games, per library in the same alternating child processes:
    nstep       selfplay_nstep_targets(n_step) at n_step 5 and 1000 (both libraries; the parent's is the yardstick)
    lambda      selfplay_lambda_targets(n_step, 0.9): one rule for every net (this build)
    lambda nets the same with 8 per-net rules, lambda 0.3 .. 1 (this build)
    copy        the call's host-to-device copy alone: 32 bytes per net on the engine's stream (this build)
and writes the ratios lambda / parent nstep and the copy's share of the lambda call."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "pendulum_2x256_4096x200": (dict(env_id=2, mode=1, n_trees=4096, n_sims=200, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [256, 256], 2, "elu"), 200),
    "cartpole_2x128_4096x100": (dict(env_id=0, mode=0, n_trees=4096, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34), (4, [128, 128], 2, "relu"), 200),
    "pendulum_4x1024_1024x50": (dict(env_id=2, mode=1, n_trees=1024, n_sims=50, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [1024] * 4, 2, "elu"), 200),
}
CALLS, CAPACITY = 20, 64
N_STEPS = (5, 1000)


def _timed(e, call, repeats):
    out = []
    for _ in range(repeats):
        e.sync()
        t0 = time.perf_counter()
        for i in range(CALLS):
            call(i)
        e.sync()
        out.append((time.perf_counter() - t0) * 1e3 / CALLS)
    return out


def child(repeats):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {shape: {variant: [ms per call, ...]}}."""
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    res = {}
    for name, (kw, (in_dim, hidden, nd, act), max_len) in SHAPES.items():
        e = _native.HipEngine(**kw)
        e.set_weights(_capi.make_desc(in_dim, hidden, nd, act), make_weights(34, in_dim, hidden, nd))
        have = "selfplay_nstep_targets" in _native.fns()
        r = {}
        for variant in ("step", "step+keep") if have else ("step",):
            e.selfplay_begin(max_len, False, capacity_steps=CAPACITY, fifo=True)
            if variant == "step+keep":
                e.selfplay_keep_transitions(True)
            for _ in range(CAPACITY):   # (warm-up; fills the ring)
                e.selfplay_step()
            r[variant] = _timed(e, lambda i: e.selfplay_step(), repeats)
        if have:   # (the ring is full and has wrapped; the transitions are kept)
            for n in N_STEPS:
                e.selfplay_nstep_targets(n)
                r[f"nstep{n}"] = _timed(e, lambda i: e.selfplay_nstep_targets(n), repeats)
            r["rows"] = e.selfplay_ring()[0] * kw["n_trees"]
        res[name] = r
        e.close()
    print("RESULT " + json.dumps(res), flush=True)


LAMBDA_NETS, LAMBDA_GAMES = 8, 512
LAMBDA_KW = dict(env_id=0, mode=0, n_trees=LAMBDA_NETS * LAMBDA_GAMES, n_sims=50, c_uct=1.5, gamma=0.99, num_actions=2, seed=34)


def lambda_child(repeats):
    """One library: a JSON line {variant: [ms per call, ...]} over the full ring of the 8-net population."""
    import numpy as np
    import torch
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    e = _native.HipEngine(**LAMBDA_KW)
    e.set_population(LAMBDA_NETS)
    desc = _capi.make_desc(4, [128, 128], 2, "relu")
    for k in range(LAMBDA_NETS):
        e.set_net_weights(k, desc, make_weights(34 + k, 4, [128, 128], 2))
    e.population_selfplay_begin(200, False, capacity_steps=CAPACITY, fifo=True)
    e.selfplay_keep_transitions(True)
    for _ in range(CAPACITY):
        e.selfplay_step()
    r = {"rows": e.selfplay_ring()[0] * LAMBDA_KW["n_trees"]}
    have = "selfplay_lambda_targets" in _native.fns()
    lams = list(np.linspace(0.3, 1.0, LAMBDA_NETS))
    for n in N_STEPS:
        e.selfplay_nstep_targets(n)
        r[f"nstep{n}"] = _timed(e, lambda i: e.selfplay_nstep_targets(n), repeats)
        if have:
            e.selfplay_lambda_targets(n, 0.9)
            r[f"lambda{n}"] = _timed(e, lambda i: e.selfplay_lambda_targets(n, 0.9), repeats)
            e.selfplay_lambda_targets(n, lams)
            r[f"lambda_nets{n}"] = _timed(e, lambda i: e.selfplay_lambda_targets(n, lams), repeats)
    if have:   # the rule table's copy alone: the same bytes from pageable host memory, on a stream of its own kind
        src = torch.zeros(LAMBDA_NETS * 32, dtype=torch.uint8)
        dst = torch.zeros(LAMBDA_NETS * 32, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        out = []
        with torch.cuda.stream(stream):
            for _ in range(repeats + 1):
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    dst.copy_(src, non_blocking=True)
                stream.synchronize()
                out.append((time.perf_counter() - t0) * 1e3 / CALLS)
        r["copy"] = out[1:]
    e.close()
    print("RESULT " + json.dumps(r), flush=True)


def lambda_main(a):
    parent, new = [], []
    for _ in range(a.rounds):
        parent.append(_run_child(os.path.abspath(a.parent_lib), a.repeats, "--lambda-child"))
        new.append(_run_child(None, a.repeats, "--lambda-child"))
    med = statistics.median

    def m(runs, key):
        return med([x for r in runs for x in r[key]])

    def rounds(runs, key):
        return ", ".join(f"{med(r[key]):.4f}" for r in runs)

    lines = [f"lambda_latency: ms per call, host clock around {CALLS} calls + one stream synchronisation; {a.rounds} rounds x {a.repeats} repeats per library,",
             f"parent-commit library and this build in alternating child processes of one run on one MI355X; CartPole 2x128 ReLU, {LAMBDA_NETS} nets x",
             f"{LAMBDA_GAMES} games, FIFO ring of {CAPACITY} steps, full ({new[0]['rows']} stored rows)", ""]
    copy = m(new, "copy")
    for n in N_STEPS:
        p, own = m(parent, f"nstep{n}"), m(new, f"nstep{n}")
        one, nets = m(new, f"lambda{n}"), m(new, f"lambda_nets{n}")
        lines += [f"n_step {n}",
                  f"  parent nstep_targets          {p:9.4f} ms   per-round medians {rounds(parent, f'nstep{n}')}",
                  f"  nstep_targets (this build)    {own:9.4f} ms   ratio to parent {own / p:.3f}",
                  f"  lambda_targets, one rule      {one:9.4f} ms   ratio to parent nstep {one / p:.3f}   per-round medians {rounds(new, f'lambda{n}')}",
                  f"  lambda_targets, 8 net rules   {nets:9.4f} ms   ratio to parent nstep {nets / p:.3f}   per-round medians {rounds(new, f'lambda_nets{n}')}",
                  f"  the 256-byte copy alone       {copy:9.4f} ms   share of the one-rule call {copy / one:.2f}", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


def _run_child(lib, repeats, mode="--child"):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    else:
        env.pop("AZG_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--repeats", str(repeats)], env=env, check=True, capture_output=True,
                         text=True, timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lambda-child", action="store_true")
    ap.add_argument("--lambda-call", action="store_true", help="measure the lambda-return call (default --out: profiles/lambda_latency.txt)")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "lambda_latency.txt" if a.lambda_call else "nstep_latency.txt")
    if a.child:
        return child(a.repeats)
    if a.lambda_child:
        return lambda_child(a.repeats)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the libazgym_hip.so of a build of the parent commit (the yardstick is measured in the same run)")
    if a.lambda_call:
        return lambda_main(a)
    parent, new = [], []
    for _ in range(a.rounds):
        parent.append(_run_child(os.path.abspath(a.parent_lib), a.repeats))
        new.append(_run_child(None, a.repeats))
    med = statistics.median
    lines = [f"nstep_latency: ms per call, host clock around {CALLS} calls + one stream synchronisation; {a.rounds} rounds x {a.repeats} repeats per library,",
             f"parent-commit library and this build in alternating child processes of one run on one MI355X; FIFO ring of {CAPACITY} steps, full", ""]
    for name in SHAPES:
        rounds_p = [med(r[name]["step"]) for r in parent]
        p = med([x for r in parent for x in r[name]["step"]])
        spread = (max(rounds_p) - min(rounds_p)) / p
        n = {v: med([x for r in new for x in r[name][v]]) for v in ["step", "step+keep"] + [f"nstep{k}" for k in N_STEPS]}
        rounds_n = ", ".join(f"{med(r[name]['step']):.4f}" for r in new)
        rounds_k = ", ".join(f"{med(r[name]['step+keep']):.4f}" for r in new)
        keep = n["step+keep"] / p
        lines += [f"{name}   ({new[0][name]['rows']} stored rows)",
                  f"  parent step             {p:9.4f} ms   per-round medians {', '.join(f'{x:.4f}' for x in rounds_p)}   spread {100 * spread:.2f} %",
                  f"  step (nothing kept)     {n['step']:9.4f} ms   ratio to parent {n['step'] / p:.4f}   per-round medians {rounds_n}",
                  f"  step + keep_transitions {n['step+keep']:9.4f} ms   ratio to parent {keep:.4f}   per-round medians {rounds_k}   "
                  f"({'within' if abs(keep - 1) <= spread else 'OUTSIDE'} the parent's spread)"]
        for k in N_STEPS:
            v = n[f"nstep{k}"]
            lines.append(f"  nstep_targets n_step {k:<5d}{v:9.4f} ms   ratio to parent step {v / p:.4f}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
