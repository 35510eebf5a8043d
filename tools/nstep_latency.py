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
Nothing is gated: the figures are a record."""
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


def _run_child(lib, repeats):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    else:
        env.pop("AZG_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)], env=env, check=True, capture_output=True,
                         text=True, timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_latency.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.repeats)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the libazgym_hip.so of a build of the parent commit (the yardstick is measured in the same run)")
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
