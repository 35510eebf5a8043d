#!/usr/bin/env python3
"""What a reanalysis of one ring slot costs (azg_selfplay_reanalyse), what keeping the states costs a self-play step, and whether the
default self-play step moved, against a library built from the PARENT commit on the same box in the same run.
GPU box only:
    python tools/reanalyse_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 3] [--out profiles/reanalyse_latency.txt]

Shapes: CartPole 2x128 ReLU x 4096 games x 100 simulations, Pendulum-v1 2x256 ELU x 4096 x 200, Pendulum-v1 4x1024 ELU x 1024 x 50.
Every round starts one child process per library (AZG_HIP_LIB), parent and this build alternating; a child measures, per shape,
    step       selfplay_step, states not kept (both libraries)
    step+keep  selfplay_step after selfplay_keep_states (this build)
    reanalyse  selfplay_reanalyse of one slot, the slots taken in turn (this build)
each as the host clock around 20 calls and ONE stream synchronisation after them, repeated; ms per call.  The table gives medians over
all rounds and repeats, the parent step's spread (max - min of its per-round medians, relative), and the ratios.  The yardstick of a
reanalysis is the parent's step: the same search plus a row kernel that does less, plus one gather launch -- expected ratio <= 1.10,
or the parent step's own spread if that is larger.  With --bench each child's library also runs `python bench.py --gpus 1`."""
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
    "cartpole_2x128_4096x100": (dict(env_id=0, mode=0, n_trees=4096, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34), (4, [128, 128], 2, "relu"), 200),
    "pendulum_2x256_4096x200": (dict(env_id=2, mode=1, n_trees=4096, n_sims=200, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [256, 256], 2, "elu"), 200),
    "pendulum_4x1024_1024x50": (dict(env_id=2, mode=1, n_trees=1024, n_sims=50, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [1024] * 4, 2, "elu"), 200),
}
CALLS, CAPACITY = 20, 8


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
        have = "selfplay_reanalyse" in _native.fns()
        r = {}
        for variant in ("step", "step+keep") if have else ("step",):
            e.selfplay_begin(max_len, False, capacity_steps=CAPACITY, fifo=True)
            if variant == "step+keep":
                e.selfplay_keep_states(True)
            for _ in range(CAPACITY):   # (warm-up; fills the ring)
                e.selfplay_step()
            r[variant] = _timed(e, lambda i: e.selfplay_step(), repeats)
        if have:
            e.selfplay_reanalyse(0, search_index=1 << 31)   # (warm-up: the fresh-root search may be another kernel than the step's)
            r["reanalyse"] = _timed(e, lambda i: e.selfplay_reanalyse(i % CAPACITY, search_index=(1 << 31) + 1 + i), repeats)
            r["form"] = e.search_info()["kernel_name"]
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


def _bench(lib):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env, check=True,
                         capture_output=True, text=True, timeout=600, cwd=ROOT).stdout
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return line["value"], line.get("unit", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_latency.txt"))
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
    lines = [f"reanalyse_latency: ms per call, host clock around {CALLS} calls + one stream synchronisation; {a.rounds} rounds x {a.repeats} repeats per library,",
             "parent-commit library and this build in alternating child processes of one run on one MI355X", ""]
    for name in SHAPES:
        rounds_p = [med(r[name]["step"]) for r in parent]
        p = med([x for r in parent for x in r[name]["step"]])
        spread = (max(rounds_p) - min(rounds_p)) / p
        n = {v: med([x for r in new for x in r[name][v]]) for v in ("step", "step+keep", "reanalyse")}
        margin = max(0.10, spread)
        rounds_n = ", ".join(f"{med(r[name]['step']):.4f}" for r in new)
        lines += [f"{name}   (reanalysis search: {new[0][name]['form']})",
                  f"  parent step            {p:9.4f} ms   per-round medians {', '.join(f'{x:.4f}' for x in rounds_p)}   spread {100 * spread:.2f} %",
                  f"  step (states not kept) {n['step']:9.4f} ms   ratio to parent {n['step'] / p:.4f}   per-round medians {rounds_n}",
                  f"  step + keep_states     {n['step+keep']:9.4f} ms   ratio to parent {n['step+keep'] / p:.4f}",
                  f"  reanalyse one slot     {n['reanalyse']:9.4f} ms   ratio to parent step {n['reanalyse'] / p:.4f}   "
                  f"(expected <= {1 + margin:.2f}: {'within' if n['reanalyse'] / p <= 1 + margin else 'ABOVE'})", ""]
    if a.bench:
        vals = [(_bench(os.path.abspath(a.parent_lib)), _bench(None)) for _ in range(2)]
        lines.append("python bench.py --gpus 1 --steps 20 --warmup 5, `value` (parent, this build), two alternating runs:")
        for (pv, unit), (nv, _) in vals:
            lines.append(f"  parent {pv:.6g}   this build {nv:.6g} {unit}   ratio {nv / pv:.4f}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
