#!/usr/bin/env python3
"""What one step of a search rollout costs (azg_search_rollout: a search plus the step kernel without a replay row), against the
self-play step of a library built from the PARENT commit on the same box in the same run, and whether the self-play step itself moved.
GPU box only:
    python tools/search_rollout_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 3] [--out profiles/search_rollout_latency.txt]

Shapes: Pendulum-v1 2x256 ELU x 4096 games x 200 simulations, CartPole 2x128 ReLU x 4096 x 100, Pendulum-v1 4x1024 ELU x 1024 x 50.
Every round starts one child process per library (AZG_HIP_LIB), parent and this build alternating; a child measures, per shape,
    step      selfplay_step (both libraries): host clock around 20 calls and ONE stream synchronisation after them
    rollout   search_rollout of one episode of 20 steps per game, no poll before its end (this build): host clock around the call --
              20 searches and step kernels, plus the call's start kernel, its final synchronisation and the copy of its outputs
    rollout40 the same with 40 steps: (40-step call - 20-step call) / 20 is what a further step costs, the rest of the 20-step call
              is the call's fixed part
each repeated; ms per step.  The kernel time of each variant's last search (azg_last_search_ms) and the rollout's episode lengths are
printed beside them: a search's cost depends on the states it starts from, and a game that has ended is parked on a start state.
The table gives medians over all rounds and repeats, the parent step's spread (max - min of its per-round medians, relative) and the
ratios.  The yardstick of a rollout step is the parent's self-play step at the same shape.  The continuous
shapes start every search from a fresh root in both, so about 1.0 is expected there, a little less for the row that is not written;
CartPole's self-play carries the picked child's count into the next root exactly as the rollout does.  With --bench each library also
runs `python bench.py --gpus 1`."""
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
CALLS, CAPACITY = 20, 8


def child(repeats):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {shape: {variant: [ms per step, ...]}}."""
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    res = {}
    for name, (kw, (in_dim, hidden, nd, act), max_len) in SHAPES.items():
        e = _native.HipEngine(**kw)
        e.set_weights(_capi.make_desc(in_dim, hidden, nd, act), make_weights(34, in_dim, hidden, nd))
        r = {"step": []}
        e.selfplay_begin(max_len, False, capacity_steps=CAPACITY, fifo=True)
        for _ in range(CAPACITY):   # (warm-up; fills the ring)
            e.selfplay_step()
        for _ in range(repeats):
            e.sync()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                e.selfplay_step()
            e.sync()
            r["step"].append((time.perf_counter() - t0) * 1e3 / CALLS)
        r["step_kernel"] = e.last_search_ms()
        if "search_rollout" in _native.fns():
            # the self-play's own rule (sampled pi / the arg-max of the counts), one episode of CALLS steps, never polled
            rollout = lambda i, n: e.search_rollout(1, n, deterministic=False, game_id_base=1 << 30, index_base=(3 << 30) + 64 * i, poll_steps=1 << 20)   # noqa: E731
            out = rollout(0, CALLS)   # (warm-up: the buffers, and the first search's kernel)
            r["rollout_steps"] = out["steps"]
            r["rollout_mean_length"] = float(out["lengths"].mean())
            r["rollout"], r["rollout40"] = [], []
            for i in range(repeats):
                for key, n in (("rollout", CALLS), ("rollout40", 2 * CALLS)):
                    e.sync()
                    t0 = time.perf_counter()
                    out = rollout(1 + i, n)
                    r[key].append((time.perf_counter() - t0) * 1e3 / out["steps"])
                    assert out["steps"] == n
                    if key == "rollout":
                        r["rollout_kernel"] = e.last_search_ms()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_rollout_latency.txt"))
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
    lines = [f"search_rollout_latency: ms per step, host clock; self-play: {CALLS} calls + one stream synchronisation; rollout: one call of {CALLS} steps;",
             f"{a.rounds} rounds x {a.repeats} repeats per library, parent-commit library and this build in alternating child processes of one run on one MI355X", ""]
    for name in SHAPES:
        for r in parent + new:   # (one number per child)
            r[name]["step_kernel"] = [r[name]["step_kernel"]]
            if "rollout_kernel" in r[name]:
                r[name]["rollout_kernel"] = [r[name]["rollout_kernel"]]
        rounds_p = [med(r[name]["step"]) for r in parent]
        p = med([x for r in parent for x in r[name]["step"]])
        spread = (max(rounds_p) - min(rounds_p)) / p
        n = {v: med([x for r in new for x in r[name][v]]) for v in ("step", "rollout", "rollout40", "step_kernel", "rollout_kernel")}
        pk = med([x for r in parent for x in r[name]["step_kernel"]])
        further = (2 * CALLS * n["rollout40"] - CALLS * n["rollout"]) / CALLS
        fixed = CALLS * (n["rollout"] - further)
        rounds_n = ", ".join(f"{med(r[name]['step']):.4f}" for r in new)
        rounds_r = ", ".join(f"{med(r[name]['rollout']):.4f}" for r in new)
        ratio = n["rollout"] / p
        lines += [f"{name}   (rollout search: {new[0][name]['form']}; {new[0][name]['rollout_steps']} steps per call)",
                  f"  parent self-play step  {p:9.4f} ms   per-round medians {', '.join(f'{x:.4f}' for x in rounds_p)}   spread {100 * spread:.2f} %",
                  f"  self-play step         {n['step']:9.4f} ms   ratio to parent {n['step'] / p:.4f}   per-round medians {rounds_n}",
                  f"  rollout step           {n['rollout']:9.4f} ms   ratio to parent step {ratio:.4f}   per-round medians {rounds_r}   "
                  f"({'within' if abs(ratio - 1) <= spread else 'above' if ratio > 1 else 'below'} the parent step's spread)",
                  f"  a further rollout step {further:9.4f} ms   ratio to parent step {further / p:.4f}   the call's fixed part {fixed:.4f} ms   (from the {2 * CALLS}-step call: {n['rollout40']:.4f} ms per step)",
                  f"  last search, kernel    parent step {pk:.4f} ms   step {n['step_kernel']:.4f} ms   rollout {n['rollout_kernel']:.4f} ms   "
                  f"(rollout episodes: mean length {new[0][name]['rollout_mean_length']:.2f} of {CALLS} steps, then parked)", ""]
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
