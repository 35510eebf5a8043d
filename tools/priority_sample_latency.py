#!/usr/bin/env python3
"""What the prioritised sampling of a full replay ring costs -- azg_selfplay_priorities, azg_selfplay_sample_rows with n_order = N,
azg_selfplay_sample_slots -- against the self-play step of a library built from the PARENT commit on the same box in the same run, and
against the host path the draws replace (selfplay_rows() download, numpy prefix sum, searchsorted); and what keeping priorities costs
a self-play step.
GPU box only:
    python tools/priority_sample_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 3] [--out profiles/priority_sample_latency.txt]

Shapes (tools/nstep_latency.py's first two): Pendulum-v1 2x256 ELU x 4096 games x 200 simulations, CartPole 2x128 ReLU x 4096 x 100; a
FIFO ring of 64 steps, full (262144 stored rows); as one net of 4096 games and as 64 nets of 64 games.
Every round starts one child process per library (AZG_HIP_LIB), parent and this build alternating; a child measures, per shape,
    step         selfplay_step, nothing kept (both libraries; one net)
    step+keep    selfplay_step after keep_transitions and keep_priorities (this build) against step after keep_transitions alone
    priorities   selfplay_priorities (value gap, alpha 0.6) over the full ring: 20 asynchronous calls, one synchronisation
    sample_rows  selfplay_sample_rows(n_order = N rows per net): scan + draws + one synchronisation + the copy of the order, per call
    sample_slots selfplay_sample_slots: per call, with its synchronisation and copy
    host         what sample_rows replaces: selfplay_rows() of the whole ring, the value gap, (d + eps) ** alpha, per-net cumsum and
                 searchsorted of N uniform draws in numpy
each as the host clock, repeated; ms per call.  Nothing is gated: the figures are a record."""
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

SHAPES = {
    "pendulum_2x256_4096x200": (dict(env_id=2, mode=1, n_trees=4096, n_sims=200, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [256, 256], 2, "elu"), 200),
    "cartpole_2x128_4096x100": (dict(env_id=0, mode=0, n_trees=4096, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34), (4, [128, 128], 2, "relu"), 200),
}
CALLS, CAPACITY = 20, 64
NETS = (1, 64)
ALPHA, EPS = 0.6, 1e-3


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


def _engine(kw, net, n_nets):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    in_dim, hidden, nd, act = net
    e = _native.HipEngine(**kw)
    desc = _capi.make_desc(in_dim, hidden, nd, act)
    if n_nets == 1:
        e.set_weights(desc, make_weights(34, in_dim, hidden, nd))
    else:
        e.set_population(n_nets)
        for k in range(n_nets):
            e.set_net_weights(k, desc, make_weights(34 + k, in_dim, hidden, nd))
    return e


def _host_path(e, n_nets, B):
    """selfplay_rows() + transitions' values -> numpy priorities, per-net prefix sums and N draws per net."""
    rows = e.selfplay_rows(clear=False)
    value = e.selfplay_transitions()["value"]
    d = np.abs(value - rows[:, -1].astype(np.float64)).astype(np.float32)
    p = ((d + np.float32(EPS)) ** np.float32(ALPHA)).astype(np.float64).reshape(-1, n_nets, B // n_nets)
    rng = np.random.default_rng(0)
    out = []
    for k in range(n_nets):
        c = np.cumsum(p[:, k].reshape(-1))
        out.append(np.searchsorted(c, rng.random(c.shape[0]) * c[-1], side="right"))
    return out


def child(repeats):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {shape: {variant: [ms per call, ...]}}."""
    from alphazero_gym_amd import _native
    have = "selfplay_sample_rows" in _native.fns()
    res = {}
    for name, (kw, net, max_len) in SHAPES.items():
        B = kw["n_trees"]
        r = {}
        for n_nets in NETS if have else (1,):
            e = _engine(kw, net, n_nets)
            begin = e.selfplay_begin if n_nets == 1 else e.population_selfplay_begin
            tag = f"@{n_nets}"
            for variant in ("step", "step+tr", "step+keep") if have else ("step",):
                if n_nets != 1 and variant != "step+keep":
                    continue
                begin(max_len, False, capacity_steps=CAPACITY, fifo=True)
                if variant != "step":
                    e.selfplay_keep_transitions(True)
                if variant == "step+keep":
                    e.selfplay_keep_priorities(True)
                for _ in range(CAPACITY):   # (warm-up; fills the ring)
                    e.selfplay_step()
                r[variant + tag] = _timed(e, lambda i: e.selfplay_step(), repeats)
            if have:   # (the ring is full and has wrapped; transitions and priorities are kept)
                n_rows = CAPACITY * (B // n_nets)
                e.selfplay_nstep_targets(5)
                e.selfplay_priorities(ALPHA, EPS)
                r["priorities" + tag] = _timed(e, lambda i: e.selfplay_priorities(ALPHA, EPS), repeats)
                e.selfplay_sample_rows(n_rows, 0)
                r["sample_rows" + tag] = _timed(e, lambda i: e.selfplay_sample_rows(n_rows, i), repeats, calls=5)
                r["sample_rows_small" + tag] = _timed(e, lambda i: e.selfplay_sample_rows(512, i), repeats)
                r["sample_slots" + tag] = _timed(e, lambda i: e.selfplay_sample_slots(i), repeats)
                r["host" + tag] = _timed(e, lambda i: _host_path(e, n_nets, B), max(1, repeats // 2), calls=2)
                r["download" + tag] = _timed(e, lambda i: e.selfplay_rows(clear=False), max(1, repeats // 2), calls=2)
            e.close()
        res[name] = r
    print("RESULT " + json.dumps(res), flush=True)


def _run_child(lib, repeats):
    env = dict(os.environ)
    if lib:
        env["AZG_HIP_LIB"] = lib
    else:
        env.pop("AZG_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priority_sample_latency.txt"))
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
    lines = [f"priority_sample_latency: ms per call, host clock; {a.rounds} rounds x {a.repeats} repeats per library, parent-commit library and this",
             f"build in alternating child processes of one run on one MI355X; FIFO ring of {CAPACITY} steps x 4096 games, full (262144 stored rows)", ""]
    for name in SHAPES:
        def m(v, runs=new):
            return med([x for r in runs for x in r[name][v]])
        rounds_p = [med(r[name]["step@1"]) for r in parent]
        p = m("step@1", parent)
        spread = (max(rounds_p) - min(rounds_p)) / p
        keep = m("step+keep@1") / p
        lines += [name,
                  f"  parent step                         {p:9.4f} ms   per-round medians {', '.join(f'{x:.4f}' for x in rounds_p)}   spread {100 * spread:.2f} %",
                  f"  step (nothing kept)                 {m('step@1'):9.4f} ms   ratio to parent {m('step@1') / p:.4f}",
                  f"  step + keep_transitions             {m('step+tr@1'):9.4f} ms   ratio to parent {m('step+tr@1') / p:.4f}",
                  f"  step + keep_transitions + _priorities {m('step+keep@1'):7.4f} ms   ratio to parent {keep:.4f}   "
                  f"({'within' if abs(keep - 1) <= spread else 'OUTSIDE'} the parent's spread)"]
        for n_nets in NETS:
            t = f"@{n_nets}"
            host = m("host" + t)
            lines.append(f"  {n_nets} net(s) x {4096 // n_nets} games, N = {CAPACITY * 4096 // n_nets} rows per net      (step of this engine: {m('step+keep' + t):.4f} ms)")
            for v, what in (("priorities", "priorities (20 async calls, 1 sync) "), ("sample_rows", "sample_rows n_order = N             "),
                            ("sample_rows_small", "sample_rows n_order = 512           "), ("sample_slots", "sample_slots                        ")):
                x = m(v + t)
                lines.append(f"    {what}{x:9.4f} ms   ratio to parent step {x / p:.4f}   host path / this {host / x:9.1f}")
            lines.append(f"    host path (download + numpy)        {host:9.4f} ms   ratio to parent step {host / p:.4f}   of which selfplay_rows() {m('download' + t):.4f} ms")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
