#!/usr/bin/env python3
"""What a refresh of the whole ring's bootstrap values costs (azg_selfplay_refresh_values) against the two ways the PARENT commit's
library has to get there, measured on that library in the same run on the same box:
    (a) eval       azg_population_mlp_eval_device on a contiguous device tensor with the same number of rows per net: the same
                   arithmetic without the strided reads from the ring and the float64 stores into the kept column
    (b) reanalyse  azg_selfplay_reanalyse of every stored slot, one after the other: the only way the parent can refresh the column
and whether the self-play step and the plain benchmark moved.  GPU box only:
    python tools/value_refresh_latency.py --parent-lib <parent build's libazgym_hip.so> [--rounds 2] [--out profiles/value_refresh_latency.txt]

Shapes: a full ring of 64 steps of CartPole 2x128 ReLU x 4096 games x 100 simulations, Pendulum-v1 2x256 ELU x 4096 x 200 and
Pendulum-v1 4x1024 ELU x 1024 x 50, each as one net and as a population (64, 16 and 4 nets).  Every round starts one child process per
library (AZG_HIP_LIB), parent and this build alternating.  After a warm-up call, each figure is the host clock around CALLS calls and ONE
stream synchronisation after them, repeated; ms per call (a reanalysis "call": all 64 slots).  The table gives medians over all rounds and
repeats with the spread of the per-round medians (max - min, relative).  With --bench each library also runs `python bench.py --gpus 1`."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CART = dict(env_id=0, mode=0, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2, seed=34)
PEND = dict(env_id=2, mode=1, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34)
# name: (engine settings, network, nets of the population form)
SHAPES = {
    "cartpole_2x128_64x4096": (dict(CART, n_trees=4096), (4, [128, 128], 2, "relu"), 64),
    "pendulum_2x256_64x4096": (dict(PEND, n_trees=4096, n_sims=200), (3, [256, 256], 2, "elu"), 16),
    "pendulum_4x1024_64x1024": (dict(PEND, n_trees=1024, n_sims=50), (3, [1024] * 4, 2, "elu"), 4),
}
CALLS, CAPACITY, MAX_LEN = 10, 64, 200


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


def child(repeats, only):
    """One library (AZG_HIP_LIB or this tree's): a JSON line {shape/nets: {variant: [ms per call, ...]}}."""
    import torch
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    have = "selfplay_refresh_values" in _native.fns()
    res = {}
    for name, (kw, (in_dim, hidden, nd, act), pop) in SHAPES.items():
        if only and name not in only:
            continue
        for K in (1, pop):
            e = _native.HipEngine(**kw)
            desc = _capi.make_desc(in_dim, hidden, nd, act)
            if K == 1:
                e.set_weights(desc, make_weights(34, in_dim, hidden, nd))
                e.selfplay_begin(MAX_LEN, False, capacity_steps=CAPACITY, fifo=True)
            else:
                e.set_population(K)
                for k in range(K):
                    e.set_net_weights(k, desc, make_weights(34 + k, in_dim, hidden, nd))
                e.population_selfplay_begin(MAX_LEN, False, capacity_steps=CAPACITY, fifo=True)
            e.selfplay_keep_states(True)
            e.selfplay_keep_transitions(True)
            for _ in range(CAPACITY):   # (warm-up; fills the ring)
                e.selfplay_step()
            r = {"step": _timed(e, lambda i: e.selfplay_step(), repeats)}
            if have:
                e.selfplay_refresh_values()   # (warm-up: the kernel's first launch sets its attributes)
                r["refresh"] = _timed(e, lambda i: e.selfplay_refresh_values(), repeats)
            else:
                n = CAPACITY * kw["n_trees"] // K
                obs = torch.randn(K, n, in_dim, device="cuda", dtype=torch.float32)
                out = (torch.empty(K, n, device="cuda"), torch.empty(K, n, nd, device="cuda"), torch.empty(K, n, 1 + nd, device="cuda"))
                torch.cuda.synchronize()
                fn, info = e._f["population_mlp_eval_device"], _capi.AzgEvalInfo()
                info.struct_size = _capi.C.sizeof(_capi.AzgEvalInfo)

                def ev(i):   # (value only, as the refresh: the call synchronises the stream itself)
                    e._check(fn(e._h, obs.data_ptr(), n, 0, out[0].data_ptr(), None, None, _capi.C.byref(info)))
                ev(0)
                r["eval"] = _timed(e, ev, repeats)
                e.selfplay_reanalyse(0, search_index=1 << 31)   # (warm-up: the fresh-root search may be another kernel than the step's)

                def reanalyse_all(i):
                    for s in range(CAPACITY):
                        e.selfplay_reanalyse(s, search_index=(1 << 31) + 1 + s)
                r["reanalyse"] = _timed(e, reanalyse_all, max(1, repeats // 2), calls=1)
            res[f"{name}/{K}"] = r
            e.close()
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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--only", nargs="+", default=None, help="shape names (default: all)")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "value_refresh_latency.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.repeats, a.only)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the libazgym_hip.so of a build of the parent commit (both baselines are measured on it, in the same run)")
    parent, new = [], []
    for _ in range(a.rounds):
        parent.append(_run_child(os.path.abspath(a.parent_lib), a.repeats, a.only))
        new.append(_run_child(None, a.repeats, a.only))
    med = statistics.median

    def stat(runs, key, variant):
        per_round = [med(r[key][variant]) for r in runs]
        m = med([x for r in runs for x in r[key][variant]])
        return m, (max(per_round) - min(per_round)) / m

    lines = [f"value_refresh_latency: ms per call, host clock around {CALLS} calls + one stream synchronisation (reanalyse: one pass over all",
             f"{CAPACITY} slots); {a.rounds} rounds x {a.repeats} repeats per library, parent-commit library and this build in alternating child",
             f"processes of one run on one MI355X.  A full ring of {CAPACITY} steps; spread: max - min of the per-round medians, relative.", ""]
    for key in parent[0]:
        name, K = key.split("/")
        rows = CAPACITY * SHAPES[name][0]["n_trees"]
        ev, ev_s = stat(parent, key, "eval")
        ra, ra_s = stat(parent, key, "reanalyse")
        ps, ps_s = stat(parent, key, "step")
        rf, rf_s = stat(new, key, "refresh")
        ns, ns_s = stat(new, key, "step")
        lines += [f"{name}   nets {K}   ({rows} rows, {rows // int(K)} per net)",
                  f"  refresh, this build           {rf:10.4f} ms   spread {100 * rf_s:5.2f} %",
                  f"  (a) eval, parent              {ev:10.4f} ms   spread {100 * ev_s:5.2f} %   refresh / (a) {rf / ev:.4f}"
                  f"   ({'inside' if abs(rf / ev - 1.0) <= max(ev_s, rf_s) else 'outside'} the larger spread)",
                  f"  (b) reanalyse {CAPACITY} slots, parent {ra:10.4f} ms   spread {100 * ra_s:5.2f} %   (b) / refresh {ra / rf:.1f}",
                  f"  selfplay step  parent {ps:9.4f} ms (spread {100 * ps_s:.2f} %)   this build {ns:9.4f} ms (spread {100 * ns_s:.2f} %)   "
                  f"ratio {ns / ps:.4f}", ""]
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
