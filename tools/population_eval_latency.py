#!/usr/bin/env python3
"""Time per call of azg_population_mlp_eval: every net of a K-net engine evaluated on n observations each in ONE launch, host form
(numpy in and out) and device form (torch tensors on the GPU, nothing crosses PCIe), against the loop it replaces -- K one-net engines
called with azg_mlp_eval in turn (weights already set, same process), which is all a population's user could do before.
GPU box only:  python tools/population_eval_latency.py [--configs a,b] [--reps 7] [--warmup 2] > profiles/population_eval_latency.txt
Configurations: CartPole 2x128 ReLU and Pendulum 2x256 ELU at K in {1, 8, 64} x n in {16, 1024, 16384}; Pendulum 4x1024 ELU at
K in {1, 4, 16} x n in {32, 1024}.  The clock is the host's, around the synchronising call(s).  Per point the three ways are warmed up,
then measured alternately (host, device, loop, host, ...) in --reps rounds, a round timing as many calls in a row as take about 20 ms
(at most 50): ms per call as the median and min-max over the rounds, and the loop's median over each form's.  The outputs of the three ways are compared bit for bit once per point."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_gym_amd import _capi, _native  # noqa: E402
from alphazero_gym_amd.synthetic import make_weights  # noqa: E402

# name: engine kwargs, (network inputs, hidden widths, distribution outputs, activation), trees per net, the K and n points
CONFIGS = {
    "cartpole_2x128": (dict(env_id=0, mode=0, num_actions=2, n_sims=8, c_uct=1.5, gamma=1.0), (4, [128, 128], 2, "relu"), 1,
                       (1, 8, 64), (16, 1024, 16384)),
    "pendulum_2x256": (dict(env_id=2, mode=1, n_sims=8, c_uct=0.05, gamma=1.0), (3, [256, 256], 2, "elu"), 1,
                       (1, 8, 64), (16, 1024, 16384)),
    # (a population of team-shaped nets needs a multiple of 32 trees per net)
    "pendulum_4x1024": (dict(env_id=2, mode=1, n_sims=8, c_uct=0.05, gamma=1.0), (3, [1024] * 4, 2, "elu"), 32,
                        (1, 4, 16), (32, 1024)),
}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, K, n, reps, warmup):
    kw, (in_dim, hidden, n_dist, act), T, _, _ = CONFIGS[name]
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    blobs = [make_weights(34 + k, in_dim, hidden, n_dist) for k in range(K)]
    pop = _native.HipEngine(**dict(kw, n_trees=K * T))
    if K > 1:
        pop.set_population(K)
        for k in range(K):
            pop.set_net_weights(k, desc, blobs[k])
    else:
        pop.set_weights(desc, blobs[0])
    singles = []
    for k in range(K):
        e = _native.HipEngine(**dict(kw, n_trees=T))
        e.set_weights(desc, blobs[k])
        singles.append(e)
    obs = np.random.default_rng(n).standard_normal((K, n, in_dim)).astype(np.float32)
    d_obs = torch.from_numpy(obs).cuda()
    d_out = tuple(torch.empty(s, device="cuda") for s in ((K, n), (K, n, n_dist), (K, n, 1 + n_dist)))
    ways = {
        "host": lambda: pop.population_mlp_eval(obs),
        "device": lambda: pop.population_mlp_eval_device(d_obs, out=d_out),
        "loop": lambda: [e.mlp_eval(obs[k]) for k, e in enumerate(singles)],
    }
    for _ in range(warmup):
        outs = {w: fn() for w, fn in ways.items()}
    same = all(np.array_equal(outs["host"][i], np.stack([o[i] for o in outs["loop"]])) and
               np.array_equal(outs["host"][i], outs["device"][i].cpu().numpy()) for i in range(3))
    # a round times `calls` calls in a row (each synchronises), enough of them for about 20 ms, and gives ms per call
    calls = {w: int(min(50, max(1, round(20.0 / max(timed(fn)[0], 1e-3))))) for w, fn in ways.items()}
    ms = {w: [] for w in ways}
    for _ in range(reps):
        for w, fn in ways.items():
            t0 = time.perf_counter()
            for _ in range(calls[w]):
                fn()
            ms[w].append((time.perf_counter() - t0) * 1e3 / calls[w])
    info = pop.last_eval_info
    pop.close()
    for e in singles:
        e.close()
    r = dict(config=name, K=K, n=n, reps=reps, same_bits=bool(same), **info)
    for w in ways:
        r[w + "_ms"] = round(float(np.median(ms[w])), 4)
        r[w + "_ms_min"], r[w + "_ms_max"] = round(min(ms[w]), 4), round(max(ms[w]), 4)
    r["loop_over_host"] = round(r["loop_ms"] / r["host_ms"], 2)
    r["loop_over_device"] = round(r["loop_ms"] / r["device_ms"], 2)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=7, help="measured rounds per point (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5 or a.warmup < 1:
        ap.error("--reps must be at least 5 and --warmup at least 1")
    for name in a.configs.split(","):
        if name not in CONFIGS:
            ap.error(f"unknown configuration {name!r}: {', '.join(CONFIGS)}")
    os.environ.setdefault("AZG_QUIET", "1")
    for name in a.configs.split(","):
        print(f"# {name}: ms per call, median (min-max) over {a.reps} alternating rounds after {a.warmup} warm-up rounds; "
              "loop = K one-net engines, azg_mlp_eval in turn")
        print(f"# {'K':>3} {'n':>6} {'groups x tiles':>14} {'res':>3} {'host form':>24} {'device form':>24} {'loop of engines':>26} "
              f"{'loop/host':>9} {'loop/dev':>8}")
        for K in CONFIGS[name][3]:
            for n in CONFIGS[name][4]:
                r = measure(name, K, n, a.reps, a.warmup)
                cell = lambda w: f"{r[w + '_ms']:8.3f} ({r[w + '_ms_min']:.3f}-{r[w + '_ms_max']:.3f})"   # noqa: E731
                print(f"  {K:3d} {n:6d} {r['groups']:6d} x {r['tiles']:5d} {r['resident']:3d} {cell('host'):>24} {cell('device'):>24} "
                      f"{cell('loop'):>26} {r['loop_over_host']:8.2f}x {r['loop_over_device']:7.2f}x"
                      + ("" if r["same_bits"] else "   OUTPUTS DIFFER"))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
