#!/usr/bin/env python3
"""Per-act() latency of K agents at the reference defaults: one population step (AgentPopulation.act: all K trees in one launch)
against the same K agents stepped one by one (agent.act: one launch and three ABI round trips each).
GPU box only:  python tools/population_latency.py [--ks 1,3,8,32,128,256] [--steps 20] [--warmup 3]
Configurations: Pendulum-v0, 3x128 ELU GMM-2 policy, 25 rollouts (run_continuous.py with the reference's GMM); CartPole-v0, 2x128
ReLU, 8 rollouts, epsilon 0.1 (run_discrete.py).  Per K: kernel ms per launch (azg_last_search_ms; one-by-one: the mean of the K
single-tree launches, and their sum), wall ms per population step, wall ms of the K one-by-one act() calls, and the speed-up.
Every act searches from the same fresh root (reset_mcts before each step; the envs are not stepped).

--wide: populations of wide nets (padded width >= 512: team kernel / per-layer launches), engine level:
    python tools/population_latency.py --wide [--splits 1x1024,2x512,4x256,8x128,16x64,32x32] [--steps 5] [--warmup 2]
Configurations: Pendulum-v1 4x1024 ELU x 200 simulations, CartPole 2x512 ReLU x 100 simulations.  Per split K x T: ms per search of
ONE engine that holds the K nets (K x T trees in one search) and the form that ran, against the loop it replaces -- K one-net engines
of T trees searched one after another, each search synchronised before the next starts, which is all an engine could do before
it took several wide nets -- on the same box.

--per-net: per-net MCTS settings (azg_set_net_search), engine level, 64 trees per net:
    python tools/population_latency.py --per-net [--steps 20] [--warmup 3] [--out profiles/population_latency_pernet.txt]
Configurations: CartPole 2x128 ReLU x 100 simulations at K = 1 / 8 / 64 nets, Pendulum-v1 2x256 ELU x 200 simulations at K = 1 / 4 / 16.
Per K, ms per search (kernel time, azg_last_search_ms, and wall time of search()) of (a) ONE engine whose K nets search with K
different settings (search_kernel_nets), (a=) the same with a table whose K entries all equal the shared settings -- the very search
of (b) on the general kernels with the table, so (a=) against (b) is what the mechanism costs, while (a) also searches other trees --
(b) the same engine with the shared settings (the kernel it ran before there was a table, compile-time specialised where one exists),
(c) K one-net engines with net k's settings, searched one after another.  The table is printed and written to --out.

--wide --per-net: the same question for wide nets (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE), 1024 trees in all:
    python tools/population_latency.py --wide --per-net [--splits 2x512,8x128,32x32] [--steps 20] [--warmup 3] [--out profiles/population_latency_wide_pernet.txt]
Configurations: Pendulum-v1 4x1024 ELU x 200 simulations, CartPole 2x512 ReLU x 100 simulations.  Per split, INTERLEAVED -- every
measured round runs (a), (a=), (b), (b) again and (c) once, in that order -- medians of kernel / wall ms per search: (a) one engine, a
table of K distinct c_uct; (a=) the table's entries equal to the shared settings; (b) the same engine without a table, twice, so that
the spread of two runs of the same thing stands next to a/b; (c) K one-net engines with net k's c_uct, one after another.

--per-net-rollouts: per-net simulation budgets (azg_net_search.n_sims) in one launch; with --wide the wide nets' table forms:
    python tools/population_latency.py --per-net-rollouts [--wide] [--steps 10] [--warmup 2] [--out profiles/population_latency_rollouts.txt]
Configurations: CartPole 2x128 x 100 at K = 8 / 64 and Pendulum-v1 2x256 x 200 at K = 4 / 16, 64 trees per net; --wide: Pendulum-v1 4x1024
x 200 over 1024 trees at 2 / 8 / 32 nets.  The nets' budgets run from the capacity down to 1 in equal steps (rollout_budgets); all five
settings are the shared ones.  INTERLEAVED rounds, medians of kernel / wall ms per search: (a) one engine, the K distinct budgets;
(a=) every budget equal to the capacity; (b) the same table without budgets, twice -- (a=) goes in front of that pair in even rounds and
behind it in odd ones; (c) K one-net engines CREATED with net k's budget, one after another.  Simulations per search are the budgets summed over the trees.  --table-only measures (b) alone, four times per round:
run under AZG_HIP_LIB=<another build's library> it gives that build's launch of the same table and its own run-to-run spread."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_gym_amd import run  # noqa: E402
from alphazero_gym_amd.agent.population import AgentPopulation  # noqa: E402
from alphazero_gym_amd.envs import make_game  # noqa: E402
from alphazero_gym_amd.search.mcts import env_signature  # noqa: E402

CONFIGS = {
    "pendulum_3x128_gmm2_25": ("continuous", dict(game="Pendulum-v0", policy=dict(num_components=2))),
    "cartpole_2x128_8": ("discrete", dict(game="CartPole-v0")),
}


def measure(kind, over, K, steps, warmup):
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, over)
    torch.manual_seed(0)
    envs = []
    for k in range(K):
        env = make_game(cfg["game"])
        env.seed(34 + k)
        env.reset()
        envs.append(env)
    agents = [run.make_agent(kind, cfg, envs[k], tree_id_base=k) for k in range(K)]
    pop = AgentPopulation(agents, seeds=[34 + k for k in range(K)])

    def reset():
        for a in agents:
            a.reset_mcts(root_state=None)   # (return_results then takes the observation from the env)

    wall_pop, kern_pop = [], []
    for i in range(warmup + steps):
        reset()
        t0 = time.perf_counter()
        pop.act(envs)
        t1 = time.perf_counter()
        if i >= warmup:
            wall_pop.append((t1 - t0) * 1e3)
            kern_pop.append(pop.mcts.engine.last_search_ms())
    form = pop.mcts.last_search_info
    pop.close()
    wall_seq, kern_seq = [], []
    for i in range(warmup + steps):
        reset()
        ks = []
        t0 = time.perf_counter()
        for a, env in zip(agents, envs):
            a.act(env)
        t1 = time.perf_counter()
        for a, env in zip(agents, envs):
            ks.append(a.mcts._ensure_engine(env_signature(env)[0], 1).engine.last_search_ms())
        if i >= warmup:
            wall_seq.append((t1 - t0) * 1e3)
            kern_seq.append(ks)
    for a in agents:
        if a.mcts._batched is not None:
            a.mcts._batched.close()
    med = lambda x: float(np.median(x))   # noqa: E731
    ks = np.asarray(kern_seq)
    return dict(K=K, kernel_ms_population=round(med(kern_pop), 4), wall_ms_population_step=round(med(wall_pop), 3),
                kernel_ms_one_by_one_mean=round(float(np.median(ks.mean(1))), 4), kernel_ms_one_by_one_sum=round(float(np.median(ks.sum(1))), 3),
                wall_ms_one_by_one=round(med(wall_seq), 3), speedup_wall=round(med(wall_seq) / med(wall_pop), 2),
                kernel=form["kernel_name"], waves=form.get("waves"), tile_trees=form.get("tile_trees"))


# name: engine kwargs, (network inputs, hidden widths, distribution outputs, activation)
WIDE_CONFIGS = {
    "pendulum_4x1024_200": (dict(env_id=2, mode=1, n_sims=200, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [1024] * 4, 2, "elu")),
    "cartpole_2x512_100": (dict(env_id=0, mode=0, num_actions=2, n_sims=100, c_uct=1.5, gamma=1.0, seed=34), (4, [512, 512], 2, "relu")),
}
WIDE_SPLITS = "1x1024,2x512,4x256,8x128,16x64,32x32"


def parse_splits(spec):
    """"2x512,4x256" -> [(2, 512), (4, 256)]: K nets x T trees per net; T a multiple of 32 wherever K > 1 (a team serves one net)."""
    out = []
    for part in spec.split(","):
        k, t = (int(x) for x in part.lower().split("x"))
        if k < 1 or t < 1 or (k > 1 and t % 32):
            raise ValueError(f"split {part!r}: K nets x T trees per net, T a multiple of 32 when K > 1")
        out.append((k, t))
    return out


def measure_wide(name, K, T, steps, warmup):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, n_dist, act) = WIDE_CONFIGS[name]
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    blobs = [make_weights(34 + k, in_dim, hidden, n_dist) for k in range(K)]
    pop = _native.HipEngine(**dict(kw, n_trees=K * T))
    if K > 1:
        pop.set_population(K)
        for k in range(K):
            pop.set_net_weights(k, desc, blobs[k])
    else:
        pop.set_weights(desc, blobs[0])
    roots = pop.synthetic_roots()
    kern_pop, wall_pop = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        pop.search(roots)
        t1 = time.perf_counter()
        if i >= warmup:
            wall_pop.append((t1 - t0) * 1e3)
            kern_pop.append(pop.last_search_ms())
    info = pop.search_info()
    pop.close()
    singles = []
    for k in range(K):
        e = _native.HipEngine(**dict(kw, n_trees=T, tree_id_base=k * T))
        e.set_weights(desc, blobs[k])
        singles.append(e)
    kern_seq, wall_seq = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        for k, e in enumerate(singles):
            e.search(roots[k * T:(k + 1) * T])
        t1 = time.perf_counter()
        if i >= warmup:
            wall_seq.append((t1 - t0) * 1e3)
            kern_seq.append(sum(e.last_search_ms() for e in singles))
    form1 = singles[0].search_info()
    for e in singles:
        e.close()
    med = lambda x: float(np.median(x))   # noqa: E731
    return dict(K=K, T=T, kernel_ms_population=round(med(kern_pop), 3), wall_ms_population=round(med(wall_pop), 3), form=info["kernel_form"],
                kernel=info["kernel_name"], team_fallbacks=info["team_fallbacks"], kernel_ms_loop=round(med(kern_seq), 3),
                wall_ms_loop=round(med(wall_seq), 3), loop_form=form1["kernel_form"], speedup_wall=round(med(wall_seq) / med(wall_pop), 2))


# name: engine kwargs, (network inputs, hidden widths, distribution outputs, activation), the K values
PER_NET_CONFIGS = {
    "cartpole_2x128_100": (dict(env_id=0, mode=0, num_actions=2, n_sims=100, c_uct=1.5, gamma=1.0, seed=34), (4, [128, 128], 2, "relu"), (1, 8, 64)),
    "pendulum_2x256_200": (dict(env_id=2, mode=1, n_sims=200, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34), (3, [256, 256], 2, "elu"), (1, 4, 16)),
}
PER_NET_TREES = 64


def per_net_settings(kw, K):
    """K different settings around the configuration's own: c_uct over a factor of 16, gamma 1.0 / 0.99 / 0.97 in turn (the closed-form
    backup and the general chain in one launch); epsilon and the widening stay the configuration's."""
    out = []
    for k in range(K):
        f = 4.0 ** (2.0 * k / max(K - 1, 1) - 1.0) if K > 1 else 2.0
        out.append(dict(c_uct=kw["c_uct"] * f, gamma=(1.0, 0.99, 0.97)[k % 3], epsilon=0.0, c_pw=kw.get("c_pw", 1.0), kappa=kw.get("kappa", 0.5)))
    return out


def _timed_searches(search, ms, steps, warmup):
    kern, wall = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        search()
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e3)
            kern.append(ms())
    return float(np.median(kern)), float(np.median(wall))


def measure_per_net(name, K, steps, warmup):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, n_dist, act), _ = PER_NET_CONFIGS[name]
    T = PER_NET_TREES
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    blobs = [make_weights(34 + k, in_dim, hidden, n_dist) for k in range(K)]
    settings = per_net_settings(kw, K)
    pop = _native.HipEngine(**dict(kw, n_trees=K * T))
    if K > 1:
        pop.set_population(K)
        for k in range(K):
            pop.set_net_weights(k, desc, blobs[k])
    else:
        pop.set_weights(desc, blobs[0])
    roots = pop.synthetic_roots()
    b_kern, b_wall = _timed_searches(lambda: pop.search(roots), pop.last_search_ms, steps, warmup)
    b_name = pop.search_info()["kernel_name"]
    shared = dict(c_uct=kw["c_uct"], gamma=kw["gamma"], epsilon=kw.get("epsilon", 0.0), c_pw=kw.get("c_pw", 1.0), kappa=kw.get("kappa", 0.5))
    pop.set_net_search([shared] * K)
    e_kern, e_wall = _timed_searches(lambda: pop.search(roots), pop.last_search_ms, steps, warmup)
    pop.set_net_search(settings)
    a_kern, a_wall = _timed_searches(lambda: pop.search(roots), pop.last_search_ms, steps, warmup)
    a_name = pop.search_info()["kernel_name"]
    pop.close()
    singles = []
    for k in range(K):
        st = {key: v for key, v in settings[k].items() if kw["mode"] == 1 or key not in ("c_pw", "kappa")}
        e = _native.HipEngine(**dict(kw, n_trees=T, tree_id_base=k * T, **st))
        e.set_weights(desc, blobs[k])
        singles.append(e)

    def loop():
        for k, e in enumerate(singles):
            e.search(roots[k * T:(k + 1) * T])

    c_kern, c_wall = _timed_searches(loop, lambda: sum(e.last_search_ms() for e in singles), steps, warmup)
    for e in singles:
        e.close()
    return dict(K=K, T=T, a_kernel_ms=round(a_kern, 4), a_wall_ms=round(a_wall, 3), a_kernel=a_name, a_equal_kernel_ms=round(e_kern, 4),
                a_equal_wall_ms=round(e_wall, 3), b_kernel_ms=round(b_kern, 4),
                b_wall_ms=round(b_wall, 3), b_kernel=b_name, c_kernel_ms=round(c_kern, 4), c_wall_ms=round(c_wall, 3))


WIDE_PER_NET_SPLITS = "2x512,8x128,32x32"


def measure_wide_per_net(name, K, T, steps, warmup):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, n_dist, act) = WIDE_CONFIGS[name]
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    blobs = [make_weights(34 + k, in_dim, hidden, n_dist) for k in range(K)]
    shared = dict(c_uct=kw["c_uct"], gamma=kw["gamma"], epsilon=0.0, c_pw=kw.get("c_pw", 1.0), kappa=kw.get("kappa", 0.5))
    settings = [dict(shared, c_uct=kw["c_uct"] * 4.0 ** (2.0 * k / (K - 1) - 1.0)) for k in range(K)]   # c_uct over a factor of 16
    pop = _native.HipEngine(**dict(kw, n_trees=K * T))
    pop.set_population(K)
    for k in range(K):
        pop.set_net_weights(k, desc, blobs[k])
    roots = pop.synthetic_roots()
    singles = []
    for k in range(K):
        st = {key: v for key, v in settings[k].items() if kw["mode"] == 1 or key not in ("c_pw", "kappa")}
        e = _native.HipEngine(**dict(kw, n_trees=T, tree_id_base=k * T, **st))
        e.set_weights(desc, blobs[k])
        singles.append(e)

    def loop():
        for k, e in enumerate(singles):
            e.search(roots[k * T:(k + 1) * T])

    runs = {key: ([], []) for key in ("a", "a_equal", "b", "b_again", "c")}
    names = {}

    def timed(key, search, ms):
        t0 = time.perf_counter()
        search()
        t1 = time.perf_counter()
        return key, ms(), (t1 - t0) * 1e3

    for i in range(warmup + steps):
        out = []
        pop.set_net_search(settings, wide=True)
        out.append(timed("a", lambda: pop.search(roots), pop.last_search_ms))
        names["a"] = pop.search_info()
        pop.set_net_search([shared] * K, wide=True)
        out.append(timed("a_equal", lambda: pop.search(roots), pop.last_search_ms))
        pop.set_net_search(None)
        out.append(timed("b", lambda: pop.search(roots), pop.last_search_ms))
        names["b"] = pop.search_info()
        out.append(timed("b_again", lambda: pop.search(roots), pop.last_search_ms))
        out.append(timed("c", loop, lambda: sum(e.last_search_ms() for e in singles)))
        if i >= warmup:
            for key, kern, wall in out:
                runs[key][0].append(kern)
                runs[key][1].append(wall)
    pop.close()
    for e in singles:
        e.close()
    r = dict(K=K, T=T, a_kernel=names["a"]["kernel_name"], b_kernel=names["b"]["kernel_name"],
             team_fallbacks=names["a"]["team_fallbacks"] + names["b"]["team_fallbacks"])
    for key, (kern, wall) in runs.items():
        r[key + "_kernel_ms"], r[key + "_wall_ms"] = round(float(np.median(kern)), 4), round(float(np.median(wall)), 3)
    return r


def rollout_budgets(capacity, K):
    """K budgets from the capacity down to 1 in equal steps (K = 1: the capacity)."""
    if K == 1:
        return [capacity]
    return [int(round(capacity - k * (capacity - 1) / (K - 1))) for k in range(K)]


def measure_rollouts(name, K, T, steps, warmup, wide, table_only=False):
    from alphazero_gym_amd import _capi, _native
    from alphazero_gym_amd.synthetic import make_weights
    kw, (in_dim, hidden, n_dist, act) = WIDE_CONFIGS[name] if wide else PER_NET_CONFIGS[name][:2]
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    blobs = [make_weights(34 + k, in_dim, hidden, n_dist) for k in range(K)]
    shared = dict(c_uct=kw["c_uct"], gamma=kw["gamma"], epsilon=kw.get("epsilon", 0.0), c_pw=kw.get("c_pw", 1.0), kappa=kw.get("kappa", 0.5))
    budgets = rollout_budgets(kw["n_sims"], K)
    pop = _native.HipEngine(**dict(kw, n_trees=K * T))
    pop.set_population(K)
    for k in range(K):
        pop.set_net_weights(k, desc, blobs[k])
    roots = pop.synthetic_roots()
    singles = []
    for k in range(0 if table_only else K):
        e = _native.HipEngine(**dict(kw, n_trees=T, tree_id_base=k * T, n_sims=budgets[k]))
        e.set_weights(desc, blobs[k])
        singles.append(e)

    def loop():
        for k, e in enumerate(singles):
            e.search(roots[k * T:(k + 1) * T])

    keys = ("b", "b_again", "b_3", "b_4") if table_only else ("a", "a_equal", "b", "b_again", "c")
    runs = {key: ([], []) for key in keys}
    names = {}

    def timed(key, search, ms):
        t0 = time.perf_counter()
        search()
        t1 = time.perf_counter()
        return key, ms(), (t1 - t0) * 1e3

    search = lambda: pop.search(roots)   # noqa: E731
    def equal_budgets(out):
        pop.set_net_search([shared] * K, wide=wide, n_sims=[kw["n_sims"]] * K)
        out.append(timed("a_equal", search, pop.last_search_ms))

    for i in range(warmup + steps):
        out = []
        if not table_only:
            pop.set_net_search([shared] * K, wide=wide, n_sims=budgets)
            out.append(timed("a", search, pop.last_search_ms))
            names["a"] = pop.search_info()
            if i % 2 == 0:   # (a=) and the (b) pair upload the same records: they swap places every round, so that neither always follows (a)
                equal_budgets(out)
        pop.set_net_search([shared] * K, wide=wide)
        for key in keys:
            if key.startswith("b"):
                out.append(timed(key, search, pop.last_search_ms))
        names["b"] = pop.search_info()
        if not table_only and i % 2 == 1:
            equal_budgets(out)
        if not table_only:
            out.append(timed("c", loop, lambda: sum(e.last_search_ms() for e in singles)))
        if i >= warmup:
            for key, kern, wall in out:
                runs[key][0].append(kern)
                runs[key][1].append(wall)
    pop.close()
    for e in singles:
        e.close()
    r = dict(K=K, T=T, capacity=kw["n_sims"], budgets=budgets, sims_per_search_a=sum(budgets) * T, sims_per_search_b=kw["n_sims"] * K * T,
             b_kernel=names["b"]["kernel_name"], team_fallbacks=sum(n["team_fallbacks"] for n in names.values()))
    for key, (kern, wall) in runs.items():
        r[key + "_kernel_ms"], r[key + "_wall_ms"] = round(float(np.median(kern)), 4), round(float(np.median(wall)), 3)
    return r


def main_rollouts(a):
    what = "widths >= 512, AZG_NET_SEARCH_WIDE; K nets x T trees = 1024 trees" if a.wide else f"{PER_NET_TREES} trees per net"
    lines = [f"# per-net simulation budgets in one launch (azg_net_search.n_sims; {what}): ms per search, kernel / wall,",
             f"# medians over {a.steps} interleaved rounds after {a.warmup} warm-up rounds; budgets from the capacity down to 1 in equal steps",
             "# (a) one engine, K distinct budgets   (a=) every budget equal to the capacity   (b), (b') the same table without budgets, twice per round",
             "# (round order: a, a=, b, b', c in even rounds and a, b, b', a=, c in odd ones)",
             "# (c) K one-net engines created with net k's budget, one after another   M sims/s: (a)'s budgets summed over its trees / its kernel time"]
    if a.table_only:
        lines = [f"# the table without budgets alone, four launches per round ({what}): kernel ms per search, medians over {a.steps} rounds after "
                 f"{a.warmup}; library: {os.environ.get('AZG_HIP_LIB') or 'this build'}"]
    for name in a.configs.split(","):
        lines.append(f"# {name}")
        if a.table_only:
            lines.append(f"# {'K x T':>9} {'(b)':>9} {'(b)':>9} {'(b)':>9} {'(b)':>9} {'max/min':>8}")
        else:
            lines.append(f"# {'K x T':>9} {'(a) budgets ms':>20} {'(a=) capacity ms':>20} {'(b) no budgets ms':>20} {'(b) again ms':>20} {'(c) K engines ms':>20} "
                         f"{'a/b':>7} {'a=/b':>7} {'b/b':>7} {'c/a kern':>9} {'c/a wall':>9} {'(a) M sims/s':>12}")
        points = parse_splits(a.splits) if a.wide else [(K, PER_NET_TREES) for K in PER_NET_CONFIGS[name][2] if K > 1]
        for K, T in points:
            r = measure_rollouts(name, K, T, a.steps, a.warmup, a.wide, a.table_only)
            if a.table_only:
                ms = [r[key + "_kernel_ms"] for key in ("b", "b_again", "b_3", "b_4")]
                lines.append(f"  {K:3d} x {T:4d} " + " ".join(f"{m:9.4f}" for m in ms) + f" {max(ms) / min(ms):7.3f}x")
            else:
                cell = lambda key: f"{r[key + '_kernel_ms']:9.4f} / {r[key + '_wall_ms']:8.3f}"   # noqa: E731
                lines.append(f"  {K:3d} x {T:4d} {cell('a')} {cell('a_equal')} {cell('b')} {cell('b_again')} {cell('c')} "
                             f"{r['a_kernel_ms'] / r['b_kernel_ms']:6.3f}x {r['a_equal_kernel_ms'] / r['b_kernel_ms']:6.3f}x "
                             f"{r['b_again_kernel_ms'] / r['b_kernel_ms']:6.3f}x {r['c_kernel_ms'] / r['a_kernel_ms']:8.2f}x "
                             f"{r['c_wall_ms'] / r['a_wall_ms']:8.2f}x {r['sims_per_search_a'] / r['a_kernel_ms'] / 1e3:12.1f}")
            lines.append(json.dumps(dict(config=name, **r)))
            print("\n".join(lines[-2:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main_wide_per_net(a):
    lines = ["# per-net MCTS settings of wide nets in one search (azg_set_net_search_ex, AZG_NET_SEARCH_WIDE): ms per search, kernel / wall,",
             f"# medians over {a.steps} interleaved rounds after {a.warmup} warm-up rounds; K nets x T trees = 1024 trees",
             "# (a) one engine, a table of K distinct c_uct   (a=) its entries equal to the shared settings   (b), (b') the same engine without a",
             "# table (the shared-settings kernel), measured twice per round   (c) K one-net engines with net k's c_uct, one after another"]
    for name in a.configs.split(","):
        lines.append(f"# {name}")
        lines.append(f"# {'K x T':>9} {'(a) per-net ms':>20} {'(a=) equal ms':>20} {'(b) shared ms':>20} {'(b) again ms':>20} {'(c) K engines ms':>20} "
                     f"{'a/b':>7} {'a=/b':>7} {'b/b':>7} {'c/a wall':>9}")
        for K, T in parse_splits(a.splits):
            r = measure_wide_per_net(name, K, T, a.steps, a.warmup)
            cell = lambda key: f"{r[key + '_kernel_ms']:9.3f} / {r[key + '_wall_ms']:8.3f}"   # noqa: E731
            lines.append(f"  {K:3d} x {T:4d} {cell('a')} {cell('a_equal')} {cell('b')} {cell('b_again')} {cell('c')} "
                         f"{r['a_kernel_ms'] / r['b_kernel_ms']:6.3f}x {r['a_equal_kernel_ms'] / r['b_kernel_ms']:6.3f}x "
                         f"{r['b_again_kernel_ms'] / r['b_kernel_ms']:6.3f}x {r['c_wall_ms'] / r['a_wall_ms']:8.2f}x")
            lines.append(json.dumps(dict(config=name, **r)))
            print("\n".join(lines[-2:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main_per_net(a):
    lines = ["# per-net MCTS settings in one launch (azg_set_net_search): ms per search, kernel / wall, medians over "
             f"{a.steps} searches after {a.warmup} warm-up searches; {PER_NET_TREES} trees per net",
             "# (a) one engine, K nets with K different settings (search_kernel_nets)   (a=) the same, K entries equal to the shared settings:",
             "# the search of (b) on the general kernels with the table   (b) the same engine, shared settings (its kernel without a table)",
             "# (c) K one-net engines with net k's settings, one after another"]
    for name in a.configs.split(","):
        lines.append(f"# {name}")
        lines.append(f"# {'K':>4} {'(a) per-net ms':>22} {'(a=) equal entries ms':>22} {'(b) shared ms':>22} {'(c) K engines ms':>22} {'a=/b kernel':>12} {'c/a wall':>9}")
        for K in PER_NET_CONFIGS[name][2]:
            r = measure_per_net(name, K, a.steps, a.warmup)
            lines.append(f"  {K:4d} {r['a_kernel_ms']:10.4f} / {r['a_wall_ms']:9.3f} {r['a_equal_kernel_ms']:10.4f} / {r['a_equal_wall_ms']:9.3f} "
                         f"{r['b_kernel_ms']:10.4f} / {r['b_wall_ms']:9.3f} {r['c_kernel_ms']:10.4f} / {r['c_wall_ms']:9.3f} "
                         f"{r['a_equal_kernel_ms'] / r['b_kernel_ms']:11.3f}x {r['c_wall_ms'] / r['a_wall_ms']:8.2f}x")
            lines.append(json.dumps(dict(config=name, **r)))
            print("\n".join(lines[-2:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main_wide(a):
    for name in a.configs.split(","):
        print(f"# {name}: medians over {a.steps} searches (after {a.warmup} warm-up searches); loop = K one-net engines of T trees, one after another")
        print(f"# {'K x T':>9} {'population ms (kernel / wall)':>30} {'form':>10} {'loop ms (kernel / wall)':>26} {'speed-up':>9}")
        for K, T in parse_splits(a.splits):
            r = measure_wide(name, K, T, a.steps, a.warmup)
            print(f"  {K:3d} x {T:4d} {r['kernel_ms_population']:14.3f} / {r['wall_ms_population']:11.3f} {r['form']:>10} "
                  f"{r['kernel_ms_loop']:12.3f} / {r['wall_ms_loop']:9.3f} {r['speedup_wall']:8.2f}x")
            print(json.dumps(dict(config=name, **r)), flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="1,3,8,32,128,256")
    ap.add_argument("--steps", type=int, default=None, help="measured steps per point (default 20; --wide: 5)")
    ap.add_argument("--warmup", type=int, default=None, help="warm-up steps per point (default 3; --wide: 2)")
    ap.add_argument("--wide", action="store_true", help="the wide configurations: one engine of K nets against K one-net engines in a loop")
    ap.add_argument("--splits", default=None, help=f"--wide: the K x T points (default {WIDE_SPLITS}; with --per-net {WIDE_PER_NET_SPLITS})")
    ap.add_argument("--per-net", action="store_true", help="per-net MCTS settings: one launch of K settings against shared settings and K engines")
    ap.add_argument("--per-net-rollouts", action="store_true",
                    help="per-net simulation budgets: one launch of K budgets against the table without budgets and K engines (also with --wide)")
    ap.add_argument("--table-only", action="store_true", help="--per-net-rollouts: only the table without budgets, four launches per round")
    ap.add_argument("--out", default=None, help="--per-net: the file the table is written to (default profiles/population_latency_pernet.txt; "
                                                "with --wide profiles/population_latency_wide_pernet.txt)")
    ap.add_argument("--configs", default=None)
    a = ap.parse_args(argv)
    known = WIDE_CONFIGS if a.wide else PER_NET_CONFIGS if a.per_net else CONFIGS
    profiles = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    if a.per_net_rollouts:
        known = {"pendulum_4x1024_200": WIDE_CONFIGS["pendulum_4x1024_200"]} if a.wide and not a.configs else known if a.wide else PER_NET_CONFIGS
        a.out = a.out or os.path.join(profiles, "population_latency_rollouts_wide.txt" if a.wide else "population_latency_rollouts.txt")
    a.out = a.out or os.path.join(profiles, "population_latency_wide_pernet.txt" if a.wide else "population_latency_pernet.txt")
    a.splits = a.splits or (WIDE_PER_NET_SPLITS if a.per_net or a.per_net_rollouts else WIDE_SPLITS)
    a.configs = a.configs or ",".join(known)
    for name in a.configs.split(","):
        if name not in known:
            ap.error(f"unknown configuration {name!r}: {', '.join(known)}")
    if a.wide:
        try:
            if any(k < 2 for k, _ in parse_splits(a.splits)) and (a.per_net or a.per_net_rollouts):
                raise ValueError("--wide --per-net compares K >= 2 nets")
        except ValueError as err:
            ap.error(str(err))
    if a.per_net_rollouts:
        a.steps = a.steps if a.steps is not None else 10
        a.warmup = a.warmup if a.warmup is not None else 2
    a.steps = a.steps if a.steps is not None else (5 if a.wide and not a.per_net else 20)
    a.warmup = a.warmup if a.warmup is not None else (2 if a.wide and not a.per_net else 3)
    return a


def main():
    a = parse_args()
    os.environ.setdefault("AZG_QUIET", "1")
    if a.per_net_rollouts:
        return main_rollouts(a)
    if a.wide and a.per_net:
        return main_wide_per_net(a)
    if a.wide:
        return main_wide(a)
    if a.per_net:
        return main_per_net(a)
    for name in a.configs.split(","):
        kind, over = CONFIGS[name]
        print(f"# {name}: medians over {a.steps} steps (after {a.warmup} warm-up steps)")
        print(f"# {'K':>4} {'kernel ms':>10} {'pop step ms':>12} {'1-by-1 kernel ms (mean / sum)':>30} {'1-by-1 wall ms':>15} {'speed-up':>9}")
        for K in [int(k) for k in a.ks.split(",")]:
            r = measure(kind, over, K, a.steps, a.warmup)
            print(f"  {K:4d} {r['kernel_ms_population']:10.4f} {r['wall_ms_population_step']:12.3f} "
                  f"{r['kernel_ms_one_by_one_mean']:14.4f} / {r['kernel_ms_one_by_one_sum']:11.3f} {r['wall_ms_one_by_one']:15.3f} "
                  f"{r['speedup_wall']:8.2f}x")
            print(json.dumps(dict(config=name, **r)), flush=True)


if __name__ == "__main__":
    main()
