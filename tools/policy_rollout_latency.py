#!/usr/bin/env python3
"""Latency of a policy rollout (azg_policy_rollout: whole episodes of every net in one launch) against the host loop a user has to
write without it: one azg_mlp_eval round trip per environment step plus the numpy envs, on a one-net engine (azg_mlp_eval does
not serve populations, so K nets cost K such loops).
GPU box only:  python tools/policy_rollout_latency.py [--ks 1,8,64] [--episodes 64] [--reps 10] [--out profiles/policy_rollout_latency.txt]
Configurations: CartPole-v0, 2x128 ReLU discrete head; Pendulum-v1, 2x256 ELU squashed-Normal head; synthetic weights (seed 100 + 7k
for net k), rule "mode", 200 steps at most.  Per (config, K): wall ms of one azg_policy_rollout call (host clock around the call,
which synchronises; median, min and max over --reps after 2 warm-up calls), the steps played per net, and for K = 1 the wall ms of
the host loop over the same number of games.  The file records what was measured.
--wide: the wide configurations of azg_policy_rollout_ex instead (Pendulum-v1 4x1024 ELU with the mixture and the Normal head,
CartPole 2x512 ReLU), K in --ks (default 1,4,16) x G in {32, 128, 1024 / K}: per point the team form's wall ms, with --force-group
also the group form's (a second engine created under AZG_LS_TEAM=0, its calls alternating with the first one's in the same process),
for K = 1 the host loop's, and what each engine's last_rollout_info says ran.
    python tools/policy_rollout_latency.py --wide --force-group --out profiles/policy_rollout_latency_wide.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from alphazero_gym_amd import _capi, _native  # noqa: E402
from alphazero_gym_amd.envs import VecCartPole, VecPendulum  # noqa: E402
from alphazero_gym_amd.synthetic import make_weights  # noqa: E402

MAX_LEN = 200
CONFIGS = {
    "cartpole_2x128_relu": (dict(env_id=0, mode=0, num_actions=2, n_sims=8, c_uct=1.0, gamma=1.0), (4, [128, 128], 2, "relu")),
    "pendulum_v1_2x256_elu": (dict(env_id=2, mode=1, n_sims=8, c_uct=0.05, gamma=1.0), (3, [256, 256], 2, "elu")),
}


# --wide: name -> engine kwargs, (in_dim, hidden, n_dist, activation, mixture components)
WIDE_CONFIGS = {
    "pendulum_v1_4x1024_elu_gmm2": (dict(env_id=2, mode=1, n_sims=8, c_uct=0.05, gamma=1.0), (3, [1024] * 4, 6, "elu", 2)),
    "pendulum_v1_4x1024_elu_normal": (dict(env_id=2, mode=1, n_sims=8, c_uct=0.05, gamma=1.0), (3, [1024] * 4, 2, "elu", 0)),
    "cartpole_2x512_relu": (dict(env_id=0, mode=0, num_actions=2, n_sims=8, c_uct=1.0, gamma=1.0), (4, [512, 512], 2, "relu", 0)),
}


def _engine(kw, net, K, n_trees=None):
    in_dim, hidden, n_dist, act = net[:4]
    e = _native.HipEngine(**dict(kw, n_trees=n_trees or K))
    desc = _capi.make_desc(in_dim, hidden, n_dist, act, num_components=net[4] if len(net) > 4 else 0)
    if K == 1:
        e.set_weights(desc, make_weights(100, in_dim, hidden, n_dist))
    else:
        e.set_population(K)
        for k in range(K):
            e.set_net_weights(k, desc, make_weights(100 + 7 * k, in_dim, hidden, n_dist))
    return e


def _host_loop(e, kw, G):
    """The same evaluation without the entry point: rule "mode" from azg_mlp_eval's outputs, numpy envs, finished games frozen."""
    env = VecCartPole(G, seed=0) if kw["env_id"] == 0 else VecPendulum(G, version=1, seed=0)
    ret, live, steps = np.zeros(G), np.ones(G, bool), 0
    for _ in range(MAX_LEN):
        _, dist, raw = e.mlp_eval(env.obs())
        act = raw[:, 1:].argmax(1) if kw["mode"] == 0 else 2.0 * np.tanh(dist[:, 0])
        before = env.state.copy()
        r, done = env.step(act)
        env.state[~live] = before[~live]
        ret[live] += r[live]
        steps += int(live.sum())
        live &= ~done
        if not live.any():
            break
    return ret, steps


def measure(name, K, G, reps):
    kw, net = CONFIGS[name]
    e = _engine(kw, net, K)
    for _ in range(2):
        out = e.policy_rollout(G, MAX_LEN, rule="mode", game_id_base=1 << 30)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        e.policy_rollout(G, MAX_LEN, rule="mode", game_id_base=1 << 30)
        ms.append((time.perf_counter() - t0) * 1e3)
    rec = dict(K=K, steps_per_net=float(out["lengths"].sum(axis=1).mean()), longest=int(out["lengths"].max()),
               ms=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms), host_ms=None, host_steps=None)
    if K == 1:
        _host_loop(e, kw, G)
        hm = []
        for _ in range(max(3, reps // 3)):
            t0 = time.perf_counter()
            _, steps = _host_loop(e, kw, G)
            hm.append((time.perf_counter() - t0) * 1e3)
        rec["host_ms"], rec["host_steps"] = float(np.median(hm)), steps
    e.close()
    return rec


def _timed(e, G, reps_ms):
    t0 = time.perf_counter()
    out = e.policy_rollout(G, MAX_LEN, rule="mode", game_id_base=1 << 30)
    reps_ms.append((time.perf_counter() - t0) * 1e3)
    return out


def measure_wide(name, K, G, reps, force_group):
    """One point of --wide: the team engine and (force_group) the AZG_LS_TEAM=0 engine called in turn, 2 warm-ups each."""
    kw, net = WIDE_CONFIGS[name]
    team = _engine(kw, net, K, n_trees=32 * K)   # (several nets searched as teams: a multiple of 32 trees each)
    group = None
    if force_group:
        old = os.environ.get("AZG_LS_TEAM")
        os.environ["AZG_LS_TEAM"] = "0"
        group = _engine(kw, net, K, n_trees=32 * K)
        if old is None:
            del os.environ["AZG_LS_TEAM"]
        else:
            os.environ["AZG_LS_TEAM"] = old
    t_ms, g_ms = [], []
    for i in range(2 + reps):
        if i == 2:
            t_ms, g_ms = [], []
        out = _timed(team, G, t_ms)
        if group is not None:
            out_g = _timed(group, G, g_ms)
            assert all((out[k] == out_g[k]).all() for k in out), "the two forms disagree"
    rec = dict(K=K, G=G, steps_per_net=float(out["lengths"].sum(axis=1).mean()), team_ms=(float(np.median(t_ms)), min(t_ms), max(t_ms)),
               team_info=team.last_rollout_info, group_ms=None, group_info=None, host_ms=None)
    if group is not None:
        rec["group_ms"], rec["group_info"] = (float(np.median(g_ms)), min(g_ms), max(g_ms)), group.last_rollout_info
        group.close()
    if K == 1:
        _host_loop(team, kw, G)
        hm = []
        for _ in range(max(3, reps // 3)):
            t0 = time.perf_counter()
            _host_loop(team, kw, G)
            hm.append((time.perf_counter() - t0) * 1e3)
        rec["host_ms"] = float(np.median(hm))
    team.close()
    return rec


def main_wide(a):
    ks = [int(k) for k in (a.ks or "1,4,16").split(",")]
    lines = [f"# azg_policy_rollout_ex, wide nets: K nets x G episodes, rule mode, at most {MAX_LEN} steps; wall ms of one call, host clock around "
             f"the synchronising call (median min max of {a.reps} after 2 warm-ups).  team: the default engine; group: an engine created under "
             f"AZG_LS_TEAM=0, called in turn with the first in the same process; host loop (K = 1): azg_mlp_eval per env step + numpy envs "
             f"on the same engine (start states differ: numpy's RNG).  info: last_rollout_info of the last call."]
    for name in (a.configs.split(",") if a.configs else WIDE_CONFIGS):
        lines.append(f"# {name}")
        lines.append(f"# {'K':>3} {'G':>5} {'env steps per net':>18} | {'team ms':>9} {'min':>8} {'max':>8} | {'group ms':>9} {'min':>8} {'max':>8} | {'host loop ms':>12} | info")
        for K in ks:
            for G in sorted({32, 128, max(1024 // K, 1)}):
                r = measure_wide(name, K, G, a.reps, a.force_group)
                grp = "{:9.3f} {:8.3f} {:8.3f}".format(*r["group_ms"]) if r["group_ms"] else f"{'-':>9} {'-':>8} {'-':>8}"
                host = f"{r['host_ms']:12.3f}" if r["host_ms"] is not None else f"{'-':>12}"
                lines.append("  {:3d} {:5d} {:18.1f} | {:9.3f} {:8.3f} {:8.3f} | {} | {} | team engine {} group engine {}".format(
                    K, G, r["steps_per_net"], *r["team_ms"], grp, host, r["team_info"], r["group_info"]))
                print(lines[-1], flush=True)
    out = a.out or os.path.join("profiles", "policy_rollout_latency_wide.txt")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wide", action="store_true", help="the wide configurations (azg_policy_rollout_ex): team form, group form, host loop")
    ap.add_argument("--force-group", action="store_true", help="--wide: also measure the group form (an engine created under AZG_LS_TEAM=0)")
    ap.add_argument("--configs", default="", help="--wide: comma-separated names of WIDE_CONFIGS (default: all)")
    ap.add_argument("--ks", default="")
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ.setdefault("AZG_QUIET", "1")
    if a.wide:
        return main_wide(a)
    a.ks = a.ks or "1,8,64"
    a.out = a.out or os.path.join("profiles", "policy_rollout_latency.txt")
    lines = [f"# azg_policy_rollout: K nets x {a.episodes} episodes, rule mode, at most {MAX_LEN} steps; wall ms of one call (median, min, max of "
             f"{a.reps}); host loop: azg_mlp_eval per env step + numpy envs, one net x {a.episodes} games (start states differ: numpy's RNG)"]
    for name in CONFIGS:
        lines.append(f"# {name}")
        lines.append(f"# {'K':>4} {'env steps per net':>18} {'longest episode':>16} {'rollout ms':>11} {'min':>8} {'max':>8} {'host loop ms (1 net)':>21} "
                     f"{'its env steps':>14}")
        for K in [int(k) for k in a.ks.split(",")]:
            r = measure(name, K, a.episodes, a.reps)
            host = f"{r['host_ms']:21.3f} {r['host_steps']:14d}" if r["host_ms"] is not None else f"{'-':>21} {'-':>14}"
            lines.append(f"  {r['K']:4d} {r['steps_per_net']:18.1f} {r['longest']:16d} {r['ms']:11.3f} {r['ms_min']:8.3f} {r['ms_max']:8.3f} {host}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
