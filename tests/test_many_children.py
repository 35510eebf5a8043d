"""More than 16 children per node (Kmax = ceil(c_pw * n_sims^kappa) > 16): the paths the engine switches to there, against the CPU
oracle, bit for bit.

A. Search on wide networks (hidden width >= 512): trees in global memory with child lists of stride Kp = 32 / 48 under the team
   kernel, the per-layer launches and the forced one-launch kernel, and results_kernel's loop over more than 16 root children.
B. Self-play through selfplay_kernel (one thread per game, reading the published trees; selfplay_kernel16 serves Kmax <= 16 only):
   every final-action rule, the K x K on-policy target, episode ends by length and by the flag, a ring, both sides of the
   switch, a wide network with and without the team kernel, a population.
C. The Python edge behind it: rows of 20 actions train on the torch path; the device trainer (at most 16 actions per row)
   refuses them before anything is launched.

Every case's inputs are shown to reach the path on the ORACLE's output (`_check_search_case`, `_check_selfplay_case`): those
conditions run without a GPU as tests of their own and again inside every GPU test."""
import math
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _kmax(kw):
    """ceil(c_pw * n_sims^kappa): NodeContinuous.check_pw's bound at the root's last visit (states.py:271-273)."""
    return math.ceil(kw.get("c_pw", 1.0) * kw["n_sims"] ** kw.get("kappa", 0.5))


# ------------------------------------------------------------------------------------- A. search parity, wide networks, Kmax > 16

# name: (env, hidden, mixture components, B, engine settings, Kmax, least number of root children of every tree)
SEARCH_CASES = {
    "pendulum_2x512_k19": (2, [512, 512], 0, 37, dict(n_sims=40, c_uct=0.05, gamma=1.0, c_pw=2.0, kappa=0.6), 19, 17),
    # three passes of results_kernel's a += 16 loop per lane; the K x K on-policy target
    "pendulum_2x512_k46_on_policy": (2, [512, 512], 0, 37, dict(n_sims=64, c_uct=0.3, gamma=0.97, c_pw=2.5, kappa=0.7, epsilon=0.2,
                                                                v_target="on_policy"), 46, 33),
    # the first Kmax past the switch, on config E's network
    "pendulum_4x1024_k17": (2, [1024] * 4, 0, 19, dict(n_sims=257, c_uct=0.05, gamma=1.0), 17, 17),
    "pendulum_3x512_gmm2_k18": (2, [512, 512, 512], 2, 37, dict(n_sims=36, c_uct=0.05, gamma=1.0, c_pw=3.0), 18, 17),
    # terminal nodes, and nodes below the root with more than 16 children
    "mcc_2x512_k24": (4, [512, 512], 0, 37, dict(n_sims=60, c_uct=0.05, gamma=1.0, c_pw=2.0, kappa=0.6, action_bound=1.0), 24, 17),
}
# (forcing variable, the kernel form it must give: engine_host.h AZG_FORM_*)
FORMS = [(None, 2), (("AZG_LS_TEAM", "0"), 1), (("AZG_FORCE_PERSISTENT", "1"), 0)]


def _search_inputs(name):
    env, hidden, ncomp, B, extra, _, _ = SEARCH_CASES[name]
    kw = dict(env_id=env, mode=1, n_trees=B, seed=1234, tree_id_base=77, **extra)
    in_dim, n_dist = (2 if env == 4 else 3), (3 * ncomp if ncomp else 2)
    desc = _capi.make_desc(in_dim, hidden, n_dist, "elu", num_components=ncomp)
    blob = O.make_weights(99, in_dim, hidden, n_dist, scale=2.0)
    o = O.OracleEngine(**kw)
    roots = P.config_roots(env, o.synthetic_roots())
    o.close()
    return kw, desc, blob, roots


def _search(engine_cls, kw, desc, blob, roots):
    e = engine_cls(**kw)
    e.set_weights(desc, blob)
    e.set_search_index(3)
    e.search(roots)
    out = (e.results(), e.dump_tree(), e.root_children(), e.root_eval())
    info = e.search_info() if hasattr(e, "search_info") else None
    kmax = e.kmax
    e.close()
    return out, info, kmax


_search_ref = {}


def _oracle_search(name):
    """The oracle's (results, dump, root children, root evaluation) of a case: computed once, shared, never modified."""
    if name not in _search_ref:
        out, _, kmax = _search(O.OracleEngine, *_search_inputs(name))
        for part in out:
            for a in (part.values() if isinstance(part, dict) else part):
                a.setflags(write=False)
        _search_ref[name] = (out, kmax)
    return _search_ref[name]


def _assert_same(a, b, what):
    for da, db in zip(a, b):
        if isinstance(da, dict):
            for k in da:
                np.testing.assert_array_equal(da[k], db[k], err_msg=f"{what}: {k}")
        else:
            for x, y in zip(da, db):
                np.testing.assert_array_equal(x, y, err_msg=what)


def _tree_shapes(dump):
    """Per tree: (depth of its deepest node, largest number of children of a node below the root, whether it holds a terminal node).
    Continuous trees: record j > 0 is one edge with its child node, `parent[j]` the record of the node the edge leaves."""
    B = dump["n_records"].shape[0]
    deepest, widest_below, terminal = np.zeros(B, int), np.zeros(B, int), np.zeros(B, bool)
    for t in range(B):
        n = int(dump["n_records"][t])
        par = dump["parent"][t][:n]
        depth = np.zeros(n, int)
        for j in range(1, n):
            assert 0 <= par[j] < j
            depth[j] = depth[par[j]] + 1
        kids = np.bincount(par[1:], minlength=n)
        deepest[t] = depth.max()
        widest_below[t] = kids[1:].max() if n > 1 else 0
        terminal[t] = ((dump["node_flags"][t][:n] & 2) != 0).any()
    return deepest, widest_below, terminal


def _check_search_case(name):
    """The case's inputs reach the path, on the oracle's output."""
    env, _, _, B, extra, kmax, least = SEARCH_CASES[name]
    (res, dump, _, _), got_kmax = _oracle_search(name)
    assert got_kmax == kmax == _kmax(extra)
    assert kmax > 16 and -(-kmax // 16) * 16 > 16          # child lists of stride Kp = 32, 48: global trees (azg_tree_storage)
    assert (res["n_children"] >= least).all() and least > 16, res["n_children"]
    assert (res["counts"].sum(1) == extra["n_sims"]).all()
    deepest, widest_below, terminal = _tree_shapes(dump)
    np.testing.assert_array_equal(np.array([np.count_nonzero(dump["parent"][t][1:dump["n_records"][t]] == 0) for t in range(B)]),
                                  res["n_children"])       # (the root's children as the records tell them)
    assert deepest.max() >= 2, deepest
    if env == 4:
        assert terminal.sum() >= B // 3, terminal.sum()
        assert (widest_below > 16).sum() >= 1, widest_below
    return deepest, widest_below, terminal


@pytest.mark.parametrize("name", sorted(SEARCH_CASES))
def test_search_cases_reach_the_paths_on_the_oracle(name):
    deepest, widest_below, terminal = _check_search_case(name)
    print(f"{name}: Kmax {SEARCH_CASES[name][5]}, deepest node {deepest.max()}, trees with a terminal node {terminal.sum()}, "
          f"trees with > 16 children below the root {(widest_below > 16).sum()}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEARCH_CASES))
def test_wide_network_search_matches_oracle(name, monkeypatch):
    """Team kernel, per-layer launches and the one-launch kernel on a wide network whose nodes hold more than 16 children: every
    result row and tree record identical to the oracle's, the three forms identical to each other, and each run on the form it
    names."""
    from alphazero_gym_amd import _native
    _native.lib()
    _check_search_case(name)
    want, kmax = _oracle_search(name)
    inputs = _search_inputs(name)
    for var in ("AZG_LS_TEAM", "AZG_FORCE_PERSISTENT", "AZG_TEAM_SPIN_LIMIT"):
        monkeypatch.delenv(var, raising=False)
    runs = []
    for forced, form in FORMS:
        if forced:
            monkeypatch.setenv(*forced)
        got, info, got_kmax = _search(_native.HipEngine, *inputs)
        if forced:
            monkeypatch.delenv(forced[0])
        what = f"{name} {forced or 'default'}"
        assert got_kmax == kmax and info["max_children"] == kmax, what
        if form == 2 and info["kernel_form_id"] == 1:
            assert info["team_fallbacks"] >= 1, (what, info)     # (the team kernel gave up: its workgroups were not all resident)
        else:
            assert info["kernel_form_id"] == form, (what, info)
        assert info["tree_storage"] == "global", (what, info)
        _assert_same(got, want, what)
        runs.append(got)
    _assert_same(runs[0], runs[1], f"{name}: team kernel and per-layer launches")
    _assert_same(runs[0], runs[2], f"{name}: team kernel and one-launch kernel")


# ----------------------------------------------------------------------------------------- B. self-play through selfplay_kernel

PEND_V0 = dict(kw=dict(env_id=1, mode=1, n_sims=100, c_uct=0.1, gamma=0.97, c_pw=2.0, kappa=0.5, epsilon=0.1, v_target="on_policy",
                       seed=22, tree_id_base=6), desc=(3, [64], 2, "relu"), max_len=4, kmax=20)
SWITCH = dict(env_id=2, mode=1, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=25, tree_id_base=5)
SELFPLAY_CASES = {
    "pendulum_k20": dict(kw=dict(env_id=2, mode=1, n_sims=24, c_uct=0.05, gamma=1.0, c_pw=4.0, kappa=0.5, seed=21, tree_id_base=5),
                         desc=(3, [64, 64], 2, "elu"), max_len=4, kmax=20, late_pick=True),
    # the K x K on-policy target with both final-action rules (max_value: Q's arg-max, then the agent's epsilon)
    "pendulum_v0_k20_max_value_eps": dict(PEND_V0, begin=dict(final_selection="max_value", agent_epsilon=0.4), late_pick=True),
    "pendulum_v0_k20_max_visit": dict(PEND_V0, late_pick=True),
    # games start below the flag (roots uploaded after selfplay_begin): episodes end by reaching it and by length
    "mcc_k22": dict(kw=dict(env_id=4, mode=1, n_sims=30, c_uct=0.05, gamma=1.0, c_pw=4.0, kappa=0.5, seed=24, tree_id_base=9,
                            action_bound=1.0), desc=(2, [64, 64], 2, "elu"), max_len=5, kmax=22, slope=True),
    # both sides of the switch, same seeds: 256 simulations -> Kmax 16 (selfplay_kernel16), 257 -> 17 (selfplay_kernel)
    "pendulum_256_k16": dict(kw=dict(SWITCH, n_sims=256), desc=(3, [64, 64], 2, "elu"), max_len=4, kmax=16),
    "pendulum_257_k17": dict(kw=dict(SWITCH, n_sims=257), desc=(3, [64, 64], 2, "elu"), max_len=4, kmax=17),
    # a wide network: search on the team kernel (trees in global memory), no launch_results before the self-play kernel
    "pendulum_2x512_k19": dict(kw=dict(env_id=2, mode=1, n_sims=40, c_uct=0.05, gamma=1.0, c_pw=2.0, kappa=0.6, seed=26, tree_id_base=5),
                               desc=(3, [512, 512], 2, "elu"), max_len=4, kmax=19),
    # a ring of 4 steps through 9 steps: overwrites its oldest step like ReplayBuffer.store
    "pendulum_k20_ring": dict(kw=dict(env_id=2, mode=1, n_sims=24, c_uct=0.05, gamma=1.0, c_pw=4.0, kappa=0.5, seed=21, tree_id_base=5),
                              desc=(3, [64, 64], 2, "elu"), max_len=4, kmax=20, begin=dict(capacity_steps=4, fifo=True)),
}
GAMES, STEPS = 21, 9


def play(engine_cls, case):
    """test_selfplay_device.play for a case of SELFPLAY_CASES: (rows of the ring in slot order, stats, ring bookkeeping, search_info)."""
    c = SELFPLAY_CASES[case]
    e = engine_cls(n_trees=GAMES, **c["kw"])
    in_dim, hidden, nd, act = c["desc"]
    e.set_weights(_capi.make_desc(in_dim, hidden, nd, act), O.make_weights(3, in_dim, hidden, nd, scale=2.0))
    e.selfplay_begin(c["max_len"], False, **dict(dict(capacity_steps=STEPS), **c.get("begin", {})))
    if c.get("slope"):
        e.upload_roots(P.slope_roots(e.synthetic_roots()))
    for _ in range(STEPS):
        e.selfplay_step()
    rows = e.selfplay_rows(clear=False)
    out = (rows, e.selfplay_stats(), e.selfplay_ring(), e.search_info() if hasattr(e, "search_info") else None, e.kmax, e.s_obs)
    e.close()
    return out


_selfplay_ref = {}


def _oracle_play(case):
    """The oracle's rows, stats and ring of a case: computed once, shared, never modified."""
    if case not in _selfplay_ref:
        out = play(O.OracleEngine, case)
        for a in (out[0],) + tuple(out[1]):
            a.setflags(write=False)
        _selfplay_ref[case] = out
    return _selfplay_ref[case]


def _check_selfplay_case(case):
    """The case's games reach selfplay_kernel's branches, and test_selfplay_invariants_on_oracle's invariants, on the oracle's rows."""
    c = SELFPLAY_CASES[case]
    rows, (fsum, fcnt, state), ring, _, K, so = _oracle_play(case)
    kw = c["kw"]
    assert K == c["kmax"] == _kmax(kw) and so == (2 if kw["env_id"] == 4 else 3)
    stored = min(STEPS, c.get("begin", {}).get("capacity_steps", STEPS))
    assert rows.shape == (stored * GAMES, so + 3 * K + 1)
    assert ring == (stored, STEPS % stored if stored < STEPS else 0, STEPS)
    actions, counts = rows[:, so:so + K], rows[:, so + K:so + 2 * K]
    nonzero = (counts != 0).sum(1)
    if K == 16:
        assert (nonzero == 16).all(), nonzero                # (the other side of the switch)
    else:
        assert K > 16 and (nonzero > 16).all(), nonzero      # every root holds more than 16 children
    late = int((counts.argmax(1) >= 16).sum())               # rows whose most visited child lies beyond the 16th
    if c.get("late_pick"):
        assert late >= 1
    assert fcnt.sum() > 0
    # invariants
    np.testing.assert_array_equal(counts.sum(1), np.full(len(rows), float(kw["n_sims"])))
    assert (np.abs(actions) <= kw.get("action_bound", 2.0)).all()
    assert np.isfinite(state).all() and np.isfinite(rows).all()
    if kw["env_id"] == 4:
        reached = fsum > 50                                                  # +100 at the flag
        assert reached.any() and (~reached & (fcnt >= 1)).any()              # episodes end by the flag, and by length
        assert (-0.6 <= state[reached, 0]).all() and (state[:, 0] < 0.45).all()   # a game that reached the flag restarted in the valley
    else:
        np.testing.assert_allclose(np.hypot(rows[:, 0], rows[:, 1]), 1.0, atol=1e-6)
        assert (fcnt == STEPS // c["max_len"]).all() and (fsum < 0).all()    # Pendulum never terminates: episodes end by length
    return late


@pytest.mark.parametrize("case", sorted(SELFPLAY_CASES))
def test_selfplay_cases_reach_the_paths_on_the_oracle(case):
    late = _check_selfplay_case(case)
    print(f"{case}: rows whose largest count sits at column 16 or beyond: {late} of {_oracle_play(case)[0].shape[0]}")


def test_final_action_rules_differ_on_the_oracle():
    """The two Pendulum-v0 runs differ only in the final-action rule: the rule shows in the games they play."""
    a, b = _oracle_play("pendulum_v0_k20_max_value_eps"), _oracle_play("pendulum_v0_k20_max_visit")
    np.testing.assert_array_equal(a[0][:GAMES], b[0][:GAMES])      # the first step's searches start from the same roots
    assert not np.array_equal(a[1][2], b[1][2])                    # the games' states after nine steps


def _assert_played_the_same(got, want, what):
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32), err_msg=f"{what}: rows")
    assert_stats_bits(got[1], want[1], what)
    assert got[2] == want[2], what
    assert got[4:] == want[4:], what


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SELFPLAY_CASES))
def test_selfplay_hip_matches_oracle_bit_for_bit(case, monkeypatch):
    """Replay rows (float32 through their bit patterns), episode statistics, env states and the ring's bookkeeping of nine steps of 21
    games.  Kmax > 16 puts azg_selfplay_step on selfplay_kernel, which reads the published trees without launch_results."""
    from alphazero_gym_amd import _native
    _native.lib()
    for var in ("AZG_LS_TEAM", "AZG_FORCE_PERSISTENT", "AZG_TEAM_SPIN_LIMIT"):
        monkeypatch.delenv(var, raising=False)
    _check_selfplay_case(case)
    want = _oracle_play(case)
    got = play(_native.HipEngine, case)
    assert got[3]["max_children"] == SELFPLAY_CASES[case]["kmax"]
    _assert_played_the_same(got, want, case)
    if case == "pendulum_2x512_k19":
        # the team kernel; then with waits that time out at once (test_team_kernel_gives_up_instead_of_hanging's setting): the first
        # step's search is redone by the per-layer launches before selfplay_kernel reads the trees, the later ones start there
        assert got[3]["kernel_form_id"] == 2 or got[3]["team_fallbacks"] >= 1, got[3]
        monkeypatch.setenv("AZG_TEAM_SPIN_LIMIT", "0")
        again = play(_native.HipEngine, case)
        assert again[3]["team_fallbacks"] == 1 and again[3]["kernel_form_id"] == 1, again[3]
        _assert_played_the_same(again, want, f"{case}, the team kernel giving up")


def _pendulum_nets(n, device):
    import torch
    from selfplay_train import build_agent
    nets = []
    for s in range(n):
        torch.manual_seed(60 + s)
        nets.append(build_agent("Pendulum-v1", [64, 64], 24, device, 1e-3)[0].nn)
    return nets


@pytest.mark.gpu
def test_population_selfplay_with_20_children_equals_single_engines():
    """run.PopulationSelfPlay of three nets (five games each, Kmax 20) plays what three DeviceSelfPlay engines with tree_id_base
    k * 5 play: rows bit for bit, episode statistics."""
    import torch
    from alphazero_gym_amd import _native, run
    _native.lib()
    nets, T, steps = _pendulum_nets(3, "cuda:0"), 5, 9
    kw = dict(game="Pendulum-v1", n_rollouts=24, c_uct=0.05, c_pw=4.0, max_episode_length=4, capacity_steps=steps, seed=9)
    pop = run.PopulationSelfPlay(nets, games_per_net=T, **kw)
    singles = [run.DeviceSelfPlay(net, n_games=T, rank=k, **kw) for k, net in enumerate(nets)]
    K, so = pop.engine.kmax, pop.engine.s_obs
    assert K == 20 and all(s.engine.kmax == 20 and s.engine.cfg.tree_id_base == k * T for k, s in enumerate(singles))
    got, want = pop.collect(steps), [s.collect(steps) for s in singles]
    for k in range(3):
        assert got[k].shape == want[k].shape == (steps * T, so + 3 * K + 1)
        np.testing.assert_array_equal(got[k].numpy().view(np.uint32), want[k].numpy().view(np.uint32), err_msg=f"net {k}")
        counts = got[k][:, so + K:so + 2 * K]
        assert bool(((counts != 0).sum(1) > 16).all()) and torch.equal(counts.sum(1), torch.full((steps * T,), 24.0))
    assert not torch.equal(got[0], got[1])
    fsum, fcnt = pop.finished_returns()
    for k, s in enumerate(singles):
        f, c, _ = s.engine.selfplay_stats()
        acc = 0.0
        for x in f:
            acc += x
        assert fsum[k] == acc and fcnt[k] == c.sum() == T * (steps // 4)
    pop.close()
    for s in singles:
        s.close()


# --------------------------------------------------------------------------------------------- C. the Python edge behind it


@pytest.mark.gpu
def test_rows_of_20_actions_train_on_the_torch_path():
    """DeviceSelfPlay.collect_device with kmax = 20 feeds run.train_on_rows (agent.update in PyTorch: any number of actions per row)."""
    import torch
    from alphazero_gym_amd import _native, run
    from alphazero_gym_amd.agent.agents import ContinuousAgent
    _native.lib()
    cfg = run.CONTINUOUS_DEFAULTS
    policy = dict(cfg["policy"], hidden_dimensions=[64, 64], representation_dim=3, action_dim=1, action_bound=2.0)
    torch.manual_seed(0)
    agent = ContinuousAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], n_rollouts=24, device="cuda:0"),
                            loss_cfg=dict(run.LOSS_TUNED, device="cuda:0"), optimizer_cfg=run.RMSPROP, device="cuda:0", **cfg["agent"])
    sp = run.DeviceSelfPlay(agent.nn, game="Pendulum-v1", n_games=16, n_rollouts=24, c_uct=0.05, c_pw=4.0, max_episode_length=20,
                            capacity_steps=4, fifo=True, seed=3)
    K, so = sp.engine.kmax, sp.engine.s_obs
    assert K == 20
    rows = sp.collect_device(3, sp.replay(batch_size=16))
    assert rows.is_cuda and rows.shape == (3 * 16, so + 3 * K + 1)
    np.testing.assert_array_equal(rows.cpu().numpy(), sp.engine.selfplay_rows(clear=False))
    assert bool(((rows[:, so + K:so + 2 * K] != 0).sum(1) > 16).all())
    w0 = [p.detach().clone() for p in agent.nn.parameters()]
    info = run.train_on_rows(agent, rows, so, K, batch_size=16)
    assert np.isfinite(info["loss"]) and all(np.isfinite(v) for v in info.values())
    assert all(bool(torch.isfinite(p).all()) for p in agent.nn.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(w0, agent.nn.parameters()))
    sp.close()


@pytest.mark.gpu
def test_device_trainer_refuses_rows_of_20_actions_untouched():
    """The device trainer's loss kernel takes at most 16 actions per row (train.cuh: TR_MAX_ACTIONS).  On a ring of 20-action rows
    train_epoch_ring and train_on_rows (losses="device") raise the native refusal -- AZG_E_INVALID, "n_actions must be 1..16" --
    from the host checks that precede every launch: parameters, RMSprop state, the learned temperature, its Adam state and step
    count stay bit-identical, and the ring is as it was."""
    import torch
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    from trainer_util import assert_same, make_agents, state_of
    K, T, steps = 2, 4, 3
    agents = make_agents("gmm2", "a0c_tuned", K)
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="Pendulum-v1", games_per_net=T, n_rollouts=24, c_uct=0.05, c_pw=4.0,
                                capacity_steps=4)
    A, so = sp.engine.kmax, sp.engine.s_obs
    assert A == 20 and sp.play_device(steps) == (steps, 0)
    copies = torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps))
    n = steps * T
    assert copies.shape == (K, n, so + 3 * A + 1) and bool(((copies[..., so + A:so + 2 * A] != 0).sum(-1) > 16).all())
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    before = state_of(tr)
    order = np.stack([np.random.RandomState(s).permutation(n) for s in (3, 1)])
    for call in (lambda: tr.train_epoch_ring(sp, order, batch_size=8),
                 lambda: tr.train_on_rows(copies, so, A, batch_size=8, shuffle_seeds=[3, 1]),
                 lambda: tr.train_epoch(copies, so, A, batch_size=8, shuffle_seeds=[3, 1])):
        with pytest.raises(_capi.EngineError, match="n_actions must be 1..16") as ei:
            call()
        assert ei.value.code == _capi.AZG_E_INVALID
        torch.cuda.synchronize()
        assert_same(state_of(tr), before, "after the refusal")
        assert tr.last_raw is None and tr.alpha_step == 0
    for a, row in zip(agents, tr.flat):       # the agents' modules are views of the same, unchanged storage
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in _capi.policy_tensors(a.nn)[1]]), row)
    assert sp.engine.selfplay_ring()[0] == steps
    assert torch.equal(torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps)), copies)
    tr.close()
    sp.close()
