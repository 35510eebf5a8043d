"""Populations (azg_set_population): K nets with their own weights searched in one launch.

Engine level (gpu): a K-net engine computes, bit for bit, what K single-net engines with tree_id_base + k*T compute; the errors of
the population entry points.  Facade (AgentPopulation / run_population): K agents stepped together equal K standalone agents, on the
GPU and on CPU against a double made of K oracle engines."""
import random

import numpy as np
import pytest
import torch

import oracle_lib as O
import parity_util as PU
from alphazero_gym_amd import _capi

K = 5


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


# name: engine kwargs (n_trees / tree_id_base set per test), network (in_dim, hidden, n_dist, activation, mixture components),
# carried root counts (discrete reuse), environment variables that force a workgroup shape
CASES = {
    "pendulum_v1_2x256_elu": (dict(env_id=2, mode=1, n_sims=40, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34),
                              (3, [256, 256], 2, "elu", 0), False, {}),
    "pendulum_v1_2x256_elu_groups2": (dict(env_id=2, mode=1, n_sims=40, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=35),
                                      (3, [256, 256], 2, "elu", 0), False, {"AZG_GROUPS": "2"}),
    "pendulum_v0_3x128_gmm2": (dict(env_id=1, mode=1, n_sims=25, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=36),
                               (3, [128, 128, 128], 6, "elu", 2), False, {}),
    "cartpole_2x128_relu_carry_eps": (dict(env_id=0, mode=0, num_actions=2, n_sims=8, c_uct=1.5, gamma=1.0, epsilon=0.1, seed=37),
                                      (4, [128, 128], 2, "relu", 0), True, {}),
    "acrobot_2x64_relu": (dict(env_id=5, mode=0, num_actions=3, n_sims=30, c_uct=1.0, gamma=0.99, epsilon=0.05, seed=38),
                          (6, [64, 64], 3, "relu", 0), True, {}),
    "mcc_terminal_2x64_elu": (dict(env_id=4, mode=1, n_sims=50, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, action_bound=1.0, seed=39),
                              (2, [64, 64], 2, "elu", 0), False, {}),
}


def _desc(net):
    in_dim, hidden, n_dist, act, ncomp = net
    return _capi.make_desc(in_dim, hidden, n_dist, act, num_components=ncomp)


def _blob(net, k, base_seed=100):
    in_dim, hidden, n_dist, _, _ = net
    return O.make_weights(base_seed + 7 * k, in_dim, hidden, n_dist)


def _roots(name, kw, n, rng):
    """n non-terminal roots of the case's game (MountainCarContinuous: just below the flag, so that traces end in terminal nodes)."""
    e = O.OracleEngine(**dict(kw, n_trees=n, tree_id_base=1000))
    r = e.synthetic_roots()
    e.close()
    if kw["env_id"] == _capi.ENV_MOUNTAINCAR_CONT:
        r[:, 0] = 0.40 + 0.04 * rng.random(n)
        r[:, 1] = 0.01 + 0.02 * rng.random(n)
    return r


def _run_population(cls, kw, net, T, roots, carry, base, idx, dump=False):
    e = cls(**dict(kw, n_trees=K * T, tree_id_base=base))
    e.set_population(K)
    for k in range(K):
        e.set_net_weights(k, _desc(net), _blob(net, k))
    e.set_search_index(idx)
    e.search(roots, carry)
    out = dict(e.results())
    out["child_n"], out["child_state"] = e.root_children()
    if dump:
        out.update({"dump_" + k: v for k, v in e.dump_tree().items()})
    e.close()
    return out


def _run_singles(cls, kw, net, T, roots, carry, base, idx, dump=False, blob_of=None):
    parts = []
    for k in range(K):
        e = cls(**dict(kw, n_trees=T, tree_id_base=base + k * T))
        e.set_weights(_desc(net), (blob_of or _blob)(net, k))
        e.set_search_index(idx)
        sl = slice(k * T, (k + 1) * T)
        e.search(roots[sl], None if carry is None else carry[sl])
        out = dict(e.results())
        out["child_n"], out["child_state"] = e.root_children()
        if dump:
            out.update({"dump_" + k2: v for k2, v in e.dump_tree().items()})
        parts.append(out)
        e.close()
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_population_equals_single_engines(name, T, monkeypatch):
    kw, net, carried, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cls = _hip()
    rng = np.random.default_rng(T)
    roots = _roots(name, kw, K * T, rng)
    carry = rng.integers(0, 3 * kw["n_sims"], K * T).astype(np.int32) if carried else None
    base, idx = 11, 5
    dump = T == 3
    got = _run_population(cls, kw, net, T, roots, carry, base, idx, dump=dump)
    want = _run_singles(cls, kw, net, T, roots, carry, base, idx, dump=dump)
    assert set(got) == set(want)
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name} T={T}: {key}")
    assert got["counts"].sum() > 0


@pytest.mark.gpu
def test_population_matches_the_oracle_per_net():
    """Each net of a CartPole population against the CPU oracle with that net's weights and tree id base (parity_util.compare_rows)."""
    kw, net, _, _ = CASES["cartpole_2x128_relu_carry_eps"]
    T, base, idx = 3, 20, 2
    rng = np.random.default_rng(0)
    roots = _roots("cartpole", kw, K * T, rng)
    carry = rng.integers(0, 20, K * T).astype(np.int32)
    got = _run_population(_hip(), kw, net, T, roots, carry, base, idx, dump=True)
    out = [({k: got[k][i] for k in ("actions", "counts", "Q", "v_target", "n_children")},
            {k: got["dump_" + k][i] for k in PU.DUMP_INT + PU.DUMP_F32 + PU.DUMP_F64}, got["child_n"][i]) for i in range(K * T)]
    ref = _run_singles(O.OracleEngine, kw, net, T, roots, carry, base, idx, dump=True)
    z = {k: ref[k] for k in ("actions", "counts", "Q", "v_target", "n_children", "child_n")}
    z.update({k: ref["dump_" + k] for k in PU.DUMP_INT + PU.DUMP_F32 + PU.DUMP_F64})
    PU.compare_rows(out, z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pendulum_v1_2x256_elu", "pendulum_v0_3x128_gmm2", "cartpole_2x128_relu_carry_eps"])
def test_every_net_reads_its_own_weights(name):
    """Identical roots, different weights: net k's trees differ from what net 0's weights give under the same tree ids."""
    kw, net, _, _ = CASES[name]
    T = 3
    cls = _hip()
    root = _roots(name, kw, 1, np.random.default_rng(1))
    roots = np.repeat(root, K * T, axis=0)
    got = _run_population(cls, kw, net, T, roots, None, 0, 0)
    net0 = _run_singles(cls, kw, net, T, roots, None, 0, 0, blob_of=lambda n, k: _blob(n, 0))
    key = "actions" if kw["mode"] == _capi.MODE_CONTINUOUS else "Q"
    sl = lambda k: slice(k * T, (k + 1) * T)   # noqa: E731
    np.testing.assert_array_equal(got[key][sl(0)], net0[key][sl(0)])
    for k in range(1, K):
        assert not np.array_equal(got[key][sl(k)], net0[key][sl(k)]), f"net {k} searched with net 0's weights"


# ---------------------------------------------------------------------------------------------------------------- errors


def _pend(cls, n_trees=6, **over):
    kw = dict(env_id=2, mode=1, n_trees=n_trees, n_sims=10, c_uct=0.05, gamma=1.0)
    kw.update(over)
    return cls(**kw)


def _code(fn, *a):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


@pytest.mark.gpu
def test_population_errors():
    cls = _hip()
    d64, b64 = _capi.make_desc(3, [64, 64], 2, "elu"), O.make_weights(1, 3, [64, 64], 2)
    e = _pend(cls, 10)
    assert _code(e.set_population, 3)[0] == _capi.AZG_E_INVALID            # 10 trees do not split into 3 nets
    assert _code(e.set_population, 0)[0] == _capi.AZG_E_INVALID
    e.close()
    e = _pend(cls, 6)
    e.set_population(3)
    for bad in (3, -1):
        assert _code(e.set_net_weights, bad, d64, b64)[0] == _capi.AZG_E_INVALID
    assert _code(e.set_weights, d64, b64)[0] == _capi.AZG_E_STATE          # one blob for a population
    e.set_net_weights(0, d64, b64)
    e.set_net_weights(2, d64, b64)
    roots = e.synthetic_roots()
    code, msg = _code(e.search, roots)                                       # net 1 has no weights
    assert code == _capi.AZG_E_STATE and "every net" in msg
    for d, b in ((_capi.make_desc(3, [64, 128], 2, "elu"), O.make_weights(1, 3, [64, 128], 2)),
                 (_capi.make_desc(3, [64, 64], 2, "relu"), b64)):
        assert _code(e.set_net_weights, 1, d, b)[0] == _capi.AZG_E_INVALID   # every net has the same descriptor
    e.set_net_weights(1, d64, b64)
    e.search(roots)
    assert e.results()["counts"].sum() == 6 * 10
    assert _code(e.mlp_eval, np.zeros((2, 3), np.float32))[0] == _capi.AZG_E_UNSUPPORTED
    assert _code(e.root_eval)[0] == _capi.AZG_E_UNSUPPORTED
    assert _code(e.selfplay_begin, 10)[0] == _capi.AZG_E_UNSUPPORTED        # device self-play: one network per engine
    e.close()
    e = _pend(cls, 4)
    e.set_population(2)
    code, msg = _code(e.set_net_weights, 0, _capi.make_desc(3, [512, 512], 2, "elu"), O.make_weights(1, 3, [512, 512], 2))
    assert code == _capi.AZG_E_UNSUPPORTED and "team" in msg                 # HP >= 512: team / per-layer forms
    e.close()


@pytest.mark.gpu
def test_set_population_one_restores_the_single_network_engine():
    cls = _hip()
    d, b = _capi.make_desc(3, [128, 128], 2, "elu"), O.make_weights(3, 3, [128, 128], 2)
    fresh = _pend(cls, 20, n_sims=30)
    fresh.set_weights(d, b)
    roots = fresh.synthetic_roots()
    fresh.search(roots)
    want = fresh.results()
    fresh.close()
    e = _pend(cls, 20, n_sims=30)
    e.set_population(4)
    for k in range(4):
        e.set_net_weights(k, d, O.make_weights(50 + k, 3, [128, 128], 2))
    e.search(roots)
    e.set_population(1)                                                      # drops every weight
    assert _code(e.search, roots)[0] == _capi.AZG_E_STATE
    e.set_weights(d, b)
    e.set_search_index(0)
    e.search(roots)
    got = e.results()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    e.close()


def test_oracle_library_has_no_population_entry_points():
    """The CPU oracle (azo_ prefix) lacks the population entry points: _capi binds it all the same, and the methods say so."""
    e = O.OracleEngine(env_id=2, mode=1, n_trees=2, n_sims=4, c_uct=0.05, gamma=1.0)
    with pytest.raises(NotImplementedError):
        e.set_population(2)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- facade


class OraclePopulation:
    """CPU double of a HIP engine with populations: K oracle engines, net k with tree_id_base + k*T, run one after another under the
    population's search index.  Without set_population it is one oracle engine."""

    def __init__(self, **kw):
        self.kw = kw
        self.n_trees = kw["n_trees"]
        self.mode = kw["mode"]
        self.idx = 0
        self.set_population(1)

    def set_population(self, n):
        self.n_nets = n
        T = self.n_trees // n
        self.T = T
        self.engines = [O.OracleEngine(**dict(self.kw, n_trees=T, tree_id_base=self.kw.get("tree_id_base", 0) + k * T)) for k in range(n)]

    def set_net_policy(self, k, policy):
        self.engines[k].set_policy(policy)

    def set_policy(self, policy):
        self.set_net_policy(0, policy)

    def set_search_index(self, idx):
        self.idx = idx

    def search(self, roots, carry=None):
        roots = np.asarray(roots, np.float64).reshape(self.n_trees, -1)
        for k, e in enumerate(self.engines):
            sl = slice(k * self.T, (k + 1) * self.T)
            e.set_search_index(self.idx)
            e.search(roots[sl], None if carry is None else np.asarray(carry)[sl])
        self.idx += 1

    def results(self):
        parts = [e.results() for e in self.engines]
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def root_children(self):
        parts = [e.root_children() for e in self.engines]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def close(self):
        for e in self.engines:
            e.close()


FACADE = {
    "continuous": dict(game="Pendulum-v0", num_train_episodes=2, max_episode_length=12, mcts=dict(n_rollouts=25),
                       policy=dict(num_components=2, hidden_dimensions=[128, 128, 128]), buffer=dict(max_size=100, batch_size=8)),
    "discrete": dict(game="CartPole-v0", num_train_episodes=2, max_episode_length=30, mcts=dict(n_rollouts=8),
                     buffer=dict(max_size=100, batch_size=8)),
}
SEEDS = [34, 35, 36]


def _agents(kind, device="cpu"):
    from alphazero_gym_amd import run
    from alphazero_gym_amd.envs import make_game
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, dict(FACADE[kind], device=device))
    torch.manual_seed(7)
    return [run.make_agent(kind, cfg, make_game(cfg["game"]), tree_id_base=k) for k in range(len(SEEDS))], cfg


def _standalone(kind, agents, cfg):
    """Each agent alone, one after another within an episode, with its own np.random / random streams (seeded with its seed), its own
    env and buffer, searching under the population's step index (a step of a population episode is as long as its longest game)."""
    from alphazero_gym_amd.agent.buffers import ReplayBuffer
    from alphazero_gym_amd.envs import make_game
    from alphazero_gym_amd.search.mcts import env_signature
    K = len(agents)
    envs = [make_game(cfg["game"]) for _ in range(K)]
    for env, s in zip(envs, SEEDS):
        env.seed(s)
    buffers = [ReplayBuffer(**cfg["buffer"]) for _ in range(K)]
    streams = [(np.random.RandomState(s).get_state(), random.Random(s).getstate()) for s in SEEDS]
    acts = [[] for _ in range(K)]
    returns = [[] for _ in range(K)]
    base = 0
    for ep in range(cfg["num_train_episodes"]):
        longest = 0
        for k, agent in enumerate(agents):
            outer = (np.random.get_state(), random.getstate())
            np.random.set_state(streams[k][0])
            random.setstate(streams[k][1])
            env, R = envs[k], 0.0
            agent.reset_mcts(root_state=env.reset())
            for t in range(cfg["max_episode_length"]):
                agent.mcts._ensure_engine(env_signature(env)[0], 1).engine.set_search_index(base + t)
                out = agent.act(env, deterministic=False) if kind == "discrete" else agent.act(env)
                acts[k].append(out)
                action, s, actions, counts, Qs, V = out
                buffers[k].store((s, actions, counts, Qs, V))
                state, r, terminal, _ = env.step(action)
                R += float(np.asarray(r).reshape(-1)[0])
                longest = max(longest, t + 1)
                if terminal or t == cfg["max_episode_length"] - 1:
                    break
                if kind == "continuous":
                    agent.reset_mcts(root_state=state)
                else:
                    agent.mcts_forward(action, state)
            returns[k].append(R)
            agent.train(buffers[k])
            streams[k] = (np.random.get_state(), random.getstate())
            np.random.set_state(outer[0])
            random.setstate(outer[1])
        base += longest
    return acts, returns


def _population(kind, agents, cfg, monkeypatch):
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent import population
    acts = [[] for _ in agents]
    orig = population.AgentPopulation.act

    def recording_act(self, envs, deterministic=False):
        outs = orig(self, envs, deterministic)
        for k, o in enumerate(outs):
            if o is not None:
                acts[k].append(o)
        return outs

    monkeypatch.setattr(population.AgentPopulation, "act", recording_act)
    returns = run.run_population(kind, SEEDS, FACADE[kind], agents=agents)
    return acts, returns


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.fixture(params=["oracle_double", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, monkeypatch):
    from alphazero_gym_amd import _native
    if request.param == "oracle_double":
        monkeypatch.setattr(_native, "HipEngine", OraclePopulation)
    else:
        _native.lib()
    return request.param


@pytest.mark.parametrize("kind", ["continuous", "discrete"])
def test_agent_population_equals_standalone_agents(kind, backend, monkeypatch):
    pop_agents, cfg = _agents(kind)
    ref_agents, _ = _agents(kind)
    for a, b in zip(pop_agents, ref_agents):
        for p, q in zip(a.nn.parameters(), b.nn.parameters()):
            assert torch.equal(p, q)
    outer = np.random.get_state()
    pop_acts, pop_returns = _population(kind, pop_agents, cfg, monkeypatch)
    assert np.array_equal(np.random.get_state()[1], outer[1])   # the global stream is left as it was
    ref_acts, ref_returns = _standalone(kind, ref_agents, cfg)
    assert pop_returns == ref_returns
    for k in range(len(SEEDS)):
        assert len(pop_acts[k]) == len(ref_acts[k]) > 0
        for i, (x, y) in enumerate(zip(pop_acts[k], ref_acts[k])):
            _same(x, y)
        for (n, p), (_, q) in zip(pop_agents[k].nn.named_parameters(), ref_agents[k].nn.named_parameters()):
            assert torch.equal(p, q), f"agent {k}: {n} after training"
    # the agents did train, and not all alike
    assert not torch.equal(next(pop_agents[0].nn.parameters()), next(pop_agents[1].nn.parameters()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["continuous", "discrete"])
def test_agent_population_with_nets_on_the_gpu_gathers_them_in_one_upload(kind):
    """Agents whose nets live on cuda:0: the population uploads every net with one gather ("device"), again after one net changed,
    and each agent acts bit for bit as it does standalone."""
    from alphazero_gym_amd.agent.population import AgentPopulation
    from alphazero_gym_amd.envs import make_game
    from alphazero_gym_amd.search.mcts import env_signature
    _hip()
    pop_agents, cfg = _agents(kind, "cuda:0")
    ref_agents, _ = _agents(kind, "cuda:0")
    assert next(pop_agents[0].nn.parameters()).is_cuda
    K = len(SEEDS)
    pop_envs, ref_envs = [make_game(cfg["game"]) for _ in range(K)], [make_game(cfg["game"]) for _ in range(K)]
    for k in range(K):
        for env, agent in ((pop_envs[k], pop_agents[k]), (ref_envs[k], ref_agents[k])):
            env.seed(SEEDS[k])
            agent.reset_mcts(root_state=env.reset())
    streams = [(np.random.RandomState(s).get_state(), random.Random(s).getstate()) for s in SEEDS]
    pop = AgentPopulation(pop_agents, seeds=SEEDS)
    syncs = []
    for t in range(4):   # (4 steps: no CartPole game ends)
        if t == 2:       # an optimiser step of agent 1
            with torch.no_grad():
                for agent in (pop_agents[1], ref_agents[1]):
                    for p in agent.nn.parameters():
                        p.mul_(0.5)
        outs = pop.act(pop_envs, deterministic=False)
        syncs.append(pop.mcts.last_weight_sync)
        for k, agent in enumerate(ref_agents):
            outer = (np.random.get_state(), random.getstate())
            np.random.set_state(streams[k][0])
            random.setstate(streams[k][1])
            agent.mcts._ensure_engine(env_signature(ref_envs[k])[0], 1).engine.set_search_index(t)
            want = agent.act(ref_envs[k], deterministic=False) if kind == "discrete" else agent.act(ref_envs[k])
            streams[k] = (np.random.get_state(), random.getstate())
            np.random.set_state(outer[0])
            random.setstate(outer[1])
            _same(outs[k], want)
            for env, a in ((pop_envs[k], pop_agents[k]), (ref_envs[k], agent)):
                state, _, terminal, _ = env.step(want[0])
                assert not terminal
                if kind == "continuous":
                    a.reset_mcts(root_state=state)
                else:
                    a.mcts_forward(want[0], state)
    assert syncs == [None, None, "device", None]   # (the first upload happens when the first act builds the engine)
    pop.mcts.sync_weights(force=True)
    assert pop.mcts.last_weight_sync == "device"
    pop.close()


def test_agent_population_rejects_mixed_settings():
    from alphazero_gym_amd.agent.population import AgentPopulation
    agents, _ = _agents("discrete")
    agents[1].mcts.c_uct = 2.0
    with pytest.raises(ValueError):
        AgentPopulation(agents)
    cont, _ = _agents("continuous")
    with pytest.raises(ValueError):
        AgentPopulation([agents[0], cont[0]])
