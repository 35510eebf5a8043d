"""CPU: per-net search settings (azg_set_net_search) -- that the GPU matrix cannot pass by accident, and the Python layer.

The matrix (test_population_net_search.py) gives nets 1 and 2 of every row settings of their own; here, on the oracle alone, those
settings are shown to change the trees of those very nets, row by row, and net 1's narrow widening to fit every row's engine.  The
Python layer runs against a CPU double of the engine made of K oracle engines, each created with its net's settings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import net_search_util as N
import oracle_lib as O
import parity_util as P
import test_population as TP
import test_population_parity as PP
from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 19


# ------------------------------------------------------------------------------------------- the matrix cannot pass by accident


@pytest.mark.parametrize("ci", N.matrix_rows(), ids=lambda ci: f"cfg{ci}")
def test_the_settings_of_nets_1_and_2_change_their_trees(ci):
    """Nets 1 and 2 (their own weights, roots and tree ids) under their own settings against the same nets under net 0's: different
    trees.  An engine that ignored its table would therefore fail the matrix on both nets of this row."""
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    st = N.net_settings(cfg)
    assert len({tuple(sorted(s.items())) for s in st}) == 3 and st[0] == N.shared_settings(cfg)
    assert {1.0} < {s["gamma"] for s in st}, "gamma == 1 (closed-form backup) and gamma != 1 in one launch"
    if cfg[1] == 0:
        assert {s["epsilon"] == 0.0 for s in st} == {True, False}, "cached selections and epsilon-greedy descents in one launch"
    else:   # net 1's widening fits the engine the row's own pair creates, so storage and Kmax stay the row's
        ks = [N.kmax_of(s, kw["n_sims"]) for s in st]
        assert ks[1] <= ks[0] == ks[2], ks
        pw0 = _capi.pw_table(st[0]["c_pw"], st[0]["kappa"], kw["n_sims"] + 2)
        pw1 = _capi.pw_table(st[1]["c_pw"], st[1]["kappa"], kw["n_sims"] + 2)
        assert all(a <= b for a, b in zip(pw1, pw0)), "net 1's entitlement never exceeds the row's"
    own = N.oracle_nets(kw, desc, blobs, roots, carry, PP.SIDX, st, width=None if cfg[1] == 0 else N.kmax_of(st[0], kw["n_sims"]))
    shared = PP._oracle(kw, desc, blobs, roots, carry, PP.SIDX)
    sl0 = slice(0, T)
    for key in own[1]:
        np.testing.assert_array_equal(own[1][key][sl0], shared[1][key][sl0], err_msg=f"net 0 {key}")   # (its settings ARE the row's)
    for k in (1, 2):
        sl = slice(k * T, (k + 1) * T)
        differ = sum(own[1]["edge_n"][i].tobytes() != shared[1]["edge_n"][i].tobytes() or
                     own[1]["edge_Q"][i].tobytes() != shared[1]["edge_Q"][i].tobytes() for i in range(sl.start, sl.stop))
        assert differ >= T // 2, f"cfg{ci}: net {k}'s settings change only {differ} of its {T} trees"


# ------------------------------------------------------------------------------------------------------------------ Python layer


class OracleNetSearch(TP.OraclePopulation):
    """OraclePopulation with set_net_search: net k's oracle engine is re-created with its own settings (and its policy uploaded again)."""

    tables = []

    def set_population(self, n):
        super().set_population(n)
        self.policies = [None] * n

    def set_net_policy(self, k, policy):
        self.policies[k] = policy
        super().set_net_policy(k, policy)

    def set_net_search(self, entries):
        type(self).tables.append(entries)
        T = self.T
        for e in self.engines:
            e.close()
        self.engines = []
        for k in range(self.n_nets):
            own = {} if entries is None else {key: v for key, v in entries[k].items() if self.mode == 1 or key not in ("c_pw", "kappa")}
            e = O.OracleEngine(**dict(self.kw, n_trees=T, tree_id_base=self.kw.get("tree_id_base", 0) + k * T, **own))
            if self.policies[k] is not None:
                e.set_policy(self.policies[k])
            self.engines.append(e)

    @property
    def kmax(self):
        return max(e.kmax for e in self.engines)


def _sweep_agents(kind, sweep):
    from alphazero_gym_amd import run
    from alphazero_gym_amd.envs import make_game
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, dict(TP.FACADE[kind], device="cpu"))
    torch.manual_seed(7)
    return [run.make_agent(kind, dict(cfg, mcts=dict(cfg["mcts"], **{key: v[k] for key, v in sweep.items()})), make_game(cfg["game"]),
                           tree_id_base=k) for k in range(len(TP.SEEDS))], cfg


SWEEPS = {"discrete": dict(c_uct=[1.0, 4.0, 0.5], gamma=[1.0, 0.9, 0.97], epsilon=[0.0, 0.25, 0.0]),
          "continuous": dict(c_uct=[0.05, 0.2, 0.0125], gamma=[1.0, 0.9, 0.97])}


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_run_population_sweep_equals_standalone_agents(kind, monkeypatch):
    """run_population(sweep=...): agent k acts, and trains, bit for bit like a standalone agent built with its own settings."""
    from alphazero_gym_amd import _native, run
    from alphazero_gym_amd.agent import population
    monkeypatch.setattr(_native, "HipEngine", OracleNetSearch)
    OracleNetSearch.tables = []
    sweep = SWEEPS[kind]
    acts = [[] for _ in TP.SEEDS]
    orig = population.AgentPopulation.act

    def recording_act(self, envs, deterministic=False):
        outs = orig(self, envs, deterministic)
        for k, o in enumerate(outs):
            if o is not None:
                acts[k].append(o)
        return outs

    monkeypatch.setattr(population.AgentPopulation, "act", recording_act)
    torch.manual_seed(7)
    returns = run.run_population(kind, TP.SEEDS, TP.FACADE[kind], sweep=sweep)
    assert len(OracleNetSearch.tables) >= 1 and [s["c_uct"] for s in OracleNetSearch.tables[0]] == sweep["c_uct"]
    ref_agents, cfg = _sweep_agents(kind, sweep)
    ref_acts, ref_returns = TP._standalone(kind, ref_agents, cfg)
    assert returns == ref_returns
    for k in range(len(TP.SEEDS)):
        assert len(acts[k]) == len(ref_acts[k]) > 0
        for x, y in zip(acts[k], ref_acts[k]):
            TP._same(x, y)


def test_run_population_sweep_checks_its_arguments():
    from alphazero_gym_amd import run
    with pytest.raises(ValueError, match="one per seed"):
        run.run_population("discrete", TP.SEEDS, TP.FACADE["discrete"], sweep=dict(c_uct=[1.0, 2.0]))
    with pytest.raises(ValueError, match="not a per-agent search setting"):
        run.run_population("discrete", TP.SEEDS, TP.FACADE["discrete"], sweep=dict(n_rollouts=[8, 8, 8]))
    with pytest.raises(ValueError, match="not a per-agent search setting"):
        run.run_population("discrete", TP.SEEDS, TP.FACADE["discrete"], sweep=dict(c_pw=[1.0, 1.0, 1.0]))   # (no widening in discrete mode)
    with pytest.raises(ValueError, match="either sweep or agents"):
        run.run_population("discrete", TP.SEEDS, TP.FACADE["discrete"], sweep=dict(c_uct=[1.0, 2.0, 3.0]), agents=TP._agents("discrete")[0])


def test_agent_population_flag():
    """Without the flag: the error it always raised.  With it: agents that differ in the five settings only are grouped; any other
    difference still raises."""
    from alphazero_gym_amd.agent.population import AgentPopulation
    agents, _ = TP._agents("discrete")
    agents[1].mcts.c_uct, agents[2].mcts.gamma, agents[2].mcts.epsilon = 2.0, 0.9, 0.25
    with pytest.raises(ValueError, match=r"per-agent search hyper-parameters are not supported"):
        AgentPopulation(agents)
    pop = AgentPopulation(agents, per_agent_search=True)
    st = pop._net_settings()
    assert [s["c_uct"] for s in st] == [agents[0].mcts.c_uct, 2.0, agents[2].mcts.c_uct]
    assert [s["gamma"] for s in st][2] == 0.9 and st[2]["epsilon"] == 0.25 and set(st[0]) == {"c_uct", "gamma", "epsilon"}
    agents[1].mcts.n_rollouts += 1
    with pytest.raises(ValueError, match="c_uct, gamma, epsilon, c_pw and kappa only"):
        AgentPopulation(agents, per_agent_search=True)
    cont, _ = TP._agents("continuous")
    cont[0].mcts.c_pw, cont[1].mcts.kappa = 0.6, 0.45
    with pytest.raises(ValueError):
        AgentPopulation(cont)
    assert set(AgentPopulation(cont, per_agent_search=True)._net_settings()[0]) == set(_capi.NET_SEARCH_KEYS)
    cont[2].mcts.V_target_policy = "on_policy"
    with pytest.raises(ValueError):
        AgentPopulation(cont, per_agent_search=True)


def _policies(n, hidden, kind="discrete"):
    from alphazero_gym_amd.network.policies import make_policy
    out = []
    for s in range(n):
        torch.manual_seed(s)
        out.append(make_policy(4, 1, "discrete", hidden, "relu", num_actions=2) if kind == "discrete" else
                   make_policy(3, 1, "normal", hidden, "elu", num_components=1, action_bound=2.0))
    return out


def test_population_mcts_net_settings(monkeypatch):
    from alphazero_gym_amd import _native
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    monkeypatch.setattr(_native, "HipEngine", OracleNetSearch)
    kw = dict(trees_per_model=2, env_id=0, mode=0, n_rollouts=6, c_uct=1.5, gamma=1.0, epsilon=0.1, num_actions=2)
    nets = _policies(3, [16, 16])
    with pytest.raises(ValueError, match="one per net"):
        PopulationMCTS(nets, net_settings=[{}] * 2, **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        PopulationMCTS(nets, net_settings=[{}, {"c_puct": 1.0}, {}], **kw)
    with pytest.raises(ValueError, match="at most 256"):
        PopulationMCTS(_policies(3, [512, 512]), net_settings=[{}] * 3, **kw)
    OracleNetSearch.tables = []
    pop = PopulationMCTS(nets, **kw)                                   # the default: no table, today's calls only
    assert OracleNetSearch.tables == [] and pop.net_settings is None
    pop.close()
    pop = PopulationMCTS(nets, net_settings=[{}, {"c_uct": 6.0}, {"gamma": 0.9, "epsilon": 0.0}], **kw)
    want = [dict(c_uct=1.5, gamma=1.0, epsilon=0.1, c_pw=1.0, kappa=0.5), dict(c_uct=6.0, gamma=1.0, epsilon=0.1, c_pw=1.0, kappa=0.5),
            dict(c_uct=1.5, gamma=0.9, epsilon=0.0, c_pw=1.0, kappa=0.5)]
    assert OracleNetSearch.tables == [want] and pop.net_settings == want   # missing keys take the shared kwarg
    pop.set_net_settings([{"c_uct": 3.0}, {}, {}])
    assert OracleNetSearch.tables[-1][0]["c_uct"] == 3.0 and OracleNetSearch.tables[-1][1]["c_uct"] == 1.5
    with pytest.raises(ValueError):
        pop.set_net_settings([{}])
    pop.set_net_settings(None)
    assert OracleNetSearch.tables[-1] is None and pop.net_settings is None
    pop.close()


def test_engine_is_created_with_the_widest_widening(monkeypatch):
    """Continuous mode: the engine gets the (c_pw, kappa) pair of largest Kmax among the nets' -- not the shared kwarg, not net 0's."""
    from alphazero_gym_amd import _native
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    created = []

    class Recording(OracleNetSearch):
        def __init__(self, **kw):
            created.append((kw["c_pw"], kw["kappa"]))
            super().__init__(**kw)

    monkeypatch.setattr(_native, "HipEngine", Recording)
    st = [dict(c_pw=1.0, kappa=0.5), dict(c_pw=1.4, kappa=0.5), dict(c_pw=0.6, kappa=0.45)]
    assert [N.kmax_of(s, 50) for s in st] == [8, 10, 4]
    assert _capi.widest_pw([dict(s) for s in st], 50) == (1.4, 0.5)
    assert _capi.widest_pw([dict(c_pw=1.0, kappa=0.5), dict(c_pw=1.0, kappa=0.5)], 50) == (1.0, 0.5)
    pop = PopulationMCTS(_policies(3, [16], "normal"), trees_per_model=1, env_id=2, mode=1, n_rollouts=50, c_uct=0.05, gamma=1.0, c_pw=0.8,
                         kappa=0.5, net_settings=st)
    assert created == [(1.4, 0.5)] and pop.engine.kmax == 10
    pop.close()


def test_example_sweep_flags():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import population_selfplay_train as X
    a = X.parse_args(["--seeds", "0", "1", "2", "--c-ucts", "1", "2", "4", "--gammas", "1.0", "0.99", "0.9", "--search-epsilons", "0", "0.1", "0.2"])
    assert X.net_settings(a) == [dict(c_uct=1.0, gamma=1.0, epsilon=0.0), dict(c_uct=2.0, gamma=0.99, epsilon=0.1), dict(c_uct=4.0, gamma=0.9, epsilon=0.2)]
    a = X.parse_args(["--game", "Pendulum-v0", "--seeds", "0", "1", "--c-pws", "1.0", "1.5", "--kappas", "0.5", "0.6"])
    assert X.net_settings(a) == [dict(c_pw=1.0, kappa=0.5), dict(c_pw=1.5, kappa=0.6)]
    assert X.net_settings(X.parse_args(["--seeds", "0", "1"])) is None
    for flag in ("--c-ucts", "--gammas", "--search-epsilons", "--c-pws", "--kappas"):
        with pytest.raises(SystemExit):
            X.parse_args(["--seeds", "0", "1", "2", flag, "1.0", "2.0"])


def test_selfplay_passes_net_settings_through(monkeypatch):
    from alphazero_gym_amd import run
    seen = {}

    class Stop(Exception):
        pass

    def search(policies, games_per_net, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(run.PopulationSelfPlay, "_search", staticmethod(search))
    st = [{"c_uct": 1.0}, {"c_uct": 2.0}]
    with pytest.raises(Stop):
        run.PopulationSelfPlay(_policies(2, [16, 16]), game="CartPole-v0", games_per_net=2, n_rollouts=5, c_uct=1.5, net_settings=st)
    assert seen["net_settings"] == st
    seen.clear()
    with pytest.raises(Stop):
        run.PopulationSelfPlay(_policies(2, [16, 16]), game="CartPole-v0", games_per_net=2, n_rollouts=5, c_uct=1.5)
    assert "net_settings" not in seen   # the default leaves today's call as it was


# --------------------------------------------------------------------------------------------------------------------------- ABI


def test_ctypes_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of azg_net_search as gcc lays the header's struct out."""
    fields = [name for name, _ in _capi.AzgNetSearch._fields_]
    prints = "".join(f' printf("%zu ", offsetof(azg_net_search, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "azgym_population.h"\n'
                   'int main(void) { printf("%zu ", sizeof(azg_net_search));' + prints + " return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(_capi.AzgNetSearch)] + [getattr(_capi.AzgNetSearch, f).offset for f in fields]


def test_binding():
    """The entry point is optional for a library (the oracle has none): a stale library gives a clear error, not an AttributeError."""
    assert "set_net_search" in _capi.OPTIONAL_SYMBOLS and "set_net_search" not in O.fns()
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.0, gamma=1.0, num_actions=2)
    with pytest.raises(NotImplementedError, match="no set_net_search entry point"):
        e.set_net_search([dict(c_uct=1.0, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)] * 2)
    e.close()
    so = os.path.join(ROOT, "alphazero_gym_amd", "csrc", "libazgym_hip.so")
    if os.path.exists(so):   # (loads without a GPU)
        from alphazero_gym_amd import _native
        f = _native.fns()
        assert list(f["set_net_search"].argtypes) == [C.c_void_p, C.POINTER(_capi.AzgNetSearch), C.c_int32]
