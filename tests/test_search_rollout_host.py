"""Search rollouts (azg_search_rollout), the part that runs without a GPU: the CPU truth of tests/search_rollout_util.py pinned to the
restatement of device self-play, what cartpole_falls is there for, the truth's teeth, the ABI's additions, the Python layer's
refusals, the examples' flag and the sizes of the GPU file's cases."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import reanalyse_util as R
import search_rollout_util as U
import selfplay_ref as SR
from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _episodes_of(trace, T):
    """Per game: the (return, length, done) of the episodes a cpu_selfplay trace finished, in order; returns added up as the step
    does (0.0 + r1 + r2 ...)."""
    eps, ret, n = [[] for _ in range(T)], np.zeros(T), np.zeros(T, np.int64)
    for r in sorted(trace, key=lambda r: (r["step"], r["game"])):
        j = r["game"]
        ret[j] = ret[j] + r["reward"]
        n[j] += 1
        if r["ended"]:
            eps[j].append((ret[j], int(n[j]), bool(r["done"])))
            ret[j], n[j] = 0.0, 0
    return eps


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "mcc", "population"])
def test_the_truth_is_the_restated_selfplay_on_its_own_start_states(name):
    """game_id_base = tree_id_base, episode 0, index_base 0 and the self-play's rule: every game's episodes equal the per-episode
    returns and lengths read off cpu_selfplay's trace over the same number of steps, bit for bit (net by net; mcc without its slope
    roots; cartpole carries counts)."""
    case = U.CASES[name]
    compared, carried = 0, False
    for k in range(case.nets):
        kw = case.net_kw(k)
        cfg = U.config(name, game_id_base=kw.get("tree_id_base", 0), episode=0, index_base=0, final_selection="max_visit", deterministic=False,
                       temperature=1.0, agent_epsilon=0.0)
        got = U.cpu_search_rollout(kw, case.desc(), case.blob(k), case.T, cfg)
        trace = []
        SR.cpu_selfplay(kw, case.desc(), case.blob(k), case.T, got["steps"], begin=dict(max_episode_length=case.max_len), trace=trace)
        carried = carried or any(r["carry_in"] > 0 for r in trace)
        eps = _episodes_of(trace, case.T)
        for j in range(case.T):
            assert len(eps[j]) >= U.E   # (the self-play plays on where the rollout parks the game)
            for i in range(U.E):
                want = eps[j][i]
                assert R.bits64(got["returns"][j, i]) == R.bits64(want[0]), (name, k, j, i)
                assert (got["lengths"][j, i], got["terminated"][j, i]) == want[1:], (name, k, j, i)
                compared += 1
    assert compared == case.games * U.E
    assert carried == (not case.cont)


def test_the_truth_adds_rewards_as_selfplay_does():
    """Pendulum, episodes of 3 steps, 6 steps: the self-play's fsum is (0.0 + returns[:, 0]) + returns[:, 1], bit for bit."""
    case = U.CASES["pendulum"]
    kw = case.net_kw(0)
    cfg = U.config("pendulum", max_episode_length=3, game_id_base=kw["tree_id_base"], episode=0, index_base=0, deterministic=False, agent_epsilon=0.0)
    got = U.cpu_search_rollout(kw, case.desc(), case.blob(0), case.T, cfg)
    assert got["steps"] == 6 and (got["lengths"] == 3).all() and not got["terminated"].any()
    sp = SR.cpu_selfplay(kw, case.desc(), case.blob(0), case.T, 6, begin=dict(max_episode_length=3))
    assert (sp["fcnt"] == 2).all()
    np.testing.assert_array_equal(R.bits64(sp["fsum"]), R.bits64((0.0 + got["returns"][:, 0]) + got["returns"][:, 1]))


def test_cartpole_falls_parks_games_at_different_steps():
    """What the case is there for, on the CPU truth alone (weight seed and length limit: search_rollout_util.FALLS_*)."""
    t = U.truth("cartpole_falls")
    assert not U.config("cartpole_falls")["deterministic"]
    assert t["terminated"].mean() >= 0.25
    assert (~t["terminated"]).any() and (t["lengths"][~t["terminated"]] == U.FALLS_MAX_LEN).all()
    assert len(set(t["totals"].tolist())) >= 3
    assert t["steps"] < U.E * U.FALLS_MAX_LEN   # (the call ends early: the bound is not what stops it)


@pytest.mark.parametrize("mutant,name", [("parked_keeps_root", "pendulum"), ("carry_kept_over_end", "cartpole"),
                                         ("step_restarts_per_episode", "pendulum"), ("step_restarts_per_episode", "cartpole_falls")])
def test_the_truth_has_teeth(mutant, name):
    """Each wrong variant of the contract changes the truth of some case: the outputs, or what the call leaves behind (the parked
    roots and carried counts: what its last search, which azg_results describes, started from)."""
    good, bad = U.truth(name), U.truth(name, mutant)
    changed = [k for k in ("returns", "lengths", "terminated", "roots", "carry") if not np.array_equal(good[k], bad[k])]
    assert changed, (mutant, name)
    if mutant == "step_restarts_per_episode":
        assert not U.same(good, bad)


def test_abi_additions_are_optional_symbols(tmp_path):
    assert "search_rollout" in _capi.OPTIONAL_SYMBOLS and "search_rollout" not in _capi.SYMBOLS
    assert "search_rollout" not in O.fns()   # (the CPU oracle has no search rollout: the truth is composed from its searches)
    src = tmp_path / "use.c"
    src.write_text('#include "azgym_search_rollout.h"\n'
                   "int use(azg_engine* e, double* returns, int32_t* lengths) {\n"
                   "    azg_search_rollout_config c = {0};\n"
                   "    azg_search_rollout_info info = {0};\n"
                   "    c.struct_size = (int32_t)sizeof(c); c.episodes_per_game = 2; c.max_episode_length = 5; c.final_selection = AZG_FS_MAX_VISIT;\n"
                   "    c.deterministic = 1; c.poll_steps = 8; c.game_id_base = 1u << 30; c.episode = 0; c.index_base = 3u << 30;\n"
                   "    c.temperature = 1.0; c.agent_epsilon = 0.0;\n"
                   "    info.struct_size = (int32_t)sizeof(info);\n"
                   "    return azg_search_rollout(e, &c, returns, lengths, 0, &info) + info.steps + info.polls;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert _capi.ABI_VERSION == 1
    assert (_capi.AzgSearchRolloutConfig.struct_size.offset, _capi.AzgSearchRolloutConfig.temperature.offset) == (0, 40)
    import ctypes as C
    assert C.sizeof(_capi.AzgSearchRolloutConfig) == 56 and C.sizeof(_capi.AzgSearchRolloutInfo) == 12


def test_an_engine_without_the_symbol_says_so():
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.5, gamma=1.0, num_actions=2)
    e.set_weights(_capi.make_desc(4, [64], 2, "relu"), O.make_weights(1, 4, [64], 2))
    with pytest.raises(NotImplementedError):
        e.search_rollout(1, 5)
    e.close()


class _NoEngine:
    """Stands where the engine would: any native call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"evaluate_search reached the engine ({name}) with bad arguments")


def test_evaluate_search_refuses_bad_arguments_before_any_native_call():
    from alphazero_gym_amd import run
    assert run.EVAL_SEARCH_INDEX_BASE == U.INDEX_BASE == 3 << 30
    assert run.EVAL_SEARCH_INDEX_BASE > run.REANALYSE_INDEX_BASE and run.EVAL_SEARCH_INDEX_BASE + 10 ** 6 < 1 << 32
    sp = run.PopulationSelfPlay.__new__(run.PopulationSelfPlay)
    sp.engine = sp.mcts = _NoEngine()
    sp.max_episode_length, sp.tree_id_base, sp.n_games, sp.n_nets, sp.games_per_net = 10, 0, 4, 2, 2
    for bad in (dict(episodes_per_game=0), dict(final_selection="best"), dict(max_episode_length=0), dict(poll_steps=0), dict(temperature=0.0),
                dict(temperature=float("nan")), dict(agent_epsilon=-0.1), dict(agent_epsilon=1.5), dict(index_base=1 << 32), dict(index_base=-1),
                dict(episode=-1)):
        with pytest.raises(ValueError, match="evaluate_search"):
            sp.evaluate_search(**bad)
    with pytest.raises(AssertionError, match="reached the engine"):   # (good arguments do go on to the engine)
        sp.evaluate_search()
    import inspect
    sig = inspect.signature(run.PopulationSelfPlay.evaluate_search)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        episodes_per_game=1, final_selection="max_visit", deterministic=True, temperature=1.0, agent_epsilon=0.0, max_episode_length=None,
        episode=0, game_id_base=None, index_base=run.EVAL_SEARCH_INDEX_BASE, poll_steps=8)
    assert run.DeviceSelfPlay.evaluate_search is run.PopulationSelfPlay.evaluate_search


@pytest.mark.parametrize("example", ["selfplay_train", "population_selfplay_train"])
def test_examples_parse_eval_search_episodes(example):
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    mod = importlib.import_module(example)
    assert mod.parse_args(["--device", "cpu"]).eval_search_episodes == 0
    assert mod.parse_args(["--device", "cpu", "--eval-search-episodes", "3"]).eval_search_episodes == 3
    with pytest.raises(SystemExit):
        mod.parse_args(["--device", "cpu", "--eval-search-episodes", "-1"])


def test_gpu_cases_stay_small():
    import test_search_rollout as T
    assert set(T.ALL) == set(U.CASES) == set(R.CASES) | {"cartpole_falls"}
    sizes = {name: case.games for name, case in U.CASES.items()}
    assert sizes["many_children"] == 65 and sizes["wide"] == sizes["wide_team"] == 32
    assert sizes["population_wide"] == sizes["population_wide_team"] == 64
    assert (U.CASES["population"].nets, U.CASES["population"].T, U.CASES["population"].net_rollouts) == (3, 11, [16, 9, 1])
    for name, case in U.CASES.items():
        assert case.n_sims <= 32 and case.games <= 96, name
        assert sizes[name] == 33 or name in ("many_children", "wide", "wide_team", "population_wide", "population_wide_team"), name
        assert U.E * U.config(name)["max_episode_length"] <= 64, name   # (searches per call)
        assert name == "cartpole_falls" or (case.n_sims <= 16 and 3 <= case.max_len <= 5), name
