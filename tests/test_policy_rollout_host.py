"""Host side of the policy rollouts (no GPU): the binding on a library without the entry point, ``evaluate``'s argument checks
against a recording fake engine, and the example's parser."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from alphazero_gym_amd import _capi, run

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_oracle_binds_without_the_symbol():
    assert "policy_rollout" in _capi.OPTIONAL_SYMBOLS and "policy_rollout" not in O.fns()
    e = O.OracleEngine(env_id=0, mode=0, num_actions=2, n_trees=2, n_sims=4, c_uct=1.0, gamma=1.0)
    with pytest.raises(NotImplementedError):
        e.policy_rollout(4, 10)
    e.close()


def test_rollout_config_layout():
    import ctypes as C
    assert C.sizeof(_capi.AzgRolloutConfig) == 24
    assert [n for n, _ in _capi.AzgRolloutConfig._fields_] == ["struct_size", "episodes_per_net", "max_episode_length", "action_rule",
                                                               "game_id_base", "episode"]
    assert _capi.ROLLOUT_RULE == {"mode": 0, "sample": 1}


class _FakeEngine:
    def __init__(self, n_nets):
        self.n_nets, self.calls = n_nets, []

    def policy_rollout(self, episodes_per_net, max_episode_length, rule="mode", game_id_base=0, episode=0):
        self.calls.append(("policy_rollout", episodes_per_net, max_episode_length, rule, game_id_base, episode))
        shape = (self.n_nets, episodes_per_net)
        returns = np.arange(self.n_nets * episodes_per_net, dtype=np.float64).reshape(shape)
        return {"returns": returns, "lengths": np.ones(shape, np.int32), "terminated": np.zeros(shape, bool),
                "first_value": np.zeros(shape, np.float32)}


class _FakeSearch:
    def __init__(self, engine):
        self.engine = engine

    def sync_weights(self, force=False):
        self.engine.calls.append(("sync_weights", force))


def _selfplay(cls=run.PopulationSelfPlay, n_nets=3, games_per_net=4, tree_id_base=0, max_len=50):
    sp = object.__new__(cls)
    sp.engine = _FakeEngine(n_nets)
    sp.mcts = _FakeSearch(sp.engine)
    sp.n_nets, sp.games_per_net, sp.n_games = n_nets, games_per_net, n_nets * games_per_net
    sp.max_episode_length, sp.tree_id_base = max_len, tree_id_base
    return sp


def test_evaluate_defaults_and_order():
    sp = _selfplay(tree_id_base=24)
    out = sp.evaluate(5)
    # pending weight uploads first, through play's path; then one rollout with the self-play's own length limit
    assert sp.engine.calls == [("sync_weights", False), ("policy_rollout", 5, 50, "mode", run.EVAL_GAME_ID_BASE, 0)]
    assert run.EVAL_GAME_ID_BASE >= sp.tree_id_base + sp.n_games   # above every self-play game id of the engine
    np.testing.assert_array_equal(out["mean_return"], out["returns"].mean(axis=1))
    assert out["mean_return"].shape == (3,)
    sp.evaluate(2, rule="sample", max_episode_length=7, episode=3, game_id_base=99)
    assert sp.engine.calls[-1] == ("policy_rollout", 2, 7, "sample", 99, 3)


def test_evaluate_default_base_stays_above_high_game_ids():
    sp = _selfplay(tree_id_base=run.EVAL_GAME_ID_BASE + 5)
    sp.evaluate(1)
    assert sp.engine.calls[-1][4] == sp.tree_id_base + sp.n_games


def test_evaluate_one_net_form():
    sp = _selfplay(cls=run.DeviceSelfPlay, n_nets=1, games_per_net=8, tree_id_base=16)
    out = sp.evaluate(3)
    assert out["returns"].shape == (1, 3) and out["mean_return"].shape == (1,)


@pytest.mark.parametrize("kw", [dict(episodes_per_net=0), dict(episodes_per_net=-2), dict(episodes_per_net=4, rule="greedy"),
                                dict(episodes_per_net=4, rule=0), dict(episodes_per_net=4, max_episode_length=0)])
def test_evaluate_refuses(kw):
    sp = _selfplay()
    with pytest.raises(ValueError):
        sp.evaluate(**kw)
    assert sp.engine.calls == []   # refused before anything is uploaded or launched


def test_example_parser_defaults():
    import population_selfplay_train as P
    a = P.parse_args([])
    assert a.eval_episodes == 0 and a.eval_rule == "mode"
    assert a.trainer == "torch" and a.games_per_seed == 64 and a.seeds == [0, 1, 2, 3]
    a = P.parse_args(["--eval-episodes", "16", "--eval-rule", "sample"])
    assert a.eval_episodes == 16 and a.eval_rule == "sample"
    with pytest.raises(SystemExit):
        P.parse_args(["--eval-rule", "greedy"])
