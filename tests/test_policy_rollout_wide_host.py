"""Host side of the every-width policy rollout (azg_policy_rollout_ex, no GPU): the optional symbol, the wrapper's choice between
the two entry points against a fake function table, azg_rollout_info's layout, and the example's parser."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from alphazero_gym_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_symbol_is_optional_and_the_oracle_lacks_it():
    assert "policy_rollout_ex" in _capi.OPTIONAL_SYMBOLS and "policy_rollout_ex" not in _capi.SYMBOLS
    assert "policy_rollout_ex" not in O.fns() and "policy_rollout" not in O.fns()
    e = O.OracleEngine(env_id=0, mode=0, num_actions=2, n_trees=2, n_sims=4, c_uct=1.0, gamma=1.0)
    with pytest.raises(NotImplementedError):
        e.policy_rollout(4, 10)
    assert e.last_rollout_info is None
    e.close()


def test_rollout_info_layout():
    assert C.sizeof(_capi.AzgRolloutInfo) == 16
    assert [(n, t) for n, t in _capi.AzgRolloutInfo._fields_] == [("struct_size", C.c_int32), ("form", C.c_int32), ("launches", C.c_int32),
                                                                 ("team_fallbacks", C.c_int32)]
    assert _capi.ROLLOUT_FORM == {0: "group", 1: "team"}
    assert C.sizeof(_capi.AzgRolloutConfig) == 24   # (the new entry takes the old configuration as it is)


def _fake_engine(table, n_nets=2):
    e = object.__new__(_capi.Engine)
    e._f, e._h, e.n_nets = table, C.c_void_p(), n_nets
    return e


def _old(calls):
    def fn(h, cfg, returns, lengths, terminated, first_value):
        c = cfg._obj
        calls.append(("old", c.struct_size, c.episodes_per_net, c.max_episode_length, c.action_rule, c.game_id_base, c.episode))
        returns[0], lengths[0] = 1.5, 3
        return 0
    return fn


def _ex(calls, form, launches, fallbacks):
    def fn(h, cfg, returns, lengths, terminated, first_value, info):
        c, i = cfg._obj, info._obj
        calls.append(("ex", c.struct_size, c.episodes_per_net, c.max_episode_length, c.action_rule, c.game_id_base, c.episode, i.struct_size))
        returns[0], lengths[0], terminated[0], first_value[0] = 2.5, 4, 1, 0.25
        i.form, i.launches, i.team_fallbacks = form, launches, fallbacks
        return 0
    return fn


def test_wrapper_prefers_the_new_entry_and_keeps_its_info():
    calls = []
    e = _fake_engine({"policy_rollout": _old(calls), "policy_rollout_ex": _ex(calls, 1, 2, 0)})
    out = e.policy_rollout(3, 7, rule="sample", game_id_base=99, episode=5)
    assert calls == [("ex", 24, 3, 7, 1, 99, 5, 16)]
    assert sorted(out) == ["first_value", "lengths", "returns", "terminated"]
    assert out["returns"].shape == (2, 3) and out["returns"].dtype == np.float64 and out["terminated"].dtype == bool
    assert out["returns"][0, 0] == 2.5 and out["lengths"][0, 0] == 4 and out["terminated"][0, 0] and out["first_value"][0, 0] == 0.25
    assert e.last_rollout_info == {"form": "team", "launches": 2, "team_fallbacks": 0}
    # the group form after a counted fall-back
    e._f = {"policy_rollout_ex": _ex(calls, 0, 3, 1)}
    e.policy_rollout(3, 7)
    assert calls[-1] == ("ex", 24, 3, 7, 0, 0, 0, 16)
    assert e.last_rollout_info == {"form": "group", "launches": 3, "team_fallbacks": 1}
    e._h = C.c_void_p()


def test_wrapper_falls_back_to_the_old_entry():
    calls = []
    e = _fake_engine({"policy_rollout": _old(calls)}, n_nets=1)
    out = e.policy_rollout(2, 9, rule="mode", game_id_base=4)
    assert calls == [("old", 24, 2, 9, 0, 4, 0)]
    assert out["returns"].shape == (1, 2) and out["returns"][0, 0] == 1.5 and out["lengths"][0, 0] == 3
    assert e.last_rollout_info is None
    with pytest.raises(NotImplementedError):
        _fake_engine({}).policy_rollout(2, 9)


def test_wrapper_raises_the_engine_error_of_the_new_entry():
    def refuse(h, cfg, returns, lengths, terminated, first_value, info):
        return _capi.AZG_E_INVALID
    e = _fake_engine({"policy_rollout_ex": refuse, "last_error": lambda h: b"no"})
    with pytest.raises(_capi.EngineError) as ei:
        e.policy_rollout(2, 9)
    assert ei.value.code == _capi.AZG_E_INVALID


def test_example_parses_wide_eval():
    import population_selfplay_train as P
    a = P.parse_args(["--hidden", "512", "512", "--wide", "--seeds", "3", "11", "--games-per-seed", "32", "--eval-episodes", "32"])
    assert a.wide and a.eval_episodes == 32 and a.hidden == [512, 512] and a.seeds == [3, 11] and a.games_per_seed == 32
    a = P.parse_args(["--hidden", "1024", "1024", "1024", "1024", "--wide", "--seeds", "3", "--eval-episodes", "8", "--eval-rule", "sample"])
    assert a.wide and a.eval_episodes == 8 and a.eval_rule == "sample"
    assert "--wide" in P.__doc__ and "--eval-episodes" in P.__doc__
