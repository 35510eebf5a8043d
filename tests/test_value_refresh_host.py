"""Refreshing the ring's bootstrap values from the value head (include/azgym_refresh.h) on the CPU: the header compiles and the binding
is optional, ``PopulationSelfPlay.refresh_values``'s refusals and routing against a recording stub engine, the examples' flags, and
value_refresh_util's truth builders pinned on a hand-written 3-slot x 2-net example whose slot order has wrapped."""
import contextlib
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lambda_util as L
import nstep_util as N
import oracle_lib as O
import value_refresh_util as V
from alphazero_gym_amd import _capi, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_and_the_symbol_is_optional(tmp_path):
    assert "selfplay_refresh_values" in _capi.OPTIONAL_SYMBOLS and "selfplay_refresh_values" not in _capi.SYMBOLS
    assert "selfplay_refresh_values" not in O.fns()   # (the CPU oracle has no refresh: the truth is composed from its MLP evaluation)
    src = tmp_path / "use.c"
    src.write_text('#include "azgym_refresh.h"\n'
                   "int use(azg_engine* e) {\n"
                   "    const int32_t slots[2] = {1, 0};\n"
                   "    return azg_selfplay_refresh_values(e, slots, 2) + azg_selfplay_refresh_values(e, 0, 0);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert _capi.ABI_VERSION == 1


def test_an_engine_without_the_symbol_says_so():
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.5, gamma=1.0, num_actions=2)
    with pytest.raises(NotImplementedError, match="selfplay_refresh_values"):
        e.selfplay_refresh_values()
    e.close()


class _Native:
    """Stands where the library's function would: records (slots or None, n_slots) and returns ``code``."""

    def __init__(self, code=0):
        self.calls, self.code = [], code

    def __call__(self, handle, slots, n):
        self.calls.append((None if slots is None else [int(slots[i]) for i in range(n)], n, slots is None))
        return self.code


def test_the_binding_passes_null_for_every_slot_and_a_real_pointer_for_a_list():
    e = _capi.Engine.__new__(_capi.Engine)
    fn = _Native()
    e._f, e._h = {"selfplay_refresh_values": fn}, None
    e.selfplay_refresh_values()
    e.selfplay_refresh_values([3, 1, 3])
    e.selfplay_refresh_values(iter(np.asarray([2], np.int64)))
    e.selfplay_refresh_values([])   # (an empty list is a list, not "every slot": the pointer must not be NULL)
    assert fn.calls == [(None, 0, True), ([3, 1, 3], 3, False), ([2], 1, False), ([], 0, False)]


class _StubEngine:
    """The engine calls ``refresh_values`` may make, recorded in order."""

    def __init__(self, size=3, target_ready=False):
        self.log, self.size, self.target_ready, self.in_use = [], size, target_ready, "live"

    def selfplay_ring(self):
        return self.size, 0, self.size

    def weights_info(self):
        return {"in_use": self.in_use, "target_ready": self.target_ready}

    def use_weights(self, which):
        self.in_use = which
        self.log.append(("use_weights", which))

    def selfplay_refresh_values(self, slots=None):
        self.log.append(("refresh", slots, self.in_use))

    def selfplay_nstep_targets(self, n_step, gamma=None):
        self.log.append(("nstep", n_step, gamma))

    def selfplay_lambda_targets(self, n_step, td_lambda, gamma=None):
        self.log.append(("lambda", n_step, td_lambda, gamma))


class _StubMcts:
    def __init__(self, engine):
        self.engine = engine

    def sync_weights(self, force=False):
        self.engine.log.append(("sync_weights",))

    @contextlib.contextmanager
    def target_weights(self):
        self.engine.use_weights("target")
        try:
            yield self
        finally:
            self.engine.use_weights("live")


def _selfplay(cls=run.PopulationSelfPlay, n_step=3, lambda_rule=False, **engine_kw):
    sp = cls.__new__(cls)
    sp.engine = _StubEngine(**engine_kw)
    sp.mcts = _StubMcts(sp.engine)
    sp.n_nets, sp.games_per_net, sp.n_games = 2, 2, 4
    sp.n_step, sp.td_lambda, sp.target_gamma, sp._lambda_rule = n_step, (0.5 if lambda_rule else None), None, lambda_rule
    return sp


def test_refresh_values_routes_live_calls():
    sp = _selfplay()
    assert sp.refresh_values() == [0, 1, 2]
    assert sp.engine.log == [("sync_weights",), ("refresh", None, "live"), ("nstep", 3, None)]
    sp.engine.log.clear()
    assert sp.refresh_values(slots=(s for s in (2, 0, 2))) == [2, 0, 2]
    assert sp.engine.log == [("sync_weights",), ("refresh", [2, 0, 2], "live"), ("nstep", 3, None)]
    sp.engine.log.clear()
    assert sp.refresh_values(np.asarray([1]), nets="live") == [1]
    assert sp.engine.log[1] == ("refresh", [1], "live")
    lam = _selfplay(lambda_rule=True)   # (created with a lambda rule: the call ends with that one)
    lam.refresh_values([])
    assert lam.engine.log == [("sync_weights",), ("refresh", [], "live"), ("lambda", 3, 0.5, None)]
    assert run.DeviceSelfPlay.refresh_values is run.PopulationSelfPlay.refresh_values
    sig = inspect.signature(run.PopulationSelfPlay.refresh_values)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(slots=None)   # (``nets`` comes from _nets_keyword)


def test_refresh_values_with_target_weights_and_its_refusals():
    sp = _selfplay(target_ready=True)
    assert sp.refresh_values([1], nets="target") == [1]
    assert sp.engine.log == [("sync_weights",), ("use_weights", "target"), ("refresh", [1], "target"), ("use_weights", "live"), ("nstep", 3, None)]
    assert sp.engine.in_use == "live" and sp._nets == "live"
    no = _selfplay(target_ready=False)
    with pytest.raises(RuntimeError, match=r"refresh_values\(nets='target'\).*upload_target_flat"):
        no.refresh_values(nets="target")
    assert no.engine.log == [("sync_weights",)] and no._nets == "live"   # (nothing was refreshed, no target was computed)
    with pytest.raises(ValueError, match="nets must be 'live' or 'target'"):
        no.refresh_values(nets="ema")
    off = _selfplay(n_step=None)
    with pytest.raises(RuntimeError, match=r"refresh_values needs .*n_step="):
        off.refresh_values()
    assert off.engine.log == []
    with pytest.raises((TypeError, ValueError)):
        _selfplay().refresh_values(["a"])


@pytest.mark.parametrize("example", ["selfplay_train", "population_selfplay_train"])
def test_examples_parse_the_refresh_flags(example, capsys):
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    mod = importlib.import_module(example)
    base = ["--game", "CartPole-v0", "--device", "cuda"]
    assert mod.parse_args(base).refresh_values_every == 0
    a = mod.parse_args(base + ["--n-step", "3", "--replay-steps", "4", "--steps-per-iter", "2", "--refresh-values-every", "2"])
    assert a.refresh_values_every == 2
    for bad in (["--refresh-values-every", "1"], ["--refresh-values-every", "1", "--n-step", "3"],
                ["--refresh-values-every", "-1", "--n-step", "3", "--replay-steps", "4", "--steps-per-iter", "2"]):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)
    if example == "population_selfplay_train":
        assert not mod.parse_args(base).refresh_target
        ring = ["--n-step", "3", "--replay-steps", "4", "--steps-per-iter", "2", "--trainer", "device-epoch"]
        a = mod.parse_args(base + ring + ["--refresh-values-every", "1", "--ema-decay", "0.9", "--refresh-target"])
        assert a.refresh_target and a.refresh_values_every == 1
        a = mod.parse_args(base + ["--n-step", "3", "--trainer", "device-epoch", "--refresh-values-every", "1"])   # (the rows stay in the ring)
        assert a.refresh_values_every == 1
        for bad in (ring + ["--refresh-values-every", "1", "--refresh-target"], ring + ["--ema-decay", "0.9", "--refresh-target"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the truth builders, by hand

# 3 slots x 2 nets x 1 game, one observation column.  The ring has wrapped: slot 0 holds step 3 (the newest), slot 1 step 1 (the
# oldest), slot 2 step 2.  Net 0's value is 2 x, net 1's is x + 0.5.
OBS = np.asarray([[[3.0], [30.0]], [[1.0], [10.0]], [[2.0], [20.0]]], np.float32)
HELD = np.asarray([3, 1, 2])
REWARD = np.asarray([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
END = np.asarray([[N.END_NONE, N.END_NONE], [N.END_NONE, N.END_NONE], [N.END_NONE, N.END_LENGTH]], np.int32)


def _evaluate(k, x):
    assert x.dtype == np.float32 and x.shape == (3, 1)
    return (np.float32(2.0) * x[:, 0]) if k == 0 else (x[:, 0] + np.float32(0.5))


def test_net_values_gives_every_net_its_own_rows():
    got = V.net_values(OBS, 1, _evaluate)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, [[6.0, 30.5], [2.0, 10.5], [4.0, 20.5]])
    # two games per net: games 0, 1 are net 0's, and the rows reach the evaluator slot-major
    seen = []

    def ev(k, x):
        seen.append((k, x[:, 0].tolist()))
        return x[:, 0].copy()
    obs = np.arange(12, dtype=np.float32).reshape(3, 4, 1)
    np.testing.assert_array_equal(V.net_values(obs, 2, ev), obs[:, :, 0].astype(np.float64))
    assert seen == [(0, [0.0, 1.0, 4.0, 5.0, 8.0, 9.0]), (1, [2.0, 3.0, 6.0, 7.0, 10.0, 11.0])]
    # the widening is exact: a float32 that is no short decimal keeps its bits
    third = V.net_values(np.full((1, 1, 1), 1.0, np.float32), 1, lambda k, x: x[:, 0] / np.float32(3.0))
    assert third[0, 0] == float(np.float32(1.0) / np.float32(3.0)) and third[0, 0] != 1.0 / 3.0


def test_refreshed_takes_the_listed_slots_only():
    old = np.asarray([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    truth = V.net_values(OBS, 1, _evaluate)
    np.testing.assert_array_equal(V.refreshed(old, truth), truth)
    np.testing.assert_array_equal(V.refreshed(old, truth, [2, 2]), [[0.1, 0.2], [0.3, 0.4], [4.0, 20.5]])
    np.testing.assert_array_equal(V.refreshed(old, truth, [2, 0]), [[6.0, 30.5], [0.3, 0.4], [4.0, 20.5]])
    np.testing.assert_array_equal(V.refreshed(old, truth, []), old)


def test_slot_targets_sees_the_wrapped_ring_in_chronological_order():
    value = V.net_values(OBS, 1, _evaluate)   # by slot: [[6, 30.5], [2, 10.5], [4, 20.5]]; by time: 2, 4, 6 and 10.5, 20.5, 30.5
    # n_step 1, gamma 0.5.  Game 0 (no end): oldest 1 + 0.5 * 4 = 3, middle 1 + 0.5 * 6 = 4, newest its own value 6.
    # Game 1 (step 2, in slot 2, hit the time limit): oldest 1 + 0.5 * 20.5 = 11.25, middle its own value 20.5, newest 30.5.
    got = V.slot_targets(REWARD, value, END, HELD, lambda r, v, e: N.nstep_returns(r, v, e, 1, 0.5))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.asarray([[6.0, 30.5], [3.0, 11.25], [4.0, 20.5]], np.float32))
    # n_step 0: every row's own value, whatever the order
    np.testing.assert_array_equal(V.slot_targets(REWARD, value, END, HELD, lambda r, v, e: N.nstep_returns(r, v, e, 0, 0.5)), value.astype(np.float32))
    # per-net gamma (1 and 0.5) at n_step 2: game 0 oldest 1 + 1 + 6 = 8; game 1 oldest stops at the time limit: 11.25
    got = V.slot_targets(REWARD, value, END, HELD, lambda r, v, e: N.nstep_returns(r, v, e, 2, np.asarray([1.0, 0.5])))
    np.testing.assert_array_equal(got, np.asarray([[6.0, 30.5], [8.0, 11.25], [7.0, 20.5]], np.float32))
    # the lambda form at lambda 1 is the n-step return, and it agrees with nstep_util's run-indexed builder on an unwrapped ring
    lam = V.slot_targets(REWARD, value, END, HELD, lambda r, v, e: L.lambda_returns(r, v, e, 2, 1.0, np.asarray([1.0, 0.5])))
    np.testing.assert_array_equal(lam, got)
    order = np.argsort(HELD)
    np.testing.assert_array_equal(V.slot_targets(REWARD[order], value[order], END[order], np.arange(3), lambda r, v, e: N.nstep_returns(r, v, e, 2, 0.9)),
                                  N.ring_targets(REWARD[order], value[order], END[order], np.arange(3), 2, 0.9))
    with pytest.raises(AssertionError):   # (slots that do not hold a contiguous range of steps)
        V.slot_targets(REWARD, value, END, [3, 1, 5], lambda r, v, e: N.nstep_returns(r, v, e, 1, 0.5))


def test_case_truth_is_the_oracles_evaluation_net_by_net():
    """The evaluator the GPU tests use, on the population case: net k's rows carry the oracle's value under net k's weights."""
    case = V.CASES["population"]
    obs = np.random.default_rng(5).standard_normal((3, case.games, case.net[0])).astype(np.float32)
    blobs = [V.refresh_blob(case, k) for k in range(case.nets)]
    got = V.case_truth(case, obs, blobs)
    assert got.shape == (3, case.games) and got.dtype == np.float64
    T = case.T
    for k in range(case.nets):
        o = O.OracleEngine(**dict(case.net_kw(k), n_trees=1))
        o.set_weights(case.desc(), blobs[k])
        for s in range(3):
            want = o.mlp_eval(obs[s, k * T:(k + 1) * T])[0]
            np.testing.assert_array_equal(V.bits64(got[s, k * T:(k + 1) * T]), V.bits64(want.astype(np.float64)))
        o.close()
    assert len({got[0, k * T] for k in range(case.nets)}) == case.nets and np.ptp(got) > 0.0   # (the nets and the rows do differ)
    assert C.sizeof(C.c_double) == 8
