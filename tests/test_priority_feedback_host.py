"""Priorities fed back from the trainer's value errors, on the CPU: the numpy restatement (tests/priority_feedback_util.py) on
hand-computed cases -- the sentinel, NaN, +inf and 0, a net with no seen row, the ordering of non-negative float32 by their bits --
the ctypes structs, the Python refusals that need no device and the ABI of the built library (include/azgym_priority.h,
include/azgym_train_errors.h)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import priority_feedback_util as F
import priority_util as P
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer

NAN, INF = np.float32("nan"), np.float32("inf")


# ------------------------------------------------------------------------------------------------ the rule

def test_the_error_is_the_float64_difference_rounded_once():
    raw0 = np.asarray([0.1, -0.1, 1.0, 3.0e38, NAN, INF, 1.0 + 2.0 ** -23], np.float32)
    z = np.asarray([0.1, 0.1, 1.0 + 2.0 ** -23, -3.0e38, 0.0, 1.0, 1.0], np.float32)
    e = F.loss_errors(raw0, z)
    assert e.dtype == np.float32
    assert e[0] == 0.0 and F.bits(e[0:1])[0] == 0                               # +0, not -0
    assert e[1] == np.float32(np.float64(np.float32(0.1)) * 2.0)
    assert e[2] == np.float32(2.0 ** -23) and e[6] == np.float32(2.0 ** -23)     # symmetric
    assert e[3] == INF                                                           # 6e38 rounds to +inf in float32; float64 holds it
    assert np.isnan(e[4]) and e[5] == INF


def test_non_negative_floats_order_like_their_bits():
    rng = np.random.default_rng(3)
    x = np.concatenate([np.asarray([0.0, 1e-45, 1e-38, 1.0, 3.4e38, INF], np.float32),
                        (10.0 ** rng.uniform(-44, 38, 500)).astype(np.float32)])
    by_value = np.sort(x)
    by_bits = np.sort(x.view(np.uint32)).view(np.float32)
    np.testing.assert_array_equal(F.bits(by_value), F.bits(by_bits))
    assert F.bits(np.asarray([INF]))[0] == 0x7F800000 and F.bits(np.asarray([F.UNSEEN]))[0] == F.UNSEEN_BITS
    assert F.seen_max(x) == INF and F.seen_max(x[:5]) == np.float32(3.4e38)
    # the sentinel, NaN and other negatives do not count; -0.0 counts as +0.0
    assert F.seen_max(np.asarray([F.UNSEEN, NAN], np.float32)) is None
    m = F.seen_max(np.asarray([F.UNSEEN, NAN, -0.0], np.float32))
    assert m == 0.0 and F.bits(np.asarray([m]))[0] == 0
    assert F.seen_max(np.asarray([F.UNSEEN, 0.25, NAN, 2.0, 0.5], np.float32)) == np.float32(2.0)


def test_d_of_seen_and_unseen_rows_by_hand():
    """Two nets of two games, three slots.  Net 0: seen 0.25, NaN, 2.0 and three unseen; net 1: nothing seen but a NaN."""
    U = F.UNSEEN
    err = np.asarray([[0.25, U, U, U],
                      [NAN, 2.0, NAN, U],
                      [U, U, U, U]], np.float32)
    d = F.trained_d(err, 2, F.MAX)
    want = np.asarray([[0.25, 2.0, 1.0, 1.0],
                       [NAN, 2.0, NAN, 1.0],
                       [2.0, 2.0, 1.0, 1.0]], np.float32)
    np.testing.assert_array_equal(F.bits(d), F.bits(want))
    # a net whose only seen error is 0 takes 0, not 1; +inf counts as the maximum
    d = F.trained_d(np.asarray([[0.0, U], [U, INF]], np.float32), 1, F.MAX)
    np.testing.assert_array_equal(d, np.asarray([[0.0, INF], [INF, INF]], np.float32))
    d = F.trained_d(np.asarray([[0.0, U], [U, NAN]], np.float32), 1, F.MAX)
    np.testing.assert_array_equal(F.bits(d), F.bits(np.asarray([[0.0, 0.0], [0.0, NAN]], np.float32)))
    # a constant, and the value gap of the unseen rows only
    d = F.trained_d(err, 2, F.CONSTANT, unseen_d=0.75)
    assert (d[err == U] == np.float32(0.75)).all() and F.bits(d[0, 0:1])[0] == F.bits(np.asarray([0.25]))[0] and np.isnan(d[1, 0])
    gap = np.arange(12, dtype=np.float32).reshape(3, 4) + 10.0
    d = F.trained_d(err, 2, F.VALUE_GAP, gap=gap)
    np.testing.assert_array_equal(d[err == U], gap[err == U])
    assert d[0, 0] == np.float32(0.25) and d[1, 1] == np.float32(2.0)


def test_q_at_the_edges_by_hand():
    """alpha = 1 with a tiny eps: an error of 0 lands on q = 1 (p = eps < 2^-20), NaN on 1, +inf and 1e9 on 2^40; alpha = 0: every row
    2^20, NaN and the sentinel included; a net with nothing seen has d = 1: q = priorities(1.0)."""
    U = F.UNSEEN
    err = np.asarray([[0.0, NAN, INF, 1e9, 0.5, U]], np.float32)
    q = F.trained_priorities(err, 1, 1.0, 1e-9, F.CONSTANT, unseen_d=0.0)
    assert [int(v) for v in q[0, :4]] == [1, 1, P.Q_MAX, P.Q_MAX] and int(q[0, 5]) == 1
    assert 1 < int(q[0, 4]) < P.Q_MAX and int(q[0, 4]) == int(P.priorities(np.asarray([0.5], np.float32), 1.0, 1e-9)[0])
    q = F.trained_priorities(err, 1, 1.0, 1e-9, F.MAX)
    assert int(q[0, 5]) == P.Q_MAX                                               # (+inf is the largest seen error)
    q = F.trained_priorities(err, 1, 0.0, 1e-3, F.MAX)
    assert (q == P.Q_ONE).all()
    q = F.trained_priorities(np.asarray([[U, NAN], [U, U]], np.float32), 1, 0.6, 1e-3, F.MAX)
    one = int(P.priorities(np.asarray([1.0], np.float32), 0.6, 1e-3)[0])
    assert [int(v) for v in q.reshape(-1)] == [one, 1, one, one] and one > P.Q_ONE // 2


# ------------------------------------------------------------------------------------------------ structs and symbols

def test_struct_sizes_and_symbols():
    cfg = _capi.AzgTrainedPriorityConfig
    assert C.sizeof(cfg) == 20
    assert [(n, getattr(cfg, n).offset) for n, _ in cfg._fields_] == [("struct_size", 0), ("unseen", 4), ("alpha", 8), ("eps", 12),
                                                                    ("unseen_d", 16)]
    assert (_capi.UNSEEN_MAX, _capi.UNSEEN_VALUE_GAP, _capi.UNSEEN_CONSTANT) == (F.MAX, F.VALUE_GAP, F.CONSTANT)
    assert F.bits(np.asarray([_capi.ERR_UNSEEN]))[0] == F.UNSEEN_BITS
    from alphazero_gym_amd import _native
    lib = _native.lib()
    for name in ("selfplay_keep_errors", "selfplay_errors_device", "selfplay_error_values", "selfplay_set_error_values",
                 "selfplay_priorities_trained", "trainer_loss_errors", "trainer_loss_nets_errors", "trainer_epoch_opt_errors",
                 "trainer_epoch_nets_errors"):
        assert hasattr(lib, "azg_" + name), name
        assert name in _capi.OPTIONAL_SYMBOLS
    for method in ("loss_errors", "loss_nets_errors", "epoch_opt_errors", "epoch_nets_errors"):
        assert callable(getattr(_capi.Trainer, method))
    for method in ("selfplay_keep_errors", "selfplay_errors_device", "selfplay_error_values", "selfplay_set_error_values",
                   "selfplay_priorities_trained"):
        assert callable(getattr(_capi.Engine, method))
    with pytest.raises(NotImplementedError, match="azg_trainer_epoch_opt_errors"):
        _capi._require({}, "trainer_epoch_opt_errors")


# ------------------------------------------------------------------------------------------------ refusals without a GPU

def test_python_refusals():
    assert _capi.unseen_mode("max") == (_capi.UNSEEN_MAX, 0.0)
    assert _capi.unseen_mode("value_gap") == (_capi.UNSEEN_VALUE_GAP, 0.0)
    assert _capi.unseen_mode(0.5) == (_capi.UNSEEN_CONSTANT, 0.5) and _capi.unseen_mode(0) == (_capi.UNSEEN_CONSTANT, 0.0)
    for bad in ("min", "", None, True, -1.0, float("nan"), float("inf"), [1.0]):
        with pytest.raises(ValueError, match="feedback"):
            _capi.unseen_mode(bad)
    kw = dict(game="CartPole-v0", games_per_net=4, n_rollouts=8, c_uct=1.5, n_step=3)
    for bad in ("min", -1.0, float("nan")):
        with pytest.raises(ValueError, match="feedback"):
            run.PopulationSelfPlay([object()], prioritized={"alpha": 0.6, "feedback": bad}, **kw)
    with pytest.raises(ValueError, match="needs n_step"):
        run.PopulationSelfPlay([object()], prioritized={"alpha": 0.6, "feedback": "max"}, **dict(kw, n_step=None))
    # errors() / set_errors(): without feedback, before the engine is touched
    for prioritized in (None, dict(alpha=0.6, eps=1e-3), dict(alpha=0.6, eps=1e-3, beta=0.4)):
        fake = types.SimpleNamespace(prioritized=prioritized, engine=None)
        fake._feedback_refusal = types.MethodType(run.PopulationSelfPlay._feedback_refusal, fake)
        with pytest.raises(RuntimeError, match='"feedback"'):
            run.PopulationSelfPlay.errors(fake)
        with pytest.raises(RuntimeError, match='"feedback"'):
            run.PopulationSelfPlay.set_errors(fake, np.zeros(4, np.float32))
    # the trainer: errors=True needs the device losses and a self-play engine built with feedback
    with pytest.raises(ValueError, match='needs a trainer built with losses="device"'):
        PopulationTrainer.train_epoch_ring(types.SimpleNamespace(losses="torch"), None, None, errors=True)
    dev_trainer = types.SimpleNamespace(losses="device")
    for prioritized in (None, dict(alpha=0.6, eps=1e-3, beta=0.4)):
        with pytest.raises(ValueError, match='errors=True needs a self-play engine built with prioritized='):
            PopulationTrainer.train_epoch_ring(dev_trainer, types.SimpleNamespace(prioritized=prioritized), None, errors=True)


sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_the_examples_refuse_what_they_cannot_do():
    import importlib
    common = ["--game", "CartPole-v0", "--replay-steps", "4", "--steps-per-iter", "2", "--n-step", "3", "--device", "cuda"]
    one = importlib.import_module("selfplay_train")
    a = one.parse_args(common + ["--prioritized-alpha", "0.6", "--prioritized-feedback", "max"])
    assert a.prioritized_feedback == "max" and one.parse_args(common).prioritized_feedback is None
    with pytest.raises(SystemExit):
        one.parse_args(common + ["--prioritized-feedback", "max"])                # no --prioritized-alpha
    with pytest.raises(SystemExit):
        one.parse_args(common + ["--prioritized-alpha", "0.6", "--prioritized-feedback", "mean"])
    pop = importlib.import_module("population_selfplay_train")
    common += ["--seeds", "0", "1", "--games-per-seed", "8"]
    a = pop.parse_args(common + ["--trainer", "device-epoch", "--prioritized-alpha", "0.6", "--prioritized-feedback", "value_gap"])
    assert pop.prioritized(a) == {"alpha": 0.6, "eps": 1e-3, "feedback": "value_gap"}
    assert "feedback" not in pop.prioritized(pop.parse_args(common + ["--trainer", "device-epoch", "--prioritized-alpha", "0.6"]))
    for trainer in ("torch", "device", "device-fused"):
        with pytest.raises(SystemExit):
            pop.parse_args(common + ["--trainer", trainer, "--prioritized-alpha", "0.6", "--prioritized-feedback", "max"])
    with pytest.raises(SystemExit):
        pop.parse_args(common + ["--trainer", "device-epoch", "--prioritized-feedback", "max"])
