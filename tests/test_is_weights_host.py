"""Importance-sampling weights for prioritised replay on the CPU: the numpy truth of the weight rule (tests/is_weights_util.py) on
hand-written priorities, population_loss(weights=) -- ones against None bit for bit, a weighted call against the formula written out
by hand, zero-weight rows -- the Python refusals that need no GPU, and the ABI of the built library (include/azgym_priority.h,
include/azgym_train_weighted.h)."""
import types

import numpy as np
import pytest
import torch

import is_weights_util as W
import oracle_lib as O
import priority_util as P
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, population_terms
from device_loss_util import HEADS, LOG_ALPHA0, make_head, make_inputs, make_loss, torch_loss

CASES = [(h, "alphazero") for h in ("discrete2", "discrete3")] + [(h, l) for h in HEADS for l in ("a0c", "a0c_tuned")]


# ------------------------------------------------------------------------------------------------ the rule

def test_equal_priorities_weigh_one():
    for q0 in (1, P.Q_ONE, P.Q_MAX):
        q = np.full((3, 4), q0, np.uint64)
        for beta in (0.0, 0.4, 1.0, 50.0):
            np.testing.assert_array_equal(W.bits(W.is_weights(q, 2, beta)), W.bits(np.ones((3, 4), np.float32)))


def test_one_and_two_to_the_forty():
    """q = {1, 2^40}: r = 2^-40 exactly, and w is what the oracle's functions give, step by step."""
    q = np.asarray([[1, P.Q_MAX]], np.uint64)
    for beta in (0.4, 1.0, 3.0):
        w = W.is_weights(q, 1, beta)
        r = np.float32(1.0 / float(P.Q_MAX))
        assert r == np.float32(2.0 ** -40)
        m = np.float32(np.float32(beta) * np.float32(O.math_eval(3, [r])[0]))
        want = np.float32(O.math_eval(0, [m])[0])
        assert w[0, 0] == np.float32(1.0) and W.bits(w[0, 1:]) == W.bits(np.asarray([want]))
        assert 0.0 <= float(want) < 1.0
        assert abs(float(want) - 2.0 ** (-40.0 * beta)) <= 1e-5 * 2.0 ** (-40.0 * beta)
    # a large beta underflows: whatever azg_expf returns, and it stays in [0, 1]
    w = W.is_weights(q, 1, 1000.0)
    assert float(w[0, 1]) == float(np.float32(O.math_eval(0, [np.float32(np.float32(1000.0) * np.float32(O.math_eval(3, [2.0 ** -40])[0]))])[0]))
    assert 0.0 <= float(w[0, 1]) <= 1.0


def test_beta_zero_is_one_everywhere():
    rng = np.random.default_rng(5)
    q = rng.integers(1, P.Q_MAX, size=(6, 9), endpoint=True).astype(np.uint64)
    np.testing.assert_array_equal(W.bits(W.is_weights(q, 3, 0.0)), W.bits(np.ones(q.shape, np.float32)))


def test_the_minimum_row_weighs_exactly_one_and_minima_are_per_net():
    rng = np.random.default_rng(6)
    q = rng.integers(1 << 10, 1 << 30, size=(5, 6)).astype(np.uint64)
    q[2, 1] = 7          # net 0's minimum
    q[4, 5] = 900        # net 1's
    for beta in (0.4, 1.0, 7.5):
        w = W.is_weights(q, 2, beta)
        assert W.bits(w[2, 1]) == W.bits(np.float32(1.0)) and W.bits(w[4, 5]) == W.bits(np.float32(1.0))
        assert (w >= 0).all() and (w <= 1).all() and (w < 1).sum() == q.size - 2
        # net 1's weights are those of its columns alone: the other net's smaller minimum does not reach them
        np.testing.assert_array_equal(W.bits(w[:, 3:]), W.bits(W.is_weights(q[:, 3:], 1, beta)))
        # the ratio is rounded to float32 before the logarithm
        r = np.float32(900.0 / float(q[0, 3]))
        want = np.float32(O.math_eval(0, [np.float32(np.float32(beta) * np.float32(O.math_eval(3, [r])[0]))])[0])
        assert W.bits(w[0, 3]) == W.bits(want)
    # monotone: a larger priority weighs no more
    col = np.sort(q[:, :3].reshape(-1))
    ws = W.weight_rule(col, col[0], 0.4)
    assert (np.diff(ws.astype(np.float64)) <= 0).all() and ws[0] == 1.0


def test_both_clamps_in_one_net_from_given_values():
    """d = 0 and d = 1e9 at alpha = 1 with a tiny eps: q = 1 and q = 2^40 -- the pair the GPU test relies on."""
    q = P.priorities(np.asarray([0.0, 1e9, 1.0], np.float32), 1.0, 1e-9)
    assert [int(v) for v in q[:2]] == [1, P.Q_MAX] and 1 < int(q[2]) < P.Q_MAX


# ------------------------------------------------------------------------------------------------ population_loss(weights=)

def _log_alpha(loss_name, K, dtype):
    return torch.tensor(LOG_ALPHA0[:K], dtype=dtype, requires_grad=True) if loss_name == "a0c_tuned" else None


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head,loss_name", CASES, ids=lambda v: str(v))
def test_ones_are_none_bit_for_bit(head, loss_name, reduction):
    K, B = 3, 7
    policy, loss = make_head(head), make_loss(loss_name, reduction)
    inputs = make_inputs(head, K, B, 77)
    for dtype in (torch.float32, torch.float64):
        plain, g_plain = torch_loss(policy, loss, inputs, dtype, _log_alpha(loss_name, K, dtype))
        ones, g_ones = W.torch_loss_weighted(policy, loss, inputs, torch.ones((K, B)), dtype, _log_alpha(loss_name, K, dtype))
        assert set(plain) == set(ones)
        for key in plain:
            assert torch.equal(plain[key], ones[key]), (key, dtype)
        assert torch.equal(g_plain, g_ones), dtype


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head,loss_name", [("discrete3", "alphazero"), ("discrete3", "a0c_tuned"), ("normal", "a0c"), ("gmm2", "a0c_tuned")],
                         ids=lambda v: str(v))
def test_a_weighted_call_is_the_formula_by_hand(head, loss_name, reduction):
    """Three rows, float64: every loss is coeff * reduce_b(w_b * term_b) over the unweighted per-row terms, written out as Python sums;
    alpha_loss is mean_b(alpha * w_b * (H_b - target)); the gradient of row b is w_b times the unweighted call's."""
    K, B = 2, 3
    policy, loss = make_head(head), make_loss(loss_name, reduction)
    inputs = make_inputs(head, K, B, 78)
    w = torch.tensor([[0.25, 0.0, 1.0], [0.7, 0.5, 0.125]], dtype=torch.float64)
    la = _log_alpha(loss_name, K, torch.float64)
    got, g = W.torch_loss_weighted(policy, loss, inputs, w, torch.float64, la)
    _, g_plain = torch_loss(policy, loss, inputs, torch.float64, _log_alpha(loss_name, K, torch.float64))
    raw, actions, counts, values = (x.double() for x in inputs)
    with torch.no_grad():
        terms = population_terms(policy, loss, raw, actions, counts, values.unsqueeze(-1))
    div = float(B) if reduction == "mean" else 1.0
    for k in range(K):
        pol = sum(float(w[k, b]) * float(terms["policy"][k, b]) for b in range(B)) / div
        val = sum(float(w[k, b]) * float(terms["value"][k, b, 0]) for b in range(B)) / div
        assert float(got["policy_loss"][k]) == pytest.approx(loss.policy_coeff * pol, rel=1e-13, abs=1e-15)
        assert float(got["value_loss"][k]) == pytest.approx(loss.value_coeff * val, rel=1e-13, abs=1e-15)
        total = loss.policy_coeff * pol + loss.value_coeff * val
        if loss_name != "alphazero":
            ent = terms["entropy"][k]
            per_row = ent.reshape(B, -1)
            n_el = per_row.shape[1]
            e_sum = sum(float(w[k, b]) * float(per_row[b, j]) for b in range(B) for j in range(n_el))
            e_red = e_sum / (B * n_el) if reduction == "mean" else e_sum
            alpha = float(torch.tensor(LOG_ALPHA0[k], dtype=torch.float64).exp()) if loss_name == "a0c_tuned" else float(loss.alpha)
            assert float(got["entropy_loss"][k]) == pytest.approx(alpha * e_red, rel=1e-13, abs=1e-15)
            total += alpha * e_red
            if loss_name == "a0c_tuned":
                a_loss = sum(alpha * float(w[k, b]) * (float(per_row[b, j]) - loss.target_entropy) for b in range(B) for j in range(n_el)) / (B * n_el)
                assert float(got["alpha_loss"][k]) == pytest.approx(a_loss, rel=1e-13, abs=1e-15)
        assert float(got["loss"][k]) == pytest.approx(total, rel=1e-13, abs=1e-15)
    torch.testing.assert_close(g, g_plain * w.unsqueeze(-1), rtol=1e-12, atol=1e-300)
    assert bool((g[0, 1] == 0).all()) and bool((g[0, 0] != 0).any())


@pytest.mark.parametrize("head,loss_name", CASES, ids=lambda v: str(v))
def test_zero_weight_rows_have_zero_gradient_rows(head, loss_name):
    K, B = 3, 9
    policy, loss = make_head(head), make_loss(loss_name, "mean")
    inputs = make_inputs(head, K, B, 79)
    w = W.make_weights(K, B, 3)
    zero = w == 0
    assert zero.any() and (w == 1).any() and ((w > 0) & (w < 1)).any()
    for dtype in (torch.float32, torch.float64):
        _, g = W.torch_loss_weighted(policy, loss, inputs, w, dtype, _log_alpha(loss_name, K, dtype))
        assert bool((g[zero] == 0).all()) and bool((g[~zero] != 0).any())
    with pytest.raises(ValueError, match=r"\[K, B\]"):
        W.torch_loss_weighted(policy, loss, inputs, w[:, :-1], torch.float32, _log_alpha(loss_name, K, torch.float32))


# ------------------------------------------------------------------------------------------------ refusals without a GPU

def test_python_refusals():
    kw = dict(game="CartPole-v0", games_per_net=4, n_rollouts=8, c_uct=1.5, n_step=3)
    with pytest.raises(ValueError, match="beta only beside alpha"):
        run.PopulationSelfPlay([object()], prioritized={"beta": 0.4}, **kw)
    with pytest.raises(ValueError, match="beta only beside alpha"):
        run.PopulationSelfPlay([object()], prioritized={"beta": 0.4, "eps": 1e-3}, **kw)
    for beta in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta must be finite and >= 0"):
            run.PopulationSelfPlay([object()], prioritized={"alpha": 0.6, "beta": beta}, **kw)
    with pytest.raises(ValueError, match="alpha, eps and beta"):
        run.PopulationSelfPlay([object()], prioritized={"alpha": 0.6, "gamma": 1.0}, **kw)
    # is_weights: off, no beta anywhere, a negative one -- all before the engine is touched
    fake = types.SimpleNamespace(prioritized=None, engine=None)
    with pytest.raises(RuntimeError, match="prioritized"):
        run.PopulationSelfPlay.is_weights(fake)
    fake.prioritized = dict(alpha=0.6, eps=1e-3)
    with pytest.raises(ValueError, match="needs a beta"):
        run.PopulationSelfPlay.is_weights(fake)
    with pytest.raises(ValueError, match="finite and >= 0"):
        run.PopulationSelfPlay.is_weights(fake, -0.5)
    # the trainer: weighted epochs need the device losses; weights="priority" needs a prioritised engine
    torch_trainer = types.SimpleNamespace(losses="torch")
    for call in (lambda: PopulationTrainer.train_epoch(torch_trainer, None, 4, 2, weights=torch.ones((1, 4))),
                 lambda: PopulationTrainer.train_epoch_ring(torch_trainer, None, None, weights="priority")):
        with pytest.raises(ValueError, match='needs a trainer built with losses="device"'):
            call()
    dev_trainer = types.SimpleNamespace(losses="device")
    with pytest.raises(ValueError, match="prioritized="):
        PopulationTrainer.train_epoch_ring(dev_trainer, types.SimpleNamespace(prioritized=None), None, weights="priority")
    with pytest.raises(ValueError, match='"priority", a tensor or None'):
        PopulationTrainer.train_epoch_ring(dev_trainer, types.SimpleNamespace(prioritized={}), None, weights="uniform")


def test_the_built_library_has_the_entry_points():
    from alphazero_gym_amd import _native
    lib = _native.lib()
    for name in ("selfplay_is_weights", "selfplay_is_weights_device", "selfplay_is_weight_values", "trainer_loss_weighted",
                 "trainer_loss_nets_weighted", "trainer_step_opt_weighted", "trainer_step_nets_weighted", "trainer_epoch_opt_weighted",
                 "trainer_epoch_nets_weighted"):
        assert hasattr(lib, "azg_" + name), name
        assert name in _capi.OPTIONAL_SYMBOLS
    for method in ("loss_weighted", "loss_nets_weighted", "step_opt_weighted", "step_nets_weighted", "epoch_opt_weighted",
                   "epoch_nets_weighted"):
        assert callable(getattr(_capi.Trainer, method))
    with pytest.raises(NotImplementedError, match="azg_trainer_loss_weighted"):
        _capi._require({}, "trainer_loss_weighted")
