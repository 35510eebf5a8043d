"""The CPU truth of the lambda-return targets (tests/lambda_util.py) on the CPU: the fold against the explicit mixture of m-step returns
where both are exact, its three edge identities against nstep_util.nstep_returns on the restatement's self-play, and what
tests/test_lambda_targets.py needs of its own inputs."""
import ctypes as C

import numpy as np
import pytest

import lambda_util as LU
import nstep_util as N
from alphazero_gym_amd import _capi

R5 = np.array([1.0, 2.0, 4.0, 8.0, 16.0])[:, None]
V5 = np.array([10.0, 20.0, 30.0, 40.0, 50.0])[:, None]


def _ends(**at):
    e = np.zeros((5, 1), np.int32)
    for k, v in at.items():
        e[int(k[1:]), 0] = v
    return e


# gamma 1, lambda 0.5: every product and sum is exact.  (ends, n_step, the window kind of row 0, row 0's target by hand)
#   G1 = r0 + v1 = 21, G2 = r0 + r1 + v2 = 33, G3 = 1 + 2 + 4 + v3 = 47, G4 = 1 + 2 + 4 + 8 + v4 = 65
HAND = [
    (_ends(), 3, "full", 0.5 * 21 + 0.25 * 33 + 0.25 * 47),
    (_ends(), 1000, "cut_by_newest", 0.5 * 21 + 0.25 * 33 + 0.125 * 47 + 0.125 * 65),
    (_ends(), 1, "full", 21.0),
    (_ends(), 0, None, 10.0),
    # the env ends the episode at step 2: G3 is the three rewards and nothing else
    (_ends(s2=N.END_TERMINAL), 3, "terminal_inside", 0.5 * 21 + 0.25 * 33 + 0.25 * 7),
    (_ends(s2=N.END_TERMINAL), 1000, "terminal_inside", 0.5 * 21 + 0.25 * 33 + 0.25 * 7),
    (_ends(s2=N.END_TERMINAL), 2, "full", 0.5 * 21 + 0.5 * 33),
    # the length limit ends it at step 2: the window stops at step 2's own root, so G2 is the longest return
    (_ends(s2=N.END_LENGTH), 3, "length_inside", 0.5 * 21 + 0.5 * 33),
    (_ends(s2=N.END_LENGTH), 1000, "length_inside", 0.5 * 21 + 0.5 * 33),
    # an end at the row's own step
    (_ends(s0=N.END_TERMINAL), 3, "terminal_inside", 1.0),
    (_ends(s0=N.END_LENGTH), 3, "length_inside", 10.0),
]


@pytest.mark.parametrize("i", range(len(HAND)))
def test_hand_written_sequences(i):
    end, n, kind, want = HAND[i]
    got = LU.lambda_returns(R5, V5, end, n, 0.5, 1.0)
    assert N.bits64(got[0, 0]) == N.bits64(np.float64(want)), (got[0, 0], want)
    if kind is not None:   # (row 0's window is of the kind the case is there for: nstep_util.window_kinds' rule at s = 0)
        hit = [i for i in range(min(n, 5)) if end[i, 0] != N.END_NONE]
        mine = ("terminal_inside" if end[hit[0], 0] == N.END_TERMINAL else "length_inside") if hit else "cut_by_newest" if n > 4 else "full"
        assert mine == kind and N.window_kinds(end, n)[kind] >= 1
    np.testing.assert_array_equal(N.bits64(got), N.bits64(LU.mixture_returns(R5, V5, end, n, 0.5, 1.0)))
    # the newest step's row is its own value, or its reward alone where the env ended the episode there
    assert got[4, 0] == (16.0 if end[4, 0] == N.END_TERMINAL else 50.0)


@pytest.mark.parametrize("n_step", [0, 1, 2, 3, 5, 1000])
def test_fold_equals_the_explicit_mixture_where_both_are_exact(n_step):
    """gamma = 1, lambda = 0.5, unit rewards, small integer values: every product is a multiple of 2^-39 below 2^7 and every sum is
    exact, whatever its order.  The input holds windows closed by a terminal end, stopped at a length end, cut by the newest step and
    of full length."""
    rng = np.random.default_rng(5)
    S, G = 40, 30
    end = rng.choice([N.END_NONE] * 8 + [N.END_TERMINAL, N.END_LENGTH], size=(S, G)).astype(np.int32)
    end[:, 0] = N.END_NONE   # (one game that never ends: at n_step 1000 its windows are as long as the range)
    reward = np.ones((S, G))
    value = rng.integers(-20, 20, size=(S, G)).astype(np.float64)
    a, b = LU.lambda_returns(reward, value, end, n_step, 0.5, 1.0), LU.mixture_returns(reward, value, end, n_step, 0.5, 1.0)
    np.testing.assert_array_equal(N.bits64(a), N.bits64(b))
    if n_step >= 1:
        kinds = N.window_kinds(end, n_step)
        assert kinds["terminal_inside"] and kinds["length_inside"] and kinds["cut_by_newest"] and (kinds["full"] or n_step == 1000), kinds
    if n_step == 3:   # (... and the mixture is neither of its ends)
        assert (a != N.nstep_returns(reward, value, end, 3, 1.0)).any() and (a != N.nstep_returns(reward, value, end, 1, 1.0)).any()


def test_fold_is_close_to_the_explicit_mixture_elsewhere():
    rng = np.random.default_rng(6)
    S, G = 30, 20
    end = rng.choice([0, 0, 0, 0, 0, 1, 2], size=(S, G)).astype(np.int32)
    reward, value = rng.normal(size=(S, G)), rng.normal(size=(S, G))
    for n in (1, 3, 7, 1000):
        for lam in (0.0, 0.3, 0.95, 1.0):
            np.testing.assert_allclose(LU.lambda_returns(reward, value, end, n, lam, 0.97), LU.mixture_returns(reward, value, end, n, lam, 0.97),
                                       rtol=0, atol=1e-12)


def test_games_take_their_own_rule():
    end = np.concatenate([_ends(s2=N.END_TERMINAL), _ends(), _ends(s2=N.END_LENGTH)], 1)
    r, v = np.repeat(R5, 3, 1), np.repeat(V5, 3, 1)
    rules = [(0, 0.5, 0.5), (3, 0.9, 1.0), (1000, 0.3, 0.25)]
    got = LU.lambda_returns(r, v, end, [n for n, _, _ in rules], [lm for _, lm, _ in rules], [g for _, _, g in rules])
    for g, (n, lam, gamma) in enumerate(rules):
        np.testing.assert_array_equal(N.bits64(got[:, g]), N.bits64(LU.lambda_returns(R5, V5, end[:, g:g + 1], n, lam, gamma)[:, 0]))


@pytest.mark.parametrize("name", sorted(N.CASES))
@pytest.mark.parametrize("n", [1, 3, 1000])
def test_edge_identities_on_the_restatements_self_play(name, n):
    """lambda 1 is the n-step return, lambda 0 the 1-step return, and n_step 1 is the same for every lambda: bit for bit in float64,
    with the search's gamma (per net in the population) and with 0.9.  (No accumulator of these inputs is a signed zero.)"""
    ref = N.reference(name)
    case = N.CASES[name]
    for gamma in (N.search_gamma(case), 0.9):
        nstep = N.nstep_returns(ref["reward"], ref["value"], ref["end"], n, gamma)
        one = N.nstep_returns(ref["reward"], ref["value"], ref["end"], 1, gamma)
        np.testing.assert_array_equal(N.bits64(LU.lambda_returns(ref["reward"], ref["value"], ref["end"], n, 1.0, gamma)), N.bits64(nstep))
        np.testing.assert_array_equal(N.bits64(LU.lambda_returns(ref["reward"], ref["value"], ref["end"], n, 0.0, gamma)), N.bits64(one))
        for lam in (0.3, 0.9):
            np.testing.assert_array_equal(N.bits64(LU.lambda_returns(ref["reward"], ref["value"], ref["end"], 1, lam, gamma)), N.bits64(one))
    np.testing.assert_array_equal(N.bits64(LU.lambda_returns(ref["reward"], ref["value"], ref["end"], 0, 0.5, 0.9)), N.bits64(ref["value"]))


@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_share_condition_holds_for_the_truth(name, capacity, fifo):
    """At lambda 0.5 and n_step 3 (and 1000) at least 0.4 of the rows of every ring of tests/test_lambda_targets.py differ in bits from
    both the n-step and the 1-step column: a call that wrote either could not pass for the lambda call."""
    ref = N.reference(name)
    held, _ = N.ring_layout(capacity, fifo, N.STEPS[name])
    for n in (3, 1000):
        share = LU.share_apart(ref["reward"], ref["value"], ref["end"], held, n, 0.5, N.search_gamma(N.CASES[name]))
        print(f"{name} capacity {capacity} n_step {n}: share {share:.3f}")
        assert share >= LU.MIN_SHARE, (name, n, share)


def test_rule_struct_matches_the_header():
    assert C.sizeof(_capi.AzgReturnRule) == 32
    r = _capi.AzgReturnRule
    assert (r.struct_size.offset, r.n_step.offset, r.lambda_.offset, r.gamma.offset, r.flags.offset) == (0, 4, 8, 16, 24)
    assert "selfplay_lambda_targets" in _capi.OPTIONAL_SYMBOLS and "selfplay_lambda_targets_nets" in _capi.OPTIONAL_SYMBOLS
