"""The CPU truth of the n-step return targets (tests/nstep_util.py) on the CPU: the builder on hand-written sequences -- each end kind, a
window cut by the newest step, a wrapped ring --, against the explicit sum where the two are exactly equal, and on the restatement's
self-play, whose rows n_step = 0 reproduces."""
import ctypes as C

import numpy as np
import pytest

import nstep_util as N
from alphazero_gym_amd import _capi

R5 = np.array([1.0, 2.0, 4.0, 8.0, 16.0])[:, None]
V5 = np.array([10.0, 20.0, 30.0, 40.0, 50.0])[:, None]


def _ends(**at):
    e = np.zeros((5, 1), np.int32)
    for k, v in at.items():
        e[int(k[1:]), 0] = v
    return e


# gamma 0.5: every product and sum below is exact, worked out by hand
HAND = [
    # no end: s + 2 steps on, cut by the newest step (3 -> value of 4; 4 -> its own value)
    (_ends(), 2, [1 + 1 + 7.5, 2 + 2 + 10, 4 + 4 + 12.5, 8 + 25, 50]),
    (_ends(), 0, [10, 20, 30, 40, 50]),
    (_ends(), 1, [1 + 10, 2 + 15, 4 + 20, 8 + 25, 50]),
    (_ends(), 1000, [1 + 1 + 1 + 1 + 50 / 16, 2 + 2 + 2 + 50 / 8, 4 + 4 + 12.5, 8 + 25, 50]),
    # the env ends the episode at step 2: inside the window no bootstrap; at s + n_step it is an ordinary bootstrap
    (_ends(s2=N.END_TERMINAL), 2, [1 + 1 + 7.5, 2 + 2, 4, 8 + 25, 50]),
    (_ends(s2=N.END_TERMINAL), 1000, [1 + 1 + 1, 2 + 2, 4, 8 + 25, 50]),
    (_ends(s2=N.END_TERMINAL), 0, [10, 20, 30, 40, 50]),
    # the length limit ends it at step 2: the window stops at step 2's own root
    (_ends(s2=N.END_LENGTH), 2, [1 + 1 + 7.5, 2 + 15, 30, 8 + 25, 50]),
    (_ends(s2=N.END_LENGTH), 1000, [1 + 1 + 7.5, 2 + 15, 30, 8 + 25, 50]),
    (_ends(s2=N.END_LENGTH), 1, [1 + 10, 2 + 15, 30, 8 + 25, 50]),
    # ends at the newest step: a terminal one pays its reward and nothing else, a time limit is the newest step's cut
    (_ends(s4=N.END_TERMINAL), 2, [1 + 1 + 7.5, 2 + 2 + 10, 4 + 4 + 12.5, 8 + 8, 16]),
    (_ends(s4=N.END_LENGTH), 2, [1 + 1 + 7.5, 2 + 2 + 10, 4 + 4 + 12.5, 8 + 25, 50]),
    # two ends: the first one counts
    (_ends(s1=N.END_LENGTH, s3=N.END_TERMINAL), 1000, [1 + 10, 20, 4 + 4, 8, 50]),
]


@pytest.mark.parametrize("i", range(len(HAND)))
def test_hand_written_sequences(i):
    end, n, want = HAND[i]
    got = N.nstep_returns(R5, V5, end, n, 0.5)
    np.testing.assert_array_equal(N.bits64(got[:, 0]), N.bits64(np.asarray(want, np.float64)))


def test_games_are_independent_and_take_their_own_gamma():
    end = np.concatenate([_ends(s2=N.END_TERMINAL), _ends(), _ends(s2=N.END_LENGTH)], 1)
    r, v = np.repeat(R5, 3, 1), np.repeat(V5, 3, 1)
    got = N.nstep_returns(r, v, end, 2, [0.5, 1.0, 0.25])
    for g, gamma in enumerate((0.5, 1.0, 0.25)):
        np.testing.assert_array_equal(N.bits64(got[:, g]), N.bits64(N.nstep_returns(R5, V5, end[:, g:g + 1], 2, gamma)[:, 0]))
    assert got[0, 1] == 1 + 2 + 30


def test_ring_layout_and_wrap_around():
    held, oldest = N.ring_layout(3, True, 5)
    assert held.tolist() == [3, 4, 2] and oldest == 2
    held2, oldest2 = N.ring_layout(8, False, 5)
    assert held2.tolist() == [0, 1, 2, 3, 4] and oldest2 == 0
    # the wrapped ring holds steps 2, 3, 4: windows start at step 2 and see nothing older; slot j holds step held[j]
    col = N.ring_targets(np.repeat(R5, 2, 1), np.repeat(V5, 2, 1), np.repeat(_ends(s1=N.END_TERMINAL), 2, 1), held, 2, 0.5)
    np.testing.assert_array_equal(col, np.asarray([[33, 33], [50, 50], [20.5, 20.5]], np.float32))
    # an end at the oldest stored step belongs to it; the step before is not in the ring
    col = N.ring_targets(R5, V5, _ends(s2=N.END_TERMINAL), held, 2, 0.5)
    np.testing.assert_array_equal(col[:, 0], np.asarray([33, 50, 4], np.float32))


@pytest.mark.parametrize("n_step", [0, 1, 2, 3, 5, 1000])
def test_recurrence_equals_the_explicit_sum_where_both_are_exact(n_step):
    """gamma = 1, CartPole's unit rewards, small integer values: every sum is exact, whatever its order."""
    rng = np.random.default_rng(5)
    S, G = 40, 30
    end = rng.choice([N.END_NONE, N.END_NONE, N.END_NONE, N.END_NONE, N.END_TERMINAL, N.END_LENGTH], size=(S, G)).astype(np.int32)
    reward = np.ones((S, G))
    value = rng.integers(-20, 20, size=(S, G)).astype(np.float64)
    a, b = N.nstep_returns(reward, value, end, n_step, 1.0), N.direct_returns(reward, value, end, n_step, 1.0)
    np.testing.assert_array_equal(N.bits64(a), N.bits64(b))
    assert {N.END_NONE, N.END_TERMINAL, N.END_LENGTH} == set(np.unique(end))


def test_recurrence_is_close_to_the_explicit_sum_elsewhere():
    rng = np.random.default_rng(6)
    S, G = 30, 20
    end = rng.choice([0, 0, 0, 1, 2], size=(S, G)).astype(np.int32)
    reward, value = rng.normal(size=(S, G)), rng.normal(size=(S, G))
    for n in (1, 3, 7):
        np.testing.assert_allclose(N.nstep_returns(reward, value, end, n, 0.97), N.direct_returns(reward, value, end, n, 0.97), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_zero_steps_reproduce_the_restatements_rows(name):
    """n_step = 0 is (float)value: cpu_selfplay's own V_target column; the other transitions describe the same run."""
    case, steps = N.CASES[name], N.STEPS[name]
    ref = N.reference(name)
    col = N.nstep_returns(ref["reward"][:steps], ref["value"][:steps], ref["end"][:steps], 0, 0.9).astype(np.float32)
    np.testing.assert_array_equal(N.bits32(col), N.bits32(ref["rows"][:steps, :, -1]))
    held, _ = N.ring_layout(16, True, steps)
    col = N.ring_targets(ref["reward"], ref["value"], ref["end"], held, 0, 0.9)
    np.testing.assert_array_equal(N.bits32(col), N.bits32(ref["rows"][held, :, -1]))
    if case.cont:   # (time limits only; the rewards are in a tree node's units)
        assert set(np.unique(ref["end"])) == {N.END_NONE, N.END_LENGTH}
        assert np.all(ref["reward"] <= 0.0) and np.all(ref["reward"] >= -16.2736044 / _capi.PENDULUM_R_SCALE - 1e-9)
    else:
        np.testing.assert_array_equal(ref["reward"], 1.0)
        np.testing.assert_array_equal(ref["action"], np.round(ref["action"]))


def test_the_cartpole_input_holds_every_window_kind():
    """What tests/test_nstep_targets.py needs of its own input, over the 24 steps it plays."""
    steps = N.STEPS["cartpole"]
    end = N.reference("cartpole")["end"][:steps]
    assert ((end == N.END_TERMINAL).sum(), (end == N.END_LENGTH).sum()) == (15, 51)   # (terminal: 11 by the env alone, 4 with the limit on the same step)
    kinds = N.window_kinds(end, 3)
    assert kinds["terminal_inside"] and kinds["length_inside"] and kinds["cut_by_newest"] and kinds["full"], kinds


def test_config_struct_matches_the_header():
    assert C.sizeof(_capi.AzgNstepConfig) == 24
    assert (_capi.AzgNstepConfig.n_step.offset, _capi.AzgNstepConfig.gamma.offset, _capi.AzgNstepConfig.flags.offset) == (4, 8, 16)
    assert (_capi.END_NONE, _capi.END_TERMINAL, _capi.END_LENGTH, _capi.NSTEP_SEARCH_GAMMA) == (0, 1, 2, 1)
