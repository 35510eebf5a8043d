"""What the device replay ring's entry points refuse, by code AND message (azg_selfplay_*, include/azgym.h, azgym_reanalyse.h,
azgym_nstep.h, azgym_priority.h): one engine walked through the ring's states -- no begin, nothing kept, a non-empty ring, stale
priorities, an empty ring, a full STOP ring, a second begin.  The other ring tests check these refusals by code only; the texts here
are the ABI's, byte for byte.  One search in all: CartPole, 8 games as 2 nets of 4, 6 simulations, a STOP ring of one step."""
import pytest

import reanalyse_util as R
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

STATE, INVALID = _capi.AZG_E_STATE, _capi.AZG_E_INVALID
BEGIN = "azg_selfplay_begin has not been called"
KEEP_STATES = "azg_selfplay_keep_states has not been called"
KEEP_TRANSITIONS = "azg_selfplay_keep_transitions has not been called"
KEEP_PRIORITIES = "azg_selfplay_keep_priorities has not been called"
NOT_EMPTY = ": the replay ring is not empty (call it right after begin, or after clearing the rows)"
STALE = ": azg_selfplay_priorities has not run since the ring's stored rows last changed (a step, a clear or a begin)"
EMPTY = ": the replay ring is empty"
WEIGHTS_STALE = ("azg_selfplay_is_weights_device: azg_selfplay_is_weights has not run since the ring's stored rows or their priorities "
                 "last changed")
DRAWS = ("azg_selfplay_sample_rows", "azg_selfplay_sample_slots", "azg_selfplay_is_weights")


def _case():
    base = R.CASES["cartpole"]
    return R.Case(dict(base.kw, n_sims=6), base.net, games=8, max_len=3, nets=2)


def _engine(case):
    from alphazero_gym_amd import _native
    _native.lib()
    return R.make_engine(_native.HipEngine, case)


def _refuses(code, text, fn, *args):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*args)
    assert (ei.value.code, str(ei.value)) == (code, f"azgym error {code}: {text}")


def _draws(e):
    """The two draws and the weights, in DRAWS' order."""
    return ((e.selfplay_sample_rows, (4, 0)), (e.selfplay_sample_slots, (0,)), (e.selfplay_is_weights, (0.4,)))


def _assert_draws_refuse(e, tail):
    for who, (fn, args) in zip(DRAWS, _draws(e)):
        _refuses(STATE, who + tail, fn, *args)


def _assert_nothing_kept(e):
    """After a begin: every entry point that needs a kept column names the keep_* call that is missing."""
    _refuses(STATE, KEEP_STATES, e.selfplay_states)
    _refuses(STATE, KEEP_STATES + ": the stored positions' env states were not kept", e.selfplay_reanalyse, 0)
    _refuses(STATE, KEEP_TRANSITIONS, e.selfplay_transitions)
    _refuses(STATE, KEEP_TRANSITIONS + ": the stored steps' rewards and ends were not kept", e.selfplay_nstep_targets, 3)
    for fn, args in ((e.selfplay_priorities, (0.6, 1e-3)), (e.selfplay_priority_values, ())) + _draws(e) + \
            ((e.selfplay_is_weights, (-1.0,)), (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        _refuses(STATE, KEEP_PRIORITIES, fn, *args)


def test_every_ring_state_refuses_with_its_code_and_message():
    case = _case()
    e = _engine(case)
    # before any begin (selfplay_rows / selfplay_states: the test below)
    for fn, args in ((e.selfplay_step, ()), (e.selfplay_clear, ()), (e.selfplay_ring, ()), (e.selfplay_rows_device, ()),
                     (e.selfplay_stats, ()), (e.selfplay_keep_states, (True,)), (e.selfplay_keep_states, (False,)),
                     (e.selfplay_reanalyse, (0,)), (e.selfplay_keep_transitions, (True,)), (e.selfplay_transitions, ()),
                     (e.selfplay_nstep_targets, (3,)), (e.selfplay_keep_priorities, (True,)), (e.selfplay_keep_priorities, (False,)),
                     (e.selfplay_priorities, (0.6, 1e-3)), (e.selfplay_priority_values, ())) + _draws(e) + \
            ((e.selfplay_is_weights, (-1.0,)),   # (the state comes before the argument)
             (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        _refuses(STATE, BEGIN, fn, *args)

    # after a begin with nothing kept
    R.begin(e, case, 1, keep=False)
    _assert_nothing_kept(e)

    # priorities kept, never computed, on an empty ring; the value gap without kept transitions
    e.selfplay_keep_priorities(True)
    _assert_draws_refuse(e, STALE)
    _refuses(STATE, "azg_selfplay_priorities: AZG_PRIO_VALUE_GAP needs azg_selfplay_keep_transitions: the stored steps' search values "
             "were not kept", e.selfplay_priorities, 0.6, 1e-3)
    _refuses(STATE, WEIGHTS_STALE, e.selfplay_is_weights_device)
    _refuses(STATE, "azg_selfplay_is_weight_values: azg_selfplay_is_weights has not been called", e.selfplay_is_weight_values)
    e.selfplay_keep_transitions(True)
    e.selfplay_keep_states(True)
    e.selfplay_priorities(0.6, 1e-3)   # (no rows: the priorities stand for the empty ring)
    _assert_draws_refuse(e, EMPTY)
    _refuses(INVALID, "azg_selfplay_reanalyse: slot 0 is not a stored step (size_steps 0)", e.selfplay_reanalyse, 0)

    # one step: the ring is not empty, the STOP ring of one step is full, the priorities are stale
    e.selfplay_step()
    assert e.selfplay_ring() == (1, 0, 1)
    _refuses(STATE, "azg_selfplay_keep_states" + NOT_EMPTY, e.selfplay_keep_states, True)
    _refuses(STATE, "azg_selfplay_keep_states" + NOT_EMPTY, e.selfplay_keep_states, False)
    _refuses(STATE, "azg_selfplay_keep_transitions" + NOT_EMPTY, e.selfplay_keep_transitions, True)
    _refuses(STATE, "azg_selfplay_keep_transitions" + NOT_EMPTY, e.selfplay_keep_transitions, False)
    _refuses(STATE, "replay ring is full: download and clear the rows", e.selfplay_step)
    _assert_draws_refuse(e, STALE)
    _refuses(INVALID, "azg_selfplay_reanalyse: slot 1 is not a stored step (size_steps 1)", e.selfplay_reanalyse, 1)
    _refuses(INVALID, "azg_selfplay_reanalyse: slot -1 is not a stored step (size_steps 1)", e.selfplay_reanalyse, [0] * 7 + [-1])

    # priorities and weights of the stored step, then a clear: both are stale again
    e.selfplay_priorities(0.6, 1e-3)
    e.selfplay_is_weights(0.4)
    assert e.selfplay_is_weights_device() != 0
    _refuses(INVALID, "azg_selfplay_is_weights: beta must be finite and >= 0", e.selfplay_is_weights, -1.0)
    e.selfplay_clear()
    assert e.selfplay_ring() == (0, 0, 1)
    _assert_draws_refuse(e, STALE)
    _refuses(STATE, WEIGHTS_STALE, e.selfplay_is_weights_device)

    # a second begin: every kept column is gone, as on a fresh engine
    R.begin(e, case, 1, keep=False)
    _assert_nothing_kept(e)
    e.selfplay_keep_states(True)       # (and can be asked for again)
    e.selfplay_keep_transitions(True)
    e.selfplay_keep_priorities(True)
    assert len(e.selfplay_states()) == 0 and len(e.selfplay_priority_values()) == 0
    _assert_draws_refuse(e, STALE)
    e.close()


def test_downloads_before_a_begin_are_state_errors():
    """selfplay_rows / selfplay_states on a fresh engine: the engine's refusal, not an AttributeError of the binding."""
    e = _engine(_case())
    _refuses(STATE, BEGIN, e.selfplay_rows)
    _refuses(STATE, BEGIN, e.selfplay_rows, False)
    _refuses(STATE, BEGIN, e.selfplay_states)
    e.close()
