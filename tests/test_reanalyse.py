"""Reanalysis of the device replay ring (azg_selfplay_keep_states / _states / _reanalyse, run.PopulationSelfPlay.reanalyse) on the GPU:
the state ring, idempotence under unchanged weights, new weights with mixed slots against the oracle, non-interference with the
games being played, the refusals and the Python layer.  Cases, sizes and the CPU truth: tests/reanalyse_util.py."""
import numpy as np
import pytest

import reanalyse_util as R
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

ALL = sorted(R.CASES)
STEPS_A, STEPS_C, STEPS_D = 5, 4, 6
RES_KEYS = ("counts", "n_children", "actions", "Q", "v_target")


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _engine(name, monkeypatch, capacity, steps, fifo=False, keep=True):
    case = R.CASES[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    e = R.make_engine(_hip(), case)
    R.begin(e, case, capacity, fifo=fifo, keep=keep)
    for _ in range(steps):
        e.selfplay_step()
    return case, e


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _mixed_slots(case, n):
    return np.arange(case.games, dtype=np.int32) % n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_state_ring_holds_the_roots_of_the_stored_steps(name, monkeypatch):
    """a.  STOP mode: after 5 steps the kept states are the roots the restatement's searches started from, bit for bit (and the rows
    its rows: keeping states does not move them).  FIFO mode, capacity 3: the ring has wrapped, slot s holds the state of the step its
    row holds."""
    ref = R.reference(name)
    case, e = _engine(name, monkeypatch, STEPS_A, STEPS_A)
    np.testing.assert_array_equal(R.bits64(e.selfplay_states()).reshape(STEPS_A, case.games, -1), R.bits64(ref["states"][:STEPS_A]))
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(ref["rows"][:STEPS_A]))
    e.close()
    case, e = _engine(name, monkeypatch, 3, STEPS_A, fifo=True)
    assert e.selfplay_ring() == (3, 2, STEPS_A)
    held = [3, 4, 2]   # the step each slot holds after 5 stores into 3 slots
    np.testing.assert_array_equal(R.bits64(e.selfplay_states()).reshape(3, case.games, -1), R.bits64(ref["states"][held]))
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(ref["rows"][held]))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_reanalysis_with_unchanged_weights_rewrites_the_same_rows(name, monkeypatch):
    """b.  No oracle: slot s reanalysed under search index s with the weights it was played with.  Continuous: the whole ring is
    unchanged, bit for bit.  Discrete: every row whose search carried no count is unchanged; the others (the self-play search reused a
    subtree, the reanalysis starts afresh) hold a whole search's visits."""
    ref = R.reference(name)
    case, e = _engine(name, monkeypatch, R.STEPS, R.STEPS)
    before, states = R.ring(e, case).copy(), e.selfplay_states().copy()
    for s in range(R.STEPS):
        e.selfplay_reanalyse(s, search_index=s)
    after = R.ring(e, case)
    fresh = ref["carry_in"][:R.STEPS] == 0
    assert fresh.all() == case.cont
    np.testing.assert_array_equal(R.bits32(after[fresh]), R.bits32(before[fresh]))
    K, So = e.kmax, e.s_obs
    np.testing.assert_array_equal(after[..., So + K:So + 2 * K].sum(-1), np.broadcast_to(case.budget().astype(np.float32), (R.STEPS, case.games)))
    np.testing.assert_array_equal(R.bits32(after[..., :So]), R.bits32(before[..., :So]))
    np.testing.assert_array_equal(R.bits64(e.selfplay_states()), R.bits64(states))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_reanalysis_with_new_weights_and_mixed_slots_matches_the_oracle(name, monkeypatch):
    """c.  4 steps, other weights, then ONE reanalysis in which game t takes slot t % 4 under search index 2^31: rows (slots[t], t)
    are the oracle's ordinary search of the kept state, every other row is untouched, and results() describes that search."""
    case, e = _engine(name, monkeypatch, STEPS_C, STEPS_C)
    before, states = R.ring(e, case).copy(), e.selfplay_states().reshape(STEPS_C, case.games, -1).copy()
    R.set_weights(e, case, new=True)
    slots = _mixed_slots(case, STEPS_C)
    e.selfplay_reanalyse(slots, search_index=R.NEW_INDEX)
    got_res = {k: np.array(v) for k, v in e.results().items()}
    info = e.search_info()   # (the reanalysis is the last search: the form the case is there for)
    if name.endswith("_team"):
        assert info["kernel_form"] in ("team", "per_layer"), info
    else:
        assert info["kernel_form"] == "persistent", info
    if name == "many_children":
        assert info["max_children"] == 20 and (info["tree_storage"], info["lds_exit"]) == ("global", "children"), info
    if name.endswith("_global_tree"):
        assert (info["tree_storage"], info["lds_exit"]) == ("global", "forced"), info
    after = R.ring(e, case)
    kws, blobs = ([case.net_kw(k) for k in range(case.nets)], case.blobs(new=True)) if case.nets > 1 else (case.net_kw(0), case.blob(0, new=True))
    want_res = {}
    want = R.expected_rows(kws, case.desc(), blobs, states, slots, R.NEW_INDEX, before, results=want_res)
    g = np.arange(case.games)
    np.testing.assert_array_equal(R.bits32(after[slots, g]), R.bits32(want))
    assert not np.array_equal(R.bits32(want), R.bits32(before[slots, g]))   # (the new weights did change the targets)
    others = np.ones(before.shape[:2], bool)
    others[slots, g] = False
    np.testing.assert_array_equal(R.bits32(after[others]), R.bits32(before[others]))
    for k in RES_KEYS:
        a, b = got_res[k], want_res[k]
        if a.ndim == 2:
            a = a[:, :b.shape[1]]
        np.testing.assert_array_equal(a, b, err_msg=k)
    assert e.selfplay_ring() == (STEPS_C, 0, STEPS_C)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_reanalyses_do_not_disturb_the_games(name, monkeypatch):
    """d.  A plays 6 steps; B plays 3, reanalyses twice (slot 1 for every game, then mixed slots) and plays 3 more: the steps played
    after the reanalyses, the episode statistics, the games' states and the ring's books are A's, and so is the next search -- the
    running search index came back."""
    case, a = _engine(name, monkeypatch, STEPS_D, STEPS_D, keep=False)
    _, b = _engine(name, monkeypatch, STEPS_D, 3)
    b.selfplay_reanalyse(1, search_index=R.NEW_INDEX)
    b.selfplay_reanalyse(_mixed_slots(case, 3), search_index=R.NEW_INDEX + 1)
    assert b.selfplay_ring() == (3, 0, 3)
    for _ in range(3):
        b.selfplay_step()
    np.testing.assert_array_equal(R.bits32(R.ring(b, case)[3:]), R.bits32(R.ring(a, case)[3:]))
    assert_stats_bits(b.selfplay_stats(), a.selfplay_stats(), name)
    assert a.selfplay_ring() == b.selfplay_ring() == (STEPS_D, 0, STEPS_D)
    for e in (a, b):
        e.search_resident()
    ra, rb = a.results(), b.results()
    for k in RES_KEYS:
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=k)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "population"])
def test_refusals_leave_the_ring_alone(name, monkeypatch):
    """e."""
    case = R.CASES[name]
    e = R.make_engine(_hip(), case)
    assert _code(e.selfplay_reanalyse, 0) == _capi.AZG_E_STATE            # no begin
    assert _code(e.selfplay_keep_states) == _capi.AZG_E_STATE
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    before = R.ring(e, case).copy()
    assert _code(e.selfplay_reanalyse, 0) == _capi.AZG_E_STATE            # no keep_states
    assert _code(e.selfplay_states) == _capi.AZG_E_STATE
    assert _code(e.selfplay_keep_states) == _capi.AZG_E_STATE             # the ring is not empty
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(before))
    e.selfplay_clear()
    e.selfplay_keep_states(True)
    for _ in range(2):
        e.selfplay_step()
    before = R.ring(e, case).copy()
    bad = np.zeros(case.games, np.int32)
    bad[case.games - 1] = 2
    for slots in (2, -1, bad):                                            # size_steps, below 0, one bad entry
        assert _code(e.selfplay_reanalyse, slots, search_index=7) == _capi.AZG_E_INVALID
        np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(before))
    with pytest.raises(ValueError):
        e.selfplay_reanalyse(np.zeros(case.games + 1, np.int32))
    e.selfplay_reanalyse(1, search_index=1)                               # (the engine still works: same weights, same index, same row)
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)[:, :, :e.s_obs]), R.bits32(before[:, :, :e.s_obs]))
    assert e.selfplay_rows(clear=True).shape[0] == 2 * case.games
    for slot in (0, 1):                                                   # cleared: every slot is out of range
        assert _code(e.selfplay_reanalyse, slot) == _capi.AZG_E_INVALID
    e.selfplay_keep_states(False)                                         # (allowed again: the ring is empty)
    e.selfplay_step()
    assert _code(e.selfplay_reanalyse, 0) == _capi.AZG_E_STATE
    e.close()


@pytest.mark.gpu
def test_refusals_of_the_search_come_through(monkeypatch):
    """e, last item: what azg_search_resident refuses is refused with its code before anything is written -- a settings table on
    nets of width 512 that came without the wide flag (AZG_E_UNSUPPORTED); once it is gone the reanalysis runs."""
    case, e = _engine("population_wide", monkeypatch, 3, 2)
    before = R.ring(e, case).copy()
    e.set_net_search([dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)] * case.nets)
    assert _code(e.selfplay_reanalyse, 0) == _capi.AZG_E_UNSUPPORTED
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(before))
    e.set_net_search(None)
    e.selfplay_reanalyse(0, search_index=0)
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(before))   # (same weights, the step's own index: the same rows)
    e.close()


@pytest.mark.gpu
def test_population_selfplay_reanalyse():
    """f.  run.PopulationSelfPlay(..., reanalyse=True, fifo=True): reanalyse(n=2) takes two distinct stored slots; the DeviceReplay view
    shows the new rows; search indices count up from REANALYSE_INDEX_BASE (the second call is reproduced with expected_rows); without
    reanalyse=True the method raises."""
    import torch
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    from alphazero_gym_amd.network.policies import make_policy
    nets = []
    for s in range(2):
        torch.manual_seed(60 + s)
        nets.append(make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2))
    T = 11
    kw = dict(game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, max_episode_length=3, capacity_steps=3, fifo=True, seed=21)
    sp = run.PopulationSelfPlay(nets, reanalyse=True, **kw)
    sp.play(4)   # (wraps)
    view = DeviceReplay(sp.engine, 1)
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.mul_(1.5)
    first = sp.reanalyse(n=2)
    assert len(first) == 2 and len(set(first)) == 2 and all(0 <= s < 3 for s in first)
    before = sp.engine.selfplay_rows(clear=False).reshape(3, 2 * T, -1).copy()
    states = sp.engine.selfplay_states().reshape(3, 2 * T, -1).copy()
    second = sp.reanalyse(slots=[2])
    assert second == [2]
    got = view.rows().cpu().numpy().reshape(3, 2 * T, -1)
    np.testing.assert_array_equal(got, sp.engine.selfplay_rows(clear=False).reshape(3, 2 * T, -1))
    ekw = dict(env_id=0, mode=0, n_sims=8, c_uct=1.5, gamma=1.0, num_actions=2, seed=21)
    desc = _capi.policy_blob(nets[0])[0]
    want = R.expected_rows([dict(ekw, tree_id_base=k * T) for k in range(2)], desc, [_capi.policy_blob(n)[1] for n in nets], states, 2,
                           run.REANALYSE_INDEX_BASE + 2, before)
    np.testing.assert_array_equal(R.bits32(got[2]), R.bits32(want))
    np.testing.assert_array_equal(R.bits32(got[:2]), R.bits32(before[:2]))
    assert len(sp.reanalyse(n=5)) == 3   # (no more than the ring holds)
    per_game = np.arange(2 * T, dtype=np.int32) % 3
    used = sp.reanalyse(slots=per_game)
    assert len(used) == 1 and np.array_equal(used[0], per_game)
    sp.close()
    plain = run.PopulationSelfPlay(nets, **kw)
    plain.play(1)
    with pytest.raises(RuntimeError, match="reanalyse=True"):
        plain.reanalyse()
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"])])
def test_examples_train_from_a_reanalysed_ring(example, extra):
    """--replay-steps 4 --reanalyse-slots 2: the FIFO ring wraps (3 iterations of 2 steps), stored steps are reanalysed before every
    iteration's training, and the loop trains."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module(example)
    a = mod.parse_args(["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4",
                        "--reanalyse-slots", "2", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5",
                        "--device", "cuda"] + extra)
    hist = mod.train(a, log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
