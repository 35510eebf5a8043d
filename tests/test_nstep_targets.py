"""N-step return value targets for the device replay ring (azg_selfplay_keep_transitions / _transitions / _nstep_targets,
run.PopulationSelfPlay n_step=...) on the GPU: the kept transitions against the restatement's trace, the V_target column against the
numpy recurrence, what the calls leave alone, growth, clears, reanalysed values, the refusals and the Python layer.  Everything is
compared bit for bit.  Cases, sizes and the CPU truth: tests/nstep_util.py."""
import ctypes as C

import numpy as np
import pytest

import nstep_util as N
import reanalyse_util as R
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

RES_KEYS = ("counts", "n_children", "actions", "Q", "v_target")
TR_KEYS = ("reward", "value", "action", "end")
# At n_step >= 1 a target is its step's reward plus a discounted value, not the step's own value: of the rows whose window holds a step
# at all (every row but the newest step's and the time-limit steps' own) nearly all differ in bits from (float)value.  At least half
# of ALL rows must: a call that writes nothing, or the plain values, fails.
MIN_CHANGED = 0.5


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _engine(name, capacity, fifo, steps, transitions=True, states=False):
    case = N.CASES[name]
    e = R.make_engine(_hip(), case)
    R.begin(e, case, capacity, fifo=fifo, keep=states)
    if transitions:
        e.selfplay_keep_transitions(True)
    for _ in range(steps):
        e.selfplay_step()
    return case, e


def _whole_ring(e, case):
    """Every slot of the replay ring, used or not: [capacity, G, row_len] as uint32."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    e.sync()
    ring = DeviceReplay(e, 1).ring.cpu().numpy()
    return np.ascontiguousarray(ring).view(np.uint32).reshape(-1, case.games, ring.shape[1]).copy()


def _transitions(e, case):
    return {k: v.reshape(-1, case.games) for k, v in e.selfplay_transitions().items()}


def _assert_transitions(got, ref, held, what=""):
    for k in TR_KEYS:
        a, b = got[k], ref[k][held]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        view = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view), err_msg=f"{what}: {k}")


def _gamma(case, gamma):
    return N.search_gamma(case) if gamma is None else gamma


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_kept_transitions_are_the_trace(name, capacity, fifo):
    """Reward, float64 value, action and end kind of every stored step equal the restatement's trace, slot by slot (FIFO: the ring
    has wrapped), and keeping them does not move the rows.  The CartPole input must hold every kind of window."""
    steps = N.STEPS[name]
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    held, oldest = N.ring_layout(capacity, fifo, steps)
    assert e.selfplay_ring() == (len(held), oldest, steps)
    _assert_transitions(_transitions(e, case), ref, held, name)
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(ref["rows"][held]))
    e.close()
    stored = np.sort(held)
    end = ref["end"][stored]
    if name == "cartpole":
        both = ref["both"][stored]
        assert ((end == N.END_TERMINAL) & ~both).any() and (end == N.END_LENGTH).any() and both.any()
        kinds = N.window_kinds(end, 3)
        assert kinds["cut_by_newest"] > 0 and kinds["full"] > 0 and kinds["terminal_inside"] > 0 and kinds["length_inside"] > 0, kinds
    if name == "pendulum":
        assert set(np.unique(end)) == {N.END_NONE, N.END_LENGTH} and case.kw["tree_id_base"] == 5
        scale = case.kw.get("reward_scale", _capi.PENDULUM_R_SCALE)
        assert scale != 1.0 and (ref["reward"] != ref["reward"] * scale).any()   # (reward_scale is in play)


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_targets_are_the_recurrence_and_nothing_else_is_written(name, capacity, fifo):
    """For n_step in {0, 1, 3, 1000}, with the search's gamma (per net in the population) and with 0.9: the V_target column is the
    truth; every other column, every unused slot and the kept transitions are unchanged; at n_step >= 1 at least half of the targets
    differ from the plain values; a second call changes nothing."""
    steps = N.STEPS[name]
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    held, _ = N.ring_layout(capacity, fifo, steps)
    before = _whole_ring(e, case)
    assert before.shape[0] == capacity
    tr = _transitions(e, case)
    plain = R.bits32(ref["value"][held].astype(np.float32))
    np.testing.assert_array_equal(before[:len(held), :, -1], plain)
    for gamma in N.GAMMAS:
        for n in N.N_STEPS:
            what = f"{name} n_step {n} gamma {gamma}"
            e.selfplay_nstep_targets(n, gamma)
            got = _whole_ring(e, case)
            want = N.ring_targets(ref["reward"], ref["value"], ref["end"], held, n, _gamma(case, gamma))
            np.testing.assert_array_equal(got[:len(held), :, -1], R.bits32(want), err_msg=what)
            np.testing.assert_array_equal(got[:, :, :-1], before[:, :, :-1], err_msg=what)
            np.testing.assert_array_equal(got[len(held):], before[len(held):], err_msg=what)
            if n == 0:
                np.testing.assert_array_equal(got, before, err_msg=what)
            else:
                changed = float((got[:len(held), :, -1] != plain).mean())
                assert changed >= MIN_CHANGED, (what, changed)
            e.selfplay_nstep_targets(n, gamma)
            np.testing.assert_array_equal(_whole_ring(e, case), got, err_msg=what + " (second call)")
    _assert_transitions(_transitions(e, case), tr, slice(None), name)
    if case.nets > 1:   # (the nets' gammas differ, so one gamma for all would not have passed)
        one = N.ring_targets(ref["reward"], ref["value"], ref["end"], held, 3, case.kw["gamma"])
        mine = N.ring_targets(ref["reward"], ref["value"], ref["end"], held, 3, N.search_gamma(case))
        T = case.T
        assert (R.bits32(one[:, :T]) != R.bits32(mine[:, :T])).any() and (R.bits32(one[:, 2 * T:]) != R.bits32(mine[:, 2 * T:])).any()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_calls_leave_the_live_games_alone(name, capacity, fifo):
    """A keeps nothing and plays s + 1 steps; B keeps the transitions, plays s, makes two calls and plays one more: the further
    step's rows, the episode statistics, the games' states, the kept states and the next search (the carried counts) are A's."""
    steps = N.STEPS[name] if fifo else min(N.STEPS[name], capacity - 1)
    case, a = _engine(name, capacity, fifo, steps + 1, transitions=False, states=True)
    _, b = _engine(name, capacity, fifo, steps, states=True)
    b.selfplay_nstep_targets(3)
    b.selfplay_nstep_targets(1000, 0.9)
    b.selfplay_step()
    held, _ = N.ring_layout(capacity, fifo, steps + 1)
    newest = int(np.argmax(held))
    np.testing.assert_array_equal(R.bits32(R.ring(b, case)[newest]), R.bits32(R.ring(a, case)[newest]))
    np.testing.assert_array_equal(R.bits32(R.ring(b, case)[:, :, :-1]), R.bits32(R.ring(a, case)[:, :, :-1]))
    np.testing.assert_array_equal(R.bits64(b.selfplay_states()), R.bits64(a.selfplay_states()))
    assert_stats_bits(b.selfplay_stats(), a.selfplay_stats(), name)
    assert a.selfplay_ring() == b.selfplay_ring()
    for e in (a, b):
        e.search_resident()
    ra, rb = a.results(), b.results()
    for k in RES_KEYS:
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=k)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_three_more_steps_and_another_call_give_the_longer_runs_targets(name, capacity, fifo):
    steps = N.STEPS[name] if fifo else min(N.STEPS[name], capacity - 3)
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    e.selfplay_nstep_targets(3)
    first = R.ring(e, case).copy()
    held0, _ = N.ring_layout(capacity, fifo, steps)
    np.testing.assert_array_equal(R.bits32(first[:, :, -1]),
                                  R.bits32(N.ring_targets(ref["reward"], ref["value"], ref["end"], held0, 3, N.search_gamma(case))))
    for _ in range(3):
        e.selfplay_step()
    e.selfplay_nstep_targets(3)
    held, _ = N.ring_layout(capacity, fifo, steps + 3)
    got = R.ring(e, case)
    want = N.ring_targets(ref["reward"], ref["value"], ref["end"], held, 3, N.search_gamma(case))
    np.testing.assert_array_equal(R.bits32(got[:, :, -1]), R.bits32(want))
    np.testing.assert_array_equal(R.bits32(got[:, :, :-1]), R.bits32(ref["rows"][held][:, :, :-1]))
    if not fifo:   # (only rows whose window grew have changed: those that saw the newest step within 3 steps and no end before it)
        same = (R.bits32(got[:steps]) == R.bits32(first)).all(axis=-1)
        assert same[:steps - 3].all() and not same[steps - 3:].all()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_no_window_reaches_across_a_clear(name):
    """STOP mode: play 5, call, download with clear, play 4, call: the second ring's windows start at step 5."""
    ref = N.reference(name)
    case, e = _engine(name, 8, False, 5)
    e.selfplay_nstep_targets(1000)
    rows = e.selfplay_rows(clear=True).reshape(5, case.games, -1)
    g = N.search_gamma(case)
    np.testing.assert_array_equal(R.bits32(rows[:, :, -1]), R.bits32(N.ring_targets(ref["reward"], ref["value"], ref["end"], np.arange(5), 1000, g)))
    assert e.selfplay_transitions()["end"].shape == (0,)
    e.selfplay_nstep_targets(1000)   # (an empty ring: nothing to do)
    for _ in range(4):
        e.selfplay_step()
    held = np.arange(5, 9)
    _assert_transitions(_transitions(e, case), ref, held, name)
    for n in (2, 1000):
        e.selfplay_nstep_targets(n)
        got = R.ring(e, case)
        np.testing.assert_array_equal(R.bits32(got[:, :, -1]), R.bits32(N.ring_targets(ref["reward"], ref["value"], ref["end"], held, n, g)))
        np.testing.assert_array_equal(R.bits32(got[:, :, :-1]), R.bits32(ref["rows"][held][:, :, :-1]))
    # (had the first ring seen the later steps, its windows would differ wherever step 4 did not end an episode: the test can tell)
    across = N.ring_targets(ref["reward"], ref["value"], ref["end"], np.arange(9), 1000, g)
    open_at_4 = ref["end"][4] == N.END_NONE
    assert open_at_4.any() == (name == "cartpole")   # (Pendulum's length limit of 5 falls on step 4 for every game)
    assert (R.bits32(across[:5]) != R.bits32(rows[:, :, -1]))[:, open_at_4].any() == open_at_4.any()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(N.CASES))
def test_reanalysed_values_feed_the_targets(name):
    """With the states kept as well: new weights, two slots reanalysed, then a call.  The reanalysed rows' actions | counts | Q are the
    oracle's ordinary search of the kept state, the kept float64 values of those rows are that search's value targets -- reward, action
    and end stay --, and every V_target follows from the mixed old and new values."""
    steps = min(N.STEPS[name], 8)
    ref = N.reference(name)
    case, e = _engine(name, steps, False, steps, states=True)
    before = R.ring(e, case).copy()
    states = e.selfplay_states().reshape(steps, case.games, -1).copy()
    R.set_weights(e, case, new=True)
    kws, blobs = ([case.net_kw(k) for k in range(case.nets)], case.blobs(new=True)) if case.nets > 1 else (case.net_kw(0), case.blob(0, new=True))
    value = ref["value"][:steps].copy()
    want_rows = before.copy()
    for j, slot in enumerate((1, steps - 3)):
        e.selfplay_reanalyse(slot, search_index=R.NEW_INDEX + j)
        res = {}
        want_rows[slot] = R.expected_rows(kws, case.desc(), blobs, states, slot, R.NEW_INDEX + j, before, results=res)
        value[slot] = res["v_target"]
    assert (R.bits64(value) != R.bits64(ref["value"][:steps])).any()
    mid = R.ring(e, case)
    np.testing.assert_array_equal(R.bits32(mid), R.bits32(want_rows))   # (a reanalysis leaves plain search values)
    tr = _transitions(e, case)
    np.testing.assert_array_equal(R.bits64(tr["value"]), R.bits64(value))
    mixed = dict(ref, value=value)
    _assert_transitions(tr, {k: mixed[k][:steps] for k in TR_KEYS}, slice(None), name)
    for n, gamma in ((3, None), (1, 0.9), (0, None)):
        e.selfplay_nstep_targets(n, gamma)
        got = R.ring(e, case)
        np.testing.assert_array_equal(R.bits32(got[:, :, :-1]), R.bits32(want_rows[:, :, :-1]))
        want = N.ring_targets(ref["reward"][:steps], value, ref["end"][:steps], np.arange(steps), n, _gamma(case, gamma))
        np.testing.assert_array_equal(R.bits32(got[:, :, -1]), R.bits32(want), err_msg=f"{name} n_step {n} gamma {gamma}")
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(want_rows))   # (n_step 0: the reanalysed ring itself)
    e.close()


def _raw_call(e, struct_size=None, n_step=1, gamma=0.9, flags=0):
    c = _capi.AzgNstepConfig()
    c.struct_size = C.sizeof(_capi.AzgNstepConfig) if struct_size is None else struct_size
    c.n_step, c.gamma, c.flags = n_step, gamma, flags
    return e._f["selfplay_nstep_targets"](e._h, C.byref(c))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_refusals_leave_the_ring_alone(name):
    case = N.CASES[name]
    e = R.make_engine(_hip(), case)
    assert _code(e.selfplay_nstep_targets, 1) == _capi.AZG_E_STATE          # no begin
    assert _code(e.selfplay_keep_transitions) == _capi.AZG_E_STATE
    assert _code(e.selfplay_transitions) == _capi.AZG_E_STATE
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    before = _whole_ring(e, case)
    assert _code(e.selfplay_nstep_targets, 1) == _capi.AZG_E_STATE          # no keep_transitions
    assert _code(e.selfplay_transitions) == _capi.AZG_E_STATE
    assert _code(e.selfplay_keep_transitions) == _capi.AZG_E_STATE          # the ring is not empty
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    e.selfplay_clear()
    e.selfplay_keep_transitions(True)
    assert _raw_call(e) == _capi.AZG_OK                                     # an empty ring: nothing is launched
    for _ in range(2):
        e.selfplay_step()
    before = _whole_ring(e, case)
    assert _code(e.selfplay_nstep_targets, -1) == _capi.AZG_E_INVALID
    for gamma in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert _code(e.selfplay_nstep_targets, 1, gamma) == _capi.AZG_E_INVALID, gamma
    assert _raw_call(e, struct_size=C.sizeof(_capi.AzgNstepConfig) - 4) == _capi.AZG_E_INVALID
    assert _raw_call(e, struct_size=0) == _capi.AZG_E_INVALID
    assert _raw_call(e, flags=2) == _capi.AZG_E_INVALID                     # an unknown flag
    assert _raw_call(e, n_step=-1, flags=_capi.NSTEP_SEARCH_GAMMA) == _capi.AZG_E_INVALID
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    assert _raw_call(e, n_step=0, gamma=float("nan"), flags=_capi.NSTEP_SEARCH_GAMMA) == _capi.AZG_OK   # (the flag: gamma is not read)
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    e.selfplay_nstep_targets(1, 0.0)                                        # (gamma 0 is a discount like any other: the reward alone)
    tr = _transitions(e, case)
    got = R.ring(e, case)[:, :, -1]
    np.testing.assert_array_equal(R.bits32(got[0]), R.bits32(tr["reward"][0].astype(np.float32) + np.float32(0.0)))
    assert e.selfplay_rows(clear=True).shape[0] == 2 * case.games
    e.selfplay_keep_transitions(False)                                      # (allowed again: the ring is empty)
    e.selfplay_step()
    assert _code(e.selfplay_nstep_targets, 1) == _capi.AZG_E_STATE
    e.selfplay_clear()
    e.selfplay_keep_transitions(True)                                       # (on again within one begin)
    e.selfplay_step()
    e.selfplay_nstep_targets(1)
    R.begin(e, case, 4, keep=False)                                         # the next begin drops it
    e.selfplay_step()
    assert _code(e.selfplay_nstep_targets, 1) == _capi.AZG_E_STATE
    e.close()


def _policies(n):
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    nets = []
    for s in range(n):
        torch.manual_seed(80 + s)
        nets.append(make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2))
    return nets


def _cpu_run(nets, T, steps, max_len, ekw):
    """The restatement's run of these policies, net by net: rows and transitions [steps, K * T]."""
    import selfplay_ref as SR
    parts = []
    for k, net in enumerate(nets):
        desc, blob = _capi.policy_blob(net)[:2]
        trace = []
        out = SR.cpu_selfplay(dict(ekw, tree_id_base=ekw.get("tree_id_base", 0) + k * T), desc, blob, T, steps,
                              begin=dict(max_episode_length=max_len), trace=trace)
        t = N.transitions_of(trace, steps, T, False, False, 1.0)
        t["rows"] = out["rows"].reshape(steps, T, -1)
        parts.append(t)
    return {k: np.concatenate([p[k] for p in parts], 1) for k in parts[0]}


@pytest.mark.gpu
def test_population_selfplay_and_device_selfplay_return_nstep_rows():
    """run.PopulationSelfPlay(n_step=3).collect() and run.DeviceSelfPlay(n_step=3): the rows' last column is the truth, the others are
    today's; target_gamma replaces the search's gamma; nstep_targets() can be called by hand; n_step=None returns today's rows and keeps
    nothing."""
    from alphazero_gym_amd import run
    nets = _policies(2)
    T, steps, max_len = 11, 6, 4
    kw = dict(game="CartPole-v0", n_rollouts=8, c_uct=1.5, gamma=0.97, max_episode_length=max_len, capacity_steps=steps, seed=21)
    ekw = dict(env_id=0, mode=0, n_sims=8, c_uct=1.5, gamma=0.97, num_actions=2, seed=21)
    ref = _cpu_run(nets, T, steps, max_len, ekw)
    assert (ref["end"] == N.END_LENGTH).any()

    def want(n, gamma, cols=slice(None)):
        rows = ref["rows"].copy()
        rows[:, :, -1] = N.ring_targets(ref["reward"], ref["value"], ref["end"], np.arange(steps), n, gamma)
        return rows[:, cols]

    sp = run.PopulationSelfPlay(nets, games_per_net=T, n_step=3, **kw)
    got = sp.collect(steps)
    for k in range(2):
        np.testing.assert_array_equal(R.bits32(got[k].numpy().reshape(steps, T, -1)), R.bits32(want(3, 0.97, slice(k * T, (k + 1) * T))))
    sp.play(steps)                       # (the ring was cleared; the games go on: only the hand-made calls are checked here)
    sp.nstep_targets(n_step=0)
    plain = sp.engine.selfplay_rows(clear=False).copy()
    tr = sp.engine.selfplay_transitions()
    np.testing.assert_array_equal(R.bits32(plain[:, -1]), R.bits32(tr["value"].astype(np.float32)))
    sp.nstep_targets(n_step=1, gamma=0.5)
    G = 2 * T
    col = N.ring_targets(tr["reward"].reshape(steps, G), tr["value"].reshape(steps, G), tr["end"].reshape(steps, G), np.arange(steps), 1, 0.5)
    np.testing.assert_array_equal(R.bits32(sp.engine.selfplay_rows(clear=False)[:, -1].reshape(steps, G)), R.bits32(col))
    sp.close()

    one = run.DeviceSelfPlay(nets[0], n_games=T, n_step=3, target_gamma=0.9, **kw)
    np.testing.assert_array_equal(R.bits32(one.collect(steps).numpy().reshape(steps, T, -1)), R.bits32(want(3, 0.9, slice(0, T))))
    one.close()
    dev = run.DeviceSelfPlay(nets[0], n_games=T, n_step=3, **kw)   # (rows handed over on the device carry the same targets)
    got = dev.collect_device(steps, dev.replay(1)).cpu().numpy().reshape(steps, T, -1)
    np.testing.assert_array_equal(R.bits32(got), R.bits32(want(3, 0.97, slice(0, T))))
    assert dev.play_device(2) == (2, 0)
    tr = {k: v.reshape(2, T) for k, v in dev.engine.selfplay_transitions().items()}
    col = N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(2), 3, 0.97)
    np.testing.assert_array_equal(R.bits32(dev.engine.selfplay_rows(clear=False)[:, -1].reshape(2, T)), R.bits32(col))
    dev.close()

    off = run.PopulationSelfPlay(nets, games_per_net=T, **kw)
    got = off.collect(steps)
    for k in range(2):
        np.testing.assert_array_equal(R.bits32(got[k].numpy().reshape(steps, T, -1)), R.bits32(ref["rows"][:, k * T:(k + 1) * T]))
    off.play(1)
    assert _code(off.engine.selfplay_transitions) == _capi.AZG_E_STATE
    with pytest.raises(RuntimeError, match="n_step"):
        off.nstep_targets()
    off.close()
    with pytest.raises(ValueError, match="n_step"):
        run.PopulationSelfPlay(nets, games_per_net=T, n_step=-1, **kw)


@pytest.mark.gpu
def test_reanalyse_of_the_python_layer_ends_with_nstep_targets():
    """run.PopulationSelfPlay(reanalyse=True, n_step=2).reanalyse(): the reanalysed rows do not fall back to plain search values --
    the ring's last column is the recurrence over the kept transitions, whose values the reanalysis refreshed."""
    import torch
    from alphazero_gym_amd import run
    nets = _policies(2)
    T, steps = 11, 5
    sp = run.PopulationSelfPlay(nets, games_per_net=T, n_step=2, reanalyse=True, game="CartPole-v0", n_rollouts=8, c_uct=1.5, gamma=0.97,
                                max_episode_length=4, capacity_steps=steps, seed=21)
    sp.play(steps)
    old = sp.engine.selfplay_transitions()["value"].copy()
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.mul_(1.5)
    assert sp.reanalyse(slots=[1, 3]) == [1, 3]
    tr = {k: v.reshape(steps, 2 * T) for k, v in sp.engine.selfplay_transitions().items()}
    changed = (R.bits64(tr["value"]) != R.bits64(old.reshape(steps, 2 * T))).any(axis=1)
    assert changed.tolist() == [False, True, False, True, False]
    col = N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), 2, 0.97)
    got = sp.engine.selfplay_rows(clear=False)[:, -1].reshape(steps, 2 * T)
    np.testing.assert_array_equal(R.bits32(got), R.bits32(col))
    assert (R.bits32(got) != R.bits32(tr["value"].astype(np.float32))).mean() >= MIN_CHANGED
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"])])
def test_examples_train_on_nstep_targets(example, extra):
    """--n-step 3 with --replay-steps 4 --reanalyse-slots 1: the FIFO ring wraps, and the loop trains on finite targets."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module(example)
    a = mod.parse_args(["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4",
                        "--reanalyse-slots", "1", "--n-step", "3", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8",
                        "--max-episode-length", "5", "--device", "cuda"] + extra)
    assert a.n_step == 3
    hist = mod.train(a, log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
