"""Refreshing the replay ring's bootstrap values from the value head (azg_selfplay_refresh_values, include/azgym_refresh.h;
run.PopulationSelfPlay.refresh_values) on the GPU: every stored row's kept value against the oracle's MLP evaluation of the row's
observation, what the call leaves alone, slot lists, the grids of the tile loop, the value targets and priorities that follow, the target
weight set, the live games, the order with a reanalysis, the refusals and the example.  Everything is compared bit for bit.  Cases:
tests/nstep_util.py; the truth: tests/value_refresh_util.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import lambda_util as L
import nstep_util as N
import oracle_lib as O
import priority_util as P
import reanalyse_util as R
import value_refresh_util as V
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

pytestmark = pytest.mark.gpu

RES_KEYS = ("counts", "n_children", "actions", "Q", "v_target")
KEPT = ("reward", "action", "end")
ALPHA, EPS = 0.6, 1e-3
# a search value is a visit-weighted mean over a tree, a refreshed one the raw head output under other weights: nearly every row's
# bits differ.  At least half must, or the call wrote nothing.
MIN_CHANGED = 0.5
RING = dict(zip(N.RING_IDS, N.RINGS))


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _engine(name, capacity, fifo, steps, states=False, prio=False, transitions=True):
    case = V.CASES[name]
    e = R.make_engine(_hip(), case)
    R.begin(e, case, capacity, fifo=fifo, keep=states)
    if transitions:
        e.selfplay_keep_transitions(True)
    if prio:
        e.selfplay_keep_priorities(True)
        e.selfplay_keep_errors(True)
    for _ in range(steps):
        e.selfplay_step()
    if prio:   # priorities and errors that stand while the values change
        e.selfplay_priorities(ALPHA, EPS)
        n = e.selfplay_ring()[0] * case.games
        e.selfplay_set_error_values(np.random.default_rng(7).random(n).astype(np.float32))
    return case, e


def _blobs(case):
    return [V.refresh_blob(case, k) for k in range(case.nets)]


def _set_blobs(e, case, blobs):
    if case.nets == 1:
        e.set_weights(case.desc(), blobs[0])
    else:
        for k in range(case.nets):
            e.set_net_weights(k, case.desc(), blobs[k])


def _one_net(case, blobs):
    """value_refresh_util's fallback: a one-net engine holding net k's weights."""
    def make(k):
        e = _hip()(**dict(case.net_kw(k), n_trees=case.T))
        e.set_weights(case.desc(), blobs[k])
        return e
    return make


def _snapshot(e, case, states=False, prio=False):
    """Every download of the ring, as bits: the whole ring (unused slots too), the kept transitions, and where kept the states, the
    priority values and the errors."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    e.sync()
    ring = DeviceReplay(e, 1).ring.cpu().numpy()
    snap = {"ring": np.ascontiguousarray(ring).view(np.uint32).reshape(-1, case.games, ring.shape[1]).copy()}
    tr = e.selfplay_transitions()
    snap["value"] = V.bits64(tr["value"]).reshape(-1, case.games)
    snap["reward"] = V.bits64(tr["reward"]).reshape(-1, case.games)
    snap["action"] = V.bits32(tr["action"]).reshape(-1, case.games)
    snap["end"] = tr["end"].reshape(-1, case.games).copy()
    if states:
        snap["states"] = V.bits64(e.selfplay_states())
    if prio:
        snap["priority"] = e.selfplay_priority_values().copy()
        snap["errors"] = V.bits32(e.selfplay_error_values())
    return snap


def _assert_same(got, want, what, but=(), stored=None):
    """``stored``: the snapshots are of two engines, whose unused ring slots hold whatever their memory held: the stored slots only."""
    assert set(got) == set(want)
    for k in want:
        if k not in but:
            a, b = (got[k][:stored], want[k][:stored]) if k == "ring" and stored is not None else (got[k], want[k])
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k}")


def _truth(e, case, blobs):
    """float64 [size, G]: the oracle's value of every stored row's observation columns under ``blobs``."""
    obs = np.ascontiguousarray(R.ring(e, case)[:, :, :e.s_obs])
    return V.case_truth(case, obs, blobs, fallback=_one_net(case, blobs))


@functools.lru_cache(maxsize=None)
def _default_grid(ring_id):
    """(the snapshot before, the truth, the snapshot after) of a refresh of every slot on the default grid, per ring: computed once."""
    name, capacity, fifo = RING[ring_id]
    case, e = _engine(name, capacity, fifo, N.STEPS[name], states=True, prio=True)
    before = _snapshot(e, case, True, True)
    blobs = _blobs(case)
    _set_blobs(e, case, blobs)
    e.selfplay_refresh_values()
    after = _snapshot(e, case, True, True)
    truth = _truth(e, case, blobs)
    e.close()
    for part in (before, after):
        for a in part.values():
            a.setflags(write=False)
    truth.setflags(write=False)
    return before, truth, after


@pytest.mark.parametrize("ring_id", N.RING_IDS)
def test_every_stored_value_is_the_value_head_and_nothing_else_is_written(ring_id):
    name, capacity, fifo = RING[ring_id]
    case = V.CASES[name]
    before, truth, after = _default_grid(ring_id)
    size = min(capacity, N.STEPS[name])
    assert truth.shape == (size, case.games) and before["ring"].shape[0] == capacity
    np.testing.assert_array_equal(after["value"], V.bits64(truth), err_msg=ring_id)
    _assert_same(after, before, ring_id, but=("value",))
    assert (after["value"] != before["value"]).mean() >= MIN_CHANGED
    assert np.isfinite(truth).all() and np.ptp(truth) > 0.0
    if case.nets > 1:   # (net k's rows carry net k's value: under net 0's weights the other nets' columns would hold other bits)
        blobs = _blobs(case)
        obs = np.ascontiguousarray(before["ring"][:size, :, :case.net[0]]).view(np.float32)
        other = V.case_truth(case, obs, [blobs[0]] * case.nets)
        assert (V.bits64(other[:, case.T:]) != after["value"][:, case.T:]).mean() >= MIN_CHANGED
    if name == "many_children":   # (the long row: the observation stride is not the row stride)
        assert before["ring"].shape[2] > case.net[0] + 3 * 16 + 1


@pytest.mark.parametrize("ring_id", ["cartpole-fifo16", "pendulum-stop25", "population-stop11"])
def test_a_slot_list_refreshes_those_slots_only_and_twice_is_once(ring_id):
    name, capacity, fifo = RING[ring_id]
    assert ring_id in N.RING_IDS
    before, truth, _ = _default_grid(ring_id)
    case, e = _engine(name, capacity, fifo, N.STEPS[name], states=True, prio=True)
    _set_blobs(e, case, _blobs(case))
    size = truth.shape[0]
    _assert_same(_snapshot(e, case, True, True), before, ring_id, stored=size)   # (the twin of _default_grid's engine)
    before = _snapshot(e, case, True, True)
    old = before["value"].view(np.float64)
    value = old
    for slots in ([size - 1, 2], [1, 1], [2], []):
        e.selfplay_refresh_values(slots)
        value = V.refreshed(value, truth, slots)
        got = _snapshot(e, case, True, True)
        np.testing.assert_array_equal(got["value"], V.bits64(value), err_msg=f"{ring_id} slots {slots}")
        _assert_same(got, before, f"{ring_id} slots {slots}", but=("value",))
        e.selfplay_refresh_values(slots)
        _assert_same(_snapshot(e, case, True, True), got, f"{ring_id} slots {slots} (second call)")
    untouched = [s for s in range(size) if s not in (size - 1, 2, 1)]
    np.testing.assert_array_equal(V.bits64(value[untouched]), before["value"][untouched])
    assert (V.bits64(value[[1, 2, size - 1]]) != before["value"][[1, 2, size - 1]]).mean() >= MIN_CHANGED
    e.selfplay_refresh_values()
    np.testing.assert_array_equal(_snapshot(e, case, True, True)["value"], V.bits64(truth))
    e.close()


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("ring_id", ["cartpole-fifo16", "pendulum-stop25", "wide-stop8", "population-stop11"])
def test_every_grid_gives_the_same_bits(ring_id, groups, monkeypatch):
    """AZG_EVAL_GROUPS=1 / 2: one or two workgroups per net walk all of its tiles (the multi-trip tile loop)."""
    name, capacity, fifo = RING[ring_id]
    assert ring_id in N.RING_IDS
    _, truth, after = _default_grid(ring_id)
    monkeypatch.setenv("AZG_EVAL_GROUPS", str(groups))
    case, e = _engine(name, capacity, fifo, N.STEPS[name], states=True, prio=True)
    assert truth.shape[0] * case.T > 16 * groups   # (more tiles than workgroups: every workgroup makes several trips)
    _set_blobs(e, case, _blobs(case))
    e.selfplay_refresh_values()
    _assert_same(_snapshot(e, case, True, True), after, f"{ring_id} groups {groups}", stored=truth.shape[0])
    e.selfplay_refresh_values([1, 0, 1])
    _assert_same(_snapshot(e, case, True, True), after, f"{ring_id} groups {groups}, a list", stored=truth.shape[0])
    e.close()


@pytest.mark.parametrize("ring_id", ["cartpole-fifo16", "population-stop11"])
def test_priorities_follow_the_refreshed_values(ring_id):
    name, capacity, fifo = RING[ring_id]
    _, truth, _ = _default_grid(ring_id)
    case, e = _engine(name, capacity, fifo, N.STEPS[name], prio=True)
    _set_blobs(e, case, _blobs(case))
    stale = e.selfplay_priority_values().copy()
    e.selfplay_refresh_values()
    np.testing.assert_array_equal(e.selfplay_priority_values(), stale)   # (the call itself leaves them: the caller recomputes)
    e.selfplay_priorities(ALPHA, EPS)
    z = R.ring(e, case)[:, :, -1]
    want = P.priorities(P.gap(truth, z), ALPHA, EPS)
    np.testing.assert_array_equal(e.selfplay_priority_values().reshape(want.shape), want)
    assert (want.reshape(-1) != stale).mean() >= MIN_CHANGED
    e.close()


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_a_reanalysis_and_a_refresh_overwrite_each_other(name):
    """reanalyse(slot) after a refresh puts that search's value back into the slot only; a refresh after it replaces it again."""
    steps = 6
    case, e = _engine(name, steps, False, steps, states=True)
    blobs = _blobs(case)
    _set_blobs(e, case, blobs)
    truth = _truth(e, case, blobs)
    states = e.selfplay_states().reshape(steps, case.games, -1).copy()
    e.selfplay_refresh_values()
    rows = R.ring(e, case).copy()
    slot = 2
    e.selfplay_reanalyse(slot, search_index=R.NEW_INDEX)
    kws, b = ([case.net_kw(k) for k in range(case.nets)], blobs) if case.nets > 1 else (case.net_kw(0), blobs[0])
    res = {}
    want_rows = rows.copy()
    want_rows[slot] = R.expected_rows(kws, case.desc(), b, states, slot, R.NEW_INDEX, rows, results=res)
    value = truth.copy()
    value[slot] = res["v_target"]
    got = e.selfplay_transitions()["value"].reshape(steps, case.games)
    np.testing.assert_array_equal(V.bits64(got), V.bits64(value))
    assert (V.bits64(value[slot]) != V.bits64(truth[slot])).mean() >= MIN_CHANGED
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(want_rows))
    e.selfplay_refresh_values([slot])
    got = e.selfplay_transitions()["value"].reshape(steps, case.games)
    np.testing.assert_array_equal(V.bits64(got), V.bits64(truth))
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(want_rows))   # (the reanalysed rows stay)
    e.close()


@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_refreshes_leave_the_live_games_alone(name, capacity, fifo):
    """Twins: A plays s + 2 steps; B plays s, refreshes, plays one, refreshes a list, plays one, refreshes.  Every row, the kept reward /
    action / end and states, the values of the steps stored after B's refreshes' reach, the books, the games, the last search's results
    and the next search are A's."""
    steps = N.STEPS[name] if fifo else min(N.STEPS[name], capacity - 2)
    case, a = _engine(name, capacity, fifo, steps + 2, states=True)
    _, b = _engine(name, capacity, fifo, steps, states=True)
    b.selfplay_refresh_values()
    b.selfplay_step()
    b.selfplay_refresh_values([0, 1])
    b.selfplay_step()
    sa = _snapshot(a, case, True)
    b.selfplay_refresh_values([0])
    ra, rb = a.results(), b.results()   # (the last search's: the step's, not recomputed from anything the refresh touched)
    for k in RES_KEYS:
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=f"last search: {k}")
    sb = _snapshot(b, case, True)
    _assert_same(sb, sa, name, but=("value",), stored=a.selfplay_ring()[0])
    held, _ = N.ring_layout(capacity, fifo, steps + 2)
    newest = int(np.argmax(held))
    assert newest != 0
    np.testing.assert_array_equal(sb["value"][newest], sa["value"][newest])   # (stored after the last refresh that could reach it)
    if name != "many_children":   # (whose playing net has a value head of 0 everywhere, and search values to match)
        assert (sb["value"][0] != sa["value"][0]).mean() >= MIN_CHANGED
    assert_stats_bits(b.selfplay_stats(), a.selfplay_stats(), name)
    assert a.selfplay_ring() == b.selfplay_ring()
    for e in (a, b):
        e.search_resident()   # (the running search index, the roots and the carried counts)
    ra, rb = a.results(), b.results()
    for k in RES_KEYS:
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=f"next search: {k}")
    a.close()
    b.close()


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _raw(e, slots, n):
    arr = None if slots is None else np.ascontiguousarray(slots, np.int32)
    return e._f["selfplay_refresh_values"](e._h, None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)), n)


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_refusals_leave_the_ring_alone(name):
    case = V.CASES[name]
    e = R.make_engine(_hip(), case)
    assert e._f["selfplay_refresh_values"](None, None, 0) == _capi.AZG_E_INVALID   # NULL engine
    assert _code(e.selfplay_refresh_values) == _capi.AZG_E_STATE           # no begin
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    assert _code(e.selfplay_refresh_values) == _capi.AZG_E_STATE           # no keep_transitions
    assert _code(e.selfplay_refresh_values, [0]) == _capi.AZG_E_STATE
    e.selfplay_clear()
    e.selfplay_keep_transitions(True)
    assert _raw(e, None, 0) == _capi.AZG_OK                                # an empty ring: nothing is launched
    assert _raw(e, None, -5) == _capi.AZG_OK                               # (n_slots is ignored without a list)
    assert _raw(e, [0], 0) == _capi.AZG_OK
    assert _code(e.selfplay_refresh_values, [0]) == _capi.AZG_E_INVALID    # (no slot is stored)
    for _ in range(3):
        e.selfplay_step()
    before = _snapshot(e, case)
    assert _raw(e, [0, 1], -1) == _capi.AZG_E_INVALID                      # a list with n_slots < 0
    for bad in ([-1], [3], [0, 3], [1, -2, 0], [4], [1 << 30]):
        assert _code(e.selfplay_refresh_values, bad) == _capi.AZG_E_INVALID, bad
    e.use_weights("target")                                                # the set in use has no weights
    assert _code(e.selfplay_refresh_values) == _capi.AZG_E_STATE
    assert _code(e.selfplay_refresh_values, [0]) == _capi.AZG_E_STATE
    e.use_weights("live")
    assert _raw(e, [0], 0) == _capi.AZG_OK                                 # an empty list: nothing is launched
    _assert_same(_snapshot(e, case), before, name)
    e.selfplay_refresh_values([2])                                         # (and the call does work on this engine)
    after = _snapshot(e, case)
    _assert_same(after, before, name, but=("value",))
    assert (after["value"][2] != before["value"][2]).any() and (after["value"][:2] == before["value"][:2]).all()
    e.close()
    # a net without weights in the live set: refused although nothing is stored yet
    e = _hip()(**dict(case.kw, n_trees=case.games))
    if case.nets > 1:
        e.set_population(case.nets)
        e.set_net_weights(0, case.desc(), case.blob(0))
    R.begin(e, case, 4, keep=False)
    e.selfplay_keep_transitions(True)
    assert _code(e.selfplay_refresh_values) == _capi.AZG_E_STATE
    e.close()


# ------------------------------------------------------------------------------------------------ the Python layer

EKW = dict(env_id=0, mode=0, n_sims=8, c_uct=1.5, gamma=0.97, num_actions=2, seed=21)
SP_KW = dict(game="CartPole-v0", n_rollouts=8, c_uct=1.5, gamma=0.97, max_episode_length=4, seed=21)
POP_GAMMAS = (1.0, 0.97, 0.5)
SP_T, SP_CAP, SP_STEPS = 11, 4, 6   # 3 nets x 11 games; the FIFO ring of 4 steps has wrapped after 6


def _policies(n, first_seed=80, device=None):
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    nets = []
    for s in range(n):
        torch.manual_seed(first_seed + s)
        net = make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2)
        nets.append(net if device is None else net.to(device))
    return nets


def _policy_truth(sp, nets):
    """float64 [size, G]: the oracle's value of the stored observations under the torch policies ``nets``."""
    size = sp.engine.selfplay_ring()[0]
    rows = sp.engine.selfplay_rows(clear=False).reshape(size, sp.n_games, -1)
    obs = np.ascontiguousarray(rows[:, :, :4])
    desc = _capi.policy_blob(nets[0])[0]
    blobs = [_capi.policy_blob(n)[1] for n in nets]
    return V.net_values(obs, sp.games_per_net, V.oracle_evaluator([EKW] * len(nets), desc, blobs))


def _columns(sp):
    size = sp.engine.selfplay_ring()[0]
    tr = {k: v.reshape(size, sp.n_games) for k, v in sp.engine.selfplay_transitions().items()}
    z = sp.engine.selfplay_rows(clear=False)[:, -1].reshape(size, sp.n_games)
    return tr, z


def _population_selfplay(nets, **kw):
    from alphazero_gym_amd import run
    settings = [dict(c_uct=1.5, gamma=g, epsilon=0.0, c_pw=1.0, kappa=0.5) for g in POP_GAMMAS]
    sp = run.PopulationSelfPlay(nets, games_per_net=SP_T, capacity_steps=SP_CAP, fifo=True, net_settings=settings, **SP_KW, **kw)
    sp.play(SP_STEPS)
    return sp


def test_refresh_values_ends_with_the_creation_time_rule():
    """sp.refresh_values(): the kept values are the truth and V_target is the n-step return over them, with each net's own gamma, for
    n_step 0, 1, 3, 1000; created with per-net rule lists: the lambda-return of lambda_util's builder."""
    nets = _policies(3)
    held, _ = N.ring_layout(SP_CAP, True, SP_STEPS)
    gam = np.repeat(np.asarray(POP_GAMMAS), SP_T)
    sp = _population_selfplay(nets, n_step=3)
    truth = _policy_truth(sp, nets)
    old, _ = _columns(sp)
    for n in N.N_STEPS:
        sp.n_step = n
        assert sp.refresh_values() == list(range(SP_CAP))
        tr, z = _columns(sp)
        np.testing.assert_array_equal(V.bits64(tr["value"]), V.bits64(truth), err_msg=f"n_step {n}")
        want = V.slot_targets(tr["reward"], truth, tr["end"], held, lambda r, v, e: N.nstep_returns(r, v, e, n, gam))
        np.testing.assert_array_equal(V.bits32(z), V.bits32(want), err_msg=f"n_step {n}")
        if n == 3:   # (one gamma for all, or the search values, would not have passed)
            one = V.slot_targets(tr["reward"], truth, tr["end"], held, lambda r, v, e: N.nstep_returns(r, v, e, n, 0.97))
            stale = V.slot_targets(tr["reward"], old["value"], tr["end"], held, lambda r, v, e: N.nstep_returns(r, v, e, n, gam))
            assert (V.bits32(one) != V.bits32(want)).any() and (V.bits32(stale) != V.bits32(want)).mean() >= MIN_CHANGED
    for k in KEPT:
        np.testing.assert_array_equal(tr[k], old[k])
    assert (tr["end"] == N.END_LENGTH).any()
    sp.close()
    rule = dict(n_step=[3, 1, 2], td_lambda=[0.5, 0.9, 1.0], target_gamma=[None, 0.9, None])
    sp = _population_selfplay(nets, **rule)
    assert sp.refresh_values(slots=range(SP_CAP)) == list(range(SP_CAP))
    tr, z = _columns(sp)
    np.testing.assert_array_equal(V.bits64(tr["value"]), V.bits64(truth))
    per = lambda xs: np.repeat(np.asarray(xs), SP_T)
    lam_gamma = per([POP_GAMMAS[0], 0.9, POP_GAMMAS[2]])
    want = V.slot_targets(tr["reward"], truth, tr["end"], held,
                          lambda r, v, e: L.lambda_returns(r, v, e, per(rule["n_step"]), per(rule["td_lambda"]), lam_gamma))
    np.testing.assert_array_equal(V.bits32(z), V.bits32(want))
    sp.close()
    from alphazero_gym_amd import run
    off = run.PopulationSelfPlay(nets, games_per_net=SP_T, capacity_steps=SP_CAP, **SP_KW)
    off.play(2)
    with pytest.raises(RuntimeError, match="n_step"):
        off.refresh_values()
    off.close()
    one = run.DeviceSelfPlay(nets[0], n_games=SP_T, n_step=2, capacity_steps=SP_CAP, fifo=True, **SP_KW)   # (DeviceSelfPlay inherits it)
    one.play(SP_STEPS)
    assert one.refresh_values([3, 0]) == [3, 0]
    tr, z = _columns(one)
    t1 = _policy_truth(one, nets[:1])
    np.testing.assert_array_equal(V.bits64(tr["value"][[0, 3]]), V.bits64(t1[[0, 3]]))
    assert (V.bits64(tr["value"][[1, 2]]) != V.bits64(t1[[1, 2]])).mean() >= MIN_CHANGED
    want = V.slot_targets(tr["reward"], tr["value"], tr["end"], held, lambda r, v, e: N.nstep_returns(r, v, e, 2, 0.97))
    np.testing.assert_array_equal(V.bits32(z), V.bits32(want))
    one.close()


def test_refresh_values_with_the_target_weights():
    import torch
    dev = torch.device("cuda", 0)
    live, other = _policies(3, 80, dev), _policies(3, 90, dev)
    sp = _population_selfplay(live, n_step=3)
    held, _ = N.ring_layout(SP_CAP, True, SP_STEPS)
    gam = np.repeat(np.asarray(POP_GAMMAS), SP_T)
    before, z0 = _columns(sp)
    with pytest.raises(RuntimeError, match="upload_target_flat"):
        sp.refresh_values(nets="target")
    now, z = _columns(sp)
    np.testing.assert_array_equal(V.bits64(now["value"]), V.bits64(before["value"]))   # (nothing was written)
    np.testing.assert_array_equal(V.bits32(z), V.bits32(z0))
    desc = _capi.policy_blob(other[0])[0]
    sp.upload_target_flat(desc, torch.from_numpy(np.stack([_capi.policy_blob(n)[1] for n in other])).to(dev))
    t_live, t_target = _policy_truth(sp, live), _policy_truth(sp, other)
    assert (V.bits64(t_live) != V.bits64(t_target)).mean() >= MIN_CHANGED
    assert sp.refresh_values(nets="target") == list(range(SP_CAP))
    assert sp.engine.weights_info() == {"in_use": "live", "target_ready": True}
    tr, z = _columns(sp)
    np.testing.assert_array_equal(V.bits64(tr["value"]), V.bits64(t_target))
    want = V.slot_targets(tr["reward"], t_target, tr["end"], held, lambda r, v, e: N.nstep_returns(r, v, e, 3, gam))
    np.testing.assert_array_equal(V.bits32(z), V.bits32(want))
    sp.refresh_values([1])   # (live again)
    tr, _ = _columns(sp)
    np.testing.assert_array_equal(V.bits64(tr["value"]), V.bits64(V.refreshed(t_target, t_live, [1])))
    sp.close()


def test_the_population_example_refreshes_with_the_target_set(monkeypatch):
    """examples/population_selfplay_train.py end to end at toy size with --refresh-values-every 1 --refresh-target; without the new flags
    the loop never reaches the call."""
    import importlib
    import os
    import sys
    from alphazero_gym_amd import run
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module("population_selfplay_train")
    base = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4", "--n-step", "3",
            "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5", "--device", "cuda", "--seeds", "0", "1",
            "--games-per-seed", "8", "--trainer", "device-epoch", "--ema-decay", "0.9"]
    calls = []
    real = run.PopulationSelfPlay.refresh_values

    def recording(self, *a, **kw):
        calls.append((self.engine.selfplay_ring()[0], kw))
        used = real(self, *a, **kw)
        assert self.engine.weights_info()["in_use"] == "live"
        return used
    monkeypatch.setattr(run.PopulationSelfPlay, "refresh_values", recording)
    hist = mod.train(mod.parse_args(base + ["--refresh-values-every", "1", "--refresh-target"]), log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    assert calls == [(2, {"nets": "target"}), (4, {"nets": "target"}), (4, {"nets": "target"})]
    calls.clear()
    every2 = mod.train(mod.parse_args(base + ["--refresh-values-every", "2"]), log=None)
    assert calls == [(4, {})] and len(every2) == 3
    calls.clear()
    plain = mod.train(mod.parse_args(base), log=None)
    again = mod.train(mod.parse_args(base + ["--refresh-values-every", "0"]), log=None)
    assert calls == []
    for h, g in zip(plain, again):
        assert (h["loss"], h["mean_return"], h["episodes_finished"]) == (g["loss"], g["mean_return"], g["episodes_finished"])
    assert [h["loss"] for h in plain] != [h["loss"] for h in hist]   # (the refreshed targets do reach the trainer)
