"""Lambda-return value targets for the device replay ring (azg_selfplay_lambda_targets / _nets, run.PopulationSelfPlay
td_lambda=... and per-net lists) on the GPU: the V_target column against the numpy fold, device against device at the rule's edges,
a rule per net, growth, clears, reanalysed values, the refusals and the Python layer.  Everything is compared bit for bit.  Engines,
rings and sizes: tests/nstep_util.py; the truth: tests/lambda_util.py."""
import ctypes as C

import numpy as np
import pytest

import lambda_util as LU
import nstep_util as N
import priority_util as P
import reanalyse_util as R
from alphazero_gym_amd import _capi

TR_KEYS = ("reward", "value", "action", "end")
POP_RULES = [(0, 0.5, None), (3, 0.9, 0.9), (1000, 0.3, None)]   # (n_step, lambda, gamma) of the population case's three nets


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


def _column(e, case):
    return R.bits32(R.ring(e, case)[:, :, -1])


def _transitions(e, case):
    return {k: v.reshape(-1, case.games).copy() for k, v in e.selfplay_transitions().items()}


def _assert_transitions(got, want, what=""):
    for k in TR_KEYS:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        view = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view), err_msg=f"{what}: {k}")


def _gamma(case, gamma):
    return N.search_gamma(case) if gamma is None else gamma


def _want(ref, held, n, lam, gamma):
    return R.bits32(LU.ring_lambda_targets(ref["reward"], ref["value"], ref["end"], held, n, lam, gamma))


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_column_is_the_fold_and_nothing_else_is_written(name, capacity, fifo):
    """For lambda in {0, 0.5, 0.95, 1}, n_step in {0, 1, 3, 1000}, the search's gamma (per net in the population) and 0.9: the V_target
    column is the truth; every other column, every unused slot and the kept transitions are unchanged; a second call changes nothing."""
    steps = N.STEPS[name]
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    held, _ = N.ring_layout(capacity, fifo, steps)
    before = _whole_ring(e, case)
    assert before.shape[0] == capacity
    tr = _transitions(e, case)
    for gamma in N.GAMMAS:
        for n in N.N_STEPS:
            for lam in LU.LAMBDAS:
                what = f"{name} n_step {n} lambda {lam} gamma {gamma}"
                e.selfplay_lambda_targets(n, lam, gamma)
                got = _whole_ring(e, case)
                np.testing.assert_array_equal(got[:len(held), :, -1], _want(ref, held, n, lam, _gamma(case, gamma)), err_msg=what)
                np.testing.assert_array_equal(got[:, :, :-1], before[:, :, :-1], err_msg=what)
                np.testing.assert_array_equal(got[len(held):], before[len(held):], err_msg=what)
                if n == 0:
                    np.testing.assert_array_equal(got, before, err_msg=what)
                e.selfplay_lambda_targets(n, lam, gamma)
                np.testing.assert_array_equal(_whole_ring(e, case), got, err_msg=what + " (second call)")
    _assert_transitions(_transitions(e, case), tr, name)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_edges_leave_the_bits_of_the_nstep_call(name, capacity, fifo):
    """Device against device on one ring: lambda 1 leaves what selfplay_nstep_targets(n) leaves, lambda 0 what
    selfplay_nstep_targets(1) leaves, and n_step 1 the same column for lambda 0.3 and 0.9."""
    case, e = _engine(name, capacity, fifo, N.STEPS[name])
    for gamma in N.GAMMAS:
        e.selfplay_nstep_targets(1, gamma)
        one = _whole_ring(e, case)
        for n in N.N_STEPS:
            what = f"{name} n_step {n} gamma {gamma}"
            e.selfplay_nstep_targets(n, gamma)
            nstep = _whole_ring(e, case)
            e.selfplay_lambda_targets(n, 1.0, gamma)
            np.testing.assert_array_equal(_whole_ring(e, case), nstep, err_msg=what + " lambda 1")
            if n >= 1:
                e.selfplay_lambda_targets(n, 0.0, gamma)
                np.testing.assert_array_equal(_whole_ring(e, case), one, err_msg=what + " lambda 0")
        for lam in (0.3, 0.9):
            e.selfplay_nstep_targets(0, gamma)
            e.selfplay_lambda_targets(1, lam, gamma)
            np.testing.assert_array_equal(_whole_ring(e, case), one, err_msg=f"{name} n_step 1 lambda {lam}")
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_share_of_rows_apart_from_both_nstep_columns(name, capacity, fifo):
    """At lambda 0.5 and n_step 3 at least 0.4 of all stored rows differ in bits from both the n-step and the 1-step column the device
    itself writes: a lambda call that wrote either of those could not have passed the comparison with the truth.  (The truth's own
    share: 0.727 / 0.816 CartPole fifo / stop, 0.583 Pendulum, 0.429 many_children and wide, 0.600 population.)"""
    case, e = _engine(name, capacity, fifo, N.STEPS[name])
    e.selfplay_nstep_targets(3)
    nstep = _column(e, case)
    e.selfplay_nstep_targets(1)
    one = _column(e, case)
    e.selfplay_lambda_targets(3, 0.5)
    lam = _column(e, case)
    share = float(((lam != nstep) & (lam != one)).mean())
    print(f"{name} capacity {capacity}: share {share:.3f}")
    assert share >= LU.MIN_SHARE, (name, share)
    e.close()


def _pop_truth(ref, held, case, rules):
    """The population ring's column under one rule per net."""
    T = case.T
    n = np.repeat([r[0] for r in rules], T)
    lam = np.repeat([r[1] for r in rules], T)
    own = N.search_gamma(case)
    gamma = np.concatenate([own[k * T:(k + 1) * T] if r[2] is None else np.full(T, r[2]) for k, r in enumerate(rules)])
    return _want(ref, held, n, lam, gamma)


@pytest.mark.gpu
def test_every_net_follows_its_own_rule():
    """The population of 3 nets x 11 games with the rules (0, 0.5, search gamma), (3, 0.9, 0.9), (1000, 0.3, search gamma): net k's games
    carry the bits of the one-rule call with entry k -- device against device and against the truth --, the other columns stay, and
    three equal entries are the one-rule call."""
    name, capacity, fifo = "population", N.STEPS["population"] + 1, False
    steps = N.STEPS[name]
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    held, _ = N.ring_layout(capacity, fifo, steps)
    T = case.T
    assert case.nets == 3 and len(set(N.POP_GAMMAS)) == 3
    before = _whole_ring(e, case)
    single = []
    for n, lam, gamma in POP_RULES:
        e.selfplay_lambda_targets(n, lam, gamma)
        single.append(_whole_ring(e, case))
    n, lam, gamma = zip(*POP_RULES)
    e.selfplay_lambda_targets(list(n), list(lam), list(gamma))
    got = _whole_ring(e, case)
    for k in range(3):
        np.testing.assert_array_equal(got[:, k * T:(k + 1) * T], single[k][:, k * T:(k + 1) * T], err_msg=f"net {k}")
    np.testing.assert_array_equal(got[:len(held), :, -1], _pop_truth(ref, held, case, POP_RULES))
    np.testing.assert_array_equal(got[:, :, :-1], before[:, :, :-1])
    np.testing.assert_array_equal(got[len(held):], before[len(held):])
    # (the rules differ where it shows: every net's part differs from what another net's rule leaves there)
    for k in range(3):
        assert (got[:len(held), k * T:(k + 1) * T, -1] != single[(k + 1) % 3][:len(held), k * T:(k + 1) * T, -1]).any(), k
    # one scalar beside lists goes to every net; all gammas None: the flag, every net its search's gamma
    e.selfplay_lambda_targets(3, [0.5, 0.9, 0.3])
    np.testing.assert_array_equal(_column(e, case), _pop_truth(ref, held, case, [(3, 0.5, None), (3, 0.9, None), (3, 0.3, None)]))
    for rule in POP_RULES:
        e.selfplay_lambda_targets(*rule)
        one = _whole_ring(e, case)
        e.selfplay_nstep_targets(0)
        e.selfplay_lambda_targets([rule[0]] * 3, [rule[1]] * 3, [rule[2]] * 3)
        np.testing.assert_array_equal(_whole_ring(e, case), one, err_msg=str(rule))
    with pytest.raises(ValueError, match="one per net"):
        e.selfplay_lambda_targets([1, 2], 0.5)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_three_more_steps_and_another_call_give_the_longer_runs_targets(name, capacity, fifo):
    steps = N.STEPS[name] if fifo else min(N.STEPS[name], capacity - 3)
    ref = N.reference(name)
    case, e = _engine(name, capacity, fifo, steps)
    g = N.search_gamma(case)
    e.selfplay_lambda_targets(3, 0.5)
    first = R.ring(e, case).copy()
    held0, _ = N.ring_layout(capacity, fifo, steps)
    np.testing.assert_array_equal(R.bits32(first[:, :, -1]), _want(ref, held0, 3, 0.5, g))
    for _ in range(3):
        e.selfplay_step()
    e.selfplay_lambda_targets(3, 0.5)
    held, _ = N.ring_layout(capacity, fifo, steps + 3)
    got = R.ring(e, case)
    np.testing.assert_array_equal(R.bits32(got[:, :, -1]), _want(ref, held, 3, 0.5, g))
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
    g = N.search_gamma(case)
    e.selfplay_lambda_targets(1000, 0.5)
    rows = e.selfplay_rows(clear=True).reshape(5, case.games, -1)
    np.testing.assert_array_equal(R.bits32(rows[:, :, -1]), _want(ref, np.arange(5), 1000, 0.5, g))
    e.selfplay_lambda_targets(1000, 0.5)   # (an empty ring: nothing to do)
    for _ in range(4):
        e.selfplay_step()
    held = np.arange(5, 9)
    for n in (2, 1000):
        e.selfplay_lambda_targets(n, 0.5)
        got = R.ring(e, case)
        np.testing.assert_array_equal(R.bits32(got[:, :, -1]), _want(ref, held, n, 0.5, g))
        np.testing.assert_array_equal(R.bits32(got[:, :, :-1]), R.bits32(ref["rows"][held][:, :, :-1]))
    # (had the first ring seen the later steps, its windows would differ wherever step 4 did not end an episode: the test can tell)
    across = _want(ref, np.arange(9), 1000, 0.5, g)
    open_at_4 = ref["end"][4] == N.END_NONE
    assert (across[:5] != R.bits32(rows[:, :, -1]))[:, open_at_4].any() == open_at_4.any()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(N.CASES))
def test_reanalysed_values_feed_the_targets(name):
    """With the states kept as well: new weights, two slots reanalysed, then the calls.  The kept float64 values of the reanalysed rows
    are the fresh search's (the oracle's), and every V_target follows from the mixed old and new values -- also where a refreshed value
    enters as v_{i+1} of an older row's fold."""
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
    np.testing.assert_array_equal(R.bits64(_transitions(e, case)["value"]), R.bits64(value))
    held = np.arange(steps)
    for n, lam, gamma in ((3, 0.5, None), (1000, 0.95, 0.9), (1, 0.5, 0.9), (0, 0.5, None)):
        e.selfplay_lambda_targets(n, lam, gamma)
        got = R.ring(e, case)
        np.testing.assert_array_equal(R.bits32(got[:, :, :-1]), R.bits32(want_rows[:, :, :-1]))
        want = LU.ring_lambda_targets(ref["reward"][:steps], value, ref["end"][:steps], held, n, lam, _gamma(case, gamma))
        np.testing.assert_array_equal(R.bits32(got[:, :, -1]), R.bits32(want), err_msg=f"{name} n_step {n} lambda {lam} gamma {gamma}")
    stale = LU.ring_lambda_targets(ref["reward"][:steps], ref["value"][:steps], ref["end"][:steps], held, 3, 0.5, N.search_gamma(case))
    fresh = LU.ring_lambda_targets(ref["reward"][:steps], value, ref["end"][:steps], held, 3, 0.5, N.search_gamma(case))
    assert (R.bits32(stale) != R.bits32(fresh)).any()   # (the old values would not have passed)
    e.close()


def _rule(struct_size=None, n_step=1, lam=0.5, gamma=0.9, flags=0):
    c = _capi.AzgReturnRule()
    c.struct_size = C.sizeof(_capi.AzgReturnRule) if struct_size is None else struct_size
    c.n_step, c.lambda_, c.gamma, c.flags = n_step, lam, gamma, flags
    return c


def _raw(e, **kw):
    return e._f["selfplay_lambda_targets"](e._h, C.byref(_rule(**kw)))


def _raw_nets(e, rules):
    arr = (_capi.AzgReturnRule * len(rules))(*rules)
    rc = e._f["selfplay_lambda_targets_nets"](e._h, arr)
    return rc, (e._f["last_error"](e._h) or b"").decode()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_refusals_leave_the_ring_alone(name):
    case = N.CASES[name]
    K = case.nets
    size = C.sizeof(_capi.AzgReturnRule)
    e = R.make_engine(_hip(), case)
    assert _code(e.selfplay_lambda_targets, 1, 0.5) == _capi.AZG_E_STATE             # no begin
    assert _code(e.selfplay_lambda_targets, [1] * K, 0.5) == _capi.AZG_E_STATE
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    before = _whole_ring(e, case)
    assert _code(e.selfplay_lambda_targets, 1, 0.5) == _capi.AZG_E_STATE             # no keep_transitions
    assert _code(e.selfplay_lambda_targets, [1] * K, 0.5) == _capi.AZG_E_STATE
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    e.selfplay_clear()
    e.selfplay_keep_transitions(True)
    assert _raw(e) == _capi.AZG_OK                                                   # an empty ring: nothing is launched
    assert _raw_nets(e, [_rule()] * K)[0] == _capi.AZG_OK
    for _ in range(2):
        e.selfplay_step()
    before = _whole_ring(e, case)
    tr = _transitions(e, case)
    bad = [dict(struct_size=size - 4), dict(struct_size=0), dict(n_step=-1), dict(n_step=-1, flags=_capi.NSTEP_SEARCH_GAMMA), dict(flags=2),
           dict(flags=3), dict(lam=float("nan")), dict(lam=-1e-9), dict(lam=1.0 + 1e-9), dict(lam=float("inf")),
           dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=-float("inf"))]
    for kw in bad:
        assert _raw(e, **kw) == _capi.AZG_E_INVALID, kw
        for k in range(K):   # (the per-net form checks every entry, not the first alone)
            rules = [_rule() for _ in range(K)]
            rules[k] = _rule(**kw)
            rc, msg = _raw_nets(e, rules)
            assert rc == _capi.AZG_E_INVALID, (kw, k)
            if k >= 1 and ("struct_size" in kw or "flags" in kw):   # an entry that differs from entry 0: the field and the net are named
                assert ("struct_size" if "struct_size" in kw else "flags") + f" of net {k}" in msg, msg
    assert e._f["selfplay_lambda_targets"](e._h, None) == _capi.AZG_E_INVALID         # a NULL rule
    assert e._f["selfplay_lambda_targets_nets"](e._h, None) == _capi.AZG_E_INVALID
    if K > 1:   # valid entries that differ in their flags
        rules = [_rule(flags=_capi.NSTEP_SEARCH_GAMMA)] + [_rule() for _ in range(K - 1)]
        rc, msg = _raw_nets(e, rules)
        assert rc == _capi.AZG_E_INVALID and "flags of net 1" in msg, msg
    for lam in (-0.5, 1.5, float("nan")):
        assert _code(e.selfplay_lambda_targets, 1, lam) == _capi.AZG_E_INVALID
    assert _code(e.selfplay_lambda_targets, -1, 0.5) == _capi.AZG_E_INVALID
    assert _code(e.selfplay_lambda_targets, 1, 0.5, -0.5) == _capi.AZG_E_INVALID
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    _assert_transitions(_transitions(e, case), tr, name)
    assert _raw(e, n_step=0, gamma=float("nan"), flags=_capi.NSTEP_SEARCH_GAMMA) == _capi.AZG_OK   # (the flag: gamma is not read)
    np.testing.assert_array_equal(_whole_ring(e, case), before)
    for lam in (0.0, 1.0):                                                            # (the ends of the range are values like any other)
        assert _raw(e, n_step=2, lam=lam, gamma=0.0) == _capi.AZG_OK
    got = R.ring(e, case)[:, :, -1]
    np.testing.assert_array_equal(R.bits32(got[0]), R.bits32(tr["reward"][0].astype(np.float32)))   # gamma 0: the reward alone
    R.begin(e, case, 4, keep=False)                                                   # the next begin drops the kept transitions
    e.selfplay_step()
    assert _code(e.selfplay_lambda_targets, 1, 0.5) == _capi.AZG_E_STATE
    e.close()


def _policies(n):
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    nets = []
    for s in range(n):
        torch.manual_seed(80 + s)
        nets.append(make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2))
    return nets


SP_KW = dict(game="CartPole-v0", n_rollouts=8, c_uct=1.5, gamma=0.97, max_episode_length=4, seed=21)


def _spy(sp):
    """Counts the calls of this object's engine into the three target entry points."""
    calls = {"selfplay_nstep_targets": 0, "selfplay_lambda_targets": 0, "selfplay_lambda_targets_nets": 0}
    fns = dict(sp.engine._f)
    for key in calls:
        def counted(*a, _fn=fns[key], _key=key):
            calls[_key] += 1
            return _fn(*a)
        fns[key] = counted
    sp.engine._f = fns
    return calls


def _truth_of(sp, steps, n, lam, gamma):
    """(the kept transitions [steps, G], the truth's column over them)"""
    G = sp.n_games
    tr = {k: v.reshape(steps, G) for k, v in sp.engine.selfplay_transitions().items()}
    return tr, LU.ring_lambda_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), n, lam, gamma)


def _col(sp, steps):
    return R.bits32(sp.engine.selfplay_rows(clear=False)[:, -1].reshape(steps, sp.n_games))


@pytest.mark.gpu
def test_python_layer_ends_play_and_reanalyse_with_the_lambda_column():
    """run.PopulationSelfPlay(td_lambda=0.8, n_step=3): play() and reanalyse() end with the lambda column (one-rule call);
    td_lambda=None leaves today's bits through today's call; lists reach the per-net call, a list without td_lambda meaning lambda 1;
    lambda_targets() can be called by hand; DeviceSelfPlay inherits it."""
    import torch
    from alphazero_gym_amd import run
    T, steps = 11, 6
    G = 2 * T
    nets = _policies(2)
    sp = run.PopulationSelfPlay(nets, games_per_net=T, n_step=3, td_lambda=0.8, reanalyse=True, capacity_steps=steps, **SP_KW)
    calls = _spy(sp)
    sp.play(steps)
    tr, want = _truth_of(sp, steps, 3, 0.8, 0.97)
    assert (tr["end"] == N.END_LENGTH).any()
    np.testing.assert_array_equal(_col(sp, steps), R.bits32(want))
    assert calls == {"selfplay_nstep_targets": 0, "selfplay_lambda_targets": 1, "selfplay_lambda_targets_nets": 0}
    nstep3 = N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), 3, 0.97)
    assert (R.bits32(want) != R.bits32(nstep3)).any()   # (every row whose window holds two steps or more: today's column would not pass)
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.mul_(1.5)
    old = tr["value"].copy()
    assert sp.reanalyse(slots=[1, 3]) == [1, 3]
    tr, want = _truth_of(sp, steps, 3, 0.8, 0.97)
    assert (R.bits64(tr["value"]) != R.bits64(old)).any(axis=1).tolist() == [False, True, False, True, False, False]
    np.testing.assert_array_equal(_col(sp, steps), R.bits32(want))
    assert calls["selfplay_lambda_targets"] == 2 and calls["selfplay_nstep_targets"] == 0
    sp.lambda_targets(n_step=[1, 1000], td_lambda=[0.3, 0.9], gamma=[None, 0.9])      # by hand, per net
    want = LU.ring_lambda_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), np.repeat([1, 1000], T), np.repeat([0.3, 0.9], T),
                                  np.repeat([0.97, 0.9], T))
    np.testing.assert_array_equal(_col(sp, steps), R.bits32(want))
    assert calls["selfplay_lambda_targets_nets"] == 1
    sp.nstep_targets()                                                                # (still there, still today's call)
    np.testing.assert_array_equal(_col(sp, steps), R.bits32(N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), 3, 0.97)))
    assert calls["selfplay_nstep_targets"] == 1
    sp.close()

    off = run.PopulationSelfPlay(_policies(2), games_per_net=T, n_step=3, capacity_steps=steps, **SP_KW)   # td_lambda=None: today's
    calls = _spy(off)
    off.play(steps)
    tr, _ = _truth_of(off, steps, 3, 1.0, 0.97)
    np.testing.assert_array_equal(_col(off, steps), R.bits32(N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), 3, 0.97)))
    assert calls == {"selfplay_nstep_targets": 1, "selfplay_lambda_targets": 0, "selfplay_lambda_targets_nets": 0}
    off.close()

    per = run.PopulationSelfPlay(_policies(2), games_per_net=T, n_step=[1, 1000], td_lambda=[0.3, 0.9], target_gamma=[None, 0.9],
                                 capacity_steps=steps, **SP_KW)
    calls = _spy(per)
    per.play(steps)
    _, want = _truth_of(per, steps, np.repeat([1, 1000], T), np.repeat([0.3, 0.9], T), np.repeat([0.97, 0.9], T))
    np.testing.assert_array_equal(_col(per, steps), R.bits32(want))
    assert calls == {"selfplay_nstep_targets": 0, "selfplay_lambda_targets": 0, "selfplay_lambda_targets_nets": 1}
    with pytest.raises(ValueError, match="lambda_targets"):
        per.nstep_targets()
    per.close()

    lists = run.PopulationSelfPlay(_policies(2), games_per_net=T, n_step=[1, 3], capacity_steps=steps, **SP_KW)   # no td_lambda: lambda 1
    calls = _spy(lists)
    lists.play(steps)
    tr, _ = _truth_of(lists, steps, 1, 1.0, 0.97)
    for k, n in enumerate((1, 3)):
        want = N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), n, 0.97)
        np.testing.assert_array_equal(_col(lists, steps)[:, k * T:(k + 1) * T], R.bits32(want)[:, k * T:(k + 1) * T])
    assert calls["selfplay_lambda_targets_nets"] == 1 and calls["selfplay_nstep_targets"] == 0
    lists.close()

    one = run.DeviceSelfPlay(_policies(1)[0], n_games=T, n_step=3, td_lambda=0.5, target_gamma=0.9, capacity_steps=steps, **SP_KW)
    one.play(steps)
    _, want = _truth_of(one, steps, 3, 0.5, 0.9)
    np.testing.assert_array_equal(_col(one, steps), R.bits32(want))
    np.testing.assert_array_equal(R.bits32(one.collect(0).numpy().reshape(steps, T, -1)[:, :, -1]), R.bits32(want))   # (the rows handed out)
    one.close()
    none = run.DeviceSelfPlay(_policies(1)[0], n_games=T, capacity_steps=steps, **SP_KW)
    with pytest.raises(RuntimeError, match="n_step"):
        none.lambda_targets()
    none.close()


@pytest.mark.gpu
def test_priorities_follow_the_lambda_targets():
    """With prioritized=: priorities() after the lambda targets are priority_util's truth fed with the truth's lambda column."""
    from alphazero_gym_amd import run
    T, steps = 11, 6
    sp = run.PopulationSelfPlay(_policies(2), games_per_net=T, n_step=3, td_lambda=0.8, prioritized={"alpha": 0.6, "eps": 1e-3},
                                capacity_steps=steps, **SP_KW)
    sp.play(steps)
    sp.priorities()
    q = sp.engine.selfplay_priority_values().reshape(steps, 2 * T)
    tr, z = _truth_of(sp, steps, 3, 0.8, 0.97)
    np.testing.assert_array_equal(q, P.priorities(P.gap(tr["value"], z), 0.6, 1e-3))
    z3 = N.ring_targets(tr["reward"], tr["value"], tr["end"], np.arange(steps), 3, 0.97)
    assert (q != P.priorities(P.gap(tr["value"], z3), 0.6, 1e-3)).any()   # (the n-step column would not have passed)
    sp.close()


def test_value_errors_come_before_any_engine_call(monkeypatch):
    from alphazero_gym_amd import run

    def no_engine(*a, **kw):
        raise AssertionError("an engine was created")

    for cls in (run.PopulationSelfPlay, run.DeviceSelfPlay):
        monkeypatch.setattr(cls, "_search", staticmethod(no_engine))
    nets = _policies(2)
    kw = dict(games_per_net=4, capacity_steps=4, **SP_KW)
    for bad, match in ((dict(td_lambda=0.5), "n_step"), (dict(td_lambda=[0.5, 0.5]), "n_step"), (dict(target_gamma=[0.9, 0.9]), "n_step"),
                       (dict(n_step=3, td_lambda=[0.5]), "one per net"), (dict(n_step=[1, 2, 3]), "one per net"),
                       (dict(n_step=3, target_gamma=[0.9] * 3), "one per net"),
                       (dict(n_step=3, td_lambda=1.5), r"\[0, 1\]"), (dict(n_step=3, td_lambda=-0.1), r"\[0, 1\]"),
                       (dict(n_step=3, td_lambda=float("nan")), r"\[0, 1\]"), (dict(n_step=3, td_lambda=[0.5, 2.0]), r"\[0, 1\]"),
                       (dict(n_step=[3, -1]), "n_step"), (dict(n_step=[3, -1], td_lambda=0.5), "n_step")):
        with pytest.raises(ValueError, match=match):
            run.PopulationSelfPlay(nets, **kw, **bad)
    with pytest.raises(ValueError, match="n_step"):
        run.DeviceSelfPlay(nets[0], n_games=4, capacity_steps=4, td_lambda=0.5, **SP_KW)
    with pytest.raises(AssertionError, match="an engine was created"):   # (a valid rule goes on to build its engine)
        run.PopulationSelfPlay(nets, n_step=[1, 3], td_lambda=0.5, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("example,extra", [
    ("selfplay_train", ["--games", "16", "--n-step", "5", "--td-lambda", "0.9"]),
    ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch", "--n-step", "5", "--td-lambda", "0.9"]),
    ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch", "--n-steps", "1", "5",
                                   "--td-lambdas", "0.5", "1.0"])], ids=["one", "population", "per-seed"])
def test_examples_train_on_lambda_targets(example, extra):
    """--n-step 5 --td-lambda 0.9, and per-seed lists in the population example, with --replay-steps 4 --reanalyse-slots 1: the FIFO ring
    wraps, and the loop trains on finite targets."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module(example)
    a = mod.parse_args(["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4",
                        "--reanalyse-slots", "1", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8",
                        "--max-episode-length", "5", "--device", "cuda"] + extra)
    assert (a.td_lambda == 0.9) != ("--td-lambdas" in extra)
    hist = mod.train(a, log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
