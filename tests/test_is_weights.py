"""Importance-sampling weights of the device replay ring on the GPU (azg_selfplay_is_weights / _is_weights_device /
_is_weight_values, include/azgym_priority.h): the weights against the numpy rule over the device's own priorities bit for bit, the
clamps and the minimum's two levels, per-net minima, what the call leaves alone, the refusals and how long the device pointer stays
valid.  Cases and sizes: tests/nstep_util.py; the truth: tests/is_weights_util.py."""
import numpy as np
import pytest

import is_weights_util as W
import nstep_util as N
import priority_util as P
import reanalyse_util as R
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

pytestmark = pytest.mark.gpu


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _engine(name, capacity, fifo, steps, transitions=True, states=False, priorities=True, case=None):
    case = N.CASES[name] if case is None else case
    e = R.make_engine(_hip(), case)
    R.begin(e, case, capacity, fifo=fifo, keep=states)
    if transitions:
        e.selfplay_keep_transitions(True)
    if priorities:
        e.selfplay_keep_priorities(True)
    for _ in range(steps):
        e.selfplay_step()
    return case, e


def _whole_ring(e, case):
    """Every slot of the replay ring, used or not: [capacity, G, row_len] as uint32."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    e.sync()
    ring = DeviceReplay(e, 1).ring.cpu().numpy()
    return np.ascontiguousarray(ring).view(np.uint32).reshape(-1, case.games, ring.shape[1]).copy()


def _books(e, case, transitions=True):
    """What the weights' calls may not move: the whole ring, the kept transitions, the priorities, the games and the ring's books."""
    tr = e.selfplay_transitions() if transitions else {}
    return dict(ring=_whole_ring(e, case), tr={k: v.copy() for k, v in tr.items()}, q=e.selfplay_priority_values().copy(),
                stats=e.selfplay_stats(), books=e.selfplay_ring())


def _assert_books(e, case, before, what=""):
    now = _books(e, case, transitions=bool(before["tr"]))
    np.testing.assert_array_equal(now["ring"], before["ring"], err_msg=what)
    for k, v in before["tr"].items():
        view = {8: np.uint64, 4: np.uint32}[v.dtype.itemsize]
        np.testing.assert_array_equal(now["tr"][k].view(view), v.view(view), err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(now["q"], before["q"], err_msg=what)
    assert_stats_bits(now["stats"], before["stats"], what)
    assert now["books"] == before["books"], what


def _q(e, case):
    return e.selfplay_priority_values().reshape(-1, case.games)


def _w(e, case):
    return e.selfplay_is_weight_values().reshape(-1, case.games)


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _assert_weights(e, case, beta, what):
    e.selfplay_is_weights(beta)
    got, q = _w(e, case), _q(e, case)
    assert got.dtype == np.float32 and got.shape == q.shape
    np.testing.assert_array_equal(W.bits(got), W.bits(W.is_weights(q, case.nets, beta)), err_msg=what)
    assert (got >= 0).all() and (got <= 1).all()
    return got, q


@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_weights_are_the_rule_and_nothing_else_is_written(name, capacity, fifo):
    """Every ring (the wrapped FIFO one, the STOP rings with an unused slot; 1 and 3 nets), alpha in {0, 0.6, 1}, beta in {0, 0.4, 1}:
    the weights are the numpy rule over the device's own q, bit for bit; alpha = 0 or beta = 0 gives ones; the ring, the transitions,
    q, the games and the books do not move."""
    case, e = _engine(name, capacity, fifo, N.STEPS[name])
    size = e.selfplay_ring()[0]
    assert size == min(capacity, N.STEPS[name])
    e.selfplay_nstep_targets(3)
    kinds = set()
    for alpha in P.ALPHAS:
        e.selfplay_priorities(alpha, P.EPS)
        before = _books(e, case)
        for beta in W.BETAS:
            got, q = _assert_weights(e, case, beta, f"{name} alpha {alpha} beta {beta}")
            T = case.T
            for k in range(case.nets):
                block = got[:, k * T:(k + 1) * T]
                assert (block == 1.0).any()                                   # (the net's minimum row)
            if alpha == 0 or beta == 0:
                assert (got == 1.0).all()
            else:
                assert len(np.unique(got)) > size                             # (the rows' weights differ: a constant would not have passed)
            kinds.add((alpha, beta))
        _assert_books(e, case, before, f"{name} alpha {alpha}")
    assert len(kinds) == 9
    e.close()


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_both_clamps_in_one_net_and_a_net_with_one_row(name):
    """AZG_PRIO_GIVEN with d = 0 and d = 1e9 at alpha = 1 puts q = 1 and q = 2^40 into every net: r = 2^-40.  Then one stored step of
    a one-game-per-net engine: one row per net, weight 1."""
    case, e = _engine(name, 4, False, 3)
    size, G, T = 3, case.games, case.T
    given = np.full((size, G), 1.0, np.float32)
    for k in range(case.nets):
        given[0, k * T] = 0.0
        given[size - 1, k * T + T - 1] = 1e9
    want_q = P.priorities(given, 1.0, 1e-9)
    assert want_q.min() == 1 and want_q.max() == P.Q_MAX                      # (the numpy rule reaches both clamps)
    e.selfplay_priorities(1.0, 1e-9, given)
    np.testing.assert_array_equal(_q(e, case), want_q)
    for beta in (0.4, 1.0, 30.0):
        got, _ = _assert_weights(e, case, beta, f"{name} clamps beta {beta}")
        for k in range(case.nets):
            assert got[0, k * T] == 1.0
            assert W.bits(got[size - 1, k * T + T - 1]) == W.bits(W.weight_rule(np.asarray([P.Q_MAX], np.uint64), 1, beta)[0])
    e.close()
    one = R.Case(case.kw, case.net, games=case.nets, max_len=case.max_len, nets=case.nets, net_settings=case.net_settings,
                 net_rollouts=case.net_rollouts)
    _, o = _engine("", 2, False, 1, case=one)
    o.selfplay_priorities(1.0, 1e-9, np.linspace(0.5, 7.0, one.games).astype(np.float32))
    assert len(np.unique(_q(o, one))) == one.games
    o.selfplay_is_weights(0.4)
    np.testing.assert_array_equal(W.bits(_w(o, one)), W.bits(np.ones((1, one.games), np.float32)))
    o.close()


@pytest.mark.parametrize("nets", [1, 3])
def test_minima_over_more_segments_than_a_wave_has_lanes(nets):
    """4101 CartPole games x 13 steps: 53313 rows in 209 segments for one net (a partial last segment, no multiple of 256, more than
    64 x 256), 17771 rows in 70 segments for each of three nets.  The least q sits in a different place per net -- the last row of the
    partial last segment for net 0 -- and the weights are the rule's."""
    base = R.CASES["cartpole"]
    case = R.Case(dict(base.kw, n_sims=2), base.net, games=4101, max_len=3, nets=nets)
    steps = 13
    _, e = _engine("", steps, False, steps, transitions=False, case=case)
    T = case.T
    assert (steps * T) % 256 != 0 and steps * T > 64 * 256
    rng = np.random.default_rng(8)
    given = (10.0 ** rng.uniform(-3.0, 7.0, size=(steps, case.games))).astype(np.float32)
    spots = [(steps - 1, T - 1), (0, 0), (5, T // 2)][:nets]
    for k, (s, j) in enumerate(spots):
        given[s, k * T + j] = 10.0 ** (-4.0 - 0.5 * k)                            # (the net's own minimum, different per net)
    e.selfplay_priorities(1.0, 1e-9, given)
    q = _q(e, case)
    np.testing.assert_array_equal(q, P.priorities(given, 1.0, 1e-9))
    mins = [int(q[:, k * T:(k + 1) * T].min()) for k in range(nets)]
    assert len(set(mins)) == nets and all(int(q[s, k * T + j]) == mins[k] for k, (s, j) in enumerate(spots))
    for beta in (0.4, 1.0):
        got, _ = _assert_weights(e, case, beta, f"{nets} nets beta {beta}")
        assert len(np.unique(got)) > 10000
        for k, (s, j) in enumerate(spots):
            block = got[:, k * T:(k + 1) * T]
            assert block[s, j] == 1.0 and (block == 1.0).sum() == 1
    e.close()


def test_a_nets_weights_are_those_of_a_one_net_engine_at_its_rank():
    """Net k of the 3-net engine against an engine of that net alone given net k's columns of the same d: the same q, hence the same
    weights.  Every net's least d is planted and differs from the others', so a minimum over the whole ring would show."""
    name = "population"
    case, e = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name])
    size, T = e.selfplay_ring()[0], case.T
    rng = np.random.default_rng(12)
    given = (10.0 ** rng.uniform(-2.0, 2.0, size=(size, case.games))).astype(np.float32)
    for k in range(case.nets):
        given[(3 * k + 1) % size, k * T + (5 * k) % T] = 10.0 ** (-3.0 - k)
    e.selfplay_priorities(0.6, P.EPS, given)
    q = _q(e, case)
    e.selfplay_is_weights(0.4)
    w = _w(e, case).copy()
    e.close()
    assert len({int(q[:, k * T:(k + 1) * T].min()) for k in range(case.nets)}) == case.nets
    np.testing.assert_array_equal(W.bits(w), W.bits(W.is_weights(q, case.nets, 0.4)))
    assert (W.bits(w) != W.bits(W.is_weights(q, 1, 0.4))).any()              # (one minimum for the whole ring is another answer)
    for k in range(case.nets):
        one = R.Case(case.net_kw(k), case.net, games=T, max_len=case.max_len)
        one._blob = lambda j, new, k=k: case.blob(k, new)
        _, o = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name], case=one)
        o.selfplay_priorities(0.6, P.EPS, np.ascontiguousarray(given[:, k * T:(k + 1) * T]))
        np.testing.assert_array_equal(_q(o, one), q[:, k * T:(k + 1) * T], err_msg=f"net {k}")
        o.selfplay_is_weights(0.4)
        np.testing.assert_array_equal(W.bits(_w(o, one)), W.bits(w[:, k * T:(k + 1) * T]), err_msg=f"net {k}")
        o.close()


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_refusals_leave_the_weights_alone(name):
    case = N.CASES[name]
    G = case.games
    STATE, INVALID = _capi.AZG_E_STATE, _capi.AZG_E_INVALID
    e = R.make_engine(_hip(), case)
    for fn, args in ((e.selfplay_is_weights, (0.4,)), (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        assert _code(fn, *args) == STATE                                      # no begin
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    for fn, args in ((e.selfplay_is_weights, (0.4,)), (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        assert _code(fn, *args) == STATE                                      # no keep_priorities
    e.selfplay_keep_priorities(True)
    assert _code(e.selfplay_is_weights, 0.4) == STATE                         # no priorities yet
    assert _code(e.selfplay_is_weights_device) == STATE
    assert _code(e.selfplay_is_weight_values) == STATE                        # (nothing was ever computed: there is no array)
    given = np.linspace(0.0, 2.0, 2 * G).astype(np.float32)
    e.selfplay_priorities(0.6, 1e-3, given)
    assert _code(e.selfplay_is_weights_device) == STATE                       # priorities alone are not weights
    e.selfplay_is_weights(0.4)
    assert e.selfplay_is_weights_device() != 0
    before, w = _books(e, case, transitions=False), e.selfplay_is_weight_values().copy()
    np.testing.assert_array_equal(W.bits(w.reshape(2, G)), W.bits(W.is_weights(before["q"].reshape(2, G), case.nets, 0.4)))
    for beta in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf")):
        assert _code(e.selfplay_is_weights, beta) == INVALID, beta
        np.testing.assert_array_equal(W.bits(e.selfplay_is_weight_values()), W.bits(w))
    assert e._f["selfplay_is_weights_device"](e._h, None) == INVALID
    assert e.selfplay_is_weights_device() != 0                                # (a refused call does not invalidate them)
    _assert_books(e, case, before, name)
    # a step changes the set of stored rows: refused until priorities are computed again, and the array stays as it was
    e.selfplay_step()
    assert _code(e.selfplay_is_weights, 0.4) == STATE
    assert _code(e.selfplay_is_weights_device) == STATE
    np.testing.assert_array_equal(W.bits(e.selfplay_is_weight_values()[:2 * G]), W.bits(w))
    e.selfplay_priorities(1.0, 1e-3, np.linspace(0.0, 3.0, 3 * G).astype(np.float32))
    assert _code(e.selfplay_is_weights_device) == STATE
    e.selfplay_is_weights(1.0)
    w3 = e.selfplay_is_weight_values().copy()
    assert w3.shape == (3 * G,) and e.selfplay_is_weights_device() != 0
    e.selfplay_clear()                                                        # so does a clear; an empty ring has no weights
    assert _code(e.selfplay_is_weights, 0.4) == STATE
    assert _code(e.selfplay_is_weights_device) == STATE
    e.selfplay_priorities(0.6, 1e-3, np.zeros(0, np.float32))
    assert _code(e.selfplay_is_weights, 0.4) == STATE                         # priorities of an empty ring: still nothing to weigh
    assert e.selfplay_is_weight_values().shape == (0,)
    for _ in range(3):
        e.selfplay_step()
    np.testing.assert_array_equal(W.bits(e.selfplay_is_weight_values()), W.bits(w3))   # (every refusal left the array alone)
    e.selfplay_keep_priorities(False)                                         # keep_priorities(0) drops them
    for fn, args in ((e.selfplay_is_weights, (0.4,)), (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        assert _code(fn, *args) == STATE
    e.selfplay_keep_priorities(True)
    assert _code(e.selfplay_is_weights_device) == STATE
    e.selfplay_priorities(0.6, 1e-3, np.linspace(0.0, 3.0, 3 * G).astype(np.float32))
    e.selfplay_is_weights(0.4)
    assert e.selfplay_is_weights_device() != 0
    R.begin(e, case, 4, keep=False)                                           # the next begin frees them
    e.selfplay_step()
    for fn, args in ((e.selfplay_is_weights, (0.4,)), (e.selfplay_is_weights_device, ()), (e.selfplay_is_weight_values, ())):
        assert _code(fn, *args) == STATE
    e.selfplay_keep_priorities(True)
    e.selfplay_priorities(0.6, 1e-3, np.linspace(0.0, 1.0, G).astype(np.float32))
    e.selfplay_is_weights(0.4)                                                # (allocated anew for the new ring)
    q = e.selfplay_priority_values().reshape(1, G)
    np.testing.assert_array_equal(W.bits(e.selfplay_is_weight_values().reshape(1, G)), W.bits(W.is_weights(q, case.nets, 0.4)))
    e.close()


def test_how_long_the_device_pointer_stays_valid():
    """A later priorities() takes the pointer away until the weights are recomputed; a reanalysis and an n-step call leave it."""
    name = "cartpole"
    case, e = _engine(name, 8, False, 6, states=True)
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    e.selfplay_is_weights(0.4)
    ptr = e.selfplay_is_weights_device()
    w = _w(e, case).copy()
    R.set_weights(e, case, new=True)
    e.selfplay_reanalyse(2, search_index=R.NEW_INDEX)
    e.selfplay_nstep_targets(3)
    assert e.selfplay_is_weights_device() == ptr                              # (stale but valid, like the priorities they came from)
    np.testing.assert_array_equal(W.bits(_w(e, case)), W.bits(w))
    e.selfplay_priorities(0.6, P.EPS)                                         # the weights now belong to other priorities
    assert _code(e.selfplay_is_weights_device) == _capi.AZG_E_STATE
    np.testing.assert_array_equal(W.bits(_w(e, case)), W.bits(w))             # (the values are still there to be read)
    e.selfplay_is_weights(0.4)
    assert e.selfplay_is_weights_device() == ptr                              # (the same array, recomputed)
    got = _w(e, case)
    np.testing.assert_array_equal(W.bits(got), W.bits(W.is_weights(_q(e, case), 1, 0.4)))
    assert (W.bits(got) != W.bits(w)).any()                                   # (the refreshed values show)
    e.selfplay_keep_priorities(False)
    assert _code(e.selfplay_is_weights_device) == _capi.AZG_E_STATE
    e.close()
