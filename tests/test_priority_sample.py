"""Prioritised sampling from the device replay ring (azg_selfplay_keep_priorities / _priorities / _priority_values / _sample_rows /
_sample_slots, run.PopulationSelfPlay prioritized=...) on the GPU: the priorities against the rule applied to the device's own kept
values and rows, the row and slot draws against the numpy truth over the device's own priorities, population invariance, what the
calls leave alone, the refusals, the Python layer and the examples.  Everything is compared bit for bit.  Cases and sizes:
tests/nstep_util.py; the truth: tests/priority_util.py."""
import ctypes as C

import numpy as np
import pytest

import nstep_util as N
import priority_util as P
import reanalyse_util as R
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

pytestmark = pytest.mark.gpu

TR_KEYS = ("reward", "value", "action", "end")


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
    """What no call of this interface may move: the whole ring, the kept transitions, the games and the ring's books."""
    tr = e.selfplay_transitions() if transitions else {}
    return dict(ring=_whole_ring(e, case), tr={k: v.copy() for k, v in tr.items()}, stats=e.selfplay_stats(), books=e.selfplay_ring())


def _assert_books(e, case, before, what=""):
    now = _books(e, case, transitions=bool(before["tr"]))
    np.testing.assert_array_equal(now["ring"], before["ring"], err_msg=what)
    for k, v in before["tr"].items():
        view = {8: np.uint64, 4: np.uint32}[v.dtype.itemsize]
        np.testing.assert_array_equal(now["tr"][k].view(view), v.view(view), err_msg=f"{what}: {k}")
    assert_stats_bits(now["stats"], before["stats"], what)
    assert now["books"] == before["books"], what


def _q(e, case):
    return e.selfplay_priority_values().reshape(-1, case.games)


def _seed_base(case):
    return case.kw["seed"], case.kw.get("tree_id_base", 0)


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _ring_engine(name, capacity, fifo):
    return _engine(name, capacity, fifo, N.STEPS[name])


@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_priorities_are_the_rule_and_nothing_else_is_written(name, capacity, fifo):
    """After n-step targets with n_step in {0, 3, 1000} and for alpha in {0, 0.6, 1}: q is the rule applied to the device's own kept
    float64 values and V_target column, bit for bit; the ring (every slot), the transitions, the games and the books do not move."""
    case, e = _ring_engine(name, capacity, fifo)
    size = e.selfplay_ring()[0]
    assert size == min(capacity, N.STEPS[name])
    kinds = set()
    for n in (0, 3, 1000):
        e.selfplay_nstep_targets(n)
        before = _books(e, case)
        value = before["tr"]["value"].reshape(size, case.games)
        z = R.ring(e, case)[:, :, -1]
        d = P.gap(value, z)
        if n == 0:   # (z is (float)v: the gap is that rounding's error, at most half a float32 ulp of v)
            assert (d <= np.abs(value).astype(np.float32) * np.float32(2.0 ** -24)).all()
        for alpha in P.ALPHAS:
            e.selfplay_priorities(alpha, P.EPS)
            got = _q(e, case)
            want = P.priorities(d, alpha, P.EPS)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} n_step {n} alpha {alpha}")
            assert got.min() >= 1 and got.max() <= P.Q_MAX
            if alpha == 0:
                assert (got == P.Q_ONE).all()
            elif n:
                assert len(np.unique(got)) > size        # (the rows' priorities differ: a constant would not have passed)
            kinds.add((n, alpha))
            _assert_books(e, case, before, f"{name} n_step {n} alpha {alpha}")
    assert len(kinds) == 9
    e.close()


def _assert_rows(e, case, q, n_orders, index, what):
    seed, base = _seed_base(case)
    out = None
    for n_order in n_orders:
        got = e.selfplay_sample_rows(n_order, index)
        assert got.dtype == np.int32 and got.shape == (case.nets, n_order)
        want = P.sample_rows(q, case.nets, seed, base, index, n_order)
        np.testing.assert_array_equal(got, want, err_msg=f"{what} n_order {n_order}")
        out = got
    return out


@pytest.mark.parametrize("name,capacity,fifo", N.RINGS, ids=N.RING_IDS)
def test_row_draws_are_the_truth(name, capacity, fifo):
    """sample_rows against the truth over the device's own q for n_order in {1, 7, 2 N + 3} (N rows per net: a partial last scan
    segment wherever N is no multiple of 256), from the value gap and from given arrays: one huge entry among tiny ones (both clamps
    of q), only the last stored row large, only the first."""
    case, e = _ring_engine(name, capacity, fifo)
    size = e.selfplay_ring()[0]
    T, G = case.T, case.games
    n_rows = size * T
    n_orders = (1, 7, 2 * n_rows + 3)
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    before = _books(e, case)
    q = _q(e, case)
    got = _assert_rows(e, case, q, n_orders, 5, name)
    assert got.min() >= 0 and got.max() < n_rows
    assert all(len(np.unique(got[k])) > 1 for k in range(case.nets))
    # one huge entry per net among zeros, alpha 1 and a tiny eps: q is 2^40 there and 1 elsewhere
    given = np.zeros((size, G), np.float32)
    spots = [(size // 2, k * T + T // 3) for k in range(case.nets)]
    for s, t in spots:
        given[s, t] = 1e30
    e.selfplay_priorities(1.0, 1e-9, given)
    q = _q(e, case)
    np.testing.assert_array_equal(q, P.priorities(given, 1.0, 1e-9))
    assert set(np.unique(q).tolist()) == {1, P.Q_MAX}
    got = _assert_rows(e, case, q, n_orders, 6, name + " one huge entry")
    for k, (s, t) in enumerate(spots):
        assert (got[k] == s * T + (t - k * T)).all()                              # (the rest weighs n_rows * 2^-40 of the total)
    # only the last / the first stored row of every net is large: the ends of the prefix sums
    for which, (s, j) in (("last", (size - 1, T - 1)), ("first", (0, 0))):
        given = np.full((size, G), 1e-3, np.float32)
        for k in range(case.nets):
            given[s, k * T + j] = 1e4
        e.selfplay_priorities(1.0, P.EPS, given)
        q = _q(e, case)
        np.testing.assert_array_equal(q, P.priorities(given, 1.0, P.EPS))
        got = _assert_rows(e, case, q, n_orders, 7, f"{name} {which} row large")
        # the large row's share of the total is 1e4 / (1e4 + N * 2e-3) > 0.9998 at N <= 792: among 2 N + 3 draws far more than 0.99
        assert ((got == s * T + j).mean(axis=1) > 0.99).all(), which
    _assert_books(e, case, before, name)
    e.close()


@pytest.mark.parametrize("nets", [1, 3])
def test_row_draws_over_more_segments_than_a_wave_has_lanes(nets):
    """The scan of the segment totals gives every lane a run of segments once a net has more than 64 of them (N > 16384 rows): 4101
    CartPole games x 13 steps are 53313 rows in 209 segments for one net (runs of 4, the last run short, a partial last segment), and
    17771 rows in 70 segments (runs of 2) for each of three nets of 1367 games.  Priorities of many magnitudes from a given array;
    4099 row draws and the slot draws against the truth."""
    base = R.CASES["cartpole"]
    case = R.Case(dict(base.kw, n_sims=2), base.net, games=4101, max_len=3, nets=nets)
    steps = 13
    _, e = _engine("", steps, False, steps, transitions=False, case=case)
    assert e.selfplay_ring()[0] == steps
    rng = np.random.default_rng(8)
    given = (10.0 ** rng.uniform(-7.0, 7.0, size=(steps, case.games))).astype(np.float32)
    given[rng.random(given.shape) < 0.1] = 0.0
    e.selfplay_priorities(1.0, 1e-9, given)
    q = _q(e, case)
    np.testing.assert_array_equal(q, P.priorities(given, 1.0, 1e-9))
    assert q.min() == 1 and q.max() == P.Q_MAX and len(np.unique(q)) > 10000
    assert (steps * case.T + 255) // 256 == (209 if nets == 1 else 70)
    got = _assert_rows(e, case, q, (4099,), 11, f"{nets} nets")
    assert all(len(np.unique(got[k] // 256)) > 20 for k in range(nets))      # (the draws land in many segments)
    seed, tree_base = _seed_base(case)
    np.testing.assert_array_equal(e.selfplay_sample_slots(12), P.sample_slots(q, seed, tree_base, 12))
    e.close()


def test_a_nets_draws_are_those_of_a_one_net_engine_at_its_rank():
    """Net k of the 3-net engine against an engine of that net alone whose tree_id_base is the net's first game: the same rows, hence
    the same q, and the same order."""
    name = "population"
    case, e = _ring_engine(name, N.STEPS[name] + 1, False)
    size, T = e.selfplay_ring()[0], case.T
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    q = _q(e, case)
    order = e.selfplay_sample_rows(2 * size * T + 3, 9)
    slots = e.selfplay_sample_slots(4)
    e.close()
    assert len({order[k].tobytes() for k in range(case.nets)}) == case.nets
    for k in range(case.nets):
        one = R.Case(case.net_kw(k), case.net, games=T, max_len=case.max_len)
        one._blob = lambda j, new, k=k: case.blob(k, new)
        _, o = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name], case=one)
        o.selfplay_nstep_targets(3)
        o.selfplay_priorities(0.6, P.EPS)
        np.testing.assert_array_equal(_q(o, one), q[:, k * T:(k + 1) * T], err_msg=f"net {k}")
        np.testing.assert_array_equal(o.selfplay_sample_rows(order.shape[1], 9)[0], order[k], err_msg=f"net {k}")
        np.testing.assert_array_equal(o.selfplay_sample_slots(4), slots[k * T:(k + 1) * T], err_msg=f"net {k}")
        o.close()


@pytest.mark.parametrize("name,capacity,fifo", [N.RINGS[0], N.RINGS[2], N.RINGS[5]], ids=[N.RING_IDS[0], N.RING_IDS[2], N.RING_IDS[5]])
def test_slot_draws_are_the_truth(name, capacity, fifo):
    """sample_slots on the wrapped FIFO ring, on a partly filled STOP ring and on the population: the truth over the device's q, every
    slot a stored one; a column whose only large priority sits in one slot draws that slot."""
    case, e = _ring_engine(name, capacity, fifo)
    size = e.selfplay_ring()[0]
    assert (size < capacity) == (not fifo)
    seed, base = _seed_base(case)
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    before = _books(e, case)
    q = _q(e, case)
    seen = set()
    for index in (0, 1, 1 << 31):
        got = e.selfplay_sample_slots(index)
        assert got.dtype == np.int32 and got.shape == (case.games,)
        np.testing.assert_array_equal(got, P.sample_slots(q, seed, base, index), err_msg=f"{name} index {index}")
        assert got.min() >= 0 and got.max() < size
        seen.add(got.tobytes())
    assert len(seen) == 3
    given = np.zeros((size, case.games), np.float32)
    want = (np.arange(case.games) * 7) % size
    want[-1] = size - 1                                # (slot 0 and the last stored slot among them)
    assert want.min() == 0 and want.max() == size - 1
    given[want, np.arange(case.games)] = 1e30
    e.selfplay_priorities(1.0, 1e-9, given)
    np.testing.assert_array_equal(e.selfplay_sample_slots(3), want)
    np.testing.assert_array_equal(P.sample_slots(_q(e, case), seed, base, 3), want)
    _assert_books(e, case, before, name)
    e.close()


@pytest.mark.parametrize("name,capacity,fifo", [N.RINGS[0], N.RINGS[5]], ids=[N.RING_IDS[0], N.RING_IDS[5]])
def test_draws_repeat_differ_by_index_and_leave_the_games_alone(name, capacity, fifo):
    """The same index gives the same draws twice, another index other draws.  A keeps no priorities and plays s + 1 steps; B plays s,
    computes priorities, draws rows and slots, and plays one more: B's newest rows, transitions, episode statistics, ring books and
    next search are A's -- the step index and the search index were not touched."""
    steps = N.STEPS[name] if fifo else min(N.STEPS[name], capacity - 1)
    case, a = _engine(name, capacity, fifo, steps + 1, priorities=False)
    _, b = _engine(name, capacity, fifo, steps)
    b.selfplay_nstep_targets(0)
    b.selfplay_priorities(0.6, P.EPS)
    n = 3 * case.T
    first = b.selfplay_sample_rows(n, 2)
    np.testing.assert_array_equal(b.selfplay_sample_rows(n, 2), first)
    other = b.selfplay_sample_rows(n, 3)
    assert all((other[k] != first[k]).any() for k in range(case.nets))
    np.testing.assert_array_equal(b.selfplay_sample_rows(7, 2), first[:, :7])       # (draw d does not depend on n_order)
    s0 = b.selfplay_sample_slots(2)
    np.testing.assert_array_equal(b.selfplay_sample_slots(2), s0)
    assert (b.selfplay_sample_slots(3) != s0).any()
    np.testing.assert_array_equal(b.selfplay_sample_rows(n, 2), first)               # (slot draws share nothing with row draws)
    b.selfplay_step()
    np.testing.assert_array_equal(R.bits32(R.ring(b, case)), R.bits32(R.ring(a, case)))
    ta, tb = a.selfplay_transitions(), b.selfplay_transitions()
    for k in TR_KEYS:
        view = {8: np.uint64, 4: np.uint32}[ta[k].dtype.itemsize]
        np.testing.assert_array_equal(tb[k].view(view), ta[k].view(view), err_msg=k)
    assert_stats_bits(b.selfplay_stats(), a.selfplay_stats(), name)
    assert a.selfplay_ring() == b.selfplay_ring()
    for e in (a, b):
        e.search_resident()
    ra, rb = a.results(), b.results()
    for k in ("counts", "n_children", "actions", "Q", "v_target"):
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=k)
    a.close()
    b.close()


def _raw_priorities(e, struct_size=None, source=_capi.PRIO_GIVEN, alpha=0.6, eps=1e-3, given=None):
    c = _capi.AzgPriorityConfig()
    c.struct_size = C.sizeof(_capi.AzgPriorityConfig) if struct_size is None else struct_size
    c.source, c.alpha, c.eps = source, alpha, eps
    if given is not None:
        c.given = _capi._ptr(given, C.c_float)
    return e._f["selfplay_priorities"](e._h, C.byref(c))


def _raw_rows(e, struct_size=None, n_order=4, index=0, order="own"):
    c = _capi.AzgSampleConfig()
    c.struct_size = C.sizeof(_capi.AzgSampleConfig) if struct_size is None else struct_size
    c.n_order, c.sample_index = n_order, index
    buf = np.full((int(getattr(e, "n_nets", 1)), max(n_order, 1)), -7, np.int32)
    rc = e._f["selfplay_sample_rows"](e._h, C.byref(c), _capi._ptr(buf, C.c_int32) if order == "own" else None)
    return rc, buf


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_refusals_leave_the_ring_and_the_priorities_alone(name):
    case = N.CASES[name]
    G = case.games
    e = R.make_engine(_hip(), case)
    for fn, args in ((e.selfplay_keep_priorities, ()), (e.selfplay_priorities, (0.6, 1e-3)), (e.selfplay_priority_values, ()),
                     (e.selfplay_sample_rows, (4, 0)), (e.selfplay_sample_slots, (0,))):
        assert _code(fn, *args) == _capi.AZG_E_STATE                          # no begin
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    given = np.linspace(0.0, 2.0, 2 * G).astype(np.float32)
    for fn, args in ((e.selfplay_priorities, (0.6, 1e-3, given)), (e.selfplay_priority_values, ()), (e.selfplay_sample_rows, (4, 0)),
                     (e.selfplay_sample_slots, (0,))):
        assert _code(fn, *args) == _capi.AZG_E_STATE                          # no keep_priorities
    e.selfplay_keep_priorities(True)                                          # (allowed at any ring size)
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE           # no priorities yet
    assert _code(e.selfplay_sample_slots, 0) == _capi.AZG_E_STATE
    assert _code(e.selfplay_priorities, 0.6, 1e-3) == _capi.AZG_E_STATE       # the value gap without kept transitions
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE
    e.selfplay_priorities(0.6, 1e-3, given)
    before, q = _books(e, case, transitions=False), e.selfplay_priority_values().copy()
    np.testing.assert_array_equal(q, P.priorities(given, 0.6, 1e-3))
    size = C.sizeof(_capi.AzgPriorityConfig)
    assert _raw_priorities(e, struct_size=size - 4, given=given) == _capi.AZG_E_INVALID
    assert _raw_priorities(e, struct_size=0, given=given) == _capi.AZG_E_INVALID
    assert _raw_priorities(e, source=2, given=given) == _capi.AZG_E_INVALID
    assert _raw_priorities(e, source=-1, given=given) == _capi.AZG_E_INVALID
    for alpha in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert _raw_priorities(e, alpha=alpha, given=given) == _capi.AZG_E_INVALID, alpha
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        assert _raw_priorities(e, eps=eps, given=given) == _capi.AZG_E_INVALID, eps
    assert _raw_priorities(e, given=None) == _capi.AZG_E_INVALID              # AZG_PRIO_GIVEN without the array
    for bad in (-1e-6, float("nan"), -float("inf")):
        wrong = given.copy()
        wrong[-1] = bad
        assert _raw_priorities(e, given=wrong) == _capi.AZG_E_INVALID, bad
    with pytest.raises(ValueError, match="one entry per stored row"):
        e.selfplay_priorities(0.6, 1e-3, given[:-1])
    size = C.sizeof(_capi.AzgSampleConfig)
    for kw in (dict(struct_size=size - 4), dict(struct_size=0), dict(n_order=0), dict(n_order=-3), dict(order=None)):
        rc, buf = _raw_rows(e, **kw)
        assert rc == _capi.AZG_E_INVALID and (buf == -7).all(), kw
    assert e._f["selfplay_sample_slots"](e._h, 0, None) == _capi.AZG_E_INVALID
    np.testing.assert_array_equal(e.selfplay_priority_values(), q)
    _assert_books(e, case, before, name)
    want = e.selfplay_sample_rows(9, 1)                                       # (after every refusal the draws still work)
    np.testing.assert_array_equal(want, P.sample_rows(q.reshape(2, G), case.nets, *_seed_base(case), 1, 9))
    inf = given.copy()
    inf[0] = float("inf")                                                     # (not refused: the upper clamp takes it)
    e.selfplay_priorities(1.0, 1e-3, inf)
    assert int(e.selfplay_priority_values()[0]) == P.Q_MAX
    # a step changes the set of stored rows: the priorities are stale until they are computed again
    e.selfplay_step()
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE
    assert _code(e.selfplay_sample_slots, 0) == _capi.AZG_E_STATE
    e.selfplay_priorities(0.0, 1e-3, np.zeros(3 * G, np.float32))
    assert e.selfplay_sample_rows(4, 0).shape == (case.nets, 4)
    e.selfplay_clear()                                                        # so does a clear
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE
    assert _raw_priorities(e, given=given) == _capi.AZG_OK                    # an empty ring: nothing is launched
    assert e.selfplay_priority_values().shape == (0,)
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE           # ... and nothing can be drawn from it
    assert _code(e.selfplay_sample_slots, 0) == _capi.AZG_E_STATE
    # n-step calls do not change the set of stored rows: the priorities stay valid, if stale
    e.selfplay_keep_transitions(True)
    for _ in range(2):
        e.selfplay_step()
    e.selfplay_nstep_targets(0)
    e.selfplay_priorities(0.6, 1e-3)
    q = e.selfplay_priority_values().copy()
    e.selfplay_nstep_targets(3)
    np.testing.assert_array_equal(e.selfplay_priority_values(), q)
    np.testing.assert_array_equal(e.selfplay_sample_rows(5, 0), P.sample_rows(q.reshape(2, G), case.nets, *_seed_base(case), 0, 5))
    e.selfplay_keep_priorities(False)
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE
    e.selfplay_keep_priorities(True)                                          # (on again within one begin: priorities are asked for anew)
    assert _code(e.selfplay_sample_rows, 4, 0) == _capi.AZG_E_STATE
    e.selfplay_priorities(0.6, 1e-3)
    e.selfplay_sample_slots(0)
    R.begin(e, case, 4, keep=False)                                           # the next begin drops it
    e.selfplay_step()
    assert _code(e.selfplay_priorities, 0.6, 1e-3, np.zeros(G, np.float32)) == _capi.AZG_E_STATE
    assert _code(e.selfplay_sample_slots, 0) == _capi.AZG_E_STATE
    e.close()


def test_a_reanalysis_leaves_the_priorities_valid():
    """A reanalysis rewrites rows and kept values but not the set of stored rows: draws still come from the q computed before it."""
    name = "cartpole"
    case, e = _engine(name, 8, False, 6, states=True)
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    q = _q(e, case).copy()
    R.set_weights(e, case, new=True)
    e.selfplay_reanalyse(2, search_index=R.NEW_INDEX)
    np.testing.assert_array_equal(_q(e, case), q)
    np.testing.assert_array_equal(e.selfplay_sample_slots(1), P.sample_slots(q, *_seed_base(case), 1))
    e.selfplay_nstep_targets(3)
    e.selfplay_priorities(0.6, P.EPS)
    assert (_q(e, case) != q).any()                                           # (recomputed: the refreshed values show)
    e.close()


def _policies(n):
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    nets = []
    for s in range(n):
        torch.manual_seed(80 + s)
        nets.append(make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2))
    return nets


def test_reanalyse_by_priority_searches_the_drawn_slots():
    """run.PopulationSelfPlay(prioritized=..., reanalyse=True, n_step=3).reanalyse(by="priority"): the slots are the truth's draw under
    the second counter's index over the priorities as they stood, and the ring afterwards is that of a twin that reanalysed
    reanalyse(slots=that array); by="uniform" is untouched and takes no sample index."""
    import torch
    from alphazero_gym_amd import run
    T, steps, cap = 11, 6, 4
    kw = dict(game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, gamma=0.97, max_episode_length=4, capacity_steps=cap, seed=21,
              fifo=True, reanalyse=True, n_step=3)
    sps = []
    for prioritized in ({"alpha": 0.6, "eps": 1e-3}, None):
        nets = _policies(2)
        sp = run.PopulationSelfPlay(nets, prioritized=prioritized, **kw)
        sp.play(steps)
        with torch.no_grad():
            for net in nets:
                for p in net.parameters():
                    p.mul_(1.5)
        sps.append(sp)
    sp, twin = sps
    assert sp.engine.selfplay_ring()[:2] == (cap, steps - cap)
    for index in (0, 1):
        sp.priorities()
        q = sp.engine.selfplay_priority_values().reshape(cap, 2 * T)
        want = P.sample_slots(q, 21, 0, index)
        used = sp.reanalyse(by="priority")
        assert len(used) == 1
        np.testing.assert_array_equal(used[0], want)
        assert len(np.unique(want)) > 1
        twin.reanalyse(slots=want)
        np.testing.assert_array_equal(R.bits32(sp.engine.selfplay_rows(clear=False)), R.bits32(twin.engine.selfplay_rows(clear=False)))
        np.testing.assert_array_equal(R.bits64(sp.engine.selfplay_transitions()["value"]), R.bits64(twin.engine.selfplay_transitions()["value"]))
    assert (sp._slot_sample_index, sp._sample_index, sp._reanalyse_index) == (2, 0, run.REANALYSE_INDEX_BASE + 2)
    assert sp.reanalyse(n=2) == twin.reanalyse(n=2)                           # (by="uniform": today's path, the same generator)
    with pytest.raises(ValueError, match="by"):
        sp.reanalyse(by="value")
    with pytest.raises(ValueError, match="draws the slots itself"):
        sp.reanalyse(slots=[1], by="priority")
    with pytest.raises(RuntimeError, match="prioritized"):
        twin.reanalyse(by="priority")
    with pytest.raises(RuntimeError, match="prioritized"):
        twin.sample_order(4)
    assert _code(twin.engine.selfplay_priority_values) == _capi.AZG_E_STATE   # (off: nothing is kept)
    sp.close()
    twin.close()
    with pytest.raises(ValueError, match="n_step"):
        run.PopulationSelfPlay(_policies(1), prioritized={"alpha": 0.6}, **dict(kw, n_step=None))
    with pytest.raises(ValueError, match="alpha and eps"):
        run.PopulationSelfPlay(_policies(1), prioritized={"beta": 0.4}, **kw)


def test_sample_order_trains_a_population_from_the_ring():
    """PopulationSelfPlay(prioritized=...) on 2 nets: sample_order(n) is the truth over the recomputed priorities under the row
    counter's next index, train_epoch_ring takes it as it comes, and the one-net DeviceSelfPlay draws net 0's order."""
    import trainer_util as TU
    from alphazero_gym_amd import run
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    K, T, steps, batch = 2, 4, 5, 8
    agents = TU.make_agents("discrete", "a0c_tuned", K)
    kw = dict(game="CartPole-v0", n_rollouts=8, c_uct=1.5, epsilon=0.1, capacity_steps=8, n_step=3, prioritized={"alpha": 0.6, "eps": 1e-3})
    sp = run.PopulationSelfPlay([a.nn for a in agents], games_per_net=T, **kw)
    assert sp.play_device(steps) == (steps, 0)
    n = steps * T
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    start = TU.state_of(tr)
    orders = []
    for index in (0, 1):
        order = sp.sample_order(n)
        q = sp.engine.selfplay_priority_values().reshape(steps, K * T)
        tr_now = sp.engine.selfplay_transitions()["value"].reshape(steps, K * T)
        z = sp.engine.selfplay_rows(clear=False)[:, -1].reshape(steps, K * T)
        np.testing.assert_array_equal(q, P.priorities(P.gap(tr_now, z), 0.6, 1e-3))
        np.testing.assert_array_equal(order, P.sample_rows(q, K, 34, 0, index, n))
        assert order.dtype == np.int32 and order.shape == (K, n) and order.min() >= 0 and order.max() < n
        infos = tr.train_epoch_ring(sp, order, batch_size=batch)
        assert len(infos) == K and all(np.isfinite(v) for info in infos for v in info.values())
        orders.append(order)
    assert (orders[0] != orders[1]).any() and sp._sample_index == 2
    assert not np.array_equal(TU.state_of(tr)["flat"].cpu().numpy(), start["flat"].cpu().numpy())
    given = np.zeros((steps, K * T), np.float32)
    given[2, [1, T + 3]] = 1e30                                                # (a loop's own errors: one row per net stands out)
    order = sp.sample_order(6, given=given)
    assert order.tolist() == [[2 * T + 1] * 6, [2 * T + 3] * 6]
    assert sp.engine.selfplay_ring()[0] == steps
    tr.close()
    sp.close()
    agents = TU.make_agents("discrete", "a0c_tuned", K)
    one = run.DeviceSelfPlay(agents[0].nn, n_games=T, **kw)
    one.play(steps)
    np.testing.assert_array_equal(one.sample_order(n)[0], orders[0][0])
    one.close()


@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8"])])
def test_examples_train_on_prioritised_rows(example, extra):
    """--prioritized-alpha 0.6 --n-step 3 at 16 games with --replay-steps 4 --reanalyse-slots 1: the FIFO ring wraps, the draw picks
    the training rows and the reanalysed positions, and the loop trains on finite targets.  Without --n-step the flag is refused."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module(example)
    common = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4",
              "--reanalyse-slots", "1", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5",
              "--device", "cuda", "--prioritized-alpha", "0.6"] + extra
    a = mod.parse_args(common + ["--n-step", "3"])
    assert (a.prioritized_alpha, a.prioritized_eps, a.n_step) == (0.6, 1e-3, 3)
    hist = mod.train(a, log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    with pytest.raises(SystemExit):
        mod.parse_args(common)
