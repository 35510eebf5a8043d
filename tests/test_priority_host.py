"""Prioritised sampling's numpy truth (tests/priority_util.py) on the CPU: its Philox against the oracle's own draw, the priority rule
on hand-written values, the draw on a three-row example where an off-by-one shows, the draws' frequencies, and the ABI of the built
library (include/azgym_priority.h)."""
import ctypes as C

import numpy as np

import oracle_lib as O
import priority_util as P
from alphazero_gym_amd import _capi


def test_numpy_philox_is_the_oracles():
    """oracle_lib.act_draw is azg_draw(seed, tree, step, 0, AZG_STREAM_ACT): its u01 comes from word 0, its raw word is word 1."""
    for seed, tree, step in [(34, 0, 0), (34, 5, 17), (12, 1000, 3), ((7 << 32) | 9, 3, 1 << 31), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1)]:
        w = P.draw(seed, tree, step, 0, P.STREAM_ACT)
        u01, u, word1 = O.act_draw(seed, tree, step)
        assert int(w[1][0]) == word1, (seed, tree, step)
        assert (float(int(w[0][0])) + 0.5) * (1.0 / 4294967296.0) == u
        assert np.float32((int(w[0][0]) >> 8) * 2.0 ** -24 + 2.0 ** -25) == np.float32(u01)
    # (arrays of counters give the scalars' words)
    many = P.draw(34, np.arange(4, dtype=np.uint64), 17, 0, P.STREAM_ACT)
    assert [int(v) for v in many[1]] == [O.act_draw(34, t, 17)[2] for t in range(4)]
    assert (P.STREAM_SAMPLE, P.STREAM_SLOT) == (5, 6)


def test_alpha_zero_is_one_everywhere():
    d = np.asarray([0.0, 1e-30, 0.5, 3.0, 1e30, np.inf], np.float32)
    np.testing.assert_array_equal(P.priorities(d, 0.0), np.full(d.shape, P.Q_ONE, np.uint64))


def test_the_clamps_sit_at_two_to_the_minus_and_plus_twenty():
    lo, hi = np.float32(2.0 ** -20), np.float32(2.0 ** 20)
    p = np.asarray([np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)), hi,
                    np.nextafter(hi, np.float32(np.inf)), np.inf, np.nan, 0.0, -1.0, 1.0, 1.5], np.float32)
    q = [int(v) for v in P.q_of_p(p)]
    below_hi = int(float(np.nextafter(hi, np.float32(0))) * 1048576.0)
    assert q == [1, 1, 1, below_hi, 1 << 40, 1 << 40, 1 << 40, 1, 1, 1, 1 << 20, 3 << 19]
    assert below_hi == (1 << 40) - (1 << 16)          # (one float32 ulp below 2^20 is 2^-4: 2^16 in fixed point)
    # p = 2^-20 itself is 1 by the middle branch, the value just above it truncates to 1 as well: q never reaches 0
    assert min(q) == 1


def test_the_rule_rounds_every_step_to_float32():
    """d + eps, alpha * log and both functions one by one: against the oracle's functions called by hand."""
    d = np.asarray([0.0, 0.25, 3.0, 100.0], np.float32)
    alpha, eps = np.float32(0.6), np.float32(1e-3)
    want = []
    for x in d:
        s = np.float32(x + eps)
        m = np.float32(alpha * np.float32(O.math_eval(3, [s])[0]))
        want.append(int(np.float64(np.float32(O.math_eval(0, [m])[0])) * 1048576.0))
    assert [int(v) for v in P.priorities(d, 0.6, 1e-3)] == want
    assert want == sorted(want) and want[0] < want[-1]      # (monotone in d)
    assert abs(want[2] / P.Q_ONE - 3.001 ** 0.6) < 1e-5
    # the gap is taken in float64 and rounded once
    v, z = np.asarray([0.1, -2.0]), np.asarray([0.1, 1.0], np.float32)
    np.testing.assert_array_equal(P.gap(v, z), np.asarray([abs(0.1 - float(np.float32(0.1))), 3.0], np.float32))


def _pick_mutant(csum, x):
    """The draw with >= in place of >."""
    target = (int(x) * csum[-1]) >> 64
    return next(i for i, c in enumerate(csum) if c >= target)


def test_the_draw_on_one_one_two():
    csum = P.prefix([1, 1, 2])
    assert csum == [1, 2, 4]
    xs = [t << 62 for t in range(4)]                   # total 4: (x * 4) >> 64 = t
    assert [(x * 4) >> 64 for x in xs] == [0, 1, 2, 3]
    assert [P.pick(csum, x) for x in xs] == [0, 1, 2, 2]
    assert [_pick_mutant(csum, x) for x in xs] != [0, 1, 2, 2]
    assert P.pick(csum, (1 << 64) - 1) == 2            # (the largest x stays below the total)
    assert P.pick(P.prefix([P.Q_MAX] * 3), (1 << 64) - 1) == 2


def test_frequencies_follow_the_priorities():
    """q = [1 .. 8] * 2^20, 36 000 draws under a fixed seed: every row's count within 5 binomial standard deviations."""
    q = np.arange(1, 9, dtype=np.uint64) * np.uint64(P.Q_ONE)
    n = 36000
    got = P.row_draws(q, seed=34, first_tree=0, sample_index=0, n_order=n)
    counts = np.bincount(got, minlength=8)
    assert counts.sum() == n and got.min() >= 0 and got.max() <= 7
    for i in range(8):
        prob = (i + 1) / 36.0
        sd = np.sqrt(n * prob * (1.0 - prob))
        assert abs(counts[i] - n * prob) <= 5.0 * sd, (i, counts.tolist())
    # slot draws: one draw per game column over the same eight values
    cols = 4500
    slots = P.sample_slots(np.repeat(q[:, None], cols, axis=1), seed=34, tree_id_base=0, sample_index=0)
    sc = np.bincount(slots, minlength=8)
    for i in range(8):
        prob = (i + 1) / 36.0
        assert abs(sc[i] - cols * prob) <= 5.0 * np.sqrt(cols * prob * (1.0 - prob)), (i, sc.tolist())


def test_sample_rows_numbers_a_nets_rows_slot_major():
    """Net k's numbering is slot * T + game over its own columns; a net's draws do not depend on the other nets' rows."""
    rng = np.random.default_rng(3)
    q = rng.integers(1, 1 << 30, size=(5, 6)).astype(np.uint64)
    both = P.sample_rows(q, 2, seed=9, tree_id_base=4, sample_index=2, n_order=50)
    alone = P.sample_rows(q[:, 3:], 1, seed=9, tree_id_base=7, sample_index=2, n_order=50)
    np.testing.assert_array_equal(both[1], alone[0])
    one_hot = np.ones((5, 6), np.uint64)
    one_hot[3, 4] = P.Q_MAX                            # net 1 (games 3 .. 5), slot 3, game 1 of the net: row 3 * 3 + 1
    assert set(P.sample_rows(one_hot, 2, 9, 0, 0, 20)[1].tolist()) == {10}


def test_the_built_library_has_the_entry_points_and_the_structs_match_the_header():
    from alphazero_gym_amd import _native
    lib = _native.lib()
    for name in ("keep_priorities", "priorities", "priority_values", "sample_rows", "sample_slots"):
        assert hasattr(lib, "azg_selfplay_" + name), name
        assert "selfplay_" + name in _capi.OPTIONAL_SYMBOLS
    pc, sc = _capi.AzgPriorityConfig, _capi.AzgSampleConfig
    assert C.sizeof(pc) == 24 and (pc.source.offset, pc.alpha.offset, pc.eps.offset, pc.given.offset) == (4, 8, 12, 16)
    assert C.sizeof(sc) == 12 and (sc.n_order.offset, sc.sample_index.offset) == (4, 8)
    assert (_capi.PRIO_VALUE_GAP, _capi.PRIO_GIVEN) == (0, 1)
