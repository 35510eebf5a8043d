"""CPU: what the random populations of population_fuzz.py cover, asserted on the generator and the oracle alone.

For the 48 seeds test_population_fuzz.py (GPU) runs: every case builds, every net's oracle engine accepts its settings and budget, and
every tree's root counts are its own net's budget.  Over the whole set the coverage conditions below hold -- conditions, not
measurements: a seed list that misses one fails here, before any device is compared.  Then the hand-made cases whose budgets put the
16-level path boundary at a different depth for each net of one launch, and the self-play seeds."""
import functools
import time

import numpy as np
import pytest

import net_rollouts_util as R
import net_search_util as N
import population_fuzz as F


@functools.lru_cache(maxsize=None)
def _survey():
    """One pass over the seeds: per seed the case's figures (no arrays are kept)."""
    rows = []
    for seed in F.SEEDS:
        c = F.case(seed)
        t0 = time.perf_counter()
        want = F.oracle(c)
        secs = time.perf_counter() - t0
        R.assert_root_counts(want, c.sims, c.T, c.carry, F.describe(c))
        assert want[0]["counts"].shape[0] == c.K * c.T
        if c.mode == 1:
            assert want[0]["counts"].shape[1] == c.kmax
        terminal = bool(((want[1]["node_flags"] & 2) != 0).any())
        matters = None
        if c.K >= 2:   # every net with net 0's settings and budget: does some other net's result change?
            same = F.oracle(c, settings=[c.settings[0]] * c.K, sims=[c.sims[0]] * c.K)
            sl = slice(c.T, None)
            matters = any(want[1][key][sl].tobytes() != same[1][key][sl].tobytes() for key in want[1])
        rows.append(dict(c=c, secs=secs, terminal=terminal, matters=matters))
    return rows


def test_every_case_builds_and_runs_its_budgets():
    rows = _survey()
    assert len(rows) == 48
    for r in rows:
        c = r["c"]
        assert len(c.settings) == len(c.budgets) == len(c.blobs) == c.K and c.roots.shape[0] == c.K * c.T
        assert all(0 <= b <= c.cap for b in c.budgets) and all(1 <= n <= c.cap for n in c.sims)
        assert c.cap <= (F.CAP_WIDE if c.wide else F.CAP) and (not c.wide or len(c.hidden) <= 2)
        assert c.redraws <= 20
        if c.mode == 1:   # the Kmax rule: every net fits at its own budget
            assert all(N.kmax_of(s, n) <= c.kmax for s, n in zip(c.settings, c.sims))
        if c.K >= 2:
            assert any(s != c.settings[0] for s in c.settings[1:])
        if c.lockstep:
            assert c.T in F.TS_LOCKSTEP and c.K in F.KS_LOCKSTEP
    slow = max(rows, key=lambda r: r["secs"])
    print(f"slowest oracle run: {slow['secs']:.2f} s ({F.describe(slow['c'])}); all 48: {sum(r['secs'] for r in rows):.1f} s")
    assert slow["secs"] < 10.0


def test_the_generator_is_deterministic():
    a, b = F.case(5), F.case(5)
    assert F.describe(a) == F.describe(b) and a.settings == b.settings and a.roots.tobytes() == b.roots.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.blobs, b.blobs))


def test_coverage_conditions():
    rows = _survey()
    cs = [r["c"] for r in rows]

    def count(pred):
        return sum(bool(pred(c)) for c in cs)

    assert {c.mode for c in cs} == {0, 1}
    assert {c.env for c in cs} == {0, 1, 2, 3, 4, 5}                       # CartPole, both Pendulums, MountainCar, MountainCarContinuous, Acrobot
    assert count(lambda c: c.ncomp >= 2) >= 1 and count(lambda c: c.ln) >= 1
    assert count(lambda c: c.wide and c.lockstep) >= 1 and count(lambda c: c.wide and not c.lockstep) >= 1
    assert count(lambda c: c.K == 1) >= 2 and count(lambda c: c.K >= 6) >= 3
    for T in (1, 16, 17, 33):
        assert count(lambda c: c.T == T) >= 1, T
    # budget classes, as the ABI takes them (0: the engine's) -- on nets of a capacity that tells them apart
    for name, cls in (("0", lambda c, b: b == 0), ("1", lambda c, b: b == 1 and c.cap > 2), ("2", lambda c, b: b == 2 and c.cap > 3),
                      ("capacity - 1", lambda c, b: b == c.cap - 1 and c.cap > 3), ("capacity", lambda c, b: b == c.cap and c.cap > 3)):
        assert count(lambda c: any(cls(c, b) for b in c.budgets)) >= 1, name
    assert count(lambda c: c.K >= 2 and max(c.sims) > c.sims[0]) >= 5       # the largest budget on a net other than net 0
    assert count(lambda c: c.K >= 3 and len(set(c.sims)) < c.K and len(set(c.sims)) > 1) >= 3   # two nets share a budget next to a third
    fits_by_budget = count(lambda c: c.mode == 1 and any(N.kmax_of(s, c.cap) > c.kmax >= N.kmax_of(s, n) for s, n in zip(c.settings, c.sims)))
    assert fits_by_budget >= 3, fits_by_budget
    chain_next_to_branching = count(lambda c: c.mode == 1 and any(F.law_of(s) == F.CHAIN for s in c.settings)
                                    and any(N.kmax_of(s, n) >= 2 for s, n in zip(c.settings, c.sims)))
    assert chain_next_to_branching >= 3, chain_next_to_branching
    assert count(lambda c: c.kw.get("tie_break") == "random") >= 2
    for v in F.VARIANTS:
        assert count(lambda c: c.variant == v) >= 2, v
    # ... and the shapes that a forced variant only takes with LDS trees and a register-resident layer are taken, not just asked for
    import test_population_parity as PP
    for v, key, value in (("waves8", "waves", 8), ("groups2", "groups", 2), ("tile8", "tile_trees", 8)):
        assert count(lambda c: c.variant == v and PP._shape(c.cfg, v)[key] == value) >= 2, v
    # the table matters
    multi = [r for r in rows if r["c"].K >= 2]
    assert 2 * sum(r["matters"] for r in multi) >= len(multi), (sum(r["matters"] for r in multi), len(multi))
    # terminal nodes where the game has them within reach: every such case with room for them, and some of each env
    for env in (0, 4):
        with_room = [r for r in rows if r["c"].env == env and max(r["c"].sims) >= 8]
        assert len(with_room) >= 2 and all(r["terminal"] for r in with_room), (env, [F.describe(r["c"]) for r in with_room if not r["terminal"]])


def test_second_search_seeds():
    seeds = F.second_search_seeds()
    assert len(seeds) == F.SECOND_SEARCH
    modes = set()
    for seed in seeds:
        c = F.case(seed)
        raw, sims = F.rotated(c)
        assert sims != c.sims and sorted(sims) == sorted(c.sims)
        modes.add(c.mode)
    assert modes == {0, 1}


# ------------------------------------------------------------------------------------------- budgets across the 16-level boundary


@pytest.mark.parametrize("name", ["p64-lds", "p512-team"])
def test_chain_budgets_put_the_boundary_at_each_nets_own_depth(name):
    """Net k's deepest leaf is exactly its budget (a chain), and the levels <= 15, == 16, >= 17 and >= 33 are each reached."""
    depths = F.boundary_traces(name)
    sims = F.BOUNDARY_SIMS
    assert [int(d.max()) for d in depths] == sims == [15, 16, 17, 33]
    assert depths[0].max() <= 15 and (depths[1] == 16).any() and depths[1].max() == 16
    assert (depths[2] >= 17).any() and (depths[3] >= 33).any()
    kw, desc, blobs, roots, settings, sims, T, _ = F.boundary_case(name)
    assert kw["n_sims"] == F.BOUNDARY_CAP == 40 and len(blobs) == 4 and roots.shape[0] == 4 * T
    want = F.boundary_oracle(name)
    R.assert_root_counts(want, sims, T, None, name)
    nrec = want[1]["n_records"].reshape(4, T)
    assert (nrec == np.array(sims)[:, None] + 1).all()


def test_boundary_cases_share_their_nets():
    """The forced forms of a shape run the same population (one oracle result per shape)."""
    for a, b in (("p64-lds", "p64-global_tree"), ("p512-team", "p512-launches"), ("p512-team", "p512-persistent")):
        x, y = F.boundary_case(a), F.boundary_case(b)
        assert x[0] == y[0] and x[3].tobytes() == y[3].tobytes() and x[4] == y[4] and x[5] == y[5] and x[7] != y[7]


def test_discrete_budgets_on_both_sides_of_the_boundary():
    """CartPole: net 0's budget stops its trees below level 16, net 1's takes some trace beyond it (level 17 or deeper)."""
    kw, desc, blobs, roots, carry, settings, sims, T = F.discrete_boundary_case()
    depths = F.discrete_boundary_traces()
    print(f"discrete boundary budgets {sims}: deepest leaves {[int(d.max()) for d in depths]}")
    assert sims[0] < sims[1] <= sims[2] == kw["n_sims"]
    assert depths[0].max() <= 15 and depths[1].max() >= 17 and depths[2].max() >= 17
    assert depths[0].max() >= 10           # (and not far below: the budget is the last one that stays inside the lanes)
    R.assert_root_counts(F.discrete_boundary_oracle(), sims, T, carry, "discrete boundary")


# ------------------------------------------------------------------------------------------------------------------- self-play


def test_selfplay_seeds_cover_what_they_are_there_for():
    sps = [F.selfplay_case(s) for s in F.SELFPLAY_SEEDS]
    assert len(sps) == 6
    assert {"Acrobot-v1", "MountainCarContinuous-v0"} <= {sp.game for sp in sps}
    assert any(sp.T == 1 for sp in sps) and any(sp.K == 6 for sp in sps)
    assert any(sp.v_target == "on_policy" for sp in sps)
    assert any(sp.rule["final_selection"] == "max_value" for sp in sps)
    assert any(sp.rule["temperature"] != 1.0 and sp.case.mode == 0 and len(set(sp.sims)) > 1 for sp in sps)   # counts bounded by each net's budget
    for sp in sps:
        assert not sp.case.wide and all(1 <= n <= sp.cap <= F.SELFPLAY_CAP for n in sp.sims) and sp.K * sp.T <= 9 * 33
