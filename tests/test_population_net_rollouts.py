"""GPU (-m gpu): per-net simulation budgets in one search launch (azg_net_search.n_sims), bit for bit against the CPU oracle.

A K-net engine whose nets carry their own budget (and their own c_uct / gamma / epsilon / c_pw / kappa) must compute what K oracle
engines compute -- net k CREATED with n_sims = its budget, its settings, its own weights and tree_id_base + k*T: results, root
children, n_rec and every record of every tree (net_rollouts_util brings the narrower engines to the population's widths).  The
engine's own n_sims is the capacity: it sizes the storage and picks the kernel form, whatever the budgets are.  Every case also asserts
that each tree's root counts sum to its own net's budget: an engine that ignores the field runs the capacity everywhere and fails it."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import net_rollouts_util as R
import net_search_util as N
import net_search_wide_util as NW
import parity_util as P
import test_population_net_search as NS
import test_population_net_search_wide as NSW
import test_population_parity as PP
import test_population_wide as W
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

K, T, SIDX = PP.K, 19, PP.SIDX
AZG_E_INVALID = _capi.AZG_E_INVALID


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _search(e, roots, carry, sidx=SIDX):
    e.set_search_index(sidx)
    e.search(roots, carry)
    return PP._collect(e)


def _table(settings):
    return [N.full(s) for s in settings]


# ------------------------------------------------------------------------------------------------- 1. the matrix, 2. forced variants


@functools.lru_cache(maxsize=2)
def _want(ci, trees):
    kw, desc, blobs, roots, carry = PP._inputs(ci, trees)
    return R.oracle_nets(kw, desc, blobs, roots, carry, SIDX, N.net_settings(P.CONFIGS[ci]), R.budgets(kw["n_sims"]))


def _run_row(native, ci, variant, monkeypatch):
    cfg = P.CONFIGS[ci]
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    want_shape = dict(PP._shape(cfg, "no_spec" if variant == "default" else variant), spec=0)
    trees = 35 if want_shape["groups"] == 2 else T
    kw, desc, blobs, roots, carry = PP._inputs(ci, trees)
    sims = R.budgets(kw["n_sims"])
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search(_table(N.net_settings(cfg)), n_sims=sims)
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    what = f"cfg{ci}-{variant}"
    R.assert_root_counts(got, sims, trees, carry, what)
    PP._assert_same(got, _want(ci, trees), trees, what)
    shape = NS._ran_shape(info)
    print(f"{what}: K={K} T={trees} budgets {sims} {shape} {info['last_ms']:.3f} ms")
    # the capacity decides the shape: the one the row's table runs without budgets
    assert info["kernel_form"] == "persistent" and shape == want_shape, (variant, shape, want_shape)


@pytest.mark.parametrize("ci", N.matrix_rows(), ids=lambda ci: f"cfg{ci}")
def test_three_nets_three_budgets_bit_exact_vs_oracle(native, ci, monkeypatch):
    """Every row, K = 3 nets of distinct weights, settings AND budgets {capacity, 1, n_sims // 3 + 1} in one launch."""
    _run_row(native, ci, "default", monkeypatch)


@pytest.mark.parametrize("ci,variant", NS._forced_cases())
def test_forced_variants(native, ci, variant, monkeypatch):
    _run_row(native, ci, variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------- 3. wide rows


@functools.lru_cache(maxsize=None)
def _want_wide(row_key, Tw):
    row = NSW.ROWS[row_key]
    kw, desc, blobs, roots, carry = W._inputs(NW.cfg_of(row), Tw)
    return R.oracle_nets(kw, desc, blobs, roots, carry, W.SIDX, NW.net_settings(row), R.budgets(kw["n_sims"]))


@pytest.mark.parametrize("row,variant", NW.cases(), ids=[f"{NW.row_id(r)}-{v}" for r, v in NW.cases()])
def test_three_wide_nets_three_budgets_bit_exact_vs_oracle(native, row, variant, monkeypatch):
    """Widths >= 512 (AZG_NET_SEARCH_WIDE): lock-step shaped rows as 3 x 32 trees, one team per net, on the team kernel's table form,
    the per-layer launches -- whose host loop runs to the largest budget while the finished nets' tree groups sit the later launches
    out -- and the one-launch kernel; the other rows as 3 x 19 trees on the one-launch kernel."""
    for var in W.FORCING:
        monkeypatch.delenv(var, raising=False)
    cfg, Tw, ls = NW.cfg_of(row), NW.trees_per_net(row), NW.lockstep_shaped(row)
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    kw, desc, blobs, roots, carry = W._inputs(cfg, Tw)
    sims = R.budgets(kw["n_sims"])
    e = W._population(native, kw, desc, blobs)
    e.set_net_search(_table(NW.net_settings(row)), wide=True, n_sims=sims)
    e.set_search_index(W.SIDX)
    e.search(roots, carry)
    got = W._collect(e)
    info = e.search_info()
    e.close()
    what = f"{NW.row_id(row)}-{variant}"
    print(f"{what}: K={K} T={Tw} budgets {sims} {info['kernel_form']} {info['kernel_name']} fallbacks {info['team_fallbacks']}")
    R.assert_root_counts(got, sims, Tw, carry, what)
    W._assert_same(got, _want_wide(NW.row_id(row), Tw), Tw, what)
    if ls and variant in ("default", "global_tree"):
        NSW._assert_table_form(info, row, what, global_tree=variant == "global_tree")
    elif ls and variant == "launches":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, (what, info)
        assert info["kernel_name"].startswith("ls_tree_kernel_nets<"), (what, info)
    else:
        assert info["kernel_form"] == "persistent" and info["kernel_name"].startswith("search_kernel_nets<"), (what, info)


# ------------------------------------------------------------------------------------------------- 4. the capacity decides the form


@pytest.mark.parametrize("mode", ["continuous", "discrete"])
def test_capacity_decides_the_form_not_the_budget(native, mode):
    """Capacity 300 on a 2x64 net, budgets {300, 5, 1}: nets 1 and 2 equal oracle engines created with 5 and 1.
    Continuous (Pendulum-v1): 302 records per tree, so the trees take 9-bit ids in LDS whatever the nets run -- engines of 5 and 1
    simulations would have taken 8-bit ids.  Net 1 widens with (2.5, 0.7): 8 children within its own 5 simulations, which fits, and 136
    within 300, which would not -- the Kmax rule counts the net's own budget.
    Discrete (CartPole): 603 records, global trees; the roots carry counts up to 54, inside the capacity's sqrt table (1204 entries)
    and beyond the 24 entries of a 5-simulation engine, which computes those square roots in place -- the same bits."""
    if mode == "continuous":
        cfg = (2, 1, [64, 64], "elu", 300, dict(c_uct=0.05, gamma=1.0))
        kw = dict(env_id=2, mode=1, n_trees=K * T, n_sims=300, seed=1234, tree_id_base=PP.BASE, c_uct=0.05, gamma=1.0, c_pw=0.9, kappa=0.5)
        st = [dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=0.9, kappa=0.5), dict(c_uct=0.2, gamma=0.9, epsilon=0.25, c_pw=2.5, kappa=0.7),
              dict(c_uct=0.0125, gamma=0.97, epsilon=0.0, c_pw=0.9, kappa=0.5)]
        assert N.kmax_of(st[0], 300) == 16 and N.kmax_of(st[1], 5) == 8 and N.kmax_of(st[1], 300) > 16
        carry, records, storage = None, 302, "lds9"
    else:
        cfg = (0, 0, [64, 64], "relu", 300, dict(c_uct=1.5, gamma=1.0, num_actions=2))
        kw = dict(env_id=0, mode=0, n_trees=K * T, n_sims=300, seed=1234, tree_id_base=PP.BASE, c_uct=1.5, gamma=1.0, num_actions=2)
        st = [dict(c_uct=1.5, gamma=1.0, epsilon=0.0), dict(c_uct=6.0, gamma=0.9, epsilon=0.25), dict(c_uct=0.375, gamma=0.97, epsilon=0.0)]
        carry, records, storage = ((np.arange(K * T) % 7) * 9).astype(np.int32), 603, "global"
    desc = P.config_net(cfg, 99)[0]
    blobs = [P.config_net(cfg, 99 + k)[1] for k in range(K)]
    sims = [300, 5, 1]
    e = PP._population(native, kw, desc, blobs)
    assert e.max_records == records
    roots = e.synthetic_roots()
    e.set_net_search(_table(st), n_sims=sims)
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    assert info["kernel_form"] == "persistent" and info["tree_storage"] == storage, info
    R.assert_root_counts(got, sims, T, carry, f"capacity 300 {mode}")
    PP._assert_same(got, R.oracle_nets(kw, desc, blobs, roots, carry, SIDX, st, sims), T, f"capacity 300 {mode}")
    assert got[1]["n_records"][:T].min() > 100 and got[1]["n_records"][T:].max() <= 13   # (net 0 fills its trees, nets 1 and 2 a corner)


# ---------------------------------------------------------------------------------------------------- 5. defaults and equal budgets


@pytest.mark.parametrize("ci", [0, 6], ids=["pendulum_2x256", "cartpole_2x128"])
def test_zero_and_capacity_budgets_give_the_table_bits(native, ci):
    """All budgets 0 (what every caller passed before the field had a meaning) and all budgets equal to the capacity: the bits of the
    same table without budgets."""
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    table = _table(N.net_settings(cfg))
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search(table)
    plain = _search(e, roots, carry)
    e.set_net_search(table, n_sims=[0] * K)
    zeros = _search(e, roots, carry)
    e.set_net_search(table, n_sims=[kw["n_sims"]] * K)
    full = _search(e, roots, carry)
    e.close()
    PP._assert_same(zeros, plain, T, "budgets 0")
    PP._assert_same(full, plain, T, "budgets = capacity")
    R.assert_root_counts(plain, [kw["n_sims"]] * K, T, carry, "no budgets")


# ---------------------------------------------------------------------------------------- 6. budgets change between searches, reuse


def test_budgets_change_between_searches_with_tree_reuse(native):
    """CartPole 2x128, capacity 8: budgets (8, 3, 1), every root moved to its most visited child with that child's count carried, then
    budgets (1, 8, 3) -- both searches against oracle engines created per search with those budgets and carries."""
    ci = 6
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, _ = PP._inputs(ci, T)
    kw = dict(kw, n_sims=8)
    st = N.net_settings(cfg)
    e = PP._population(native, kw, desc, blobs)
    first_sims, second_sims = [8, 3, 1], [1, 8, 3]
    carry0 = np.zeros(K * T, np.int32)
    e.set_net_search(_table(st), n_sims=first_sims)
    first = _search(e, roots, carry0, SIDX)
    R.assert_root_counts(first, first_sims, T, carry0, "first search")
    PP._assert_same(first, R.oracle_nets(kw, desc, blobs, roots, carry0, SIDX, st, first_sims), T, "first search")
    child_n, child_state = first[2]
    pick = first[0]["counts"].argmax(axis=1)
    rows = np.arange(K * T)
    assert (child_n[rows, pick] >= 0).all()
    roots2 = np.ascontiguousarray(child_state[rows, pick])
    carry2 = child_n[rows, pick].astype(np.int32)
    assert carry2[:T].max() > carry2[2 * T:].max()   # (the carried counts are the budgets' too: at most 8 / 3 / 1)
    # (discrete trees: the root's children are records 1 .. A; a chosen child that ended its episode is no root: that tree starts over)
    alive = (first[1]["node_flags"][rows, 1 + pick] & 2) == 0
    assert alive.sum() > K * T // 2
    roots2[~alive], carry2[~alive] = roots[~alive], 0
    e.set_net_search(_table(st), n_sims=second_sims)
    second = _search(e, roots2, carry2, SIDX + 1)
    e.close()
    R.assert_root_counts(second, second_sims, T, carry2, "second search")
    PP._assert_same(second, R.oracle_nets(kw, desc, blobs, roots2, carry2, SIDX + 1, st, second_sims), T, "second search")


# --------------------------------------------------------------------------------------------------------- 7. self-play with budgets


@pytest.mark.parametrize("game", ["CartPole-v0", "Pendulum-v0"])
def test_selfplay_with_budgets(native, game):
    """PopulationSelfPlay(net_rollouts=...): 6 steps, episodes of at most 4 steps (they reset): net k's rows, finished returns and env
    states are those of a one-net DeviceSelfPlay created with net k's budget, its settings and tree_id_base + k*19."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from alphazero_gym_amd import run
    from selfplay_train import build_agent
    nets = []
    for s in range(K):
        torch.manual_seed(60 + s)
        nets.append(build_agent(game, [64, 64], 20, "cuda:0", 1e-3)[0].nn)
    shared = dict(c_uct=1.5 if game.startswith("Cart") else 0.1, gamma=1.0, epsilon=0.0)
    st = [dict(shared), dict(c_uct=shared["c_uct"] * 4.0, gamma=0.9, epsilon=0.25), dict(c_uct=shared["c_uct"] * 0.25, gamma=0.97)]
    sims = R.budgets(20)
    kw = dict(game=game, max_episode_length=4, capacity_steps=6, seed=11)
    pop = run.PopulationSelfPlay(nets, games_per_net=T, net_settings=st, net_rollouts=sims, tree_id_base=0, n_rollouts=20, **dict(kw, **shared))
    rows = pop.collect(6)
    assert pop.engine.search_info()["kernel_name"].startswith("search_kernel_nets<")
    fsum, fcnt, state = pop.engine.selfplay_stats()
    width = pop.engine.kmax
    pop.close()
    assert fcnt.sum() > 0   # episodes ended (and reset) inside the window
    for k in range(K):
        one = run.DeviceSelfPlay(nets[k], n_games=T, rank=k, n_rollouts=sims[k], **dict(kw, **dict(shared, **st[k])))
        r = one.collect(6)
        sf, sc, ss = one.engine.selfplay_stats()
        own = one.engine.kmax
        one.close()
        sl = slice(k * T, (k + 1) * T)
        assert torch.equal(_narrow_rows(rows[k], width, own), r), f"net {k} rows"
        np.testing.assert_array_equal(fsum[sl], sf, err_msg=f"net {k} fsum")
        np.testing.assert_array_equal(fcnt[sl], sc, err_msg=f"net {k} fcnt")
        np.testing.assert_array_equal(state[sl], ss, err_msg=f"net {k} env state")
    assert not torch.equal(rows[0], rows[1])


def _narrow_rows(rows, width, own):
    """Replay rows [obs | actions[width] | counts[width] | Q[width] | V] of an engine `width` children wide as an engine `own` wide
    writes them; the columns dropped must be empty slots."""
    if own == width:
        return rows
    import torch
    obs = rows.shape[1] - 3 * width - 1
    blocks = [rows[:, obs + j * width: obs + (j + 1) * width] for j in range(3)]
    assert all((b[:, own:] == 0).all() for b in blocks)
    return torch.cat([rows[:, :obs]] + [b[:, :own] for b in blocks] + [rows[:, -1:]], dim=1)


# ------------------------------------------------------------------------------------------------------------------ 8. invalid budgets


def test_invalid_budgets(native):
    """-1 and capacity + 1 on net 1: AZG_E_INVALID naming net 1; the next search gives the previous table's bits."""
    ci = 0
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    table, sims = _table(N.net_settings(cfg)), R.budgets(kw["n_sims"])
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search(table, n_sims=sims)
    before = _search(e, roots, carry)
    for bad in (-1, kw["n_sims"] + 1):
        with pytest.raises(_capi.EngineError) as ei:
            e.set_net_search(table, n_sims=[sims[0], bad, sims[2]])
        assert ei.value.code == AZG_E_INVALID and "net 1" in str(ei.value) and "n_sims" in str(ei.value), str(ei.value)
        PP._assert_same(_search(e, roots, carry), before, T, f"after the refused budget {bad}")
    arr = (_capi.AzgNetSearch * K)()
    for k in range(K):
        arr[k].struct_size = C.sizeof(_capi.AzgNetSearch)
        for key, v in table[k].items():
            setattr(arr[k], key, float(v))
        arr[k].n_sims = -5 if k == 1 else 0
    assert native.fns()["set_net_search"](e._h, arr, K) == AZG_E_INVALID
    R.assert_root_counts(before, sims, T, carry, "the table that stayed")
    e.close()
