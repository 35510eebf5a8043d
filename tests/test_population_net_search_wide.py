"""GPU (-m gpu): per-net MCTS settings at padded widths >= 512 (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE), bit for bit against
the CPU oracle.

A K-net engine whose nets carry their own c_uct / gamma / epsilon / c_pw / kappa must compute what K oracle engines compute -- net k
CREATED with its settings, its own weights and tree_id_base + k*T: results, root children and every record of every tree -- on the team
kernel (ls_team_kernel_nets), the per-layer launches (ls_tree_kernel_nets) and the wide one-launch kernel (search_kernel_nets at widths
512 and 1024).  Then tables of equal entries, a table changed between searches, one net with a table, device self-play, and the ABI's
rules.  (The team kernel's time-out is not forced here: its fall-back runs the per-layer path the `launches` variant covers.)"""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

import net_search_util as N
import net_search_wide_util as NW
import oracle_lib as O
import parity_util as P
import test_population_wide as W
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

K, SIDX = NW.K, W.SIDX
AZG_E_INVALID, AZG_E_UNSUPPORTED = _capi.AZG_E_INVALID, _capi.AZG_E_UNSUPPORTED
ROW_2x512, ROW_4x1024 = 18, 20


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


@pytest.fixture(autouse=True)
def _no_forcing(monkeypatch):
    for var in W.FORCING:
        monkeypatch.delenv(var, raising=False)


@functools.lru_cache(maxsize=None)
def _want(row_key, T):
    return NW.oracle(ROWS[row_key], T)


ROWS = {NW.row_id(r): r for r in NW.matrix_rows()}


def _search(e, roots, carry, sidx=SIDX):
    e.set_search_index(sidx)
    e.search(roots, carry)
    return W._collect(e)


def _table(settings):
    return [N.full(s) for s in settings]


def _assert_table_form(info, row, what, global_tree=False):
    """The table variant of the form the row's shared-settings population runs: the team kernel's (32-tree teams, two per CU) -- or, where
    its workgroups were not all resident, the per-layer launches' after one counted fall-back."""
    cfg = NW.cfg_of(row)
    hp = -(-max(cfg[2]) // 64) * 64
    if info["kernel_form"] == "team":
        m = re.fullmatch(r"ls_team_kernel_nets<(.*)>", info["kernel_name"])
        assert m, (what, info)
        a = [x.strip() for x in m.group(1).split(",")]
        assert a[1] == str(hp) and a[3] == ("0" if global_tree else "1") and a[4:] == ["2", "2"], (what, info)
        assert info["team_trees"] == 32 and info["team_parts"] == 1, (what, info)
    else:
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] >= 1, (what, info)
        assert info["kernel_name"].startswith("ls_tree_kernel_nets<"), (what, info)


# ------------------------------------------------------------------------------------------------------------------- 1. the matrix


@pytest.mark.parametrize("row,variant", NW.cases(), ids=[f"{NW.row_id(r)}-{v}" for r, v in NW.cases()])
def test_three_wide_nets_three_settings_bit_exact_vs_oracle(native, row, variant, monkeypatch):
    """K = 3 nets of distinct weights AND distinct settings.  Lock-step shaped rows: 3 x 32 trees, one team per net, on the team kernel,
    the per-layer launches, the one-launch kernel and with global trees.  The other rows: 3 x 19 trees on the one-launch kernel."""
    cfg, T, ls = NW.cfg_of(row), NW.trees_per_net(row), NW.lockstep_shaped(row)
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    kw, desc, blobs, roots, carry = W._inputs(cfg, T)
    st = NW.net_settings(row)
    e = W._population(native, kw, desc, blobs)
    e.set_net_search(_table(st), wide=True)
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    what = f"{NW.row_id(row)}-{variant}"
    print(f"{what}: K={K} T={T} {info['kernel_form']} {info['kernel_name']} fallbacks {info['team_fallbacks']}")
    W._assert_same(got, _want(NW.row_id(row), T), T, what)
    hp = -(-max(cfg[2]) // 64) * 64
    if ls and variant in ("default", "global_tree"):
        _assert_table_form(info, row, what, global_tree=variant == "global_tree")
    elif ls and variant == "launches":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, (what, info)
        assert info["kernel_name"].startswith("ls_tree_kernel_nets<"), (what, info)
    else:
        assert info["kernel_form"] == "persistent", (what, info)
        assert info["kernel_name"].startswith("search_kernel_nets<") and f", {hp}, 0," in info["kernel_name"], (what, info)
        if variant == "global_tree":
            assert info["tree_storage"] == "global" and info["lds_exit"] == "forced", (what, info)
        if not ls:
            assert -(-T // 16) == 2 and T % 16 != 0
    if cfg[1] == 0:
        np.testing.assert_array_equal(got[1]["node_n"][:, 0], carry + cfg[4])   # carried root counts
    else:   # net 1 widens less than the engine: its remaining result columns are empty slots
        k0, k1 = N.kmax_of(st[0], kw["n_sims"]), N.kmax_of(st[1], kw["n_sims"])
        assert k1 < k0 and got[0]["counts"].shape[1] == k0
        assert got[0]["n_children"][T:2 * T].max() <= k1
        assert (got[0]["counts"][T:2 * T, k1:] == 0).all() and (got[2][0][T:2 * T, k1:] == -1).all()


# ----------------------------------------------------------------------------------------------------------------- 2. equal entries


@pytest.mark.parametrize("row", [ROW_2x512, ROW_4x1024], ids=["pendulum_2x512", "pendulum_4x1024"])
def test_equal_entries_give_the_shared_settings_bits(native, row):
    """A table whose entries all equal azg_config's settings: the bits of the same population without a table -- from another kernel."""
    cfg, T = NW.cfg_of(row), 32
    kw, desc, blobs, roots, carry = W._inputs(cfg, T)
    e = W._population(native, kw, desc, blobs)
    plain = _search(e, roots, carry)
    plain_info = e.search_info()
    e.set_net_search(_table([N.shared_settings(cfg)] * K), wide=True)
    tabled = _search(e, roots, carry)
    tabled_info = e.search_info()
    e.close()
    W._assert_same(tabled, plain, T, "equal entries")
    W._assert_team_or_fell_back(plain_info, "no table")
    _assert_table_form(tabled_info, row, "equal entries")
    assert plain_info["kernel_name"] != tabled_info["kernel_name"]


# -------------------------------------------------------------------------------------------------------- 3. change between searches


def test_table_changes_between_searches(native):
    row, T = ROW_2x512, 32
    kw, desc, blobs, roots, carry = W._inputs(NW.cfg_of(row), T)
    st = NW.net_settings(row)
    e = W._population(native, kw, desc, blobs)
    e.set_net_search(_table(st), wide=True)
    first = _search(e, roots, carry)
    W._assert_same(first, _want(NW.row_id(row), T), T, "first table")
    st2 = [st[0], dict(st[1], c_uct=st[1]["c_uct"] * 0.1, gamma=0.93), st[2]]
    e.set_net_search(_table(st2), wide=True)
    second = _search(e, roots, carry)
    W._assert_same(second, NW.oracle(row, T, st2), T, "net 1 changed")
    for k in (0, 2):
        sl = slice(k * T, (k + 1) * T)
        for key in first[1]:
            assert first[1][key][sl].tobytes() == second[1][key][sl].tobytes(), f"net {k} {key}"
    assert not np.array_equal(first[1]["edge_n"][T:2 * T], second[1]["edge_n"][T:2 * T])
    e.set_net_search(None)          # back to the shared settings: the shared-settings kernel and the plain population oracle
    third = _search(e, roots, carry)
    W._assert_team_or_fell_back(e.search_info(), "table cleared")
    W._assert_same(third, W._oracle_case(row, T), T, "table cleared")
    e.close()


# ------------------------------------------------------------------------------------------------------------- 4. one net with a table


def test_one_net_with_a_table(native):
    """An engine of one net (no azg_set_population) with a table of one entry searches the population form (net_T = B): the bits of a
    one-net engine created with those settings."""
    row, T = ROW_2x512, 32
    kw, desc, blobs, roots, carry = W._inputs(NW.cfg_of(row), T, nets=1)
    s1 = NW.net_settings(row)[1]
    e = native.HipEngine(**kw)
    e.set_weights(desc, blobs[0])
    e.set_net_search(_table([s1]), wide=True)
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    _assert_table_form(info, row, "one net")
    W._assert_same(got, NW.oracle(row, T, [s1], nets=1), T, "one net with a table")


# --------------------------------------------------------------------------------------------------------------------- 5. self-play


def test_selfplay_with_a_wide_table(native):
    """PopulationSelfPlay(net_settings=..., net_settings_wide=True) on 2 x 32 games of Pendulum [512, 512]: 4 steps, episodes of at most 3
    steps (they reset): net k's rows, finished returns and env states are those of a one-net DeviceSelfPlay with net k's settings."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from alphazero_gym_amd import run
    from selfplay_train import build_agent
    game, T, steps = "Pendulum-v0", 32, 4
    nets = []
    for s in range(2):
        torch.manual_seed(60 + s)
        nets.append(build_agent(game, [512, 512], 10, "cuda:0", 1e-3)[0].nn)
    shared = dict(c_uct=0.1, gamma=1.0, epsilon=0.0)
    st = [dict(shared), dict(c_uct=shared["c_uct"] * 4.0, gamma=0.9, epsilon=0.25)]
    kw = dict(game=game, n_rollouts=10, max_episode_length=3, capacity_steps=steps, seed=11)
    pop = run.PopulationSelfPlay(nets, games_per_net=T, net_settings=st, net_settings_wide=True, tree_id_base=0, **dict(kw, **shared))
    rows = pop.collect(steps)
    info = pop.engine.search_info()
    fsum, fcnt, state = pop.engine.selfplay_stats()
    pop.close()
    _assert_table_form(info, ROW_2x512, "self-play")
    assert fcnt.sum() > 0   # episodes ended (and reset) inside the window
    for k in range(2):
        one = run.DeviceSelfPlay(nets[k], n_games=T, rank=k, **dict(kw, **st[k]))
        r = one.collect(steps)
        sf, sc, ss = one.engine.selfplay_stats()
        one.close()
        sl = slice(k * T, (k + 1) * T)
        assert torch.equal(rows[k], r), f"net {k} rows"
        np.testing.assert_array_equal(fsum[sl], sf, err_msg=f"net {k} fsum")
        np.testing.assert_array_equal(fcnt[sl], sc, err_msg=f"net {k} fcnt")
        np.testing.assert_array_equal(state[sl], ss, err_msg=f"net {k} env state")
    assert not torch.equal(rows[0], rows[1])


# --------------------------------------------------------------------------------------------------------------------------- 6. ABI


def _raw_table(settings):
    arr = (_capi.AzgNetSearch * len(settings))()
    for k, s in enumerate(settings):
        arr[k].struct_size = C.sizeof(_capi.AzgNetSearch)
        for key, v in N.full(s).items():
            setattr(arr[k], key, float(v))
    return arr


def _refused(e, roots, carry):
    with pytest.raises(_capi.EngineError) as ei:
        e.search(roots, carry)
    assert ei.value.code == AZG_E_UNSUPPORTED and "256" in str(ei.value) and "azg_set_net_search" in str(ei.value), str(ei.value)


def test_flags(native):
    """flags = 0 is azg_set_net_search: a wide engine still refuses at the search and launches nothing; unknown bits are
    AZG_E_INVALID and leave the table alone; the flag lets the search through; a later plain azg_set_net_search drops the permission."""
    row, T = ROW_2x512, 32
    kw, desc, blobs, roots, carry = W._inputs(NW.cfg_of(row), T)
    st = NW.net_settings(row)
    e = W._population(native, kw, desc, blobs)
    ex = native.fns()["set_net_search_ex"]
    arr = _raw_table(st)
    assert ex(e._h, arr, K, 0) == 0
    _refused(e, roots, carry)
    assert e.search_info()["kernel_form"] == "none"   # nothing was launched
    for bad in (2, 3, 1 << 31):
        assert ex(e._h, arr, K, bad) == AZG_E_INVALID
    _refused(e, roots, carry)                         # (the table and its missing permission are as they were)
    assert ex(e._h, arr, K, _capi.NET_SEARCH_WIDE) == 0
    got = _search(e, roots, carry)
    W._assert_same(got, _want(NW.row_id(row), T), T, "with the flag")
    assert ex(e._h, arr, K, 2) == AZG_E_INVALID       # a failed call keeps the table and the permission
    W._assert_same(_search(e, roots, carry), got, T, "after a failed call")
    e.set_net_search(_table(st))                      # plain azg_set_net_search: the permission goes
    _refused(e, roots, carry)
    assert ex(e._h, None, 0, _capi.NET_SEARCH_WIDE) == 0   # NULL / 0 clears the table
    third = _search(e, roots, carry)
    W._assert_team_or_fell_back(e.search_info(), "cleared")
    W._assert_same(third, W._oracle_case(row, T), T, "cleared")
    e.close()


def test_nine_bit_tree_size_takes_global_trees(native):
    """254 simulations: 256 records per tree, 9-bit ids -- the table variants exist for 8-bit ids and global trees, so the trees go to
    global memory, bit-exact."""
    T, nets = 32, 2
    cfg = (2, 1, [512, 512], "elu", 254, dict(c_uct=0.05, gamma=1.0))
    kw, desc, blobs, roots, carry = W._inputs(cfg, T, nets)
    st = NW.net_settings(cfg)[:nets]
    e = W._population(native, kw, desc, blobs)
    assert e.max_records == 256
    e.set_net_search(_table(st), wide=True)
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    _assert_table_form(info, cfg, "9-bit ids", global_tree=True)
    W._assert_same(got, N.oracle_nets(kw, desc, blobs, roots, carry, SIDX, st, width=N.kmax_of(st[0], 254)), T, "9-bit ids")
