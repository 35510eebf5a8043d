"""GPU (-m gpu): per-net MCTS settings in one search launch (azg_set_net_search, search_kernel_nets).

A K-net engine whose nets carry their own c_uct / gamma / epsilon (/ c_pw / kappa) must compute, bit for bit, what K oracle engines
compute -- net k CREATED with its settings, its own weights and tree_id_base + k*T: results, root children and every record of every
tree.  The matrix takes every parity_util.CONFIGS row a population runs at widths <= 256; the forced variants re-run one row per env
family on the other kernel shapes; then tables of equal entries, tables changed between searches, nets of different widening, device
self-play, and the refusals."""
import functools
import re

import numpy as np
import pytest

import net_search_util as N
import oracle_lib as O
import parity_util as P
import test_population_parity as PP
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

K, T, SIDX = PP.K, 19, PP.SIDX   # 19 trees per net: a full 16-tree workgroup and a ragged one; 8 + 8 + 3 under half-filled tiles
AZG_E_INVALID, AZG_E_UNSUPPORTED = _capi.AZG_E_INVALID, _capi.AZG_E_UNSUPPORTED


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _nets_args(info):
    m = re.fullmatch(r"search_kernel_nets<(.*)>", info["kernel_name"])
    assert m, info["kernel_name"]
    return [a.strip() for a in m.group(1).split(",")]


def _ran_shape(info):
    args = _nets_args(info)
    return dict(HP=int(args[1]), nreg=int(args[2]), tree_storage=info["tree_storage"], waves=info["waves"], groups=info["groups"],
                tile_trees=info["tile_trees"], spec=info["spec"])


def _search(e, roots, carry, sidx=SIDX):
    e.set_search_index(sidx)
    e.search(roots, carry)
    return PP._collect(e)


@functools.lru_cache(maxsize=2)
def _want(ci, trees):
    kw, desc, blobs, roots, carry = PP._inputs(ci, trees)
    return N.oracle_nets(kw, desc, blobs, roots, carry, SIDX, N.net_settings(P.CONFIGS[ci]), width=None if kw["mode"] == 0 else
                         N.kmax_of(N.shared_settings(P.CONFIGS[ci]), kw["n_sims"]))


def _run_row(native, ci, variant, monkeypatch):
    cfg = P.CONFIGS[ci]
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    want_shape = dict(PP._shape(cfg, "no_spec" if variant == "default" else variant), spec=0)
    trees = 35 if want_shape["groups"] == 2 else T
    kw, desc, blobs, roots, carry = PP._inputs(ci, trees)
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search([N.full(s) for s in N.net_settings(cfg)])
    got = _search(e, roots, carry)
    info = e.search_info()
    e.close()
    PP._assert_same(got, _want(ci, trees), trees, f"cfg{ci}-{variant}")
    shape = _ran_shape(info)
    print(f"cfg{ci}-{variant}: K={K} T={trees} {shape} {info['last_ms']:.3f} ms")
    assert info["kernel_form"] == "persistent" and shape == want_shape, (variant, shape, want_shape)
    tpw = shape["tile_trees"] * shape["groups"]
    assert -(-trees // tpw) >= 2 and trees % tpw != 0, (trees, tpw)
    if cfg[1] == 0:
        np.testing.assert_array_equal(got[1]["node_n"][:, 0], carry + cfg[4])   # carried root counts


# ------------------------------------------------------------------------------------------------------------------- 1. the matrix


@pytest.mark.parametrize("ci", N.matrix_rows(), ids=lambda ci: f"cfg{ci}")
def test_three_nets_three_settings_bit_exact_vs_oracle(native, ci, monkeypatch):
    """Every row, K = 3 nets of distinct weights AND distinct settings in one launch of search_kernel_nets on the shape the general
    kernels take for the row."""
    _run_row(native, ci, "default", monkeypatch)


# --------------------------------------------------------------------------------------------------------------- 2. forced variants

FORCED = ["global_tree", "stream_weights", "waves4", "groups2", "tile16", "trace_cap1"]
# one row per family: Pendulum 2x256, CartPole 2x128, MountainCar 2x64, MountainCarContinuous 2x64 and 2x256, Acrobot 2x64, the mixture row, the LayerNorm row
FORCED_ROWS = [0, 6, 26, 31, 32, 37, 16, 13]


def _forced_cases():
    cases = []
    for ci in FORCED_ROWS:
        cfg = P.CONFIGS[ci]
        for v in FORCED:
            same = v != "trace_cap1" and PP._shape(cfg, v) == PP._shape(cfg, "default")
            if not (P.moot(cfg, v) or same):
                cases.append(pytest.param(ci, v, id=f"cfg{ci}-{v}"))
    return cases


@pytest.mark.parametrize("ci,variant", _forced_cases())
def test_forced_variants(native, ci, variant, monkeypatch):
    _run_row(native, ci, variant, monkeypatch)


def test_forced_variants_cover_every_variant_and_family():
    seen_v = {p.values[1] for p in _forced_cases()}
    seen_env = {P.CONFIGS[p.values[0]][0] for p in _forced_cases()}
    assert seen_v == set(FORCED) and seen_env == {0, 2, 3, 4, 5}, (seen_v, seen_env)


# ----------------------------------------------------------------------------------------------------------------- 3. equal entries


@pytest.mark.parametrize("ci", [0, 6, 1], ids=["pendulum_2x256", "cartpole_2x128", "pendulum_2x256_eps"])
def test_equal_entries_give_the_shared_settings_bits(native, ci):
    """A table whose entries all equal azg_config's settings: the bits of the same population without a table -- from another kernel."""
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    e = PP._population(native, kw, desc, blobs)
    plain = _search(e, roots, carry)
    plain_name = e.search_info()["kernel_name"]
    e.set_net_search([N.full(N.shared_settings(cfg))] * K)
    tabled = _search(e, roots, carry)
    tabled_name = e.search_info()["kernel_name"]
    e.close()
    PP._assert_same(tabled, plain, T, "equal entries")
    assert plain_name.startswith("search_kernel<") and tabled_name.startswith("search_kernel_nets<"), (plain_name, tabled_name)


# -------------------------------------------------------------------------------------------------------- 4. change between searches


@pytest.mark.parametrize("ci", [6, 2], ids=["cartpole_2x128", "pendulum_v0_3x128"])
def test_table_changes_between_searches(native, ci):
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    width = None if kw["mode"] == 0 else N.kmax_of(N.shared_settings(cfg), kw["n_sims"])
    st = N.net_settings(cfg)
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search([N.full(s) for s in st])
    first = _search(e, roots, carry)
    PP._assert_same(first, N.oracle_nets(kw, desc, blobs, roots, carry, SIDX, st, width), T, "first table")
    st2 = [st[0], dict(st[1], c_uct=st[1]["c_uct"] * 0.1, gamma=0.93), st[2]]
    e.set_net_search([N.full(s) for s in st2])
    second = _search(e, roots, carry)
    PP._assert_same(second, N.oracle_nets(kw, desc, blobs, roots, carry, SIDX, st2, width), T, "net 1 changed")
    for k in (0, 2):
        sl = slice(k * T, (k + 1) * T)
        for key in first[1]:
            np.testing.assert_array_equal(first[1][key][sl], second[1][key][sl], err_msg=f"net {k} {key}")
    sl = slice(T, 2 * T)
    assert not np.array_equal(first[1]["edge_n"][sl], second[1]["edge_n"][sl])
    # back to the shared settings: the engine's own kernel and the plain population oracle
    e.set_net_search(None)
    third = _search(e, roots, carry)
    assert e.search_info()["kernel_name"].startswith("search_kernel<")
    PP._assert_same(third, PP._oracle(kw, desc, blobs, roots, carry, SIDX), T, "table cleared")
    e.close()


def test_resplit_clears_the_table(native):
    """45 trees: a table for 3 nets, then azg_set_population(5): the five nets search with the shared settings."""
    ci = 6
    kw, desc, blobs, roots, carry = PP._inputs(ci, 15, nets=3)
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search([N.full(s) for s in N.net_settings(P.CONFIGS[ci])])
    _search(e, roots, carry)
    assert e.search_info()["kernel_name"].startswith("search_kernel_nets<")
    kw5, desc, blobs5, roots5, carry5 = PP._inputs(ci, 9, nets=5)
    e.set_population(5)
    for k in range(5):
        e.set_net_weights(k, desc, blobs5[k])
    got = _search(e, roots5, carry5)
    assert e.search_info()["kernel_name"].startswith("search_kernel<")
    PP._assert_same(got, PP._oracle(kw5, desc, blobs5, roots5, carry5, SIDX), 9, "after the resplit")
    with pytest.raises(_capi.EngineError) as ei:   # (a table for the old split no longer fits)
        e.set_net_search([N.full(s) for s in N.net_settings(P.CONFIGS[ci])])
    assert ei.value.code == AZG_E_INVALID
    e.close()


# ----------------------------------------------------------------------------------------------------------- 5. differing widening


@pytest.mark.parametrize("widest", [(1.4, 0.5), (2.5, 0.7)], ids=["kmax10_lds", "kmax39_global"])
def test_nets_of_different_widening(native, widest):
    """Continuous mode, three different Kmax, the largest in net 1: every net's first Kmax_k result columns are its own engine's, the
    others empty slots; every tree record identical."""
    ci = 3   # Pendulum-v1, one hidden layer of 64, 50 simulations
    cfg = P.CONFIGS[ci]
    kw, desc, blobs, roots, carry = PP._inputs(ci, T)
    st = [dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5),
          dict(c_uct=0.2, gamma=0.97, epsilon=0.0, c_pw=widest[0], kappa=widest[1]),
          dict(c_uct=0.05, gamma=1.0, epsilon=0.1, c_pw=0.6, kappa=0.45)]
    kmaxes = [N.kmax_of(s, kw["n_sims"]) for s in st]
    assert kmaxes[1] == max(kmaxes) and len(set(kmaxes)) == 3, kmaxes
    assert _capi.widest_pw(st, kw["n_sims"]) == widest
    kw = dict(kw, c_pw=widest[0], kappa=widest[1])
    e = PP._population(native, kw, desc, blobs)
    assert e.kmax == kmaxes[1]
    e.set_net_search(st)
    got = _search(e, roots, carry)
    e.close()
    PP._assert_same(got, N.oracle_nets(kw, desc, blobs, roots, carry, SIDX, st, width=kmaxes[1]), T, f"widening {kmaxes}")
    for k in range(K):   # (what oracle_nets filled in, said once more in the open)
        sl = slice(k * T, (k + 1) * T)
        assert got[0]["n_children"][sl].max() <= kmaxes[k]
        assert (got[0]["counts"][sl, kmaxes[k]:] == 0).all() and (got[2][0][sl, kmaxes[k]:] == -1).all()


# --------------------------------------------------------------------------------------------------------------------- 6. self-play


@pytest.mark.parametrize("game", ["CartPole-v0", "Pendulum-v0"])
def test_selfplay_with_a_table(native, game):
    """PopulationSelfPlay(net_settings=...): 6 steps, episodes of at most 4 steps (they reset): net k's rows, finished returns and env
    states are those of a one-net DeviceSelfPlay with net k's settings and tree_id_base + k*19."""
    import os
    import sys

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
    kw = dict(game=game, n_rollouts=20, max_episode_length=4, capacity_steps=6, seed=11)
    pop = run.PopulationSelfPlay(nets, games_per_net=T, net_settings=st, tree_id_base=0, **dict(kw, **shared))
    rows = pop.collect(6)
    assert pop.engine.search_info()["kernel_name"].startswith("search_kernel_nets<")
    fsum, fcnt, state = pop.engine.selfplay_stats()
    pop.close()
    assert fcnt.sum() > 0   # episodes ended (and reset) inside the window
    for k in range(K):
        one = run.DeviceSelfPlay(nets[k], n_games=T, rank=k, **dict(kw, **dict(shared, **st[k])))
        r = one.collect(6)
        sf, sc, ss = one.engine.selfplay_stats()
        one.close()
        sl = slice(k * T, (k + 1) * T)
        assert torch.equal(rows[k], r), f"net {k} rows"
        np.testing.assert_array_equal(fsum[sl], sf, err_msg=f"net {k} fsum")
        np.testing.assert_array_equal(fcnt[sl], sc, err_msg=f"net {k} fcnt")
        np.testing.assert_array_equal(state[sl], ss, err_msg=f"net {k} env state")
    assert not torch.equal(rows[0], rows[1])


# --------------------------------------------------------------------------------------------------------------------- 7. refusals


def test_wide_population_with_a_table_is_refused(native):
    """2x512 nets: the table is accepted (the width is the weights'), the search returns AZG_E_UNSUPPORTED and launches nothing."""
    kw = dict(env_id=2, mode=1, n_trees=64, n_sims=10, c_uct=0.05, gamma=1.0, seed=3)
    desc = _capi.make_desc(3, [512, 512], 2, "elu")
    e = native.HipEngine(**kw)
    e.set_population(2)
    for k in range(2):
        e.set_net_weights(k, desc, O.make_weights(5 + k, 3, [512, 512], 2))
    e.set_net_search([dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5), dict(c_uct=0.2, gamma=0.9, epsilon=0.0, c_pw=1.0, kappa=0.5)])
    roots = e.synthetic_roots()
    with pytest.raises(_capi.EngineError) as ei:
        e.search(roots)
    assert ei.value.code == AZG_E_UNSUPPORTED and "256" in str(ei.value) and "azg_set_net_search" in str(ei.value)
    assert e.search_info()["kernel_form"] == "none"   # nothing was launched
    e.set_net_search(None)
    e.search(roots)                                    # the shared settings still search
    assert e.search_info()["kernel_form"] != "none"
    e.close()


def test_invalid_tables(native):
    import ctypes as C
    kw = dict(env_id=2, mode=1, n_trees=6, n_sims=20, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=3)
    e = native.HipEngine(**kw)
    e.set_population(3)
    ok = dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)

    def code(entries):
        with pytest.raises(_capi.EngineError) as ei:
            e.set_net_search(entries)
        return ei.value.code, str(ei.value)

    assert code([ok] * 2)[0] == AZG_E_INVALID                                  # wrong n_nets
    assert code([ok, dict(ok, c_pw=0.0), ok])[0] == AZG_E_INVALID              # c_pw <= 0
    assert code([ok, ok, dict(ok, c_uct=float("nan"))])[0] == AZG_E_INVALID    # NaN
    assert code([ok, ok, dict(ok, kappa=float("nan"))])[0] == AZG_E_INVALID
    c, msg = code([ok, ok, dict(ok, c_pw=3.0, kappa=0.9)])                     # 3 * 20^0.9 = 45 children > the engine's 5
    assert c == AZG_E_INVALID and "net 2" in msg and str(e.kmax) in msg, msg
    arr = (_capi.AzgNetSearch * 3)()
    for k in range(3):
        arr[k].struct_size = C.sizeof(_capi.AzgNetSearch) - (4 if k == 1 else 0)   # wrong struct_size
        arr[k].c_uct, arr[k].gamma, arr[k].c_pw, arr[k].kappa = 0.05, 1.0, 1.0, 0.5
    assert native.fns()["set_net_search"](e._h, arr, 3) == AZG_E_INVALID
    e.set_net_search([ok] * 3)   # (and a valid table still goes in)
    e.close()
