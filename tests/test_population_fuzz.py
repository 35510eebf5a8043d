"""GPU (-m gpu): seeded random populations with a per-net table (settings AND simulation budgets), bit for bit against the CPU oracle.

tests/population_fuzz.py draws the cases -- env, network, K nets x T trees, each net's c_uct / gamma / epsilon / widening law / budget,
a forced kernel variant -- and computes what the population must give: net k on an oracle engine CREATED with its settings, its budget,
its weights and tree_id_base + k*T.  What the 48 seeds cover is asserted on the CPU in test_population_fuzz_host.py.  Here: (a) every
seed, one search; (b) eight seeds search a second time with the budgets rotated by one net; (c) budgets that put the 16-level path
boundary at a different depth for each net of one launch; (d) device self-play over six random populations against one-net engines
created with each net's budget and settings."""
import functools

import numpy as np
import pytest

import deep_paths as D
import net_rollouts_util as R
import net_search_util as N
import parity_util as P
import population_fuzz as F
import test_population_net_rollouts as NR
import test_population_net_search as NS
import test_population_net_search_wide as NSW
import test_population_parity as PP
import test_population_wide as W

pytestmark = pytest.mark.gpu

FORCING = tuple(sorted({v[0] for v in P.VARIANT_ENV.values()} | set(W.FORCING)))


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


@pytest.fixture(autouse=True)
def _no_forcing(monkeypatch):
    for var in FORCING:
        monkeypatch.delenv(var, raising=False)


def _force(monkeypatch, variant):
    if variant != "default":
        monkeypatch.setenv(*P.VARIANT_ENV[variant])


def _engine(native, kw, desc, blobs):
    """K == 1: a plain engine with a table of one entry (net_T = B); else a population."""
    if len(blobs) == 1:
        e = native.HipEngine(**kw)
        e.set_weights(desc, blobs[0])
        return e
    return PP._population(native, kw, desc, blobs)


def _search(e, roots, carry, sidx):
    e.set_search_index(sidx)
    e.search(roots, carry)
    return PP._collect(e)


def _assert_form(c, info, what):
    """A table form ran, and the one the variant names (as far as the files of the fixed matrices know how to tell)."""
    name = info["kernel_name"]
    assert "_nets<" in name, (what, name)
    if not c.wide:
        assert info["kernel_form"] == "persistent" and name.startswith("search_kernel_nets<"), (what, info)
        shape = NS._ran_shape(info)
        want = dict(PP._shape(c.cfg, "no_spec" if c.variant == "default" else c.variant), spec=0)
        key = {"global_tree": "tree_storage", "stream_weights": "nreg", "waves8": "waves", "groups2": "groups", "tile8": "tile_trees"}.get(c.variant)
        if key:
            assert shape[key] == want[key], (what, key, shape, want)
        assert shape["spec"] == 0 and shape["HP"] == want["HP"], (what, shape, want)
    elif c.lockstep and c.variant in ("default", "global_tree"):
        if c.kmax <= 16:     # (more than 16 children per node: the trees leave LDS whatever is forced)
            NSW._assert_table_form(info, c.cfg, what, global_tree=c.variant == "global_tree")
        else:
            assert info["kernel_form"] in ("team", "per_layer"), (what, info)
    elif c.lockstep and c.variant == "launches":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0 and name.startswith("ls_tree_kernel_nets<"), (what, info)
    else:
        assert info["kernel_form"] == "persistent" and name.startswith("search_kernel_nets<"), (what, info)
        if c.variant == "global_tree":
            assert info["tree_storage"] == "global", (what, info)


def run_case(native, c, monkeypatch=None, second=False):
    """One search of case c on the device against the oracle; second: then the budgets rotated by one net under a new search index,
    on the same engine, against fresh oracle engines.  Returns the first search's search_info."""
    if monkeypatch is not None:
        _force(monkeypatch, c.variant)
    what = F.describe(c)
    e = _engine(native, c.kw, c.desc, c.blobs)
    try:
        e.set_net_search(F.table(c), wide=c.wide, n_sims=c.budgets)
        got = _search(e, c.roots, c.carry, c.sidx)
        info = e.search_info()
        R.assert_root_counts(got, c.sims, c.T, c.carry, what)
        PP._assert_same(got, F.oracle(c), c.T, what)
        _assert_form(c, info, what)
        if second:
            raw, sims = F.rotated(c)
            e.set_net_search(F.table(c), wide=c.wide, n_sims=raw)
            again = _search(e, c.roots, c.carry, c.sidx + 7)
            R.assert_root_counts(again, sims, c.T, c.carry, what + " rotated")
            PP._assert_same(again, F.oracle(c, sims=sims, sidx=c.sidx + 7), c.T, what + " rotated")
            assert "_nets<" in e.search_info()["kernel_name"]
    finally:
        e.close()
    return info


# ------------------------------------------------------------------------------------------------------------- a. every seed


@pytest.mark.parametrize("seed", F.SEEDS)
def test_random_population_bit_exact_vs_oracle(native, seed, monkeypatch):
    """Every result, root child and record of every tree of case(seed), on a table form of the kernel its variant names.  (A scratch
    build whose search_kernel_nets keeps the capacity as its loop bound fails 32 of these 48 seeds; one that takes a net's widening row at
    k * (its own budget + 2) fails 13.)"""
    c = F.case(seed)
    info = run_case(native, c, monkeypatch)
    print(f"{F.describe(c)}: {info['kernel_form']} {info['kernel_name']} {info['last_ms']:.3f} ms")


# ------------------------------------------------------------------------------------------------------------- b. a second search


@pytest.mark.parametrize("seed", F.second_search_seeds())
def test_second_search_with_rotated_budgets(native, seed, monkeypatch):
    """The table is uploaded again and the largest budget (the per-layer launches' step count) found again: the second search runs
    net k with net k-1's budget."""
    run_case(native, F.case(seed), monkeypatch, second=True)


# --------------------------------------------------------------------------------------- c. budgets across the 16-level boundary


@functools.lru_cache(maxsize=2)
def _boundary_want(shape):
    return F.boundary_oracle({"p64": "p64-lds", "p512": "p512-team"}[shape])


@pytest.mark.parametrize("name", sorted(F.BOUNDARY))
def test_chain_budgets_across_the_16_level_boundary(native, name, monkeypatch):
    """Four nets under the chain law with budgets 15, 16, 17 and 33 at capacity 40: paths that stay inside the lanes' 16 levels, fill them,
    hand the 16th return over and take backup_from's second round, in one launch (test_population_fuzz_host.py asserts the depths)."""
    kw, desc, blobs, roots, settings, sims, T, variant = F.boundary_case(name)
    _force(monkeypatch, variant)
    wide = max(D.SHAPES[F.BOUNDARY[name][0]]["hidden"]) >= 512
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search([N.full(s) for s in settings], wide=wide, n_sims=sims)
    got = _search(e, roots, None, D.SIDX)
    info = e.search_info()
    e.close()
    R.assert_root_counts(got, sims, T, None, name)
    PP._assert_same(got, _boundary_want(F.BOUNDARY[name][0]), T, name)
    assert (got[1]["n_records"].reshape(4, T) == np.array(sims)[:, None] + 1).all()
    if name == "p64-lds":
        assert info["kernel_name"].startswith("search_kernel_nets<") and info["tree_storage"] == "lds8", info
    elif name == "p64-global_tree":
        assert info["kernel_name"].startswith("search_kernel_nets<") and info["tree_storage"] == "global", info
    elif name == "p512-team":
        NSW._assert_table_form(info, (2, 1, [512, 512], "elu", F.BOUNDARY_CAP, {}), name)
    elif name == "p512-launches":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0 and info["kernel_name"].startswith("ls_tree_kernel_nets<"), info
    else:
        assert info["kernel_form"] == "persistent" and info["kernel_name"].startswith("search_kernel_nets<"), info


def test_discrete_budgets_across_the_16_level_boundary(native):
    """CartPole on the balancing line: net 0 stops below level 16, net 1 goes beyond it, net 2 runs the capacity."""
    kw, desc, blobs, roots, carry, settings, sims, T = F.discrete_boundary_case()
    e = PP._population(native, kw, desc, blobs)
    e.set_net_search([N.full(s) for s in settings], n_sims=sims)
    got = _search(e, roots, carry, 3)
    info = e.search_info()
    e.close()
    R.assert_root_counts(got, sims, T, carry, "discrete boundary")
    PP._assert_same(got, F.discrete_boundary_oracle(), T, "discrete boundary")
    assert info["kernel_name"].startswith("search_kernel_nets<"), info


# ------------------------------------------------------------------------------------------------------------------ d. self-play


@pytest.mark.parametrize("seed", F.SELFPLAY_SEEDS)
def test_selfplay_over_a_random_population(native, seed):
    """PopulationSelfPlay(net_settings=..., net_rollouts=...) for four steps, episodes of at most three (they reset): net k's rows,
    finished returns and env states are those of a one-net DeviceSelfPlay created with net k's budget and settings."""
    import torch
    from alphazero_gym_amd import run
    sp = F.selfplay_case(seed)
    nets = F.selfplay_policies(sp, "cuda:0")
    steps = F.SELFPLAY_STEPS
    kw = dict(game=sp.game, max_episode_length=F.SELFPLAY_MAX_LEN, capacity_steps=steps, seed=sp.engine_seed, V_target_policy=sp.v_target, **sp.rule)
    pop = run.PopulationSelfPlay(nets, games_per_net=sp.T, net_settings=sp.settings, net_rollouts=sp.sims, tree_id_base=0, n_rollouts=sp.cap,
                                 **dict(kw, **sp.shared))
    rows = pop.collect(steps)
    assert pop.engine.search_info()["kernel_name"].startswith("search_kernel_nets<")
    fsum, fcnt, state = pop.engine.selfplay_stats()
    width = pop.engine.kmax
    pop.close()
    assert fcnt.sum() > 0   # episodes ended (and reset) inside the window
    for k in range(sp.K):
        one = run.DeviceSelfPlay(nets[k], n_games=sp.T, rank=k, n_rollouts=sp.sims[k], **dict(kw, **dict(sp.shared, **sp.settings[k])))
        r = one.collect(steps)
        sf, sc, ss = one.engine.selfplay_stats()
        own = one.engine.kmax
        one.close()
        sl = slice(k * sp.T, (k + 1) * sp.T)
        assert torch.equal(NR._narrow_rows(rows[k], width, own), r), f"seed {seed} net {k} rows"
        np.testing.assert_array_equal(fsum[sl], sf, err_msg=f"net {k} fsum")
        np.testing.assert_array_equal(fcnt[sl], sc, err_msg=f"net {k} fcnt")
        np.testing.assert_array_equal(state[sl], ss, err_msg=f"net {k} env state")
