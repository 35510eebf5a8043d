"""GPU (-m gpu): populations of wide nets (padded hidden width >= 512) against the CPU oracle, bit for bit.

Lock-step shaped nets (two or more hidden layers, no LayerNorm, at most four inputs) are searched by the team kernel / the per-layer
launches: every 32-tree team and tile pair reads the weights of the net its trees belong to (lockstep.cuh: ls_net_wofs), which needs a
multiple of 32 trees per net.  The other wide shapes (one hidden layer, six inputs, LayerNorm) run on the one-launch search kernel at
any number of trees per net.  The comparison is test_population_parity's: a K-net engine against K oracle engines with tree_id_base +
k*T, net k's weights and the same search index -- results(), dump_tree() and root_children() byte for byte."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

K = 3
BASE, SIDX = 77, 3      # tree_id_base, search index
VARIANTS = ["default", "launches", "persistent", "global_tree"]
FORCING = ("AZG_LS_TEAM", "AZG_FORCE_PERSISTENT", "AZG_FORCE_GLOBAL_TREE", "AZG_TEAM_SPIN_LIMIT", "AZG_TEAM_WIDE", "AZG_TEAM_TT")

PENDULUM_2x512 = next(i for i, c in enumerate(P.CONFIGS) if c[0] == 2 and c[2] == [512, 512])
PENDULUM_2x512_LN = (2, 1, [512, 512], "elu", 30, dict(c_uct=0.05, gamma=1.0, _ln=True))
NARROW = (2, 1, [64, 64], "elu", 30, dict(c_uct=0.05, gamma=1.0))


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


@pytest.fixture(autouse=True)
def _no_forcing(monkeypatch):
    for var in FORCING:
        monkeypatch.delenv(var, raising=False)


def _lockstep_shaped(cfg):
    _, _, hidden, _, _, _, _, ln = P.split_config(cfg)
    return _capi.lockstep_shaped(P.config_dims(cfg)[0], hidden, ln)


def _matrix():
    cases = []
    for ci, cfg in enumerate(P.CONFIGS):
        if max(cfg[2]) <= 256:
            continue                                           # (test_population_parity's rows)
        ls = _lockstep_shaped(cfg)
        for v in VARIANTS:
            # (the shapes that are not lock-step shaped run on the search kernel whatever is forced: `launches` and `persistent` would
            # re-run the default's kernel)
            if P.moot(cfg, v) or (not ls and v in ("launches", "persistent")):
                continue
            cases.append(pytest.param(ci, v, id=f"cfg{ci}-{v}"))
    return cases


CASES = _matrix()


def _cfg(c):
    return P.CONFIGS[c] if isinstance(c, int) else c


def _inputs(c, T, nets=K):
    """Engine kwargs, descriptor, one blob per net (distinct weights and LayerNorm parameters), roots and carried counts of a
    population of `nets` x T trees: every net's segment gets the configuration's hand-placed roots."""
    cfg = _cfg(c)
    env, mode, hidden, act, n_sims, extra, ncomp, ln = P.split_config(cfg)
    kw = dict(env_id=env, mode=mode, n_trees=nets * T, n_sims=n_sims, seed=1234, tree_id_base=BASE, **extra)
    desc = P.config_net(cfg, 99)[0]
    blobs = [P.config_net(cfg, 99 + k, ln_seed=7 + k)[1] for k in range(nets)]
    o = O.OracleEngine(**kw)
    roots = o.synthetic_roots()
    o.close()
    for k in range(nets):
        roots[k * T:(k + 1) * T] = P.config_roots(env, roots[k * T:(k + 1) * T])
    carry = (np.arange(nets * T) % 7).astype(np.int32) if mode == 0 else None
    return kw, desc, blobs, roots, carry


def _collect(e):
    return dict(e.results()), dict(e.dump_tree()), e.root_children()


def _one_net(cls, kw, desc, blob, roots, carry, sidx, k, T):
    """Net k's T trees on an engine of their own: tree_id_base + k*T, the population's search index."""
    e = cls(**dict(kw, n_trees=T, tree_id_base=kw.get("tree_id_base", 0) + k * T))
    e.set_weights(desc, blob)
    e.set_search_index(sidx)
    sl = slice(k * T, (k + 1) * T)
    e.search(roots[sl], None if carry is None else carry[sl])
    out = _collect(e)
    e.close()
    return out


def _concat(parts):
    res = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    dump = {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
    return res, dump, (np.concatenate([p[2][0] for p in parts]), np.concatenate([p[2][1] for p in parts]))


def _oracle(kw, desc, blobs, roots, carry, sidx):
    """K oracle engines, concatenated: what the population must compute."""
    T = kw["n_trees"] // len(blobs)
    return _concat([_one_net(O.OracleEngine, kw, desc, blobs[k], roots, carry, sidx, k, T) for k in range(len(blobs))])


@functools.lru_cache(maxsize=None)
def _oracle_case(ci, T, nets=K):
    kw, desc, blobs, roots, carry = _inputs(ci, T, nets)
    return _oracle(kw, desc, blobs, roots, carry, SIDX)


def _population(native, kw, desc, blobs):
    e = native.HipEngine(**kw)
    e.set_population(len(blobs))
    for k in range(len(blobs)):
        e.set_net_weights(k, desc, blobs[k])
    return e


def _search(native, kw, desc, blobs, roots, carry, sidx=SIDX):
    e = _population(native, kw, desc, blobs)
    e.set_search_index(sidx)
    e.search(roots, carry)
    got, info = _collect(e), e.search_info()
    e.close()
    return got, info


def _assert_same(got, want, T, what=""):
    (rg, dg, cg), (rw, dw, cw) = got, want
    assert set(rg) == set(rw) and set(dg) == set(dw)
    arrays = [("results " + k, rg[k], rw[k]) for k in rw] + [("dump " + k, dg[k], dw[k]) for k in dw]
    arrays += [("child_n", cg[0], cw[0]), ("child_state", cg[1], cw[1])]
    for name, a, b in arrays:
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        rows = [i for i in range(a.shape[0]) if a[i].tobytes() != b[i].tobytes()]
        msg = f"{what} {name}: trees {rows[:8]} of nets {sorted({i // T for i in rows})} differ"
        np.testing.assert_array_equal(a, b, err_msg=msg)


def _nets(x, T):
    """(results, dump, children) cut into per-net pieces."""
    n = x[2][0].shape[0] // T
    return [({k: v[i * T:(i + 1) * T] for k, v in x[0].items()}, {k: v[i * T:(i + 1) * T] for k, v in x[1].items()},
             (x[2][0][i * T:(i + 1) * T], x[2][1][i * T:(i + 1) * T])) for i in range(n)]


def _team_args(info):
    """ls_team_kernel<ENV, HP, GMM, tree storage, chunk, workgroups per CU, SPEC, trees per team, population form>"""
    m = re.fullmatch(r"ls_team_kernel<(.*)>", info["kernel_name"])
    assert m, info["kernel_name"]
    return [a.strip() for a in m.group(1).split(",")]


def _assert_team_or_fell_back(info, what, global_tree=False):
    """The default path of a lock-step shaped population: the team kernel's population form (32-tree teams, two per CU, general tree
    phases) -- or, where its workgroups were not all resident, the per-layer launches after one counted fall-back."""
    if info["kernel_form"] == "team":
        a = _team_args(info)
        assert a[4:] == ["2", "2", "0", "32", "true"] and info["team_trees"] == 32 and info["team_parts"] == 1, (what, info)
        assert a[3] == ("0" if global_tree else "1"), (what, info)
    else:
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] >= 1, (what, info)


# ---------------------------------------------------------------------------------------------------------------- 1. the matrix


@pytest.mark.parametrize("ci,variant", CASES)
def test_wide_population_bit_exact_vs_oracle(native, ci, variant, monkeypatch):
    """K = 3 nets of distinct weights on every wide row of the parity matrix.  Lock-step shaped rows: 3 x 32 trees -- an odd number of
    tile pairs, a last net, net boundaries that no coarser alignment hides -- on the team kernel, the per-layer launches, the one-launch
    kernel and with global trees.  The other rows: 3 x 24 trees on the search kernel, a full workgroup and a ragged one per net."""
    cfg = P.CONFIGS[ci]
    ls = _lockstep_shaped(cfg)
    T = 32 if ls else 24
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    got, info = _search(native, kw, desc, blobs, roots, carry)
    what = f"cfg{ci}-{variant}"
    print(f"{what}: K={K} T={T} {info['kernel_form']} {info['kernel_name']} fallbacks {info['team_fallbacks']}")
    _assert_same(got, _oracle_case(ci, T), T, what)
    if ls and variant in ("default", "global_tree"):
        _assert_team_or_fell_back(info, what, global_tree=variant == "global_tree")
    elif ls and variant == "launches":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, (what, info)
    else:
        assert info["kernel_form"] == "persistent", (what, info)
        assert info["kernel_name"].startswith("search_kernel<") and f", {-(-max(cfg[2]) // 64) * 64}, 0," in info["kernel_name"], (what, info)
        if variant == "global_tree":
            assert info["tree_storage"] == "global" and info["lds_exit"] == "forced", (what, info)
        if not ls:
            assert -(-T // 16) == 2 and T % 16 != 0
    if cfg[1] == 0:
        np.testing.assert_array_equal(got[1]["node_n"][:, 0], carry + cfg[4])   # carried root counts


def test_the_matrix_is_not_thin():
    by = {}
    for p in CASES:
        ci, v = p.values
        by.setdefault(ci, []).append(v)
    wide = [ci for ci, c in enumerate(P.CONFIGS) if max(c[2]) > 256]
    assert sorted(by) == wide and len(wide) == 7
    for ci, vs in by.items():
        assert vs == (VARIANTS if _lockstep_shaped(P.CONFIGS[ci]) else ["default", "global_tree"]), (ci, vs)
    assert sum(_lockstep_shaped(P.CONFIGS[ci]) for ci in wide) == 5


# ---------------------------------------------------------------------------------------------------------------- 2. two teams per net


@pytest.mark.parametrize("variant", ["default", "launches"])
def test_two_teams_per_net(native, variant, monkeypatch):
    """K = 2 nets x 64 trees of Pendulum [512, 512]: the net index is the team's first tree over net_T, not the team's index."""
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    kw, desc, blobs, roots, carry = _inputs(PENDULUM_2x512, 64, nets=2)
    got, info = _search(native, kw, desc, blobs, roots, carry)
    _assert_same(got, _oracle_case(PENDULUM_2x512, 64, 2), 64, variant)
    if variant == "default":
        _assert_team_or_fell_back(info, variant)
    else:
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, info


# ---------------------------------------------------------------------------------------------------------------- 3. wide LayerNorm


def test_wide_layernorm_population(native):
    """K = 3 x 24 trees of Pendulum [512, 512] with LayerNorm, every net with its own gamma and beta: not lock-step shaped, so the
    one-launch search kernel at any number of trees per net."""
    T = 24
    kw, desc, blobs, roots, carry = _inputs(PENDULUM_2x512_LN, T)
    got, info = _search(native, kw, desc, blobs, roots, carry)
    _assert_same(got, _oracle(kw, desc, blobs, roots, carry, SIDX), T, "layernorm")
    assert info["kernel_form"] == "persistent" and info["kernel_name"].startswith("search_kernel<2, 512, 0,"), info


# ---------------------------------------------------------------------------------------------------------------- 4. refusals


def _code(fn, *a):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("T", [16, 48])
def test_lockstep_nets_need_32_trees_per_net(native, T):
    """T = 16 and T = 48 trees per lock-step shaped net: AZG_E_UNSUPPORTED with the reason; the engine keeps the complete narrow
    population it held and searches on with it, the same results as before."""
    kw, ndesc, nblobs, roots, carry = _inputs(NARROW, T, nets=2)
    e = _population(native, kw, ndesc, nblobs)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    before = _collect(e)
    wdesc, wblob = P.config_net(P.CONFIGS[PENDULUM_2x512], 99)
    for upload in (lambda: e.set_net_weights(1, wdesc, wblob), lambda: e.set_net_weights(0, wdesc, wblob)):
        code, msg = _code(upload)
        assert code == _capi.AZG_E_UNSUPPORTED and "team" in msg and "multiple of 32" in msg and f"got {T}" in msg, (code, msg)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    _assert_same(_collect(e), before, T, "after the refusal")
    e.close()
    _assert_same(before, _oracle(kw, ndesc, nblobs, roots, carry, SIDX), T, "narrow population")


def test_32_trees_per_net_are_accepted(native):
    kw, desc, blobs, roots, carry = _inputs(PENDULUM_2x512, 32, nets=2)
    got, info = _search(native, kw, desc, blobs, roots, carry)
    _assert_same(got, _oracle_case(PENDULUM_2x512, 32, 2), 32, "2 x 32")
    _assert_team_or_fell_back(info, "2 x 32")


# ---------------------------------------------------------------------------------------------------------------- 5. fall-back


def test_team_kernel_of_a_population_gives_up_instead_of_hanging(native, monkeypatch):
    """Every hand-off wait counts as timed out (AZG_TEAM_SPIN_LIMIT=0): the population's search is redone by the per-layer launches."""
    monkeypatch.setenv("AZG_TEAM_SPIN_LIMIT", "0")
    kw, desc, blobs, roots, carry = _inputs(PENDULUM_2x512, 32, nets=2)
    got, info = _search(native, kw, desc, blobs, roots, carry)
    assert info["team_fallbacks"] == 1 and info["kernel_form"] == "per_layer", info
    _assert_same(got, _oracle_case(PENDULUM_2x512, 32, 2), 32, "fall-back")


# ---------------------------------------------------------------------------------------------------------------- 6. self-play


@pytest.mark.parametrize("variant", ["default", "launches"])
def test_population_selfplay_equals_one_net_engines(native, variant, monkeypatch):
    """population_selfplay_begin on K = 2 x 32 games of Pendulum [512, 512], three steps: net k's rows, stats and env states are
    those of a one-net self-play engine of 32 games with tree_id_base + 32k and net k's weights."""
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    nets, T, steps = 2, 32, 3
    kw, desc, blobs, _, _ = _inputs(PENDULUM_2x512, T, nets=nets)
    begin = dict(max_episode_length=2, capacity_steps=steps)
    pop = _population(native, kw, desc, blobs)
    pop.population_selfplay_begin(**begin)
    singles = []
    for k in range(nets):
        s = native.HipEngine(**dict(kw, n_trees=T, tree_id_base=BASE + k * T))
        s.set_weights(desc, blobs[k])
        s.selfplay_begin(**begin)
        singles.append(s)
    for _ in range(steps):
        pop.selfplay_step()
        for s in singles:
            s.selfplay_step()
    info = pop.search_info()
    ring = pop.selfplay_rows(clear=False)
    assert ring.shape[0] == steps * nets * T
    ring = ring.reshape(steps, nets, T, -1)
    fsum, fcnt, state = pop.selfplay_stats()
    for k, s in enumerate(singles):
        r = s.selfplay_rows(clear=False)
        np.testing.assert_array_equal(ring[:, k].reshape(-1, r.shape[1]), r, err_msg=f"net {k} rows")
        sl = slice(k * T, (k + 1) * T)
        for name, a, b in zip(("fsum", "fcnt", "state"), (fsum[sl], fcnt[sl], state[sl]), s.selfplay_stats()):
            np.testing.assert_array_equal(a, b, err_msg=f"net {k} {name}")
        s.close()
    pop.close()
    assert fcnt.sum() > 0                  # episodes ended (and games were reset) inside the window
    assert not np.array_equal(ring[:, 0], ring[:, 1])
    if variant == "default":
        _assert_team_or_fell_back(info, "self-play")
    else:
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, info


# ---------------------------------------------------------------------------------------------------------------- 7. reuse


def test_one_wide_net_gets_new_weights(native):
    """Search; replace net 1 from a device blob; search again: nets 0 and 2 equal a one-net engine's trees for that search index, net 1
    the oracle's with the new weights.  Then all three nets in one azg_set_population_weights_device call."""
    import torch
    T = 32
    kw, desc, blobs, roots, carry = _inputs(PENDULUM_2x512, T)
    e = _population(native, kw, desc, blobs)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    first = _collect(e)
    _assert_same(first, _oracle_case(PENDULUM_2x512, T), T, "before")
    new1 = P.config_net(P.CONFIGS[PENDULUM_2x512], 150)[1]
    dev = torch.from_numpy(new1).cuda()
    torch.cuda.synchronize()
    e.set_net_weights_device(1, desc, dev.data_ptr(), new1.size)
    e.set_search_index(SIDX + 1)
    e.search(roots, carry)
    second = _nets(_collect(e), T)
    for k in (0, 2):
        _assert_same(second[k], _one_net(native.HipEngine, kw, desc, blobs[k], roots, carry, SIDX + 1, k, T), T, f"net {k} kept its weights")
    _assert_same(second[1], _one_net(O.OracleEngine, kw, desc, new1, roots, carry, SIDX + 1, 1, T), T, "net 1 got new ones")
    assert not np.array_equal(second[1][0]["Q"], _nets(first, T)[1][0]["Q"])
    again = [P.config_net(P.CONFIGS[PENDULUM_2x512], 200 + k)[1] for k in range(K)]
    devs = torch.from_numpy(np.stack(again)).cuda()
    torch.cuda.synchronize()
    e.set_population_weights_device(desc, devs.data_ptr(), again[0].size, K)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    third = _collect(e)
    e.close()
    _assert_same(third, _oracle(kw, desc, again, roots, carry, SIDX), T, "all three at once")


# ---------------------------------------------------------------------------------------------------------------- 8. facade


def test_population_mcts_of_wide_policies(native):
    """PopulationMCTS of two torch policies of [512, 512] at 32 trees each returns what two BatchedMCTS of 32 trees return."""
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    from alphazero_gym_amd.search.mcts import BatchedMCTS, PopulationMCTS
    pols = []
    for s in (4, 5):
        torch.manual_seed(s)
        pols.append(make_policy(representation_dim=3, action_dim=1, distribution="normal", hidden_dimensions=[512, 512], nonlinearity="elu",
                                num_components=1, action_bound=2.0))
    T = 32
    kw = dict(env_id=2, mode=1, n_rollouts=20, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=9)
    pm = PopulationMCTS(pols, trees_per_model=T, tree_id_base=BASE, **kw)
    roots = pm.engine.synthetic_roots()
    pm.search(roots)
    got, gc = pm.results(), pm.root_children()
    assert pm.last_search_info["kernel_form"] in ("team", "per_layer")
    pm.close()
    for k, pol in enumerate(pols):
        bm = BatchedMCTS(pol, n_trees=T, tree_id_base=BASE + k * T, **kw)
        bm.search(roots[k * T:(k + 1) * T])
        want, wc = bm.results(), bm.root_children()
        bm.close()
        for name in want:
            np.testing.assert_array_equal(got[name][k * T:(k + 1) * T], want[name], err_msg=f"net {k} {name}")
        for a, b in zip(gc, wc):
            np.testing.assert_array_equal(a[k * T:(k + 1) * T], b, err_msg=f"net {k} children")
    assert not np.array_equal(got["Q"][:T], got["Q"][T:])


def test_agent_population_still_refuses_lockstep_nets(native):
    """One tree per agent is no multiple of 32: the facade raises the engine's reason."""
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    torch.manual_seed(1)
    pols = [make_policy(representation_dim=3, action_dim=1, distribution="normal", hidden_dimensions=[512, 512], nonlinearity="elu",
                        num_components=1, action_bound=2.0) for _ in range(2)]
    with pytest.raises(_capi.EngineError, match="multiple of 32 trees per net"):
        PopulationMCTS(pols, trees_per_model=1, env_id=2, mode=1, n_rollouts=10, c_uct=0.05, gamma=1.0)


def test_example_wide_with_two_seeds():
    """examples/population_selfplay_train.py --wide --seeds 3 11 --hidden 512 512 --games-per-seed 32: two wide nets in one engine,
    trained by the fused device trainer."""
    import population_selfplay_train as X
    a = X.parse_args(["--wide", "--seeds", "3", "11", "--hidden", "512", "512", "--games-per-seed", "32", "--iters", "2", "--trainer",
                      "device-fused", "--n-rollouts", "8", "--steps-per-iter", "10"])
    final = []
    hist = X.train(a, log=None, on_end=lambda agents: final.extend(_capi.policy_blob(ag.nn)[1].copy() for ag in agents))
    assert len(hist) == 2 and len(final) == 2
    for h in hist:
        assert len(h["loss"]) == 2 and np.isfinite(h["loss"]).all() and h["weight_sync"] == "device"
        assert h["env_steps"] == (h["iter"] + 1) * 10 * 64
    assert np.isfinite(final[0]).all() and np.isfinite(final[1]).all() and not np.array_equal(final[0], final[1])
