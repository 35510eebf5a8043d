"""Batched inference for populations (azg_population_mlp_eval / _device / azg_population_root_eval, include/azgym_eval.h).

gpu: a K-net engine's one-launch evaluation equals, bit for bit, azg_mlp_eval of K one-net engines (and the CPU oracle's) -- for every
kernel form, every grid the tile loop can take, shared observations, NULL outputs and the device form; the calls leave the engine's
searches and self-play untouched; azg_population_root_eval equals the one-net engines' azg_root_eval on every search form; the trainer's
forward pass agrees for every net; the errors.  CPU: the documented prototypes are the header's, and the bindings check shapes first."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle_lib as O
from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3

# name: (network (in_dim, hidden, n_dist, activation, mixture components), layernorm, engine kwargs, register-resident hidden weights)
CARTPOLE = dict(env_id=0, mode=0, num_actions=2, n_sims=8, c_uct=1.5, gamma=1.0, epsilon=0.1, seed=37)
ACROBOT = dict(env_id=5, mode=0, num_actions=3, n_sims=8, c_uct=1.0, gamma=0.99, epsilon=0.05, seed=38)
PENDULUM = dict(env_id=2, mode=1, n_sims=16, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34)
SHAPES = {
    "acrobot_2x64": ((6, [64, 64], 3, "relu", 0), False, ACROBOT, 1),
    "cartpole_2x128": ((4, [128, 128], 2, "relu", 0), False, CARTPOLE, 1),
    "pendulum_2x256": ((3, [256, 256], 2, "elu", 0), False, PENDULUM, 1),
    "pendulum_3x128_gmm2": ((3, [128, 128, 128], 6, "elu", 2), False, PENDULUM, 1),
    "cartpole_2x64_ln": ((4, [64, 64], 2, "relu", 0), True, CARTPOLE, 0),
    "cartpole_2x512": ((4, [512, 512], 2, "relu", 0), False, CARTPOLE, 0),
    "pendulum_4x1024": ((3, [1024] * 4, 2, "elu", 0), False, PENDULUM, 0),
}
WIDE = ("cartpole_2x512", "pendulum_4x1024")   # searched as teams: a population needs a multiple of 32 trees per net


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _desc(name):
    (in_dim, hidden, n_dist, act, ncomp), ln, _, _ = SHAPES[name]
    return _capi.make_desc(in_dim, hidden, n_dist, act, num_components=ncomp, layernorm=ln)


def _blob(name, k):
    (in_dim, hidden, n_dist, _, _), ln, _, _ = SHAPES[name]
    b = O.make_weights(100 + 7 * k, in_dim, hidden, n_dist)
    return O.add_layernorm(b, in_dim, hidden, n_dist, 300 + k) if ln else b


def _trees(name):
    return 32 if name in WIDE else 2


def _population(name, nets=K, T=None, weights=True, **over):
    T = T or _trees(name)
    e = _hip()(**dict(SHAPES[name][2], n_trees=nets * T, **over))
    if nets > 1:
        e.set_population(nets)
    for k in range(nets if weights else 0):
        if nets > 1:
            e.set_net_weights(k, _desc(name), _blob(name, k))
        else:
            e.set_weights(_desc(name), _blob(name, k))
    return e


def _single(cls, name, k, T=None, **over):
    e = cls(**dict(SHAPES[name][2], n_trees=T or _trees(name), **over))
    e.set_weights(_desc(name), _blob(name, k))
    return e


@functools.lru_cache(maxsize=None)
def _obs(name, n):
    """[K, n, obs_dim]: standard normals, with one all-zero row (net 1's last) and one row of +-1e3 (net 2's first)."""
    in_dim = SHAPES[name][0][0]
    obs = np.random.default_rng(1000 + n).standard_normal((K, n, in_dim)).astype(np.float32)
    obs[1, n - 1] = 0.0
    obs[2, 0] = 1e3 * (1.0 - 2.0 * (np.arange(in_dim) % 2))
    obs.setflags(write=False)
    return obs


@functools.lru_cache(maxsize=None)
def _yardstick(name, n):
    """(value, dist, raw) [K, n, ...] of K one-net HIP engines' azg_mlp_eval: computed once per (shape, n), never written again."""
    parts = []
    for k in range(K):
        e = _single(_hip(), name, k)
        parts.append(e.mlp_eval(_obs(name, n)[k]))
        e.close()
    out = tuple(np.stack([p[i] for p in parts]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def _equal(got, want, what):
    for g, w, key in zip(got, want, ("value", "dist", "raw")):
        assert g.shape == w.shape, f"{what}: {key} shape"
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {key}")


CASES_1 = [(name, n) for name in SHAPES for n in ((1, 17) if name == "pendulum_4x1024" else (1, 16, 17, 50))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES_1, ids=[f"{a}-n{b}" for a, b in CASES_1])
def test_population_equals_single_engines(name, n):
    e = _population(name)
    got = e.population_mlp_eval(_obs(name, n))
    info = e.last_eval_info
    e.close()
    _equal(got, _yardstick(name, n), f"{name} n={n}")
    assert info["tiles"] == (n + 15) // 16 and info["groups"] == info["tiles"] and info["resident"] == SHAPES[name][3]
    assert np.isfinite(got[0][0]).all()
    assert not np.array_equal(got[2][0], got[2][1])   # (the nets do differ)


@pytest.mark.gpu
def test_population_equals_the_oracle_per_net():
    name, n = "pendulum_3x128_gmm2", 50
    e = _population(name)
    got = e.population_mlp_eval(_obs(name, n))
    e.close()
    for k in range(K):
        o = _single(O.OracleEngine, name, k)
        want = o.mlp_eval(_obs(name, n)[k])
        o.close()
        _equal([g[k] for g in got], want, f"{name} net {k} against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("name", ["cartpole_2x128", "pendulum_2x256", "cartpole_2x64_ln", "cartpole_2x512"])
def test_tile_loop(name, groups, monkeypatch):
    """n = 50: four tiles, the last with two rows, walked by 1, 2 or 3 workgroups per net."""
    n = 50
    free = _population(name)
    uncapped = free.population_mlp_eval(_obs(name, n))
    assert free.last_eval_info == {"resident": SHAPES[name][3], "groups": 4, "tiles": 4}
    free.close()
    monkeypatch.setenv("AZG_EVAL_GROUPS", str(groups))
    e = _population(name)
    got = e.population_mlp_eval(_obs(name, n))
    info = e.last_eval_info
    e.close()
    assert info == {"resident": SHAPES[name][3], "groups": groups, "tiles": 4}
    _equal(got, uncapped, f"{name} groups={groups} against the uncapped call")
    _equal(got, _yardstick(name, n), f"{name} groups={groups}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole_2x128", "pendulum_3x128_gmm2", "cartpole_2x512"])
def test_shared_observations(name):
    n = 17
    rows = _obs(name, n)[2]
    e = _population(name)
    got = e.population_mlp_eval(rows, shared=True)
    want = e.population_mlp_eval(np.tile(rows[None], (K, 1, 1)))
    e.close()
    _equal(got, want, f"{name} shared")
    one = _population(name, nets=1)
    want1 = one.mlp_eval(rows)
    for shared, obs in ((True, rows), (False, rows[None])):
        _equal(one.population_mlp_eval(obs, shared=shared), [w[None] for w in want1], f"{name} K=1 shared={shared}")
    one.close()
    _equal([g[0] for g in got], want1, f"{name} net 0 of the shared call")


def _fp(a):
    return _capi._ptr(a, C.c_float)


def _sentinels(name, nets, n):
    nd = _desc(name).n_dist
    return [np.full(s, -77.0, np.float32) for s in ((nets, n), (nets, n, nd), (nets, n, 1 + nd))]


@pytest.mark.gpu
def test_null_outputs():
    name, n = "pendulum_2x256", 17
    e = _population(name)
    fn = e._f["population_mlp_eval"]
    obs = np.ascontiguousarray(_obs(name, n))
    full = e.population_mlp_eval(obs)
    for skip in range(3):
        outs = _sentinels(name, K, n)
        ptrs = [None if i == skip else _fp(a) for i, a in enumerate(outs)]
        assert fn(e._h, _fp(obs), n, 0, *ptrs, None) == 0
        for i, a in enumerate(outs):
            if i == skip:
                assert (a == -77.0).all()
            else:
                np.testing.assert_array_equal(a, full[i], err_msg=f"output {i} with output {skip} NULL")
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole_2x128", "pendulum_3x128_gmm2", "cartpole_2x64_ln", "cartpole_2x512"])
def test_device_form(name):
    n = 17
    e = _population(name)
    obs = torch.from_numpy(_obs(name, n).copy()).cuda()
    nd = _desc(name).n_dist
    out = tuple(torch.full(s, float("nan"), device="cuda") for s in ((K, n), (K, n, nd), (K, n, 1 + nd)))
    got = e.population_mlp_eval_device(obs, out=out)
    assert all(g is o for g, o in zip(got, out))
    _equal([g.cpu().numpy() for g in got], _yardstick(name, n), f"{name} device form")
    assert e.last_eval_info == {"resident": SHAPES[name][3], "groups": 2, "tiles": 2}
    fresh = e.population_mlp_eval_device(obs[2], shared=True)
    _equal([g.cpu().numpy() for g in fresh], e.population_mlp_eval(_obs(name, n)[2], shared=True), f"{name} device form, shared")
    e.close()


def _search_outputs(e):
    out = dict(e.results())
    out["child_n"], out["child_state"] = e.root_children()
    return out


@pytest.mark.gpu
def test_eval_leaves_a_search_untouched():
    name, T = "cartpole_2x128", 3
    e, twin = _population(name, T=T), _population(name, T=T)
    roots = e.synthetic_roots()
    for x in (e, twin):
        x.set_search_index(4)
        x.search(roots)
    before = _search_outputs(e)
    _equal(e.population_mlp_eval(_obs(name, 50)), _yardstick(name, 50), "between results")
    e.population_mlp_eval_device(torch.from_numpy(_obs(name, 17).copy()).cuda())
    after = _search_outputs(e)
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    dump, want = e.dump_tree(), twin.dump_tree()
    assert dump["n_records"].sum() > K * T
    for key in want:
        np.testing.assert_array_equal(dump[key], want[key], err_msg=f"dump {key}")
    e.close()
    twin.close()


@pytest.mark.gpu
def test_eval_between_selfplay_steps():
    name, T = "cartpole_2x128", 3
    e, twin = _population(name, T=T), _population(name, T=T)
    for x in (e, twin):
        x.population_selfplay_begin(20, capacity_steps=4)
        x.selfplay_step()
    _equal(e.population_mlp_eval(_obs(name, 50)), _yardstick(name, 50), "between self-play steps")
    for x in (e, twin):
        x.selfplay_step()
    got, want = e.selfplay_rows(clear=False), twin.selfplay_rows(clear=False)
    assert got.shape[0] == 2 * K * T
    np.testing.assert_array_equal(got, want)
    assert e.selfplay_ring() == twin.selfplay_ring()
    e.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,env,form", [("cartpole_2x128", 3, {}, "persistent"), ("pendulum_2x256", 16, {}, "persistent"),
                                             ("cartpole_2x512", 32, {}, "team"), ("cartpole_2x512", 32, {"AZG_LS_TEAM": "0"}, "per_layer")],
                         ids=["cartpole_2x128", "pendulum_2x256", "cartpole_2x512_team", "cartpole_2x512_per_layer"])
def test_root_eval(name, T, env, form, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base, idx = 11, 5
    e = _population(name, T=T, tree_id_base=base)
    roots = e.synthetic_roots()
    e.set_search_index(idx)
    e.search(roots)
    assert e.search_info()["kernel_form"] == form
    value, dist = e.population_root_eval()
    e.close()
    want_v, want_d = [], []
    for k in range(K):
        s = _single(_hip(), name, k, T=T, tree_id_base=base + k * T)
        s.set_search_index(idx)
        s.search(roots[k * T:(k + 1) * T])
        v, d = s.root_eval()
        want_v.append(v)
        want_d.append(d)
        s.close()
    np.testing.assert_array_equal(value, np.concatenate(want_v))
    np.testing.assert_array_equal(dist, np.concatenate(want_d))
    assert np.isfinite(value).all() and len(set(value.tolist())) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole_2x128", "pendulum_2x256"])
def test_trainer_forward_for_every_net(name):
    """The trainer's raw of all K nets on 32 rows each within 1e-5 of the engine's (the bound of the existing forward tests, which look at
    net 0 through a one-net engine: the trainer orders its head sums differently from mlp.cuh's chunked ones)."""
    from alphazero_gym_amd import _native
    _native.lib()
    B = 32
    desc = _desc(name)
    params = torch.from_numpy(np.stack([_blob(name, k) for k in range(K)])).cuda()
    obs = np.random.default_rng(5).standard_normal((K, B, SHAPES[name][0][0])).astype(np.float32)
    e = _population(name)
    _, _, want = e.population_mlp_eval(obs)
    e.close()
    tr = _native.HipTrainer(desc, K, 64)
    raw = torch.empty((K, B, tr.n_raw), device="cuda")
    d_obs = torch.from_numpy(obs).cuda()
    torch.cuda.synchronize()
    tr.forward(params.data_ptr(), d_obs.data_ptr(), B, raw.data_ptr())
    got = raw.cpu().numpy()
    tr.close()
    for k in range(K):
        err = np.abs(got[k] - want[k]).max()
        print(f"{name} net {k}: trainer raw against population_mlp_eval, max abs difference {err:.3g}")
        assert err <= 1e-5, f"net {k}"


@pytest.mark.gpu
def test_population_mcts_surface():
    """PopulationMCTS.evaluate_observations (numpy and device tensors, shared rows) and root_eval against K BatchedMCTS of one model."""
    from alphazero_gym_amd.network.policies import make_policy
    from alphazero_gym_amd.search.mcts import BatchedMCTS, PopulationMCTS
    _hip()
    torch.manual_seed(3)
    models = [make_policy(4, 1, "discrete", [128, 128], "relu", num_actions=2) for _ in range(K)]
    kw = dict(env_id=0, mode=0, n_rollouts=8, c_uct=1.5, gamma=1.0, epsilon=0.1, num_actions=2, seed=37)
    T, n = 2, 17
    obs = np.ascontiguousarray(_obs("cartpole_2x128", n))
    pm = PopulationMCTS(models, trees_per_model=T, tree_id_base=5, **kw)
    roots = pm.engine.synthetic_roots()
    pm.search(roots)
    host = pm.evaluate_observations(obs)
    dev = pm.evaluate_observations(torch.from_numpy(obs.copy()).cuda())
    shared = pm.evaluate_observations(torch.from_numpy(obs[1].copy()), shared=True)   # (a CPU tensor takes the host form)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev) and all(isinstance(a, np.ndarray) for a in host + shared)
    _equal([t.cpu().numpy() for t in dev], host, "device tensors against numpy")
    value, dist = pm.root_eval()
    pm.close()
    for k in range(K):
        one = BatchedMCTS(models[k], n_trees=T, tree_id_base=5 + k * T, **kw)
        one.search(roots[k * T:(k + 1) * T])
        _equal([h[k] for h in host], one.engine.mlp_eval(obs[k]), f"model {k}")
        _equal([s[k] for s in shared], one.engine.mlp_eval(obs[1]), f"model {k}, shared rows")
        _equal([h[0] for h in one.evaluate_observations(obs[k][None])], one.engine.mlp_eval(obs[k]), f"BatchedMCTS of model {k}")
        v1, d1 = one.root_eval()
        one.close()
        np.testing.assert_array_equal(value[k * T:(k + 1) * T], v1)
        np.testing.assert_array_equal(dist[k * T:(k + 1) * T], d1)


@pytest.mark.gpu
def test_errors():
    name, n = "cartpole_2x128", 5
    obs = np.ascontiguousarray(_obs(name, n)[:2])
    e = _population(name, nets=2, weights=False)
    e.set_net_weights(0, _desc(name), _blob(name, 0))
    fns = (e._f["population_mlp_eval"], e._f["population_mlp_eval_device"])
    outs = _sentinels(name, 2, n)
    ptrs = [_fp(a) for a in outs]
    info = _capi.AzgEvalInfo()
    info.struct_size = C.sizeof(_capi.AzgEvalInfo)
    info.groups = -5
    assert fns[0](e._h, _fp(obs), n, 0, *ptrs, C.byref(info)) == _capi.AZG_E_STATE          # net 1 has no weights
    assert "every net" in e._f["last_error"](e._h).decode()
    e.set_net_weights(1, _desc(name), _blob(name, 1))
    for fn in fns:   # (every check comes before the first read of obs or write of an output: host pointers do for the device form here)
        args = ([_fp(obs)] if fn is fns[0] else [C.c_void_p(obs.ctypes.data)])
        outp = ptrs if fn is fns[0] else [C.c_void_p(a.ctypes.data) for a in outs]
        assert fn(e._h, *args, (1 << 23) + 1, 0, *outp, C.byref(info)) == _capi.AZG_E_INVALID   # 2 * n > 2^24
        assert fn(None, *args, n, 0, *outp, C.byref(info)) == _capi.AZG_E_INVALID
        assert fn(e._h, None, n, 0, *outp, C.byref(info)) == _capi.AZG_E_INVALID
        bad = _capi.AzgEvalInfo()
        bad.struct_size = C.sizeof(_capi.AzgEvalInfo) + 4
        assert fn(e._h, *args, n, 0, *outp, C.byref(bad)) == _capi.AZG_E_INVALID
        assert fn(e._h, *args, 0, 0, *outp, C.byref(info)) == _capi.AZG_OK                     # n = 0: nothing happens
    assert info.groups == -5                                                                   # (info is written on success only)
    for a in outs:
        assert (a == -77.0).all()
    assert fns[0](e._h, _fp(obs), n, 0, *ptrs, C.byref(info)) == 0 and info.groups == 1 and info.tiles == 1
    assert not any((a == -77.0).any() for a in outs)
    with pytest.raises(_capi.EngineError) as ei:                                              # the old entry point names the new one
        e.mlp_eval(obs[0])
    assert ei.value.code == _capi.AZG_E_UNSUPPORTED and "azg_population_mlp_eval" in str(ei.value)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- no GPU


def test_documented_prototypes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "azgym_eval.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    protos = re.findall(r"^int azg_population_(?:mlp_eval|mlp_eval_device|root_eval)\([^;]*\);", doc, flags=re.M)
    assert len(protos) == 3 and len(set(protos)) == 3
    for p in protos:
        assert p in header, p


def test_bindings_check_shapes_before_the_library():
    """On the CPU oracle, whose library lacks the symbols: a wrong shape is a ValueError naming both shapes, a right one reaches _optional."""
    e = O.OracleEngine(env_id=2, mode=1, n_trees=2, n_sims=4, c_uct=0.05, gamma=1.0)
    for method, make in ((e.population_mlp_eval, lambda *s: np.zeros(s, np.float32)), (e.population_mlp_eval_device, lambda *s: torch.zeros(s))):
        for shape, shared, expected in (((5, 3), False, "[1, n, 3]"), ((2, 5, 3), False, "[1, n, 3]"), ((1, 5, 4), False, "[1, n, 3]"),
                                        ((1, 5, 3), True, "[n, 3]"), ((5, 4), True, "[n, 3]"), ((3,), True, "[n, 3]")):
            with pytest.raises(ValueError) as ei:
                method(make(*shape), shared=shared)
            assert str(list(shape)) in str(ei.value) and expected in str(ei.value)
        for shape, shared in (((1, 5, 3), False), ((5, 3), True)):
            with pytest.raises(NotImplementedError, match="no population_mlp_eval"):
                method(make(*shape), shared=shared)
    with pytest.raises(NotImplementedError, match="no population_root_eval"):
        e.population_root_eval()
    e.close()
