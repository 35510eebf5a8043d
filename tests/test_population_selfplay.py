"""Device self-play for populations (azg_population_selfplay_begin, azg_set_population_weights_device, run.PopulationSelfPlay).

Engine level (gpu): a K-net self-play engine plays, bit for bit, what K single-net self-play engines with tree_id_base + k*T play
(rows of every step, ring, stats), also when nets get new weights between steps; the one-launch weight upload equals per-net host
uploads.  Facade: PopulationSelfPlay's per-net splitting on CPU against a double made of K oracle self-play engines, and the
example's training loop against K single-net loops on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits
from test_population import CASES, K, _blob, _desc, _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

STEPS = 12
MAX_LEN = 5   # episodes reset inside the window


def _begin(e, population, v):
    kw = dict(max_episode_length=MAX_LEN, deterministic=v.get("deterministic", False), capacity_steps=v.get("capacity", STEPS),
              final_selection=v.get("final_selection", "max_visit"), temperature=v.get("temperature", 1.0),
              agent_epsilon=v.get("agent_epsilon", 0.0), fifo=v.get("fifo", False))
    (e.population_selfplay_begin if population else e.selfplay_begin)(**kw)


def _pop_engine(cls, kw, net, T, base, blob_of=_blob):
    e = cls(**dict(kw, n_trees=K * T, tree_id_base=base))
    e.set_population(K)
    for k in range(K):
        e.set_net_weights(k, _desc(net), blob_of(net, k))
    return e


def _single_engines(cls, kw, net, T, base, blob_of=_blob):
    out = []
    for k in range(K):
        e = cls(**dict(kw, n_trees=T, tree_id_base=base + k * T))
        e.set_weights(_desc(net), blob_of(net, k))
        out.append(e)
    return out


def _compare_step(pop, singles, T, what):
    """Ring (every stored row, slot order), ring bookkeeping and stats of the population against the singles', net by net."""
    ring = pop.selfplay_rows(clear=False)
    assert pop.selfplay_ring() == singles[0].selfplay_ring(), what
    steps = ring.shape[0] // (K * T)
    ring = ring.reshape(steps, K, T, -1)
    fsum, fcnt, state = pop.selfplay_stats()
    for k, s in enumerate(singles):
        assert s.selfplay_ring() == pop.selfplay_ring(), what
        r = s.selfplay_rows(clear=False)
        np.testing.assert_array_equal(ring[:, k].reshape(-1, r.shape[1]), r, err_msg=f"{what}: net {k} rows")
        sf, sc, ss = s.selfplay_stats()
        sl = slice(k * T, (k + 1) * T)
        assert_stats_bits((fsum[sl], fcnt[sl], state[sl]), (sf, sc, ss), f"{what}: net {k}")
    return fcnt


def _close(*es):
    for e in es:
        if isinstance(e, list):
            _close(*e)
        else:
            e.close()


VARIANTS = {
    "fifo_wrap": dict(fifo=True, capacity=5),
    "stop": dict(),
    "max_value": dict(final_selection="max_value"),
    "temperature": dict(temperature=0.5),
    "agent_epsilon": dict(agent_epsilon=0.3),
    "deterministic": dict(deterministic=True),
}


def _applies(name, variant):
    discrete = CASES[name][0]["mode"] == _capi.MODE_DISCRETE
    return not ((variant == "temperature" and not discrete) or (variant == "agent_epsilon" and discrete))


MATRIX = [(n, T, "fifo_wrap") for n in CASES for T in (1, 3, 32)]
MATRIX += [(n, 3, v) for n in CASES for v in VARIANTS if v != "fifo_wrap" and _applies(n, v)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,variant", MATRIX)
def test_population_selfplay_equals_single_engines(name, T, variant, monkeypatch):
    kw, net, _, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cls, v = _hip(), VARIANTS[variant]
    base = 7
    pop, singles = _pop_engine(cls, kw, net, T, base), _single_engines(cls, kw, net, T, base)
    _begin(pop, True, v)
    for s in singles:
        _begin(s, False, v)
    for step in range(STEPS):
        pop.selfplay_step()
        for s in singles:
            s.selfplay_step()
        fcnt = _compare_step(pop, singles, T, f"{name} T={T} {variant} step {step}")
    assert fcnt.sum() > 0   # episodes ended (and reset) inside the window
    if v.get("fifo"):
        assert pop.selfplay_ring() == (5, STEPS % 5, STEPS)
    _close(pop, singles)


def _new_blob(net, k):
    return _blob(net, k, base_seed=900)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("name", ["cartpole_2x128_relu_carry_eps", "pendulum_v0_3x128_gmm2"])
def test_weights_replaced_between_steps(name, how):
    kw, net, _, _ = CASES[name]
    cls, T, base, v = _hip(), 3, 0, dict(fifo=True, capacity=4)
    pop, singles = _pop_engine(cls, kw, net, T, base), _single_engines(cls, kw, net, T, base)
    ref = _pop_engine(cls, kw, net, T, base)   # the same population, weights never replaced
    for e, p in [(pop, True), (ref, True)] + [(s, False) for s in singles]:
        _begin(e, p, v)
    changed = (1, 3)
    for step in range(STEPS):
        if step == 5:
            if how == "host":
                for k in changed:
                    pop.set_net_weights(k, _desc(net), _new_blob(net, k))
            else:
                blobs = np.stack([_new_blob(net, k) if k in changed else _blob(net, k) for k in range(K)])
                dev = torch.from_numpy(blobs).cuda()
                torch.cuda.synchronize()
                pop.set_population_weights_device(_desc(net), dev.data_ptr(), blobs.shape[1], K)
            for k in changed:
                singles[k].set_weights(_desc(net), _new_blob(net, k))
        for e in [pop, ref] + singles:
            e.selfplay_step()
        _compare_step(pop, singles, T, f"{name} {how} step {step}")
    got = pop.selfplay_rows(clear=False).reshape(4, K, T, -1)
    unchanged = ref.selfplay_rows(clear=False).reshape(4, K, T, -1)
    for k in range(K):
        same = np.array_equal(got[:, k], unchanged[:, k])
        assert same == (k not in changed), f"net {k}"
    _close(pop, ref, singles)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole_2x128_relu_carry_eps", "pendulum_v1_2x256_elu"])
def test_population_selfplay_begin_with_one_net_is_selfplay_begin_ex(name):
    kw, net, _, _ = CASES[name]
    cls = _hip()
    a, b = cls(**dict(kw, n_trees=9)), cls(**dict(kw, n_trees=9))
    for e in (a, b):
        e.set_weights(_desc(net), _blob(net, 0))
    b.set_population(1)
    v = dict(fifo=True, capacity=4)
    _begin(a, False, v)
    _begin(b, True, v)
    for _ in range(8):
        a.selfplay_step()
        b.selfplay_step()
    np.testing.assert_array_equal(a.selfplay_rows(clear=False), b.selfplay_rows(clear=False))
    assert a.selfplay_ring() == b.selfplay_ring()
    assert_stats_bits(a.selfplay_stats(), b.selfplay_stats(), name)
    _close(a, b)


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _search_out(e, roots):
    e.set_search_index(3)
    e.search(roots)
    out = dict(e.results())
    out["child_n"], out["child_state"] = e.root_children()
    out.update({"dump_" + k: v for k, v in e.dump_tree().items()})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pendulum_v0_3x128_gmm2", "cartpole_2x128_relu_carry_eps", "pendulum_v1_2x256_elu"])
def test_population_weights_device_equals_host_uploads(name):
    kw, net, _, _ = CASES[name]
    cls, n = _hip(), 3
    blobs = np.stack([_blob(net, k) for k in range(n)])
    dev = torch.from_numpy(blobs).cuda()
    torch.cuda.synchronize()
    host, one = cls(**dict(kw, n_trees=n * 4)), cls(**dict(kw, n_trees=n * 4))
    host.set_population(n)
    one.set_population(n)
    for k in range(n):
        host.set_net_weights(k, _desc(net), blobs[k])
    one.set_population_weights_device(_desc(net), dev.data_ptr(), blobs.shape[1], n)
    roots = host.synthetic_roots()
    want, got = _search_out(host, roots), _search_out(one, roots)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # one net from a device blob
    host.set_net_weights(1, _desc(net), _blob(net, 0))
    one.set_net_weights_device(1, _desc(net), dev.data_ptr(), blobs.shape[1])   # (blob 0 is the first row)
    want, got = _search_out(host, roots), _search_out(one, roots)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    _close(host, one)


@pytest.mark.gpu
def test_population_weights_device_with_one_net_is_set_weights_device():
    kw, net, _, _ = CASES["pendulum_v1_2x256_elu"]
    cls = _hip()
    blob = torch.from_numpy(_blob(net, 2)).cuda()
    torch.cuda.synchronize()
    a, b = cls(**dict(kw, n_trees=7)), cls(**dict(kw, n_trees=7))
    a.set_weights_device(_desc(net), blob.data_ptr(), blob.numel())
    b.set_population_weights_device(_desc(net), blob.data_ptr(), blob.numel(), 1)
    roots = a.synthetic_roots()
    want, got = _search_out(a, roots), _search_out(b, roots)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    _close(a, b)


@pytest.mark.gpu
def test_population_weights_device_and_selfplay_errors():
    cls = _hip()
    d64, b64 = _capi.make_desc(3, [64, 64], 2, "elu"), O.make_weights(1, 3, [64, 64], 2)
    e = cls(env_id=2, mode=1, n_trees=6, n_sims=10, c_uct=0.05, gamma=1.0)
    e.set_population(3)
    dev = torch.from_numpy(np.stack([b64] * 3)).cuda()
    torch.cuda.synchronize()
    n = b64.size
    f = e._f["set_population_weights_device"]
    assert f(e._h, None, dev.data_ptr(), n, 3) == _capi.AZG_E_INVALID                            # NULL descriptor
    assert f(e._h, _capi.C.byref(d64), None, n, 3) == _capi.AZG_E_INVALID                        # NULL blobs
    assert _code(e.set_population_weights_device, d64, dev.data_ptr(), n - 1, 3) == _capi.AZG_E_INVALID   # wrong size
    for bad in (1, 2, 6):
        assert _code(e.set_population_weights_device, d64, dev.data_ptr(), n, bad) == _capi.AZG_E_INVALID   # n_nets != engine's
    for bad in (3, -1):
        assert _code(e.set_net_weights_device, bad, d64, dev.data_ptr(), n) == _capi.AZG_E_INVALID
    assert _code(e.search, e.synthetic_roots()) == _capi.AZG_E_STATE                             # nothing was written
    e.population_selfplay_begin(5, capacity_steps=4)
    assert _code(e.selfplay_step) == _capi.AZG_E_STATE                                            # no net has weights yet
    e.set_net_weights(0, d64, b64)
    e.set_net_weights(1, d64, b64)
    assert _code(e.selfplay_step) == _capi.AZG_E_STATE                                            # net 2 has none
    e.set_population_weights_device(d64, dev.data_ptr(), n, 3)
    e.selfplay_step()
    assert _code(e.set_population, 2) == _capi.AZG_E_UNSUPPORTED                                 # self-play is running
    assert _code(e.selfplay_begin, 10) == _capi.AZG_E_UNSUPPORTED                                # plain self-play: one net
    c = _capi.AzgSelfplayConfig()
    c.struct_size = _capi.C.sizeof(c)
    c.max_episode_length, c.capacity_steps, c.temperature = 10, 4, 1.0
    assert e._f["selfplay_begin_ex"](e._h, _capi.C.byref(c)) == _capi.AZG_E_UNSUPPORTED
    # a failed upload leaves the complete weights it found: the next step plays on
    before = e.selfplay_rows(clear=False)
    assert _code(e.set_population_weights_device, d64, dev.data_ptr(), n + 1, 3) == _capi.AZG_E_INVALID
    w512 = O.make_weights(1, 3, [512, 512], 2)
    big = torch.from_numpy(np.stack([w512] * 3)).cuda()
    torch.cuda.synchronize()
    assert _code(e.set_population_weights_device, _capi.make_desc(3, [512, 512], 2, "elu"), big.data_ptr(), w512.size, 3) == \
        _capi.AZG_E_UNSUPPORTED                                                                    # HP >= 512: team forms
    e.selfplay_step()
    assert e.selfplay_rows(clear=False).shape[0] == before.shape[0] + 6
    _close(e)


# ---------------------------------------------------------------------------------------------------------------- facade


def _example(**over):
    import population_selfplay_train as P
    a = P.parse_args(["--game", "CartPole-v0", "--seeds", "3", "11", "--games-per-seed", "4", "--n-rollouts", "6", "--iters", "3",
                      "--steps-per-iter", "6", "--train-rows", "20", "--batch-size", "8", "--hidden", "32", "32",
                      "--max-episode-length", "8", "--device", "cpu"])
    for k, v in over.items():
        setattr(a, k, v)
    return P, a


def _single_loops(a):
    """What the example computes, as one DeviceSelfPlay per seed (rank k: global games k*T ...) trained by its own loop."""
    from alphazero_gym_amd import run
    from selfplay_train import build_agent
    agents, sps = [], []
    for k, s in enumerate(a.seeds):
        torch.manual_seed(s)
        agent, state_dim = build_agent(a.game, a.hidden, a.n_rollouts, a.device, a.lr)
        m = agent.mcts
        agents.append(agent)
        sps.append(run.DeviceSelfPlay(agent.nn, game=a.game, n_games=a.games_per_seed, n_rollouts=a.n_rollouts, c_uct=m.c_uct,
                                      gamma=m.gamma, epsilon=m.epsilon, max_episode_length=a.max_episode_length,
                                      capacity_steps=a.steps_per_iter, seed=a.engine_seed, rank=k))
    rngs = [np.random.RandomState(s) for s in a.seeds]
    rows_per_iter = []
    for it in range(a.iters):
        rows = [sp.collect(a.steps_per_iter) for sp in sps]
        rows_per_iter.append(rows)
        for agent, rng, r, sp in zip(agents, rngs, rows, sps):
            pick = rng.choice(r.shape[0], size=min(a.train_rows, r.shape[0]), replace=False)
            run.train_on_rows(agent, r[torch.from_numpy(pick)], state_dim, sp.engine.kmax, batch_size=a.batch_size,
                              shuffle_seed=int(rng.randint(2 ** 31 - 1)))
    for sp in sps:
        sp.engine.close()
    return agents, rows_per_iter


@pytest.mark.gpu
def test_example_trains_like_single_net_loops(monkeypatch):
    _hip()
    P, a = _example()
    got_rows, agents = [], []
    build = P.build_population

    def keep(args):
        out = build(args)
        agents.extend(out[0])
        return out

    monkeypatch.setattr(P, "build_population", keep)
    hist = P.train(a, log=None, on_rows=lambda it, rows: got_rows.append([r.clone() for r in rows]))
    assert len(hist) == a.iters and all(len(h["mean_return"]) == 2 for h in hist)
    assert hist[-1]["weight_sync"] == "host"
    ref_agents, ref_rows = _single_loops(a)
    for it in range(a.iters):
        for k in range(2):
            assert torch.equal(got_rows[it][k], ref_rows[it][k]), f"iteration {it}, seed {k}"
    for k in range(2):
        for (n, p), (_, q) in zip(agents[k].nn.named_parameters(), ref_agents[k].nn.named_parameters()):
            assert torch.equal(p, q), f"seed {k}: {n}"
    assert not torch.equal(next(agents[0].nn.parameters()), next(agents[1].nn.parameters()))


@pytest.mark.gpu
@pytest.mark.parametrize("fifo", [False, True])
def test_collect_device_equals_collect_with_policies_on_the_gpu(fifo):
    from alphazero_gym_amd import run
    from selfplay_train import build_agent
    _hip()
    nets = []
    for s in (1, 2, 3):
        torch.manual_seed(s)
        nets.append(build_agent("CartPole-v0", [32, 32], 6, "cuda:0", 1e-3)[0].nn)
    kw = dict(game="CartPole-v0", games_per_net=4, n_rollouts=6, c_uct=1.5, epsilon=0.1, max_episode_length=6, capacity_steps=3,
              fifo=fifo)
    a, b = run.PopulationSelfPlay(nets, **kw), run.PopulationSelfPlay(nets, **kw)
    assert a.last_weight_sync == b.last_weight_sync == "device"
    for it in range(3):
        if it == 1:
            with torch.no_grad():
                for p in nets[1].parameters():
                    p.mul_(0.5)
        ra, rb = a.collect(2), b.collect_device(2)   # (FIFO: b's ring is not cleared, it wraps from the second iteration on)
        assert a.last_weight_sync == b.last_weight_sync == ("device" if it == 1 else None)
        for x, y in zip(ra, rb):
            assert y.is_cuda and x.shape == y.shape == (2 * 4, x.shape[1])
            assert torch.equal(x, y.cpu())
        for x, y in zip(a.finished_returns(), b.finished_returns()):
            np.testing.assert_array_equal(x, y)
    if fifo:
        assert b.engine.selfplay_ring() == (3, 0, 6)
    a.close()
    b.close()


class OracleSelfPlayPopulation:
    """CPU double of a HIP engine with population self-play: K oracle engines (net k: tree_id_base + k*T), stepped one after
    another; the ring is laid out as the HIP engine's, [steps][K*T][row]."""

    def __init__(self, **kw):
        self.kw = kw
        self.n_trees = kw["n_trees"]
        self.engines = [O.OracleEngine(**kw)]
        self.cfg, self.kmax, self.s_obs, self.mode = (self.engines[0].cfg, self.engines[0].kmax, self.engines[0].s_obs,
                                                      self.engines[0].mode)
        self.uploads = []

    def set_population(self, n):
        self.close()
        self.T = self.n_trees // n
        base = self.kw.get("tree_id_base", 0)
        self.engines = [O.OracleEngine(**dict(self.kw, n_trees=self.T, tree_id_base=base + k * self.T)) for k in range(n)]

    def set_net_policy(self, k, policy):
        self.uploads.append(k)
        self.engines[k].set_policy(policy)

    def population_selfplay_begin(self, *a, **kw):
        for e in self.engines:
            e.selfplay_begin(*a, **kw)

    def selfplay_step(self):
        for e in self.engines:
            e.selfplay_step()

    def selfplay_ring(self):
        return self.engines[0].selfplay_ring()

    def selfplay_rows(self, clear=True):
        parts = [e.selfplay_rows(clear=clear) for e in self.engines]
        steps = parts[0].shape[0] // self.T
        return np.stack([p.reshape(steps, self.T, -1) for p in parts], axis=1).reshape(steps * self.n_trees, -1)

    def selfplay_stats(self):
        parts = [e.selfplay_stats() for e in self.engines]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

    def close(self):
        for e in self.engines:
            e.close()


def _cpu_nets(n):
    from selfplay_train import build_agent
    nets = []
    for s in range(n):
        torch.manual_seed(40 + s)
        nets.append(build_agent("CartPole-v0", [16, 16], 5, "cpu", 1e-3)[0].nn)
    return nets


@pytest.mark.parametrize("fifo", [False, True])
def test_population_selfplay_splits_like_single_net_selfplay(fifo, monkeypatch):
    from alphazero_gym_amd import _native, run
    nets, T = _cpu_nets(3), 2
    kw = dict(game="CartPole-v0", n_rollouts=5, c_uct=1.5, epsilon=0.1, max_episode_length=4, capacity_steps=3, fifo=fifo,
              seed=9)
    monkeypatch.setattr(_native, "HipEngine", O.OracleEngine)
    singles = [run.DeviceSelfPlay(net, n_games=T, rank=k, **kw) for k, net in enumerate(nets)]
    monkeypatch.setattr(_native, "HipEngine", OracleSelfPlayPopulation)
    pop = run.PopulationSelfPlay(nets, games_per_net=T, **kw)
    assert pop.engine.uploads == [0, 1, 2] and pop.last_weight_sync == "host"
    plan = [(2, 0), (3, 0), (1, 4)] if fifo else [(2, 0), (3, 0), (1, 0)]   # (collect n, extra steps played before it; FIFO: wraps)
    for n, extra in plan:
        for sp in singles + [pop]:
            sp.play(extra)
        got = pop.collect(n)
        want = [sp.collect(n) for sp in singles]
        assert len(got) == 3
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.shape[0] == min(n + extra, 3) * T
            assert torch.equal(g, w)
        fsum, fcnt = pop.finished_returns()
        for k, sp in enumerate(singles):
            f, c, _ = sp.engine.selfplay_stats()
            acc = 0.0
            for x in f:
                acc += x
            assert fsum[k] == acc and fcnt[k] == c.sum()
    assert fcnt.sum() > 0
    # weights: only the changed net goes up again
    with torch.no_grad():
        next(nets[2].parameters()).add_(0.1)
    pop.engine.uploads.clear()
    pop.play(1)
    assert pop.engine.uploads == [2] and pop.last_weight_sync == "host"
    pop.play(1)
    assert pop.engine.uploads == [2] and pop.last_weight_sync is None
    for sp in singles:
        sp.engine.close()
    pop.close()


class RecordingOracle(O.OracleEngine):
    """The oracle engine, recording which weight-upload and self-play entry points are called."""

    calls = []

    def __getattribute__(self, name):
        if name in ("set_policy", "set_net_policy", "set_population", "set_population_policies", "selfplay_begin",
                    "population_selfplay_begin"):
            RecordingOracle.calls.append(name)
        return super().__getattribute__(name)


@pytest.mark.parametrize("fifo", [False, True])
def test_population_selfplay_of_one_policy_is_device_selfplay(fifo, monkeypatch):
    """A population of one plays on the plain engine (selfplay_begin, set_policy: the CPU oracle has no population entry points), and
    yields DeviceSelfPlay's rows and stats."""
    from alphazero_gym_amd import _native, run
    (net,), T = _cpu_nets(1), 3
    kw = dict(game="CartPole-v0", n_rollouts=5, c_uct=1.5, epsilon=0.1, max_episode_length=4, capacity_steps=3, fifo=fifo, seed=9)
    monkeypatch.setattr(_native, "HipEngine", O.OracleEngine)
    single = run.DeviceSelfPlay(net, n_games=T, rank=2, **kw)
    assert single.mcts.model is net   # (DeviceSelfPlay.mcts is still the single-net BatchedMCTS)
    monkeypatch.setattr(_native, "HipEngine", RecordingOracle)
    RecordingOracle.calls = []
    pop = run.PopulationSelfPlay([net], games_per_net=T, tree_id_base=2 * T, **kw)
    assert RecordingOracle.calls == ["set_policy", "selfplay_begin"] and pop.last_weight_sync == "host"
    for n, extra in ([(2, 0), (3, 0), (1, 4)] if fifo else [(2, 0), (3, 0), (1, 0)]):
        for sp in (single, pop):
            sp.play(extra)
        (got,), want = pop.collect(n), single.collect(n)
        assert got.shape == want.shape and torch.equal(got, want)
        fsum, fcnt = pop.finished_returns()
        f, c, _ = single.engine.selfplay_stats()
        acc = 0.0
        for x in f:
            acc += x
        assert fsum[0] == acc and fcnt[0] == c.sum()
    assert fcnt[0] > 0
    with torch.no_grad():
        next(net.parameters()).add_(0.1)
    RecordingOracle.calls = []
    pop.play(1)
    assert RecordingOracle.calls == ["set_policy"] and pop.last_weight_sync == "host"
    single.close()
    pop.close()


def test_selfplay_rejects_an_unknown_game(monkeypatch):
    """The game names are make_game's: an unknown one raises instead of playing CartPole."""
    from alphazero_gym_amd import _native, run
    monkeypatch.setattr(_native, "HipEngine", O.OracleEngine)
    kw = dict(game="Breakout-v0", n_rollouts=5, c_uct=1.5, capacity_steps=2)
    with pytest.raises(ValueError):
        run.DeviceSelfPlay(_cpu_nets(1)[0], n_games=2, **kw)
    monkeypatch.setattr(_native, "HipEngine", OracleSelfPlayPopulation)
    with pytest.raises(ValueError):
        run.PopulationSelfPlay(_cpu_nets(2), games_per_net=2, **kw)


def test_population_selfplay_argument_errors(monkeypatch):
    from alphazero_gym_amd import _native, run
    monkeypatch.setattr(_native, "HipEngine", OracleSelfPlayPopulation)
    kw = dict(game="CartPole-v0", n_rollouts=5, c_uct=1.5, capacity_steps=2)
    with pytest.raises(ValueError):
        run.PopulationSelfPlay([], games_per_net=2, **kw)
    with pytest.raises(ValueError):
        run.PopulationSelfPlay(_cpu_nets(2), games_per_net=0, **kw)
    pop = run.PopulationSelfPlay(_cpu_nets(2), games_per_net=2, **kw)
    with pytest.raises(AssertionError):
        pop.collect(3)   # more steps than the ring holds
    with pytest.raises(AssertionError):
        pop.play(3)
    pop.close()


def test_oracle_library_binds_without_the_population_selfplay_entry_points():
    """The CPU oracle lacks the new entry points: _capi binds it all the same, and the methods say so."""
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.5, gamma=1.0, num_actions=2)
    d = _capi.make_desc(4, [16], 2, "relu")
    for name in ("set_population_weights_device", "set_net_weights_device", "population_selfplay_begin"):
        assert name in _capi.OPTIONAL_SYMBOLS and name not in e._f
    with pytest.raises(NotImplementedError):
        e.population_selfplay_begin(5)
    with pytest.raises(NotImplementedError):
        e.set_population_weights_device(d, 0, 1, 1)
    with pytest.raises(NotImplementedError):
        e.set_net_weights_device(0, d, 0, 1)
    with pytest.raises(NotImplementedError):
        e.set_population_policies(_cpu_nets(1))
    e.close()
