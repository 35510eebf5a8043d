"""GPU: LayerNorm trunks in the population trainer (azg_trainer_create_ex, PopulationTrainer(layernorm=True)) -- population
invariance bit for bit in both backward forms, the forward pass against the engine's azg_mlp_eval, gradients (ln.weight and ln.bias
included) against float64 autograd with float32 autograd as the yardstick, the optimiser step given the gradient, the end-to-end
update and epoch, the hand-off of the trained weights to the search, and that the feature is opt-in.  Every LayerNorm here has
gamma = 1 + 0.5 randn and beta = 0.5 randn, so that neither drops out of the arithmetic."""
import copy
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.network.policies import make_policy
from trainer_util import DEV, OPT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

KIND = "layernorm"


def _policy(in_dim, hidden, head, act, seed):
    return TU.policy(in_dim, hidden, head, act, seed, layernorm=True)


# (in_dim, hidden, head, activation): the smallest trunks that reach every path -- one tile per row; partial 64-column strips;
# three layers; the widest and the narrowest layer together
SHAPES = [
    (2, [16], ("normal",), "elu"),
    (4, [48, 80], ("discrete", 2), "relu"),
    (3, [128, 128, 128], ("gmm", 2), "elu"),
    (6, [256, 16], ("discrete", 3), "relu"),
]
SHAPE_IDS = ["16_normal", "48x80_discrete2", "3x128_gmm2", "256x16_discrete3"]


@pytest.mark.parametrize("form", ["fused_rmsprop", "adam_clip"])
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_population_invariance(shape, B, form):
    """K = 5, one backward form per case; the deferred form's grad_clip of 1e-3 is small enough to clip."""
    pols = [_policy(*shape, 50 + k) for k in range(5)]
    got = TU.check_population_invariance(shape, B, KIND, pols, forms=("fused",) if form == "fused_rmsprop" else ("adam",), grad_clip=1e-3)
    if form == "adam_clip":
        norms = got["adam"][5]
        assert bool((norms > 1e-3).all()), norms


ENGINE_SHAPES = [(4, [128, 128], ("discrete", 2), "relu"), SHAPES[2], SHAPES[3]]


@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=["cartpole", "pendulum_gmm2", "acrobot"])
def test_forward_against_engine(shape):
    TU.check_forward_against_engine(shape, KIND, _policy(*shape, 3), f"LayerNorm forward vs azg_mlp_eval {shape}")


GRAD_CASES = [(s, 128) for s in SHAPES] + [(SHAPES[1], 17), (SHAPES[2], 17)] + [
    ((4, [64, 32], ("discrete", 16), a), 128) for a in ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradients_against_autograd(shape, B):
    TU.check_gradients_against_autograd(shape, B, KIND, _policy(*shape, 21), f"LayerNorm grad {shape} B={B}")


@pytest.mark.parametrize("form", ["fused_rmsprop", "deferred_adam"])
def test_optimiser_step_given_gradient(form):
    """Three consecutive steps of the mixture shape."""
    TU.check_optimiser_step_given_gradient(SHAPES[2], KIND, _policy(*SHAPES[2], 31), form, "LayerNorm")


# ---------------------------------------------------------------------------------------------------------------- end to end
def _e2e_cfg(kind):
    base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
    return run._merge(base, dict(device=DEV, policy=dict(layernorm=True)))


def _agents_from(kind, cfg, states):
    from alphazero_gym_amd.envs import make_game
    env = make_game(cfg["game"])
    agents = []
    for k, sd in enumerate(states):
        a = run.make_agent(kind, cfg, env, tree_id_base=k)
        a.nn.load_state_dict({name: v.to(DEV) for name, v in sd.items()})
        agents.append(a)
    return agents


@functools.lru_cache(maxsize=None)
def _e2e(kind):
    """K = 4 LayerNorm nets (as CPU state_dicts) and 64 self-played rows per net (8 games x 8 steps), computed once per kind."""
    from alphazero_gym_amd.envs import make_game
    K = 4
    cfg = _e2e_cfg(kind)
    env = make_game(cfg["game"])
    agents = []
    for k in range(K):
        torch.manual_seed(70 + k)
        a = run.make_agent(kind, cfg, env, tree_id_base=k)
        assert a.nn.layernorm
        TU.randomise_layernorms(a.nn, 70 + k)
        agents.append(a)
    m = cfg["mcts"]
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=8, n_rollouts=m["n_rollouts"], c_uct=m["c_uct"],
                                gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                capacity_steps=8)
    rows = torch.stack([r.detach().clone() for r in sp.collect_device(8)])
    S, A = sp.engine.s_obs, sp.engine.kmax
    sp.close()
    states = tuple({name: v.detach().cpu().clone() for name, v in a.nn.state_dict().items()} for a in agents)
    return cfg, states, rows, S, A


@pytest.mark.parametrize("losses", ["torch", "device"])
@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_end_to_end_update(kind, losses):
    """PopulationTrainer(agents, layernorm=True).update against the float64 CPU twin, float32 agent.update as the yardstick (4 x);
    the step lands in the agents' own parameters; and the hand-off: after upload_flat a search of the population equals the search
    of a fresh PopulationMCTS built from policies holding those weights, so the trained gamma and beta reach the search kernels."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    cfg, states, rows, S, A = _e2e(kind)
    agents = _agents_from(kind, cfg, states)
    K = len(agents)
    batches = TU.batches(rows, S, A)
    truth = [TU.update_f64(kind, cfg, a, b) for a, b in zip(agents, batches)]
    yard = [TU.twin(kind, cfg, a, DEV).update(b) for a, b in zip(agents, batches)]
    with pytest.raises(ValueError, match="LayerNorm"):
        PopulationTrainer(agents, losses=losses)
    tr = PopulationTrainer(agents, layernorm=True, losses=losses, keep_grads=True)
    assert tr.desc.layernorm == 1 and tr.trainer.n_params == sum(p.numel() for p in agents[0].nn.parameters()) == tr.flat.shape[1]
    before = tr.flat.clone()
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    for key in yard[0]:
        e_y = max(abs(yard[k][key] - truth[k][key]) for k in range(K))
        e_t = max(abs(got[k][key] - truth[k][key]) for k in range(K))
        print(f"LayerNorm {kind} {losses} {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g} (largest of {K} nets)")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    assert not fails, fails
    # every parameter tensor moved (ln.weight and ln.bias too), its RMSprop state is a view of square_avg, its gradient was kept
    for k, a in enumerate(agents):
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], tr.flat[k].cpu().numpy())
        off = 0
        for name, p in zip([n for n, _ in a.nn.named_parameters()], _capi.policy_tensors(a.nn)[1]):
            sl = slice(off, off + p.numel())
            assert not torch.equal(tr.flat[k, sl], before[k, sl]), name
            assert bool((tr.grads[k, sl] != 0).any()) and bool((tr.square_avg[k, sl] != 0).any()), name
            assert a.optimizer.state[p]["square_avg"].data_ptr() == tr.square_avg[k, off:].data_ptr()
            off += p.numel()
        assert off == tr.flat.shape[1]
    # the hand-off
    m = cfg["mcts"]
    kw = dict(run._game_engine_kwargs(cfg["game"], agents[0].nn, m.get("c_pw", 1.0), m.get("kappa", 0.5)), trees_per_model=4,
              n_rollouts=m["n_rollouts"], c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"])
    pm = PopulationMCTS([a.nn for a in agents], **kw)
    got2 = tr.update(batches)   # behind torch's back: the engine's weights are now stale
    assert all(np.isfinite(list(g.values())).all() for g in got2)
    pm.upload_flat(tr.desc, tr.flat)
    assert pm.last_weight_sync == "device"
    pm.sync_weights()
    roots = pm.engine.synthetic_roots()
    pm.engine.set_search_index(5)
    pm.search(roots)
    res = pm.results()
    fresh_models = [copy.deepcopy(a.nn) for a in agents]
    for k, fm in enumerate(fresh_models):
        np.testing.assert_array_equal(_capi.policy_blob(fm)[1], tr.flat[k].cpu().numpy())
    fresh = PopulationMCTS(fresh_models, **kw)
    fresh.engine.set_search_index(5)
    fresh.search(roots)
    want = fresh.results()
    for key in want:
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    for x in (pm, fresh, tr):
        x.close()


@pytest.mark.parametrize("optimizers", ["rmsprop", "agents"])
@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_epoch_is_its_updates(kind, optimizers):
    """One train_epoch of three minibatches (48 rows, batch_size 16) equals three update calls on the same minibatches, bit for bit
    in flat, the optimiser state and the learned temperatures; afterwards the agents' own parameters are tr.flat[k]."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
    cfg, states, rows, S, A = _e2e(kind)
    if optimizers == "agents":
        cfg = dict(cfg, optimizer=dict(run.ADAM), agent=dict(cfg["agent"], grad_clip=0.1))
    rows = rows[:, :48].contiguous()
    K, n, batch = rows.shape[0], 48, 16
    seeds = [5, 6, 7, 8]
    assert minibatch_bounds(n, batch) == [(0, 16), (16, 32), (32, 48)]
    one = PopulationTrainer(_agents_from(kind, cfg, states), max_batch=64, losses="device", optimizers=optimizers, layernorm=True)
    ep = PopulationTrainer(_agents_from(kind, cfg, states), max_batch=64, losses="device", optimizers=optimizers, layernorm=True)
    order = torch.from_numpy(np.stack([np.random.RandomState(s).permutation(n) for s in seeds])).to(DEV)
    net = torch.arange(K, device=DEV)[:, None]
    sums = [{} for _ in range(K)]
    for i, j in minibatch_bounds(n, batch):
        b = rows[net, order[:, i:j]]
        infos = one.update((b[..., :S], b[..., S:S + A], b[..., S + A:S + 2 * A], b[..., S + 2 * A:S + 3 * A], b[..., -1]))
        for s, info in zip(sums, infos):
            for key, val in info.items():
                s[key] = s.get(key, 0.0) + val
    init = ep.flat.clone()
    got = ep.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
    assert got == sums and all(np.isfinite(v) for g in got for v in g.values())
    state = ("flat", "square_avg", "exp_avg", "exp_avg_sq", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq", "last_grad_norms")
    compared = 0
    for name in state:
        a, b = getattr(one, name), getattr(ep, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b), f"{name}: the epoch and its three updates differ"
            compared += 1
    assert compared >= 2 and (one.opt_step, one.alpha_step) == (ep.opt_step, ep.alpha_step)
    for k, a in enumerate(ep.agents):
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], ep.flat[k].cpu().numpy())
        assert not torch.equal(ep.flat[k], init[k])
    one.close()
    ep.close()


def test_opt_in_only():
    N = TU.native()
    f = N.fns()
    ln = _capi.make_desc(4, [128, 128], 2, "relu", layernorm=True)
    pol = _policy(4, [128, 128], ("discrete", 2), "relu", 1)
    assert bytes(_capi.policy_tensors(pol)[0]) == bytes(ln)
    tr = N.HipTrainer(ln, 2, 64, layernorm=True)
    assert tr.n_params == sum(p.numel() for p in pol.parameters()) == 4 * 128 + 128 * 128 + 2 * 3 * 128 + 3 * 128 + 3
    tr.close()
    with pytest.raises(_capi.EngineError) as ei:
        N.HipTrainer(ln, 2, 64)
    assert ei.value.code == _capi.AZG_E_UNSUPPORTED and "LayerNorm" in str(ei.value)
    # a trainer made by create_ex takes a plain descriptor too and gives the bits of azg_trainer_create's
    plain = make_policy(4, 1, "discrete", [48, 80], "relu", num_actions=2)
    desc = _capi.policy_tensors(plain)[0]
    obs, d_raw = (t.to(DEV) for t in TU.data(1, 17, 4, 3, 2))
    outs = []
    for kw in (dict(), dict(layernorm=True)):
        t = N.HipTrainer(desc, 1, 64, **kw)
        params, sq = TU.flat([plain]), torch.zeros((1, t.n_params), device=DEV)
        raw, grads = TU.step(t, params, obs, d_raw, _capi.rmsprop_opt(**OPT), sq)
        outs.append((raw, grads, params, sq))
        t.close()
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # the other limits are azg_trainer_create's; a wrong struct_size or a NULL options pointer is AZG_E_INVALID
    for bad in (_capi.make_desc(4, [512], 2, "relu", layernorm=True), _capi.make_desc(9, [64], 2, "relu", layernorm=True),
                _capi.make_desc(4, [40], 2, "relu", layernorm=True)):
        with pytest.raises(_capi.EngineError) as ei:
            N.HipTrainer(bad, 2, 64, layernorm=True)
        assert ei.value.code == _capi.AZG_E_UNSUPPORTED
    h = C.c_void_p()
    opts = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions) - 4, 1)
    assert f["trainer_create_ex"](0, C.byref(ln), 2, 64, C.byref(opts), C.byref(h)) == _capi.AZG_E_INVALID and not h.value
    assert f["trainer_last_error"](None)
    assert f["trainer_create_ex"](0, C.byref(ln), 2, 64, None, C.byref(h)) == _capi.AZG_E_INVALID and not h.value
    assert f["trainer_create_ex"](0, None, 2, 64, C.byref(_capi.AzgTrainerOptions(8, 1)), C.byref(h)) == _capi.AZG_E_INVALID
    opts0 = _capi.AzgTrainerOptions(8, 0)
    assert f["trainer_create_ex"](0, C.byref(ln), 2, 64, C.byref(opts0), C.byref(h)) == _capi.AZG_E_UNSUPPORTED and not h.value


def test_example_layernorm():
    """examples/population_selfplay_train.py --layernorm: the fused device trainer and the epoch trainer take the same steps."""
    import population_selfplay_train as X
    base = ["--game", "CartPole-v0", "--seeds", "0", "1", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "10",
            "--train-rows", "64", "--batch-size", "32", "--hidden", "32", "32", "--device", DEV, "--layernorm"]
    assert not X.parse_args(base[:-1]).layernorm
    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None)
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None)
    assert len(fused) == len(epoch) == 2
    for a, b in zip(fused, epoch):
        assert len(a["loss"]) == 2 and np.isfinite(a["loss"]).all() and a["weight_sync"] == "device"
        assert a["loss"] == b["loss"] and a["mean_return"] == b["mean_return"]
