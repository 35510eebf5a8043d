"""GPU: LayerNorm trunks in the wide population trainer (azg_trainer_create_wide_ex, PopulationTrainer(wide_layernorm=True)).  Where
azg_trainer_create_ex's trainer takes the shape too, the wide one must give its bits; a descriptor without LayerNorm must give
azg_trainer_create_wide's.  On the wide shapes: population invariance and repeatability bit for bit in both backward forms, strips
of 2 and 4 tiles, gradients (ln.weight and ln.bias included) against float64 autograd with float32 autograd as the yardstick, the
forward pass against the engine, the optimiser steps given the gradient, the end-to-end update and epoch with the hand-off to the
search, the ABI's errors and the example.  Every LayerNorm here has gamma = 1 + 0.5 randn and beta = 0.5 randn, so that neither drops
out of the arithmetic."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import trainer_edges as E
import trainer_util as TU
from alphazero_gym_amd import _capi, run
from trainer_util import DEV, OPT, W1, W2, W5, WIDE

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

KIND = "wide_layernorm"
CLIP = 1e-3   # the deferred form's grad_clip in the bit-for-bit comparisons

# (in_dim, hidden, head, activation), all with LayerNorm.  The overlap with azg_trainer_create_ex: test_population_trainer_layernorm.py's
# four shapes and the largest net that trainer takes.
NARROW = [
    (2, [16], ("normal",), "elu"),
    (4, [48, 80], ("discrete", 2), "relu"),
    (3, [128, 128, 128], ("gmm", 2), "elu"),
    (6, [256, 16], ("discrete", 3), "relu"),
    (3, [256, 256, 256], ("normal",), "elu"),
]


def _id(s):
    return f"{s[0]}in_{'x'.join(map(str, s[1]))}_{'_'.join(map(str, s[2]))}_{s[3]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _policies(shape_key, K, first_seed, layernorm=True):
    """K policies of one shape, built once per module run and never changed (the trainers work on copies of their blobs)."""
    in_dim, hidden, head, act = shape_key
    return tuple(TU.policy(in_dim, list(hidden), head, act, first_seed + k, layernorm) for k in range(K))


def _two_trainers_same_bits(desc, K, max_batch, kinds, pols, obs, d_raw, what):
    """Both backward forms on a trainer of each of the two kinds: the same bits, and the second kind's are sane."""
    got = {}
    for kind in kinds:
        tr = TU.trainer(desc, K, max_batch, kind)
        assert tr.n_params == sum(p.numel() for p in pols[0].parameters())
        got[kind] = TU.run_forms(tr, pols, obs, d_raw, CLIP)
        tr.close()
    TU.same(got[kinds[0]], got[kinds[1]], what)
    TU.sane(got[kinds[1]], pols)


# ------------------------------------------------------------------------------------------------ 1. the first LayerNorm trainer's bits
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_overlap_bit_for_bit(shape, B):
    """An azg_trainer_create_wide_ex trainer and an azg_trainer_create_ex trainer on the same inputs: forward + backward_step, and
    forward + backward_step_opt with Adam, a clip, grad_norms and step 3, give the same bits in raw, grads, params, every optimiser
    state and the norms."""
    K = 3
    pols = _policies(TU.key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 1
    obs, d_raw = (t.to(DEV) for t in TU.data(K, B, shape[0], 1 + desc.n_dist, 7))
    _two_trainers_same_bits(desc, K, 512, ("layernorm", KIND), pols, obs, d_raw,
                            "the wide LayerNorm trainer's bits differ from azg_trainer_create_ex's")


def test_overlap_constant_row():
    """trainer_edges.py's LayerNorm net, whose all-zero observation gives a LayerNorm row of equal values (var = 0): the same bits."""
    pol = E.layernorm_net()
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = (t.unsqueeze(0).contiguous().to(DEV) for t in E.layernorm_data())
    _two_trainers_same_bits(desc, 1, 64, ("layernorm", KIND), [pol], obs, d_raw, "the wide LayerNorm trainer's bits differ on the constant row")


# ------------------------------------------------------------------------------------------------ 2. a descriptor without LayerNorm
@pytest.mark.parametrize("shape", [W1, (4, [128, 128], ("discrete", 2), "relu")], ids=_id)
def test_plain_descriptor_gives_create_wide_bits(shape):
    K, B = 3, 17
    pols = _policies(TU.key(shape), K, 50, False)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 0
    obs, d_raw = (t.to(DEV) for t in TU.data(K, B, shape[0], 1 + desc.n_dist, 7))
    _two_trainers_same_bits(desc, K, 512, ("wide", KIND), pols, obs, d_raw,
                            "azg_trainer_create_wide_ex differs from azg_trainer_create_wide on a plain trunk")


# ------------------------------------------------------------------------------------------------ 3. invariance and repeatability
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", WIDE, ids=_id)
def test_population_invariance(shape, B):
    """K = 3, the fused and the deferred form."""
    TU.check_population_invariance(shape, B, KIND, _policies(TU.key(shape), 3, 50), grad_clip=CLIP)


# ------------------------------------------------------------------------------------------------ 4. wider strips
def test_strip_rule_of_the_cases():
    TU.check_strip_rule_of_the_cases()


@pytest.mark.parametrize("K,B", [(16, 128), (16, 512), (8, 128)], ids=["K16_B128", "K16_B512", "K8_B128"])
def test_wider_strips(K, B):
    """The first and the last net of the K-net trainer against the K = 1 trainer."""
    TU.check_wider_strips(KIND, _policies(TU.key(W5), 16, 50)[:K], B, (0, K - 1), CLIP)


# ------------------------------------------------------------------------------------------------ 5. gradients against autograd
GRAD_CASES = [(s, 128) for s in WIDE] + [(W1, 17), (W2, 17)] + [
    ((4, [272, 32], ("discrete", 16), a), 128) for a in ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: _id(v))
def test_gradients_against_autograd(shape, B):
    TU.check_gradients_against_autograd(shape, B, KIND, _policies(TU.key(shape), 1, 21)[0], f"wide LayerNorm grad {_id(shape)} B={B}")


# ------------------------------------------------------------------------------------------------ 6. forward against the engine
ENGINE_SHAPES = [(4, [512, 272], ("discrete", 2), "relu"), (3, [1024, 1024], ("gmm", 2), "elu")]


@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=["cartpole_512x272", "pendulum_2x1024_gmm2"])
def test_forward_against_engine(shape):
    """At widths the engine pads to 512 and 1024."""
    TU.check_forward_against_engine(shape, KIND, _policies(TU.key(shape), 1, 3)[0], f"wide LayerNorm forward vs azg_mlp_eval {_id(shape)}",
                                    against_float64=True)


# ------------------------------------------------------------------------------------------------ 7. the optimiser steps
@pytest.mark.parametrize("form", ["fused_rmsprop", "deferred_adam"])
def test_optimiser_step_given_gradient(form):
    """Three consecutive steps of W2."""
    TU.check_optimiser_step_given_gradient(W2, KIND, _policies(TU.key(W2), 1, 31)[0], form, "wide LayerNorm")


# ------------------------------------------------------------------------------------------------ 8. end to end
E2E_HIDDEN = [512, 272]


def _e2e_cfg():
    return run._merge(run.CONTINUOUS_DEFAULTS, dict(device=DEV, policy=dict(hidden_dimensions=E2E_HIDDEN, layernorm=True)))


def _agents_from(cfg, states, device=DEV, dtype=torch.float32):
    from alphazero_gym_amd.envs import make_game
    env = make_game(cfg["game"])
    agents = []
    for k, sd in enumerate(states):
        a = run.make_agent("continuous", dict(cfg, device=device), env, tree_id_base=k)
        a.nn.load_state_dict({name: v.to(device) for name, v in sd.items()})
        a.nn.to(dtype)
        agents.append(a)
    return agents


@functools.lru_cache(maxsize=None)
def _e2e():
    """Two Pendulum [512, 272] LayerNorm nets (as CPU state_dicts) and 24 hand-made replay rows per net: obs (cos, sin, velocity) |
    5 actions inside the bound | 5 counts summing to 25 | 5 Q values (not read) | V."""
    from alphazero_gym_amd.envs import make_game
    cfg = _e2e_cfg()
    env = make_game(cfg["game"])
    K, n, A = 2, 24, 5
    states = []
    for k in range(K):
        torch.manual_seed(70 + k)
        a = run.make_agent("continuous", cfg, env, tree_id_base=k)
        assert a.nn.layernorm and list(a.nn.hidden_dimensions) == E2E_HIDDEN
        TU.randomise_layernorms(a.nn, 70 + k)
        states.append({name: v.detach().cpu().clone() for name, v in a.nn.state_dict().items()})
    g = torch.Generator().manual_seed(12)
    th = 3.0 * torch.randn((K, n), generator=g)
    obs = torch.stack([torch.cos(th), torch.sin(th), 2.0 * torch.randn((K, n), generator=g)], dim=-1)
    actions = 0.98 * 2.0 * torch.tanh(torch.randn((K, n, A), generator=g))
    extra = torch.randint(0, A, (K, n, 25 - A), generator=g)
    counts = torch.ones((K, n, A)).scatter_add_(2, extra, torch.ones(extra.shape))
    values = torch.randn((K, n, 1), generator=g)
    rows = torch.cat([obs, actions, counts, torch.zeros_like(actions), values], dim=-1).contiguous()
    return cfg, tuple(states), rows, 3, A


def _update_and_params_f64(agent, batch):
    """agent.update in float64 on the CPU (agent: a float64 CPU twin): the loss dictionary and the parameters after the step."""
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    agent.optimizer.zero_grad(set_to_none=True)
    d = agent._loss(s, ac, c, v.reshape(-1, 1))
    d["loss"].backward()
    agent.optimizer.step()
    info = {k: float(x.detach()) if hasattr(x, "detach") else float(x) for k, x in d.items()}
    return info, torch.cat([t.detach().reshape(-1) for t in _capi.policy_tensors(agent.nn)[1]])


def test_end_to_end_update_and_handoff():
    """PopulationTrainer(wide_layernorm=True, losses="device").update against agent.update on copies of the agents: truth is the
    float64 CPU run, the yardstick agent.update in float32; for every key of the loss dictionary and for the parameters after the
    step (one figure: the largest absolute error over the parameter vector, the larger of the two nets, as for each loss key) the
    trainer's error may be at most 4 x the yardstick's.  Then the trained weights of net 0 go into a one-net engine, a short search
    runs, and its mlp_eval agrees with the trainer's forward within 1e-5."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    cfg, states, rows_cpu, S, A = _e2e()
    rows = rows_cpu.to(DEV)
    K = rows.shape[0]
    batches = TU.batches(rows[:, :16], S, A)
    truth = [_update_and_params_f64(a, b) for a, b in zip(_agents_from(cfg, states, "cpu", torch.float64), batches)]
    yard_agents = _agents_from(cfg, states)
    yard = [a.update(b) for a, b in zip(yard_agents, batches)]
    yard_params = [torch.from_numpy(_capi.policy_blob(a.nn)[1]).double() for a in yard_agents]
    agents = _agents_from(cfg, states)
    with pytest.raises(ValueError, match="LayerNorm"):
        PopulationTrainer(agents, wide=True, losses="device")
    tr = PopulationTrainer(agents, wide_layernorm=True, losses="device")
    assert tr.desc.layernorm == 1 and tr.trainer.n_params == sum(p.numel() for p in agents[0].nn.parameters()) == tr.flat.shape[1]
    before = tr.flat.clone()
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    for key in yard[0]:
        e_y = max(abs(yard[k][key] - truth[k][0][key]) for k in range(K))
        e_t = max(abs(got[k][key] - truth[k][0][key]) for k in range(K))
        print(f"wide LayerNorm end to end {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g} (largest of {K} nets)")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    e_y = max(float((yard_params[k] - truth[k][1]).abs().max()) for k in range(K))
    e_t = max(float((tr.flat[k].cpu().double() - truth[k][1]).abs().max()) for k in range(K))
    print(f"wide LayerNorm end to end parameters after the step: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g}")
    if not e_t <= 4 * e_y:
        fails.append(("parameters", e_y, e_t))
    assert not fails, fails
    for k, a in enumerate(agents):   # the step went into the agents' own parameters, ln.weight and ln.bias too
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], tr.flat[k].cpu().numpy())
        off = 0
        for name, p in zip([n for n, _ in a.nn.named_parameters()], _capi.policy_tensors(a.nn)[1]):
            assert not torch.equal(tr.flat[k, off:off + p.numel()], before[k, off:off + p.numel()]), name
            off += p.numel()
    # the hand-off: net 0's trained weights in a one-net engine
    desc = tr.desc
    e = TU.engine_for(("gmm", 1))
    e.set_weights(desc, tr.flat[0].cpu().numpy())
    e.search(e.synthetic_roots())
    res = e.results()
    assert np.isfinite(res["Q"][res["counts"] > 0]).all() and np.isfinite(res["v_target"]).all() and (res["counts"].sum(axis=1) > 0).all()
    B = 77
    obs, _ = TU.data(K, B, S, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    raw = TU.forward(tr.trainer, tr.flat, obs.to(DEV))
    err = np.abs(raw[0].cpu().numpy() - want).max()
    print(f"wide LayerNorm end to end: trained net 0, trainer forward vs azg_mlp_eval max abs difference {err:.3g}")
    assert err <= 1e-5
    tr.close()


@pytest.mark.parametrize("optimizers", ["rmsprop", "agents"])
def test_epoch_is_its_updates(optimizers):
    """One train_epoch of three minibatches (24 rows, batch_size 8) equals three update calls on the same minibatches, bit for bit in
    flat, the optimiser state, the learned temperatures and the loss sums."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
    cfg, states, rows_cpu, S, A = _e2e()
    if optimizers == "agents":
        cfg = dict(cfg, optimizer=dict(run.ADAM), agent=dict(cfg["agent"], grad_clip=0.1))
    rows = rows_cpu.to(DEV)
    K, n, batch = rows.shape[0], rows.shape[1], 8
    seeds = [5, 6]
    assert minibatch_bounds(n, batch) == [(0, 8), (8, 16), (16, 24)]
    one = PopulationTrainer(_agents_from(cfg, states), max_batch=64, losses="device", optimizers=optimizers, wide_layernorm=True)
    ep = PopulationTrainer(_agents_from(cfg, states), max_batch=64, losses="device", optimizers=optimizers, wide_layernorm=True)
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


# ------------------------------------------------------------------------------------------------ 9. the ABI's errors
def test_abi_errors():
    N = TU.native()
    f = N.fns()
    on = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions), 1)
    off = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions), 0)
    short = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions) - 4, 1)
    desc = _capi.make_desc(4, [512, 32], 2, "relu", layernorm=True)
    h = C.c_void_p(12345)   # *out is untouched on every error

    def create(d, n_nets, max_batch, opts, out=True):
        return f["trainer_create_wide_ex"](0, C.byref(d) if d is not None else None, n_nets, max_batch,
                                           C.byref(opts) if opts is not None else None, C.byref(h) if out else None)

    for args in ((None, 2, 64, on), (desc, 2, 64, None), (desc, 2, 64, short), (desc, 0, 64, on), (desc, 2, 0, on)):
        assert create(*args) == _capi.AZG_E_INVALID, args[1:3]
        assert h.value == 12345 and f["trainer_last_error"](None)
    assert create(desc, 2, 64, on, out=False) == _capi.AZG_E_INVALID
    for hidden in ([16] * 9, [1040], [40], [512, 40]):
        bad = _capi.make_desc(4, hidden[:8], 2, "relu", layernorm=True)
        bad.n_hidden = len(hidden)
        assert create(bad, 2, 64, on) == _capi.AZG_E_UNSUPPORTED, hidden
        assert h.value == 12345 and f["trainer_last_error"](None)
    assert create(_capi.make_desc(9, [64], 2, "relu", layernorm=True), 2, 64, on) == _capi.AZG_E_UNSUPPORTED and h.value == 12345
    # opts.layernorm = 0: azg_trainer_create_wide, its refusal of a LayerNorm descriptor included
    assert create(desc, 2, 64, off) == _capi.AZG_E_UNSUPPORTED and h.value == 12345
    assert b"LayerNorm" in f["trainer_last_error"](None)
    plain = _capi.make_desc(4, [512, 32], 2, "relu")
    h2 = C.c_void_p()
    assert f["trainer_create_wide_ex"](0, C.byref(plain), 2, 64, C.byref(off), C.byref(h2)) == 0 and h2.value
    assert f["trainer_param_count"](h2) == 4 * 512 + 512 + 512 * 32 + 32 + 3 * 32 + 3
    f["trainer_destroy"](h2)
    # a LayerNorm handle: the parameter count has gamma and beta, and the entry points' own refusals are the wide trainer's
    tr = N.HipTrainer(desc, 2, 64, wide_layernorm=True)
    assert tr.n_params == 4 * 512 + 3 * 512 + 512 * 32 + 3 * 32 + 3 * 32 + 3
    params = torch.randn((2, tr.n_params), device=DEV)
    sq = torch.zeros_like(params)
    keep = [t.clone() for t in (params, sq)]
    obs, d_raw = (t.to(DEV) for t in TU.data(2, 64, 4, 3, 1))
    raw = torch.zeros((2, 64, 3), device=DEV)
    opt = _capi.rmsprop_opt(**OPT)
    torch.cuda.synchronize()

    def code(fn, *a):
        with pytest.raises(_capi.EngineError) as ei:
            fn(*a)
        assert str(ei.value)
        return ei.value.code

    def unchanged():
        return all(torch.equal(t, k) for t, k in zip((params, sq), keep))

    P, O, D, R, S = params.data_ptr(), obs.data_ptr(), d_raw.data_ptr(), raw.data_ptr(), sq.data_ptr()
    assert code(tr.forward, P, O, 65, R) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # no forward yet
    tr.forward(P, O, 64, R)
    assert code(tr.backward_step, P, D, 32, opt, S) == _capi.AZG_E_STATE      # not the forward's n_rows
    assert unchanged()
    tr.backward_step(P, D, 64, opt, S)
    assert not torch.equal(params, keep[0]) and not torch.equal(sq, keep[1]) and torch.isfinite(params).all()
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # the scratch is consumed
    tr.close()


# ------------------------------------------------------------------------------------------------ 10. the example
def test_example_wide_layernorm():
    """examples/population_selfplay_train.py --seeds 0 --hidden 512 272 --wide --layernorm: the fused device trainer and the epoch
    trainer take the same steps (same losses, same returns, same final parameters)."""
    import population_selfplay_train as X
    base = ["--seeds", "0", "--hidden", "512", "272", "--wide", "--layernorm", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2",
            "--steps-per-iter", "10"]
    a = X.parse_args(base)
    assert a.wide and a.layernorm
    final = {}

    def keep(name):
        return lambda agents: final.__setitem__(name, [_capi.policy_blob(ag.nn)[1].copy() for ag in agents])

    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None, on_end=keep("fused"))
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None, on_end=keep("epoch"))
    assert len(fused) == len(epoch) == 2
    for x, y in zip(fused, epoch):
        assert len(x["loss"]) == 1 and np.isfinite(x["loss"]).all() and x["weight_sync"] == "device"
        assert x["loss"] == y["loss"] and x["mean_return"] == y["mean_return"]
    assert len(final["fused"]) == 1 and np.isfinite(final["fused"][0]).all()
    np.testing.assert_array_equal(final["fused"][0], final["epoch"][0])
