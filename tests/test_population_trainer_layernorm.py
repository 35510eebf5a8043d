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

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.network.policies import make_policy

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

DEV = "cuda"
U = 2.0 ** -24
OPT = dict(lr=1e-3, alpha=0.9, eps=1e-10)
ADAM = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-7)


def _native():
    from alphazero_gym_amd import _native as N
    N.lib()
    return N


def _randomise_layernorms(pol, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for mod in pol.trunk:
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_((1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g)).to(mod.weight.device))
                mod.bias.copy_((0.5 * torch.randn(mod.bias.shape, generator=g)).to(mod.bias.device))


def _policy(in_dim, hidden, head, act, seed):
    """head: ("discrete", n_actions) | ("normal",) | ("gmm", components); LayerNorm after every trunk activation"""
    torch.manual_seed(seed)
    if head[0] == "discrete":
        pol = make_policy(in_dim, 1, "discrete", list(hidden), act, num_actions=head[1], layernorm=True)
    else:
        pol = make_policy(in_dim, 1, "normal", list(hidden), act, num_components=1 if head[0] == "normal" else head[1], action_bound=2.0,
                          layernorm=True)
    _randomise_layernorms(pol, seed)
    return pol


def _flat(policies):
    return torch.from_numpy(np.stack([_capi.policy_blob(p)[1] for p in policies])).to(DEV)


def _raw_of(pol, x):
    h = pol.trunk(x)
    return torch.cat([pol.value_head(h), pol.dist_head(h)], dim=-1)


def _data(K, B, in_dim, n_raw, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((K, B, in_dim), generator=g)
    d_raw = torch.randn((K, B, n_raw), generator=g) / B
    return obs, d_raw


def _forward(tr, params, obs):
    K, B = obs.shape[:2]
    raw = torch.empty((K, B, tr.n_raw), device=DEV)
    torch.cuda.synchronize()
    tr.forward(params.data_ptr(), obs.data_ptr(), B, raw.data_ptr())
    return raw


def _step(tr, params, obs, d_raw, opt, sq):
    """One forward + fused backward/RMSprop step: (raw, grads); params and sq are updated in place."""
    raw = _forward(tr, params, obs)
    grads = torch.zeros_like(params)
    tr.backward_step(params.data_ptr(), d_raw.data_ptr(), obs.shape[1], opt, sq.data_ptr(), grads.data_ptr())
    return raw, grads


def _step_opt(tr, params, obs, d_raw, make_opt):
    """forward + backward_step_opt; make_opt(grad_norms address) -> azg_optim.  Returns (raw, grads, grad_norms)."""
    K, B = obs.shape[:2]
    raw = _forward(tr, params, obs)
    grads, norms = torch.zeros_like(params), torch.full((K,), -1.0, device=DEV)
    tr.backward_step_opt(params.data_ptr(), d_raw.data_ptr(), B, make_opt(norms.data_ptr()), grads.data_ptr())
    return raw, grads, norms


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
    """Net k of a K = 5 trainer equals a K = 1 trainer on net k's data, bit for bit (raw, gradients, parameters, optimiser state,
    and the norms of the deferred form); so do two runs of the same call."""
    N = _native()
    in_dim, hidden, head, act = shape
    K = 5
    pols = [_policy(in_dim, hidden, head, act, 50 + k) for k in range(K)]
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 1
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))

    def run_once(tr, ks):
        n = len(ks)
        params = _flat([pols[k] for k in ks])
        o, d = obs[ks].contiguous(), d_raw[ks].contiguous()
        if form == "fused_rmsprop":
            sq = torch.full((n, tr.n_params), 0.25, device=DEV)
            raw, grads = _step(tr, params, o, d, _capi.rmsprop_opt(weight_decay=1e-4, **OPT), sq)
            out = (raw, grads, params, sq)
        else:
            m, v = torch.full((n, tr.n_params), 0.01, device=DEV), torch.full((n, tr.n_params), 0.25, device=DEV)
            raw, grads, norms = _step_opt(tr, params, o, d, lambda nn: _capi.optim(
                "adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=1e-4, grad_clip=1e-3, step=3,
                grad_norms=nn))
            assert bool((norms > 1e-3).all()), norms   # small enough to clip
            out = (raw, grads, params, m, v, norms)
        return [t.cpu() for t in out]

    names = ("raw", "grads", "params", "square_avg") if form == "fused_rmsprop" else ("raw", "grads", "params", "exp_avg", "exp_avg_sq", "norms")
    runs = []
    for _ in range(2):
        tr = N.HipTrainer(desc, K, 512, layernorm=True)
        runs.append(run_once(tr, list(range(K))))
        tr.close()
    for a, b, name in zip(runs[0], runs[1], names):
        assert torch.equal(a, b), f"{name}: two runs differ"
    assert all(torch.isfinite(t).all() for t in runs[0]) and not torch.equal(runs[0][2], _flat(pols).cpu())
    tr1 = N.HipTrainer(desc, 1, 512, layernorm=True)
    for k in range(K):
        for a, b, name in zip(runs[0], run_once(tr1, [k]), names):
            assert torch.equal(a[k], b[0]), f"{name} of net {k}: K = 5 and K = 1 differ"
    tr1.close()


ENGINE_SHAPES = [(4, [128, 128], ("discrete", 2), "relu"), SHAPES[2], SHAPES[3]]


@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=["cartpole", "pendulum_gmm2", "acrobot"])
def test_forward_against_engine(shape):
    """raw against azg_mlp_eval's raw of a single-net engine with the same LayerNorm weights (T2: 1e-5; the engine's row statistics
    are float32 and its head sums chunked, so not bit for bit)."""
    N = _native()
    in_dim, hidden, head, act = shape
    pol = _policy(in_dim, hidden, head, act, 3)
    desc, blob = _capi.policy_blob(pol)
    if head[0] == "discrete":
        kw = dict(env_id={4: _capi.ENV_CARTPOLE, 6: _capi.ENV_ACROBOT}[in_dim], mode=_capi.MODE_DISCRETE, num_actions=head[1])
    else:
        kw = dict(env_id=_capi.ENV_PENDULUM_V0, mode=_capi.MODE_CONTINUOUS)
    e = N.HipEngine(n_trees=16, n_sims=8, c_uct=1.0, gamma=1.0, **kw)
    e.set_weights(desc, blob)
    B = 77
    obs, _ = _data(1, B, in_dim, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    tr = N.HipTrainer(desc, 1, 128, layernorm=True)
    raw = _forward(tr, _flat([pol]), obs.to(DEV))
    tr.close()
    err = np.abs(raw[0].cpu().numpy() - want).max()
    print(f"LayerNorm forward vs azg_mlp_eval {shape}: max abs difference {err:.3g}")
    assert err <= 1e-5


def _autograd(pol, obs, d_raw, dtype):
    p = copy.deepcopy(pol).to(dtype)
    raw = _raw_of(p, obs.to(dtype))
    (raw * d_raw.to(dtype)).sum().backward()
    return [t.grad for t in _capi.policy_tensors(p)[1]]


GRAD_CASES = [(s, 128) for s in SHAPES] + [(SHAPES[1], 17), (SHAPES[2], 17)] + [
    ((4, [64, 32], ("discrete", 16), a), 128) for a in ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradients_against_autograd(shape, B):
    """Truth: float64 autograd on CPU.  Yardstick: float32 autograd on CPU, error max|g32 - g64| / max|g64| per parameter tensor;
    the kernel's error by the same measure may be at most 4 x that, for ln.weight and ln.bias like the rest.  B = 17: padded rows
    must contribute nothing and nothing may be non-finite."""
    N = _native()
    in_dim, hidden, head, act = shape
    pol = _policy(in_dim, hidden, head, act, 21)
    desc, tensors = _capi.policy_tensors(pol)
    assert len(tensors) == 4 * len(hidden) + 4
    obs, d_raw = _data(1, B, in_dim, 1 + desc.n_dist, 13)
    g64 = _autograd(pol, obs[0], d_raw[0], torch.float64)
    g32 = _autograd(pol, obs[0], d_raw[0], torch.float32)
    tr = N.HipTrainer(desc, 1, 512, layernorm=True)
    n_params = tr.n_params
    params, sq = _flat([pol]), torch.zeros((1, n_params), device=DEV)
    raw, grads = _step(tr, params, obs.to(DEV), d_raw.to(DEV), _capi.rmsprop_opt(**OPT), sq)
    tr.close()
    grads = grads[0].cpu()
    assert torch.isfinite(raw).all() and torch.isfinite(grads).all() and torch.isfinite(params).all()
    off, fails = 0, []
    names = [n for n, _ in pol.named_parameters()]
    assert sum("trunk" in n and g.dim() == 1 for n, g in zip(names, g64)) == 3 * len(hidden)   # bias, ln.weight, ln.bias per layer
    for name, a64, a32 in zip(names, g64, g32):
        gk = grads[off:off + a64.numel()].view_as(a64).double()
        off += a64.numel()
        scale = a64.abs().max()
        e32, ek = float((a32.double() - a64).abs().max() / scale), float((gk - a64).abs().max() / scale)
        print(f"LayerNorm grad {shape} B={B} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g}")
        if not ek <= 4 * e32:
            fails.append((name, e32, ek))
    assert off == n_params == grads.numel() == sum(p.numel() for p in pol.parameters())
    assert not fails, fails


@pytest.mark.parametrize("form", ["fused_rmsprop", "deferred_adam"])
def test_optimiser_step_given_gradient(form):
    """Three consecutive steps of the mixture shape; after each, every parameter (gamma and beta included) against torch's optimiser
    in float64 fed the kernel's own gradients and started from the kernel's parameters and state: at most half an ulp of the
    parameter plus 16 * 2^-24 * |delta p|."""
    N = _native()
    in_dim, hidden, head, act = SHAPES[2]
    pol = _policy(in_dim, hidden, head, act, 31)
    desc = _capi.policy_tensors(pol)[0]
    tr = N.HipTrainer(desc, 1, 512, layernorm=True)
    wd = 1e-4
    params = _flat([pol])
    s0, s1 = torch.zeros_like(params), torch.zeros_like(params)   # square_avg | exp_avg_sq, exp_avg
    for step in range(3):
        obs, d_raw = (t.to(DEV) for t in _data(1, 64, in_dim, 1 + desc.n_dist, 40 + step))
        before, b0, b1 = (t[0].cpu().double().clone() for t in (params, s0, s1))
        ref = before.clone().requires_grad_(True)
        if form == "fused_rmsprop":
            _, grads = _step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=wd, **OPT), s0)
            ropt = torch.optim.RMSprop([ref], weight_decay=wd, momentum=0, centered=False, foreach=False, **OPT)
            ropt.state[ref] = {"step": torch.tensor(float(step)), "square_avg": b0.clone()}
        else:
            _, grads, _ = _step_opt(tr, params, obs, d_raw, lambda n: _capi.optim(
                "adam", ADAM["lr"], s0.data_ptr(), s1.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=wd, step=step))
            ropt = torch.optim.Adam([ref], weight_decay=wd, amsgrad=False, foreach=False, **ADAM)
            if step:
                ropt.state[ref] = {"step": torch.tensor(float(step)), "exp_avg": b1.clone(), "exp_avg_sq": b0.clone()}
        ref.grad = grads[0].cpu().double()
        ropt.step()
        got, want = params[0].cpu(), ref.detach()
        ulp = torch.from_numpy(np.spacing(np.abs(got.numpy()))).double()
        bound = 0.5 * ulp + 16 * U * (want - before).abs()
        err = (got.double() - want).abs()
        print(f"LayerNorm {form} step {step}: max err/bound {float((err / bound).max()):.3g}")
        assert torch.all(err <= bound)
        assert not torch.equal(got.double(), before)
    tr.close()


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
        _randomise_layernorms(a.nn, 70 + k)
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


def _batches(rows, S, A):
    return [(r[:, :S], r[:, S:S + A], r[:, S + A:S + 2 * A], r[:, S + 2 * A:S + 3 * A], r[:, -1]) for r in rows]


def _twin(kind, cfg, agent, device, dtype=torch.float32):
    from alphazero_gym_amd.envs import make_game
    a = run.make_agent(kind, dict(cfg, device=device), make_game(cfg["game"]))
    a.nn.load_state_dict({k: v.detach().to(device) for k, v in agent.nn.state_dict().items()})
    a.nn.to(dtype)
    return a


def _update_f64(kind, cfg, agent, batch):
    """The agent's loss dictionary in float64 on the CPU."""
    a = _twin(kind, cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    d = a._loss(s, ac, c, v.reshape(-1, 1))
    return {k: float(x.detach()) if hasattr(x, "detach") else float(x) for k, x in d.items()}


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
    batches = _batches(rows, S, A)
    truth = [_update_f64(kind, cfg, a, b) for a, b in zip(agents, batches)]
    yard = [_twin(kind, cfg, a, DEV).update(b) for a, b in zip(agents, batches)]
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
    N = _native()
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
    obs, d_raw = (t.to(DEV) for t in _data(1, 17, 4, 3, 2))
    outs = []
    for kw in (dict(), dict(layernorm=True)):
        t = N.HipTrainer(desc, 1, 64, **kw)
        params, sq = _flat([plain]), torch.zeros((1, t.n_params), device=DEV)
        raw, grads = _step(t, params, obs, d_raw, _capi.rmsprop_opt(**OPT), sq)
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
