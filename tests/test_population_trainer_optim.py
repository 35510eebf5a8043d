"""GPU: Adam and gradient clipping in the population trainer (azg_optim, the *_opt entry points, PopulationTrainer(optimizers="agents")).
The backward launch's deferred form writes the gradients first and runs norm, clip and update after the last layer: its gradients
against the fused form's bit for bit, the norm against a float64 sum, the clip and both update rules against torch's optimisers in
float64 with float32 torch as the yardstick, invariance in K, the composition of step and epoch, the end-to-end update, the ABI's
errors and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.buffers import DeviceReplay
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import ADAM, DEV, DIMS, OPT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SHAPES = TU.NARROW
TWO = [(SHAPES[0], 1), (SHAPES[2], 17)]              # a width-16 single layer with one row; three layers with padded rows


@pytest.mark.parametrize("shape,B", TWO, ids=["16_normal_B1", "3x128_gmm2_B17"])
def test_plain_rmsprop_runs_the_fused_kernel(shape, B):
    """backward_step_opt with RMSprop, no clipping and no grad_norms against backward_step: the same bits."""
    N = TU.native()
    in_dim, hidden, head, act = shape
    K = 2
    pols = [TU.policy(in_dim, hidden, head, act, 60 + k) for k in range(K)]
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in TU.data(K, B, in_dim, 1 + desc.n_dist, 5))
    tr = N.HipTrainer(desc, K, 64)
    p0, s0 = TU.flat(pols), torch.full((K, tr.n_params), 0.25, device=DEV)
    _, g0 = TU.step(tr, p0, obs, d_raw, _capi.rmsprop_opt(weight_decay=1e-4, **OPT), s0)
    p1, s1 = TU.flat(pols), torch.full((K, tr.n_params), 0.25, device=DEV)
    TU.forward(tr, p1, obs)
    g1 = torch.zeros_like(p1)
    tr.backward_step_opt(p1.data_ptr(), d_raw.data_ptr(), B, _capi.optim("rmsprop", OPT["lr"], s1.data_ptr(), alpha=OPT["alpha"],
                                                                          eps=OPT["eps"], weight_decay=1e-4), g1.data_ptr())
    tr.close()
    assert torch.equal(p0, p1) and torch.equal(s0, s1) and torch.equal(g0, g1)
    assert not torch.equal(p0, TU.flat(pols))


@pytest.mark.parametrize("shape,B", TWO, ids=["16_normal_B1", "3x128_gmm2_B17"])
def test_deferred_gradients_and_norm(shape, B):
    """The deferred form (Adam) hands back the fused form's gradients bit for bit, and grad_norms is sqrt(sum g^2) of them: the
    kernel's sum is float64 (exact products, 2^-53-scale chain error) rounded to float32 once, so it lies within one float32 ulp
    of the float64 value however that is summed."""
    N = TU.native()
    in_dim, hidden, head, act = shape
    K = 2
    pols = [TU.policy(in_dim, hidden, head, act, 60 + k) for k in range(K)]
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in TU.data(K, B, in_dim, 1 + desc.n_dist, 5))
    tr = N.HipTrainer(desc, K, 64)
    p0 = TU.flat(pols)
    _, g0 = TU.step(tr, p0, obs, d_raw, _capi.rmsprop_opt(**OPT), torch.zeros((K, tr.n_params), device=DEV))
    p1, m, v = TU.flat(pols), torch.zeros((K, tr.n_params), device=DEV), torch.zeros((K, tr.n_params), device=DEV)
    _, g1, norms = TU.step_opt(tr, p1, obs, d_raw, lambda n: _capi.optim("adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"],
                                                                   betas=ADAM["betas"], grad_norms=n))
    tr.close()
    assert torch.equal(g0, g1)
    assert not torch.equal(p1, TU.flat(pols)) and bool((m != 0).any()) and bool((v != 0).any())
    for k in range(K):
        want = float(torch.sqrt((g1[k].cpu().double() ** 2).sum()))
        got = float(norms[k])
        print(f"norm {shape} B={B} net {k}: kernel {got!r} float64 {want!r}")
        assert want > 0 and abs(got - want) <= float(np.spacing(np.float32(want)))


def test_clip():
    """RMSprop with clip_grad_norm_: a net whose norm is below the bound steps exactly as without clipping (coef == 1), a net above
    it as float64 clip_grad_norm_ + torch.optim.RMSprop step from the kernel's own gradients."""
    N = TU.native()
    in_dim, hidden, head, act = SHAPES[1]
    K, B = 3, 64
    pols = [TU.policy(in_dim, hidden, head, act, 80 + k) for k in range(K)]
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = TU.data(K, B, in_dim, 1 + desc.n_dist, 9)
    d_raw[0] *= 1e-3
    d_raw[2] *= 1e3
    obs, d_raw = obs.to(DEV), d_raw.to(DEV)
    tr = N.HipTrainer(desc, K, 64)
    mk = lambda sq, clip: (lambda n: _capi.optim("rmsprop", OPT["lr"], sq.data_ptr(), alpha=OPT["alpha"], eps=OPT["eps"],   # noqa: E731
                                                 grad_clip=clip, grad_norms=n))
    pa, sa = TU.flat(pols), torch.zeros((K, tr.n_params), device=DEV)
    _, ga, na = TU.step_opt(tr, pa, obs, d_raw, mk(sa, 0.0))
    clip = float(na[1])
    pb, sb = TU.flat(pols), torch.zeros((K, tr.n_params), device=DEV)
    _, gb, nb = TU.step_opt(tr, pb, obs, d_raw, mk(sb, clip))
    tr.close()
    print(f"clip: norms {na.tolist()}, bound {clip}")
    assert float(nb[0]) < clip < float(nb[2])
    assert torch.equal(na, nb) and torch.equal(ga, gb)
    assert torch.equal(pa[0], pb[0]) and torch.equal(sa[0], sb[0])
    assert not torch.equal(pa[2], pb[2])
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = TU.flat(pols)[2].cpu().to(dtype).clone().requires_grad_(True)
        p.grad = gb[2].cpu().to(dtype)
        torch.nn.utils.clip_grad_norm_([p], clip)
        o = torch.optim.RMSprop([p], momentum=0, centered=False, foreach=False, **OPT)
        o.step()
        res[dtype] = (p.detach(), o.state[p]["square_avg"])
    fails, sizes = [], TU.sizes(pols[0])
    TU.against_yardstick("clip params", pb[2].cpu(), res[torch.float64][0], res[torch.float32][0], sizes, fails)
    TU.against_yardstick("clip square_avg", sb[2].cpu(), res[torch.float64][1], res[torch.float32][1], sizes, fails)
    assert not fails, fails


@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_adam_step_given_gradient(weight_decay):
    """Three consecutive steps from step 0 and one from step 1000, no clip."""
    TU.check_adam_step_given_gradient(SHAPES[2], None, TU.policy(*SHAPES[2], 31), weight_decay, (0, 1, 2, 1000),
                                      f"adam step {{step}} wd {weight_decay}")


@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=["16_normal", "3x128_gmm2", "256x16_discrete3"])
def test_population_invariance(shape, B):
    """Adam + grad_clip + weight_decay, K = 5."""
    TU.check_population_invariance(shape, B, None, [TU.policy(*shape, 50 + k) for k in range(5)], forms=("adam",), grad_clip=0.05)


def _adam_agents(head, K, first_seed=0):
    """A0C-tuned agents with the reference's Adam settings, weight decay and a grad_clip of 0.5."""
    return TU.make_agents(head, "a0c_tuned", K, first_seed, optimizer=TU.ADAM_WD, clip=0.5)


@pytest.mark.parametrize("head", ["discrete", "gmm2"])
def test_step_is_forward_loss_backward(head):
    """step_opt against azg_trainer_forward + azg_trainer_loss + backward_step_opt on the same inputs."""
    K, B = 3, 24
    S, A = DIMS[head]
    one = PopulationTrainer(_adam_agents(head, K), max_batch=64, losses="device", optimizers="agents")
    parts = PopulationTrainer(_adam_agents(head, K), max_batch=64, losses="device", optimizers="agents")
    rows = TU.make_rows(head, K, B, 3)
    batch = TU.split_rows(rows, S, A)
    got = one.update(batch)
    obs, actions, counts, values = (t.contiguous() for t in (batch[0], batch[1], batch[2], batch[4]))
    t = parts.trainer
    raw, d_raw = torch.empty((K, B, t.n_raw), device=DEV), torch.empty((K, B, t.n_raw), device=DEV)
    table = torch.empty((K, len(_capi.LOSS_KEYS)), device=DEV)
    torch.cuda.synchronize()
    t.forward(parts.flat.data_ptr(), obs.data_ptr(), B, raw.data_ptr())
    t.loss(raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), B, A, parts.loss_cfg,
           _capi.alpha_state(0, parts.log_alpha.data_ptr(), parts.alpha_exp_avg.data_ptr(), parts.alpha_exp_avg_sq.data_ptr()),
           d_raw.data_ptr(), table.data_ptr())
    t.backward_step_opt(parts.flat.data_ptr(), d_raw.data_ptr(), B, parts._optim())
    parts.alpha_step, parts.opt_step = 1, 1
    TU.assert_same(TU.state_of_agents_optimisers(one), TU.state_of_agents_optimisers(parts), "step_opt against its parts")
    assert torch.equal(one.last_d_raw, d_raw) and torch.equal(one.last_raw, raw)
    want = table.cpu().tolist()
    for k in range(K):
        for key, val in got[k].items():
            assert val == want[k][_capi.LOSS_KEYS.index(key)], (k, key)
    assert bool((one.last_grad_norms > 0).all()) and not torch.equal(one.exp_avg, torch.zeros_like(one.exp_avg))
    one.close()
    parts.close()


@pytest.mark.parametrize("head", ["discrete", "gmm2"])
def test_epoch_is_its_steps(head):
    """epoch_opt (the array form) against its two minibatches, 16 + 24 rows, passed one by one to step_opt with step + m."""
    K, n, batch = 3, 40, 16
    S, A = DIMS[head]
    ref = PopulationTrainer(_adam_agents(head, K), max_batch=64, losses="device", optimizers="agents")
    ep = PopulationTrainer(_adam_agents(head, K), max_batch=64, losses="device", optimizers="agents")
    for epoch in range(2):   # (the second epoch starts from Adam step 2)
        rows = TU.make_rows(head, K, n, 100 + epoch)
        seeds = [11 + epoch, 22, 33]
        want = ref.train_on_rows(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
        got = ep.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
        assert got == want and all(np.isfinite(v) for g in got for v in g.values())
        TU.assert_same(TU.state_of_agents_optimisers(ref, 24), TU.state_of_agents_optimisers(ep, 24), f"epoch {epoch}")
        assert ep.opt_step == ep.alpha_step == 2 * (epoch + 1)
    ref.close()
    ep.close()


def test_ring_epoch_is_its_steps():
    """epoch_opt on the self-play ring (K = 3, T = 4, 10 steps: 40 rows per net, minibatches of 16 + 24) against step_opt on copies."""
    K, T, steps, batch = 3, 4, 10, 16
    S, A = DIMS["discrete"]
    agents = _adam_agents("discrete", K)
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, epsilon=0.1,
                                capacity_steps=16)
    assert sp.play_device(steps) == (steps, 0)
    copies = torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps))
    n = steps * T
    ring = PopulationTrainer(agents, max_batch=64, losses="device", optimizers="agents")
    ref = PopulationTrainer(_adam_agents("discrete", K), max_batch=64, losses="device", optimizers="agents")
    seeds = [3, 1, 4]
    order = np.stack([np.random.RandomState(s).permutation(n) for s in seeds])
    got = ring.train_epoch_ring(sp, order, batch_size=batch)
    want = ref.train_on_rows(copies, S, A, batch_size=batch, shuffle_seeds=seeds)
    assert got == want
    TU.assert_same(TU.state_of_agents_optimisers(ring, 24), TU.state_of_agents_optimisers(ref, 24), "ring")
    assert ring.opt_step == ring.alpha_step == 2
    ring.close()
    ref.close()
    sp.close()


def _f64_step(kind, cfg, agent, batch, clip):
    """The agent's optimiser step in float64 on the CPU: (parameters after it, the gradient norm before clipping)."""
    a = TU.twin(kind, cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    a.optimizer.zero_grad(set_to_none=True)
    a._loss(s, ac, c, v.reshape(-1, 1))["loss"].backward()
    norm = float(torch.nn.utils.clip_grad_norm_(a.nn.parameters(), clip))
    a.optimizer.step()
    return [t.detach() for t in _capi.policy_tensors(a.nn)[1]], norm


@pytest.mark.parametrize("losses", ["torch", "device"])
@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_end_to_end_update(kind, losses):
    """PopulationTrainer(optimizers="agents").update of K = 4 default agents with the reference's Adam settings and a grad_clip
    against their float64 twins' steps, float32 agent.update twins as the yardstick."""
    K, clip = 4, 0.1
    cfg, _ = TU.e2e_agents(kind, 0)
    cfg["optimizer"] = dict(run.ADAM)
    cfg["agent"] = dict(cfg["agent"], grad_clip=clip)
    from alphazero_gym_amd.envs import make_game
    env = make_game(cfg["game"])
    agents = []
    for k in range(K):
        torch.manual_seed(70 + k)
        agents.append(run.make_agent(kind, cfg, env, tree_id_base=k))
    m = cfg["mcts"]
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=8, n_rollouts=m["n_rollouts"], c_uct=m["c_uct"],
                                gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                capacity_steps=8)
    rows = sp.collect_device(8)
    S, A = sp.engine.s_obs, sp.engine.kmax
    sp.close()
    batches = TU.batches(rows, S, A)
    truth = [_f64_step(kind, cfg, a, b, clip) for a, b in zip(agents, batches)]
    print(f"{kind}: float64 gradient norms {[t[1] for t in truth]}, grad_clip {clip}")
    assert any(t[1] > clip for t in truth)
    yard_agents = [TU.twin(kind, cfg, a, DEV) for a in agents]
    yard = [y.update(b) for y, b in zip(yard_agents, batches)]
    tr = PopulationTrainer(agents, optimizers="agents", losses=losses)
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    norms = tr.last_grad_norms.cpu().tolist()
    for k in range(K):
        assert abs(norms[k] - truth[k][1]) <= 1e-5 * truth[k][1], (k, norms[k], truth[k][1])
        off = 0
        for i, (want, y) in enumerate(zip(truth[k][0], _capi.policy_tensors(yard_agents[k].nn)[1])):
            mine = tr.flat[k, off:off + want.numel()].view_as(want).cpu().double()
            off += want.numel()
            e_y, e_t = (y.detach().cpu().double() - want).abs().max(), (mine - want).abs()
            print(f"{kind} {losses} net {k} tensor {i}: agent.update float32 distance {float(e_y):.3g}, trainer distance {float(e_t.max()):.3g}")
            if not torch.all(e_t <= 4 * e_y + TU.ulp(want)):
                fails.append((k, i, float(e_y), float(e_t.max())))
    assert not fails, fails
    before = tr.flat.clone()
    tr.close()
    for k, a in enumerate(agents):
        off = 0
        for p in _capi.policy_tensors(a.nn)[1]:
            st = a.optimizer.state[p]
            assert float(st["step"]) == 1.0
            assert st["exp_avg"].data_ptr() == tr.exp_avg[k, off:].data_ptr()
            assert st["exp_avg"].untyped_storage().data_ptr() == tr.exp_avg.untyped_storage().data_ptr()
            off += p.numel()
        info = a.update(batches[k])
        assert np.isfinite(list(info.values())).all() and not torch.equal(tr.flat[k], before[k])
        assert float(a.optimizer.state[next(iter(a.nn.parameters()))]["step"]) == 2.0


def test_abi_errors():
    N = TU.native()
    desc = _capi.make_desc(4, [32, 32], 2, "relu")
    tr = N.HipTrainer(desc, 2, 64)
    params = torch.randn((2, tr.n_params), device=DEV)
    m, v = torch.zeros_like(params), torch.full_like(params, 0.25)
    keep = [t.clone() for t in (params, m, v)]
    obs, d_raw = (t.to(DEV) for t in TU.data(2, 64, 4, 3, 1))
    raw = torch.zeros((2, 64, 3), device=DEV)
    P, O, D, R, M, V = (t.data_ptr() for t in (params, obs, d_raw, raw, m, v))
    torch.cuda.synchronize()

    def code(*a):
        with pytest.raises(_capi.EngineError) as ei:
            tr.backward_step_opt(*a)
        assert str(ei.value)
        return ei.value.code

    def adam(**kw):
        return _capi.optim("adam", **dict(dict(lr=1e-3, state0=V, state1=M, eps=1e-7, betas=(0.9, 0.99)), **kw))

    INV, UNS = _capi.AZG_E_INVALID, _capi.AZG_E_UNSUPPORTED
    assert code(P, D, 64, adam()) == _capi.AZG_E_STATE   # no forward yet
    tr.forward(P, O, 64, R)
    assert code(P, D, 64, None) == INV
    assert code(None, D, 64, adam()) == INV
    assert code(P, None, 64, adam()) == INV
    assert code(P, D, 64, adam(state0=None)) == INV
    assert code(P, D, 64, adam(state1=None)) == INV
    assert code(P, D, 64, _capi.optim("rmsprop", 1e-3, None)) == INV
    bad = adam()
    bad.struct_size -= 4
    assert code(P, D, 64, bad) == INV
    assert code(P, D, 64, adam(lr=-1e-3)) == INV
    assert code(P, D, 64, adam(eps=-1e-7)) == INV
    assert code(P, D, 64, adam(betas=(1.0, 0.99))) == INV
    assert code(P, D, 64, adam(betas=(0.9, -0.1))) == INV
    assert code(P, D, 64, adam(grad_clip=-1.0)) == INV
    assert code(P, D, 64, adam(step=-1)) == INV
    assert code(P, D, 0, adam()) == INV
    assert code(P, D, 65, adam()) == INV
    assert code(P, D, 32, adam()) == _capi.AZG_E_STATE
    unknown = adam()
    unknown.kind = 7
    assert code(P, D, 64, unknown) == UNS
    # the first entry points answer as they always did
    with pytest.raises(_capi.EngineError) as ei:
        tr.backward_step(P, D, 64, _capi.rmsprop_opt(grad_clip=1.0, **OPT), V)
    assert ei.value.code == UNS
    # step_opt and epoch_opt make the same checks before their first launch
    A = 2
    act = torch.arange(A, dtype=torch.float32, device=DEV).repeat(2, 64, 1).contiguous()
    cnt, val, table = torch.ones((2, 64, A), device=DEV), torch.zeros((2, 64), device=DEV), torch.zeros((2, 5), device=DEV)
    cfg = _capi.AzgLossCfg()
    cfg.struct_size = C.sizeof(_capi.AzgLossCfg)
    cfg.kind, cfg.head, cfg.reduction, cfg.policy_coeff, cfg.value_coeff = _capi.LOSS_ALPHAZERO, _capi.HEAD_DISCRETE, 0, 1.0, 0.5
    for o, want in ((adam(state1=None), INV), (adam(grad_clip=-1.0), INV), (unknown, UNS), (None, INV)):
        with pytest.raises(_capi.EngineError) as ei:
            tr.step_opt(P, O, act.data_ptr(), cnt.data_ptr(), val.data_ptr(), 64, A, cfg, None, o, None, R, table.data_ptr())
        assert ei.value.code == want and str(ei.value)
    rows = torch.randn((2, 64, 4 + 3 * A + 1), device=DEV)
    rows[..., 4:4 + A] = act
    rows[..., 4 + A:4 + 2 * A] = 1.0
    where = _capi.epoch_rows(rows.data_ptr(), 4, A, 64)
    order = np.tile(np.arange(64, dtype=np.int32), (2, 1))
    sums = torch.zeros((2, 5), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    for o, want in ((adam(state0=None), INV), (adam(step=-1), INV), (unknown, UNS), (None, INV)):
        with pytest.raises(_capi.EngineError) as ei:
            tr.epoch_opt(P, where, order, 32, cfg, None, o, sums.data_ptr())
        assert ei.value.code == want and str(ei.value)
    for t, k in zip((params, m, v), keep):
        assert torch.equal(t, k)
    assert float(table.abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0
    # valid calls afterwards succeed
    tr.forward(P, O, 64, R)
    tr.backward_step_opt(P, D, 64, adam(grad_clip=1.0))
    assert not torch.equal(params, keep[0]) and not torch.equal(m, keep[1]) and not torch.equal(v, keep[2])
    tr.step_opt(P, O, act.data_ptr(), cnt.data_ptr(), val.data_ptr(), 64, A, cfg, None, adam(step=1), None, R, table.data_ptr())
    assert tr.epoch_opt(P, where, order, 32, cfg, None, adam(step=2), sums.data_ptr()) == 2
    assert torch.isfinite(params).all() and float(sums.abs().sum()) > 0.0
    tr.close()


def test_example_adam_clip():
    import population_selfplay_train as X
    base = ["--game", "CartPole-v0", "--seeds", "0", "1", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "10",
            "--train-rows", "64", "--batch-size", "32", "--hidden", "32", "32", "--device", DEV, "--optimizer", "adam", "--grad-clip", "1.0"]
    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None)
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None)
    assert len(fused) == len(epoch) == 2
    for a, b in zip(fused, epoch):
        assert len(a["loss"]) == 2 and np.isfinite(a["loss"]).all()
        assert a["loss"] == b["loss"] and a["mean_return"] == b["mean_return"]
