"""GPU: the population trainer's losses on the device (azg_trainer_loss / azg_trainer_step, PopulationTrainer(losses="device")) --
d_raw and the loss values against float64 autograd with float32 PyTorch as the yardstick, determinism and population invariance
bit for bit, the learned temperature's Adam step, the end-to-end update against the losses="torch" path, the ABI's errors and
the example."""
import os
import sys

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from device_loss_util import HEADS, LOG_ALPHA0, alpha_tensors, kernel_loss, make_head, make_inputs, make_loss, make_trainer, torch_loss, ulp32
from trainer_util import DEV

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

CASES = [(h, "alphazero") for h in ("discrete2", "discrete3")] + [(h, l) for h in HEADS for l in ("a0c", "a0c_tuned")]


@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head,loss_name", CASES, ids=lambda v: str(v))
def test_d_raw_and_losses_against_autograd(head, loss_name, reduction, B):
    """Truth: population_loss in float64 on the CPU, .sum().backward().  Yardstick: the same in float32.  Per net the kernel's error
    (max|d_raw - truth| / max|truth|; |x - truth| per loss key) may be at most 4 x the yardstick's plus one float32 ulp of
    max|truth|; on the log_std columns d_raw is exactly 0 wherever the clamp gates the element, which is where autograd's zeros are (an
    element inside the clamp may still underflow to 0 in float32, so the kernel's zeros are held to autograd's float32 ones)."""
    K = 3
    policy, tr = make_trainer(head, K)
    loss = make_loss(loss_name, reduction)
    inputs = make_inputs(head, K, B, 1000 + B)
    tuned = loss_name == "a0c_tuned"
    la64 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float64, requires_grad=True) if tuned else None
    la32 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float32, requires_grad=True) if tuned else None
    truth, g64 = torch_loss(policy, loss, inputs, torch.float64, la64)
    yard, g32 = torch_loss(policy, loss, inputs, torch.float32, la32)
    state = None
    if tuned:
        la, m, v = alpha_tensors(K)
        state = _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr())
    got, d_raw = kernel_loss(tr, _capi.loss_cfg(policy, loss), inputs, state)
    tr.close()
    fails = []
    for k in range(K):
        scale = float(g64[k].abs().max())
        e_y = float((g32[k].double() - g64[k]).abs().max()) / scale
        e_k = float((d_raw[k].double() - g64[k]).abs().max()) / scale
        print(f"loss {head} {loss_name} {reduction} B={B} net {k} d_raw: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
        if not e_k <= 4 * e_y + ulp32(scale) / scale:
            fails.append(("d_raw", k, e_y, e_k))
        for slot, key in enumerate(_capi.LOSS_KEYS):
            if key not in truth:
                assert float(got[k, slot]) == 0.0, (key, k)
                continue
            t = float(truth[key][k])
            e_y, e_k = abs(float(yard[key][k]) - t), abs(float(got[k, slot]) - t)
            print(f"loss {head} {loss_name} {reduction} B={B} net {k} {key}: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
            if not e_k <= 4 * e_y + ulp32(t):
                fails.append((key, k, e_y, e_k))
    assert set(truth) == set(_capi.LOSS_KEYS_OF[_capi.loss_cfg(policy, loss).kind])
    assert not fails, fails
    kind, n, _ = HEADS[head]
    if kind != "discrete":
        cols = slice(2, 3) if kind == "normal" else slice(1 + n, 1 + 2 * n)
        ls = inputs[0][..., cols]
        gated = (ls < policy.log_param_min) | (ls > policy.log_param_max)
        if B > 1:
            assert gated.any() and not gated.all()
        assert bool((g64[..., cols][gated] == 0).all()) and bool((d_raw[..., cols][gated] == 0).all())
        assert torch.equal(d_raw[..., cols] == 0, g64[..., cols].float() == 0)


@pytest.mark.parametrize("B", [17, 128])
@pytest.mark.parametrize("head", ["gmm2", "discrete3"])
def test_determinism_and_population_invariance(head, B):
    """Two K = 5 calls give the same bits, and net k of them equals a K = 1 call on net k's slices: d_raw, losses and the alpha state."""
    K = 5
    policy, tr = make_trainer(head, K)
    cfg = _capi.loss_cfg(policy, make_loss("a0c_tuned", "mean", clip=0.5))
    inputs = make_inputs(head, K, B, 2000 + B)
    runs = []
    for _ in range(2):
        la, m, v = alpha_tensors(K)
        losses, d_raw = kernel_loss(tr, cfg, inputs, _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()))
        runs.append((d_raw, losses, la.cpu(), m.cpu(), v.cpu()))
    tr.close()
    names = ("d_raw", "losses", "log_alpha", "exp_avg", "exp_avg_sq")
    for a, b, name in zip(runs[0], runs[1], names):
        assert torch.equal(a, b), f"{name}: two runs differ"
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert not torch.equal(runs[0][2], torch.tensor(LOG_ALPHA0[:K]))
    _, tr1 = make_trainer(head, 1)
    for k in range(K):
        la, m, v = (t[k:k + 1].clone() for t in alpha_tensors(K))
        losses, d_raw = kernel_loss(tr1, cfg, tuple(x[k:k + 1] for x in inputs), _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()))
        for a, b, name in zip(runs[0], (d_raw, losses, la.cpu(), m.cpu(), v.cpu()), names):
            assert torch.equal(a[k], b[0]), f"{name} of net {k}: K = 5 and K = 1 differ"
    tr1.close()


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("head", ["gmm2", "discrete2"])
def test_alpha_step(head, clip):
    """Three consecutive calls.  After each: torch.optim.Adam in float64 on log_alpha, started from the kernel's state before the
    call and stepped by float64 population_loss, is the truth; the same in float32 is the yardstick.  log_alpha and both moments
    may be off by at most 4 x the yardstick's error plus one float32 ulp; the step count is the caller's and must be the reference's."""
    K, B = 3, 33
    policy, tr = make_trainer(head, K)
    loss = make_loss("a0c_tuned", "mean", clip=clip)
    cfg = _capi.loss_cfg(policy, loss)
    la, m, v = alpha_tensors(K)
    fails = []
    for step in range(3):
        inputs = make_inputs(head, K, B, 3000 + step)
        before = [t.cpu().clone() for t in (la, m, v)]
        refs = {}
        for dtype in (torch.float64, torch.float32):
            p = before[0].to(dtype).clone().requires_grad_(True)
            opt = torch.optim.Adam([p], lr=1e-3)
            if step:
                opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": before[1].to(dtype).clone(),
                                "exp_avg_sq": before[2].to(dtype).clone()}
            torch_loss(policy, loss, inputs, dtype, p, opt)
            assert float(opt.state[p]["step"]) == step + 1
            refs[dtype] = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
        kernel_loss(tr, cfg, inputs, _capi.alpha_state(step, la.data_ptr(), m.data_ptr(), v.data_ptr()))
        for name, got, t64, t32 in zip(("log_alpha", "exp_avg", "exp_avg_sq"), (la, m, v), refs[torch.float64], refs[torch.float32]):
            for k in range(K):
                t = float(t64[k])
                e_y, e_k = abs(float(t32[k]) - t), abs(float(got[k].cpu()) - t)
                print(f"alpha {head} clip {clip} step {step} net {k} {name}: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
                if not e_k <= 4 * e_y + ulp32(t):
                    fails.append((step, name, k, e_y, e_k))
        assert not torch.equal(la.cpu(), before[0])
    tr.close()
    assert not fails, fails


def _step_f64(kind, cfg, agent, batch):
    """The agent's whole optimiser step in float64 on the CPU: the parameters after it, in blob order."""
    a = TU.twin(kind, cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    a.optimizer.zero_grad(set_to_none=True)
    a._loss(s, ac, c, v.reshape(-1, 1))["loss"].backward()
    a.optimizer.step()
    return torch.cat([t.detach().reshape(-1) for t in _capi.policy_tensors(a.nn)[1]])


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_end_to_end_update(kind):
    """PopulationTrainer(losses="device").update on self-play rows: the returned dictionaries against the float64 truth within 4 x
    the error of a float32 agent.update twin; the step lands in the agents' parameters; close() hands log_alpha and Adam step 1
    back; and against a losses="torch" population from the same initial nets, after one step: per net, the device-loss parameters'
    largest distance from a float64 step of the same net may be at most 4 x that of the losses="torch" ones.  (The per-element
    bound 0.5 ulp + 16 * 2^-24 * |delta p| between the two paths, test_optimiser_step_given_gradient's, is too tight here: the
    two paths' d_raw differ by 1.5e-8 of the largest, and on one MI355X the largest err/bound was 1.42 for CartPole.)"""
    K = 4
    cfg, agents = TU.e2e_agents(kind, K)
    others = [TU.twin(kind, cfg, a, DEV) for a in agents]
    m = cfg["mcts"]
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=8, n_rollouts=m["n_rollouts"], c_uct=m["c_uct"],
                                gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                capacity_steps=8)
    rows = sp.collect_device(8)
    S, A = sp.engine.s_obs, sp.engine.kmax
    sp.close()
    batches = TU.batches(rows, S, A)
    truth = [TU.update_f64(kind, cfg, a, b) for a, b in zip(agents, batches)]
    p64 = torch.stack([_step_f64(kind, cfg, a, b) for a, b in zip(agents, batches)])
    yard = [TU.twin(kind, cfg, a, DEV).update(b) for a, b in zip(agents, batches)]
    before = torch.from_numpy(np.stack([_capi.policy_blob(a.nn)[1] for a in agents])).double()
    tr = PopulationTrainer(agents, losses="device")
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    for key in yard[0]:
        e_y = max(abs(yard[k][key] - truth[k][key]) for k in range(K))
        e_t = max(abs(got[k][key] - truth[k][key]) for k in range(K))
        print(f"device losses {kind} {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g} (largest of {K} nets)")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    assert not fails, fails
    for k, a in enumerate(agents):
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], tr.flat[k].cpu().numpy())
    assert tr.last_raw.shape == tr.last_d_raw.shape == (K, batches[0][0].shape[0], tr.trainer.n_raw)
    assert torch.isfinite(tr.last_d_raw).all() and bool((tr.last_d_raw != 0).any())
    # the losses="torch" population from the same initial nets
    tt = PopulationTrainer(others, losses="torch")
    tt.update(batches)
    p_dev, p_torch = tr.flat.cpu().double(), tt.flat.cpu().double()
    d_dev, d_torch = tr.last_d_raw.cpu().double(), tt.last_d_raw.cpu().double()
    print(f"device losses {kind}: d_raw of the two paths differ by {float((d_dev - d_torch).abs().max() / d_torch.abs().max()):.3g} of the largest")
    ulp = torch.from_numpy(np.spacing(np.abs(tt.flat.cpu().numpy()))).double()
    bound = 0.5 * ulp + 16 * 2.0 ** -24 * (p_torch - before).abs()
    err = (p_dev - p_torch).abs()
    print(f"device losses {kind}: parameters after one step, the two paths' max err/bound {float((err / bound).max()):.3g}")
    assert not torch.equal(p_dev, before)
    for k in range(K):
        e_t, e_d = float((p_torch[k] - p64[k]).abs().max()), float((p_dev[k] - p64[k]).abs().max())
        print(f"device losses {kind} net {k}: parameters against a float64 step, losses='torch' {e_t:.3g}, losses='device' {e_d:.3g}")
        assert e_d <= 4 * e_t
    tuned = tr.log_alpha is not None
    learned = tr.log_alpha.cpu().clone() if tuned else None
    tt.close()
    tr.close()
    if tuned:
        for k, a in enumerate(agents):
            assert float(a.loss.log_alpha.detach()) == float(learned[k]) != float(np.log(1.0))
            assert float(a.loss.alpha.detach()) == float(learned[k].exp())
            assert float(a.loss.optimizer.state[a.loss.log_alpha]["step"]) == 1.0


def test_abi_errors():
    N = TU.native()
    K, B, A = 2, 16, 5
    policy = make_head("gmm2")
    desc = _capi.policy_tensors(policy)[0]
    tr = N.HipTrainer(desc, K, 32)
    loss = make_loss("a0c_tuned", "mean")
    cfg = _capi.loss_cfg(policy, loss)
    inputs = [x.to(DEV).contiguous() for x in make_inputs("gmm2", K, B, 5)]
    raw, actions, counts, values = inputs
    g = torch.Generator().manual_seed(9)
    params = (0.1 * torch.randn((K, tr.n_params), generator=g)).to(DEV)
    obs = torch.randn((K, B, 3), generator=g).to(DEV)
    sq = torch.full_like(params, 0.25)
    d_raw = torch.full_like(raw, 7.0)
    losses = torch.full((K, 5), 7.0, device=DEV)
    la, m, v = alpha_tensors(K)
    written = (params, sq, d_raw, losses, la, m, v, raw)
    keep = [t.clone() for t in written]
    st = _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr())
    opt = _capi.rmsprop_opt(lr=1e-3, alpha=0.9, eps=1e-10)
    torch.cuda.synchronize()

    def code(fn, *a):
        with pytest.raises(_capi.EngineError) as ei:
            fn(*a)
        assert str(ei.value).split(": ", 1)[1]
        return ei.value.code

    def edit(obj, **kw):
        c = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    R, AC, CN, V, D, L = (t.data_ptr() for t in (raw, actions, counts, values, d_raw, losses))
    P, O, S = params.data_ptr(), obs.data_ptr(), sq.data_ptr()
    INV, UNS = _capi.AZG_E_INVALID, _capi.AZG_E_UNSUPPORTED
    good = [R, AC, CN, V, B, A, cfg, st, D, L]
    for i in (0, 1, 2, 3, 6, 7, 8, 9):   # every required pointer (the alpha state is required by the tuned loss)
        assert code(tr.loss, *[None if j == i else x for j, x in enumerate(good)]) == INV
    for rows in (0, 33):
        assert code(tr.loss, R, AC, CN, V, rows, A, cfg, st, D, L) == INV
    for n_act in (0, 17):
        assert code(tr.loss, R, AC, CN, V, B, n_act, cfg, st, D, L) == INV
    assert code(tr.loss, R, AC, CN, V, B, A, edit(cfg, struct_size=8), st, D, L) == INV
    assert code(tr.loss, R, AC, CN, V, B, A, cfg, edit(st, struct_size=8), D, L) == INV
    assert code(tr.loss, R, AC, CN, V, B, A, cfg, edit(st, log_alpha=None), D, L) == INV
    assert code(tr.loss, R, AC, CN, V, B, A, edit(cfg, kind=7), st, D, L) == UNS
    assert code(tr.loss, R, AC, CN, V, B, A, edit(cfg, kind=_capi.LOSS_ALPHAZERO), st, D, L) == UNS      # AlphaZeroLoss, continuous head
    assert code(tr.loss, R, AC, CN, V, B, A, edit(cfg, head=_capi.HEAD_NORMAL), st, D, L) == UNS         # n_dist = 6 is no Normal head
    six = N.HipTrainer(edit(desc, num_components=6), K, 32)
    assert code(six.loss, R, AC, CN, V, B, A, cfg, st, D, L) == UNS
    six.close()
    good = [P, O, AC, CN, V, B, A, cfg, st, opt, S, None, R, L]
    for i in (0, 1, 2, 3, 4, 7, 8, 9, 10, 13):
        assert code(tr.step, *[None if j == i else x for j, x in enumerate(good)]) == INV
    for rows in (0, 33):
        assert code(tr.step, P, O, AC, CN, V, rows, A, cfg, st, opt, S, None, R, L) == INV
    for n_act in (0, 17):
        assert code(tr.step, P, O, AC, CN, V, B, n_act, cfg, st, opt, S, None, R, L) == INV
    assert code(tr.step, P, O, AC, CN, V, B, A, edit(cfg, struct_size=8), st, opt, S, None, R, L) == INV
    assert code(tr.step, P, O, AC, CN, V, B, A, cfg, st, edit(opt, struct_size=8), S, None, R, L) == INV
    assert code(tr.step, P, O, AC, CN, V, B, A, edit(cfg, kind=7), st, opt, S, None, R, L) == UNS
    assert code(tr.step, P, O, AC, CN, V, B, A, edit(cfg, kind=_capi.LOSS_ALPHAZERO), st, opt, S, None, R, L) == UNS
    for bad in (dict(grad_clip=1.0), dict(momentum=0.9), dict(centered=1)):
        assert code(tr.step, P, O, AC, CN, V, B, A, cfg, st, edit(opt, **bad), S, None, R, L) == UNS
    assert code(tr.read_d_raw, B, D) == _capi.AZG_E_STATE      # no step yet
    for t, k in zip(written, keep):
        assert torch.equal(t, k)
    # the trainer is still usable: both calls, raw_out given and NULL
    tr.loss(R, AC, CN, V, B, A, cfg, st, D, L)
    assert torch.isfinite(d_raw).all() and torch.isfinite(losses).all() and not torch.equal(la, keep[4])
    tr.step(P, O, AC, CN, V, B, A, cfg, _capi.alpha_state(1, la.data_ptr(), m.data_ptr(), v.data_ptr()), opt, S, None, R, L)
    assert not torch.equal(params, keep[0]) and not torch.equal(raw, keep[7])
    first = losses.clone()
    params.copy_(keep[0]); sq.copy_(keep[1]); la.copy_(keep[4])
    torch.cuda.synchronize()
    tr.step(P, O, AC, CN, V, B, A, cfg, st, opt, S, None, None, L)
    tr.read_d_raw(B, D)
    assert torch.isfinite(d_raw).all() and torch.equal(losses[:, 1:3], first[:, 1:3])   # (alpha differs: policy and value losses)
    tr.close()


def test_example_device_fused():
    import population_selfplay_train as X
    base = ["--game", "CartPole-v0", "--seeds", "0", "1", "2", "3", "--games-per-seed", "16", "--n-rollouts", "8", "--iters", "3",
            "--steps-per-iter", "10", "--train-rows", "150", "--batch-size", "64", "--device", DEV]
    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None)
    assert len(fused) == 3 and all(np.isfinite(r["loss"]).all() and len(r["loss"]) == 4 for r in fused)
    assert all(r["weight_sync"] == "device" for r in fused)
    dev = X.train(X.parse_args(base + ["--trainer", "device"]), log=None)
    assert fused[0]["mean_return"] == dev[0]["mean_return"]
