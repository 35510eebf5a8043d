"""GPU: the wide population trainer (azg_trainer_create_wide, PopulationTrainer(wide=True)): nets of up to 8 hidden layers and widths
up to 1024, a launch per layer.  Where the first trainer takes the shape too, the wide one must give its bits; on the wide shapes:
population invariance and repeatability bit for bit in both backward forms, gradients against float64 autograd with float32 autograd
as the yardstick, the forward pass against the engine, the optimiser steps given the gradient, the end-to-end update with the epoch on
the self-play ring and the hand-off to the search, the ABI's errors and the example."""
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
from alphazero_gym_amd.agent.losses import A0CLossTuned, AlphaZeroLoss
from trainer_util import DEV, OPT, W1, W2, W5, WIDE

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

KIND = "wide"
NARROW = TU.NARROW   # the overlap: test_population_trainer.py's five shapes, which both trainers take
CLIP = 0.5          # the deferred form's grad_clip in the bit-for-bit comparisons


def _id(s):
    return f"{s[0]}in_{'x'.join(map(str, s[1]))}_{'_'.join(map(str, s[2]))}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _policies(shape_key, K, first_seed):
    """K policies of one shape, built once per module run and never changed (the trainers work on copies of their blobs)."""
    in_dim, hidden, head, act = shape_key
    return tuple(TU.policy(in_dim, list(hidden), head, act, first_seed + k) for k in range(K))


# ------------------------------------------------------------------------------------------------ 1. the overlap, bit for bit
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_overlap_bit_for_bit(shape, B):
    """A wide trainer and an azg_trainer_create trainer on the same inputs: forward + backward_step, and forward + backward_step_opt
    with Adam, a clip and grad_norms, give the same bits."""
    K = 3
    pols = _policies(TU.key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in TU.data(K, B, shape[0], 1 + desc.n_dist, 7))
    got = {}
    for kind in (None, KIND):
        tr = TU.trainer(desc, K, 512, kind)
        got[kind] = TU.run_forms(tr, pols, obs, d_raw, CLIP)
        tr.close()
    TU.same(got[None], got[KIND], "the wide trainer's bits differ")
    TU.sane(got[KIND], pols)


LOSS_CASES = [(NARROW[2], "a0c_tuned"), (NARROW[1], "alphazero")]


def _loss_inputs(head, K, B, seed):
    """(actions [K, B, A], counts [K, B, A], values [K, B]) as device_loss_util.py's make_inputs draws them."""
    g = torch.Generator().manual_seed(seed)
    if head[0] == "discrete":
        A = head[1]
        actions = torch.arange(A, dtype=torch.float32).repeat(K, B, 1)
        counts = torch.randint(0, 9, (K, B, A), generator=g).float()
    else:
        A = 5
        actions = 0.98 * 2.0 * torch.tanh(torch.randn((K, B, A), generator=g))
        extra = torch.randint(0, A, (K, B, 25 - A), generator=g)      # positive integers that sum to 25
        counts = torch.ones((K, B, A)).scatter_add_(2, extra, torch.ones(extra.shape))
    values = torch.randn((K, B), generator=g)
    return actions, counts, values


@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape,loss_name", LOSS_CASES, ids=["3x128_gmm2_a0c_tuned", "2x128_discrete2_alphazero"])
def test_overlap_step_and_epoch(shape, loss_name, B):
    """azg_trainer_step with the losses on the device, then azg_trainer_epoch over 40 rows in minibatches of 16 + 24: losses, d_raw,
    log_alpha, raw, params, square_avg and the epoch's loss sums of a wide trainer equal the first trainer's."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(TU.key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    if loss_name == "alphazero":
        loss = AlphaZeroLoss(policy_coeff=1.0, value_coeff=0.5, reduction="mean")
    else:
        loss = A0CLossTuned(action_dim=1, alpha_init=1.0, lr=1e-3, tau=0.1, policy_coeff=0.1, value_coeff=1.0, reduction="mean",
                            grad_clip=0.5, device="cpu")
    cfg = _capi.loss_cfg(pols[0], loss)
    obs, _ = TU.data(K, B, in_dim, 1, 7)
    actions, counts, values = _loss_inputs(head, K, B, 8)
    A = actions.shape[2]
    n = 40
    eobs, _ = TU.data(K, n, in_dim, 1, 9)
    eact, ecnt, eval_ = _loss_inputs(head, K, n, 10)
    rows = torch.cat([eobs, eact, ecnt, torch.zeros_like(eact), eval_.unsqueeze(-1)], dim=-1).to(DEV).contiguous()
    order = np.stack([np.random.RandomState(s).permutation(n) for s in (3, 1, 4)]).astype(np.int32)
    opt = _capi.rmsprop_opt(weight_decay=1e-4, **OPT)
    names = ("raw", "losses", "d_raw", "log_alpha", "params", "square_avg", "epoch sums", "params after the epoch", "log_alpha after it")
    got = {}
    for kind in (None, KIND):
        tr = TU.trainer(desc, K, 512, kind)
        params, sq = TU.flat(pols), torch.full((K, tr.n_params), 0.25, device=DEV)
        la = torch.tensor([float(np.log(a)) for a in (0.5, 1.0, 2.0)], device=DEV)
        m, v = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        tuned = loss_name == "a0c_tuned"
        raw, d_raw = torch.empty((K, B, tr.n_raw), device=DEV), torch.empty((K, B, tr.n_raw), device=DEV)
        table = torch.empty((K, len(_capi.LOSS_KEYS)), device=DEV)
        dev = [t.to(DEV).contiguous() for t in (obs, actions, counts, values)]
        torch.cuda.synchronize()
        tr.step(params.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), B, A, cfg,
                _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()) if tuned else None, opt, sq.data_ptr(), None,
                raw.data_ptr(), table.data_ptr())
        tr.read_d_raw(B, d_raw.data_ptr())
        out = [t.cpu().clone() for t in (raw, table, d_raw, la, params, sq)]
        sums = torch.zeros((K, len(_capi.LOSS_KEYS)), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        n_mb = tr.epoch(params.data_ptr(), _capi.epoch_rows(rows.data_ptr(), in_dim, A, n), order, 16, cfg,
                        _capi.alpha_state(1, la.data_ptr(), m.data_ptr(), v.data_ptr()) if tuned else None, opt, sq.data_ptr(),
                        sums.data_ptr())
        assert n_mb == 2
        got[kind] = out + [sums.cpu(), params.cpu(), la.cpu()]
        tr.close()
    for a, b, name in zip(got[None], got[KIND], names):
        assert torch.equal(a, b), f"{name}: the wide trainer's bits differ"
    assert torch.isfinite(got[KIND][1]).all() and torch.isfinite(got[KIND][6]).all()
    assert not torch.equal(got[KIND][4], TU.flat(pols).cpu()) and not torch.equal(got[KIND][7], got[KIND][4])
    if loss_name == "a0c_tuned":
        assert not torch.equal(got[KIND][3], torch.tensor([float(np.log(a)) for a in (0.5, 1.0, 2.0)]))


# ------------------------------------------------------------------------------------------------ 2. invariance and repeatability
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", WIDE, ids=_id)
def test_population_invariance(shape, B):
    """K = 3, the fused and the deferred form."""
    TU.check_population_invariance(shape, B, KIND, _policies(TU.key(shape), 3, 50), grad_clip=CLIP)


# ------------------------------------------------------------------------------------------------ 3. gradients against autograd
GRAD_CASES = [(s, 128) for s in WIDE] + [(W2, 17)]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: _id(v))
def test_gradients_against_autograd(shape, B):
    TU.check_gradients_against_autograd(shape, B, KIND, _policies(TU.key(shape), 1, 21)[0], f"grad {shape} B={B}")


# ------------------------------------------------------------------------------------------------ 3b. wider strips
def test_strip_rule_of_the_cases():
    TU.check_strip_rule_of_the_cases()


@pytest.mark.parametrize("K,B", [(16, 128), (16, 512), (8, 128)], ids=["K16_B128", "K16_B512", "K8_B128"])
def test_wider_strips(K, B):
    """Every net of the K-net trainer against the K = 1 trainer, and net 0's gradients pass the autograd check of
    test_gradients_against_autograd (factor 4 * sqrt(528 / 256) = 5.74)."""
    pols = _policies(TU.key(W5), 16, 50)[:K]
    got, obs, d_raw = TU.check_wider_strips(KIND, pols, B, range(K), CLIP)
    g64 = TU.autograd(pols[0], obs[0], d_raw[0], torch.float64)
    g32 = TU.autograd(pols[0], obs[0], d_raw[0], torch.float32)
    grads = got["fused"][1][0]
    off, fails = TU.hold_grads_to_autograd(f"grad {W5} K={K} B={B}", KIND, pols[0], grads, g64, g32, TU.grad_factor(KIND, W5[1]))
    assert off == grads.numel() and not fails, fails


# ------------------------------------------------------------------------------------------------ 4. forward against the engine
@pytest.mark.parametrize("shape", [W1, (3, [512, 512], ("gmm", 2), "elu")], ids=["cartpole_512", "pendulum_2x512_gmm2"])
def test_forward_against_engine(shape):
    TU.check_forward_against_engine(shape, KIND, _policies(TU.key(shape), 1, 3)[0], f"forward vs azg_mlp_eval {shape}")


# ------------------------------------------------------------------------------------------------ 5. the optimiser steps
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_rmsprop_step_given_gradient(weight_decay):
    """W2, test_optimiser_step_given_gradient's check and bound."""
    TU.check_rmsprop_step_given_gradient(W2, KIND, _policies(TU.key(W2), 1, 31)[0], weight_decay)


def test_adam_clip_step_given_gradient():
    """W2, three consecutive deferred steps with Adam and a grad_clip below the gradient's norm (test_population_trainer_optim.py's
    check and bounds)."""
    TU.check_adam_step_given_gradient(W2, KIND, _policies(TU.key(W2), 1, 31)[0], 1e-4, (0, 1, 2), "adam+clip step {step}", clip=0.01)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_end_to_end():
    """One continuous agent with hidden_dimensions [512, 272] and its DeviceSelfPlay of 16 games, 8 rollouts, 8 steps.  update's loss
    dictionary against float64 (trainer error <= 4 x agent.update's float32 error per key); train_epoch_ring against the same
    minibatches passed to a twin trainer's update one by one, bit for bit; after upload_flat a search equals that of a fresh engine."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
    from alphazero_gym_amd.envs import make_game
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    cfg = run._merge(run.CONTINUOUS_DEFAULTS, dict(device=DEV, policy=dict(hidden_dimensions=[512, 272])))
    torch.manual_seed(70)
    agent = run.make_agent("continuous", cfg, make_game(cfg["game"]))
    other = TU.twin("continuous", cfg, agent, DEV)
    m = cfg["mcts"]
    T, steps, batch_size = 16, 8, 32
    sp = run.DeviceSelfPlay(agent.nn, game=cfg["game"], n_games=T, n_rollouts=8, c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"],
                            c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5), capacity_steps=steps)
    assert sp.play_device(steps) == (steps, 0)
    S, A = sp.engine.s_obs, sp.engine.kmax
    rows = sp._split(DeviceReplay(sp.engine, 1).rows(), steps)[0]
    n = steps * T
    assert rows.shape[0] == n
    first = TU.split_rows(rows[:64], S, A)
    truth = TU.update_f64("continuous", cfg, agent, first)
    yard = TU.twin("continuous", cfg, agent, DEV).update(first)
    tr = PopulationTrainer([agent], wide=True, losses="device")
    ref = PopulationTrainer([other], wide=True, losses="device")
    got = tr.update([first])
    assert ref.update([first]) == got
    assert set(got[0]) == set(yard)
    fails = []
    for key in yard:
        e_y, e_t = abs(yard[key] - truth[key]), abs(got[0][key] - truth[key])
        print(f"wide continuous {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g}")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    assert not fails, fails
    np.testing.assert_array_equal(_capi.policy_blob(agent.nn)[1], tr.flat[0].cpu().numpy())   # the step went into the agent's parameters
    # the epoch on the ring against its minibatches one by one
    order = np.random.RandomState(5).permutation(n)[None, :]
    sums = tr.train_epoch_ring(sp, order, batch_size=batch_size)
    want = {}
    for i, j in minibatch_bounds(n, batch_size):
        info = ref.update([TU.split_rows(rows[torch.from_numpy(order[0, i:j]).to(DEV)], S, A)])[0]
        for key, val in info.items():
            want[key] = want.get(key, 0.0) + val
    assert sums[0] == want
    for name in ("flat", "square_avg", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq"):
        assert torch.equal(getattr(tr, name), getattr(ref, name)), f"{name}: the ring epoch and its steps differ"
    assert tr.alpha_step == ref.alpha_step == 1 + n // batch_size
    # the hand-off: a search after upload_flat equals a search of a fresh engine built from a copy of the policy
    kw = dict(run._game_engine_kwargs(cfg["game"], agent.nn, m.get("c_pw", 1.0), m.get("kappa", 0.5)), trees_per_model=T, n_rollouts=8,
              c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"])
    pm = PopulationMCTS([agent.nn], **kw)
    tr.update([first])   # behind torch's back: the engine's weights are now stale and no parameter's _version has moved
    pm.upload_flat(tr.desc, tr.flat)
    assert pm.last_weight_sync == "device"
    roots = pm.engine.synthetic_roots()
    pm.engine.set_search_index(5)
    pm.search(roots)
    res = pm.results()
    fresh_model = copy.deepcopy(agent.nn)
    np.testing.assert_array_equal(_capi.policy_blob(fresh_model)[1], tr.flat[0].cpu().numpy())
    fresh = PopulationMCTS([fresh_model], **kw)
    fresh.engine.set_search_index(5)
    fresh.search(roots)
    want = fresh.results()
    for key in want:
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    sp.upload_flat(tr.desc, tr.flat)
    for x in (pm, fresh, sp, tr, ref):
        x.close()


# ------------------------------------------------------------------------------------------------ 7. the ABI's errors
def test_abi_errors():
    N = TU.native()
    f = N.fns()
    for bad in (_capi.make_desc(4, [128, 128], 2, "relu", layernorm=True), _capi.make_desc(9, [64], 2, "relu"),
                _capi.make_desc(4, [40], 2, "relu"), _capi.make_desc(4, [1040], 2, "relu"), _capi.make_desc(4, [512, 40], 2, "relu")):
        with pytest.raises(_capi.EngineError) as ei:
            N.HipTrainer(bad, 2, 64, wide=True)
        assert ei.value.code == _capi.AZG_E_UNSUPPORTED and str(ei.value)
    desc = _capi.make_desc(4, [512, 32], 2, "relu")
    h = C.c_void_p()
    assert f["trainer_create_wide"](0, None, 2, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 0, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 2, 0, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 2, 64, None) == _capi.AZG_E_INVALID
    assert not h.value
    tr = N.HipTrainer(desc, 2, 64, wide=True)
    params = torch.randn((2, tr.n_params), device=DEV)
    sq = torch.zeros_like(params)
    mm, vv = torch.zeros_like(params), torch.full_like(params, 0.25)
    keep = [t.clone() for t in (params, sq, mm, vv)]
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
        return all(torch.equal(t, k) for t, k in zip((params, sq, mm, vv), keep))

    def adam(**kw):
        return _capi.optim("adam", **dict(dict(lr=1e-3, state0=vv.data_ptr(), state1=mm.data_ptr(), eps=1e-7, betas=(0.9, 0.99)), **kw))

    P, O, D, R, S = params.data_ptr(), obs.data_ptr(), d_raw.data_ptr(), raw.data_ptr(), sq.data_ptr()
    assert code(tr.forward, None, O, 64, R) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, O, 65, R) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # no forward yet
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 64, adam()) == _capi.AZG_E_STATE
    assert unchanged()
    tr.forward(P, O, 64, R)
    assert code(tr.backward_step, P, None, 64, opt, S) == _capi.AZG_E_INVALID
    assert unchanged()
    assert code(tr.backward_step, P, D, 32, opt, S) == _capi.AZG_E_STATE      # not the forward's n_rows
    assert unchanged()
    assert code(tr.backward_step, P, D, 64, _capi.rmsprop_opt(grad_clip=1.0, **OPT), S) == _capi.AZG_E_UNSUPPORTED
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 64, adam(state1=None)) == _capi.AZG_E_INVALID
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 32, adam()) == _capi.AZG_E_STATE
    assert unchanged()
    tr.backward_step(P, D, 64, opt, S)   # the refused calls left the forward's state usable
    assert not torch.equal(params, keep[0]) and not torch.equal(sq, keep[1])
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # the scratch is consumed
    tr.close()


# ------------------------------------------------------------------------------------------------ 8. the example
def test_example_wide():
    """examples/population_selfplay_train.py --seeds 0 --hidden 512 272 --wide: the fused device trainer and the epoch trainer take
    the same steps (same losses, same returns, same final parameters)."""
    import population_selfplay_train as X
    base = ["--seeds", "0", "--hidden", "512", "272", "--wide", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2",
            "--steps-per-iter", "10"]
    assert X.parse_args(base).wide and not X.parse_args([a for a in base if a != "--wide"]).wide
    final = {}

    def keep(name):
        return lambda agents: final.__setitem__(name, [_capi.policy_blob(a.nn)[1].copy() for a in agents])

    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None, on_end=keep("fused"))
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None, on_end=keep("epoch"))
    assert len(fused) == len(epoch) == 2
    for a, b in zip(fused, epoch):
        assert len(a["loss"]) == 1 and np.isfinite(a["loss"]).all() and a["weight_sync"] == "device"
        assert a["loss"] == b["loss"] and a["mean_return"] == b["mean_return"]
    assert len(final["fused"]) == 1 and np.isfinite(final["fused"][0]).all()
    np.testing.assert_array_equal(final["fused"][0], final["epoch"][0])
