"""GPU: the population trainer (include/azgym_train.h, agent/population_trainer.py) -- population invariance bit for bit, the
forward pass against the engine's azg_mlp_eval, gradients against float64 autograd with float32 autograd as the yardstick, the
RMSprop step given the gradient, the end-to-end PopulationTrainer.update, the ABI's errors and the example."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import _capi, run
from trainer_util import DEV, OPT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SHAPES = TU.NARROW


@pytest.mark.parametrize("B", [1, 17, 128, 383])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}in_{'x'.join(map(str, s[1]))}_{'_'.join(map(str, s[2]))}")
def test_population_invariance(shape, B):
    """Net k of a K = 5 trainer equals a K = 1 trainer on net k's data, bit for bit; so do two runs of the same call."""
    TU.check_population_invariance(shape, B, None, [TU.policy(*shape, 50 + k) for k in range(5)], forms=("fused",))


@pytest.mark.parametrize("shape", SHAPES[1:4], ids=["cartpole", "pendulum_gmm2", "acrobot"])
def test_forward_against_engine(shape):
    TU.check_forward_against_engine(shape, None, TU.policy(*shape, 3), f"forward vs azg_mlp_eval {shape}")


GRAD_CASES = [(s, 128) for s in SHAPES] + [(SHAPES[1], 17), (SHAPES[2], 17)] + [
    ((4, [64, 32], ("discrete", 16), a), 128) for a in ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradients_against_autograd(shape, B):
    TU.check_gradients_against_autograd(shape, B, None, TU.policy(*shape, 21), f"grad {shape} B={B}")


@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_optimiser_step_given_gradient(weight_decay):
    TU.check_rmsprop_step_given_gradient(SHAPES[2], None, TU.policy(*SHAPES[2], 31), weight_decay)


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_end_to_end_update(kind):
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    K = 4
    cfg, agents = TU.e2e_agents(kind, K)
    m = cfg["mcts"]
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=8, n_rollouts=m["n_rollouts"], c_uct=m["c_uct"],
                                gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                capacity_steps=8)
    rows = sp.collect_device(8)
    S, A = sp.engine.s_obs, sp.engine.kmax
    batches = TU.batches(rows, S, A)
    truth = [TU.update_f64(kind, cfg, a, b) for a, b in zip(agents, batches)]
    yard = [TU.twin(kind, cfg, a, DEV).update(b) for a, b in zip(agents, batches)]
    tr = PopulationTrainer(agents)
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    for key in yard[0]:
        e_y = max(abs(yard[k][key] - truth[k][key]) for k in range(K))
        e_t = max(abs(got[k][key] - truth[k][key]) for k in range(K))
        print(f"{kind} {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g} (largest of {K} nets)")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    assert not fails, fails
    for k, a in enumerate(agents):   # the step went into the agents' own parameters
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], tr.flat[k].cpu().numpy())
    # the hand-off: a search after upload_flat equals a search of a fresh engine built from policies loaded with the rows
    kw = dict(run._game_engine_kwargs(cfg["game"], agents[0].nn, m.get("c_pw", 1.0), m.get("kappa", 0.5)), trees_per_model=4,
              n_rollouts=m["n_rollouts"], c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"])
    pm = PopulationMCTS([a.nn for a in agents], **kw)
    got2 = tr.update(batches)   # behind torch's back: the engine's weights are now stale and no parameter's _version has moved
    assert all(np.isfinite(list(g.values())).all() for g in got2)
    pm.upload_flat(tr.desc, tr.flat)
    assert pm.last_weight_sync == "device"
    pm.sync_weights()
    assert pm.last_weight_sync is None
    roots = pm.engine.synthetic_roots()
    pm.engine.set_search_index(5)
    pm.search(roots)
    assert pm.last_weight_sync is None
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
    sp.upload_flat(tr.desc, tr.flat)
    sp.sync_weights()
    assert sp.last_weight_sync is None
    # close() hands the learned temperatures and their Adam state back to the agents' loss objects
    learned = tr.log_alpha.detach().cpu().clone()
    for x in (pm, fresh, sp, tr):
        x.close()
    for k, a in enumerate(agents):
        assert float(a.loss.log_alpha.detach()) == float(learned[k]) != float(np.log(1.0))
        assert float(a.loss.alpha.detach()) == float(learned[k].exp())
        assert float(a.loss.optimizer.state[a.loss.log_alpha]["step"]) == 2.0


def test_abi_errors():
    N = TU.native()
    f = N.fns()
    ln = _capi.make_desc(4, [128, 128], 2, "relu", layernorm=True)
    wide = _capi.make_desc(4, [512], 2, "relu")
    for bad in (ln, wide, _capi.make_desc(9, [64], 2, "relu"), _capi.make_desc(4, [64, 64, 64, 64], 2, "relu"), _capi.make_desc(4, [40], 2, "relu")):
        with pytest.raises(_capi.EngineError) as ei:
            N.HipTrainer(bad, 2, 64)
        assert ei.value.code == _capi.AZG_E_UNSUPPORTED and str(ei.value)
    desc = _capi.make_desc(4, [32, 32], 2, "relu")
    h = C.c_void_p()
    assert f["trainer_create"](0, None, 2, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create"](0, C.byref(desc), 0, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create"](0, C.byref(desc), 2, 0, C.byref(h)) == _capi.AZG_E_INVALID
    tr = N.HipTrainer(desc, 2, 64)
    params = torch.randn((2, tr.n_params), device=DEV)
    sq = torch.zeros_like(params)
    keep, keep_sq = params.clone(), sq.clone()
    obs, d_raw = (t.to(DEV) for t in TU.data(2, 64, 4, 3, 1))
    raw = torch.zeros((2, 64, 3), device=DEV)
    opt = _capi.rmsprop_opt(**OPT)
    torch.cuda.synchronize()

    def code(fn, *a):
        with pytest.raises(_capi.EngineError) as ei:
            fn(*a)
        assert str(ei.value)
        return ei.value.code

    P, O, D, R, S = params.data_ptr(), obs.data_ptr(), d_raw.data_ptr(), raw.data_ptr(), sq.data_ptr()
    assert code(tr.forward, None, O, 64, R) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, None, 64, R) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, O, 64, None) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, O, 0, R) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, O, 65, R) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # no forward yet
    tr.forward(P, O, 64, R)
    assert code(tr.backward_step, None, D, 64, opt, S) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, None, 64, opt, S) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, None, S) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, None) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 0, opt, S) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 65, opt, S) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 32, opt, S) == _capi.AZG_E_STATE      # not the forward's n_rows
    assert code(tr.backward_step, P, D, 64, _capi.rmsprop_opt(grad_clip=1.0, **OPT), S) == _capi.AZG_E_UNSUPPORTED
    assert code(tr.backward_step, P, D, 64, _capi.rmsprop_opt(momentum=0.9, **OPT), S) == _capi.AZG_E_UNSUPPORTED
    assert code(tr.backward_step, P, D, 64, _capi.rmsprop_opt(centered=True, **OPT), S) == _capi.AZG_E_UNSUPPORTED
    assert torch.equal(params, keep) and torch.equal(sq, keep_sq)
    tr.backward_step(P, D, 64, opt, S)   # the refused calls left the forward's state usable
    assert not torch.equal(params, keep)
    tr.close()


def test_example_trainers():
    import population_selfplay_train as X
    base = ["--game", "CartPole-v0", "--seeds", "0", "1", "2", "3", "--games-per-seed", "16", "--n-rollouts", "8", "--iters", "3",
            "--steps-per-iter", "10", "--train-rows", "150", "--batch-size", "64", "--device", DEV]
    assert X.parse_args(base).trainer == "torch"
    dev = X.train(X.parse_args(base + ["--trainer", "device"]), log=None)
    assert len(dev) == 3 and all(np.isfinite(r["loss"]).all() and len(r["loss"]) == 4 for r in dev)
    assert all(r["weight_sync"] == "device" for r in dev)
    # --trainer torch is the default, i.e. the loop that test_population_selfplay.py holds against K single-net loops.  Both
    # trainers start from the same nets and play the same first iteration.
    a = X.train(X.parse_args(base + ["--trainer", "torch"]), log=None)
    assert all(r["weight_sync"] == "device" and np.isfinite(r["loss"]).all() for r in a)
    assert dev[0]["mean_return"] == a[0]["mean_return"]
