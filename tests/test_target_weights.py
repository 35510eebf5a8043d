"""GPU: the engine's second weight set (include/azgym_target.h) behind ``upload_target_flat``, ``target_weights()`` and ``nets="target"``.

Engine A holds the weights W0 live and W1 as its target set; whatever it computes with ``nets="target"`` must hold the bytes an engine
with W1 live computes, and whatever it computes live afterwards the bytes of an engine with W0 that never had a target set.  Two
population shapes: two CartPole nets of [64, 64] with 11 games each (the one-launch search kernel), and two Pendulum nets of
[512, 512] with 32 games each, which the engine searches as teams of 32 trees with their own settle and weight-offset logic."""
import os
import sys

import numpy as np
import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.network.policies import make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {
    "cartpole": dict(make=lambda: make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2),
                     kw=dict(game="CartPole-v0", games_per_net=11, n_rollouts=8, c_uct=1.5)),
    "pendulum_team": dict(make=lambda: make_policy(3, 1, "normal", [512, 512], "elu", num_components=1, action_bound=2.0),
                          kw=dict(game="Pendulum-v0", games_per_net=32, n_rollouts=10, c_uct=0.05)),
}
COMMON = dict(max_episode_length=3, capacity_steps=3, fifo=True, seed=21)
W0, W1 = 60, 70   # the seeds of the two parameter sets' first nets


def _nets(case, first_seed):
    nets = []
    for s in range(2):
        torch.manual_seed(first_seed + s)
        nets.append(CASES[case]["make"]().to(DEV))
    return nets


def _flat(nets):
    """(desc, [K, P] float32 on the GPU) of the nets, in the engine's blob order."""
    desc = _capi.policy_blob(nets[0])[0]
    return desc, torch.from_numpy(np.stack([_capi.policy_blob(n)[1] for n in nets])).to(DEV)


def _selfplay(case, first_seed, **kw):
    return run.PopulationSelfPlay(_nets(case, first_seed), **CASES[case]["kw"], **COMMON, **kw)


def _same(got, want, what):
    assert set(got) == set(want)
    for key in want:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {key}"


def _differ(got, other):
    return any(np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(other[k]).tobytes() for k in got)


def _info(sp):
    return sp.engine.weights_info()


@pytest.mark.parametrize("case", list(CASES))
def test_evaluations_with_the_target_set(case):
    A, B, C = _selfplay(case, W0), _selfplay(case, W1), _selfplay(case, W0)
    assert _info(A) == {"in_use": "live", "target_ready": False}
    for call in (lambda: A.evaluate(2, nets="target"), lambda: A.evaluate_search(nets="target")):
        with pytest.raises(RuntimeError, match="upload_target_flat"):
            call()
    A.upload_target_flat(*_flat(_nets(case, W1)))
    assert _info(A) == {"in_use": "live", "target_ready": True} and _info(C) == {"in_use": "live", "target_ready": False}
    for name, call in (("evaluate", lambda sp, **kw: sp.evaluate(2, **kw)), ("evaluate_search", lambda sp, **kw: sp.evaluate_search(**kw))):
        target, live_b, live_c = call(A, nets="target"), call(B), call(C)
        _same(target, live_b, f"{name}(nets='target') against an engine with those weights live")
        assert _info(A)["in_use"] == "live"
        _same(call(A), live_c, f"{name}() after it against an engine that never had a target set")
        _same(call(A, nets="live"), live_c, f"{name}(nets='live')")
        # the two parameter sets give different results, or the equalities above would mean nothing (two untrained CartPole nets under
        # a search of 8 simulations act alike, measured up to 40 steps: there the raw-policy evaluation above is what tells them apart)
        assert _differ(live_b, live_c) or (case, name) == ("cartpole", "evaluate_search")
    if case == "pendulum_team":
        A.play(1)
        assert A.mcts.last_search_info["kernel_form"] in ("team", "per_layer")
    for sp in (A, B, C):
        sp.close()


@pytest.mark.parametrize("case", list(CASES))
def test_reanalysis_with_the_target_set_and_the_games_after_it(case):
    """A and B play 3 steps with W0; A reanalyses slot 1 with W1 as its target set, B after taking W1 as its live weights: the rings
    are equal.  Then A plays on as D does, which kept W0 and never reanalysed: LIVE is back and the games were left alone."""
    A, B, D = (_selfplay(case, W0, reanalyse=True) for _ in range(3))
    for sp in (A, B, D):
        sp.play(3)
    rows0 = A.engine.selfplay_rows(clear=False)
    assert rows0.tobytes() == B.engine.selfplay_rows(clear=False).tobytes() == D.engine.selfplay_rows(clear=False).tobytes()
    desc, flat1 = _flat(_nets(case, W1))
    A.upload_target_flat(desc, flat1)
    assert A.reanalyse(slots=[1], nets="target") == [1]
    assert _info(A)["in_use"] == "live"
    B.upload_flat(desc, flat1)
    assert B.reanalyse(slots=[1]) == [1]
    rows_a, rows_b = A.engine.selfplay_rows(clear=False), B.engine.selfplay_rows(clear=False)
    assert rows_a.tobytes() == rows_b.tobytes()
    G = A.n_games
    ra, r0 = rows_a.reshape(3, G, -1), rows0.reshape(3, G, -1)
    assert ra[1].tobytes() != r0[1].tobytes() and ra[[0, 2]].tobytes() == r0[[0, 2]].tobytes()
    A.play(1)
    D.play(1)
    ra, rd = A.engine.selfplay_rows(clear=False).reshape(3, G, -1), D.engine.selfplay_rows(clear=False).reshape(3, G, -1)
    S = A.engine.s_obs
    assert A.engine.selfplay_ring() == D.engine.selfplay_ring()
    assert ra[..., :S].tobytes() == rd[..., :S].tobytes()            # every stored observation
    assert ra[[0, 2]].tobytes() == rd[[0, 2]].tobytes()              # the new step's rows (slot 0, the ring wrapped) and the untouched slot
    assert ra[1].tobytes() != rd[1].tobytes()                        # ... and the reanalysed slot stays reanalysed
    for x, y in zip(A.finished_returns(), D.finished_returns()):
        assert x.tobytes() == y.tobytes()
    assert A.finished_returns()[1].sum() > 0                          # (episodes of 3 steps: some have finished)
    for sp in (A, B, D):
        sp.close()


def test_target_weights_restores_live_and_keeps_live_uploads_out():
    A, C = _selfplay("cartpole", W0), _selfplay("cartpole", W0)
    A.upload_target_flat(*_flat(_nets("cartpole", W1)))
    want_target, want_live = A.evaluate(2, nets="target"), C.evaluate(2)
    with pytest.raises(KeyError, match="inside"):
        with A.mcts.target_weights():
            assert _info(A) == {"in_use": "target", "target_ready": True}
            with pytest.raises(RuntimeError, match="already inside"):
                with A.mcts.target_weights():
                    pass
            assert _info(A)["in_use"] == "target"
            raise KeyError("inside")
    assert _info(A) == {"in_use": "live", "target_ready": True} and A.mcts._in_target is False
    _same(A.evaluate(2), want_live, "live after an exception inside target_weights()")
    # a live model changed inside the context is not written into the target set; it is uploaded, live, after it
    with A.mcts.target_weights():
        with torch.no_grad():
            for p in A.policies[0].parameters():
                p.mul_(1.25)
        A.sync_weights()
        A.sync_weights(force=True)
        inside = A.engine.policy_rollout(2, 3, rule="mode", game_id_base=run.EVAL_GAME_ID_BASE, episode=0)
    _same({k: inside[k] for k in inside}, {k: want_target[k] for k in inside}, "the target set inside the context")
    _same(A.evaluate(2, nets="target"), want_target, "the target set after a live model changed")
    assert _differ(A.evaluate(2), want_live)
    A.close()
    C.close()


def test_another_descriptor_empties_the_other_set():
    A = _selfplay("cartpole", W0)
    A.upload_target_flat(*_flat(_nets("cartpole", W1)))
    assert _info(A)["target_ready"]
    A.upload_flat(*_flat(_nets("cartpole", W1)))   # the same descriptor: the target set stays
    assert _info(A) == {"in_use": "live", "target_ready": True}
    small = []
    for s in range(2):
        torch.manual_seed(80 + s)
        small.append(make_policy(4, 1, "discrete", [32, 32], "relu", num_actions=2).to(DEV))
    A.upload_flat(*_flat(small))
    assert _info(A) == {"in_use": "live", "target_ready": False}
    for call in (lambda: A.evaluate(2, nets="target"), lambda: A.evaluate_search(nets="target")):
        with pytest.raises(RuntimeError, match="upload_target_flat"):
            call()
    assert np.isfinite(A.evaluate(2)["returns"]).all()   # the live set, of the new shape, plays
    # selecting the emptied set by hand: the engine's own no-weights refusal
    A.engine.use_weights("target")
    with pytest.raises(_capi.EngineError):
        A.engine.policy_rollout(2, 3, rule="mode", game_id_base=run.EVAL_GAME_ID_BASE, episode=0)
    A.engine.use_weights("live")
    with pytest.raises(_capi.EngineError, match="AZG_WEIGHTS_LIVE or AZG_WEIGHTS_TARGET"):
        A.engine.use_weights(2)
    assert np.isfinite(A.evaluate(2)["returns"]).all()
    A.close()


sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_the_example_trains_with_an_average_as_its_target_set():
    import population_selfplay_train as mod
    common = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "2", "--replay-steps", "4",
              "--reanalyse-slots", "2", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5",
              "--device", "cuda", "--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch", "--eval-episodes", "2"]
    hist = mod.train(mod.parse_args(common + ["--ema-decay", "0.9", "--reanalyse-target", "--eval-target"]), log=None)
    assert len(hist) == 2
    for key in ("loss", "mean_return", "eval_return"):
        assert np.isfinite(np.asarray([h[key] for h in hist], np.float64)).all(), key
    plain = mod.train(mod.parse_args(common), log=None)
    assert [sorted(h) for h in hist] == [sorted(h) for h in plain]   # (the records' keys are what they were)
    for argv in (["--reanalyse-target"], ["--eval-target"], ["--ema-every", "2"], ["--ema-decay", "1.0"],
                 ["--ema-decay", "0.9", "--trainer", "torch"], ["--ema-decay", "0.9", "--ema-every", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(common + argv)
