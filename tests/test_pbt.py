"""GPU: population-based training's exploit/explore step (alphazero_gym_amd.pbt, PopulationTrainer.copy_nets,
PopulationSelfPlay.copy_nets).  A clone is held to its source bit for bit: it trains like it, the engine evaluates and plays it like
it, its settings are the source's, and what explore then changes is what the documented draw protocol gives."""
import os
import sys

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import pbt, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import DEV

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

K4, B8 = 4, 8
NARROW, WIDE = (16, 16), (272, 32)   # the wide kinds: the per-net tests' wide shape (several update workgroups per net)
LRS = [1e-3, 3e-4, 1e-2, 3e-3]
# name: (hidden, LayerNorm trunks, agents' optimiser per net, grad_clip, PopulationTrainer keywords)
CLONE_KINDS = {
    "rmsprop": (NARROW, False, [TU.RMSPROP_WD] * K4, 0, {}),
    "adam_clip": (NARROW, False, [TU.ADAM_WD] * K4, 0.5, dict(optimizers="agents")),
    "per_net": (NARROW, False, [dict(TU.RMSPROP_WD, lr=lr) for lr in LRS], 0, dict(optimizers="agents", per_net=True)),
    "layernorm": (NARROW, True, [TU.RMSPROP_WD] * K4, 0, dict(layernorm=True)),
    "wide": (WIDE, False, [TU.RMSPROP_WD] * K4, 0, dict(wide=True)),
    "wide_layernorm": (WIDE, True, [TU.RMSPROP_WD] * K4, 0, dict(wide_layernorm=True)),
}
CLONE_CASES = [(kind, "discrete", losses) for kind in CLONE_KINDS for losses in ("torch", "device")] + \
              [("rmsprop", "gmm2", "device"), ("wide", "gmm2", "torch")]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _population(kind, head, losses):
    hidden, ln, opts, clip, kw = CLONE_KINDS[kind]
    agents = [TU.make_agent(head, seed=k, hidden=hidden, layernorm=ln, optimizer=opts[k], grad_clip=clip, device=DEV) for k in range(K4)]
    return PopulationTrainer(agents, max_batch=32, losses=losses, **kw)


def _minibatch(head, seed):
    """B8 rows of trainer_util.make_batch as ``update``'s tuple (states, actions, counts, Q, V)."""
    s, a, c, v = (x[:B8] for x in TU.make_batch(head, seed))
    return (s, a, c, c, v)


def _trainer_state(tr):
    """Every per-net tensor of a trainer, by name (clones)."""
    out = {"flat": tr.flat, "square_avg": tr.square_avg, "exp_avg": tr.exp_avg, "exp_avg_sq": tr.exp_avg_sq, "log_alpha": tr.log_alpha}
    if tr.alpha_optimizer is not None:
        st = tr.alpha_optimizer.state[tr.log_alpha]
        out.update(alpha_exp_avg=st["exp_avg"], alpha_exp_avg_sq=st["exp_avg_sq"])
    else:
        out.update(alpha_exp_avg=tr.alpha_exp_avg, alpha_exp_avg_sq=tr.alpha_exp_avg_sq)
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


@pytest.mark.parametrize("kind,head,losses", CLONE_CASES, ids=["-".join(c) for c in CLONE_CASES])
def test_a_clone_trains_like_its_source(kind, head, losses):
    """Two identical populations A and B take two steps on four distinct minibatches; A.copy_nets([0, 1, 0, 1]); in a third step A's
    nets 2 and 3 get the minibatches of nets 0 and 1.  Then A's rows 2, 3 hold the bits of its rows 0, 1 in the parameters, every
    optimiser-state tensor and the alpha state, and A's rows 0, 1 hold B's: copying disturbed no bystander.  (That a net's bits do
    not depend on its index is trainer_util.check_population_invariance's, held by the existing suite.)"""
    A, B = _population(kind, head, losses), _population(kind, head, losses)
    for i in range(2):
        mbs = [_minibatch(head, 10 + 4 * i + k) for k in range(K4)]
        A.update(mbs)
        B.update(mbs)
    before = _trainer_state(A)
    assert set(before) >= {"flat", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq"} and len(before) >= 5
    for name, t in before.items():   # every state row is non-trivial and differs between the nets
        assert torch.isfinite(t).all() and bool((t != 0).any(dim=-1).all() if t.dim() > 1 else (t != 0).all()), name
        assert not _same_bits(t[2], t[0]) and not _same_bits(t[3], t[1]), name
    steps = (A.opt_step, A.alpha_step)
    A.copy_nets([0, 1, 0, 1])
    assert (A.opt_step, A.alpha_step) == steps
    after = _trainer_state(A)
    for name in before:
        assert _same_bits(after[name][2:], before[name][:2]) and _same_bits(after[name][:2], before[name][:2]), name
    if kind == "per_net":
        assert [a.optimizer.param_groups[0]["lr"] for a in A.agents] == [LRS[0], LRS[1], LRS[0], LRS[1]]
    # the agents' modules and torch optimisers are still views of the rows: they saw the copy
    for dst, src in ((2, 0), (3, 1)):
        for p, q in zip(A.agents[dst].nn.parameters(), A.agents[src].nn.parameters()):
            assert _same_bits(p, q) and p.data_ptr() != q.data_ptr()
            for name in ("square_avg", "exp_avg", "exp_avg_sq"):
                if name in A.agents[src].optimizer.state[q]:
                    assert _same_bits(A.agents[dst].optimizer.state[p][name], A.agents[src].optimizer.state[q][name])
    third = [_minibatch(head, 30 + k) for k in range(K4)]
    out_a = A.update([third[0], third[1], third[0], third[1]])
    out_b = B.update(third)
    got, ref = _trainer_state(A), _trainer_state(B)
    for name in got:
        assert _same_bits(got[name][2:], got[name][:2]), f"{name}: the clones left their sources"
        assert _same_bits(got[name][:2], ref[name][:2]), f"{name}: the copy disturbed nets 0 and 1"
        assert not _same_bits(got[name][:2], after[name][:2]) and torch.isfinite(got[name]).all(), name
    assert out_a[2] == out_a[0] and out_a[3] == out_a[1] and out_a[:2] == out_b[:2]
    for p, q in zip(A.agents[2].nn.parameters(), A.agents[0].nn.parameters()):
        assert _same_bits(p, q)
    A.close()
    B.close()


def test_copy_nets_refuses_before_writing():
    tr = _population("rmsprop", "discrete", "device")
    tr.update([_minibatch("discrete", 10 + k) for k in range(K4)])
    before = _trainer_state(tr)
    for bad in ([1, 2, 2, 3], [0, 1, 2], [0, 1, 2, 4]):
        with pytest.raises(ValueError, match="copy_nets"):
            tr.copy_nets(bad)
    tr.copy_nets([0, 1, 2, 3])
    after = _trainer_state(tr)
    assert all(_same_bits(before[n], after[n]) for n in before)
    tr.close()


# ---------------------------------------------------------------------------------------------------------------- the engine
def _cartpole(hidden, K, trainer_kw, lrs=None, **sp_kw):
    """K CartPole agents (weights from torch.manual_seed(k)), their self-play engine of 32 games each and their trainer."""
    from selfplay_train import build_agent
    agents = []
    for k in range(K):
        torch.manual_seed(k)
        agents.append(build_agent("CartPole-v0", list(hidden), 8, DEV, 1e-3 if lrs is None else lrs[k])[0])
    m = agents[0].mcts
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=32, n_rollouts=8, c_uct=m.c_uct, gamma=m.gamma,
                                epsilon=m.epsilon, max_episode_length=20, capacity_steps=4, **sp_kw)
    return agents, sp, PopulationTrainer(agents, max_batch=64, **trainer_kw)


OBS8 = np.random.RandomState(5).uniform(-0.2, 0.2, (8, 4)).astype(np.float32)


@pytest.mark.parametrize("hidden,K,kw,fraction", [((16, 16), 4, {}, 0.25), ((512, 512), 2, dict(wide=True), 0.5)], ids=["narrow", "wide"])
def test_the_engine_receives_the_clone(hidden, K, kw, fraction):
    """One step with an empty explore in which the last net copies net 0: the engine then evaluates and plays the last net as net 0."""
    agents, sp, tr = _cartpole(hidden, K, kw)
    last = K - 1
    raw0 = sp.mcts.evaluate_observations(OBS8, shared=True)[2]
    assert not np.array_equal(raw0[last], raw0[0])
    driver = pbt.PopulationBasedTraining(sp, tr, {}, fraction=fraction, seed=1)
    rec = driver.step([float(K - k) for k in range(K)])   # net 0 is the best, the last net the worst
    assert rec["src"] == list(range(last)) + [0] and rec["replaced"] == [last] and not rec["identity"] and driver.history == [rec]
    assert sp.last_weight_sync == "device"
    value, dist, raw = sp.mcts.evaluate_observations(OBS8, shared=True)
    for got, was in ((value, None), (dist, None), (raw, raw0)):
        assert np.array_equal(got[last].view(np.int32), got[0].view(np.int32))
        assert was is None or np.array_equal(got[:last].view(np.int32), was[:last].view(np.int32))
    ev = sp.evaluate(2, rule="mode")
    for name in ("returns", "lengths", "first_value"):
        assert np.array_equal(ev[name][last], ev[name][0]), name
    tr.close()
    sp.close()


C_UCTS, BUDGETS, N_STEPS, LAMBDAS = [0.5, 1.0, 1.5, 2.0], [8, 6, 4, 2], [1, 2, 3, 4], [1.0, 0.9, 0.8, 0.7]
EXPLORE = {"c_uct": {"factors": [0.8, 1.25], "min": 0.1, "max": 4.0},
           "n_rollouts": {"factors": [0.5, 0.75], "min": 1, "max": 8, "integer": True},
           "lr": {"factors": [0.5, 2.0], "min": 1e-5, "max": 1e-1}}


def _swept():
    return _cartpole((16, 16), 4, dict(optimizers="agents", per_net=True, losses="device"), lrs=LRS,
                     net_settings=[{"c_uct": c} for c in C_UCTS], net_rollouts=BUDGETS, n_step=N_STEPS, td_lambda=LAMBDAS)


def _everything(agents, sp, tr):
    tensors = _trainer_state(tr)
    host = dict(lrs=[a.optimizer.param_groups[0]["lr"] for a in agents], clips=[a.clip for a in agents],
                settings=[dict(e) for e in sp.mcts.net_settings], rollouts=list(sp.mcts.net_rollouts), n_step=list(sp.n_step),
                td_lambda=list(sp.td_lambda), target_gamma=sp.target_gamma)
    return tensors, host


def test_settings_travel_and_explore_is_reproducible():
    agents, sp, tr = _swept()
    seed = 12
    driver = pbt.PopulationBasedTraining(sp, tr, EXPLORE, fraction=0.25, seed=seed)
    rec = driver.step([4.0, 3.0, 2.0, 1.0])   # net 3 copies net 0, then perturbs what it inherited
    twin = np.random.Generator(np.random.PCG64(seed))   # the documented protocol: select's draw, then one draw per name, in order
    assert twin.integers(1) == 0
    want = {name: pbt.perturb(old, EXPLORE[name], twin) for name, old in (("c_uct", C_UCTS[0]), ("n_rollouts", BUDGETS[0]), ("lr", LRS[0]))}
    assert want["c_uct"] in (0.8 * 0.5, 1.25 * 0.5) and want["n_rollouts"] in (4, 6) and want["lr"] in (0.5 * LRS[0], 2.0 * LRS[0])
    assert rec["src"] == [0, 1, 2, 0]
    assert rec["explored"] == {3: {"c_uct": {"old": C_UCTS[0], "new": want["c_uct"]}, "n_rollouts": {"old": 8, "new": want["n_rollouts"]},
                                   "lr": {"old": LRS[0], "new": want["lr"]}}}
    assert driver.rng.bit_generator.state == twin.bit_generator.state
    assert [e["c_uct"] for e in sp.mcts.net_settings] == C_UCTS[:3] + [want["c_uct"]]
    assert all(e[key] == sp.mcts.net_settings[0][key] for e in sp.mcts.net_settings for key in ("gamma", "epsilon", "c_pw", "kappa"))
    assert sp.mcts.net_rollouts == BUDGETS[:3] + [want["n_rollouts"]]
    assert sp.n_step == N_STEPS[:3] + [N_STEPS[0]] and sp.td_lambda == LAMBDAS[:3] + [LAMBDAS[0]]
    assert [a.optimizer.param_groups[0]["lr"] for a in agents] == LRS[:3] + [want["lr"]]
    assert tr._net_opt_settings[3][1] == want["lr"] and tr._net_opt_settings[0][1] == LRS[0]   # reload_settings ran
    assert _same_bits(tr.flat[3], tr.flat[0]) and sp.last_weight_sync == "device"
    sp.play(2)
    order = np.stack([np.random.RandomState(k).permutation(64) for k in range(4)])
    infos = tr.train_epoch_ring(sp, order, batch_size=16)
    assert all(np.isfinite(i["loss"]) for i in infos) and torch.isfinite(tr.flat).all()
    assert not _same_bits(tr.flat[3], tr.flat[0])   # its own games and its own lr from here on
    tr.close()
    sp.close()


def test_a_refused_step_writes_nothing():
    """A spec whose max exceeds the engine's capacity: the budget 8 * 4 is clipped to 16, above n_rollouts = 8, which the budgets'
    check refuses before the first write."""
    agents, sp, tr = _swept()
    tr.update([_minibatch_cartpole(20 + k) for k in range(4)])   # (optimiser state worth comparing)
    explore = {"lr": EXPLORE["lr"], "n_rollouts": {"factors": [4.0], "min": 1, "max": 16, "integer": True}}
    driver = pbt.PopulationBasedTraining(sp, tr, explore, fraction=0.25, seed=3)
    tensors, host = _everything(agents, sp, tr)
    rng_state = driver.rng.bit_generator.state
    with pytest.raises(ValueError, match="net_rollouts"):
        driver.step([4.0, 3.0, 2.0, 1.0])
    tensors2, host2 = _everything(agents, sp, tr)
    assert host2 == host and set(tensors2) == set(tensors) and all(_same_bits(tensors[n], tensors2[n]) for n in tensors)
    assert driver.history == [] and driver.rng.bit_generator.state == rng_state
    sp.play(1)   # the engine still searches with the table it had
    tr.close()
    sp.close()


def _minibatch_cartpole(seed):
    rng = np.random.RandomState(seed)
    counts = rng.randint(0, 9, (B8, 2)).astype(np.float32)
    return (rng.randn(B8, 4).astype(np.float32), np.tile(np.arange(2, dtype=np.float32), (B8, 1)), counts, counts,
            rng.randn(B8).astype(np.float32))


def test_construction_names_the_argument_to_pass():
    agents, sp, tr = _cartpole((16, 16), 4, {})
    spec = {"factors": [0.8, 1.25], "min": 0.0, "max": 10.0}
    for name, arg in (("lr", "per_net=True"), ("tau", "per_net=True"), ("c_uct", "net_settings="), ("n_rollouts", "net_rollouts="),
                      ("n_step", "n_step=["), ("td_lambda", "td_lambda=["), ("target_gamma", "target_gamma=[")):
        with pytest.raises(ValueError, match=arg.replace("[", r"\[")):
            pbt.PopulationBasedTraining(sp, tr, {name: dict(spec, integer=True, min=1.0, max=1.0)})
    with pytest.raises(ValueError, match="not a hyper-parameter"):
        pbt.PopulationBasedTraining(sp, tr, {"momentum": spec})
    with pytest.raises(ValueError, match="fraction"):
        pbt.PopulationBasedTraining(sp, tr, {}, fraction=0.75)
    # a step that replaces nobody (floor(4 * 0.2) = 0) says so, writes nothing and draws nothing
    idle = pbt.PopulationBasedTraining(sp, tr, {}, fraction=0.2, seed=9)
    flat = tr.flat.clone()
    rec = idle.step([1.0, 2.0, 3.0, 4.0])
    assert rec == {"src": [0, 1, 2, 3], "identity": True, "replaced": [], "explored": {}} and idle.history == [rec]
    assert idle.rng.bit_generator.state == np.random.Generator(np.random.PCG64(9)).bit_generator.state
    assert _same_bits(tr.flat, flat)
    with pytest.raises(ValueError, match="scores must be"):
        idle.step([1.0, 2.0])

    class Two:
        n_nets = 2
    with pytest.raises(ValueError, match="2 nets, the trainer 4"):
        pbt.PopulationBasedTraining(Two(), tr, {})
    tr.close()
    sp.close()


@pytest.mark.parametrize("reset", [True, False])
def test_errors_of_replaced_nets_are_reset(reset):
    agents, sp, tr = _cartpole((16, 16), 4, dict(losses="device"), n_step=3, prioritized={"alpha": 0.6, "eps": 1e-3, "feedback": "max"})
    sp.play(2)
    order = np.stack([np.arange(64)] * 4)
    tr.train_epoch_ring(sp, order, batch_size=16, errors=True)
    before = sp.errors().reshape(-1, sp.n_games).copy()
    assert before.shape == (2, 128) and (before >= 0).all()   # every stored row was trained on
    sp.copy_nets([0, 1, 2, 0], reset_errors=reset)
    after = sp.errors().reshape(-1, sp.n_games)
    assert np.array_equal(after[:, :96], before[:, :96])
    if reset:
        assert (after[:, 96:] == -1.0).all()
    else:
        assert np.array_equal(after[:, 96:], before[:, 96:])
    with pytest.raises(ValueError, match="copy_nets"):
        sp.copy_nets([1, 2, 2, 3])
    tr.close()
    sp.close()


# ---------------------------------------------------------------------------------------------------------------- the example
TIMES = ("selfplay_s", "train_s", "sync_s", "elapsed_s")


def _records(hist):
    return [{k: v for k, v in h.items() if k not in TIMES} for h in hist]


def test_the_example_end_to_end():
    import argparse

    import population_selfplay_train as P
    common = ["--game", "CartPole-v0", "--seeds", "1", "2", "3", "4", "--games-per-seed", "32", "--n-rollouts", "8", "--iters", "4",
              "--steps-per-iter", "8", "--trainer", "device-epoch", "--lrs", "1e-5", "1e-3", "3e-3", "1e-1", "--hidden", "16", "16",
              "--device", "cuda"]
    hist = P.train(P.parse_args(common + ["--pbt-every", "2", "--pbt-explore", "lr", "--pbt-score", "selfplay"]), log=None)
    assert len(hist) == 4 and [i for i, h in enumerate(hist) if "pbt" in h] == [1, 3]
    for h in (hist[1], hist[3]):
        src = np.asarray(h["pbt"]["src"])
        assert src.shape == (4,) and np.array_equal(src[src], src) and int((src != np.arange(4)).sum()) == 1
        (k, moved), = h["pbt"]["explored"].items()
        assert int(k) == int(np.nonzero(src != np.arange(4))[0][0]) and moved["lr"]["new"] in (0.8 * moved["lr"]["old"], 1.25 * moved["lr"]["old"])
    assert np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    # without the flags the run is the one the example made before it had them: the parser's namespace, and one without the fields
    plain_args = P.parse_args(common)
    plain = P.train(plain_args, log=None)
    bare = argparse.Namespace(**{k: v for k, v in vars(plain_args).items() if not k.startswith("pbt_")})
    assert _records(P.train(bare, log=None)) == _records(plain) and not any("pbt" in h for h in plain)
    # and the iterations before the first step are the plain run's
    assert _records(hist)[0] == _records(plain)[0]
    assert {k: v for k, v in _records(hist)[1].items() if k != "pbt"} == _records(plain)[1]
