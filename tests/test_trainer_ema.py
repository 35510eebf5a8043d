"""GPU: the moving average of the trainer's parameters (include/azgym_train_ema.h, PopulationTrainer(ema=...)).

The rule is held bit for bit.  A twin trainer without an average takes the same optimiser steps one minibatch at a time (the other
trainer tests establish that steps and epochs compose bit for bit), which gives the parameters after every step; tests/ema_util.py
applies the rule to those in numpy float32; ``trainer.ema`` after the native call must hold exactly those bits.  The twin's
parameters, optimiser state and returned losses must equal the averaging trainer's: the average disturbs nothing.

Shapes: TU.NARROW[0] (one hidden layer of 16; P = 99, so the 16-byte groups have a scalar tail and straddle the nets' boundaries) with
K = 3 and three decays, one of them 0; TU.NARROW[2] (3 x 128, a mixture of 2) with minibatches of 17 rows; Pendulum [512, 512] at K = 2
on the wide trainer; LayerNorm on both LayerNorm trainers; the smallest ring of the online-replay tests."""
import numpy as np
import pytest
import torch

import ema_util as E
import test_priority_feedback as TF
import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent import population_trainer as PT
from alphazero_gym_amd.agent.agents import ContinuousAgent, DiscreteAgent
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
from trainer_util import DEV

pytestmark = pytest.mark.gpu

SMALL, GMM = TU.NARROW[0], TU.NARROW[2]
PENDULUM_WIDE = (3, [512, 512], ("normal",), "elu")
DECAYS = [0.9, 0.0, 0.999]
LOSS_TUNED = dict(run.LOSS_TUNED, device=DEV)
PRIO = {"alpha": 0.6, "eps": 1e-3, "beta": 0.4, "feedback": "max"}


def _actions(shape):
    return shape[2][1] if shape[2][0] == "discrete" else 4


def _agents(shape, K, loss, optimizer=TU.RMSPROP_WD, clip=None, layernorm=False, lrs=None):
    """K GPU agents of ``shape`` (trainer_util's (in_dim, hidden, head, activation)); net k's weights from torch.manual_seed(k): two
    calls give identical populations.  ``lrs``: net k's learning rate."""
    in_dim, hidden, head, act = shape
    loss_cfg = LOSS_TUNED if loss == "a0c_tuned" else TU.LOSSES[loss]
    agents = []
    for k in range(K):
        torch.manual_seed(k)
        opt = optimizer if lrs is None else dict(optimizer, lr=lrs[k])
        if head[0] == "discrete":
            cfg = run.DISCRETE_DEFAULTS
            pol = dict(cfg["policy"], hidden_dimensions=list(hidden), nonlinearity=act, representation_dim=in_dim, action_dim=1,
                       num_actions=head[1], layernorm=layernorm)
            extra = cfg["agent"] if clip is None else dict(cfg["agent"], grad_clip=clip)
            a = DiscreteAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=DEV, num_actions=head[1]), loss_cfg=loss_cfg,
                              optimizer_cfg=opt, device=DEV, **extra)
        else:
            cfg = run.CONTINUOUS_DEFAULTS
            pol = dict(cfg["policy"], hidden_dimensions=list(hidden), nonlinearity=act, representation_dim=in_dim, action_dim=1,
                       action_bound=2.0, num_components=1 if head[0] == "normal" else head[1], layernorm=layernorm)
            extra = cfg["agent"] if clip is None else dict(cfg["agent"], grad_clip=clip)
            a = ContinuousAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=DEV), loss_cfg=loss_cfg, optimizer_cfg=opt,
                                device=DEV, **extra)
        if layernorm:
            TU.randomise_layernorms(a.nn, k)
        agents.append(a)
    return agents


def _rows(shape, K, n, seed):
    """[K, n, row] float32 on the GPU: obs | actions[A] | counts[A] | Q[A] | V."""
    S, A = shape[0], _actions(shape)
    rng = np.random.RandomState(seed)
    obs = rng.randn(K, n, S)
    if shape[2][0] == "discrete":
        actions, counts = np.tile(np.arange(A, dtype=np.float64), (K, n, 1)), rng.randint(0, 9, (K, n, A))
    else:
        actions, counts = rng.uniform(-1.9, 1.9, (K, n, A)), rng.randint(1, 9, (K, n, A))
    return torch.from_numpy(np.concatenate([obs, actions, counts, rng.randn(K, n, A), rng.randn(K, n, 1)], axis=-1).astype(np.float32)).to(DEV)


def _state(tr):
    names = ("flat", "square_avg", "exp_avg", "exp_avg_sq", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq", "last_grad_norms")
    torch.cuda.synchronize()
    out = {n: getattr(tr, n).detach().cpu().clone() for n in names if getattr(tr, n) is not None}
    out["steps"] = torch.tensor([tr.opt_step, tr.alpha_step])
    return out


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


def _add(total, infos):
    for s, info in zip(total, infos):
        for key, val in info.items():
            s[key] = s.get(key, 0.0) + val


class Pair:
    """A trainer with an average and its twin without one, on identical populations; every call is made on both -- in one native
    call on the first, one minibatch at a time on the twin -- and ``ema`` is held to the numpy rule over the twin's snapshots."""

    def __init__(self, shape, K, ema, loss, losses="device", agent_kw=None, **trainer_kw):
        self.shape, self.K, self.S, self.A = shape, K, shape[0], _actions(shape)
        self.tr = PopulationTrainer(_agents(shape, K, loss, **(agent_kw or {})), max_batch=64, losses=losses, ema=ema, **trainer_kw)
        self.twin = PopulationTrainer(_agents(shape, K, loss, **(agent_kw or {})), max_batch=64, losses=losses, **trainer_kw)
        assert self.twin.ema is None and self.twin.ema_updates == 0
        self.decay, self.every = PT._ema_settings(ema, K)
        assert (self.tr.ema_decay, self.tr.ema_every) == (self.decay, self.every)
        assert self.tr.ema.shape == self.tr.flat.shape and self.tr.ema.data_ptr() != self.tr.flat.data_ptr()
        assert torch.equal(self.tr.ema, self.tr.flat)
        self.want = self.tr.flat.cpu().numpy().copy()
        self.step, self.updates = 0, 0

    def restart(self, decay=None):
        """The native count starts again (a re-attach); the average goes on from where it stands."""
        self.step, self.updates = 0, 0
        if decay is not None:
            self.decay = decay
        torch.cuda.synchronize()
        self.want = self.tr.ema.cpu().numpy().copy()

    def hold(self, snapshots, got, want):
        self.want, made = E.ema_after(self.want, snapshots, self.decay, self.every, first_step=self.step + 1)
        self.step += len(snapshots)
        self.updates += made
        assert got == want and all(np.isfinite(v) for i in got for v in i.values())
        a, b = _state(self.tr), _state(self.twin)
        assert set(a) == set(b)
        for name in a:
            assert torch.equal(a[name], b[name]), f"the average disturbed {name}"
        np.testing.assert_array_equal(_bits(self.tr.ema), _bits(self.want))
        assert self.tr.trainer.ema_info() == (self.step, self.updates) and self.tr.ema_updates == self.updates

    def snap(self):
        torch.cuda.synchronize()
        return self.twin.flat.cpu().numpy().copy()

    def update(self, B, seed):
        batch = TU.split_rows(_rows(self.shape, self.K, B, seed), self.S, self.A)
        got, want = self.tr.update(batch), self.twin.update(batch)
        self.hold([self.snap()], got, want)

    def epoch(self, n, batch, seed):
        rows, seeds = _rows(self.shape, self.K, n, seed), list(range(seed, seed + self.K))
        got = self.tr.train_epoch(rows, self.S, self.A, batch_size=batch, shuffle_seeds=seeds)
        order = torch.from_numpy(np.stack([np.random.RandomState(s).permutation(n) for s in seeds])).to(DEV)
        net = torch.arange(self.K, device=DEV)[:, None]
        snaps, want = [], [{} for _ in range(self.K)]
        for i, j in minibatch_bounds(n, batch):
            _add(want, self.twin.update(TU.split_rows(rows[net, order[:, i:j]], self.S, self.A)))
            snaps.append(self.snap())
        self.hold(snaps, got, want)
        return len(snaps)

    def close(self):
        self.tr.close()
        self.twin.close()


def test_update_and_epochs_on_the_small_shape():
    """K = 3, P = 99, decays 0.9 / 0 / 0.999: ``update`` (the fused RMSprop step entry point), an epoch of 5 minibatches, and with
    ``every=3`` two epochs of 5 in a row (updates after steps 3, 6, 9 of the 10)."""
    p = Pair(SMALL, 3, DECAYS, "a0c")
    P = p.tr.flat.shape[1]
    assert P == 99 and P % 4 != 0 and (3 * P) % 4 != 0   # a scalar tail, and groups that straddle both net boundaries
    p.update(8, 1)
    assert p.epoch(40, 8, 2) == 5
    assert p.updates == 6 and not torch.equal(p.tr.ema, p.tr.flat)
    # decay 0 is ema + (p - ema): the parameters up to one rounding
    torch.cuda.synchronize()
    np.testing.assert_allclose(p.tr.ema[1].cpu().numpy(), p.tr.flat[1].cpu().numpy(), rtol=2.0 ** -23, atol=0)
    p.close()
    q = Pair(SMALL, 3, {"decay": DECAYS, "every": 3}, "a0c")
    assert q.epoch(40, 8, 3) == 5 and (q.step, q.updates) == (5, 1)
    assert q.epoch(40, 8, 4) == 5 and (q.step, q.updates) == (10, 3)
    q.close()


def test_update_with_torch_losses():
    """``losses="torch"``: the step ends in azg_trainer_backward_step, which the average follows too."""
    p = Pair(SMALL, 3, DECAYS, "a0c", losses="torch")
    p.update(8, 5)
    p.update(8, 6)
    assert p.updates == 2
    p.close()


def test_minibatches_of_17_rows_on_three_layers_of_128():
    p = Pair(GMM, 2, 0.99, "a0c_tuned")
    p.update(17, 7)
    assert p.epoch(34, 17, 8) == 2
    assert p.tr.alpha_step == 3 and p.updates == 3
    p.close()


@pytest.mark.parametrize("form", ["rmsprop", "agents_adam_clip", "per_net"])
def test_optimiser_forms(form):
    """The fused, the deferred and the table form of the backward launch."""
    kw = {"rmsprop": dict(),
          "agents_adam_clip": dict(optimizers="agents", agent_kw=dict(optimizer=TU.ADAM_WD, clip=0.05)),
          "per_net": dict(optimizers="agents", per_net=True, agent_kw=dict(optimizer=TU.RMSPROP_WD, lrs=[1e-3, 3e-4, 3e-3]))}[form]
    p = Pair(SMALL, 3, DECAYS, "a0c", **kw)
    assert p.epoch(16, 8, 9) == 2
    if form != "rmsprop":
        assert p.tr.opt_step == 2
    p.close()


@pytest.mark.parametrize("kind", ["layernorm", "wide", "wide_layernorm"])
def test_trainer_kinds(kind):
    """One epoch of 2 minibatches on each of the other three native trainers."""
    if kind == "wide":
        p = Pair(PENDULUM_WIDE, 2, [0.9, 0.5], "a0c", wide=True)
        assert p.tr.flat.shape[1] % 4 != 0
    else:
        p = Pair(SMALL, 3, DECAYS, "a0c", agent_kw=dict(layernorm=True), **{kind: True})
        assert p.tr.flat.shape[1] == 99 + 2 * 16
    assert p.epoch(16, 8, 10) == 2 and p.updates == 2
    p.close()


def _ring_sides(ema):
    """(trainer, self-play) twice over identical populations and rings of 5 stored steps: with the average, and without."""
    sides = []
    for kw in (dict(ema=ema), dict()):
        agents, sp = TF._tiny(PRIO)
        assert sp.play_device(5) == (5, 0)
        sides.append((PopulationTrainer(agents, max_batch=64, losses="device", **kw), sp))
    return sides


def _hold_ring(tr, twin, sp, sp2, start, snaps, decay, got, want):
    ema, made = E.ema_after(start, snaps, decay)
    assert got == want
    a, b = _state(tr), _state(twin)
    for name in a:
        assert torch.equal(a[name], b[name]), f"the average disturbed {name}"
    np.testing.assert_array_equal(_bits(sp.errors()), _bits(sp2.errors()))
    np.testing.assert_array_equal(_bits(tr.ema), _bits(ema))
    assert tr.ema_updates == made == len(snaps)


def test_ring_epoch_with_priority_weights_and_errors():
    """train_epoch_ring(weights="priority", errors=True): the errors form of the epoch, rows gathered from the self-play ring."""
    decay = [0.9, 0.5]
    (tr, sp), (twin, sp2) = _ring_sides(decay)
    start = tr.ema.cpu().numpy().copy()
    orders = [s.sample_order(16) for s in (sp, sp2)]
    np.testing.assert_array_equal(orders[0], orders[1])
    sp.is_weights()
    sp2.is_weights()
    got = tr.train_epoch_ring(sp, orders[0], batch_size=8, weights="priority", errors=True)
    snaps, want = [], [{} for _ in range(2)]
    for i, j in minibatch_bounds(16, 8):
        _add(want, twin.train_epoch_ring(sp2, orders[1][:, i:j], batch_size=8, weights="priority", errors=True))
        snaps.append(twin.flat.cpu().numpy().copy())
    _hold_ring(tr, twin, sp, sp2, start, snaps, decay, got, want)
    for x in (tr, twin, sp, sp2):
        x.close()


def test_online_ring_epoch():
    """train_online_ring: every minibatch redrawn inside one native call."""
    decay = [0.0, 0.99]
    (tr, sp), (twin, sp2) = _ring_sides(decay)
    start = tr.ema.cpu().numpy().copy()
    got = tr.train_online_ring(sp, 3, batch_size=8)
    snaps, want = [], [{} for _ in range(2)]
    for _ in range(3):
        _add(want, twin.train_online_ring(sp2, 1, batch_size=8))
        snaps.append(twin.flat.cpu().numpy().copy())
    _hold_ring(tr, twin, sp, sp2, start, snaps, decay, got, want)
    for x in (tr, twin, sp, sp2):
        x.close()


def test_a_net_that_does_not_move_keeps_its_average_equal():
    """Per-net learning rates with net 1's 0 (and no weight decay): its ``ema`` row stays bit-equal to its ``flat`` row, whatever
    its decay; the others' move away from theirs."""
    agents = _agents(SMALL, 3, "a0c", optimizer=run.RMSPROP, lrs=[1e-3, 0.0, 3e-3])
    tr = PopulationTrainer(agents, max_batch=64, losses="device", optimizers="agents", per_net=True, ema=[0.9, 0.7, 0.999])
    start = tr.flat.cpu().clone()
    tr.train_epoch(_rows(SMALL, 3, 24, 11), SMALL[0], 4, batch_size=8, shuffle_seeds=[0, 1, 2])
    torch.cuda.synchronize()
    assert tr.ema_updates == 3
    flat, ema = tr.flat.cpu(), tr.ema.cpu()
    assert torch.equal(flat[1], start[1]) and torch.equal(ema[1].view(torch.int32), flat[1].view(torch.int32))
    for k in (0, 2):
        assert not torch.equal(flat[k], start[k]) and not torch.equal(ema[k], flat[k]) and not torch.equal(ema[k], start[k])
    tr.close()


def test_detach_reattach_reset_and_close():
    p = Pair(SMALL, 3, DECAYS, "a0c")
    p.update(8, 12)
    before = p.tr.ema.cpu().clone()
    p.tr.set_ema(None)
    assert p.tr.ema_decay is None and p.tr.ema_updates == 0
    p.tr.update(TU.split_rows(_rows(SMALL, 3, 8, 13), p.S, p.A))
    p.twin.update(TU.split_rows(_rows(SMALL, 3, 8, 13), p.S, p.A))
    torch.cuda.synchronize()
    assert torch.equal(p.tr.ema.cpu(), before) and p.tr.trainer.ema_info() == (0, 0)   # detached: the old tensor is left alone
    with pytest.raises(ValueError, match="detached: give a decay"):
        p.tr.set_ema(every=2)
    with pytest.raises(ValueError, match=r"finite and in \[0, 1\)"):
        p.tr.set_ema(decay=1.0)
    p.tr.set_ema(decay=0.5, every=2)   # re-attached: the count starts again, the average goes on from where it stands
    p.every = 2
    p.restart(0.5)
    assert (p.tr.ema_decay, p.tr.ema_every) == (0.5, 2)
    p.update(8, 14)
    p.update(8, 15)
    assert (p.step, p.updates) == (2, 1)
    p.tr.reset_ema([2])
    torch.cuda.synchronize()
    assert torch.equal(p.tr.ema[2], p.tr.flat[2]) and not torch.equal(p.tr.ema[0], p.tr.flat[0])
    with pytest.raises(ValueError, match="nets must be in 0 .. 2"):
        p.tr.reset_ema([3])
    p.tr.reset_ema()
    assert torch.equal(p.tr.ema, p.tr.flat)
    for call in (p.twin.set_ema, p.twin.reset_ema):
        with pytest.raises(ValueError, match="needs a trainer built with ema="):
            call()
    kept = p.tr.ema.cpu().clone()
    p.close()
    assert p.tr.ema_decay is None and p.tr.ema_updates == 0 and torch.equal(p.tr.ema.cpu(), kept)


def test_native_refusals_leave_the_trainer_as_it_was():
    p = Pair(SMALL, 3, DECAYS, "a0c")
    p.update(8, 16)
    native, ptr = p.tr.trainer, p.tr.ema.data_ptr()
    invalid = -1
    for args, reason in (((0, 0.5, 1), "NULL pointer"), ((ptr, 1.0, 1), "finite and in [0, 1)"), ((ptr, -0.5, 1), "finite and in [0, 1)"),
                         ((ptr, float("nan"), 1), "finite and in [0, 1)"), ((ptr, float("inf"), 1), "finite and in [0, 1)"),
                         ((ptr, [0.5, 0.5], 1), "n_decay must be 1 or"), ((ptr, [0.5, 0.5, 0.5, 0.5], 1), "n_decay must be 1 or"),
                         ((ptr, [0.5, 0.5, 1.0], 1), "decay of net 2"), ((ptr, 0.5, 0), "every must be at least 1"),
                         ((ptr, 0.5, -3), "every must be at least 1")):
        with pytest.raises(_capi.EngineError) as err:
            native.set_ema(*args)
        assert err.value.code == invalid and reason in str(err.value), (args, str(err.value))
        assert native.ema_info() == (1, 1)
    cfg = _capi.AzgEmaCfg(4, 1, 1, 0, ptr, (_capi.C.c_double * 1)(0.5))
    assert native._f["trainer_set_ema"](native._h, _capi.C.byref(cfg)) == invalid
    assert native._f["trainer_set_ema"](None, None) == invalid and native._f["trainer_ema_info"](None, None, None) == invalid
    p.update(8, 17)   # the settings in force are still the constructor's
    assert native.ema_info() == (2, 2)
    p.close()


def test_a_clone_takes_the_average_and_its_pace():
    """copy_nets([0, 0, 2]): net 1's ``ema`` row and decay become net 0's; the next epoch's row follows net 0's decay."""
    p = Pair(SMALL, 3, [0.5, 0.9, 0.0], "a0c")
    assert p.epoch(16, 8, 18) == 2
    for tr in (p.tr, p.twin):
        tr.copy_nets([0, 0, 2])
    torch.cuda.synchronize()
    assert torch.equal(p.tr.ema[1], p.tr.ema[0]) and torch.equal(p.tr.flat[1], p.tr.flat[0])
    assert p.tr.ema_decay == [0.5, 0.5, 0.0] and p.tr.ema_decay[1] == p.tr.ema_decay[0]
    assert p.tr.ema_updates == 0   # (re-attached with the cloned decays)
    p.restart([0.5, 0.5, 0.0])
    assert p.epoch(16, 8, 19) == 2
    p.close()
    # one decay for all: the row is cloned, nothing is re-attached
    q = Pair(SMALL, 3, 0.9, "a0c")
    q.update(8, 20)
    for tr in (q.tr, q.twin):
        tr.copy_nets([2, 1, 2])
    torch.cuda.synchronize()
    assert torch.equal(q.tr.ema[0], q.tr.ema[2]) and q.tr.ema_decay == 0.9 and q.tr.ema_updates == 1
    q.want = q.tr.ema.cpu().numpy().copy()
    q.update(8, 21)
    q.close()
