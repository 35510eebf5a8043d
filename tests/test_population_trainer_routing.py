"""GPU: which native entry point every PopulationTrainer call reaches, and how the step counts move.  The arithmetic behind the entry
points is tested where they are (test_population_trainer*.py, test_weighted_loss.py, test_priority_feedback.py, test_online_replay.py);
here the trainer's ``azg_trainer_*`` symbols are wrapped in recorders that forward to the real functions, and every call of the table
below is made once on the smallest inputs that take its path: K = 2 nets with one hidden layer of width 16, minibatches of 4 rows,
epochs over 8 rows per net (two minibatches), a self-play ring as small as test_online_replay.py's smallest."""
import numpy as np
import pytest
import torch

import test_priority_feedback as TF
import trainer_util as TU
from alphazero_gym_amd import run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import DEV

pytestmark = pytest.mark.gpu

K, B, N_ROWS, N_MB = 2, 4, 8, 2   # N_ROWS rows per net in minibatches of B: N_MB optimiser steps per epoch
M_ONLINE = 3                      # minibatches of one train_online_ring call

# column: (PopulationTrainer keywords, the optimisers of the K agents, whether opt_step counts)
LRS = (1e-3, 3e-3)
COLUMNS = {
    "rmsprop": (dict(), [run.RMSPROP] * K, False),
    "agents": (dict(optimizers="agents"), [run.ADAM] * K, True),
    "per_net": (dict(optimizers="agents", per_net=True), [dict(run.RMSPROP, lr=lr) for lr in LRS], True),
}
# call: the symbols it reaches, per column
TABLE = {
    "update_torch": dict(rmsprop=["trainer_forward", "trainer_backward_step"], agents=["trainer_forward", "trainer_backward_step_opt"],
                         per_net=["trainer_forward", "trainer_backward_step_nets"]),
    "update": dict(rmsprop=["trainer_step"], agents=["trainer_step_opt"], per_net=["trainer_step_nets"]),
    "update_weighted": dict(rmsprop=["trainer_step_opt_weighted"], agents=["trainer_step_opt_weighted"],
                            per_net=["trainer_step_nets_weighted"]),
    "epoch": dict(rmsprop=["trainer_epoch"], agents=["trainer_epoch_opt"], per_net=["trainer_epoch_nets"]),
    "epoch_weighted": dict(rmsprop=["trainer_epoch_opt_weighted"], agents=["trainer_epoch_opt_weighted"],
                           per_net=["trainer_epoch_nets_weighted"]),
    "epoch_errors": dict(rmsprop=["trainer_epoch_opt_errors"], agents=["trainer_epoch_opt_errors"], per_net=["trainer_epoch_nets_errors"]),
    "online": dict(rmsprop=["trainer_epoch_online"], agents=["trainer_epoch_online"], per_net=["trainer_epoch_online_nets"]),
}


def _cartpole_agents(optimizers):
    """One agent per optimiser configuration, as run.make_agent builds it for CartPole (4 inputs, 2 actions) with one hidden layer of
    16 and AlphaZeroLoss: the shape of the rows of TF._tiny's ring and of TU.make_rows("discrete", ...)."""
    from alphazero_gym_amd.envs import make_game
    base = run._merge(run.DISCRETE_DEFAULTS, dict(device=DEV, policy=dict(hidden_dimensions=[16])))
    env = make_game(base["game"])
    agents = []
    for k, opt in enumerate(optimizers):
        torch.manual_seed(k)
        agents.append(run.make_agent("discrete", dict(base, loss=TU.LOSSES["alphazero"], optimizer=opt), env))
    return agents


class Recorded:
    """A PopulationTrainer whose native trainer's ``trainer_*`` symbols record their names before they forward.  ``made(call, ...)``
    runs ``call`` and holds the trainer to the symbols and step counts given."""

    def __init__(self, agents, counts_steps, **kw):
        self.tr = PopulationTrainer(agents, max_batch=16, **kw)
        self.calls = []
        self.counts_steps = counts_steps
        self.tuned = self.tr.log_alpha is not None and self.tr.losses == "device"
        native = self.tr.trainer
        native._f = {name: self._recorder(name, fn) if name.startswith("trainer_") else fn for name, fn in native._f.items()}

    def _recorder(self, name, fn):
        def forward(*args):
            self.calls.append(name)
            return fn(*args)
        return forward

    def made(self, call, symbols, steps):
        tr = self.tr
        opt_step, alpha_step = tr.opt_step, tr.alpha_step
        del self.calls[:]
        out = call()
        assert self.calls == symbols
        assert tr.opt_step == opt_step + (steps if self.counts_steps else 0)
        assert tr.alpha_step == alpha_step + (steps if self.tuned else 0)
        return out

    def close(self):
        del self.calls[:]
        self.tr.close()
        assert self.calls == ["trainer_destroy"]


def _finite(infos):
    assert len(infos) == K and all(np.isfinite(v) for info in infos for v in info.values())


def _updates_and_epochs(rec, column, head):
    """The ``update`` and ``train_epoch`` rows of the table on ``rec`` (``losses="device"``), rows as TU.make_rows(head) makes them."""
    tr = rec.tr
    S, A = TU.DIMS[head]
    rows = TU.make_rows(head, K, N_ROWS, seed=3)
    batch = TU.split_rows(rows[:, :B], S, A)
    ones_b, ones_n = torch.ones((K, B), device=DEV), torch.ones((K, N_ROWS), device=DEV)
    errors = torch.full((K, N_ROWS), -1.0, device=DEV)
    cell = {name: TABLE[name][column] for name in TABLE}
    _finite(rec.made(lambda: tr.update(batch), cell["update"], 1))
    del rec.calls[:]
    assert tr.last_d_raw.shape == (K, B, tr.trainer.n_raw) and rec.calls == ["trainer_read_d_raw"]
    _finite(rec.made(lambda: tr.update(batch, weights=ones_b), cell["update_weighted"], 1))
    epoch = lambda **kw: tr.train_epoch(rows, S, A, batch_size=B, shuffle_seeds=[5, 6], **kw)   # noqa: E731
    _finite(rec.made(epoch, cell["epoch"], N_MB))
    assert tr.last_d_raw is None   # (an epoch leaves nothing to read, and nothing was read)
    _finite(rec.made(lambda: epoch(weights=ones_n), cell["epoch_weighted"], N_MB))
    _finite(rec.made(lambda: epoch(errors=errors), cell["epoch_errors"], N_MB))
    assert (errors >= 0).all()
    _finite(rec.made(lambda: epoch(weights=ones_n, errors=errors), cell["epoch_errors"], N_MB))


@pytest.mark.parametrize("column", list(COLUMNS))
def test_updates_and_epochs(column):
    kw, optimizers, counts = COLUMNS[column]
    rec = Recorded(_cartpole_agents(optimizers), counts, losses="device", **kw)
    _updates_and_epochs(rec, column, "discrete")
    assert rec.tr.opt_step == (2 + 4 * N_MB if counts else 0) and rec.tr.alpha_step == 0
    rec.close()


def test_a_tuned_loss_counts_its_alpha_steps():
    """per_net=True with a Normal head and A0CLossTuned: ``alpha_step`` moves with ``opt_step``."""
    agents = [TU.make_agent("normal", "a0c_tuned", seed=k, hidden=(16,), optimizer=dict(run.RMSPROP, lr=lr), device=DEV)
              for k, lr in enumerate(LRS)]
    rec = Recorded(agents, True, losses="device", optimizers="agents", per_net=True)
    assert rec.tuned
    _updates_and_epochs(rec, "per_net", "gmm2")   # (its rows: 3 inputs, 4 continuous actions per row)
    assert rec.tr.opt_step == rec.tr.alpha_step == 2 + 4 * N_MB
    rec.close()


@pytest.mark.parametrize("column", list(COLUMNS))
def test_torch_losses(column):
    kw, optimizers, counts = COLUMNS[column]
    rec = Recorded(_cartpole_agents(optimizers), counts, losses="torch", **kw)
    S, A = TU.DIMS["discrete"]
    batch = TU.split_rows(TU.make_rows("discrete", K, B, seed=4), S, A)
    for weights in (None, torch.ones((K, B), device=DEV)):
        _finite(rec.made(lambda: rec.tr.update(batch, weights=weights), TABLE["update_torch"][column], 1))
        del rec.calls[:]
        assert rec.tr.last_d_raw.shape == (K, B, rec.tr.trainer.n_raw) and rec.calls == []   # (autograd's, not the native trainer's)
    rec.close()


@pytest.fixture(scope="module")
def ring():
    """TF._tiny's self-play object (K = 2 CartPole nets, 4 games each, a ring of 8 steps) after 3 steps: 12 stored rows per net."""
    _, sp = TF._tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4, "feedback": "max"})
    assert sp.play_device(3)[0] == 3
    yield sp
    sp.close()


@pytest.mark.parametrize("column", list(COLUMNS))
def test_ring_epochs_and_the_online_epoch(ring, column):
    kw, optimizers, counts = COLUMNS[column]
    rec = Recorded(_cartpole_agents(optimizers), counts, losses="device", **kw)
    tr = rec.tr
    order = np.tile(np.arange(N_ROWS), (K, 1))
    ring.priorities()
    ring.is_weights()
    epoch = lambda **kw: tr.train_epoch_ring(ring, order, batch_size=B, **kw)   # noqa: E731
    cell = {name: TABLE[name][column] for name in TABLE}
    _finite(rec.made(epoch, cell["epoch"], N_MB))
    _finite(rec.made(lambda: epoch(weights="priority"), cell["epoch_weighted"], N_MB))
    _finite(rec.made(lambda: epoch(errors=True), cell["epoch_errors"], N_MB))
    _finite(rec.made(lambda: epoch(weights="priority", errors=True), cell["epoch_errors"], N_MB))
    index = ring._sample_index
    _finite(rec.made(lambda: tr.train_online_ring(ring, M_ONLINE, batch_size=B), cell["online"], M_ONLINE))
    assert ring._sample_index == index + M_ONLINE
    assert tr.opt_step == (4 * N_MB + M_ONLINE if counts else 0) and tr.last_d_raw is None
    rec.close()
