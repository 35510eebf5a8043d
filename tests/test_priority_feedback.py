"""GPU: priorities fed back from the trainer's value errors (include/azgym_priority.h: azg_selfplay_keep_errors, _errors_device,
_error_values, _set_error_values, _priorities_trained; include/azgym_train_errors.h: the *_errors forms of the loss and the epoch;
PopulationSelfPlay(prioritized={..., "feedback"}), PopulationTrainer.train_epoch_ring(errors=True)).  Every comparison is bit for
bit: the rules are exact.  The truth: tests/priority_feedback_util.py; rings and sizes: tests/nstep_util.py; the trainer at the raw
ABI: tests/test_weighted_loss.py's Pop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import is_weights_util as W
import nstep_util as N
import priority_feedback_util as F
import priority_util as P
import reanalyse_util as R
import test_is_weights as TW
import test_weighted_loss as WL
import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from device_loss_util import HEADS, kernel_loss, make_inputs, make_loss, make_trainer
from trainer_util import DEV

pytestmark = pytest.mark.gpu

STATE, INVALID = _capi.AZG_E_STATE, _capi.AZG_E_INVALID
NAN, INF = np.float32("nan"), np.float32("inf")


def _engine(name, capacity, fifo, steps, errors=True, case=None, transitions=True):
    case, e = TW._engine(name, capacity, fifo, steps, transitions=transitions, case=case)
    if errors:
        e.selfplay_keep_errors(True)
    return case, e


def _err(e, case):
    return e.selfplay_error_values().reshape(-1, case.games)


def _q1(d, alpha, eps):
    return int(P.priorities(np.asarray([d], np.float32), alpha, eps)[0])


def _per_net(x, K):
    """[size, G, ...] -> [K, size * T, ...]: net k's row i is slot i // T, game k * T + i % T."""
    size, G = x.shape[:2]
    T = G // K
    x = x.reshape((size, K, T) + x.shape[2:])
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((K, size * T) + x.shape[3:])


# ------------------------------------------------------------------------------------------------ a. the loss launch's errors

def _kernel_loss_errors(tr, cfg, inputs, weights, state=None, nets=False):
    """azg_trainer_loss_errors (``nets``: _nets_errors); weights None: NULL.  (losses [K, 5], d_raw, errors [K, B]) on the CPU."""
    raw, actions, counts, values = (x.to(DEV).contiguous() for x in inputs)
    w = None if weights is None else weights.to(DEV).contiguous()
    d_raw = torch.full_like(raw, float("nan"))
    losses = torch.full((raw.shape[0], 5), float("nan"), device=DEV)
    errors = torch.full(values.shape, -7.0, device=DEV)
    torch.cuda.synchronize()
    fn = tr.loss_nets_errors if nets else tr.loss_errors
    fn(raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), None if w is None else w.data_ptr(), errors.data_ptr(),
       raw.shape[1], actions.shape[2], cfg, state, d_raw.data_ptr(), losses.data_ptr())
    return losses.cpu(), d_raw.cpu(), errors.cpu()


@pytest.mark.parametrize("nets", [False, True], ids=["opt", "nets"])
@pytest.mark.parametrize("loss_name", ["a0c", "a0c_tuned"])
@pytest.mark.parametrize("head", ["discrete3", "gmm2"])
def test_loss_errors(head, loss_name, nets):
    """K = 3, B in {17, 300} (300: the kernel's 256 threads take a second pass): errors are float32(|float64(raw[:, 0]) - float64(z)|);
    d_raw, losses and the alpha state are the weighted call's, and with NULL weights the unweighted call's."""
    K = 3
    policy, tr = make_trainer(head, K, 320)
    cfg = _capi.loss_cfg(policy, make_loss(loss_name, "mean", clip=0.5))
    cfgs = [cfg] * K if nets else cfg
    for B in (17, 300):
        inputs = make_inputs(head, K, B, 4100 + B)
        w = W.make_weights(K, B, 4200 + B)
        want_e = F.loss_errors(inputs[0][..., 0].numpy(), inputs[3].numpy())
        assert len(np.unique(want_e)) > B
        st, a_w = WL._alpha_state(loss_name, K)
        want = W.kernel_loss_weighted(tr, cfgs, inputs, w, st, nets=nets)
        st, a_e = WL._alpha_state(loss_name, K)
        got = _kernel_loss_errors(tr, cfgs, inputs, w, st, nets=nets)
        for x, y, name in zip(want, got, ("losses", "d_raw")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"B = {B}: {name} (weighted)"
        for x, y in zip(a_w, a_e):
            assert torch.equal(x, y), f"B = {B}: alpha state (weighted)"
        np.testing.assert_array_equal(F.bits(got[2].numpy()), F.bits(want_e), err_msg=f"B = {B}")
        st, a_p = WL._alpha_state(loss_name, K)
        plain = kernel_loss(tr, cfg, inputs, st)
        st, a_n = WL._alpha_state(loss_name, K)
        got = _kernel_loss_errors(tr, cfgs, inputs, None, st, nets=nets)
        for x, y, name in zip(plain, got, ("losses", "d_raw")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"B = {B}: {name} (NULL weights)"
        for x, y in zip(a_p, a_n):
            assert torch.equal(x, y), f"B = {B}: alpha state (NULL weights)"
        np.testing.assert_array_equal(F.bits(got[2].numpy()), F.bits(want_e), err_msg=f"B = {B} (NULL weights)")
        assert not torch.equal(plain[1], want[1])                                 # (the weights matter)
    tr.close()


# ------------------------------------------------------------------------------------------------ b, c. the epoch

class EPop(WL.Pop):
    def epoch_errors(self, where, weights, errors_ptr, order, batch, nets=False):
        sums = torch.full((self.K, 5), float("nan"), dtype=torch.float64, device=DEV)
        cfg = self.cfgs if nets else self.cfgs[0]
        opt = [self.optim(k, 0) for k in range(self.K)] if nets else self.optim(0, 0)
        torch.cuda.synchronize()
        fn = self.tr.epoch_nets_errors if nets else self.tr.epoch_opt_errors
        n = fn(self.params.data_ptr(), where, None if weights is None else weights.data_ptr(), errors_ptr, order, batch, cfg,
               self.alpha(0), opt, sums.data_ptr())
        return sums.cpu(), n


def _order_with_every_case(K, size, T, batch, seed):
    """[K, 2 * batch + 3]: per net a row of every slot, a row twice in the first minibatch, a row in both minibatches, and a row that
    is never drawn (returned)."""
    n, n_order = size * T, 2 * batch + 3
    rng = np.random.RandomState(seed)
    order, never = np.zeros((K, n_order), np.int32), []
    for k in range(K):
        cover = [s * T + (s + k) % T for s in range(size)]
        never.append(next(r for r in range(n) if r not in cover))
        pool = [r for r in range(n) if r != never[k]]
        fill = rng.choice(pool, n_order - size)
        fill[1] = fill[0]                                                         # twice in the first minibatch
        fill[batch + 2] = fill[2]                                                 # in both minibatches
        order[k] = np.concatenate([fill, cover])
        assert batch + 2 < n_order - size and never[k] not in order[k]
        assert set(order[k] // T) == set(range(size))
    return order, never


def _loop_with_errors(pop, pieces, w_net, order, batch, n, nets):
    """The epoch's minibatches one by one through the weighted step; the errors from each step's raw_out, the later minibatch winning."""
    obs, actions, counts, values = pieces
    K, n_order = order.shape
    sums = torch.zeros((K, 5), dtype=torch.float64)
    want = np.full((K, n), F.UNSEEN, np.float32)
    idx = torch.from_numpy(order.astype(np.int64))
    net = torch.arange(K)[:, None]
    i, m = 0, 0
    while i < n_order:
        j = n_order if i + 2 * batch > n_order else i + batch
        pick = idx[:, i:j]
        losses, raw = pop.step(obs[net, pick], actions[net, pick], counts[net, pick], values[net, pick], w_net[net, pick], m, nets=nets)
        e = F.loss_errors(raw[..., 0].numpy(), values[net, pick].numpy())
        for k in range(K):
            want[k, pick[k].numpy()] = e[k]
        sums = sums + losses.double()
        i, m = j, m + 1
    return sums, m, want


def _pieces(rows_net, S, A):
    t = torch.from_numpy(rows_net)
    return t[..., :S].contiguous(), t[..., S:S + A].contiguous(), t[..., S + A:S + 2 * A].contiguous(), t[..., -1].contiguous()


@pytest.fixture(scope="module")
def rings():
    made = {}

    def get(name):
        if name not in made:
            capacity, fifo = (16, True) if name == "cartpole" else (N.STEPS[name] + 1, False)
            made[name] = _engine(name, capacity, fifo, N.STEPS[name])
        case, e = made[name]
        e.selfplay_set_error_values(np.full(e.selfplay_ring()[0] * case.games, F.UNSEEN, np.float32))
        return case, e
    yield get
    for _, e in made.values():
        e.close()


@pytest.mark.parametrize("nets", [False, True], ids=["opt", "nets"])
@pytest.mark.parametrize("layout", ["plain", "ring"])
@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_epoch_errors_over_the_ring(rings, name, layout, nets):
    """The wrapped CartPole FIFO ring (33 games, capacity 16, 24 steps) and the 3-net population's ring, read where they lie
    (``ring``: the engine's rows and its kept errors) or as a copy per net (``plain``: [K][n] rows and errors).  Errors, parameters,
    optimiser state, alpha state and loss sums are those of the loop of weighted steps; undrawn entries stay -1; nothing else of the
    ring moves."""
    case, e = rings(name)
    K, T, G = case.nets, case.T, case.games
    size = e.selfplay_ring()[0]
    n, batch = size * T, 16
    S, A = 4, 2
    ring = R.ring(e, case)
    assert ring.shape == (size, G, S + 3 * A + 1)
    rows_net = _per_net(ring, K)
    rng = np.random.RandomState(5)
    w_ring = (1.0 - 0.9 * rng.rand(e._sp_cap, G)).astype(np.float32)
    w_net = torch.from_numpy(_per_net(w_ring[:size], K))
    order, never = _order_with_every_case(K, size, T, batch, 80)
    policy = TU.policy(S, [32, 16], ("discrete", A), "relu", 3)
    losses, lrs = WL._per_net_settings(K) if nets else (None, None)
    ep, loop, wt = (EPop(policy, "discrete2", K, 64, losses=losses, lrs=lrs) for _ in range(3))
    want_sums, m, want_err = _loop_with_errors(loop, _pieces(rows_net, S, A), w_net, order, batch, n, nets)
    if layout == "plain":
        rows_dev = torch.from_numpy(rows_net).to(DEV).contiguous()
        where = _capi.epoch_rows(rows_dev.data_ptr(), S, A, n)
        w_dev = w_net.to(DEV).contiguous()
        err_dev = torch.full((K, n), -1.0, device=DEV)
        got_sums, n_mb = ep.epoch_errors(where, w_dev, err_dev.data_ptr(), order, batch, nets=nets)
        got_err = err_dev.cpu().numpy()
    else:
        before = TW._books(e, case)
        ptr, _, row_len = e.selfplay_rows_device()
        where = _capi.epoch_rows(ptr, S, A, n, ring_trees=G, games_per_net=T)
        w_dev = torch.from_numpy(w_ring).to(DEV).contiguous()
        e.sync()
        got_sums, n_mb = ep.epoch_errors(where, w_dev, e.selfplay_errors_device(), order, batch, nets=nets)
        got_err = _per_net(_err(e, case), K)
        TW._assert_books(e, case, before, f"{name} ring")
    assert n_mb == m == 2
    assert torch.equal(got_sums.view(torch.int64), want_sums.view(torch.int64))
    WL._same(ep.state(), loop.state(), f"{name} {layout}")
    np.testing.assert_array_equal(F.bits(got_err), F.bits(want_err))
    for k in range(K):
        drawn = np.zeros(n, bool)
        drawn[order[k]] = True
        assert (got_err[k][~drawn] == F.UNSEEN).all() and not drawn[never[k]] and (got_err[k][drawn] >= 0).all()
        assert len(np.unique(got_err[k][drawn])) > batch
    # ... and everything but the errors is the weighted epoch's
    wt_sums, _ = wt.epoch(where, w_dev, order, batch, nets=nets)
    assert torch.equal(wt_sums.view(torch.int64), got_sums.view(torch.int64))
    WL._same(ep.state(), wt.state(), f"{name} {layout}: weighted epoch")
    for p in (ep, loop, wt):
        p.close()


@pytest.mark.parametrize("kind,hidden", [("layernorm", [32, 16]), ("wide", [512]), ("wide_layernorm", [512])])
def test_epoch_errors_on_the_other_handles(kind, hidden):
    """LayerNorm, wide and wide LayerNorm handles: one epoch of two minibatches over plain rows against the weighted epoch (state and
    loss sums) and the loop of weighted steps (the errors); with NULL weights against the plain epoch."""
    head, K, n, batch = "normal", 2, 41, 16
    A = HEADS[head][2]
    policy = TU.policy(WL.IN_DIM, hidden, ("normal",), "elu", 5, layernorm=TU.has_layernorm(kind))
    rows, pieces = WL._plain_rows(head, K, n, 930)
    where = _capi.epoch_rows(rows.data_ptr(), WL.IN_DIM, A, n)
    w_net = W.make_weights(K, n, 931)
    rng = np.random.RandomState(81)
    order = np.stack([rng.choice(np.arange(1, n), 2 * batch + 3) for _ in range(K)]).astype(np.int32)   # (row 0 is never drawn)
    order[:, 1], order[:, batch + 2] = order[:, 0], order[:, 2]                   # twice in one minibatch; in both minibatches
    ep, loop, wt, ep0, plain = (EPop(policy, head, K, 64, kind=kind) for _ in range(5))
    want_sums, m, want_err = _loop_with_errors(loop, pieces, w_net, order, batch, n, False)
    err = torch.full((K, n), -1.0, device=DEV)
    got_sums, n_mb = ep.epoch_errors(where, w_net.to(DEV), err.data_ptr(), order, batch)
    assert n_mb == m
    np.testing.assert_array_equal(F.bits(err.cpu().numpy()), F.bits(want_err))
    assert (want_err == F.UNSEEN).any() and (want_err >= 0).any()
    wt_sums, _ = wt.epoch(where, w_net.to(DEV), order, batch)
    assert torch.equal(got_sums.view(torch.int64), wt_sums.view(torch.int64)) and torch.equal(got_sums.view(torch.int64), want_sums.view(torch.int64))
    WL._same(ep.state(), wt.state(), f"{kind}: weighted epoch")
    WL._same(ep.state(), loop.state(), f"{kind}: loop")
    err0 = torch.full((K, n), -1.0, device=DEV)
    got0, _ = ep0.epoch_errors(where, None, err0.data_ptr(), order, batch)
    want0, _ = plain.epoch(where, None, order, batch)
    assert torch.equal(got0.view(torch.int64), want0.view(torch.int64))
    WL._same(ep0.state(), plain.state(), f"{kind}: NULL weights")
    assert ((err0.cpu().numpy() == F.UNSEEN) == (want_err == F.UNSEEN)).all()
    for p in (ep, loop, wt, ep0, plain):
        p.close()


# ------------------------------------------------------------------------------------------------ d. the step's reset

def test_a_step_resets_its_slot_and_nothing_else():
    """The wrapped FIFO ring with planted errors: one more step sets the overwritten slot's block to -1 and leaves every other entry's
    bits.  The same run without kept errors leaves the same ring, transitions, games and books."""
    name = "cartpole"
    case, e = _engine(name, 16, True, N.STEPS[name])
    G = case.games
    size, insert, _ = e.selfplay_ring()
    assert size == 16 and insert == N.STEPS[name] % 16
    np.testing.assert_array_equal(F.bits(_err(e, case)), np.full((size, G), F.UNSEEN_BITS, np.uint32))
    rng = np.random.default_rng(2)
    planted = rng.uniform(0.0, 3.0, (size, G)).astype(np.float32)
    planted[3, 5], planted[insert, 0], planted[15, G - 1] = NAN, INF, 0.0
    e.selfplay_set_error_values(planted)
    np.testing.assert_array_equal(F.bits(_err(e, case)), F.bits(planted))
    e.selfplay_step()
    want = planted.copy()
    want[insert] = F.UNSEEN
    np.testing.assert_array_equal(F.bits(_err(e, case)), F.bits(want))
    # a clear, an n-step call leave the errors; the rows stored after the clear are reset by their steps
    e.selfplay_nstep_targets(3)
    np.testing.assert_array_equal(F.bits(_err(e, case)), F.bits(want))
    e.selfplay_clear()
    e.selfplay_step()
    got = _err(e, case)
    assert got.shape == (1, G) and (got == F.UNSEEN).all()
    _, plain = _engine(name, 16, True, N.STEPS[name] + 1, errors=False)
    _, kept = _engine(name, 16, True, N.STEPS[name] + 1)
    for x in (plain, kept):
        x.selfplay_priorities(0.6, P.EPS)
    TW._assert_books(kept, case, TW._books(plain, case), "errors kept against not kept")
    for x in (e, plain, kept):
        x.close()


# ------------------------------------------------------------------------------------------------ e. priorities_trained

def _plant(case, size, seed):
    """Errors with every kind of entry.  A population: net 0 mixed, net 1 entirely unseen, net 2 with exactly one seen row."""
    rng = np.random.default_rng(seed)
    G, T = case.games, case.T
    err = (10.0 ** rng.uniform(-3.0, 1.0, (size, G))).astype(np.float32)
    err[rng.random((size, G)) < 0.4] = F.UNSEEN
    err[0, 0], err[0, 1], err[1, 0], err[1, 1], err[2, 0], err[2, 1] = 0.0, 1e-30, 1e30, INF, NAN, F.UNSEEN
    err[size - 1, T - 1] = 7.5
    if case.nets > 1:
        err[:, T:] = F.UNSEEN
        err[size // 2, 2 * T + 3] = 0.125
    return err


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_priorities_trained_are_the_rule(name):
    """All three unseen modes, alpha in {0, 0.6, 1}: q is the numpy rule's, bit for bit, on 0, tiny, huge, +inf, NaN and the sentinel;
    then the row draws and the weights on that q are the existing numpy helpers'."""
    case, e = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name])
    e.selfplay_nstep_targets(3)
    size, G, K = e.selfplay_ring()[0], case.games, case.nets
    err = _plant(case, size, 21)
    e.selfplay_set_error_values(err)
    tr = e.selfplay_transitions()
    gap = P.gap(tr["value"].reshape(size, G), R.ring(e, case)[..., -1])
    before = TW._books(e, case)
    seen = set()
    for alpha in P.ALPHAS:
        for unseen, mode, d in (("max", F.MAX, 0.0), ("value_gap", F.VALUE_GAP, 0.0), (0.75, F.CONSTANT, 0.75), (0.0, F.CONSTANT, 0.0)):
            e.selfplay_priorities_trained(alpha, P.EPS, unseen)
            q = TW._q(e, case)
            want = F.trained_priorities(err, K, alpha, P.EPS, mode, d, gap)
            np.testing.assert_array_equal(q, want, err_msg=f"{name} alpha {alpha} unseen {unseen}")
            seen.add(q.tobytes())
            if alpha:
                assert int(q[1, 1]) == P.Q_MAX and int(q[2, 0]) == 1             # +inf and NaN
    assert len(seen) >= 6
    np.testing.assert_array_equal(F.bits(_err(e, case)), F.bits(err))            # (the call reads the errors)
    # under max: the all-unseen net has d = 1, the one-seen net takes that row's error everywhere
    e.selfplay_priorities_trained(0.6, P.EPS, "max")
    q = TW._q(e, case)
    if K > 1:
        T = case.T
        assert (q[:, T:2 * T] == _q1(1.0, 0.6, P.EPS)).all()
        assert (q[:, 2 * T:] == _q1(0.125, 0.6, P.EPS)).all()
    order = e.selfplay_sample_rows(40, 3)
    np.testing.assert_array_equal(order, P.sample_rows(q, K, case.kw["seed"], case.kw.get("tree_id_base", 0), 3, 40))
    e.selfplay_is_weights(0.4)
    np.testing.assert_array_equal(W.bits(TW._w(e, case)), W.bits(W.is_weights(q, K, 0.4)))
    now = TW._books(e, case)
    np.testing.assert_array_equal(now["ring"], before["ring"])
    assert now["books"] == before["books"]
    e.close()


# ------------------------------------------------------------------------------------------------ f. more segments than lanes

@pytest.mark.parametrize("nets", [1, 3])
def test_the_maximum_over_more_segments_than_a_wave_has_lanes(nets):
    """4101 CartPole games x 13 steps: 209 segments for one net (a partial last one), 70 for each of three.  The largest seen error of
    net 0 is the last row of its partial last segment; the other nets' sit elsewhere and differ."""
    base = R.CASES["cartpole"]
    case = R.Case(dict(base.kw, n_sims=2), base.net, games=4101, max_len=3, nets=nets)
    steps = 13
    _, e = _engine("", steps, False, steps, transitions=False, case=case)
    T = case.T
    assert (steps * T) % 256 != 0 and steps * T > 64 * 256
    rng = np.random.default_rng(9)
    err = (10.0 ** rng.uniform(-3.0, 1.0, (steps, case.games))).astype(np.float32)
    err[rng.random(err.shape) < 0.5] = F.UNSEEN
    spots = [(steps - 1, T - 1), (0, 0), (5, T // 2)][:nets]
    for k, (s, j) in enumerate(spots):
        err[s, k * T + j] = 50.0 + 10.0 * k
    e.selfplay_set_error_values(err)
    e.selfplay_priorities_trained(1.0, 1e-3, "max")
    q = TW._q(e, case)
    np.testing.assert_array_equal(q, F.trained_priorities(err, nets, 1.0, 1e-3, F.MAX))
    for k, (s, j) in enumerate(spots):
        block, miss = q[:, k * T:(k + 1) * T], err[:, k * T:(k + 1) * T] == F.UNSEEN
        assert miss.sum() > 1000 and (block[miss] == block[s, j]).all() and (block[~miss] < block[s, j]).sum() == (~miss).sum() - 1
    assert len({int(q[s, k * T + j]) for k, (s, j) in enumerate(spots)}) == nets
    e.close()


# ------------------------------------------------------------------------------------------------ g. rank invariance

def test_a_nets_trained_priorities_are_those_of_a_one_net_engine_at_its_rank():
    name = "population"
    case, e = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name])
    size, T, K = e.selfplay_ring()[0], case.T, case.nets
    rng = np.random.default_rng(13)
    err = (10.0 ** rng.uniform(-2.0, 1.0, (size, case.games))).astype(np.float32)
    err[rng.random(err.shape) < 0.5] = F.UNSEEN
    for k in range(K):
        err[(3 * k + 1) % size, k * T + (5 * k) % T] = 20.0 + k                  # every net's own maximum
    e.selfplay_set_error_values(err)
    e.selfplay_priorities_trained(0.6, P.EPS, "max")
    q = TW._q(e, case).copy()
    e.close()
    np.testing.assert_array_equal(q, F.trained_priorities(err, K, 0.6, P.EPS, F.MAX))
    assert (q != F.trained_priorities(err, 1, 0.6, P.EPS, F.MAX)).any()           # (one maximum for the whole ring is another answer)
    for k in range(K):
        one = R.Case(case.net_kw(k), case.net, games=T, max_len=case.max_len)
        one._blob = lambda j, new, k=k: case.blob(k, new)
        _, o = _engine(name, N.STEPS[name] + 1, False, N.STEPS[name], case=one)
        o.selfplay_set_error_values(np.ascontiguousarray(err[:, k * T:(k + 1) * T]))
        o.selfplay_priorities_trained(0.6, P.EPS, "max")
        np.testing.assert_array_equal(TW._q(o, one), q[:, k * T:(k + 1) * T], err_msg=f"net {k}")
        o.close()


# ------------------------------------------------------------------------------------------------ h. refusals

def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    assert str(ei.value).split(": ", 1)[1]
    return ei.value.code


def _raw_trained(e, **kw):
    c = _capi.AzgTrainedPriorityConfig()
    c.struct_size, c.unseen, c.alpha, c.eps, c.unseen_d = C.sizeof(c), _capi.UNSEEN_MAX, 0.6, 1e-3, 0.0
    for k, v in kw.items():
        setattr(c, k, v)
    return e._f["selfplay_priorities_trained"](e._h, C.byref(c))


@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_engine_refusals_leave_q_and_the_errors_alone(name):
    case = N.CASES[name]
    G = case.games
    e = R.make_engine(TW._hip(), case)
    calls = ((e.selfplay_errors_device, ()), (e.selfplay_error_values, ()), (e.selfplay_set_error_values, (np.zeros(G, np.float32),)),
             (e.selfplay_priorities_trained, (0.6, 1e-3)))
    for fn, args in calls + ((e.selfplay_keep_errors, ()),):
        assert _code(fn, *args) == STATE                                          # no begin
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    for fn, args in calls + ((e.selfplay_keep_errors, ()),):
        assert _code(fn, *args) == STATE                                          # no keep_priorities
    e.selfplay_keep_errors(False)                                                 # (switching off what is off is no error)
    e.selfplay_keep_priorities(True)
    for fn, args in calls:
        assert _code(fn, *args) == STATE                                          # no keep_errors
    e.selfplay_keep_errors(True)                                                  # at a ring of two steps
    ptr = e.selfplay_errors_device()
    assert ptr != 0 and (e.selfplay_error_values() == F.UNSEEN).all() and e.selfplay_error_values().shape == (2 * G,)
    err = np.linspace(0.0, 2.0, 2 * G).astype(np.float32)
    err[1::3] = F.UNSEEN
    e.selfplay_set_error_values(err)
    e.selfplay_priorities_trained(0.6, 1e-3, "max")
    q = e.selfplay_priority_values().copy()
    np.testing.assert_array_equal(q.reshape(2, G), F.trained_priorities(err.reshape(2, G), case.nets, 0.6, 1e-3, F.MAX))
    # uploads
    assert _code(e.selfplay_set_error_values, err[:-1]) == INVALID
    assert _code(e.selfplay_set_error_values, np.concatenate([err, err[:1]])) == INVALID
    for bad in (-0.5, -INF, -2.0, np.float32(-1.0000001)):
        x = err.copy()
        x[G + 1] = bad
        assert _code(e.selfplay_set_error_values, x) == INVALID, bad
    assert e._f["selfplay_set_error_values"](e._h, None, 2 * G) == INVALID
    assert e._f["selfplay_errors_device"](e._h, None) == INVALID
    # priorities_trained
    assert e._f["selfplay_priorities_trained"](e._h, None) == INVALID
    assert _raw_trained(e, struct_size=16) == INVALID
    for unseen in (-1, 3, 99):
        assert _raw_trained(e, unseen=unseen) == INVALID
    assert _raw_trained(e, unseen=_capi.UNSEEN_VALUE_GAP) == STATE                # no keep_transitions
    assert _code(e.selfplay_priorities_trained, 0.6, 1e-3, "value_gap") == STATE
    for alpha in (-0.1, float("nan"), float("inf")):
        assert _raw_trained(e, alpha=alpha) == INVALID
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        assert _raw_trained(e, eps=eps) == INVALID
    for d in (-1.0, -1e-9, float("nan"), float("inf")):
        assert _raw_trained(e, unseen=_capi.UNSEEN_CONSTANT, unseen_d=d) == INVALID
    assert _raw_trained(e, unseen_d=float("nan")) == _capi.AZG_OK                 # (not read under max)
    with pytest.raises(ValueError, match="feedback"):
        e.selfplay_priorities_trained(0.6, 1e-3, "mean")
    # the existing entry point knows its two sources only
    c = _capi.AzgPriorityConfig()
    c.struct_size, c.source, c.alpha, c.eps = C.sizeof(c), 2, 0.6, 1e-3
    assert e._f["selfplay_priorities"](e._h, C.byref(c)) == INVALID
    np.testing.assert_array_equal(e.selfplay_priority_values(), q)
    np.testing.assert_array_equal(F.bits(e.selfplay_error_values()), F.bits(err))
    e.selfplay_sample_rows(4, 0)                                                  # (the trained priorities count as computed)
    # how long the pointer stays valid
    e.selfplay_keep_errors(False)
    for fn, args in calls:
        assert _code(fn, *args) == STATE
    e.selfplay_keep_errors(True)
    assert e.selfplay_errors_device() == ptr and (e.selfplay_error_values() == F.UNSEEN).all()   # (the same array, refilled)
    e.selfplay_set_error_values(err)
    e.selfplay_keep_priorities(False)                                             # switches the errors off too
    for fn, args in calls + ((e.selfplay_keep_errors, ()),):
        assert _code(fn, *args) == STATE
    e.selfplay_keep_priorities(True)
    for fn, args in calls:
        assert _code(fn, *args) == STATE
    e.selfplay_keep_errors(True)
    assert e.selfplay_errors_device() == ptr and (e.selfplay_error_values() == F.UNSEEN).all()
    assert _code(e.selfplay_sample_rows, 4, 0) == STATE                           # (gen was dropped with the priorities)
    R.begin(e, case, 4, keep=False)                                               # the next begin frees them
    e.selfplay_step()
    for fn, args in calls + ((e.selfplay_keep_errors, ()),):
        assert _code(fn, *args) == STATE
    e.selfplay_keep_priorities(True)
    e.selfplay_keep_errors(True)
    assert (e.selfplay_error_values() == F.UNSEEN).all() and e.selfplay_error_values().shape == (G,)
    e.selfplay_priorities_trained(0.6, 1e-3, "max")
    assert (e.selfplay_priority_values() == _q1(1.0, 0.6, 1e-3)).all()
    e.close()


def test_trainer_refusals_write_nothing():
    """NULL errors: AZG_E_INVALID from all four entry points, the namesake's refusals keep their codes, and nothing is written."""
    head, K, B, n = "gmm2", 2, 16, 24
    pop = EPop(WL.make_head(head), head, K, 32)
    tr, A = pop.tr, pop.A
    raw_in, actions, counts, values = (x.to(DEV).contiguous() for x in make_inputs(head, K, B, 41))
    w = torch.ones((K, B), device=DEV)
    d_raw = torch.full_like(raw_in, float("nan"))
    losses = torch.full((K, 5), float("nan"), device=DEV)
    sums = torch.full((K, 5), float("nan"), dtype=torch.float64, device=DEV)
    err_b, err_n = torch.full((K, B), float("nan"), device=DEV), torch.full((K, n), float("nan"), device=DEV)
    rows, _ = WL._plain_rows(head, K, n, 42)
    where = _capi.epoch_rows(rows.data_ptr(), WL.IN_DIM, A, n)
    w_rows = torch.ones((K, n), device=DEV)
    order = np.stack([np.random.RandomState(k).permutation(n) for k in range(K)]).astype(np.int32)
    before = pop.state()
    cfg, cfgs, st = pop.cfgs[0], pop.cfgs, pop.alpha(0)
    opt, opts = pop.optim(0, 0), [pop.optim(k, 0) for k in range(K)]
    Pp, AC, CN, V, Rw, D, L, S = (t.data_ptr() for t in (pop.params, actions, counts, values, raw_in, d_raw, losses, sums))
    torch.cuda.synchronize()

    def edit(obj, **kw):
        c = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    for wp in (w.data_ptr(), None):
        assert _code(tr.loss_errors, Rw, AC, CN, V, wp, None, B, A, cfg, st, D, L) == INVALID
        assert _code(tr.loss_nets_errors, Rw, AC, CN, V, wp, None, B, A, cfgs, st, D, L) == INVALID
    for wp in (w_rows.data_ptr(), None):
        assert _code(tr.epoch_opt_errors, Pp, where, wp, None, order, 8, cfg, st, opt, S) == INVALID
        assert _code(tr.epoch_nets_errors, Pp, where, wp, None, order, 8, cfgs, st, opts, S) == INVALID
    E, En = err_b.data_ptr(), err_n.data_ptr()
    assert _code(tr.loss_errors, Rw, AC, CN, V, None, E, 0, A, cfg, st, D, L) == INVALID
    assert _code(tr.loss_errors, Rw, AC, CN, V, None, E, 33, A, cfg, st, D, L) == INVALID
    assert _code(tr.loss_errors, Rw, AC, CN, V, None, E, B, A, edit(cfg, struct_size=8), st, D, L) == INVALID
    assert _code(tr.loss_errors, Rw, AC, CN, V, None, E, B, A, edit(cfg, kind=7), st, D, L) == _capi.AZG_E_UNSUPPORTED
    assert _code(tr.epoch_opt_errors, Pp, where, None, En, order, 0, cfg, st, opt, S) == INVALID
    assert _code(tr.epoch_opt_errors, Pp, edit(where, struct_size=8), None, En, order, 8, cfg, st, opt, S) == INVALID
    assert _code(tr.epoch_opt_errors, Pp, where, None, En, np.tile(order, (1, 2)), 64, cfg, st, opt, S) == INVALID
    bad = order.copy()
    bad[1, 3] = n
    assert _code(tr.epoch_opt_errors, Pp, where, None, En, bad, 8, cfg, st, opt, S) == INVALID
    torch.cuda.synchronize()
    for t in (d_raw, losses, sums, err_b, err_n):
        assert bool(torch.isnan(t).all())
    WL._same(pop.state(), before, "after refusals")
    assert tr.epoch_opt_errors(Pp, where, None, En, order, 8, cfg, st, opt, S) == 3   # the trainer is still usable
    assert torch.isfinite(sums).all() and bool((err_n >= 0).all())
    pop.close()


# ------------------------------------------------------------------------------------------------ i. end to end

def _tiny(prioritized):
    K, T = 2, 4
    agents = TU.make_agents("discrete", "a0c_tuned", K)
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, epsilon=0.1,
                                capacity_steps=8, n_step=3, prioritized=prioritized)
    return agents, sp


def test_the_closed_loop_in_python():
    """play, priorities, sample_order, is_weights, train_epoch_ring(weights="priority", errors=True), priorities, sample_order: the
    second draw is numpy's from the downloaded errors.  Without "feedback" the calls are what they were and errors=True is refused."""
    K, T, steps, batch, n_order = 2, 4, 5, 8, 12
    G = K * T
    agents, sp = _tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4, "feedback": "max"})
    assert sp.play_device(steps) == (steps, 0)
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    assert (sp.errors() == F.UNSEEN).all() and sp.errors().shape == (steps * G,)
    sp.priorities()
    one = _q1(1.0, 0.6, 1e-3)
    assert (sp.engine.selfplay_priority_values() == one).all()                    # nothing trained on yet: every row d = 1
    order = sp.sample_order(n_order)
    np.testing.assert_array_equal(order, P.sample_rows(np.full((steps, G), one, np.uint64), K, 34, 0, 0, n_order))
    sp.is_weights()
    info = tr.train_epoch_ring(sp, order, batch_size=batch, weights="priority", errors=True)
    assert len(info) == K and all(np.isfinite(v) for i in info for v in i.values())
    err = sp.errors().reshape(steps, G)
    per_net = _per_net(err, K)
    for k in range(K):
        drawn = np.zeros(steps * T, bool)
        drawn[order[k]] = True
        assert (per_net[k][drawn] >= 0).all() and (per_net[k][~drawn] == F.UNSEEN).all() and (~drawn).any()
    sp.priorities()
    q = sp.engine.selfplay_priority_values().reshape(steps, G)
    want_q = F.trained_priorities(err, K, 0.6, 1e-3, F.MAX)
    np.testing.assert_array_equal(q, want_q)
    assert len(np.unique(q)) > K
    order2 = sp.sample_order(n_order)
    np.testing.assert_array_equal(order2, P.sample_rows(want_q, K, 34, 0, 1, n_order))
    # given errors still go through the existing entry point; set_errors uploads
    sp.priorities(np.full(steps * G, 0.5, np.float32))
    assert (sp.engine.selfplay_priority_values() == _q1(0.5, 0.6, 1e-3)).all()
    sp.set_errors(np.full(steps * G, 0.25, np.float32))
    sp.priorities()
    assert (sp.engine.selfplay_priority_values() == _q1(0.25, 0.6, 1e-3)).all()
    # a plain rows array takes an errors tensor
    rows = torch.stack(sp._split(torch.from_numpy(sp.engine.selfplay_rows(clear=False)).to(DEV), steps))
    errs = torch.full((K, steps * T), -1.0, device=DEV)
    tr.train_epoch(rows, sp.engine.s_obs, sp.engine.kmax, batch_size=batch, errors=errs)
    assert bool((errs >= 0).all())
    with pytest.raises(ValueError, match="errors must be a contiguous float32 tensor"):
        tr.train_epoch(rows, sp.engine.s_obs, sp.engine.kmax, batch_size=batch, errors=errs[:, :-1])
    tr.close()
    sp.close()
    agents, sp = _tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4})
    sp.play_device(steps)
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    order = sp.sample_order(n_order)
    with pytest.raises(ValueError, match="errors=True needs a self-play engine built with"):
        tr.train_epoch_ring(sp, order, batch_size=batch, errors=True)
    with pytest.raises(RuntimeError, match='"feedback"'):
        sp.errors()
    assert TW._code(sp.engine.selfplay_error_values) == STATE                     # nothing was kept
    tr.close()
    sp.close()


sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"])])
def test_examples_train_with_feedback(example, extra):
    """--prioritized-feedback max: a short session runs to completion on finite losses and differs from the session without it."""
    import importlib
    mod = importlib.import_module(example)
    common = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "2", "--replay-steps", "4",
              "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5", "--device", "cuda",
              "--n-step", "3", "--prioritized-alpha", "0.6", "--prioritized-beta", "0.4"] + extra
    hist = mod.train(mod.parse_args(common + ["--prioritized-feedback", "max"]), log=None)
    assert len(hist) == 2 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    plain = mod.train(mod.parse_args(common), log=None)
    assert [h["loss"] for h in hist] != [h["loss"] for h in plain]
