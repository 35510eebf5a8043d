"""GPU: a whole training epoch in one native call (azg_trainer_epoch, PopulationTrainer.train_epoch / train_epoch_ring) -- bit for
bit the loop of azg_trainer_step calls that train_on_rows makes, from a plain array and from the self-play ring, population
invariance, the ABI's errors and the example."""
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
from trainer_util import DEV, DIMS

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

COMBOS = [("discrete", "alphazero"), ("discrete", "a0c_tuned"), ("gmm2", "a0c"), ("gmm2", "a0c_tuned")]


@pytest.mark.parametrize("n,batch", [(150, 64), (33, 16), (10, 32), (1, 1), (96, 32)])
@pytest.mark.parametrize("head,loss", COMBOS)
def test_epoch_equals_loop_of_steps(head, loss, n, batch):
    """train_epoch against train_on_rows(losses="device") from identical nets on the same rows and seeds, two epochs in a row:
    parameters, RMSprop state, the learned temperature with its Adam state and step count are torch.equal, the returned sums ==.
    (150, 64): 64 + 86, a last minibatch above batch_size; (33, 16): 16 + 17, padded to 32 rows inside; (10, 32): one short
    minibatch; (1, 1); (96, 32): three equal minibatches."""
    K = 3
    S, A = DIMS[head]
    ref = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=128, losses="device")
    ep = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=128, losses="device")
    start = TU.state_of(ref)
    TU.assert_same(start, TU.state_of(ep), "initial state")
    for epoch in range(2):
        rows = TU.make_rows(head, K, n, 100 + epoch)
        keep = rows.clone()
        seeds = [11 + epoch, 22, 33 + 5 * epoch]
        want = ref.train_on_rows(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
        got = ep.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
        assert torch.equal(rows, keep)
        assert got == want, f"epoch {epoch}"
        assert all(isinstance(v, float) and np.isfinite(v) for g in got for v in g.values())
        TU.assert_same(TU.state_of(ref), TU.state_of(ep), f"epoch {epoch}")
    end = TU.state_of(ep)
    assert not torch.equal(end["flat"], start["flat"]) and not torch.equal(end["square_avg"], start["square_avg"])
    n_mb = 2 * max(1, n // batch)
    assert int(end["alpha_step"]) == (n_mb if loss == "a0c_tuned" else 0)
    if loss == "a0c_tuned":
        assert not torch.equal(end["log_alpha"], start["log_alpha"])
    # a list of K tensors is stacked as train_on_rows stacks it
    rows = TU.make_rows(head, K, n, 200)
    assert ep.train_epoch(list(rows), S, A, batch_size=batch) == ref.train_on_rows(list(rows), S, A, batch_size=batch)
    TU.assert_same(TU.state_of(ref), TU.state_of(ep), "rows given as a list")
    ref.close()
    ep.close()


def test_ring_addressing():
    """train_epoch_ring on a PopulationSelfPlay's ring (K = 3, T = 4, 5 steps) against the same orders on _split's copies."""
    K, T, steps, batch = 3, 4, 5, 8
    S, A = DIMS["discrete"]
    agents = TU.make_agents("discrete", "a0c_tuned", K)
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, epsilon=0.1,
                                capacity_steps=8)
    assert sp.play_device(steps) == (steps, 0)   # (insert_index moves only once the ring is full)
    copies = torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps))
    n = steps * T
    assert copies.shape == (K, n, S + 3 * A + 1) and len({c.cpu().numpy().tobytes() for c in copies}) == K
    ring = PopulationTrainer(agents, max_batch=64, losses="device")
    copy = PopulationTrainer(TU.make_agents("discrete", "a0c_tuned", K), max_batch=64, losses="device")
    # (a) every row once: the orders train_epoch draws from these seeds
    seeds = [3, 1, 4]
    order = np.stack([np.random.RandomState(s).permutation(n) for s in seeds])
    got = ring.train_epoch_ring(sp, order, batch_size=batch)
    want = copy.train_epoch(copies, S, A, batch_size=batch, shuffle_seeds=seeds)
    assert got == want
    TU.assert_same(TU.state_of(ring), TU.state_of(copy), "ring, whole permutation")
    # (b) a hand-made order: first and last row, repeats, 13 entries (the remainder of 5 is absorbed: one minibatch of 13)
    order = np.array([[0, n - 1, 5, 5, 7, 12, 19, 3, 8, 1, 16, 11, 4], [n - 1, 0, 2, 9, 9, 9, 14, 6, 18, 10, 13, 17, 15],
                      [4, 8, 12, 16, 0, 1, 2, 3, n - 1, n - 2, 7, 7, 6]])
    got = ring.train_epoch_ring(sp, order, batch_size=batch)
    want = copy._epoch("train_epoch", _capi.epoch_rows(copies.data_ptr(), S, A, n), order.astype(np.int32), batch)
    assert got == want
    TU.assert_same(TU.state_of(ring), TU.state_of(copy), "ring, hand-made order")
    assert ring.alpha_step == 2 + 1   # (a): 8 + 12 rows
    # the ring is read, not changed or cleared
    assert sp.engine.selfplay_ring()[0] == steps
    assert torch.equal(torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps)), copies)
    # refusals, before anything is touched
    before = TU.state_of(ring)
    with pytest.raises(ValueError, match="outside the ring"):
        ring.train_epoch_ring(sp, np.array([[0, 1], [2, n], [3, 4]]), batch_size=batch)
    with pytest.raises(ValueError, match="outside the ring"):
        ring.train_epoch_ring(sp, np.array([[0, 1], [2, -1], [3, 4]]), batch_size=batch)
    one = PopulationTrainer(TU.make_agents("discrete", "a0c_tuned", 1, first_seed=9), max_batch=64, losses="device")
    with pytest.raises(ValueError, match="3 nets, the trainer 1"):
        one.train_epoch_ring(sp, np.array([[0, 1]]), batch_size=batch)
    one.close()
    TU.assert_same(TU.state_of(ring), before, "after refusals")
    # the trained nets go to the search as after train_on_rows
    sp.upload_flat(ring.desc, ring.flat)
    assert sp.last_weight_sync == "device"
    ring.close()
    copy.close()
    sp.close()


def test_strides_are_independent():
    """The C level on a synthetic buffer with group_stride > n_nets * group and net_stride > group, the gaps full of NaN: equal to
    the same rows in a plain array."""
    K, G, groups, n_stride, g_stride, batch = 3, 4, 3, 5, 17, 5
    head, loss = "gmm2", "a0c_tuned"
    S, A = DIMS[head]
    n = groups * G
    plain = TU.make_rows(head, K, n, 300)
    row_len = plain.shape[2]
    buf = torch.full(((groups - 1) * g_stride + (K - 1) * n_stride + G, row_len), float("nan"), device=DEV)
    for k in range(K):
        for i in range(n):
            buf[(i // G) * g_stride + k * n_stride + i % G] = plain[k, i]
    where = _capi.epoch_rows(buf.data_ptr(), S, A, n)
    where.group, where.group_stride, where.net_stride = G, g_stride, n_stride
    order = np.stack([np.random.RandomState(40 + k).permutation(n) for k in range(K)]).astype(np.int32)
    a = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=32, losses="device")
    b = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=32, losses="device")
    got = a._epoch("train_epoch", where, order, batch)
    want = b._epoch("train_epoch", _capi.epoch_rows(plain.data_ptr(), S, A, n), order, batch)
    assert got == want and all(np.isfinite(v) for g in got for v in g.values())
    TU.assert_same(TU.state_of(a), TU.state_of(b), "strided buffer")
    assert torch.isfinite(a.flat).all()
    a.close()
    b.close()


@pytest.mark.parametrize("head,loss", [("discrete", "a0c_tuned"), ("gmm2", "a0c_tuned")])
def test_population_invariance_and_determinism(head, loss):
    """Net k of a K = 3 epoch equals a K = 1 trainer's epoch on net k's rows and seed, bit for bit; two K = 3 runs are equal."""
    K, n, batch = 3, 33, 16
    S, A = DIMS[head]
    rows = TU.make_rows(head, K, n, 400)
    seeds = [7, 8, 9]
    runs = []
    for _ in range(2):
        tr = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=64, losses="device")
        info = tr.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
        runs.append((info, TU.state_of(tr)))
        tr.close()
    assert runs[0][0] == runs[1][0]
    TU.assert_same(runs[0][1], runs[1][1], "two runs")
    for k in range(K):
        tr = PopulationTrainer(TU.make_agents(head, loss, 1, first_seed=k), max_batch=64, losses="device")
        info = tr.train_epoch(rows[k:k + 1].contiguous(), S, A, batch_size=batch, shuffle_seeds=seeds[k:k + 1])
        assert info[0] == runs[0][0][k]
        TU.assert_same(runs[0][1], TU.state_of(tr), f"net {k}: K = 3 and K = 1", nets=(k, 0))
        tr.close()


def test_abi_errors_leave_everything_untouched():
    """Every refusal of azg_trainer_epoch through the raw ABI: the host checks reject each input before a launch, params,
    square_avg, loss_sums and the alpha state stay as they were, and a valid call follows."""
    N = TU.native()
    K, n, batch, max_batch = 2, 40, 16, 32
    head = "gmm2"
    S, A = DIMS[head]
    agent = TU.make_agents(head, "a0c_tuned", 1)[0]
    desc = _capi.policy_tensors(agent.nn)[0]
    cfg = _capi.loss_cfg(agent.nn, agent.loss)
    tr = N.HipTrainer(desc, K, max_batch)
    g = torch.Generator().manual_seed(9)
    params = (0.1 * torch.randn((K, tr.n_params), generator=g)).to(DEV)
    sq = torch.full_like(params, 0.25)
    sums = torch.full((K, 5), 7.0, dtype=torch.float64, device=DEV)
    la, m, v = (torch.tensor([0.1, -0.2], device=DEV), torch.zeros(K, device=DEV), torch.zeros(K, device=DEV))
    rows = TU.make_rows(head, K, n, 500)
    written = (params, sq, sums, la, m, v, rows)
    keep = [t.clone() for t in written]
    st = _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr())
    opt = _capi.rmsprop_opt(lr=1e-3, alpha=0.9, eps=1e-10, weight_decay=1e-4)
    where = _capi.epoch_rows(rows.data_ptr(), S, A, n)
    order = np.stack([np.random.RandomState(k).permutation(n) for k in range(K)]).astype(np.int32)
    torch.cuda.synchronize()

    def code(*a):
        with pytest.raises(_capi.EngineError) as ei:
            tr.epoch(*a)
        assert str(ei.value).split(": ", 1)[1]
        return ei.value.code

    def edit(obj, **kw):
        c = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    def swapped(at, value):
        o = order.copy()
        o[at] = value
        return o

    P, Q, L = params.data_ptr(), sq.data_ptr(), sums.data_ptr()
    INV, UNS = _capi.AZG_E_INVALID, _capi.AZG_E_UNSUPPORTED
    good = [P, where, order, batch, cfg, st, opt, Q, L]
    for i in (0, 1, 2, 4, 5, 6, 7, 8):   # every required pointer (the alpha state is required by the tuned loss)
        assert code(*[None if j == i else x for j, x in enumerate(good)]) == INV, i
    null_out = tr._f["trainer_epoch"](tr._h, P, where, order.ctypes.data_as(C.POINTER(C.c_int32)), n, batch, cfg, st, opt, Q, L, None)
    assert null_out == INV
    assert code(P, edit(where, rows=None), order, batch, cfg, st, opt, Q, L) == INV
    assert code(P, edit(where, struct_size=8), order, batch, cfg, st, opt, Q, L) == INV
    assert code(P, where, order, batch, edit(cfg, struct_size=8), st, opt, Q, L) == INV
    assert code(P, where, order, batch, cfg, edit(st, struct_size=8), opt, Q, L) == INV
    assert code(P, where, order, batch, cfg, edit(st, log_alpha=None), opt, Q, L) == INV
    assert code(P, where, order, batch, cfg, st, edit(opt, struct_size=8), Q, L) == INV
    for bad in (0, -3):
        assert code(P, where, order, bad, cfg, st, opt, Q, L) == INV
    assert code(P, where, order[:, :0], batch, cfg, st, opt, Q, L) == INV                       # n_order = 0
    for n_act in (0, 17):
        assert code(P, edit(where, n_actions=n_act, row_len=S + 3 * n_act + 1), order, batch, cfg, st, opt, Q, L) == INV
    for off in (-1, 1):
        assert code(P, edit(where, row_len=where.row_len + off), order, batch, cfg, st, opt, Q, L) == INV
    assert code(P, edit(where, state_dim=S + 1, row_len=where.row_len + 1), order, batch, cfg, st, opt, Q, L) == INV
    for grp in (0, -1):
        assert code(P, edit(where, group=grp), order, batch, cfg, st, opt, Q, L) == INV
    assert code(P, edit(where, rows_per_net=0), order, batch, cfg, st, opt, Q, L) == INV
    assert code(P, edit(where, net_stride=-1), order, batch, cfg, st, opt, Q, L) == INV
    for at, value in (((0, 0), n), ((1, n - 1), n), ((1, 7), -1), ((0, 3), 2 ** 31 - 1)):     # an entry outside 0 .. rows_per_net - 1
        assert code(P, where, swapped(at, value), batch, cfg, st, opt, Q, L) == INV
    assert code(P, edit(where, rows_per_net=n - 1), order, batch, cfg, st, opt, Q, L) == INV    # ... the entry n - 1 now is
    assert code(P, where, order[:, :33], 64, cfg, st, opt, Q, L) == INV                         # one minibatch of 33 > max_batch
    assert code(P, where, order[:, :39], 20, cfg, st, opt, Q, L) == INV                         # the last one absorbs 19: 39 rows
    assert code(P, where, order, batch, cfg, edit(st, step=-1), opt, Q, L) == INV
    assert code(P, where, order, batch, cfg, edit(st, step=2 ** 31 - 1), opt, Q, L) == INV
    assert code(P, where, order, batch, edit(cfg, kind=7), st, opt, Q, L) == UNS
    assert code(P, where, order, batch, edit(cfg, head=9), st, opt, Q, L) == UNS
    assert code(P, where, order, batch, edit(cfg, reduction=5), st, opt, Q, L) == UNS
    assert code(P, where, order, batch, edit(cfg, kind=_capi.LOSS_ALPHAZERO), st, opt, Q, L) == UNS   # AlphaZeroLoss, continuous head
    assert code(P, where, order, batch, edit(cfg, head=_capi.HEAD_NORMAL), st, opt, Q, L) == UNS      # n_dist = 6 is no Normal head
    for bad in (dict(grad_clip=1.0), dict(momentum=0.9), dict(centered=1)):
        assert code(P, where, order, batch, cfg, st, edit(opt, **bad), Q, L) == UNS
    torch.cuda.synchronize()
    for t, k in zip(written, keep):
        assert torch.equal(t, k)
    # a valid call follows: 16 + 24 rows, two Adam steps
    assert tr.epoch(P, where, order, batch, cfg, st, opt, Q, L) == 2
    assert not torch.equal(params, keep[0]) and not torch.equal(sq, keep[1]) and not torch.equal(la, keep[3])
    assert torch.isfinite(params).all() and torch.isfinite(sums).all() and bool((sums != 7.0).all())
    assert torch.equal(rows, keep[6])
    # an untuned loss needs no alpha state, and leaves it alone
    after = la.clone()
    assert tr.epoch(P, where, order, 8, edit(cfg, kind=_capi.LOSS_A0C, alpha=0.05), None, opt, Q, L) == 5
    assert torch.equal(la, after) and float(sums[0, 4]) == 0.0
    tr.close()


def test_example_device_epoch():
    import population_selfplay_train as X
    base = ["--game", "CartPole-v0", "--seeds", "0", "1", "2", "3", "--games-per-seed", "16", "--n-rollouts", "8", "--iters", "3",
            "--steps-per-iter", "10", "--train-rows", "150", "--batch-size", "64", "--device", DEV]
    assert X.parse_args(base).trainer == "torch"
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None)
    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None)
    assert len(epoch) == 3 and all(len(r["loss"]) == 4 and np.isfinite(r["loss"]).all() for r in epoch)
    assert all(r["weight_sync"] == "device" for r in epoch)
    assert [r["loss"] for r in epoch] == [r["loss"] for r in fused]
    assert [r["mean_return"] for r in epoch] == [r["mean_return"] for r in fused]
    assert [r["episodes_finished"] for r in epoch] == [r["episodes_finished"] for r in fused]
