"""The online epoch (azg_trainer_epoch_online, include/azgym_train_online.h): its truth -- the host loop of the four existing entry
points, made from the existing bindings -- and the planted errors of tests/test_online_replay.py and tests/test_online_replay_host.py.
TEST INFRASTRUCTURE ONLY.  Importing it needs neither a GPU nor the native library.

``pop`` is a population at the raw ABI (tests/test_weighted_loss.py's Pop): params, optimiser and alpha state, ``optim(k, step)``,
``alpha(step)``, ``cfgs`` and the native trainer ``tr``."""
import numpy as np

import priority_feedback_util as F
import priority_util as P

NAN, INF = np.float32("nan"), np.float32("inf")
SEEN, LARGE = np.float32(1e-3), np.float32(10.0)
UNSEEN_OF = {"max": (F.MAX, 0.0), "value_gap": (F.VALUE_GAP, 0.0)}


def plant(size, games, nets, seed, n_large=8, n_unseen=6, specials=True):
    """Errors [size, games]: most rows seen at 1e-3, per net ``n_large`` rows at 10.0 and ``n_unseen`` unseen; with ``specials`` one NaN
    and one +inf, both in net 0.  Returns (err, spots): spots[k] the net-numbered rows (slot * T + game) that are not at 1e-3."""
    rng = np.random.default_rng(seed)
    T = games // nets
    err = np.full((size, games), SEEN, np.float32)
    spots = []
    for k in range(nets):
        n_special = 2 if (specials and k == 0) else 0
        rows = rng.choice(size * T, n_large + n_unseen + n_special, replace=False)
        values = [LARGE] * n_large + [F.UNSEEN] * n_unseen + [NAN, INF][:n_special]
        for i, v in zip(rows, values):
            err[i // T, k * T + i % T] = v
        spots.append(np.sort(rows))
    return err, spots


def unseen_mode(unseen):
    """(AZG_UNSEEN_*, unseen_d) of the binding's ``unseen`` argument, for priority_feedback_util."""
    return UNSEEN_OF[unseen] if isinstance(unseen, str) else (F.CONSTANT, float(unseen))


def numpy_draw(err, nets, alpha, eps, unseen, seed, tree_id_base, sample_index, batch, gap=None):
    """What a minibatch draws from the errors as they stand: numpy's q of ``err`` and numpy's row draws on it.  (q, order [nets, batch])."""
    mode, d = unseen_mode(unseen)
    q = F.trained_priorities(err, nets, alpha, eps, mode, d, gap)
    return q, P.sample_rows(q, nets, seed, tree_id_base, sample_index, batch)


def ring_where(e, games, T):
    """azg_epoch_rows of the engine's ring as it stands."""
    from alphazero_gym_amd import _capi
    ptr, _, row_len = e.selfplay_rows_device()
    S, A = e.s_obs, e.kmax
    assert row_len == S + 3 * A + 1
    return _capi.epoch_rows(ptr, S, A, e.selfplay_ring()[0] * T, ring_trees=games, games_per_net=T)


def host_loop(pop, e, games, M, batch, sample_index, beta, alpha, eps, unseen, nets=False, step0=0):
    """The truth: per minibatch priorities_trained, sample_rows, is_weights and a one-minibatch errors epoch over the ring with
    opt.step + m and alpha_state.step + m.  Returns (loss sums [K, 5] float64: the chain from 0.0 over the minibatches' float32
    losses, orders [M, K, batch] int32)."""
    import torch
    K = pop.K
    where = ring_where(e, games, games // K)
    total = torch.zeros((K, 5), dtype=torch.float64)
    orders = []
    for m in range(M):
        e.selfplay_priorities_trained(alpha, eps, unseen)
        order = e.selfplay_sample_rows(batch, (sample_index + m) & 0xFFFFFFFF)
        e.selfplay_is_weights(beta)
        w_ptr, err_ptr = e.selfplay_is_weights_device(), e.selfplay_errors_device()
        e.sync()
        sums = torch.full((K, 5), float("nan"), dtype=torch.float64, device=pop.params.device)
        cfg = pop.cfgs if nets else pop.cfgs[0]
        opt = [pop.optim(k, step0 + m) for k in range(K)] if nets else pop.optim(0, step0 + m)
        torch.cuda.synchronize()
        fn = pop.tr.epoch_nets_errors if nets else pop.tr.epoch_opt_errors
        assert fn(pop.params.data_ptr(), where, w_ptr, err_ptr, order, batch, cfg, pop.alpha(step0 + m), opt, sums.data_ptr()) == 1
        one = sums.cpu()
        assert bool((one == one.float().double()).all())                          # (one minibatch: its float32 losses)
        total = total + one
        orders.append(order.copy())
    return total, np.stack(orders)


def online(pop, e, M, batch, sample_index, beta, alpha, eps, unseen, nets=False, step0=0, sums=None):
    """The call under test.  Returns (loss sums [K, 5] float64 on the CPU, drawn [M, K, batch] int32)."""
    import torch
    from alphazero_gym_amd import _capi
    K = pop.K
    if sums is None:
        sums = torch.full((K, 5), float("nan"), dtype=torch.float64, device=pop.params.device)
    prio = _capi.trained_priority_config(alpha, eps, unseen)
    torch.cuda.synchronize()
    if nets:
        drawn = pop.tr.epoch_online_nets(e, pop.params.data_ptr(), M, batch, sample_index, beta, prio, pop.cfgs, pop.alpha(step0),
                                         [pop.optim(k, step0) for k in range(K)], sums.data_ptr(), return_drawn=True)
    else:
        drawn = pop.tr.epoch_online(e, pop.params.data_ptr(), M, batch, sample_index, beta, prio, pop.cfgs[0], pop.alpha(step0),
                                    pop.optim(0, step0), sums.data_ptr(), return_drawn=True)
    return sums.cpu(), drawn


def per_net(x, K):
    """[size, G, ...] -> [K, size * T, ...]: net k's row i is slot i // T, game k * T + i % T."""
    size, G = x.shape[:2]
    T = G // K
    x = x.reshape((size, K, T) + x.shape[2:])
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((K, size * T) + x.shape[3:])
