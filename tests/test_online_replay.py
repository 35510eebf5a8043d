"""GPU: the online epoch (include/azgym_train_online.h: azg_trainer_epoch_online, _online_nets;
PopulationTrainer.train_online_ring; the examples' --prioritized-online).  The call is defined as the host loop of
azg_selfplay_priorities_trained, _sample_rows, _is_weights and a one-minibatch azg_trainer_epoch_*_errors, so every comparison is
with that loop (tests/online_replay_util.py) on a twin trainer from the same initial state, bit for bit.  Rings and sizes:
tests/nstep_util.py; the trainer at the raw ABI: tests/test_weighted_loss.py's Pop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import nstep_util as N
import online_replay_util as U
import priority_feedback_util as F
import priority_util as P
import reanalyse_util as R
import test_is_weights as TW
import test_priority_feedback as TF
import test_weighted_loss as WL
import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import DEV

pytestmark = pytest.mark.gpu

STATE, INVALID = _capi.AZG_E_STATE, _capi.AZG_E_INVALID
S, A = 4, 2                       # CartPole's observation and actions
ALPHA, EPS, BETA = 1.0, 1e-3, 0.4


class OPop(WL.Pop):
    """Pop with a choice of optimiser: Adam with grad_clip (Pop's), or plain RMSprop (the fused backward form)."""

    def __init__(self, *a, optimiser="adam", **kw):
        super().__init__(*a, **kw)
        self.optimiser = optimiser

    def optim(self, k, step):
        if self.optimiser == "adam":
            return super().optim(k, step)
        return _capi.optim("rmsprop", self.lrs[k], self.v.data_ptr(), eps=1e-8, alpha=0.99, weight_decay=1e-4, step=step)


def _policy(hidden=(32, 16), layernorm=False):
    return TU.policy(S, list(hidden), ("discrete", A), "relu", 3, layernorm=layernorm)


def _twins(n, K, nets=False, optimiser="adam", kind=None, hidden=(32, 16), max_batch=64):
    policy = _policy(hidden, TU.has_layernorm(kind))
    losses, lrs = WL._per_net_settings(K) if nets else (None, None)
    return [OPop(policy, "discrete2", K, max_batch, kind=kind, losses=losses, lrs=lrs, optimiser=optimiser) for _ in range(n)]


def _ids(case):
    return case.kw["seed"], case.kw.get("tree_id_base", 0)


def _err(e, case):
    return e.selfplay_error_values().reshape(-1, case.games)


def _both(e, case, planted, pops, M, batch, si, beta=BETA, alpha=ALPHA, unseen="max", nets=False):
    """The loop on pops[0], the call on pops[1], each from the planted errors.  Returns both sides' (sums, orders, err, q)."""
    out = []
    for pop, fn in zip(pops, (U.host_loop, U.online)):
        e.selfplay_set_error_values(planted)
        args = (pop, e, case.games) if fn is U.host_loop else (pop, e)
        sums, orders = fn(*args, M, batch, si, beta, alpha, EPS, unseen, nets=nets)
        out.append((sums, orders, _err(e, case).copy(), TW._q(e, case).copy()))
    return out


def _assert_same(want, got, pops, what):
    assert torch.equal(got[0].view(torch.int64), want[0].view(torch.int64)), f"{what}: loss sums"
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: drawn")
    np.testing.assert_array_equal(F.bits(got[2]), F.bits(want[2]), err_msg=f"{what}: err")
    np.testing.assert_array_equal(got[3], want[3], err_msg=f"{what}: q")
    WL._same(pops[1].state(), pops[0].state(), what)


@pytest.fixture(scope="module")
def rings():
    made = {}

    def get(name):
        if name not in made:
            capacity, fifo = (16, True) if name == "cartpole" else (N.STEPS[name] + 1, False)
            made[name] = TF._engine(name, capacity, fifo, N.STEPS[name])
        return made[name]
    yield get
    for _, e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ 1. against the loop

@pytest.mark.parametrize("optimiser", ["rmsprop", "adam"])
@pytest.mark.parametrize("nets", [False, True], ids=["opt", "nets"])
@pytest.mark.parametrize("name", ["cartpole", "population"])
def test_the_call_is_the_loop(rings, name, nets, optimiser):
    """The wrapped CartPole FIFO ring (528 rows: three scan segments, the last partial) and the 3-net population's ring; M = 4
    minibatches of 16 rows, A0CLossTuned, alpha 1, beta 0.4, unseen "max", planted errors of every kind.  Parameters, optimiser
    state, alpha state, err, q, loss sums and drawn are the loop's -- and the loop itself redraws from refreshed priorities, draws a
    row twice in one minibatch and a row in two minibatches, and leaves the rows it never drew alone."""
    case, e = rings(name)
    K, T, G = case.nets, case.T, case.games
    size = e.selfplay_ring()[0]
    M, batch, si = 4, 16, 7
    planted, spots = U.plant(size, G, K, 30)
    assert np.isnan(planted).sum() == 1 and np.isinf(planted).sum() == 1 and (planted == F.UNSEEN).sum() == 6 * K
    before = TW._books(e, case)
    pops = _twins(2, K, nets=nets, optimiser=optimiser)
    start = pops[0].state()
    want, got = _both(e, case, planted, pops, M, batch, si, nets=nets)
    _assert_same(want, got, pops, f"{name} {optimiser}")
    # the loop alone: the first minibatch is numpy's draw on numpy's priorities of the planted errors ...
    seed, base = _ids(case)
    q0, first = U.numpy_draw(planted, K, ALPHA, EPS, "max", seed, base, si, batch)
    orders = want[1]
    assert orders.shape == (M, K, batch) and orders.min() >= 0 and orders.max() < size * T
    np.testing.assert_array_equal(orders[0], first)
    # ... a later one is not what the first minibatch's priorities would have drawn: the refresh matters
    stale = [P.sample_rows(q0, K, seed, base, si + m, batch) for m in range(1, M)]
    assert any((orders[m + 1] != stale[m]).any() for m in range(M - 1))
    planted_net, err_net = U.per_net(planted, K), U.per_net(want[2], K)
    for k in range(K):
        sets = [set(orders[m, k].tolist()) for m in range(M)]
        assert any(len(s) < batch for s in sets), f"net {k}: no row twice in one minibatch"
        assert any(sets[a] & sets[b] for a in range(M) for b in range(a + 1, M)), f"net {k}: no row in two minibatches"
        drawn = np.zeros(size * T, bool)
        drawn[orders[:, k].reshape(-1)] = True
        assert (~drawn).sum() > size * T // 2
        np.testing.assert_array_equal(F.bits(err_net[k][~drawn]), F.bits(planted_net[k][~drawn]))   # never drawn: the planted bits
        assert (err_net[k][drawn] >= 0).all() and np.isfinite(err_net[k][drawn]).all()
        assert (F.bits(err_net[k][drawn]) != F.bits(planted_net[k][drawn])).any()
    assert all(not torch.equal(pops[0].state()[n], start[n]) for n in ("params", "v", "la"))
    assert torch.isfinite(want[0]).all()
    # the ring, the transitions, the games and the books did not move (q did: it is the last refresh's)
    now = TW._books(e, case)
    np.testing.assert_array_equal(now["ring"], before["ring"])
    assert now["books"] == before["books"]
    for k, v in before["tr"].items():
        np.testing.assert_array_equal(now["tr"][k].view(np.uint8), v.view(np.uint8))
    for p in pops:
        p.close()


# ------------------------------------------------------------------------------------------------ 2. modes

@pytest.mark.parametrize("mode", ["value_gap", "constant", "alpha0", "beta0", "M1"])
def test_modes(rings, mode):
    case, e = rings("cartpole")
    K, G = case.nets, case.games
    size = e.selfplay_ring()[0]
    planted, _ = U.plant(size, G, K, 31)
    kw = dict(value_gap=dict(unseen="value_gap"), constant=dict(unseen=0.75), alpha0=dict(alpha=0.0), beta0=dict(beta=0.0), M1=dict())[mode]
    M = 1 if mode == "M1" else 3
    pops = _twins(3 if mode == "beta0" else 2, K)
    want, got = _both(e, case, planted, pops, M, 16, 2, **kw)
    _assert_same(want, got, pops, mode)
    if mode == "alpha0":
        assert (got[3] == P.Q_ONE).all()
    if mode == "beta0":
        # every staged weight is exactly 1.0f: the state is that of the loop run with NULL weights (the unweighted bits)
        e.selfplay_set_error_values(planted)
        pop, where = pops[2], U.ring_where(e, G, case.T)
        for m in range(M):
            e.selfplay_priorities_trained(ALPHA, EPS, "max")
            order = e.selfplay_sample_rows(16, 2 + m)
            e.sync()
            sums = torch.empty((K, 5), dtype=torch.float64, device=DEV)
            pop.tr.epoch_opt_errors(pop.params.data_ptr(), where, None, e.selfplay_errors_device(), order, 16, pop.cfgs[0], pop.alpha(m),
                                    pop.optim(0, m), sums.data_ptr())
        WL._same(pops[1].state(), pop.state(), "beta 0 against NULL weights")
    for p in pops:
        p.close()


def test_a_ring_of_one_stored_step():
    """The population's ring after one step: 11 rows per net, fewer than the 16 of a minibatch."""
    name = "population"
    case, e = TF._engine(name, 4, False, 1)
    K, G = case.nets, case.games
    assert e.selfplay_ring()[0] == 1 and case.T < 16
    planted = np.full((1, G), F.UNSEEN, np.float32)
    planted[0, ::3] = np.linspace(0.01, 2.0, len(planted[0, ::3])).astype(np.float32)
    pops = _twins(2, K)
    want, got = _both(e, case, planted, pops, 2, 16, 0)
    _assert_same(want, got, pops, "one stored step")
    assert got[1].max() < case.T
    for p in pops:
        p.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 3. more segments than lanes

@pytest.mark.parametrize("nets", [1, 3])
def test_more_segments_than_a_wave_has_lanes(nets):
    """4101 CartPole games x 13 steps: 209 scan segments for one net (a partial last one), 70 for each of three."""
    base = R.CASES["cartpole"]
    case = R.Case(dict(base.kw, n_sims=2), base.net, games=4101, max_len=3, nets=nets)
    steps = 13
    _, e = TF._engine("", steps, False, steps, transitions=False, case=case)
    T = case.T
    assert (steps * T) % 256 != 0 and steps * T > 64 * 256
    rng = np.random.default_rng(9)
    planted = (10.0 ** rng.uniform(-3.0, 1.0, (steps, case.games))).astype(np.float32)
    planted[rng.random(planted.shape) < 0.5] = F.UNSEEN
    pops = _twins(2, nets, hidden=(16,))
    want, got = _both(e, case, planted, pops, 2, 32, 5)
    _assert_same(want, got, pops, f"{nets} nets")
    seed, tree_base = _ids(case)
    np.testing.assert_array_equal(want[1][0], U.numpy_draw(planted, nets, ALPHA, EPS, "max", seed, tree_base, 5, 32)[1])
    assert (want[1] // 256 >= 64).any() and (want[1] // 256 < 64).any()           # (draws on both sides of a wave's 64 segments)
    for p in pops:
        p.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 4. the other handles

@pytest.mark.parametrize("kind,hidden", [("layernorm", (32, 16)), ("wide", (512,)), ("wide_layernorm", (512,))])
def test_other_handles(rings, kind, hidden):
    case, e = rings("cartpole")
    planted, _ = U.plant(e.selfplay_ring()[0], case.games, case.nets, 32)
    pops = _twins(2, case.nets, kind=kind, hidden=hidden)
    want, got = _both(e, case, planted, pops, 2, 16, 11)
    _assert_same(want, got, pops, kind)
    for p in pops:
        p.close()


# ------------------------------------------------------------------------------------------------ 5. rank invariance

def test_a_net_is_a_one_net_engine_and_trainer_at_its_rank():
    name = "population"
    case, e = TF._engine(name, N.STEPS[name] + 1, False, N.STEPS[name])
    size, T, K = e.selfplay_ring()[0], case.T, case.nets
    planted, _ = U.plant(size, case.games, K, 33)
    pop, = _twins(1, K)
    e.selfplay_set_error_values(planted)
    start = pop.state()
    sums, drawn = U.online(pop, e, 3, 16, 4, BETA, ALPHA, EPS, "max")
    err, q, state = _err(e, case).copy(), TW._q(e, case).copy(), pop.state()
    pop.close()
    e.close()
    for k in range(K):
        one = R.Case(case.net_kw(k), case.net, games=T, max_len=case.max_len)
        one._blob = lambda j, new, k=k: case.blob(k, new)
        _, o = TF._engine(name, N.STEPS[name] + 1, False, N.STEPS[name], case=one)
        o.selfplay_set_error_values(np.ascontiguousarray(planted[:, k * T:(k + 1) * T]))
        p1, = _twins(1, 1)
        for n in ("params", "la", "am", "av"):
            getattr(p1, n).copy_(start[n][k:k + 1])
        s1, d1 = U.online(p1, o, 3, 16, 4, BETA, ALPHA, EPS, "max")
        np.testing.assert_array_equal(d1[:, 0], drawn[:, k], err_msg=f"net {k}: drawn")
        assert torch.equal(s1[0].view(torch.int64), sums[k].view(torch.int64)), f"net {k}: loss sums"
        np.testing.assert_array_equal(F.bits(_err(o, one)), F.bits(err[:, k * T:(k + 1) * T]), err_msg=f"net {k}: err")
        np.testing.assert_array_equal(TW._q(o, one), q[:, k * T:(k + 1) * T], err_msg=f"net {k}: q")
        st1 = p1.state()
        for n in st1:
            assert torch.equal(st1[n].view(torch.int32)[0], state[n].view(torch.int32)[k]), f"net {k}: {n}"
        p1.close()
        o.close()


# ------------------------------------------------------------------------------------------------ 6. refusals

def _cfg(M=2, batch=16, beta=BETA, drawn=None, **prio):
    c = _capi.AzgOnlineEpoch()
    c.struct_size, c.n_minibatches, c.batch_size, c.sample_index, c.beta = C.sizeof(c), M, batch, 0, beta
    c.prio = _capi.trained_priority_config(ALPHA, EPS, "max")
    for k, v in prio.items():
        setattr(c.prio, k, v)
    if drawn is not None:
        c.drawn = drawn.ctypes.data_as(C.POINTER(C.c_int32))
    return c


def test_refusals_write_nothing():
    name = "cartpole"
    case = N.CASES[name]
    K, G = case.nets, case.games
    pop, = _twins(1, K)
    tr = pop.tr
    fn = tr._f["trainer_epoch_online"]
    sums = torch.full((K, 5), float("nan"), dtype=torch.float64, device=DEV)
    drawn = np.full((2, K, 16), -7, np.int32)
    before = pop.state()
    torch.cuda.synchronize()

    def call(e, cfg=None, trainer=tr, cfg_loss=pop.cfgs[0], alpha=None, opt=None, params=pop.params.data_ptr(), out=sums.data_ptr()):
        cfg = _cfg(drawn=drawn) if cfg is None else cfg
        alpha = pop.alpha(0) if alpha is None else alpha
        opt = pop.optim(0, 0) if opt is None else opt
        rc = fn(trainer._h, None if e is None else e._h, params, None if cfg is False else C.byref(cfg), C.byref(cfg_loss), C.byref(alpha),
                C.byref(opt), out)
        if rc != 0:
            assert trainer._f["trainer_last_error"](trainer._h)
        return rc

    def edit(obj, **kw):
        c = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    e = R.make_engine(TW._hip(), case)
    assert call(None) == INVALID                                                  # NULL engine
    assert call(e) == STATE                                                       # no begin
    R.begin(e, case, 16, fifo=True, keep=False)
    assert call(e) == STATE                                                       # no keep_priorities
    e.selfplay_keep_priorities(True)
    assert call(e) == STATE                                                       # no keep_errors
    e.selfplay_keep_errors(True)
    assert call(e) == STATE                                                       # an empty ring
    for _ in range(3):
        e.selfplay_step()
    planted, _ = U.plant(3, G, K, 34)
    e.selfplay_set_error_values(planted)
    e.selfplay_priorities_trained(0.6, EPS, "max")
    q = e.selfplay_priority_values().copy()
    assert call(e, False) == INVALID                                              # NULL cfg
    assert call(e, edit(_cfg(), struct_size=16)) == INVALID
    for M in (0, -1):
        assert call(e, _cfg(M=M)) == INVALID
    for batch in (0, -3, 65):
        assert call(e, _cfg(batch=batch)) == INVALID
    # prio and beta: their own calls' codes
    assert call(e, _cfg(struct_size=12)) == INVALID
    assert call(e, _cfg(unseen=7)) == INVALID
    assert call(e, _cfg(unseen=_capi.UNSEEN_VALUE_GAP)) == STATE                  # no keep_transitions
    for alpha in (-0.1, float("nan"), float("inf")):
        assert call(e, _cfg(alpha=alpha)) == INVALID
    for eps in (0.0, -1e-3, float("nan")):
        assert call(e, _cfg(eps=eps)) == INVALID
    assert call(e, _cfg(unseen=_capi.UNSEEN_CONSTANT, unseen_d=-1.0)) == INVALID
    for beta in (-0.5, float("nan"), float("inf")):
        assert call(e, _cfg(beta=beta)) == INVALID
    # the two handles do not fit
    other, = _twins(1, 2)
    assert call(e, trainer=other.tr, params=other.params.data_ptr()) == INVALID   # another n_nets
    other.close()
    wrong = OPop(TU.policy(3, [16], ("discrete", A), "relu", 3), "discrete2", K, 64)
    assert call(e, trainer=wrong.tr, params=wrong.params.data_ptr()) == INVALID   # in_dim is not the observation width
    wrong.close()
    if torch.cuda.device_count() > 1:
        far = OPop.__new__(OPop)
        far.tr = TU.native().HipTrainer(_capi.policy_tensors(_policy())[0], K, 64, device_id=1)
        assert call(e, trainer=far.tr) == INVALID                                 # another device
        far.tr.close()
    # the epoch's own checks, for every minibatch's step
    assert call(e, params=None) == INVALID
    assert call(e, out=None) == INVALID
    assert call(e, cfg_loss=edit(pop.cfgs[0], struct_size=8)) == INVALID
    assert call(e, cfg_loss=edit(pop.cfgs[0], kind=7)) == _capi.AZG_E_UNSUPPORTED
    assert call(e, opt=edit(pop.optim(0, 0), struct_size=8)) == INVALID
    assert call(e, opt=pop.optim(0, 2 ** 31 - 2)) == INVALID                      # step + M - 1 does not fit
    assert call(e, alpha=pop.alpha(2 ** 31 - 2)) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(sums).all()) and (drawn == -7).all()
    WL._same(pop.state(), before, "after refusals")
    np.testing.assert_array_equal(e.selfplay_priority_values(), q)
    np.testing.assert_array_equal(F.bits(e.selfplay_error_values()), F.bits(planted.reshape(-1)))
    # both handles are still usable; afterwards q counts as computed and the weights as not
    e.selfplay_is_weights(BETA)
    assert e.selfplay_is_weights_device() != 0
    assert call(e) == 0
    assert torch.isfinite(sums).all() and drawn.min() >= 0 and drawn.max() < 3 * G
    assert TW._code(e.selfplay_is_weights_device) == STATE
    e.selfplay_sample_rows(4, 0)
    e.selfplay_is_weights(BETA)
    assert e.selfplay_is_weights_device() != 0
    e.selfplay_step()                                                             # a step makes the priorities stale, as ever
    assert TW._code(e.selfplay_sample_rows, 4, 0) == STATE
    assert call(e) == 0                                                           # (the call refreshes them itself)
    pop.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 7. Python

def _state_of(tr, sp):
    torch.cuda.synchronize()
    s = dict(flat=tr.flat, log_alpha=tr.log_alpha, alpha_exp_avg=tr.alpha_exp_avg, alpha_exp_avg_sq=tr.alpha_exp_avg_sq)
    for n in ("square_avg", "exp_avg", "exp_avg_sq"):
        if getattr(tr, n) is not None:
            s[n] = getattr(tr, n)
    out = {n: t.detach().cpu().clone() for n, t in s.items()}
    out["err"] = torch.from_numpy(sp.errors().copy())
    return out, (tr.opt_step, tr.alpha_step, sp._sample_index)


@pytest.mark.parametrize("form", ["rmsprop", "agents", "per_net"])
def test_train_online_ring_is_the_python_loop(form):
    K, T, steps, batch, M = 2, 4, 5, 8, 3
    kw = dict(rmsprop={}, agents=dict(optimizers="agents"), per_net=dict(optimizers="agents", per_net=True))[form]
    sides = []
    for online in (False, True):
        agents, sp = TF._tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4, "feedback": "max"})
        assert sp.play_device(steps) == (steps, 0)
        tr = PopulationTrainer(agents, max_batch=64, losses="device", **kw)
        sp.sample_order(4)                                                        # (the counter does not start at 0)
        if online:
            info, drawn = tr.train_online_ring(sp, M, batch_size=batch, return_drawn=True)
            assert TW._code(sp.engine.selfplay_is_weights_device) == STATE
        else:
            info, drawn = [{} for _ in range(K)], []
            for _ in range(M):
                sp.priorities()
                order = sp.sample_order(batch)
                sp.is_weights()
                one = tr.train_epoch_ring(sp, order, batch_size=batch, weights="priority", errors=True)
                drawn.append(order)
                for total, i in zip(info, one):
                    for key, val in i.items():
                        total[key] = total.get(key, 0.0) + val
            drawn = np.stack(drawn)
        sides.append((info, drawn, _state_of(tr, sp)))
        tr.close()
        sp.close()
    (want_info, want_drawn, (want, want_counts)), (info, drawn, (got, counts)) = sides
    np.testing.assert_array_equal(drawn, want_drawn)
    assert drawn.shape == (M, K, batch) and drawn.dtype == np.int32
    assert info == want_info and all(np.isfinite(v) for i in info for v in i.values())
    assert counts == want_counts and counts[2] == 1 + M
    assert set(got) == set(want)
    for n in want:
        assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), n
    assert (got["err"] >= 0).any() and (got["err"] == -1).any()


def test_train_online_ring_refusals():
    agents, sp = TF._tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4})
    sp.play_device(3)
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    with pytest.raises(ValueError, match='"feedback"'):
        tr.train_online_ring(sp, 2, batch_size=8)
    tr.close()
    sp.close()
    agents, sp = TF._tiny({"alpha": 0.6, "eps": 1e-3, "feedback": 0.5})
    sp.play_device(3)
    tr = PopulationTrainer(agents, max_batch=64, losses="torch")
    with pytest.raises(ValueError, match='losses="device"'):
        tr.train_online_ring(sp, 2, batch_size=8)
    tr.close()
    tr = PopulationTrainer(agents, max_batch=64, losses="device")
    for M, batch in ((0, 8), (2, 0), (2, 65)):
        with pytest.raises(ValueError, match="n_minibatches >= 1 and a batch_size"):
            tr.train_online_ring(sp, M, batch_size=batch)
    assert sp._sample_index == 0 and tr.opt_step == 0
    info = tr.train_online_ring(sp, 2, batch_size=8)                              # beta absent: 0
    assert len(info) == 2 and all(np.isfinite(v) for i in info for v in i.values()) and sp._sample_index == 2
    tr.close()
    sp.close()


sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"])])
def test_examples_train_online(example, extra):
    """--prioritized-online: a short session runs to completion on finite losses and differs from the session without it."""
    import importlib
    mod = importlib.import_module(example)
    common = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "2", "--replay-steps", "4",
              "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5", "--device", "cuda",
              "--n-step", "3", "--prioritized-alpha", "0.6", "--prioritized-beta", "0.4", "--prioritized-feedback", "max"] + extra
    hist = mod.train(mod.parse_args(common + ["--prioritized-online"]), log=None)
    assert len(hist) == 2 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    plain = mod.train(mod.parse_args(common), log=None)
    assert [h["loss"] for h in hist] != [h["loss"] for h in plain]
