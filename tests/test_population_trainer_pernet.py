"""GPU: per-net optimiser and loss settings in the population trainer (the *_nets entry points, PopulationTrainer(per_net=True)).
The truth is always the existing one-net trainer: net k of a *_nets call against a one-net trainer of the same shape given entry k
through the *_opt entry point on net k's slices, compared with torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.agents import ContinuousAgent, DiscreteAgent
from alphazero_gym_amd.agent.buffers import DeviceReplay
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import ADAM_WD as ADAM_CFG, DEV, DIMS

pytestmark = pytest.mark.gpu

K3, B21, IN_DIM = 3, 21, 3   # 21 rows pad to 32: two row tiles

# (name, hidden, HipTrainer keywords, LayerNorm descriptor); [272, 32] has P > 2 * 4096: several update workgroups per net
TRAINERS = [("narrow", [32, 16], {}, False), ("layernorm", [16], dict(layernorm=True), True),
            ("wide", [272, 32], dict(wide=True), False), ("wide_layernorm", [272, 32], dict(wide_layernorm=True), True)]
PAIRS = ["alphazero_discrete", "a0c_normal", "tuned_gmm2"]
# the loss / head pairs spread over the matrix: every pair meets both optimisers, every trainer two pairs
MATRIX = [(t, o, PAIRS[(i + j) % 3]) for i, t in enumerate(TRAINERS) for j, o in enumerate(("rmsprop", "adam"))]

# per net: lr, weight_decay, grad_clip, eps, RMSprop's alpha, Adam's betas.  Net 0 plain, net 1 everything else, net 2 lr 0.
OPT_NETS = [dict(lr=1e-3, weight_decay=0.0, grad_clip=0.0, eps=1e-8, alpha=0.99, betas=(0.9, 0.999)),
            dict(lr=3e-4, weight_decay=1e-2, grad_clip=0.5, eps=1e-6, alpha=0.9, betas=(0.8, 0.99)),
            dict(lr=0.0, weight_decay=0.0, grad_clip=0.0, eps=1e-8, alpha=0.99, betas=(0.9, 0.999))]
LOSS_NETS = {
    "alphazero_discrete": [dict(policy_coeff=1.0, value_coeff=0.5), dict(policy_coeff=0.7, value_coeff=1.3), dict(policy_coeff=2.0, value_coeff=0.25)],
    "a0c_normal": [dict(tau=1.0, alpha=0.1), dict(tau=0.5, alpha=0.3), dict(tau=2.0, alpha=0.01)],
    "tuned_gmm2": [dict(target_entropy=-1.0, alpha_lr=1e-3, alpha_clip=0.0), dict(target_entropy=-0.5, alpha_lr=3e-3, alpha_clip=0.1),
                   dict(target_entropy=-2.0, alpha_lr=1e-2, alpha_clip=1.0)],
}
# pair -> (n_dist, num_components, n_actions, loss kind, head kind, action_bound)
PAIR_DIMS = {"alphazero_discrete": (3, 0, 3, _capi.LOSS_ALPHAZERO, _capi.HEAD_DISCRETE, 0.0),
             "a0c_normal": (2, 0, 4, _capi.LOSS_A0C, _capi.HEAD_NORMAL, 2.0),
             "tuned_gmm2": (6, 2, 4, _capi.LOSS_A0C_TUNED, _capi.HEAD_GMM, 2.0)}


def _cfg(pair, **kw):
    _, _, _, kind, head, bound = PAIR_DIMS[pair]
    c = _capi.AzgLossCfg()
    c.struct_size = C.sizeof(_capi.AzgLossCfg)
    c.kind, c.head, c.reduction, c.action_bound = kind, head, _capi.REDUCE["mean"], bound
    c.tau, c.policy_coeff, c.value_coeff, c.alpha = 1.0, 1.0, 0.5, 0.2
    c.target_entropy, c.alpha_lr, c.alpha_beta1, c.alpha_beta2, c.alpha_eps = -1.0, 1e-3, 0.9, 0.999, 1e-8
    for key, val in kw.items():
        assert hasattr(c, key)
        setattr(c, key, val)
    return c


def _desc(pair, hidden, ln, in_dim=IN_DIM):
    n_dist, comps = PAIR_DIMS[pair][:2]
    return _capi.make_desc(in_dim, hidden, n_dist, "elu", num_components=comps, layernorm=ln)


def _batch(pair, K, B, seed, in_dim=IN_DIM):
    """obs [K, B, in_dim], actions / counts [K, B, A], values [K, B] on the GPU; large value targets, so that gradient norms pass
    net 1's grad_clip."""
    A = PAIR_DIMS[pair][2]
    rng = np.random.RandomState(seed)
    obs = rng.randn(K, B, in_dim)
    if pair == "alphazero_discrete":
        actions, counts = np.tile(np.arange(A, dtype=np.float64), (K, B, 1)), rng.randint(0, 9, (K, B, A))
    else:
        actions, counts = rng.uniform(-1.9, 1.9, (K, B, A)), rng.randint(1, 9, (K, B, A))
    values = 10.0 * rng.randn(K, B)
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV) for x in (obs, actions, counts, values))


class State:
    """Everything a step reads and writes for n nets: params, optimiser state, alpha state, and the outputs of the last step."""

    def __init__(self, P, n_raw, ks, B, seed=5):
        g = torch.Generator().manual_seed(seed)
        full = 0.2 * torch.randn((K3, P), generator=g)
        self.params = full[ks].contiguous().to(DEV)
        n = len(ks)
        self.s0, self.s1 = torch.full((n, P), 0.25, device=DEV), torch.full((n, P), 0.01, device=DEV)
        self.log_alpha = torch.tensor([-0.5, 0.1, -1.0])[ks].contiguous().to(DEV)
        self.a_m, self.a_v = torch.full((n,), 0.01, device=DEV), torch.full((n,), 0.02, device=DEV)
        self.grads, self.norms = torch.zeros((n, P), device=DEV), torch.full((n,), -1.0, device=DEV)
        self.raw, self.d_raw = torch.zeros((n, B, n_raw), device=DEV), torch.zeros((n, B, n_raw), device=DEV)
        self.losses = torch.zeros((n, len(_capi.LOSS_KEYS)), device=DEV)

    def alpha(self, step):
        return _capi.alpha_state(step, self.log_alpha.data_ptr(), self.a_m.data_ptr(), self.a_v.data_ptr())

    def optim(self, kind, net, step, norms=True):
        """azg_optim of net ``net``'s settings over this state's arrays."""
        s = OPT_NETS[net]
        return _capi.optim(kind, s["lr"], self.s0.data_ptr(), self.s1.data_ptr() if kind == "adam" else None, eps=s["eps"],
                           weight_decay=s["weight_decay"], alpha=s["alpha"], betas=s["betas"], grad_clip=s["grad_clip"], step=step,
                           grad_norms=self.norms.data_ptr() if norms else None)

    def snapshot(self):
        names = ("params", "s0", "s1", "log_alpha", "a_m", "a_v", "grads", "norms", "raw", "d_raw", "losses")
        return {n: getattr(self, n).detach().cpu().clone() for n in names}


def _step_args(st, batch, B, A):
    obs, actions, counts, values = batch
    return (st.params.data_ptr(), obs.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), B, A)


def _same(got, want, k, what):
    for name in want:
        assert torch.equal(got[name][k], want[name][0]), f"{what}: {name} of net {k} differs from its one-net run"


@pytest.mark.parametrize("trainer,optimizer,pair", MATRIX, ids=[f"{t[0]}-{o}-{p}" for t, o, p in MATRIX])
def test_nets_against_one_net_trainers(trainer, optimizer, pair):
    """step_nets of K = 3 nets with three different settings, two consecutive steps, against three one-net step_opt runs.  With
    RMSprop no grad_norms are asked for, so net 0's and net 2's one-net runs take the FUSED backward kernel; with Adam they are."""
    N = TU.native()
    _, hidden, kw, ln = trainer
    desc = _desc(pair, hidden, ln)
    A = PAIR_DIMS[pair][2]
    norms = optimizer == "adam"
    cfgs = [_cfg(pair, **s) for s in LOSS_NETS[pair]]
    batches = [_batch(pair, K3, B21, 31 + i) for i in range(2)]
    pop = N.HipTrainer(desc, K3, 32, **kw)
    st = State(pop.n_params, pop.n_raw, list(range(K3)), B21)
    start = st.snapshot()
    got = []
    torch.cuda.synchronize()
    for i, batch in enumerate(batches):
        pop.step_nets(*_step_args(st, batch, B21, A), cfgs, st.alpha(i), [st.optim(optimizer, k, i, norms) for k in range(K3)],
                      st.grads.data_ptr(), st.raw.data_ptr(), st.losses.data_ptr())
        pop.read_d_raw(B21, st.d_raw.data_ptr())
        got.append(st.snapshot())
    pop.close()
    one = N.HipTrainer(desc, 1, 32, **kw)
    for k in range(K3):
        s1 = State(one.n_params, one.n_raw, [k], B21)
        for i, batch in enumerate(batches):
            mine = tuple(x[k:k + 1].contiguous() for x in batch)
            torch.cuda.synchronize()
            one.step_opt(*_step_args(s1, mine, B21, A), cfgs[k], s1.alpha(i), s1.optim(optimizer, k, i, norms), s1.grads.data_ptr(),
                         s1.raw.data_ptr(), s1.losses.data_ptr())
            one.read_d_raw(B21, s1.d_raw.data_ptr())
            want = s1.snapshot()
            if not norms:
                want.pop("norms")
            if optimizer != "adam":
                want.pop("s1")
            _same(got[i], want, k, f"step {i}")
    one.close()
    last = got[-1]
    assert torch.isfinite(last["params"]).all() and torch.isfinite(last["losses"]).all()
    # net 2 has lr 0: its parameters come back unchanged, its optimiser state has stepped
    assert torch.equal(last["params"][2], start["params"][2]) and not torch.equal(last["s0"][2], start["s0"][2])
    assert not torch.equal(last["params"][0], start["params"][0]) and not torch.equal(last["params"][1], start["params"][1])
    if norms:
        print(f"{trainer[0]} {pair}: gradient norms {last['norms'].tolist()}, net 1 clips at {OPT_NETS[1]['grad_clip']}")
        assert float(last["norms"][1]) > OPT_NETS[1]["grad_clip"], "the batch must make net 1 clip"
    if pair == "tuned_gmm2":
        assert not torch.equal(last["log_alpha"], start["log_alpha"])


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_identical_entries_are_step_opt(optimizer):
    """K identical entries: step_nets gives step_opt's bits (RMSprop without clip or norms: the fused kernel's)."""
    N = TU.native()
    pair = "tuned_gmm2"
    desc = _desc(pair, [32, 16], False)
    A = PAIR_DIMS[pair][2]
    net = 0 if optimizer == "rmsprop" else 1
    norms = optimizer == "adam"
    cfg = _cfg(pair, **LOSS_NETS[pair][1])
    batch = _batch(pair, K3, B21, 77)
    tr = N.HipTrainer(desc, K3, 32)
    outs = []
    for nets in (False, True):
        st = State(tr.n_params, tr.n_raw, list(range(K3)), B21)
        torch.cuda.synchronize()
        if nets:
            tr.step_nets(*_step_args(st, batch, B21, A), [cfg] * K3, st.alpha(4), [st.optim(optimizer, net, 4, norms) for _ in range(K3)],
                         st.grads.data_ptr(), st.raw.data_ptr(), st.losses.data_ptr())
        else:
            tr.step_opt(*_step_args(st, batch, B21, A), cfg, st.alpha(4), st.optim(optimizer, net, 4, norms), st.grads.data_ptr(),
                        st.raw.data_ptr(), st.losses.data_ptr())
        tr.read_d_raw(B21, st.d_raw.data_ptr())
        outs.append(st.snapshot())
    tr.close()
    for name in outs[0]:
        assert torch.equal(outs[0][name], outs[1][name]), name
    assert not torch.equal(outs[0]["params"], State(outs[0]["params"].shape[1], 7, list(range(K3)), B21).params.cpu())


def test_epoch_nets():
    """epoch_nets over 7 ordered rows, batch_size 2 (minibatches of 2, 2 and 3 rows), Adam and a tuned alpha with three settings:
    against the same minibatches through step_nets one by one (steps + 0, + 1, + 2), and per net against a one-net epoch_opt."""
    N = TU.native()
    pair, optimizer, n, in_dim = "tuned_gmm2", "adam", 7, 3
    desc = _desc(pair, [32, 16], False)
    A = PAIR_DIMS[pair][2]
    cfgs = [_cfg(pair, **s) for s in LOSS_NETS[pair]]
    obs, actions, counts, values = _batch(pair, K3, n, 13)
    rows = torch.cat([obs, actions, counts, torch.zeros_like(actions), values[..., None]], dim=-1).contiguous()
    order = np.tile(np.arange(n, dtype=np.int32), (K3, 1))
    step0 = 5
    tr = N.HipTrainer(desc, K3, 32)
    ep = State(tr.n_params, tr.n_raw, list(range(K3)), 3)
    sums = torch.zeros((K3, 5), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    n_mb = tr.epoch_nets(ep.params.data_ptr(), _capi.epoch_rows(rows.data_ptr(), in_dim, A, n), order, 2, cfgs, ep.alpha(step0),
                         [ep.optim(optimizer, k, step0) for k in range(K3)], sums.data_ptr())
    assert n_mb == 3
    tr.read_d_raw(3, ep.d_raw.data_ptr())
    torch.cuda.synchronize()
    # the same minibatches one by one
    by = State(tr.n_params, tr.n_raw, list(range(K3)), 3)
    chain = np.zeros((K3, 5))
    for m, (i, j) in enumerate(((0, 2), (2, 4), (4, 7))):
        mb = tuple(x[:, i:j].contiguous() for x in (obs, actions, counts, values))
        torch.cuda.synchronize()
        tr.step_nets(*_step_args(by, mb, j - i, A), cfgs, by.alpha(step0 + m), [by.optim(optimizer, k, step0 + m) for k in range(K3)],
                     None, None, by.losses.data_ptr())
        chain = chain + by.losses.cpu().double().numpy()
    tr.read_d_raw(3, by.d_raw.data_ptr())
    torch.cuda.synchronize()
    tr.close()
    a, b = ep.snapshot(), by.snapshot()
    for name in ("params", "s0", "s1", "log_alpha", "a_m", "a_v", "norms", "d_raw"):
        assert torch.equal(a[name], b[name]), f"epoch_nets against its steps: {name}"
    assert np.array_equal(sums.cpu().numpy(), chain)
    # per net: a one-net epoch_opt
    one = N.HipTrainer(desc, 1, 32)
    for k in range(K3):
        s1 = State(one.n_params, one.n_raw, [k], 3)
        sums1 = torch.zeros((1, 5), dtype=torch.float64, device=DEV)
        rows1 = rows[k:k + 1].contiguous()
        torch.cuda.synchronize()
        assert one.epoch_opt(s1.params.data_ptr(), _capi.epoch_rows(rows1.data_ptr(), in_dim, A, n), order[:1], 2, cfgs[k],
                             s1.alpha(step0), s1.optim(optimizer, k, step0), sums1.data_ptr()) == 3
        one.read_d_raw(3, s1.d_raw.data_ptr())
        torch.cuda.synchronize()
        want = s1.snapshot()
        for name in ("params", "s0", "s1", "log_alpha", "a_m", "a_v", "norms", "d_raw"):
            assert torch.equal(a[name][k], want[name][0]), f"epoch_nets net {k} against epoch_opt: {name}"
        assert torch.equal(sums[k].cpu(), sums1[0].cpu())
    one.close()
    assert torch.isfinite(a["params"]).all() and float(sums.abs().sum()) > 0


# ---- PopulationTrainer(per_net=True) ----

LOSS_TUNED = dict(run.LOSS_TUNED, device=DEV)
NET_SETTINGS = [dict(lr=1e-3, clip=0.5, tau=1.0), dict(lr=3e-4, clip=0.0, tau=0.5), dict(lr=3e-3, clip=0.05, tau=2.0)]


def _agents(head, ks, hidden, settings=NET_SETTINGS):
    """A0C-tuned Adam agents, net k's weights from torch.manual_seed(k), with net k's lr / grad_clip / tau."""
    agents = []
    for k in ks:
        torch.manual_seed(k)
        if head == "discrete":
            cfg = run.DISCRETE_DEFAULTS
            policy = dict(cfg["policy"], hidden_dimensions=hidden, representation_dim=4, action_dim=1, num_actions=2)
            a = DiscreteAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=DEV, num_actions=2), loss_cfg=LOSS_TUNED,
                              optimizer_cfg=ADAM_CFG, device=DEV, **dict(cfg["agent"], grad_clip=0.5))
        else:
            cfg = run.CONTINUOUS_DEFAULTS
            policy = dict(cfg["policy"], hidden_dimensions=hidden, representation_dim=3, action_dim=1, action_bound=2.0, num_components=2)
            a = ContinuousAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=DEV), loss_cfg=LOSS_TUNED, optimizer_cfg=ADAM_CFG,
                                device=DEV, **dict(cfg["agent"], grad_clip=0.5))
        s = settings[k]
        a.optimizer.param_groups[0]["lr"], a.clip, a.loss.tau = s["lr"], s["clip"], s["tau"]
        agents.append(a)
    return agents


def _rows(head, K, n, seed):
    """[K, n, row] float32 on the GPU: obs | actions[A] | counts[A] | Q[A] | V."""
    S, A = DIMS[head]
    rng = np.random.RandomState(seed)
    obs = rng.randn(K, n, S)
    if head == "discrete":
        actions, counts = np.tile(np.arange(A, dtype=np.float64), (K, n, 1)), rng.randint(0, 9, (K, n, A))
    else:
        actions, counts = rng.uniform(-1.9, 1.9, (K, n, A)), rng.randint(1, 9, (K, n, A))
    return torch.from_numpy(np.concatenate([obs, actions, counts, rng.randn(K, n, A), 5.0 * rng.randn(K, n, 1)], axis=-1).astype(np.float32)).to(DEV)


def _state(tr):
    s = dict(flat=tr.flat, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq, log_alpha=tr.log_alpha, alpha_exp_avg=tr.alpha_exp_avg,
             alpha_exp_avg_sq=tr.alpha_exp_avg_sq, grad_norms=tr.last_grad_norms)
    return {k: v.detach().cpu().clone() for k, v in s.items()}


def test_population_trainer_per_net():
    """update and train_epoch of three agents with different lr / grad_clip / tau against three one-agent PopulationTrainers."""
    head, K = "gmm2", 3
    S, A = DIMS[head]
    tr = PopulationTrainer(_agents(head, range(K), [32, 16]), max_batch=64, losses="device", optimizers="agents", per_net=True)
    ones = [PopulationTrainer(_agents(head, [k], [32, 16]), max_batch=64, losses="device", optimizers="agents") for k in range(K)]
    batch, rows, seeds = _rows(head, K, 21, 3), _rows(head, K, 40, 4), [5, 6, 7]
    got = tr.update(TU.split_rows(batch, S, A))
    after_update = _state(tr)
    got_epoch = tr.train_epoch(rows, S, A, batch_size=16, shuffle_seeds=seeds)
    after_epoch = _state(tr)
    assert tr.opt_step == tr.alpha_step == 3
    for k, one in enumerate(ones):
        assert one.update(TU.split_rows(batch[k:k + 1], S, A)) == [got[k]]
        for key, val in _state(one).items():
            assert torch.equal(after_update[key][k], val[0]), f"update: {key} of net {k}"
        assert one.train_epoch(rows[k:k + 1], S, A, batch_size=16, shuffle_seeds=seeds[k:k + 1]) == [got_epoch[k]]
        for key, val in _state(one).items():
            assert torch.equal(after_epoch[key][k], val[0]), f"train_epoch: {key} of net {k}"
        one.close()
    assert float(after_update["grad_norms"][0]) > NET_SETTINGS[0]["clip"]
    tr.close()
    # export_alpha (close) handed every net its own temperature
    for k, a in enumerate(tr.agents):
        assert float(a.loss.log_alpha.detach()) == float(after_epoch["log_alpha"][k])


def test_per_net_equal_settings_is_the_shared_trainer():
    """per_net=True on agents with equal settings gives per_net=False's bits."""
    head, K = "gmm2", 3
    S, A = DIMS[head]
    same = [NET_SETTINGS[0]] * K
    a = PopulationTrainer(_agents(head, range(K), [32, 16], same), max_batch=64, losses="device", optimizers="agents", per_net=True)
    b = PopulationTrainer(_agents(head, range(K), [32, 16], same), max_batch=64, losses="device", optimizers="agents")
    batch, rows = _rows(head, K, 21, 3), _rows(head, K, 40, 4)
    assert a.update(TU.split_rows(batch, S, A)) == b.update(TU.split_rows(batch, S, A))
    assert a.train_epoch(rows, S, A, batch_size=16, shuffle_seeds=[1, 2, 3]) == b.train_epoch(rows, S, A, batch_size=16, shuffle_seeds=[1, 2, 3])
    sa, sb = _state(a), _state(b)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    a.close()
    b.close()


def test_per_net_ring_epoch():
    """train_epoch_ring on a 2-net CartPole [16] self-play ring of 4 games x 3 steps against train_epoch on a copy of the rows."""
    K, T, steps, batch = 2, 4, 3, 4
    S, A = DIMS["discrete"]
    agents = _agents("discrete", range(K), [16])
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, epsilon=0.1,
                                capacity_steps=4)
    assert sp.play_device(steps) == (steps, 0)
    copies = torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps))
    n = steps * T
    ring = PopulationTrainer(agents, max_batch=16, losses="device", optimizers="agents", per_net=True)
    ref = PopulationTrainer(_agents("discrete", range(K), [16]), max_batch=16, losses="device", optimizers="agents", per_net=True)
    seeds = [3, 1]
    order = np.stack([np.random.RandomState(s).permutation(n) for s in seeds])
    got = ring.train_epoch_ring(sp, order, batch_size=batch)
    want = ref.train_epoch(copies, S, A, batch_size=batch, shuffle_seeds=seeds)
    assert got == want and ring.opt_step == ring.alpha_step == 3
    sa, sb = _state(ring), _state(ref)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert not torch.equal(sa["flat"][0], sa["flat"][1])
    ring.close()
    ref.close()
    sp.close()


def test_reload_settings():
    """reload_settings() after changing one agent's lr changes that net's next step only."""
    head, K = "gmm2", 3
    S, A = DIMS[head]
    changed = PopulationTrainer(_agents(head, range(K), [32, 16]), max_batch=64, losses="device", optimizers="agents", per_net=True)
    kept = PopulationTrainer(_agents(head, range(K), [32, 16]), max_batch=64, losses="device", optimizers="agents", per_net=True)
    b0, b1 = TU.split_rows(_rows(head, K, 21, 8), S, A), TU.split_rows(_rows(head, K, 21, 9), S, A)
    assert changed.update(b0) == kept.update(b0)
    changed.agents[1].optimizer.param_groups[0]["lr"] = 5e-3
    before = _state(changed)
    changed.update(b1)   # not reloaded yet: the old settings
    stale = _state(changed)
    kept.update(b1)
    for key, val in _state(kept).items():
        assert torch.equal(stale[key], val), f"before reload_settings: {key}"
    # again from the state before that step, now reloaded
    again = PopulationTrainer(_agents(head, range(K), [32, 16]), max_batch=64, losses="device", optimizers="agents", per_net=True)
    again.update(b0)
    for key, val in _state(again).items():
        assert torch.equal(before[key], val)
    again.agents[1].optimizer.param_groups[0]["lr"] = 5e-3
    again.reload_settings()
    again.update(b1)
    new, old = _state(again), _state(kept)
    for key in new:
        for k in (0, 2):
            assert torch.equal(new[key][k], old[key][k]), f"net {k} must not change: {key}"
    assert not torch.equal(new["flat"][1], old["flat"][1])
    assert torch.equal(new["exp_avg"][1], old["exp_avg"][1])   # (Adam's moments do not depend on lr)
    # a refusal keeps the settings
    again.agents[2].clip = -1.0
    with pytest.raises(ValueError, match="grad_clip must be >= 0"):
        again.reload_settings()
    again.agents[2].clip = NET_SETTINGS[2]["clip"]
    assert [s[1] for s in again._net_opt_settings] == [1e-3, 5e-3, 3e-3]
    with pytest.raises(ValueError, match="per_net=True"):
        PopulationTrainer(_agents(head, [0], [32, 16]), max_batch=64, losses="device", optimizers="agents").reload_settings()
    for t in (changed, kept, again):
        t.close()


# ---- refusals ----

def test_refusals_write_nothing():
    N = TU.native()
    pair, K, B = "tuned_gmm2", 2, 8
    A = PAIR_DIMS[pair][2]
    desc = _desc(pair, [32, 16], False)
    tr = N.HipTrainer(desc, K, 32)
    st = State(tr.n_params, tr.n_raw, [0, 1], B)
    other = torch.zeros_like(st.s0)
    batch = _batch(pair, K, B, 3)
    obs, actions, counts, values = batch
    rows = torch.cat([obs, actions, counts, torch.zeros_like(actions), values[..., None]], dim=-1).contiguous()
    order = np.tile(np.arange(B, dtype=np.int32), (K, 1))
    sums = torch.zeros((K, 5), dtype=torch.float64, device=DEV)
    keep = st.snapshot()
    INV = _capi.AZG_E_INVALID

    def opts(**kw1):
        """Valid Adam entries; kw1 changes entry 1."""
        o = [st.optim("adam", 1, 3) for _ in range(K)]
        for key, val in kw1.items():
            setattr(o[1], key, val)
        return o

    def cfgs(**kw1):
        return [_cfg(pair), _cfg(pair, **kw1)]

    # (entries, expected code, words the message must hold)
    cases = [
        (opts(kind=_capi.OPT_RMSPROP), cfgs(), INV, ("azg_optim.kind", "net 1")),
        (opts(state0=other.data_ptr()), cfgs(), INV, ("azg_optim.state0", "net 1")),
        (opts(step=4), cfgs(), INV, ("azg_optim.step", "net 1")),
        (opts(), cfgs(head=_capi.HEAD_NORMAL), INV, ("azg_loss_cfg.head", "net 1")),
        (opts(), cfgs(reduction=_capi.REDUCE["sum"]), INV, ("azg_loss_cfg.reduction", "net 1")),
        (opts(lr=-1e-3), cfgs(), INV, ("lr", "net 1")),
        (opts(beta1=1.0), cfgs(), INV, ("beta", "net 1")),
        (None, cfgs(), INV, ("NULL",)),
        (opts(), None, INV, ("NULL",)),
    ]
    torch.cuda.synchronize()
    for o, c, want, words in cases:
        calls = [lambda: tr.step_nets(*_step_args(st, batch, B, A), c, st.alpha(3), o, st.grads.data_ptr(), st.raw.data_ptr(),
                                      st.losses.data_ptr()),
                 lambda: tr.epoch_nets(st.params.data_ptr(), _capi.epoch_rows(rows.data_ptr(), IN_DIM, A, B), order, 4, c, st.alpha(3), o,
                                       sums.data_ptr())]
        for call in calls:
            with pytest.raises(_capi.EngineError) as ei:
                call()
            assert ei.value.code == want, str(ei.value)
            for w in words:
                assert w in str(ei.value), (w, str(ei.value))
    # the two halves alone
    tr.forward(st.params.data_ptr(), obs.data_ptr(), B, st.raw.data_ptr())
    raw_keep = st.raw.clone()
    for o, words in ((opts(kind=_capi.OPT_RMSPROP), ("azg_optim.kind", "net 1")), (opts(lr=-1e-3), ("lr", "net 1")), (None, ("NULL",))):
        with pytest.raises(_capi.EngineError) as ei:
            tr.backward_step_nets(st.params.data_ptr(), st.raw.data_ptr(), B, o, st.grads.data_ptr())
        assert ei.value.code == INV and all(w in str(ei.value) for w in words), str(ei.value)
    for c, words in ((cfgs(head=_capi.HEAD_NORMAL), ("azg_loss_cfg.head", "net 1")), (None, ("NULL",))):
        with pytest.raises(_capi.EngineError) as ei:
            tr.loss_nets(st.raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), B, A, c, st.alpha(3),
                         st.d_raw.data_ptr(), st.losses.data_ptr())
        assert ei.value.code == INV and all(w in str(ei.value) for w in words), str(ei.value)
    with pytest.raises(ValueError, match="per net"):
        tr.step_nets(*_step_args(st, batch, B, A), cfgs()[:1], st.alpha(3), opts(), None, None, st.losses.data_ptr())
    torch.cuda.synchronize()
    after = st.snapshot()
    after["raw"] = keep["raw"]   # (the forward call above wrote raw, as it should)
    for name in keep:
        assert torch.equal(keep[name], after[name]), f"a refused call wrote {name}"
    assert float(sums.abs().sum()) == 0.0 and float(other.abs().sum()) == 0.0
    # the halves, valid, give the whole: forward + loss_nets + backward_step_nets = step_nets
    whole = State(tr.n_params, tr.n_raw, [0, 1], B)
    two = [_cfg(pair, **s) for s in LOSS_NETS[pair][:2]]
    torch.cuda.synchronize()
    tr.step_nets(*_step_args(whole, batch, B, A), two, whole.alpha(3), [whole.optim("adam", k, 3) for k in range(K)], whole.grads.data_ptr(),
                 whole.raw.data_ptr(), whole.losses.data_ptr())
    tr.read_d_raw(B, whole.d_raw.data_ptr())
    assert torch.equal(st.raw, raw_keep)
    tr.forward(st.params.data_ptr(), obs.data_ptr(), B, st.raw.data_ptr())
    tr.loss_nets(st.raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), B, A, two, st.alpha(3), st.d_raw.data_ptr(),
                 st.losses.data_ptr())
    tr.backward_step_nets(st.params.data_ptr(), st.d_raw.data_ptr(), B, [st.optim("adam", k, 3) for k in range(K)], st.grads.data_ptr())
    tr.close()
    a, b = whole.snapshot(), st.snapshot()
    for name in a:
        assert torch.equal(a[name], b[name]), f"step_nets against its parts: {name}"
    assert not torch.equal(a["params"], keep["params"])
