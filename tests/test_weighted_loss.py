"""GPU: the population trainer's weighted losses (include/azgym_train_weighted.h; PopulationTrainer.update / train_epoch /
train_epoch_ring with weights) -- weights of 1 against the unweighted calls bit for bit, d_raw and the losses against float64
population_loss(weights=) with float32 PyTorch as the yardstick, determinism and population invariance, the weighted epoch against
the loop of weighted steps with hand-gathered weights, the LayerNorm and wide handles, the ABI's refusals, the Python layer on a tiny
prioritised ring and the examples.  Inputs: tests/device_loss_util.py; weights and truth: tests/is_weights_util.py."""
import os
import sys

import numpy as np
import pytest
import torch

import is_weights_util as W
import trainer_util as TU
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.losses import A0CLossTuned
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from device_loss_util import HEADS, LOG_ALPHA0, alpha_tensors, kernel_loss, make_head, make_inputs, make_loss, make_trainer, ulp32
from trainer_util import DEV

pytestmark = pytest.mark.gpu

CASES = [(h, "alphazero") for h in ("discrete2", "discrete3")] + [(h, l) for h in HEADS for l in ("a0c", "a0c_tuned")]
MAX_BATCH = 320
IN_DIM = 3


def _alpha_state(loss_name, K, step=0):
    if loss_name != "a0c_tuned":
        return None, ()
    la, m, v = alpha_tensors(K)
    return _capi.alpha_state(step, la.data_ptr(), m.data_ptr(), v.data_ptr()), (la, m, v)


# ------------------------------------------------------------------------------------------------ ones give the unweighted bits

@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head,loss_name", CASES, ids=lambda v: str(v))
def test_ones_give_the_unweighted_loss_bits(head, loss_name, reduction):
    """loss_weighted with weights of 1.0f against loss at B in {1, 17, 300} (300 crosses the kernel's 256-row stride), K = 3,
    max_batch 320: d_raw, losses and the alpha state hold the same bits."""
    K = 3
    policy, tr = make_trainer(head, K, MAX_BATCH)
    cfg = _capi.loss_cfg(policy, make_loss(loss_name, reduction, clip=0.5))
    for B in (1, 17, 300):
        inputs = make_inputs(head, K, B, 4000 + B)
        st, plain_alpha = _alpha_state(loss_name, K)
        want = kernel_loss(tr, cfg, inputs, st)
        st, ones_alpha = _alpha_state(loss_name, K)
        got = W.kernel_loss_weighted(tr, cfg, inputs, torch.ones((K, B)), st)
        assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
        for a, b, name in zip(want, got, ("losses", "d_raw")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"B = {B}: {name}"
        for a, b, name in zip(plain_alpha, ones_alpha, ("log_alpha", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a, b), f"B = {B}: {name}"
        if plain_alpha:
            assert not torch.equal(plain_alpha[0].cpu(), torch.tensor(LOG_ALPHA0[:K]))
    tr.close()


# ------------------------------------------------------------------------------------------------ a population at the raw ABI

class Pop:
    """K nets of one shape with Adam state, a tuned alpha's state and a native trainer of ``kind``: what the step and epoch calls
    change, and the calls in their four forms (weighted or not, shared settings or one entry per net)."""

    def __init__(self, policy, head, K, max_batch, kind=None, losses=None, lrs=None, reduction="mean", seed=0):
        self.policy, self.head, self.K = policy, head, K
        self.A = HEADS[head][2]
        self.tr = TU.trainer(_capi.policy_tensors(policy)[0], K, max_batch, kind)
        g = torch.Generator().manual_seed(seed)
        self.params = (0.1 * torch.randn((K, self.tr.n_params), generator=g)).to(DEV)
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.norms = torch.zeros(K, device=DEV)
        self.la, self.am, self.av = alpha_tensors(K)
        self.losses = losses or [make_loss("a0c_tuned", reduction, clip=0.5)] * K
        self.cfgs = [_capi.loss_cfg(policy, l) for l in self.losses]
        self.lrs = lrs or [1e-3] * K

    def optim(self, k, step):
        return _capi.optim("adam", self.lrs[k], self.v.data_ptr(), self.m.data_ptr(), eps=1e-7, betas=(0.9, 0.99), weight_decay=1e-4,
                           grad_clip=0.05, step=step, grad_norms=self.norms.data_ptr())

    def alpha(self, step):
        return _capi.alpha_state(step, self.la.data_ptr(), self.am.data_ptr(), self.av.data_ptr())

    def state(self):
        torch.cuda.synchronize()
        names = ("params", "m", "v", "norms", "la", "am", "av")
        return {n: getattr(self, n).detach().cpu().clone() for n in names}

    def step(self, obs, actions, counts, values, weights, step, nets=False):
        """One step; weights None: the unweighted call.  Returns (losses [K, 5], raw [K, B, NO]) on the CPU."""
        K, B = obs.shape[:2]
        t = [x.to(DEV).contiguous() for x in (obs, actions, counts, values)]
        raw = torch.full((K, B, self.tr.n_raw), float("nan"), device=DEV)
        losses = torch.full((K, 5), float("nan"), device=DEV)
        cfg = self.cfgs if nets else self.cfgs[0]
        opt = [self.optim(k, step) for k in range(K)] if nets else self.optim(0, step)
        head = [self.params.data_ptr()] + [x.data_ptr() for x in t]
        tail = [B, self.A, cfg, self.alpha(step), opt, None, raw.data_ptr(), losses.data_ptr()]
        torch.cuda.synchronize()
        if weights is None:
            (self.tr.step_nets if nets else self.tr.step_opt)(*head, *tail)
        else:
            w = weights.to(DEV).contiguous()
            (self.tr.step_nets_weighted if nets else self.tr.step_opt_weighted)(*head, w.data_ptr(), *tail)
        return losses.cpu(), raw.cpu()

    def epoch(self, where, weights, order, batch, nets=False):
        """One epoch from step 0; weights: a device tensor addressed like the rows, or None.  Returns loss_sums [K, 5] float64."""
        sums = torch.full((self.K, 5), float("nan"), dtype=torch.float64, device=DEV)
        cfg = self.cfgs if nets else self.cfgs[0]
        opt = [self.optim(k, 0) for k in range(self.K)] if nets else self.optim(0, 0)
        torch.cuda.synchronize()
        if weights is None:
            n = (self.tr.epoch_nets if nets else self.tr.epoch_opt)(self.params.data_ptr(), where, order, batch, cfg, self.alpha(0), opt,
                                                                   sums.data_ptr())
        else:
            n = (self.tr.epoch_nets_weighted if nets else self.tr.epoch_opt_weighted)(self.params.data_ptr(), where, weights.data_ptr(), order,
                                                                                     batch, cfg, self.alpha(0), opt, sums.data_ptr())
        return sums.cpu(), n

    def d_raw(self, B):
        d = torch.empty((self.K, B, self.tr.n_raw), device=DEV)
        self.tr.read_d_raw(B, d.data_ptr())
        return d.cpu()

    def close(self):
        self.tr.close()


def _same(a, b, what):
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), f"{what}: {name} differs"


def _step_inputs(head, K, B, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((K, B, IN_DIM), generator=g)
    _, actions, counts, values = make_inputs(head, K, B, seed + 1)
    return obs, actions, counts, values


def _per_net_settings(K, reduction="mean"):
    """Distinct numeric loss and optimiser settings per net; class, reduction and the rest shared."""
    losses = [A0CLossTuned(action_dim=1, alpha_init=1.0, lr=1e-3 * (k + 1), tau=0.1 + 0.05 * k, policy_coeff=0.1 * (k + 1),
                           value_coeff=1.0 - 0.1 * k, reduction=reduction, grad_clip=0.5, device="cpu") for k in range(K)]
    return losses, [1e-3 * (1 + 0.5 * k) for k in range(K)]


@pytest.mark.parametrize("nets", [False, True], ids=["opt", "nets"])
def test_ones_give_the_unweighted_step_and_epoch_bits(nets):
    """step_opt_weighted / step_nets_weighted and epoch_opt_weighted / epoch_nets_weighted with weights of 1 against their namesakes
    from identical states: parameters, Adam state, gradient norms, the alpha state, raw, d_raw, losses and loss sums."""
    head, K, B, n, batch = "gmm2", 3, 17, 2 * 16 + 3, 16
    losses, lrs = _per_net_settings(K) if nets else (None, None)
    a, b = (Pop(make_head(head), head, K, 64, losses=losses, lrs=lrs) for _ in range(2))
    inputs = _step_inputs(head, K, B, 10)
    want = a.step(*inputs, None, 0, nets=nets)
    got = b.step(*inputs, torch.ones((K, B)), 0, nets=nets)
    for x, y, name in zip(want, got, ("losses", "raw")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert torch.equal(a.d_raw(B).view(torch.int32), b.d_raw(B).view(torch.int32))
    _same(a.state(), b.state(), "step")
    for p in (a, b):
        p.close()
    a, b = (Pop(make_head(head), head, K, 64, losses=losses, lrs=lrs) for _ in range(2))
    rows, _ = _plain_rows(head, K, n, 20)
    where = _capi.epoch_rows(rows.data_ptr(), IN_DIM, a.A, n)
    order = np.stack([np.random.RandomState(60 + k).permutation(n) for k in range(K)]).astype(np.int32)
    want, n_a = a.epoch(where, None, order, batch, nets=nets)
    got, n_b = b.epoch(where, torch.ones((K, n), device=DEV), order, batch, nets=nets)
    assert n_a == n_b == 2 and torch.equal(want.view(torch.int64), got.view(torch.int64)) and torch.isfinite(want[:, :4]).all()
    _same(a.state(), b.state(), "epoch")
    start = Pop(make_head(head), head, K, 64, losses=losses, lrs=lrs)
    assert not torch.equal(a.state()["params"], start.state()["params"])
    for p in (a, b, start):
        p.close()


# ------------------------------------------------------------------------------------------------ against float64

def _hold_to_truth(tag, policy, loss, inputs, w, got, d_raw, K, fails):
    """The rule of tests/test_population_device_loss.py: per net and key the kernel's error may be at most 4 x the float32 PyTorch
    yardstick's plus one float32 ulp, on d_raw (relative to max|truth|) and on every loss slot."""
    tuned = type(loss) is A0CLossTuned
    la64 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float64, requires_grad=True) if tuned else None
    la32 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float32, requires_grad=True) if tuned else None
    truth, g64 = W.torch_loss_weighted(policy, loss, inputs, w, torch.float64, la64)
    yard, g32 = W.torch_loss_weighted(policy, loss, inputs, w, torch.float32, la32)
    for k in range(K):
        scale = float(g64[k].abs().max())
        e_y = float((g32[k].double() - g64[k]).abs().max()) / scale
        e_k = float((d_raw[k].double() - g64[k]).abs().max()) / scale
        print(f"weighted loss {tag} net {k} d_raw: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
        if not e_k <= 4 * e_y + ulp32(scale) / scale:
            fails.append((tag, "d_raw", k, e_y, e_k))
        for slot, key in enumerate(_capi.LOSS_KEYS):
            if key not in truth:
                assert float(got[k, slot]) == 0.0, (key, k)
                continue
            t = float(truth[key][k])
            e_y, e_k = abs(float(yard[key][k]) - t), abs(float(got[k, slot]) - t)
            print(f"weighted loss {tag} net {k} {key}: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
            if not e_k <= 4 * e_y + ulp32(t):
                fails.append((tag, key, k, e_y, e_k))
    return g64


@pytest.mark.parametrize("B", [17, 300])
@pytest.mark.parametrize("head,loss_name", CASES, ids=lambda v: str(v))
def test_weighted_d_raw_and_losses_against_autograd(head, loss_name, B):
    """Truth: population_loss(weights=w) in float64 on the CPU; yardstick: the same in float32; both reductions.  Weights uniform in
    (0, 1] with some rows exactly 0 and some exactly 1.  Zero-weight rows have d_raw exactly +-0; the clamp-gated log_std elements are
    exactly 0 where autograd's are."""
    K = 3
    policy, tr = make_trainer(head, K, MAX_BATCH)
    inputs = make_inputs(head, K, B, 5000 + B)
    w = W.make_weights(K, B, 6000 + B)
    assert (w == 0).any() and (w == 1).any() and ((w > 0) & (w < 1)).any()
    fails = []
    for reduction in ("mean", "sum"):
        loss = make_loss(loss_name, reduction)
        st, _ = _alpha_state(loss_name, K)
        got, d_raw = W.kernel_loss_weighted(tr, _capi.loss_cfg(policy, loss), inputs, w, st)
        g64 = _hold_to_truth(f"{head} {loss_name} {reduction} B={B}", policy, loss, inputs, w, got, d_raw, K, fails)
        assert bool((d_raw[w == 0] == 0).all()) and bool((d_raw[w != 0] != 0).any())
        kind, n, _ = HEADS[head]
        if kind != "discrete":
            cols = slice(2, 3) if kind == "normal" else slice(1 + n, 1 + 2 * n)
            ls = inputs[0][..., cols]
            gated = (ls < policy.log_param_min) | (ls > policy.log_param_max)
            assert gated.any() and not gated.all()
            assert bool((g64[..., cols][gated] == 0).all()) and bool((d_raw[..., cols][gated] == 0).all())
            assert torch.equal(d_raw[..., cols] == 0, g64[..., cols].float() == 0)
    tr.close()
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ determinism, population invariance

@pytest.mark.parametrize("head", ["gmm2", "discrete3"])
def test_determinism_and_population_invariance(head):
    """Two K = 5 weighted calls give the same bits; net k equals a K = 1 call on net k's slices and weights."""
    K, B = 5, 300
    policy, tr = make_trainer(head, K, MAX_BATCH)
    cfg = _capi.loss_cfg(policy, make_loss("a0c_tuned", "mean", clip=0.5))
    inputs, w = make_inputs(head, K, B, 7000), W.make_weights(K, B, 7001)
    runs = []
    for _ in range(2):
        st, alpha = _alpha_state("a0c_tuned", K)
        losses, d_raw = W.kernel_loss_weighted(tr, cfg, inputs, w, st)
        runs.append((d_raw, losses) + tuple(t.cpu() for t in alpha))
    tr.close()
    names = ("d_raw", "losses", "log_alpha", "exp_avg", "exp_avg_sq")
    for a, b, name in zip(runs[0], runs[1], names):
        assert torch.equal(a, b), f"{name}: two runs differ"
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    _, tr1 = make_trainer(head, 1, MAX_BATCH)
    for k in range(K):
        la, m, v = (t[k:k + 1].clone() for t in alpha_tensors(K))
        st = _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr())
        losses, d_raw = W.kernel_loss_weighted(tr1, cfg, tuple(x[k:k + 1] for x in inputs), w[k:k + 1], st)
        for a, b, name in zip(runs[0], (d_raw, losses, la.cpu(), m.cpu(), v.cpu()), names):
            assert torch.equal(a[k], b[0]), f"{name} of net {k}: K = 5 and K = 1 differ"
    tr1.close()


def test_per_net_settings_are_the_one_net_calls():
    """loss_nets_weighted and step_nets_weighted with distinct settings per net: net k has the bits of a one-net trainer's
    loss_weighted / step_opt_weighted with entry k on net k's slices and weights."""
    head, K, B = "gmm2", 3, 33
    policy = make_head(head)
    losses, lrs = _per_net_settings(K)
    cfgs = [_capi.loss_cfg(policy, l) for l in losses]
    assert len({bytes(c) for c in cfgs}) == K
    _, tr = make_trainer(head, K, 64)
    inputs, w = make_inputs(head, K, B, 8000), W.make_weights(K, B, 8001)
    st, alpha = _alpha_state("a0c_tuned", K)
    got = W.kernel_loss_weighted(tr, cfgs, inputs, w, st, nets=True)
    tr.close()
    _, tr1 = make_trainer(head, 1, 64)
    for k in range(K):
        la, m, v = (t[k:k + 1].clone() for t in alpha_tensors(K))
        one = W.kernel_loss_weighted(tr1, cfgs[k], tuple(x[k:k + 1] for x in inputs), w[k:k + 1],
                                     _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()))
        assert torch.equal(got[0][k], one[0][0]) and torch.equal(got[1][k], one[1][0]), f"net {k}"
        assert torch.equal(alpha[0][k:k + 1], la) and torch.equal(alpha[1][k:k + 1], m) and torch.equal(alpha[2][k:k + 1], v)
    tr1.close()
    pop = Pop(policy, head, K, 64, losses=losses, lrs=lrs)
    inputs = _step_inputs(head, K, B, 8100)
    start = pop.state()
    pop_losses, pop_raw = pop.step(*inputs, w, 0, nets=True)
    state = pop.state()
    pop.close()
    for k in range(K):
        one = Pop(policy, head, 1, 64, losses=[losses[k]], lrs=[lrs[k]])
        for name in ("params", "la"):
            getattr(one, name).copy_(start[name][k:k + 1])
        l1, r1 = one.step(*(x[k:k + 1] for x in inputs), w[k:k + 1], 0)
        assert torch.equal(pop_losses[k], l1[0]) and torch.equal(pop_raw[k], r1[0]), f"net {k}"
        for name, t in one.state().items():
            assert torch.equal(state[name][k:k + 1], t), f"net {k}: {name}"
        one.close()


# ------------------------------------------------------------------------------------------------ the epoch

def _plain_rows(head, K, n, seed):
    """([K, n, row] rows on the device: obs | actions | counts | Q | V, the pieces on the CPU)."""
    obs, actions, counts, values = _step_inputs(head, K, n, seed)
    rows = torch.cat([obs, actions, counts, torch.zeros_like(actions), values.unsqueeze(-1)], dim=-1).to(DEV).contiguous()
    return rows, (obs, actions, counts, values)


def _loop_of_steps(pop, pieces, weights_of_net, order, batch, nets=False):
    """The epoch's minibatches passed one by one to the weighted step, the weights gathered by hand; the float64 loss sums."""
    obs, actions, counts, values = pieces
    K, n_order = order.shape
    sums = torch.zeros((K, 5), dtype=torch.float64)
    idx = torch.from_numpy(order.astype(np.int64))
    net = torch.arange(K)[:, None]
    i, m = 0, 0
    while i < n_order:
        j = n_order if i + 2 * batch > n_order else i + batch
        pick = idx[:, i:j]
        losses, _ = pop.step(obs[net, pick], actions[net, pick], counts[net, pick], values[net, pick], weights_of_net[net, pick], m, nets=nets)
        sums = sums + losses.double()
        i, m = j, m + 1
    return sums, m


@pytest.mark.parametrize("nets", [False, True], ids=["opt", "nets"])
@pytest.mark.parametrize("layout", ["plain", "ring"])
def test_weighted_epoch_equals_the_loop_of_weighted_steps(layout, nets):
    """epoch_opt_weighted (and _nets_weighted) over a plain [K][n] weight array, and over a ring-shaped one ([slots][games], group =
    T < n_trees), with a remainder minibatch (n_order = 2 * batch + 3), Adam and a clip: parameters, Adam state, alpha state and the
    loss sums are those of the weighted steps.  The weights differ per (slot, game), so a wrong gather address shows."""
    head, K, batch = "gmm2", 3, 16
    n_order = 2 * batch + 3
    A = HEADS[head][2]
    losses, lrs = _per_net_settings(K) if nets else (None, None)
    ep, loop = (Pop(make_head(head), head, K, 64, losses=losses, lrs=lrs) for _ in range(2))
    if layout == "plain":
        n = 41
        rows, pieces = _plain_rows(head, K, n, 30)
        where = _capi.epoch_rows(rows.data_ptr(), IN_DIM, A, n)
        w_net = (1.0 + torch.arange(K * n, dtype=torch.float32).reshape(K, n)) / (K * n)
        w_dev = w_net.to(DEV).contiguous()
    else:
        T, slots = 4, 11
        G, n = K * T, slots * T
        flat_rows, flat_pieces = _plain_rows(head, 1, slots * G, 31)
        rows = flat_rows.reshape(slots, G, -1).contiguous()
        where = _capi.epoch_rows(rows.data_ptr(), IN_DIM, A, n, ring_trees=G, games_per_net=T)
        w_ring = (1.0 + torch.arange(slots * G, dtype=torch.float32).reshape(slots, G)) / (slots * G)

        def per_net(x):   # [1, slots * G, ...] -> [K, n, ...]: net k's row i is slot i // T, game k * T + i % T
            x = x.reshape((slots, K, T) + x.shape[2:])
            return x.transpose(0, 1).reshape((K, n) + x.shape[3:]).contiguous()
        pieces = tuple(per_net(p) for p in flat_pieces)
        w_net = per_net(w_ring.reshape(1, slots * G))
        w_dev = w_ring.to(DEV).contiguous()
    assert len(np.unique(w_net.numpy())) == w_net.numel()
    order = np.stack([np.random.RandomState(70 + k).randint(0, n, n_order) for k in range(K)]).astype(np.int32)
    got, n_mb = ep.epoch(where, w_dev, order, batch, nets=nets)
    want, m = _loop_of_steps(loop, pieces, w_net, order, batch, nets=nets)
    assert n_mb == m == 2
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (got, want)
    _same(ep.state(), loop.state(), f"{layout} epoch")
    # ... and the weights matter: the unweighted epoch from the same start ends elsewhere
    plain = Pop(make_head(head), head, K, 64, losses=losses, lrs=lrs)
    plain.epoch(where, None, order, batch, nets=nets)
    assert not torch.equal(plain.state()["params"], ep.state()["params"])
    for p in (ep, loop, plain):
        p.close()


# ------------------------------------------------------------------------------------------------ the other handles

@pytest.mark.parametrize("kind,hidden", [("layernorm", [32, 16]), ("wide", [512]), ("wide_layernorm", [512])])
def test_other_handles(kind, hidden):
    """A LayerNorm handle, a wide handle (one hidden layer of 512) and a wide LayerNorm handle: the weighted step's losses and d_raw
    against the float64 truth of the losses on the step's own raw output, and weights of 1 against the unweighted step's bits."""
    head, K, B = "normal", 2, 33
    policy = TU.policy(IN_DIM, hidden, ("normal",), "elu", 5, layernorm=TU.has_layernorm(kind))
    inputs = _step_inputs(head, K, B, 9000)
    w = W.make_weights(K, B, 9001)
    a, b, c = (Pop(policy, head, K, 64, kind=kind) for _ in range(3))
    got, raw = a.step(*inputs, w, 0)
    fails = []
    _hold_to_truth(f"{kind} step", policy, a.losses[0], (raw,) + tuple(inputs[1:]), w, got, a.d_raw(B), K, fails)
    assert not fails, fails
    assert bool((a.d_raw(B)[w == 0] == 0).all())
    want = b.step(*inputs, None, 0)
    ones = c.step(*inputs, torch.ones((K, B)), 0)
    for x, y, name in zip(want, ones, ("losses", "raw")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    _same(b.state(), c.state(), f"{kind}: ones")
    assert not torch.equal(a.state()["params"], b.state()["params"])
    for p in (a, b, c):
        p.close()


# ------------------------------------------------------------------------------------------------ the ABI

def test_abi_refusals_write_nothing():
    """NULL weights: AZG_E_INVALID from all six entry points with nothing written (outputs pre-filled with NaN stay NaN, parameters
    and state unchanged); a refusal of the namesake (n_rows 0, a wrong struct_size) comes back with the namesake's code."""
    head, K, B, n = "gmm2", 2, 16, 24
    pop = Pop(make_head(head), head, K, 32)
    tr, A = pop.tr, pop.A
    obs, actions, counts, values = (x.to(DEV).contiguous() for x in _step_inputs(head, K, B, 40))
    raw_in = make_inputs(head, K, B, 41)[0].to(DEV).contiguous()
    w = torch.ones((K, B), device=DEV)
    raw = torch.full((K, B, tr.n_raw), float("nan"), device=DEV)
    d_raw = torch.full_like(raw, float("nan"))
    losses = torch.full((K, 5), float("nan"), device=DEV)
    sums = torch.full((K, 5), float("nan"), dtype=torch.float64, device=DEV)
    rows, _ = _plain_rows(head, K, n, 42)
    where = _capi.epoch_rows(rows.data_ptr(), IN_DIM, A, n)
    w_rows = torch.ones((K, n), device=DEV)
    order = np.stack([np.random.RandomState(k).permutation(n) for k in range(K)]).astype(np.int32)
    before = pop.state()
    cfg, cfgs, st = pop.cfgs[0], pop.cfgs, pop.alpha(0)
    opt, opts = pop.optim(0, 0), [pop.optim(k, 0) for k in range(K)]
    P, O, AC, CN, V, R, D, L, S = (t.data_ptr() for t in (pop.params, obs, actions, counts, values, raw_in, d_raw, losses, sums))
    INV = _capi.AZG_E_INVALID
    torch.cuda.synchronize()

    def code(fn, *a):
        with pytest.raises(_capi.EngineError) as ei:
            fn(*a)
        assert str(ei.value).split(": ", 1)[1]
        return ei.value.code

    def edit(obj, **kw):
        c = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    for weights, rows_n, c1 in ((None, B, cfg), (w.data_ptr(), 0, cfg), (w.data_ptr(), 33, cfg), (w.data_ptr(), B, edit(cfg, struct_size=8))):
        assert code(tr.loss_weighted, R, AC, CN, V, weights, rows_n, A, c1, st, D, L) == INV
        assert code(tr.step_opt_weighted, P, O, AC, CN, V, weights, rows_n, A, c1, st, opt, None, raw.data_ptr(), L) == INV
    assert code(tr.loss_nets_weighted, R, AC, CN, V, None, B, A, cfgs, st, D, L) == INV
    assert code(tr.step_nets_weighted, P, O, AC, CN, V, None, B, A, cfgs, st, opts, None, raw.data_ptr(), L) == INV
    assert code(tr.step_opt_weighted, P, O, AC, CN, V, w.data_ptr(), B, A, cfg, st, edit(opt, struct_size=8), None, raw.data_ptr(), L) == INV
    assert code(tr.loss_weighted, R, AC, CN, V, w.data_ptr(), B, A, edit(cfg, kind=7), st, D, L) == _capi.AZG_E_UNSUPPORTED
    assert code(tr.epoch_opt_weighted, P, where, None, order, 8, cfg, st, opt, S) == INV
    assert code(tr.epoch_nets_weighted, P, where, None, order, 8, cfgs, st, opts, S) == INV
    assert code(tr.epoch_opt_weighted, P, where, w_rows.data_ptr(), order, 0, cfg, st, opt, S) == INV
    assert code(tr.epoch_opt_weighted, P, edit(where, struct_size=8), w_rows.data_ptr(), order, 8, cfg, st, opt, S) == INV
    assert code(tr.epoch_opt_weighted, P, where, w_rows.data_ptr(), np.tile(order, (1, 2)), 64, cfg, st, opt, S) == INV   # one minibatch of 48 > max_batch
    torch.cuda.synchronize()
    for t in (raw, d_raw, losses, sums):
        assert bool(torch.isnan(t).all())
    _same(pop.state(), before, "after refusals")
    # the trainer is still usable
    assert tr.epoch_opt_weighted(P, where, w_rows.data_ptr(), order, 8, cfg, st, opt, S) == 3
    assert torch.isfinite(sums).all() and not torch.equal(pop.state()["params"], before["params"])
    pop.close()


# ------------------------------------------------------------------------------------------------ Python on a tiny ring

def _tiny(prioritized):
    K, T = 2, 4
    agents = TU.make_agents("discrete", "a0c_tuned", K)
    sp = run.PopulationSelfPlay([a.nn for a in agents], game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, epsilon=0.1,
                                capacity_steps=8, n_step=3, prioritized=prioritized)
    return agents, sp


def test_train_epoch_ring_with_the_engines_weights():
    """PopulationSelfPlay(prioritized={alpha, eps, beta}) on a tiny CartPole ring: train_epoch_ring(weights="priority") equals
    train_epoch_ring(weights=<the same array as a tensor>) bit for bit and differs from weights=None; per_net and agents' optimisers
    take the weights too; the engine's refusal surfaces when is_weights has not run."""
    K, T, steps, batch = 2, 4, 5, 8
    n = steps * T
    runs = {}
    for mode in ("priority", "tensor", None):
        agents, sp = _tiny({"alpha": 0.6, "eps": 1e-3, "beta": 0.4})
        assert sp.play_device(steps) == (steps, 0)
        tr = PopulationTrainer(agents, max_batch=64, losses="device")
        order = sp.sample_order(n)
        if mode == "priority":
            with pytest.raises(_capi.EngineError) as ei:                      # (sample_order recomputed the priorities: no weights yet)
                tr.train_epoch_ring(sp, order, batch_size=batch, weights="priority")
            assert ei.value.code == _capi.AZG_E_STATE
        assert sp.is_weights() is None
        values = sp.engine.selfplay_is_weight_values().reshape(steps, K * T)
        q = sp.engine.selfplay_priority_values().reshape(steps, K * T)
        np.testing.assert_array_equal(W.bits(values), W.bits(W.is_weights(q, K, 0.4)))
        assert len(np.unique(values)) > K
        if mode == "tensor":
            ring_w = torch.ones((8, K * T), device=DEV)
            ring_w[:steps] = torch.from_numpy(values).to(DEV)
            info = tr.train_epoch_ring(sp, order, batch_size=batch, weights=ring_w)
        else:
            info = tr.train_epoch_ring(sp, order, batch_size=batch, weights=mode)
        assert len(info) == K and all(np.isfinite(v) for i in info for v in i.values())
        runs[mode] = (order.copy(), info, TU.state_of(tr))
        if mode == "tensor":
            with pytest.raises(ValueError, match=r"\[capacity_steps, n_games\]"):
                tr.train_epoch_ring(sp, order, batch_size=batch, weights=ring_w[:steps])
        tr.close()
        sp.close()
    np.testing.assert_array_equal(runs["priority"][0], runs["tensor"][0])
    np.testing.assert_array_equal(runs["priority"][0], runs[None][0])
    assert runs["priority"][1] == runs["tensor"][1]
    TU.assert_same(runs["priority"][2], runs["tensor"][2], "priority and tensor weights")
    assert runs["priority"][1] != runs[None][1]
    assert not torch.equal(runs["priority"][2]["flat"], runs[None][2]["flat"])
    # without a beta nothing is ever computed, and is_weights says what it lacks
    agents, sp = _tiny({"alpha": 0.6, "eps": 1e-3})
    sp.play_device(steps)
    sp.sample_order(n)
    with pytest.raises(ValueError, match="needs a beta"):
        sp.is_weights()
    assert _code_of(sp.engine.selfplay_is_weight_values) == _capi.AZG_E_STATE
    sp.is_weights(1.0)
    assert sp.engine.selfplay_is_weight_values().shape == (n * K,)
    sp.close()


def _code_of(fn, *a):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a)
    return ei.value.code


@pytest.mark.parametrize("kw", [dict(), dict(optimizers="agents"), dict(optimizers="agents", per_net=True)], ids=["rmsprop", "agents", "per_net"])
def test_weighted_epochs_in_every_call_form(kw):
    """train_epoch(weights=[K, n]) in the trainer's three call forms: weights of 1 end where the unweighted epoch ends, bit for bit
    (the RMSprop family has no weighted form: its trainer goes through *_opt_weighted), other weights end elsewhere, and the
    epoch equals train_on_rows-style updates with the gathered weights."""
    head, loss, K, n, batch = "gmm2", "a0c_tuned", 3, 35, 16
    S, A = TU.DIMS[head]
    rows = TU.make_rows(head, K, n, 600)
    seeds = [5, 6, 7]
    w = W.make_weights(K, n, 601)
    ends = {}
    for name, weights in (("none", None), ("ones", torch.ones((K, n))), ("w", w)):
        tr = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=64, losses="device", **kw)
        info = tr.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds, weights=weights)
        ends[name] = (info, tr.flat.detach().cpu().clone(), tr.log_alpha.detach().cpu().clone())
        tr.close()
    assert ends["none"][0] == ends["ones"][0]
    assert torch.equal(ends["none"][1], ends["ones"][1]) and torch.equal(ends["none"][2], ends["ones"][2])
    assert not torch.equal(ends["none"][1], ends["w"][1])
    # the loop of update(weights=) calls over the same minibatches
    tr = PopulationTrainer(TU.make_agents(head, loss, K), max_batch=64, losses="device", **kw)
    order = torch.from_numpy(np.stack([np.random.RandomState(s).permutation(n) for s in seeds])).to(DEV)
    net = torch.arange(K, device=DEV)[:, None]
    i = 0
    while i < n:
        j = n if i + 2 * batch > n else i + batch
        b = rows[net, order[:, i:j]]
        tr.update(TU.split_rows(b, S, A), weights=w.to(DEV)[net, order[:, i:j]])
        i = j
    assert torch.equal(tr.flat.detach().cpu(), ends["w"][1]) and torch.equal(tr.log_alpha.detach().cpu(), ends["w"][2])
    tr.close()


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_weighted_update_against_the_torch_path(kind):
    """update(weights=) with losses="device" against the losses="torch" path from the same nets, in test_end_to_end_update's bound:
    per net, the device-loss parameters' largest distance from a float64 step of the same weighted loss may be at most 4 x that of
    the losses="torch" ones."""
    K = 4
    cfg, agents = TU.e2e_agents(kind, K)
    others = [TU.twin(kind, cfg, a, DEV) for a in agents]
    m = cfg["mcts"]
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=8, n_rollouts=m["n_rollouts"], c_uct=m["c_uct"],
                                gamma=m["gamma"], epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5),
                                capacity_steps=8)
    rows = sp.collect_device(8)
    S, A = sp.engine.s_obs, sp.engine.kmax
    sp.close()
    batches = TU.batches(rows, S, A)
    B = batches[0][0].shape[0]
    w = W.make_weights(K, B, 11)
    p64 = torch.stack([_weighted_step_f64(kind, cfg, a, b, w[k]) for k, (a, b) in enumerate(zip(agents, batches))])
    before = torch.from_numpy(np.stack([_capi.policy_blob(a.nn)[1] for a in agents])).double()
    tr = PopulationTrainer(agents, losses="device")
    got = tr.update(batches, weights=w)
    tt = PopulationTrainer(others, losses="torch")
    want = tt.update(batches, weights=w)
    assert [set(g) for g in got] == [set(x) for x in want]
    p_dev, p_torch = tr.flat.cpu().double(), tt.flat.cpu().double()
    assert not torch.equal(p_dev, before)
    for k in range(K):
        e_t, e_d = float((p_torch[k] - p64[k]).abs().max()), float((p_dev[k] - p64[k]).abs().max())
        print(f"weighted update {kind} net {k}: parameters against a float64 step, losses='torch' {e_t:.3g}, losses='device' {e_d:.3g}")
        assert e_d <= 4 * e_t
    assert bool((tr.last_d_raw.cpu()[w == 0] == 0).all()) and bool((tt.last_d_raw.cpu()[w == 0] == 0).all())
    tt.close()
    tr.close()


def _weighted_step_f64(kind, cfg, agent, batch, w):
    """The agent's whole optimiser step on the weighted loss in float64 on the CPU (population_loss with K = 1 on the agent's own
    raw output): the parameters after it, in blob order."""
    from alphazero_gym_amd.agent.population_trainer import population_loss
    a = TU.twin(kind, cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    a.optimizer.zero_grad(set_to_none=True)
    raw = TU.raw_of(a.nn, s).unsqueeze(0)
    la = a.loss.log_alpha.detach().double().reshape(1) if hasattr(a.loss, "log_alpha") else None
    out = population_loss(a.nn, a.loss, raw, ac.reshape(1, s.shape[0], -1), c.reshape(1, s.shape[0], -1), v.reshape(1, -1, 1), la,
                          weights=w.double().reshape(1, -1))
    out["loss"].sum().backward()
    if a.clip:
        torch.nn.utils.clip_grad_norm_(a.nn.parameters(), a.clip)
    a.optimizer.step()
    return torch.cat([t.detach().reshape(-1) for t in _capi.policy_tensors(a.nn)[1]])


# ------------------------------------------------------------------------------------------------ the examples

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device-epoch"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--trainer", "device"])])
def test_examples_train_with_importance_weights(example, extra):
    """--prioritized-alpha 0.6 --prioritized-beta 0.4 --n-step 3: a short session runs to completion on finite losses, and differs
    from the session without the weights; --prioritized-beta without --prioritized-alpha is refused, and so is the population
    example's per-agent --trainer torch, whose update loop takes no weights."""
    import importlib
    mod = importlib.import_module(example)
    common = ["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "3", "--steps-per-iter", "2", "--replay-steps", "4",
              "--reanalyse-slots", "1", "--hidden", "16", "16", "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5",
              "--device", "cuda", "--n-step", "3"] + extra
    a = mod.parse_args(common + ["--prioritized-alpha", "0.6", "--prioritized-beta", "0.4"])
    assert (a.prioritized_alpha, a.prioritized_beta) == (0.6, 0.4)
    hist = mod.train(a, log=None)
    assert len(hist) == 3 and np.isfinite(np.asarray([h["loss"] for h in hist], np.float64)).all()
    plain = mod.train(mod.parse_args(common + ["--prioritized-alpha", "0.6"]), log=None)
    assert [h["loss"] for h in hist] != [h["loss"] for h in plain]
    with pytest.raises(SystemExit):
        mod.parse_args(common + ["--prioritized-beta", "0.4"])
    with pytest.raises(SystemExit):
        mod.parse_args(common + ["--prioritized-alpha", "0.6", "--prioritized-beta", "-1"])
    if "--trainer" in extra:
        with pytest.raises(SystemExit):
            mod.parse_args(common[:-2] + ["--trainer", "torch", "--prioritized-alpha", "0.6", "--prioritized-beta", "0.4"])
