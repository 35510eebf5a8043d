"""GPU: the wide population trainer (azg_trainer_create_wide, PopulationTrainer(wide=True)): nets of up to 8 hidden layers and widths
up to 1024, a launch per layer.  Where the first trainer takes the shape too, the wide one must give its bits; on the wide shapes:
population invariance and repeatability bit for bit in both backward forms, gradients against float64 autograd with float32 autograd
as the yardstick, the forward pass against the engine, the optimiser steps given the gradient, the end-to-end update with the epoch on
the self-play ring and the hand-off to the search, the ABI's errors and the example."""
import copy
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.losses import A0CLossTuned, AlphaZeroLoss
from alphazero_gym_amd.network.policies import make_policy

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

DEV = "cuda"
U = 2.0 ** -24
OPT = dict(lr=1e-3, alpha=0.9, eps=1e-10)
ADAM = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-7)   # the reference's Adam settings

# (in_dim, hidden, head, activation).  The overlap: test_population_trainer.py's five shapes, which both trainers take.
NARROW = [
    (2, [16], ("normal",), "elu"),
    (4, [128, 128], ("discrete", 2), "relu"),
    (3, [128, 128, 128], ("gmm", 2), "elu"),
    (6, [256, 16], ("discrete", 3), "relu"),
    (3, [256, 256, 256], ("normal",), "elu"),
]
# The wide shapes: the shape test_abi_errors proves refused without the opt-in; four layers of 17, 33 and 20 tiles (strips of 1 and 4
# tiles); the widest k chain; the full depth.
W1 = (4, [512], ("discrete", 2), "relu")
W2 = (3, [272, 528, 272, 320], ("gmm", 2), "elu")
W3 = (6, [1024, 1024], ("normal",), "elu")
W4 = (4, [64] * 8, ("discrete", 3), "silu")
WIDE = [W1, W2, W3, W4]


def _id(s):
    return f"{s[0]}in_{'x'.join(map(str, s[1]))}_{'_'.join(map(str, s[2]))}" if isinstance(s, tuple) else str(s)


def _native():
    from alphazero_gym_amd import _native as N
    N.lib()
    return N


def _trainer(desc, K, max_batch, wide):
    N = _native()
    return N.HipTrainer(desc, K, max_batch, wide=True) if wide else N.HipTrainer(desc, K, max_batch)


def _policy(in_dim, hidden, head, act, seed):
    """head: ("discrete", n_actions) | ("normal",) | ("gmm", components)"""
    torch.manual_seed(seed)
    if head[0] == "discrete":
        return make_policy(in_dim, 1, "discrete", list(hidden), act, num_actions=head[1])
    return make_policy(in_dim, 1, "normal", list(hidden), act, num_components=1 if head[0] == "normal" else head[1], action_bound=2.0)


@functools.lru_cache(maxsize=None)
def _policies(shape_key, K, first_seed):
    """K policies of one shape, built once per module run and never changed (the trainers work on copies of their blobs)."""
    in_dim, hidden, head, act = shape_key
    return tuple(_policy(in_dim, list(hidden), head, act, first_seed + k) for k in range(K))


def _key(shape):
    return (shape[0], tuple(shape[1]), shape[2], shape[3])


def _flat(policies):
    return torch.from_numpy(np.stack([_capi.policy_blob(p)[1] for p in policies])).to(DEV)


def _raw_of(pol, x):
    h = pol.trunk(x)
    return torch.cat([pol.value_head(h), pol.dist_head(h)], dim=-1)


def _data(K, B, in_dim, n_raw, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((K, B, in_dim), generator=g)
    d_raw = torch.randn((K, B, n_raw), generator=g) / B
    return obs, d_raw


def _forward(tr, params, obs):
    K, B = obs.shape[:2]
    raw = torch.empty((K, B, tr.n_raw), device=DEV)
    torch.cuda.synchronize()
    tr.forward(params.data_ptr(), obs.data_ptr(), B, raw.data_ptr())
    return raw


def _step(tr, params, obs, d_raw, opt, sq):
    """One forward + backward/optimiser step: (raw, grads); params and sq are updated in place."""
    raw = _forward(tr, params, obs)
    grads = torch.zeros_like(params)
    tr.backward_step(params.data_ptr(), d_raw.data_ptr(), obs.shape[1], opt, sq.data_ptr(), grads.data_ptr())
    return raw, grads


def _step_opt(tr, params, obs, d_raw, make_opt):
    """forward + backward_step_opt; make_opt(grad_norms address) -> azg_optim.  Returns (grads, grad_norms)."""
    K, B = obs.shape[:2]
    _forward(tr, params, obs)
    grads, norms = torch.zeros_like(params), torch.full((K,), -1.0, device=DEV)
    tr.backward_step_opt(params.data_ptr(), d_raw.data_ptr(), B, make_opt(norms.data_ptr()), grads.data_ptr())
    return grads, norms


FUSED_NAMES = ("raw", "grads", "params", "square_avg")
ADAM_NAMES = ("grads", "params", "exp_avg", "exp_avg_sq", "grad_norms")


def _run_fused(tr, pols, obs, d_raw):
    """forward + backward_step (RMSprop, weight decay, square_avg 0.25) from the policies' weights: CPU copies, FUSED_NAMES' order."""
    params, sq = _flat(pols), torch.full((len(pols), tr.n_params), 0.25, device=DEV)
    raw, grads = _step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=1e-4, **OPT), sq)
    return [t.cpu() for t in (raw, grads, params, sq)]


def _run_adam(tr, pols, obs, d_raw):
    """forward + backward_step_opt (Adam, grad_clip 0.5, step 3, grad_norms): CPU copies, ADAM_NAMES' order."""
    n = len(pols)
    params = _flat(pols)
    m, v = torch.full((n, tr.n_params), 0.01, device=DEV), torch.full((n, tr.n_params), 0.25, device=DEV)
    grads, norms = _step_opt(tr, params, obs, d_raw, lambda nn: _capi.optim("adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"],
                                                                           betas=ADAM["betas"], weight_decay=1e-4, grad_clip=0.5, step=3,
                                                                           grad_norms=nn))
    return [t.cpu() for t in (grads, params, m, v, norms)]


# ------------------------------------------------------------------------------------------------ 1. the overlap, bit for bit
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_overlap_bit_for_bit(shape, B):
    """A wide trainer and an azg_trainer_create trainer on the same inputs: forward + backward_step, and forward + backward_step_opt
    with Adam, a clip and grad_norms, give the same bits."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(_key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    got = {}
    for wide in (False, True):
        tr = _trainer(desc, K, 512, wide)
        got[wide] = (_run_fused(tr, pols, obs, d_raw), _run_adam(tr, pols, obs, d_raw))
        tr.close()
    start = _flat(pols).cpu()
    for form, names in ((0, FUSED_NAMES), (1, ADAM_NAMES)):
        for a, b, name in zip(got[False][form], got[True][form], names):
            assert torch.equal(a, b), f"{name} ({'fused' if form == 0 else 'adam'}): the wide trainer's bits differ"
        moved = got[True][form][names.index("params")]
        assert torch.isfinite(moved).all() and not torch.equal(moved, start)
    assert bool((got[True][1][4] > 0).all())


LOSS_CASES = [(NARROW[2], "a0c_tuned"), (NARROW[1], "alphazero")]


def _loss_inputs(head, K, B, seed):
    """(actions [K, B, A], counts [K, B, A], values [K, B]) as test_population_device_loss.py's make_inputs draws them."""
    g = torch.Generator().manual_seed(seed)
    if head[0] == "discrete":
        A = head[1]
        actions = torch.arange(A, dtype=torch.float32).repeat(K, B, 1)
        counts = torch.randint(0, 9, (K, B, A), generator=g).float()
    else:
        A = 5
        actions = 0.98 * 2.0 * torch.tanh(torch.randn((K, B, A), generator=g))
        extra = torch.randint(0, A, (K, B, 25 - A), generator=g)      # positive integers that sum to 25
        counts = torch.ones((K, B, A)).scatter_add_(2, extra, torch.ones(extra.shape))
    values = torch.randn((K, B), generator=g)
    return actions, counts, values


@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape,loss_name", LOSS_CASES, ids=["3x128_gmm2_a0c_tuned", "2x128_discrete2_alphazero"])
def test_overlap_step_and_epoch(shape, loss_name, B):
    """azg_trainer_step with the losses on the device, then azg_trainer_epoch over 40 rows in minibatches of 16 + 24: losses, d_raw,
    log_alpha, raw, params, square_avg and the epoch's loss sums of a wide trainer equal the first trainer's."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(_key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    if loss_name == "alphazero":
        loss = AlphaZeroLoss(policy_coeff=1.0, value_coeff=0.5, reduction="mean")
    else:
        loss = A0CLossTuned(action_dim=1, alpha_init=1.0, lr=1e-3, tau=0.1, policy_coeff=0.1, value_coeff=1.0, reduction="mean",
                            grad_clip=0.5, device="cpu")
    cfg = _capi.loss_cfg(pols[0], loss)
    obs, _ = _data(K, B, in_dim, 1, 7)
    actions, counts, values = _loss_inputs(head, K, B, 8)
    A = actions.shape[2]
    n = 40
    eobs, _ = _data(K, n, in_dim, 1, 9)
    eact, ecnt, eval_ = _loss_inputs(head, K, n, 10)
    rows = torch.cat([eobs, eact, ecnt, torch.zeros_like(eact), eval_.unsqueeze(-1)], dim=-1).to(DEV).contiguous()
    order = np.stack([np.random.RandomState(s).permutation(n) for s in (3, 1, 4)]).astype(np.int32)
    opt = _capi.rmsprop_opt(weight_decay=1e-4, **OPT)
    names = ("raw", "losses", "d_raw", "log_alpha", "params", "square_avg", "epoch sums", "params after the epoch", "log_alpha after it")
    got = {}
    for wide in (False, True):
        tr = _trainer(desc, K, 512, wide)
        params, sq = _flat(pols), torch.full((K, tr.n_params), 0.25, device=DEV)
        la = torch.tensor([float(np.log(a)) for a in (0.5, 1.0, 2.0)], device=DEV)
        m, v = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        tuned = loss_name == "a0c_tuned"
        raw, d_raw = torch.empty((K, B, tr.n_raw), device=DEV), torch.empty((K, B, tr.n_raw), device=DEV)
        table = torch.empty((K, len(_capi.LOSS_KEYS)), device=DEV)
        dev = [t.to(DEV).contiguous() for t in (obs, actions, counts, values)]
        torch.cuda.synchronize()
        tr.step(params.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), B, A, cfg,
                _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()) if tuned else None, opt, sq.data_ptr(), None,
                raw.data_ptr(), table.data_ptr())
        tr.read_d_raw(B, d_raw.data_ptr())
        out = [t.cpu().clone() for t in (raw, table, d_raw, la, params, sq)]
        sums = torch.zeros((K, len(_capi.LOSS_KEYS)), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        n_mb = tr.epoch(params.data_ptr(), _capi.epoch_rows(rows.data_ptr(), in_dim, A, n), order, 16, cfg,
                        _capi.alpha_state(1, la.data_ptr(), m.data_ptr(), v.data_ptr()) if tuned else None, opt, sq.data_ptr(),
                        sums.data_ptr())
        assert n_mb == 2
        got[wide] = out + [sums.cpu(), params.cpu(), la.cpu()]
        tr.close()
    for a, b, name in zip(got[False], got[True], names):
        assert torch.equal(a, b), f"{name}: the wide trainer's bits differ"
    assert torch.isfinite(got[True][1]).all() and torch.isfinite(got[True][6]).all()
    assert not torch.equal(got[True][4], _flat(pols).cpu()) and not torch.equal(got[True][7], got[True][4])
    if loss_name == "a0c_tuned":
        assert not torch.equal(got[True][3], torch.tensor([float(np.log(a)) for a in (0.5, 1.0, 2.0)]))


# ------------------------------------------------------------------------------------------------ 2. invariance and repeatability
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", WIDE, ids=_id)
def test_population_invariance(shape, B):
    """Net k of a K = 3 wide trainer equals a K = 1 wide trainer on net k's data and two runs of the same call are equal, bit for
    bit, in the fused and the deferred form; the two forms' gradients are equal."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(_key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    runs = []
    for _ in range(2):
        tr = _trainer(desc, K, 512, True)
        runs.append((_run_fused(tr, pols, obs, d_raw), _run_adam(tr, pols, obs, d_raw)))
        tr.close()
    for form, names in ((0, FUSED_NAMES), (1, ADAM_NAMES)):
        for a, b, name in zip(runs[0][form], runs[1][form], names):
            assert torch.equal(a, b), f"{name}: two runs differ"
    fused, adam = runs[0]
    assert torch.equal(fused[1], adam[0]), "the fused and the deferred form's gradients differ"
    start = _flat(pols).cpu()
    assert torch.isfinite(fused[1]).all() and not torch.equal(fused[2], start) and not torch.equal(adam[1], start)
    tr1 = _trainer(desc, 1, 512, True)
    for k in range(K):
        o, d = obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous()
        for a, b, name in zip(fused, _run_fused(tr1, pols[k:k + 1], o, d), FUSED_NAMES):
            assert torch.equal(a[k], b[0]), f"{name} of net {k}: K = 3 and K = 1 differ"
        for a, b, name in zip(adam, _run_adam(tr1, pols[k:k + 1], o, d), ADAM_NAMES):
            assert torch.equal(a[k], b[0]), f"{name} of net {k} (deferred): K = 3 and K = 1 differ"
    tr1.close()


# ------------------------------------------------------------------------------------------------ 3. gradients against autograd
def _autograd(pol, obs, d_raw, dtype):
    p = copy.deepcopy(pol).to(dtype)
    raw = _raw_of(p, obs.to(dtype))
    (raw * d_raw.to(dtype)).sum().backward()
    return [t.grad for t in _capi.policy_tensors(p)[1]]


GRAD_CASES = [(s, 128) for s in WIDE] + [(W2, 17)]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: _id(v))
def test_gradients_against_autograd(shape, B):
    """Truth: float64 autograd on the CPU.  Yardstick: float32 autograd on the CPU, error max|g32 - g64| / max|g64| per parameter
    tensor.  The kernel's error by the same measure may be at most 4 * sqrt(max(Hmax, 256) / 256) x that: the project's factor 4 up
    to width 256, 5.75 at 528, 8 at 1024 (an accumulator is one sequential chain whose rounding error grows with the square root of its
    length, where torch's blocked float32 sums stay flat).  B = 17: padded rows must contribute nothing."""
    in_dim, hidden, head, act = shape
    pol = _policies(_key(shape), 1, 21)[0]
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = _data(1, B, in_dim, 1 + desc.n_dist, 13)
    g64 = _autograd(pol, obs[0], d_raw[0], torch.float64)
    g32 = _autograd(pol, obs[0], d_raw[0], torch.float32)
    tr = _trainer(desc, 1, 512, True)
    params, sq = _flat([pol]), torch.zeros((1, tr.n_params), device=DEV)
    _, grads = _step(tr, params, obs.to(DEV), d_raw.to(DEV), _capi.rmsprop_opt(**OPT), sq)
    tr.close()
    grads = grads[0].cpu()
    factor = 4.0 * float(np.sqrt(max(max(hidden), 256) / 256.0))
    off, fails = 0, []
    names = [n for n, _ in pol.named_parameters()]
    for name, a64, a32 in zip(names, g64, g32):
        gk = grads[off:off + a64.numel()].view_as(a64).double()
        off += a64.numel()
        scale = a64.abs().max()
        e32, ek = float((a32.double() - a64).abs().max() / scale), float((gk - a64).abs().max() / scale)
        print(f"grad {shape} B={B} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g} (bound {factor:.3g} x)")
        if not ek <= factor * e32:
            fails.append((name, e32, ek))
    assert off == grads.numel() and not fails, fails


# ------------------------------------------------------------------------------------------------ 3b. wider strips
# The launches take strips of NT = 1, 2 or 4 tiles (dispatch_train_wide.hip: pick_nt, the widest NT with row tiles * ceil(tiles / NT)
# * K >= 2048 strips, else 1), and the cases above, K <= 3 and B <= 128, all run NT = 1.  [528, 272] has 33 and 17 tiles, so every strip
# row of 2 or 4 tiles ends in a partial strip of 1.  With 8 row tiles at B = 128 and 32 at B = 512 (forward and (a) over the layer's
# width; (b) of layer 1 over 17 row tiles x 33 tiles):
#   K = 16, B = 128: forward of layer 0 and (a) of layer 1  8 * 17 * 16 = 2176 -> NT = 2;  (b) of layer 1  17 * 9 * 16 = 2448 -> NT = 4
#   K = 16, B = 512: forward of both layers and both (a)    32 * 9 * 16, 32 * 5 * 16 -> NT = 4;  (b) of layer 1 NT = 4
#   K =  8, B = 128: (b) of layer 1  17 * 9 * 8 = 1224, 17 * 17 * 8 = 2312 -> NT = 2;  everything else NT = 1
# A K = 1 trainer runs NT = 1 everywhere at both batch sizes (at most 32 * 33 = 1056 strips).
W5 = (3, [528, 272], ("gmm", 2), "elu")


def _pick_nt(row_tiles, tiles, K):
    """pick_nt of dispatch_train_wide.hip, restated: what the cases below rely on to reach the wider strips."""
    for nt in (4, 2):
        if row_tiles * -(-tiles // nt) * K >= 2048:
            return nt
    return 1


def test_strip_rule_of_the_cases():
    """The arithmetic of the comment above (if the rule in the launch code moves, the cases below have to move with it)."""
    assert (_pick_nt(8, 33, 16), _pick_nt(8, 17, 16), _pick_nt(17, 33, 16)) == (2, 1, 4)
    assert (_pick_nt(32, 33, 16), _pick_nt(32, 17, 16)) == (4, 4)
    assert (_pick_nt(17, 33, 8), _pick_nt(8, 33, 8), _pick_nt(8, 17, 8)) == (2, 1, 1)
    assert max(_pick_nt(mt, t, 1) for mt in (8, 32, 17) for t in (33, 17)) == 1


@pytest.mark.parametrize("K,B", [(16, 128), (16, 512), (8, 128)], ids=["K16_B128", "K16_B512", "K8_B128"])
def test_wider_strips(K, B):
    """Strips of 2 and 4 tiles with a partial last strip in the forward, (a) and (b) launches: every net of the K-net trainer equals
    the K = 1 trainer (strips of one tile) on its data bit for bit, in the fused and the deferred form, and net 0's gradients pass the
    autograd check of test_gradients_against_autograd (factor 4 * sqrt(528 / 256) = 5.74)."""
    in_dim, hidden, head, act = W5
    pols = _policies(_key(W5), 16, 50)[:K]
    desc = _capi.policy_tensors(pols[0])[0]
    obs_c, d_raw_c = _data(K, B, in_dim, 1 + desc.n_dist, 7)
    obs, d_raw = obs_c.to(DEV), d_raw_c.to(DEV)
    tr = _trainer(desc, K, 512, True)
    fused, adam = _run_fused(tr, pols, obs, d_raw), _run_adam(tr, pols, obs, d_raw)
    tr.close()
    assert torch.equal(fused[1], adam[0]), "the fused and the deferred form's gradients differ"
    start = _flat(pols).cpu()
    assert torch.isfinite(fused[1]).all() and not torch.equal(fused[2], start) and not torch.equal(adam[1], start)
    tr1 = _trainer(desc, 1, 512, True)
    for k in range(K):
        o, d = obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous()
        for a, b, name in zip(fused, _run_fused(tr1, pols[k:k + 1], o, d), FUSED_NAMES):
            assert torch.equal(a[k], b[0]), f"{name} of net {k}: K = {K} and K = 1 differ"
        for a, b, name in zip(adam, _run_adam(tr1, pols[k:k + 1], o, d), ADAM_NAMES):
            assert torch.equal(a[k], b[0]), f"{name} of net {k} (deferred): K = {K} and K = 1 differ"
    tr1.close()
    g64 = _autograd(pols[0], obs_c[0], d_raw_c[0], torch.float64)
    g32 = _autograd(pols[0], obs_c[0], d_raw_c[0], torch.float32)
    factor = 4.0 * float(np.sqrt(max(max(hidden), 256) / 256.0))
    grads, off, fails = fused[1][0], 0, []
    for (name, _), a64, a32 in zip(pols[0].named_parameters(), g64, g32):
        gk = grads[off:off + a64.numel()].view_as(a64).double()
        off += a64.numel()
        scale = a64.abs().max()
        e32, ek = float((a32.double() - a64).abs().max() / scale), float((gk - a64).abs().max() / scale)
        print(f"grad {W5} K={K} B={B} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g} (bound {factor:.3g} x)")
        if not ek <= factor * e32:
            fails.append((name, e32, ek))
    assert off == grads.numel() and not fails, fails


# ------------------------------------------------------------------------------------------------ 4. forward against the engine
@pytest.mark.parametrize("shape", [W1, (3, [512, 512], ("gmm", 2), "elu")], ids=["cartpole_512", "pendulum_2x512_gmm2"])
def test_forward_against_engine(shape):
    """raw against azg_mlp_eval's raw of a single-net engine of 16 trees with the same weights (the existing test's bound: 1e-5)."""
    N = _native()
    in_dim, hidden, head, act = shape
    pol = _policies(_key(shape), 1, 3)[0]
    desc, blob = _capi.policy_blob(pol)
    if head[0] == "discrete":
        kw = dict(env_id=_capi.ENV_CARTPOLE, mode=_capi.MODE_DISCRETE, num_actions=head[1])
    else:
        kw = dict(env_id=_capi.ENV_PENDULUM_V0, mode=_capi.MODE_CONTINUOUS)
    e = N.HipEngine(n_trees=16, n_sims=8, c_uct=1.0, gamma=1.0, **kw)
    e.set_weights(desc, blob)
    B = 77
    obs, _ = _data(1, B, in_dim, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    tr = _trainer(desc, 1, 128, True)
    raw = _forward(tr, _flat([pol]), obs.to(DEV))
    tr.close()
    err = np.abs(raw[0].cpu().numpy() - want).max()
    print(f"forward vs azg_mlp_eval {shape}: max abs difference {err:.3g}")
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------ 5. the optimiser steps
def _sizes(pol):
    return [t.numel() for t in _capi.policy_tensors(pol)[1]]


def _ulp(x):
    """One float32 unit in the last place of every element of the (float64) tensor x."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32))).double()


def _against_yardstick(name, got, truth, yard, sizes, fails):
    """Per parameter tensor: the kernel's error against the float64 truth is at most 4 x the float32 yardstick's largest error
    plus one ulp of the element (test_population_trainer_optim.py's bound)."""
    off = 0
    for i, n in enumerate(sizes):
        sl = slice(off, off + n)
        off += n
        e_k, e_y = (got[sl].double() - truth[sl]).abs(), (yard[sl].double() - truth[sl]).abs()
        print(f"{name} tensor {i}: float32 torch error {float(e_y.max()):.3g}, kernel error {float(e_k.max()):.3g}")
        if not torch.all(e_k <= 4 * e_y.max() + _ulp(truth[sl])):
            fails.append((name, i, float(e_y.max()), float(e_k.max())))
    assert off == got.numel()


@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_rmsprop_step_given_gradient(weight_decay):
    """W2, three consecutive fused steps; after each, the kernel's parameters against torch.optim.RMSprop in float64 fed the kernel's
    own gradients: at most half an ulp of the parameter plus 16 * 2^-24 * |delta p| (test_optimiser_step_given_gradient's bound)."""
    in_dim, hidden, head, act = W2
    pol = _policies(_key(W2), 1, 31)[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = _trainer(desc, 1, 512, True)
    params, sq = _flat([pol]), torch.zeros((1, tr.n_params), device=DEV)
    ref = params[0].cpu().double().clone().requires_grad_(True)
    ropt = torch.optim.RMSprop([ref], weight_decay=weight_decay, momentum=0, centered=False, **OPT)
    opt = _capi.rmsprop_opt(weight_decay=weight_decay, **OPT)
    for step in range(3):
        obs, d_raw = _data(1, 64, in_dim, 1 + desc.n_dist, 40 + step)
        before = params[0].cpu().double()
        # the float64 optimiser starts every step from the kernel's parameters, so only this step's arithmetic is compared
        with torch.no_grad():
            ref.copy_(before)
        sq_before = sq[0].cpu().double()
        _, grads = _step(tr, params, obs.to(DEV), d_raw.to(DEV), opt, sq)
        ref.grad = grads[0].cpu().double()
        ropt.step()
        got, want = params[0].cpu(), ref.detach()
        ulp = torch.from_numpy(np.spacing(np.abs(got.numpy()))).double()
        bound = 0.5 * ulp + 16 * U * (want - before).abs()
        err = (got.double() - want).abs()
        print(f"step {step} wd {weight_decay}: max err/bound {float((err / bound).max()):.3g}")
        assert torch.all(err <= bound) and not torch.equal(got.double(), before)
        sq_want = OPT["alpha"] * sq_before + (1 - OPT["alpha"]) * (ref.grad + weight_decay * before) ** 2
        sq_tol = 8 * U * (OPT["alpha"] * sq_before + (1 - OPT["alpha"]) * (ref.grad.abs() + weight_decay * before.abs()) ** 2)
        assert torch.all((sq[0].cpu().double() - sq_want).abs() <= sq_tol)
    tr.close()


def test_adam_clip_step_given_gradient():
    """W2, three consecutive deferred steps with Adam and a grad_clip below the gradient's norm.  Truth: clip_grad_norm_ +
    torch.optim.Adam (single-tensor) in float64 on the CPU, fed the kernel's gradients and restarted every step from the kernel's
    parameters and state; yardstick: the same in float32 (test_population_trainer_optim.py's bounds)."""
    in_dim, hidden, head, act = W2
    pol = _policies(_key(W2), 1, 31)[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = _trainer(desc, 1, 512, True)
    params = _flat([pol])
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    sizes, fails, clip = _sizes(pol), [], 0.01
    for step in range(3):
        obs, d_raw = _data(1, 64, in_dim, 1 + desc.n_dist, 40 + step)
        before = [t[0].cpu().clone() for t in (params, m, v)]
        grads, norms = _step_opt(tr, params, obs.to(DEV), d_raw.to(DEV),
                                 lambda n: _capi.optim("adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"],
                                                       weight_decay=1e-4, grad_clip=clip, step=step, grad_norms=n))
        want_norm = float(torch.sqrt((grads[0].cpu().double() ** 2).sum()))
        print(f"adam step {step}: kernel norm {float(norms[0])!r}, float64 {want_norm!r}, grad_clip {clip}")
        assert want_norm > clip and abs(float(norms[0]) - want_norm) <= float(np.spacing(np.float32(want_norm)))
        res = {}
        for dtype in (torch.float64, torch.float32):
            p = before[0].to(dtype).clone().requires_grad_(True)
            p.grad = grads[0].cpu().to(dtype)
            torch.nn.utils.clip_grad_norm_([p], clip)
            o = torch.optim.Adam([p], weight_decay=1e-4, amsgrad=False, foreach=False, **ADAM)
            if step:
                o.state[p] = {"step": torch.tensor(float(step)), "exp_avg": before[1].to(dtype).clone(), "exp_avg_sq": before[2].to(dtype).clone()}
            o.step()
            res[dtype] = (p.detach(), o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"])
        for j, (name, got) in enumerate((("params", params), ("exp_avg", m), ("exp_avg_sq", v))):
            _against_yardstick(f"adam+clip step {step} {name}", got[0].cpu(), res[torch.float64][j], res[torch.float32][j], sizes, fails)
        assert not torch.equal(params[0].cpu(), before[0])
    tr.close()
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 6. end to end
def _twin(cfg, agent, device, dtype=torch.float32):
    """A new agent with ``agent``'s weights (the agents here have taken no optimiser step yet, so their optimisers and learned
    temperatures are as new; a tuned loss holds a non-leaf alpha, which copy.deepcopy refuses)."""
    from alphazero_gym_amd.envs import make_game
    a = run.make_agent("continuous", dict(cfg, device=device), make_game(cfg["game"]))
    a.nn.load_state_dict({k: v.detach().to(device) for k, v in agent.nn.state_dict().items()})
    a.nn.to(dtype)
    return a


def _update_f64(cfg, agent, batch):
    """The agent's loss dictionary in float64 on the CPU."""
    a = _twin(cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    d = a._loss(s, ac, c, v.reshape(-1, 1))
    return {k: float(x.detach()) if hasattr(x, "detach") else float(x) for k, x in d.items()}


def _batch(rows, S, A):
    return (rows[:, :S], rows[:, S:S + A], rows[:, S + A:S + 2 * A], rows[:, S + 2 * A:S + 3 * A], rows[:, -1])


def test_end_to_end():
    """One continuous agent with hidden_dimensions [512, 272] and its DeviceSelfPlay of 16 games, 8 rollouts, 8 steps.  update's loss
    dictionary against float64 (trainer error <= 4 x agent.update's float32 error per key); train_epoch_ring against the same
    minibatches passed to a twin trainer's update one by one, bit for bit; after upload_flat a search equals that of a fresh engine."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
    from alphazero_gym_amd.envs import make_game
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    cfg = run._merge(run.CONTINUOUS_DEFAULTS, dict(device=DEV, policy=dict(hidden_dimensions=[512, 272])))
    torch.manual_seed(70)
    agent = run.make_agent("continuous", cfg, make_game(cfg["game"]))
    other = _twin(cfg, agent, DEV)
    m = cfg["mcts"]
    T, steps, batch_size = 16, 8, 32
    sp = run.DeviceSelfPlay(agent.nn, game=cfg["game"], n_games=T, n_rollouts=8, c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"],
                            c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5), capacity_steps=steps)
    assert sp.play_device(steps) == (steps, 0)
    S, A = sp.engine.s_obs, sp.engine.kmax
    rows = sp._split(DeviceReplay(sp.engine, 1).rows(), steps)[0]
    n = steps * T
    assert rows.shape[0] == n
    first = _batch(rows[:64], S, A)
    truth = _update_f64(cfg, agent, first)
    yard = _twin(cfg, agent, DEV).update(first)
    tr = PopulationTrainer([agent], wide=True, losses="device")
    ref = PopulationTrainer([other], wide=True, losses="device")
    got = tr.update([first])
    assert ref.update([first]) == got
    assert set(got[0]) == set(yard)
    fails = []
    for key in yard:
        e_y, e_t = abs(yard[key] - truth[key]), abs(got[0][key] - truth[key])
        print(f"wide continuous {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g}")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    assert not fails, fails
    np.testing.assert_array_equal(_capi.policy_blob(agent.nn)[1], tr.flat[0].cpu().numpy())   # the step went into the agent's parameters
    # the epoch on the ring against its minibatches one by one
    order = np.random.RandomState(5).permutation(n)[None, :]
    sums = tr.train_epoch_ring(sp, order, batch_size=batch_size)
    want = {}
    for i, j in minibatch_bounds(n, batch_size):
        info = ref.update([_batch(rows[torch.from_numpy(order[0, i:j]).to(DEV)], S, A)])[0]
        for key, val in info.items():
            want[key] = want.get(key, 0.0) + val
    assert sums[0] == want
    for name in ("flat", "square_avg", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq"):
        assert torch.equal(getattr(tr, name), getattr(ref, name)), f"{name}: the ring epoch and its steps differ"
    assert tr.alpha_step == ref.alpha_step == 1 + n // batch_size
    # the hand-off: a search after upload_flat equals a search of a fresh engine built from a copy of the policy
    kw = dict(run._game_engine_kwargs(cfg["game"], agent.nn, m.get("c_pw", 1.0), m.get("kappa", 0.5)), trees_per_model=T, n_rollouts=8,
              c_uct=m["c_uct"], gamma=m["gamma"], epsilon=m["epsilon"])
    pm = PopulationMCTS([agent.nn], **kw)
    tr.update([first])   # behind torch's back: the engine's weights are now stale and no parameter's _version has moved
    pm.upload_flat(tr.desc, tr.flat)
    assert pm.last_weight_sync == "device"
    roots = pm.engine.synthetic_roots()
    pm.engine.set_search_index(5)
    pm.search(roots)
    res = pm.results()
    fresh_model = copy.deepcopy(agent.nn)
    np.testing.assert_array_equal(_capi.policy_blob(fresh_model)[1], tr.flat[0].cpu().numpy())
    fresh = PopulationMCTS([fresh_model], **kw)
    fresh.engine.set_search_index(5)
    fresh.search(roots)
    want = fresh.results()
    for key in want:
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    sp.upload_flat(tr.desc, tr.flat)
    for x in (pm, fresh, sp, tr, ref):
        x.close()


# ------------------------------------------------------------------------------------------------ 7. the ABI's errors
def test_abi_errors():
    N = _native()
    f = N.fns()
    for bad in (_capi.make_desc(4, [128, 128], 2, "relu", layernorm=True), _capi.make_desc(9, [64], 2, "relu"),
                _capi.make_desc(4, [40], 2, "relu"), _capi.make_desc(4, [1040], 2, "relu"), _capi.make_desc(4, [512, 40], 2, "relu")):
        with pytest.raises(_capi.EngineError) as ei:
            N.HipTrainer(bad, 2, 64, wide=True)
        assert ei.value.code == _capi.AZG_E_UNSUPPORTED and str(ei.value)
    desc = _capi.make_desc(4, [512, 32], 2, "relu")
    h = C.c_void_p()
    assert f["trainer_create_wide"](0, None, 2, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 0, 64, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 2, 0, C.byref(h)) == _capi.AZG_E_INVALID
    assert f["trainer_create_wide"](0, C.byref(desc), 2, 64, None) == _capi.AZG_E_INVALID
    assert not h.value
    tr = N.HipTrainer(desc, 2, 64, wide=True)
    params = torch.randn((2, tr.n_params), device=DEV)
    sq = torch.zeros_like(params)
    mm, vv = torch.zeros_like(params), torch.full_like(params, 0.25)
    keep = [t.clone() for t in (params, sq, mm, vv)]
    obs, d_raw = (t.to(DEV) for t in _data(2, 64, 4, 3, 1))
    raw = torch.zeros((2, 64, 3), device=DEV)
    opt = _capi.rmsprop_opt(**OPT)
    torch.cuda.synchronize()

    def code(fn, *a):
        with pytest.raises(_capi.EngineError) as ei:
            fn(*a)
        assert str(ei.value)
        return ei.value.code

    def unchanged():
        return all(torch.equal(t, k) for t, k in zip((params, sq, mm, vv), keep))

    def adam(**kw):
        return _capi.optim("adam", **dict(dict(lr=1e-3, state0=vv.data_ptr(), state1=mm.data_ptr(), eps=1e-7, betas=(0.9, 0.99)), **kw))

    P, O, D, R, S = params.data_ptr(), obs.data_ptr(), d_raw.data_ptr(), raw.data_ptr(), sq.data_ptr()
    assert code(tr.forward, None, O, 64, R) == _capi.AZG_E_INVALID
    assert code(tr.forward, P, O, 65, R) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # no forward yet
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 64, adam()) == _capi.AZG_E_STATE
    assert unchanged()
    tr.forward(P, O, 64, R)
    assert code(tr.backward_step, P, None, 64, opt, S) == _capi.AZG_E_INVALID
    assert unchanged()
    assert code(tr.backward_step, P, D, 32, opt, S) == _capi.AZG_E_STATE      # not the forward's n_rows
    assert unchanged()
    assert code(tr.backward_step, P, D, 64, _capi.rmsprop_opt(grad_clip=1.0, **OPT), S) == _capi.AZG_E_UNSUPPORTED
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 64, adam(state1=None)) == _capi.AZG_E_INVALID
    assert unchanged()
    assert code(tr.backward_step_opt, P, D, 32, adam()) == _capi.AZG_E_STATE
    assert unchanged()
    tr.backward_step(P, D, 64, opt, S)   # the refused calls left the forward's state usable
    assert not torch.equal(params, keep[0]) and not torch.equal(sq, keep[1])
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # the scratch is consumed
    tr.close()


# ------------------------------------------------------------------------------------------------ 8. the example
def test_example_wide():
    """examples/population_selfplay_train.py --seeds 0 --hidden 512 272 --wide: the fused device trainer and the epoch trainer take
    the same steps (same losses, same returns, same final parameters)."""
    import population_selfplay_train as X
    base = ["--seeds", "0", "--hidden", "512", "272", "--wide", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2",
            "--steps-per-iter", "10"]
    assert X.parse_args(base).wide and not X.parse_args([a for a in base if a != "--wide"]).wide
    final = {}

    def keep(name):
        return lambda agents: final.__setitem__(name, [_capi.policy_blob(a.nn)[1].copy() for a in agents])

    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None, on_end=keep("fused"))
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None, on_end=keep("epoch"))
    assert len(fused) == len(epoch) == 2
    for a, b in zip(fused, epoch):
        assert len(a["loss"]) == 1 and np.isfinite(a["loss"]).all() and a["weight_sync"] == "device"
        assert a["loss"] == b["loss"] and a["mean_return"] == b["mean_return"]
    assert len(final["fused"]) == 1 and np.isfinite(final["fused"][0]).all()
    np.testing.assert_array_equal(final["fused"][0], final["epoch"][0])
