"""GPU: LayerNorm trunks in the wide population trainer (azg_trainer_create_wide_ex, PopulationTrainer(wide_layernorm=True)).  Where
azg_trainer_create_ex's trainer takes the shape too, the wide one must give its bits; a descriptor without LayerNorm must give
azg_trainer_create_wide's.  On the wide shapes: population invariance and repeatability bit for bit in both backward forms, strips
of 2 and 4 tiles, gradients (ln.weight and ln.bias included) against float64 autograd with float32 autograd as the yardstick, the
forward pass against the engine, the optimiser steps given the gradient, the end-to-end update and epoch with the hand-off to the
search, the ABI's errors and the example.  Every LayerNorm here has gamma = 1 + 0.5 randn and beta = 0.5 randn, so that neither drops
out of the arithmetic."""
import copy
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import trainer_edges as E
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.network.policies import make_policy

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

DEV = "cuda"
U = 2.0 ** -24
OPT = dict(lr=1e-3, alpha=0.9, eps=1e-10)
ADAM = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-7)   # the reference's Adam settings

# (in_dim, hidden, head, activation), all with LayerNorm.  The overlap with azg_trainer_create_ex: test_population_trainer_layernorm.py's
# four shapes and the largest net that trainer takes.
NARROW = [
    (2, [16], ("normal",), "elu"),
    (4, [48, 80], ("discrete", 2), "relu"),
    (3, [128, 128, 128], ("gmm", 2), "elu"),
    (6, [256, 16], ("discrete", 3), "relu"),
    (3, [256, 256, 256], ("normal",), "elu"),
]
# The wide shapes: one layer beyond the first trainer's width; lane chains of 17, 33 and 20 links with partial strips; the longest
# chain (64 links); the full depth.
W1 = (4, [512], ("discrete", 2), "relu")
W2 = (3, [272, 528, 272, 320], ("gmm", 2), "elu")
W3 = (6, [1024, 1024], ("normal",), "elu")
W4 = (4, [64] * 8, ("discrete", 3), "silu")
WIDE = [W1, W2, W3, W4]


def _id(s):
    return f"{s[0]}in_{'x'.join(map(str, s[1]))}_{'_'.join(map(str, s[2]))}_{s[3]}" if isinstance(s, tuple) else str(s)


def _native():
    from alphazero_gym_amd import _native as N
    N.lib()
    return N


def _trainer(desc, K, max_batch, which):
    """which: "wide_ex" (azg_trainer_create_wide_ex, options.layernorm = 1) | "ex" (azg_trainer_create_ex) | "wide" (azg_trainer_create_wide)"""
    kw = {"wide_ex": dict(wide_layernorm=True), "ex": dict(layernorm=True), "wide": dict(wide=True)}[which]
    return _native().HipTrainer(desc, K, max_batch, **kw)


def _randomise_layernorms(pol, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for mod in pol.trunk:
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_((1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g)).to(mod.weight.device))
                mod.bias.copy_((0.5 * torch.randn(mod.bias.shape, generator=g)).to(mod.bias.device))


def _policy(in_dim, hidden, head, act, seed, layernorm=True):
    """head: ("discrete", n_actions) | ("normal",) | ("gmm", components)"""
    torch.manual_seed(seed)
    if head[0] == "discrete":
        pol = make_policy(in_dim, 1, "discrete", list(hidden), act, num_actions=head[1], layernorm=layernorm)
    else:
        pol = make_policy(in_dim, 1, "normal", list(hidden), act, num_components=1 if head[0] == "normal" else head[1], action_bound=2.0,
                          layernorm=layernorm)
    _randomise_layernorms(pol, seed)
    return pol


@functools.lru_cache(maxsize=None)
def _policies(shape_key, K, first_seed, layernorm=True):
    """K policies of one shape, built once per module run and never changed (the trainers work on copies of their blobs)."""
    in_dim, hidden, head, act = shape_key
    return tuple(_policy(in_dim, list(hidden), head, act, first_seed + k, layernorm) for k in range(K))


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
    """forward + backward_step_opt; make_opt(grad_norms address) -> azg_optim.  Returns (raw, grads, grad_norms)."""
    K, B = obs.shape[:2]
    raw = _forward(tr, params, obs)
    grads, norms = torch.zeros_like(params), torch.full((K,), -1.0, device=DEV)
    tr.backward_step_opt(params.data_ptr(), d_raw.data_ptr(), B, make_opt(norms.data_ptr()), grads.data_ptr())
    return raw, grads, norms


FUSED_NAMES = ("raw", "grads", "params", "square_avg")
ADAM_NAMES = ("raw", "grads", "params", "exp_avg", "exp_avg_sq", "grad_norms")
FORMS = ((0, FUSED_NAMES, "fused"), (1, ADAM_NAMES, "adam"))


def _run_fused(tr, pols, obs, d_raw):
    """forward + backward_step (RMSprop, weight decay, square_avg 0.25) from the policies' weights: CPU copies, FUSED_NAMES' order."""
    params, sq = _flat(pols), torch.full((len(pols), tr.n_params), 0.25, device=DEV)
    raw, grads = _step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=1e-4, **OPT), sq)
    return [t.cpu() for t in (raw, grads, params, sq)]


def _run_adam(tr, pols, obs, d_raw):
    """forward + backward_step_opt (Adam, grad_clip 1e-3, step 3, grad_norms): CPU copies, ADAM_NAMES' order."""
    n = len(pols)
    params = _flat(pols)
    m, v = torch.full((n, tr.n_params), 0.01, device=DEV), torch.full((n, tr.n_params), 0.25, device=DEV)
    raw, grads, norms = _step_opt(tr, params, obs, d_raw, lambda nn: _capi.optim(
        "adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=1e-4, grad_clip=1e-3, step=3,
        grad_norms=nn))
    return [t.cpu() for t in (raw, grads, params, m, v, norms)]


def _both(tr, pols, obs, d_raw):
    return _run_fused(tr, pols, obs, d_raw), _run_adam(tr, pols, obs, d_raw)


def _same(a, b, what):
    for form, names, label in FORMS:
        assert len(a[form]) == len(b[form]) == len(names)
        for x, y, name in zip(a[form], b[form], names):
            assert torch.equal(x, y), f"{name} ({label}): {what}"


def _sane(got, pols):
    """Everything is finite, the parameters moved in both forms, the norms are positive."""
    start = _flat(pols).cpu()
    for form, names, _ in FORMS:
        assert all(torch.isfinite(t).all() for t in got[form])
        assert not torch.equal(got[form][names.index("params")], start)
    assert bool((got[1][5] > 0).all())


# ------------------------------------------------------------------------------------------------ 1. the first LayerNorm trainer's bits
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_overlap_bit_for_bit(shape, B):
    """An azg_trainer_create_wide_ex trainer and an azg_trainer_create_ex trainer on the same inputs: forward + backward_step, and
    forward + backward_step_opt with Adam, a clip, grad_norms and step 3, give the same bits in raw, grads, params, every optimiser
    state and the norms."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(_key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 1
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    got = {}
    for which in ("ex", "wide_ex"):
        tr = _trainer(desc, K, 512, which)
        assert tr.n_params == sum(p.numel() for p in pols[0].parameters())
        got[which] = _both(tr, pols, obs, d_raw)
        tr.close()
    _same(got["ex"], got["wide_ex"], "the wide LayerNorm trainer's bits differ from azg_trainer_create_ex's")
    _sane(got["wide_ex"], pols)


def test_overlap_constant_row():
    """trainer_edges.py's LayerNorm net, whose all-zero observation gives a LayerNorm row of equal values (var = 0): the same bits."""
    pol = E.layernorm_net()
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = (t.unsqueeze(0).contiguous().to(DEV) for t in E.layernorm_data())
    got = {}
    for which in ("ex", "wide_ex"):
        tr = _trainer(desc, 1, 64, which)
        got[which] = _both(tr, [pol], obs, d_raw)
        tr.close()
    _same(got["ex"], got["wide_ex"], "the wide LayerNorm trainer's bits differ on the constant row")
    _sane(got["wide_ex"], [pol])


# ------------------------------------------------------------------------------------------------ 2. a descriptor without LayerNorm
@pytest.mark.parametrize("shape", [W1, (4, [128, 128], ("discrete", 2), "relu")], ids=_id)
def test_plain_descriptor_gives_create_wide_bits(shape):
    in_dim, hidden, head, act = shape
    K, B = 3, 17
    pols = _policies(_key(shape), K, 50, False)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 0
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    got = {}
    for which in ("wide", "wide_ex"):
        tr = _trainer(desc, K, 512, which)
        got[which] = _both(tr, pols, obs, d_raw)
        tr.close()
    _same(got["wide"], got["wide_ex"], "azg_trainer_create_wide_ex differs from azg_trainer_create_wide on a plain trunk")
    _sane(got["wide_ex"], pols)


# ------------------------------------------------------------------------------------------------ 3. invariance and repeatability
@pytest.mark.parametrize("B", [1, 17, 128])
@pytest.mark.parametrize("shape", WIDE, ids=_id)
def test_population_invariance(shape, B):
    """Net k of a K = 3 trainer equals a K = 1 trainer on net k's data and two runs of the same call are equal, bit for bit, in the
    fused and the deferred form; the two forms' gradients are equal; everything is finite and the parameters moved."""
    in_dim, hidden, head, act = shape
    K = 3
    pols = _policies(_key(shape), K, 50)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == 1
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    runs = []
    for _ in range(2):
        tr = _trainer(desc, K, 512, "wide_ex")
        runs.append(_both(tr, pols, obs, d_raw))
        tr.close()
    _same(runs[0], runs[1], "two runs differ")
    fused, adam = runs[0]
    assert torch.equal(fused[1], adam[1]), "the fused and the deferred form's gradients differ"
    _sane(runs[0], pols)
    tr1 = _trainer(desc, 1, 512, "wide_ex")
    for k in range(K):
        o, d = obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous()
        one = _both(tr1, pols[k:k + 1], o, d)
        for form, names, label in FORMS:
            for a, b, name in zip(runs[0][form], one[form], names):
                assert torch.equal(a[k], b[0]), f"{name} of net {k} ({label}): K = 3 and K = 1 differ"
    tr1.close()


# ------------------------------------------------------------------------------------------------ 4. wider strips
# The launches take strips of NT = 1, 2 or 4 tiles (dispatch_train_wide.hip: pick_nt, the widest NT with row tiles * ceil(tiles / NT)
# * K >= 2048 strips, else 1), and the cases above, K <= 3 and B <= 128, all run NT = 1.  [528, 272] has 33 and 17 tiles, so every strip
# row of 2 or 4 tiles ends in a partial strip of 1.  With 8 row tiles at B = 128 and 32 at B = 512 (forward and (a) over the layer's
# width; (b) of layer 1 over 17 row tiles x 33 tiles):
#   K = 16, B = 128: forward of layer 0 and (a) of layer 1 (G's store)  8 * 17 * 16 = 2176 -> NT = 2;  (b) of layer 1 -> NT = 4
#   K = 16, B = 512: forward of both layers and both (a)  32 * 9 * 16, 32 * 5 * 16 -> NT = 4;  (b) of layer 1 NT = 4
#   K =  8, B = 128: (b) of layer 1  17 * 17 * 8 = 2312 -> NT = 2;  everything else NT = 1
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
    """Strips of 2 and 4 tiles with a partial last strip in the forward, (a) (G's store) and (b) launches: the first and the last net
    of the K-net trainer equal the K = 1 trainer (strips of one tile) on their data bit for bit, in the fused and the deferred form."""
    in_dim, hidden, head, act = W5
    pols = _policies(_key(W5), 16, 50)[:K]
    desc = _capi.policy_tensors(pols[0])[0]
    obs, d_raw = (t.to(DEV) for t in _data(K, B, in_dim, 1 + desc.n_dist, 7))
    tr = _trainer(desc, K, 512, "wide_ex")
    got = _both(tr, pols, obs, d_raw)
    tr.close()
    assert torch.equal(got[0][1], got[1][1]), "the fused and the deferred form's gradients differ"
    _sane(got, pols)
    tr1 = _trainer(desc, 1, 512, "wide_ex")
    for k in (0, K - 1):
        one = _both(tr1, pols[k:k + 1], obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous())
        for form, names, label in FORMS:
            for a, b, name in zip(got[form], one[form], names):
                assert torch.equal(a[k], b[0]), f"{name} of net {k} ({label}): K = {K} and K = 1 differ"
    tr1.close()


# ------------------------------------------------------------------------------------------------ 5. gradients against autograd
def _autograd(pol, obs, d_raw, dtype):
    p = copy.deepcopy(pol).to(dtype)
    raw = _raw_of(p, obs.to(dtype))
    (raw * d_raw.to(dtype)).sum().backward()
    return [t.grad for t in _capi.policy_tensors(p)[1]]


GRAD_CASES = [(s, 128) for s in WIDE] + [(W1, 17), (W2, 17)] + [
    ((4, [272, 32], ("discrete", 16), a), 128) for a in ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda v: _id(v))
def test_gradients_against_autograd(shape, B):
    """Truth: float64 autograd on the CPU.  Yardstick: float32 autograd on the CPU, error max|g32 - g64| / max|g64| per parameter
    tensor.  The kernel's error by the same measure may be at most 4 * sqrt(max(Hmax, 256) / 256) x that (the wide trainer's rule: 4
    up to width 256, 5.75 at 528, 8 at 1024), for ln.weight and ln.bias like the rest.  B = 17: padded rows must contribute nothing
    and nothing may be non-finite."""
    in_dim, hidden, head, act = shape
    pol = _policies(_key(shape), 1, 21)[0]
    desc, tensors = _capi.policy_tensors(pol)
    assert len(tensors) == 4 * len(hidden) + 4
    obs, d_raw = _data(1, B, in_dim, 1 + desc.n_dist, 13)
    g64 = _autograd(pol, obs[0], d_raw[0], torch.float64)
    g32 = _autograd(pol, obs[0], d_raw[0], torch.float32)
    tr = _trainer(desc, 1, 512, "wide_ex")
    params, sq = _flat([pol]), torch.zeros((1, tr.n_params), device=DEV)
    raw, grads = _step(tr, params, obs.to(DEV), d_raw.to(DEV), _capi.rmsprop_opt(**OPT), sq)
    tr.close()
    grads = grads[0].cpu()
    assert torch.isfinite(raw).all() and torch.isfinite(grads).all() and torch.isfinite(params).all()
    factor = 4.0 * float(np.sqrt(max(max(hidden), 256) / 256.0))
    off, fails = 0, []
    names = [n for n, _ in pol.named_parameters()]
    for name, a64, a32 in zip(names, g64, g32):
        gk = grads[off:off + a64.numel()].view_as(a64).double()
        off += a64.numel()
        scale = a64.abs().max()
        e32, ek = float((a32.double() - a64).abs().max() / scale), float((gk - a64).abs().max() / scale)
        print(f"wide LayerNorm grad {_id(shape)} B={B} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g}, ratio "
              f"{ek / e32 if e32 else float('inf'):.3g} (bound {factor:.3g})")
        if not ek <= factor * e32:
            fails.append((name, e32, ek))
    assert off == grads.numel() == sum(p.numel() for p in pol.parameters())
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 6. forward against the engine
ENGINE_SHAPES = [(4, [512, 272], ("discrete", 2), "relu"), (3, [1024, 1024], ("gmm", 2), "elu")]


def _engine_for(head):
    N = _native()
    if head[0] == "discrete":
        kw = dict(env_id=_capi.ENV_CARTPOLE, mode=_capi.MODE_DISCRETE, num_actions=head[1])
    else:
        kw = dict(env_id=_capi.ENV_PENDULUM_V0, mode=_capi.MODE_CONTINUOUS)
    return N.HipEngine(n_trees=16, n_sims=8, c_uct=1.0, gamma=1.0, **kw)


@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=["cartpole_512x272", "pendulum_2x1024_gmm2"])
def test_forward_against_engine(shape):
    """raw against azg_mlp_eval's raw of a single-net engine of 16 trees with the same LayerNorm weights, at widths the engine pads to
    512 and 1024 (the bound of the two existing tests of this kind: 1e-5; the engine's row statistics are float32)."""
    in_dim, hidden, head, act = shape
    pol = _policies(_key(shape), 1, 3)[0]
    desc, blob = _capi.policy_blob(pol)
    e = _engine_for(head)
    e.set_weights(desc, blob)
    B = 77
    obs, _ = _data(1, B, in_dim, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    tr = _trainer(desc, 1, 128, "wide_ex")
    raw = _forward(tr, _flat([pol]), obs.to(DEV))
    tr.close()
    got = raw[0].cpu().numpy()
    with torch.no_grad():
        truth = _raw_of(copy.deepcopy(pol).double(), obs[0].double()).numpy()
    err = np.abs(got - want).max()
    print(f"wide LayerNorm forward vs azg_mlp_eval {_id(shape)}: max abs difference {err:.3g}; against float64 PyTorch: trainer "
          f"{np.abs(got - truth).max():.3g}, engine {np.abs(want - truth).max():.3g}")
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------ 7. the optimiser steps
@pytest.mark.parametrize("form", ["fused_rmsprop", "deferred_adam"])
def test_optimiser_step_given_gradient(form):
    """Three consecutive steps of W2; after each, every parameter (gamma and beta included) against torch's optimiser in float64 fed
    the kernel's own gradients and started from the kernel's parameters and state: at most half an ulp of the parameter plus
    16 * 2^-24 * |delta p|."""
    in_dim, hidden, head, act = W2
    pol = _policies(_key(W2), 1, 31)[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = _trainer(desc, 1, 512, "wide_ex")
    wd = 1e-4
    params = _flat([pol])
    s0, s1 = torch.zeros_like(params), torch.zeros_like(params)   # square_avg | exp_avg_sq, exp_avg
    sizes = [t.numel() for t in _capi.policy_tensors(pol)[1]]
    names = [n for n, _ in pol.named_parameters()]
    for step in range(3):
        obs, d_raw = (t.to(DEV) for t in _data(1, 64, in_dim, 1 + desc.n_dist, 40 + step))
        before, b0, b1 = (t[0].cpu().double().clone() for t in (params, s0, s1))
        ref = before.clone().requires_grad_(True)
        if form == "fused_rmsprop":
            _, grads = _step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=wd, **OPT), s0)
            ropt = torch.optim.RMSprop([ref], weight_decay=wd, momentum=0, centered=False, foreach=False, **OPT)
            ropt.state[ref] = {"step": torch.tensor(float(step)), "square_avg": b0.clone()}
        else:
            _, grads, _ = _step_opt(tr, params, obs, d_raw, lambda n: _capi.optim(
                "adam", ADAM["lr"], s0.data_ptr(), s1.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=wd, step=step))
            ropt = torch.optim.Adam([ref], weight_decay=wd, amsgrad=False, foreach=False, **ADAM)
            if step:
                ropt.state[ref] = {"step": torch.tensor(float(step)), "exp_avg": b1.clone(), "exp_avg_sq": b0.clone()}
        ref.grad = grads[0].cpu().double()
        ropt.step()
        got, want = params[0].cpu(), ref.detach()
        ulp = torch.from_numpy(np.spacing(np.abs(got.numpy()))).double()
        bound = 0.5 * ulp + 16 * U * (want - before).abs()
        err = (got.double() - want).abs()
        print(f"wide LayerNorm {form} step {step}: max err/bound {float((err / bound).max()):.3g}")
        assert torch.all(err <= bound)
        off = 0
        for name, n in zip(names, sizes):   # every tensor moved, gamma and beta among them
            assert not torch.equal(got[off:off + n].double(), before[off:off + n]), name
            off += n
    tr.close()


# ------------------------------------------------------------------------------------------------ 8. end to end
E2E_HIDDEN = [512, 272]


def _e2e_cfg():
    return run._merge(run.CONTINUOUS_DEFAULTS, dict(device=DEV, policy=dict(hidden_dimensions=E2E_HIDDEN, layernorm=True)))


def _agents_from(cfg, states, device=DEV, dtype=torch.float32):
    from alphazero_gym_amd.envs import make_game
    env = make_game(cfg["game"])
    agents = []
    for k, sd in enumerate(states):
        a = run.make_agent("continuous", dict(cfg, device=device), env, tree_id_base=k)
        a.nn.load_state_dict({name: v.to(device) for name, v in sd.items()})
        a.nn.to(dtype)
        agents.append(a)
    return agents


@functools.lru_cache(maxsize=None)
def _e2e():
    """Two Pendulum [512, 272] LayerNorm nets (as CPU state_dicts) and 24 hand-made replay rows per net: obs (cos, sin, velocity) |
    5 actions inside the bound | 5 counts summing to 25 | 5 Q values (not read) | V."""
    from alphazero_gym_amd.envs import make_game
    cfg = _e2e_cfg()
    env = make_game(cfg["game"])
    K, n, A = 2, 24, 5
    states = []
    for k in range(K):
        torch.manual_seed(70 + k)
        a = run.make_agent("continuous", cfg, env, tree_id_base=k)
        assert a.nn.layernorm and list(a.nn.hidden_dimensions) == E2E_HIDDEN
        _randomise_layernorms(a.nn, 70 + k)
        states.append({name: v.detach().cpu().clone() for name, v in a.nn.state_dict().items()})
    g = torch.Generator().manual_seed(12)
    th = 3.0 * torch.randn((K, n), generator=g)
    obs = torch.stack([torch.cos(th), torch.sin(th), 2.0 * torch.randn((K, n), generator=g)], dim=-1)
    actions = 0.98 * 2.0 * torch.tanh(torch.randn((K, n, A), generator=g))
    extra = torch.randint(0, A, (K, n, 25 - A), generator=g)
    counts = torch.ones((K, n, A)).scatter_add_(2, extra, torch.ones(extra.shape))
    values = torch.randn((K, n, 1), generator=g)
    rows = torch.cat([obs, actions, counts, torch.zeros_like(actions), values], dim=-1).contiguous()
    return cfg, tuple(states), rows, 3, A


def _batches(rows, S, A):
    return [(r[:, :S], r[:, S:S + A], r[:, S + A:S + 2 * A], r[:, S + 2 * A:S + 3 * A], r[:, -1]) for r in rows]


def _update_f64(agent, batch):
    """agent.update in float64 on the CPU (agent: a float64 CPU twin): the loss dictionary and the parameters after the step."""
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    agent.optimizer.zero_grad(set_to_none=True)
    d = agent._loss(s, ac, c, v.reshape(-1, 1))
    d["loss"].backward()
    agent.optimizer.step()
    info = {k: float(x.detach()) if hasattr(x, "detach") else float(x) for k, x in d.items()}
    return info, torch.cat([t.detach().reshape(-1) for t in _capi.policy_tensors(agent.nn)[1]])


def test_end_to_end_update_and_handoff():
    """PopulationTrainer(wide_layernorm=True, losses="device").update against agent.update on copies of the agents: truth is the
    float64 CPU run, the yardstick agent.update in float32; for every key of the loss dictionary and for the parameters after the
    step (one figure: the largest absolute error over the parameter vector, the larger of the two nets, as for each loss key) the
    trainer's error may be at most 4 x the yardstick's.  Then the trained weights of net 0 go into a one-net engine, a short search
    runs, and its mlp_eval agrees with the trainer's forward within 1e-5."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    cfg, states, rows_cpu, S, A = _e2e()
    rows = rows_cpu.to(DEV)
    K = rows.shape[0]
    batches = _batches(rows[:, :16], S, A)
    truth = [_update_f64(a, b) for a, b in zip(_agents_from(cfg, states, "cpu", torch.float64), batches)]
    yard_agents = _agents_from(cfg, states)
    yard = [a.update(b) for a, b in zip(yard_agents, batches)]
    yard_params = [torch.from_numpy(_capi.policy_blob(a.nn)[1]).double() for a in yard_agents]
    agents = _agents_from(cfg, states)
    with pytest.raises(ValueError, match="LayerNorm"):
        PopulationTrainer(agents, wide=True, losses="device")
    tr = PopulationTrainer(agents, wide_layernorm=True, losses="device")
    assert tr.desc.layernorm == 1 and tr.trainer.n_params == sum(p.numel() for p in agents[0].nn.parameters()) == tr.flat.shape[1]
    before = tr.flat.clone()
    got = tr.update(batches)
    assert [set(g) for g in got] == [set(y) for y in yard]
    fails = []
    for key in yard[0]:
        e_y = max(abs(yard[k][key] - truth[k][0][key]) for k in range(K))
        e_t = max(abs(got[k][key] - truth[k][0][key]) for k in range(K))
        print(f"wide LayerNorm end to end {key}: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g} (largest of {K} nets)")
        if not e_t <= 4 * e_y:
            fails.append((key, e_y, e_t))
    e_y = max(float((yard_params[k] - truth[k][1]).abs().max()) for k in range(K))
    e_t = max(float((tr.flat[k].cpu().double() - truth[k][1]).abs().max()) for k in range(K))
    print(f"wide LayerNorm end to end parameters after the step: agent.update float32 error {e_y:.3g}, trainer error {e_t:.3g}")
    if not e_t <= 4 * e_y:
        fails.append(("parameters", e_y, e_t))
    assert not fails, fails
    for k, a in enumerate(agents):   # the step went into the agents' own parameters, ln.weight and ln.bias too
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], tr.flat[k].cpu().numpy())
        off = 0
        for name, p in zip([n for n, _ in a.nn.named_parameters()], _capi.policy_tensors(a.nn)[1]):
            assert not torch.equal(tr.flat[k, off:off + p.numel()], before[k, off:off + p.numel()]), name
            off += p.numel()
    # the hand-off: net 0's trained weights in a one-net engine
    desc = tr.desc
    e = _engine_for(("gmm", 1))
    e.set_weights(desc, tr.flat[0].cpu().numpy())
    e.search(e.synthetic_roots())
    res = e.results()
    assert np.isfinite(res["Q"][res["counts"] > 0]).all() and np.isfinite(res["v_target"]).all() and (res["counts"].sum(axis=1) > 0).all()
    B = 77
    obs, _ = _data(K, B, S, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    raw = _forward(tr.trainer, tr.flat, obs.to(DEV))
    err = np.abs(raw[0].cpu().numpy() - want).max()
    print(f"wide LayerNorm end to end: trained net 0, trainer forward vs azg_mlp_eval max abs difference {err:.3g}")
    assert err <= 1e-5
    tr.close()


@pytest.mark.parametrize("optimizers", ["rmsprop", "agents"])
def test_epoch_is_its_updates(optimizers):
    """One train_epoch of three minibatches (24 rows, batch_size 8) equals three update calls on the same minibatches, bit for bit in
    flat, the optimiser state, the learned temperatures and the loss sums."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer, minibatch_bounds
    cfg, states, rows_cpu, S, A = _e2e()
    if optimizers == "agents":
        cfg = dict(cfg, optimizer=dict(run.ADAM), agent=dict(cfg["agent"], grad_clip=0.1))
    rows = rows_cpu.to(DEV)
    K, n, batch = rows.shape[0], rows.shape[1], 8
    seeds = [5, 6]
    assert minibatch_bounds(n, batch) == [(0, 8), (8, 16), (16, 24)]
    one = PopulationTrainer(_agents_from(cfg, states), max_batch=64, losses="device", optimizers=optimizers, wide_layernorm=True)
    ep = PopulationTrainer(_agents_from(cfg, states), max_batch=64, losses="device", optimizers=optimizers, wide_layernorm=True)
    order = torch.from_numpy(np.stack([np.random.RandomState(s).permutation(n) for s in seeds])).to(DEV)
    net = torch.arange(K, device=DEV)[:, None]
    sums = [{} for _ in range(K)]
    for i, j in minibatch_bounds(n, batch):
        b = rows[net, order[:, i:j]]
        infos = one.update((b[..., :S], b[..., S:S + A], b[..., S + A:S + 2 * A], b[..., S + 2 * A:S + 3 * A], b[..., -1]))
        for s, info in zip(sums, infos):
            for key, val in info.items():
                s[key] = s.get(key, 0.0) + val
    init = ep.flat.clone()
    got = ep.train_epoch(rows, S, A, batch_size=batch, shuffle_seeds=seeds)
    assert got == sums and all(np.isfinite(v) for g in got for v in g.values())
    state = ("flat", "square_avg", "exp_avg", "exp_avg_sq", "log_alpha", "alpha_exp_avg", "alpha_exp_avg_sq", "last_grad_norms")
    compared = 0
    for name in state:
        a, b = getattr(one, name), getattr(ep, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b), f"{name}: the epoch and its three updates differ"
            compared += 1
    assert compared >= 2 and (one.opt_step, one.alpha_step) == (ep.opt_step, ep.alpha_step)
    for k, a in enumerate(ep.agents):
        np.testing.assert_array_equal(_capi.policy_blob(a.nn)[1], ep.flat[k].cpu().numpy())
        assert not torch.equal(ep.flat[k], init[k])
    one.close()
    ep.close()


# ------------------------------------------------------------------------------------------------ 9. the ABI's errors
def test_abi_errors():
    N = _native()
    f = N.fns()
    on = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions), 1)
    off = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions), 0)
    short = _capi.AzgTrainerOptions(C.sizeof(_capi.AzgTrainerOptions) - 4, 1)
    desc = _capi.make_desc(4, [512, 32], 2, "relu", layernorm=True)
    h = C.c_void_p(12345)   # *out is untouched on every error

    def create(d, n_nets, max_batch, opts, out=True):
        return f["trainer_create_wide_ex"](0, C.byref(d) if d is not None else None, n_nets, max_batch,
                                           C.byref(opts) if opts is not None else None, C.byref(h) if out else None)

    for args in ((None, 2, 64, on), (desc, 2, 64, None), (desc, 2, 64, short), (desc, 0, 64, on), (desc, 2, 0, on)):
        assert create(*args) == _capi.AZG_E_INVALID, args[1:3]
        assert h.value == 12345 and f["trainer_last_error"](None)
    assert create(desc, 2, 64, on, out=False) == _capi.AZG_E_INVALID
    for hidden in ([16] * 9, [1040], [40], [512, 40]):
        bad = _capi.make_desc(4, hidden[:8], 2, "relu", layernorm=True)
        bad.n_hidden = len(hidden)
        assert create(bad, 2, 64, on) == _capi.AZG_E_UNSUPPORTED, hidden
        assert h.value == 12345 and f["trainer_last_error"](None)
    assert create(_capi.make_desc(9, [64], 2, "relu", layernorm=True), 2, 64, on) == _capi.AZG_E_UNSUPPORTED and h.value == 12345
    # opts.layernorm = 0: azg_trainer_create_wide, its refusal of a LayerNorm descriptor included
    assert create(desc, 2, 64, off) == _capi.AZG_E_UNSUPPORTED and h.value == 12345
    assert b"LayerNorm" in f["trainer_last_error"](None)
    plain = _capi.make_desc(4, [512, 32], 2, "relu")
    h2 = C.c_void_p()
    assert f["trainer_create_wide_ex"](0, C.byref(plain), 2, 64, C.byref(off), C.byref(h2)) == 0 and h2.value
    assert f["trainer_param_count"](h2) == 4 * 512 + 512 + 512 * 32 + 32 + 3 * 32 + 3
    f["trainer_destroy"](h2)
    # a LayerNorm handle: the parameter count has gamma and beta, and the entry points' own refusals are the wide trainer's
    tr = N.HipTrainer(desc, 2, 64, wide_layernorm=True)
    assert tr.n_params == 4 * 512 + 3 * 512 + 512 * 32 + 3 * 32 + 3 * 32 + 3
    params = torch.randn((2, tr.n_params), device=DEV)
    sq = torch.zeros_like(params)
    keep = [t.clone() for t in (params, sq)]
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
        return all(torch.equal(t, k) for t, k in zip((params, sq), keep))

    P, O, D, R, S = params.data_ptr(), obs.data_ptr(), d_raw.data_ptr(), raw.data_ptr(), sq.data_ptr()
    assert code(tr.forward, P, O, 65, R) == _capi.AZG_E_INVALID
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # no forward yet
    tr.forward(P, O, 64, R)
    assert code(tr.backward_step, P, D, 32, opt, S) == _capi.AZG_E_STATE      # not the forward's n_rows
    assert unchanged()
    tr.backward_step(P, D, 64, opt, S)
    assert not torch.equal(params, keep[0]) and not torch.equal(sq, keep[1]) and torch.isfinite(params).all()
    assert code(tr.backward_step, P, D, 64, opt, S) == _capi.AZG_E_STATE      # the scratch is consumed
    tr.close()


# ------------------------------------------------------------------------------------------------ 10. the example
def test_example_wide_layernorm():
    """examples/population_selfplay_train.py --seeds 0 --hidden 512 272 --wide --layernorm: the fused device trainer and the epoch
    trainer take the same steps (same losses, same returns, same final parameters)."""
    import population_selfplay_train as X
    base = ["--seeds", "0", "--hidden", "512", "272", "--wide", "--layernorm", "--games-per-seed", "8", "--n-rollouts", "8", "--iters", "2",
            "--steps-per-iter", "10"]
    a = X.parse_args(base)
    assert a.wide and a.layernorm
    final = {}

    def keep(name):
        return lambda agents: final.__setitem__(name, [_capi.policy_blob(ag.nn)[1].copy() for ag in agents])

    fused = X.train(X.parse_args(base + ["--trainer", "device-fused"]), log=None, on_end=keep("fused"))
    epoch = X.train(X.parse_args(base + ["--trainer", "device-epoch"]), log=None, on_end=keep("epoch"))
    assert len(fused) == len(epoch) == 2
    for x, y in zip(fused, epoch):
        assert len(x["loss"]) == 1 and np.isfinite(x["loss"]).all() and x["weight_sync"] == "device"
        assert x["loss"] == y["loss"] and x["mean_return"] == y["mean_return"]
    assert len(final["fused"]) == 1 and np.isfinite(final["fused"][0]).all()
    np.testing.assert_array_equal(final["fused"][0], final["epoch"][0])
