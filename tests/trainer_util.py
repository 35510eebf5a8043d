"""What the population trainer's tests share (test_population_trainer*.py, test_population_device_loss*.py,
test_population_train_epoch*.py): constants and shape tables, construction of policies, trainers and agents, one training step in each
call form, the float64 truths and float32 yardsticks, and the bodies of the tests that every trainer kind repeats.  Importing it needs
neither a GPU nor the native library; the functions that launch kernels do.

A trainer ``kind`` is None (azg_trainer_create), "layernorm" (azg_trainer_create_ex), "wide" (azg_trainer_create_wide) or
"wide_layernorm" (azg_trainer_create_wide_ex)."""
import copy
import re

import numpy as np
import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.agents import ContinuousAgent, DiscreteAgent
from alphazero_gym_amd.network.policies import make_policy

DEV = "cuda"
U = 2.0 ** -24   # float32 unit round-off
OPT = dict(lr=1e-3, alpha=0.9, eps=1e-10)
ADAM = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-7)   # the reference's Adam settings

# (in_dim, hidden, head, activation): 1, 2 and 3 hidden layers; widths 16, 128, 256; 2, 3, 4 and 6 inputs; the three head kinds.
# test_population_trainer.py's SHAPES, and the overlap of the wide trainer's tests: the shapes that both trainers take.
NARROW = [
    (2, [16], ("normal",), "elu"),
    (4, [128, 128], ("discrete", 2), "relu"),
    (3, [128, 128, 128], ("gmm", 2), "elu"),
    (6, [256, 16], ("discrete", 3), "relu"),
    (3, [256, 256, 256], ("normal",), "elu"),
]
# The wide shapes: one layer beyond the first trainer's width (the shape test_abi_errors proves refused without the opt-in); four layers
# of 17, 33 and 20 tiles (strips of 1 and 4 tiles, partial strips); the widest k chain (64 links); the full depth.
W1 = (4, [512], ("discrete", 2), "relu")
W2 = (3, [272, 528, 272, 320], ("gmm", 2), "elu")
W3 = (6, [1024, 1024], ("normal",), "elu")
W4 = (4, [64] * 8, ("discrete", 3), "silu")
WIDE = [W1, W2, W3, W4]
W5 = (3, [528, 272], ("gmm", 2), "elu")   # 33 and 17 tiles: every strip row of 2 or 4 tiles ends in a partial strip of 1

KINDS = {None: dict(), "layernorm": dict(layernorm=True), "wide": dict(wide=True), "wide_layernorm": dict(wide_layernorm=True)}


def has_layernorm(kind):
    return kind in ("layernorm", "wide_layernorm")


# ------------------------------------------------------------------------------------------------ loading and construction
def native():
    from alphazero_gym_amd import _native as N
    N.lib()
    return N


def trainer(desc, K, max_batch, kind=None):
    return native().HipTrainer(desc, K, max_batch, **KINDS[kind])


def engine_for(head, in_dim=4):
    """A single-net engine of 16 trees whose azg_mlp_eval takes the head: CartPole or Acrobot (6 inputs), or Pendulum."""
    if head[0] == "discrete":
        kw = dict(env_id={4: _capi.ENV_CARTPOLE, 6: _capi.ENV_ACROBOT}[in_dim], mode=_capi.MODE_DISCRETE, num_actions=head[1])
    else:
        kw = dict(env_id=_capi.ENV_PENDULUM_V0, mode=_capi.MODE_CONTINUOUS)
    return native().HipEngine(n_trees=16, n_sims=8, c_uct=1.0, gamma=1.0, **kw)


def randomise_layernorms(pol, seed):
    """gamma = 1 + 0.5 randn, beta = 0.5 randn, so that neither drops out of the arithmetic."""
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for mod in pol.trunk:
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_((1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g)).to(mod.weight.device))
                mod.bias.copy_((0.5 * torch.randn(mod.bias.shape, generator=g)).to(mod.bias.device))


def policy(in_dim, hidden, head, act, seed, layernorm=False):
    """head: ("discrete", n_actions) | ("normal",) | ("gmm", components); with ``layernorm`` a LayerNorm after every trunk activation,
    randomised by randomise_layernorms(seed)."""
    torch.manual_seed(seed)
    if head[0] == "discrete":
        pol = make_policy(in_dim, 1, "discrete", list(hidden), act, num_actions=head[1], layernorm=layernorm)
    else:
        pol = make_policy(in_dim, 1, "normal", list(hidden), act, num_components=1 if head[0] == "normal" else head[1], action_bound=2.0,
                          layernorm=layernorm)
    if layernorm:
        randomise_layernorms(pol, seed)
    return pol


def key(shape):
    """The shape as a hashable cache key."""
    return (shape[0], tuple(shape[1]), shape[2], shape[3])


def flat(policies):
    return torch.from_numpy(np.stack([_capi.policy_blob(p)[1] for p in policies])).to(DEV)


def raw_of(pol, x):
    h = pol.trunk(x)
    return torch.cat([pol.value_head(h), pol.dist_head(h)], dim=-1)


def data(K, B, in_dim, n_raw, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((K, B, in_dim), generator=g)
    d_raw = torch.randn((K, B, n_raw), generator=g) / B
    return obs, d_raw


def sizes(pol):
    return [t.numel() for t in _capi.policy_tensors(pol)[1]]


# ------------------------------------------------------------------------------------------------ one step in each call form
def forward(tr, params, obs):
    K, B = obs.shape[:2]
    raw = torch.empty((K, B, tr.n_raw), device=DEV)
    torch.cuda.synchronize()
    tr.forward(params.data_ptr(), obs.data_ptr(), B, raw.data_ptr())
    return raw


def step(tr, params, obs, d_raw, opt, sq):
    """One forward + fused backward/RMSprop step: (raw, grads); params and sq are updated in place."""
    raw = forward(tr, params, obs)
    grads = torch.zeros_like(params)
    tr.backward_step(params.data_ptr(), d_raw.data_ptr(), obs.shape[1], opt, sq.data_ptr(), grads.data_ptr())
    return raw, grads


def step_opt(tr, params, obs, d_raw, make_opt):
    """forward + backward_step_opt; make_opt(grad_norms address) -> azg_optim.  Returns (raw, grads, grad_norms)."""
    K, B = obs.shape[:2]
    raw = forward(tr, params, obs)
    grads, norms = torch.zeros_like(params), torch.full((K,), -1.0, device=DEV)
    tr.backward_step_opt(params.data_ptr(), d_raw.data_ptr(), B, make_opt(norms.data_ptr()), grads.data_ptr())
    return raw, grads, norms


FUSED_NAMES = ("raw", "grads", "params", "square_avg")
ADAM_NAMES = ("raw", "grads", "params", "exp_avg", "exp_avg_sq", "grad_norms")
FORM_NAMES = {"fused": FUSED_NAMES, "adam": ADAM_NAMES}


def run_fused(tr, pols, obs, d_raw):
    """forward + backward_step (RMSprop, weight decay, square_avg 0.25) from the policies' weights: CPU copies, FUSED_NAMES' order."""
    params, sq = flat(pols), torch.full((len(pols), tr.n_params), 0.25, device=DEV)
    raw, grads = step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=1e-4, **OPT), sq)
    return [t.cpu() for t in (raw, grads, params, sq)]


def run_adam(tr, pols, obs, d_raw, grad_clip):
    """forward + backward_step_opt (Adam, weight decay, grad_clip, step 3, grad_norms; exp_avg 0.01, exp_avg_sq 0.25): CPU copies,
    ADAM_NAMES' order."""
    n = len(pols)
    params = flat(pols)
    m, v = torch.full((n, tr.n_params), 0.01, device=DEV), torch.full((n, tr.n_params), 0.25, device=DEV)
    raw, grads, norms = step_opt(tr, params, obs, d_raw, lambda nn: _capi.optim(
        "adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=1e-4, grad_clip=grad_clip, step=3,
        grad_norms=nn))
    return [t.cpu() for t in (raw, grads, params, m, v, norms)]


def run_forms(tr, pols, obs, d_raw, grad_clip, forms=("fused", "adam")):
    """{form: run_fused's or run_adam's result}, run in the order of ``forms`` on the one trainer."""
    return {f: run_fused(tr, pols, obs, d_raw) if f == "fused" else run_adam(tr, pols, obs, d_raw, grad_clip) for f in forms}


def same(a, b, what):
    """Two results of run_forms hold the same bits."""
    assert list(a) == list(b)
    for form in a:
        names = FORM_NAMES[form]
        assert len(a[form]) == len(b[form]) == len(names)
        for x, y, name in zip(a[form], b[form], names):
            assert torch.equal(x, y), f"{name} ({form}): {what}"


def same_net(got, one, k, what):
    """Net k of the K-net result ``got`` holds the bits of the one-net result ``one``."""
    for form in got:
        for a, b, name in zip(got[form], one[form], FORM_NAMES[form]):
            assert torch.equal(a[k], b[0]), f"{name} of net {k} ({form}): {what}"


def sane(got, pols):
    """Everything is finite, the parameters moved in every form, the norms are positive, and the forms' gradients are equal."""
    start = flat(pols).cpu()
    for form, out in got.items():
        assert all(torch.isfinite(t).all() for t in out)
        assert not torch.equal(out[2], start)
    if "adam" in got:
        assert bool((got["adam"][5] > 0).all())
    if len(got) == 2:
        assert torch.equal(got["fused"][1], got["adam"][1]), "the fused and the deferred form's gradients differ"


# ------------------------------------------------------------------------------------------------ truth and yardsticks
def autograd(pol, obs, d_raw, dtype):
    """Gradients of sum(raw * d_raw) by every parameter in blob order, on the CPU in ``dtype``."""
    p = copy.deepcopy(pol).to(dtype)
    (raw_of(p, obs.to(dtype)) * d_raw.to(dtype)).sum().backward()
    return [t.grad for t in _capi.policy_tensors(p)[1]]


def ulp(x):
    """One float32 unit in the last place of every element of the (float64) tensor x."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32))).double()


def grad_factor(kind, hidden):
    """How many times float32 autograd's error the kernel's gradient error may be.  The first trainers: 4, the project's factor.  The
    wide ones: 4 * sqrt(max(Hmax, 256) / 256) -- 4 up to width 256, 5.75 at 528, 8 at 1024 (an accumulator is one sequential chain whose
    rounding error grows with the square root of its length, where torch's blocked float32 sums stay flat).  One function: the first
    trainers take no width above 256."""
    if kind in (None, "layernorm"):
        assert max(hidden) <= 256
        return 4
    return 4.0 * float(np.sqrt(max(max(hidden), 256) / 256.0))


def hold_grads_to_autograd(tag, kind, pol, grads, g64, g32, factor):
    """Per parameter tensor: max|g - g64| / max|g64| of the kernel's flat gradient is at most ``factor`` x float32 autograd's.  Prints
    a line per tensor; returns (elements seen, [(name, float32 error, kernel error)] of the tensors that miss)."""
    off, fails = 0, []
    for (name, _), a64, a32 in zip(pol.named_parameters(), g64, g32):
        gk = grads[off:off + a64.numel()].view_as(a64).double()
        off += a64.numel()
        scale = a64.abs().max()
        e32, ek = float((a32.double() - a64).abs().max() / scale), float((gk - a64).abs().max() / scale)
        tail = {"wide": f" (bound {factor:.3g} x)",
                "wide_layernorm": f", ratio {ek / e32 if e32 else float('inf'):.3g} (bound {factor:.3g})"}.get(kind, "")
        print(f"{tag} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g}{tail}")
        if not ek <= factor * e32:
            fails.append((name, e32, ek))
    return off, fails


def against_yardstick(name, got, truth, yard, sizes, fails):
    """Per parameter tensor: the kernel's error against the float64 truth is at most 4 x the float32 yardstick's largest error
    plus one ulp of the element."""
    off = 0
    for i, n in enumerate(sizes):
        sl = slice(off, off + n)
        off += n
        e_k, e_y = (got[sl].double() - truth[sl]).abs(), (yard[sl].double() - truth[sl]).abs()
        print(f"{name} tensor {i}: float32 torch error {float(e_y.max()):.3g}, kernel error {float(e_k.max()):.3g}")
        if not torch.all(e_k <= 4 * e_y.max() + ulp(truth[sl])):
            fails.append((name, i, float(e_y.max()), float(e_k.max())))
    assert off == got.numel()


# ------------------------------------------------------------------------------------------------ the repeated tests' bodies
def check_population_invariance(shape, B, kind, pols, forms=("fused", "adam"), grad_clip=1e-3):
    """Net k of a K = len(pols) trainer equals a K = 1 trainer on net k's data, bit for bit (raw, gradients, parameters, optimiser
    state, and the norms of the deferred form); so do two runs of the same call; everything is finite, the parameters moved, and
    where both forms run their gradients are equal.  Returns the K-net result."""
    K = len(pols)
    desc = _capi.policy_tensors(pols[0])[0]
    assert desc.layernorm == int(has_layernorm(kind))
    obs, d_raw = (t.to(DEV) for t in data(K, B, shape[0], 1 + desc.n_dist, 7))
    runs = []
    for _ in range(2):
        tr = trainer(desc, K, 512, kind)
        runs.append(run_forms(tr, pols, obs, d_raw, grad_clip, forms))
        tr.close()
    same(runs[0], runs[1], "two runs differ")
    sane(runs[0], pols)
    tr1 = trainer(desc, 1, 512, kind)
    for k in range(K):
        one = run_forms(tr1, pols[k:k + 1], obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous(), grad_clip, forms)
        same_net(runs[0], one, k, f"K = {K} and K = 1 differ")
    tr1.close()
    return runs[0]


def check_forward_against_engine(shape, kind, pol, label, against_float64=False):
    """raw against azg_mlp_eval's raw of a single-net engine of 16 trees with the same weights (T2: 1e-5; the head sums are ordered
    differently from mlp.cuh's chunked ones and the engine's LayerNorm row statistics are float32, so not bit for bit).
    ``against_float64`` adds both sides' distance from float64 PyTorch to the printed line."""
    in_dim, hidden, head, act = shape
    desc, blob = _capi.policy_blob(pol)
    e = engine_for(head, in_dim)
    e.set_weights(desc, blob)
    B = 77
    obs, _ = data(1, B, in_dim, 1, 11)
    _, _, want = e.mlp_eval(obs[0].numpy())
    e.close()
    tr = trainer(desc, 1, 128, kind)
    raw = forward(tr, flat([pol]), obs.to(DEV))
    tr.close()
    got = raw[0].cpu().numpy()
    err = np.abs(got - want).max()
    more = ""
    if against_float64:
        with torch.no_grad():
            truth = raw_of(copy.deepcopy(pol).double(), obs[0].double()).numpy()
        more = f"; against float64 PyTorch: trainer {np.abs(got - truth).max():.3g}, engine {np.abs(want - truth).max():.3g}"
    print(f"{label}: max abs difference {err:.3g}{more}")
    assert err <= 1e-5


def check_gradients_against_autograd(shape, B, kind, pol, tag):
    """Truth: float64 autograd on the CPU.  Yardstick: float32 autograd on the CPU, error max|g32 - g64| / max|g64| per parameter
    tensor; the kernel's error by the same measure may be at most grad_factor(kind, hidden) x that, for ln.weight and ln.bias like
    the rest.  B = 17: padded rows must contribute nothing, and with LayerNorm nothing may be non-finite."""
    in_dim, hidden, head, act = shape
    ln = has_layernorm(kind)
    desc, tensors = _capi.policy_tensors(pol)
    if ln:
        assert len(tensors) == 4 * len(hidden) + 4
    obs, d_raw = data(1, B, in_dim, 1 + desc.n_dist, 13)
    g64 = autograd(pol, obs[0], d_raw[0], torch.float64)
    g32 = autograd(pol, obs[0], d_raw[0], torch.float32)
    tr = trainer(desc, 1, 512, kind)
    n_params = tr.n_params
    params, sq = flat([pol]), torch.zeros((1, n_params), device=DEV)
    raw, grads = step(tr, params, obs.to(DEV), d_raw.to(DEV), _capi.rmsprop_opt(**OPT), sq)
    tr.close()
    grads = grads[0].cpu()
    if ln:
        assert torch.isfinite(raw).all() and torch.isfinite(grads).all() and torch.isfinite(params).all()
        names = [n for n, _ in pol.named_parameters()]
        assert sum("trunk" in n and g.dim() == 1 for n, g in zip(names, g64)) == 3 * len(hidden)   # bias, ln.weight, ln.bias per layer
    off, fails = hold_grads_to_autograd(tag, kind, pol, grads, g64, g32, grad_factor(kind, hidden))
    assert off == n_params == grads.numel() == sum(p.numel() for p in pol.parameters())
    assert not fails, fails


def check_rmsprop_step_given_gradient(shape, kind, pol, weight_decay):
    """Three consecutive fused steps; after each, the kernel's parameters against torch.optim.RMSprop in float64 fed the kernel's own
    gradients: at most half an ulp of the parameter plus 16 * 2^-24 * |delta p|; square_avg within 8 * 2^-24 of its terms."""
    in_dim = shape[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = trainer(desc, 1, 512, kind)
    params, sq = flat([pol]), torch.zeros((1, tr.n_params), device=DEV)
    ref = params[0].cpu().double().clone().requires_grad_(True)
    ropt = torch.optim.RMSprop([ref], weight_decay=weight_decay, momentum=0, centered=False, **OPT)
    opt = _capi.rmsprop_opt(weight_decay=weight_decay, **OPT)
    for i in range(3):
        obs, d_raw = data(1, 64, in_dim, 1 + desc.n_dist, 40 + i)
        before = params[0].cpu().double()
        # the float64 optimiser starts every step from the kernel's parameters, so only this step's arithmetic is compared
        # (its square_avg carries over on its own)
        with torch.no_grad():
            ref.copy_(before)
        sq_before = sq[0].cpu().double()
        _, grads = step(tr, params, obs.to(DEV), d_raw.to(DEV), opt, sq)
        ref.grad = grads[0].cpu().double()
        ropt.step()
        got, want = params[0].cpu(), ref.detach()
        bound = 0.5 * torch.from_numpy(np.spacing(np.abs(got.numpy()))).double() + 16 * U * (want - before).abs()
        err = (got.double() - want).abs()
        print(f"step {i} wd {weight_decay}: max err/bound {float((err / bound).max()):.3g}")
        assert torch.all(err <= bound) and not torch.equal(got.double(), before)
        # square_avg = alpha sq + (1 - alpha) g'^2 with g' = g + wd p rounded in float32: |g'| <= |g| + wd |p| bounds both terms' rounding
        sq_want = OPT["alpha"] * sq_before + (1 - OPT["alpha"]) * (ref.grad + weight_decay * before) ** 2
        sq_tol = 8 * U * (OPT["alpha"] * sq_before + (1 - OPT["alpha"]) * (ref.grad.abs() + weight_decay * before.abs()) ** 2)
        assert torch.all((sq[0].cpu().double() - sq_want).abs() <= sq_tol)
    tr.close()


def check_optimiser_step_given_gradient(shape, kind, pol, form, label):
    """The LayerNorm kinds' form of the check above, ``form`` "fused_rmsprop" or "deferred_adam" with weight decay 1e-4: three
    consecutive steps; after each, every parameter (gamma and beta included) against torch's optimiser in float64 fed the kernel's own
    gradients and started from the kernel's parameters and state: at most half an ulp of the parameter plus 16 * 2^-24 * |delta p|;
    and every tensor moved."""
    in_dim = shape[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = trainer(desc, 1, 512, kind)
    wd = 1e-4
    params = flat([pol])
    s0, s1 = torch.zeros_like(params), torch.zeros_like(params)   # square_avg | exp_avg_sq, exp_avg
    names = [n for n, _ in pol.named_parameters()]
    for i in range(3):
        obs, d_raw = (t.to(DEV) for t in data(1, 64, in_dim, 1 + desc.n_dist, 40 + i))
        before, b0, b1 = (t[0].cpu().double().clone() for t in (params, s0, s1))
        ref = before.clone().requires_grad_(True)
        if form == "fused_rmsprop":
            _, grads = step(tr, params, obs, d_raw, _capi.rmsprop_opt(weight_decay=wd, **OPT), s0)
            ropt = torch.optim.RMSprop([ref], weight_decay=wd, momentum=0, centered=False, foreach=False, **OPT)
            ropt.state[ref] = {"step": torch.tensor(float(i)), "square_avg": b0.clone()}
        else:
            _, grads, _ = step_opt(tr, params, obs, d_raw, lambda n: _capi.optim(
                "adam", ADAM["lr"], s0.data_ptr(), s1.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=wd, step=i))
            ropt = torch.optim.Adam([ref], weight_decay=wd, amsgrad=False, foreach=False, **ADAM)
            if i:
                ropt.state[ref] = {"step": torch.tensor(float(i)), "exp_avg": b1.clone(), "exp_avg_sq": b0.clone()}
        ref.grad = grads[0].cpu().double()
        ropt.step()
        got, want = params[0].cpu(), ref.detach()
        bound = 0.5 * torch.from_numpy(np.spacing(np.abs(got.numpy()))).double() + 16 * U * (want - before).abs()
        err = (got.double() - want).abs()
        print(f"{label} {form} step {i}: max err/bound {float((err / bound).max()):.3g}")
        assert torch.all(err <= bound)
        off = 0
        for name, n in zip(names, sizes(pol)):   # every tensor moved, gamma and beta among them
            assert not torch.equal(got[off:off + n].double(), before[off:off + n]), name
            off += n
    tr.close()


def check_adam_step_given_gradient(shape, kind, pol, weight_decay, steps, label, clip=0.0):
    """Consecutive deferred Adam steps at the step counts ``steps``; with ``clip`` (below the gradient's norm) the kernel also clips
    and hands back the norm, which must lie within one float32 ulp of the float64 one.  Truth: clip_grad_norm_ (with a clip) +
    torch.optim.Adam (single-tensor) in float64 on the CPU, fed the kernel's gradients and restarted every step from the kernel's
    parameters and state; yardstick: the same in float32 (against_yardstick's bound for params, exp_avg and exp_avg_sq).
    ``label`` is the printed lines' prefix with ``{step}`` in it."""
    in_dim = shape[0]
    desc = _capi.policy_tensors(pol)[0]
    tr = trainer(desc, 1, 512, kind)
    params = flat([pol])
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    fails = []
    for i, at in enumerate(steps):
        obs, d_raw = data(1, 64, in_dim, 1 + desc.n_dist, 40 + i)
        before = [t[0].cpu().clone() for t in (params, m, v)]
        _, grads, norms = step_opt(tr, params, obs.to(DEV), d_raw.to(DEV), lambda n: _capi.optim(
            "adam", ADAM["lr"], v.data_ptr(), m.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], weight_decay=weight_decay, grad_clip=clip,
            step=at, grad_norms=n if clip else None))
        if clip:
            want_norm = float(torch.sqrt((grads[0].cpu().double() ** 2).sum()))
            print(f"adam step {at}: kernel norm {float(norms[0])!r}, float64 {want_norm!r}, grad_clip {clip}")
            assert want_norm > clip and abs(float(norms[0]) - want_norm) <= float(np.spacing(np.float32(want_norm)))
        res = {}
        for dtype in (torch.float64, torch.float32):
            p = before[0].to(dtype).clone().requires_grad_(True)
            p.grad = grads[0].cpu().to(dtype)
            if clip:
                torch.nn.utils.clip_grad_norm_([p], clip)
            o = torch.optim.Adam([p], weight_decay=weight_decay, amsgrad=False, foreach=False, **ADAM)
            if at:
                o.state[p] = {"step": torch.tensor(float(at)), "exp_avg": before[1].to(dtype).clone(), "exp_avg_sq": before[2].to(dtype).clone()}
            o.step()
            assert float(o.state[p]["step"]) == at + 1
            res[dtype] = (p.detach(), o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"])
        for j, (name, got) in enumerate((("params", params), ("exp_avg", m), ("exp_avg_sq", v))):
            against_yardstick(f"{label.format(step=at)} {name}", got[0].cpu(), res[torch.float64][j], res[torch.float32][j], sizes(pol), fails)
        assert not torch.equal(params[0].cpu(), before[0])
    tr.close()
    assert not fails, fails


def pick_nt(row_tiles, tiles, K):
    """pick_nt of dispatch_train_wide.hip, restated: what the wider-strip cases rely on to reach strips of 2 and 4 tiles."""
    for nt in (4, 2):
        if row_tiles * -(-tiles // nt) * K >= 2048:
            return nt
    return 1


def check_strip_rule_of_the_cases():
    """The arithmetic of the comment above check_wider_strips (if the rule in the launch code moves, the cases have to move with it)."""
    assert (pick_nt(8, 33, 16), pick_nt(8, 17, 16), pick_nt(17, 33, 16)) == (2, 1, 4)
    assert (pick_nt(32, 33, 16), pick_nt(32, 17, 16)) == (4, 4)
    assert (pick_nt(17, 33, 8), pick_nt(8, 33, 8), pick_nt(8, 17, 8)) == (2, 1, 1)
    assert max(pick_nt(mt, t, 1) for mt in (8, 32, 17) for t in (33, 17)) == 1


# The wide launches take strips of NT = 1, 2 or 4 tiles (dispatch_train_wide.hip: pick_nt, the widest NT with row tiles * ceil(tiles / NT)
# * K >= 2048 strips, else 1), and the other cases, K <= 3 and B <= 128, all run NT = 1.  W5 = [528, 272] has 33 and 17 tiles, so every
# strip row of 2 or 4 tiles ends in a partial strip of 1.  With 8 row tiles at B = 128 and 32 at B = 512 (forward and (a), G's store with
# LayerNorm, over the layer's width; (b) of layer 1 over 17 row tiles x 33 tiles):
#   K = 16, B = 128: forward of layer 0 and (a) of layer 1  8 * 17 * 16 = 2176 -> NT = 2;  (b) of layer 1  17 * 9 * 16 = 2448 -> NT = 4
#   K = 16, B = 512: forward of both layers and both (a)    32 * 9 * 16, 32 * 5 * 16 -> NT = 4;  (b) of layer 1 NT = 4
#   K =  8, B = 128: (b) of layer 1  17 * 9 * 8 = 1224, 17 * 17 * 8 = 2312 -> NT = 2;  everything else NT = 1
# A K = 1 trainer runs NT = 1 everywhere at both batch sizes (at most 32 * 33 = 1056 strips).
def check_wider_strips(kind, pols, B, nets, grad_clip):
    """Strips of 2 and 4 tiles with a partial last strip in the forward, (a) and (b) launches: the nets ``nets`` of the K-net W5 trainer
    equal the K = 1 trainer (strips of one tile) on their data bit for bit, in the fused and the deferred form.  Returns the K-net
    result and the CPU inputs."""
    K = len(pols)
    desc = _capi.policy_tensors(pols[0])[0]
    obs_c, d_raw_c = data(K, B, W5[0], 1 + desc.n_dist, 7)
    obs, d_raw = obs_c.to(DEV), d_raw_c.to(DEV)
    tr = trainer(desc, K, 512, kind)
    got = run_forms(tr, pols, obs, d_raw, grad_clip)
    tr.close()
    sane(got, pols)
    tr1 = trainer(desc, 1, 512, kind)
    for k in nets:
        one = run_forms(tr1, pols[k:k + 1], obs[k:k + 1].contiguous(), d_raw[k:k + 1].contiguous(), grad_clip)
        same_net(got, one, k, f"K = {K} and K = 1 differ")
    tr1.close()
    return got, obs_c, d_raw_c


# ------------------------------------------------------------------------------------------------ end to end
def e2e_agents(kind, K):
    """(the default configuration of ``kind`` on the GPU, K agents whose weights come from torch.manual_seed(70 + k))"""
    from alphazero_gym_amd.envs import make_game
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, dict(device=DEV))
    env = make_game(cfg["game"])
    agents = []
    for k in range(K):
        torch.manual_seed(70 + k)
        agents.append(run.make_agent(kind, cfg, env, tree_id_base=k))
    return cfg, agents


def twin(kind, cfg, agent, device, dtype=torch.float32):
    """A new agent with ``agent``'s weights (the agents here have taken no optimiser step yet, so their optimisers and learned
    temperatures are as new; a tuned loss holds a non-leaf alpha, which copy.deepcopy refuses)."""
    from alphazero_gym_amd.envs import make_game
    a = run.make_agent(kind, dict(cfg, device=device), make_game(cfg["game"]))
    a.nn.load_state_dict({k: v.detach().to(device) for k, v in agent.nn.state_dict().items()})
    a.nn.to(dtype)
    return a


def update_f64(kind, cfg, agent, batch):
    """The agent's loss dictionary in float64 on the CPU."""
    a = twin(kind, cfg, agent, "cpu", torch.float64)
    s, ac, c, _, v = (x.detach().cpu().double() for x in batch)
    d = a._loss(s, ac, c, v.reshape(-1, 1))
    return {k: float(x.detach()) if hasattr(x, "detach") else float(x) for k, x in d.items()}


def split_rows(rows, S, A):
    """Replay rows [..., S + 3 A + 1] as the batch tuple (obs, actions, counts, Q, V)."""
    return (rows[..., :S], rows[..., S:S + A], rows[..., S + A:S + 2 * A], rows[..., S + 2 * A:S + 3 * A], rows[..., -1])


def batches(rows, S, A):
    return [split_rows(r, S, A) for r in rows]


# ------------------------------------------------------------------------------------------------ small hand-made populations
LOSSES = {
    "alphazero": dict(_target_="alphazero_gym_amd.agent.losses.AlphaZeroLoss", policy_coeff=1.0, value_coeff=0.5, reduction="mean"),
    "a0c": dict(_target_="alphazero_gym_amd.agent.losses.A0CLoss", tau=0.1, policy_coeff=0.1, alpha=0.05, value_coeff=1.0, reduction="mean"),
    "a0c_tuned": run.LOSS_TUNED,
}
RMSPROP_WD = dict(run.RMSPROP, weight_decay=1e-4)
ADAM_WD = dict(run.ADAM, weight_decay=1e-4)
# head: (observations, actions per row)
DIMS = {"discrete": (4, 2), "gmm2": (3, 4)}


def make_agents(head, loss, K, first_seed=0, optimizer=RMSPROP_WD, clip=None):
    """K GPU agents; net k's initial weights come from torch.manual_seed(first_seed + k): two calls give identical populations.
    ``clip`` replaces the default configuration's grad_clip."""
    loss_cfg = dict(LOSSES[loss], device=DEV) if loss == "a0c_tuned" else LOSSES[loss]
    agents = []
    for k in range(K):
        torch.manual_seed(first_seed + k)
        cfg = run.DISCRETE_DEFAULTS if head == "discrete" else run.CONTINUOUS_DEFAULTS
        extra = cfg["agent"] if clip is None else dict(cfg["agent"], grad_clip=clip)
        if head == "discrete":   # 4 inputs, [32, 32], 2 actions, ReLU
            pol = dict(cfg["policy"], hidden_dimensions=[32, 32], representation_dim=4, action_dim=1, num_actions=2)
            agents.append(DiscreteAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=DEV, num_actions=2), loss_cfg=loss_cfg,
                                        optimizer_cfg=optimizer, device=DEV, **extra))
        else:                    # 3 inputs, [32, 16], a mixture of 2, ELU
            pol = dict(cfg["policy"], hidden_dimensions=[32, 16], representation_dim=3, action_dim=1, action_bound=2.0, num_components=2)
            agents.append(ContinuousAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=DEV), loss_cfg=loss_cfg,
                                          optimizer_cfg=optimizer, device=DEV, **extra))
    return agents


def make_rows(head, K, n, seed):
    """[K, n, row] float32 on the GPU: obs | actions[A] | counts[A] | Q[A] | V."""
    S, A = DIMS[head]
    rng = np.random.RandomState(seed)
    obs = rng.randn(K, n, S)
    if head == "discrete":
        actions, counts = np.tile(np.arange(A, dtype=np.float64), (K, n, 1)), rng.randint(0, 9, (K, n, A))
    else:
        actions, counts = rng.uniform(-1.9, 1.9, (K, n, A)), rng.randint(1, 9, (K, n, A))
    q = rng.randn(K, n, A)
    v = rng.randn(K, n, 1)
    return torch.from_numpy(np.concatenate([obs, actions, counts, q, v], axis=-1).astype(np.float32)).to(DEV)


def state_of(tr):
    """Everything an epoch of an RMSprop PopulationTrainer may change, as CPU copies."""
    s = {"flat": tr.flat, "square_avg": tr.square_avg}
    if tr.log_alpha is not None:
        s.update(log_alpha=tr.log_alpha, alpha_exp_avg=tr.alpha_exp_avg, alpha_exp_avg_sq=tr.alpha_exp_avg_sq)
    out = {k: v.detach().cpu().clone() for k, v in s.items()}
    out["alpha_step"] = torch.tensor(tr.alpha_step)
    return out


def state_of_agents_optimisers(tr, rows_of_d_raw=None):
    """state_of for PopulationTrainer(optimizers="agents") with Adam and a tuned loss: Adam's moments, the gradient norms and both
    step counts in place of square_avg (and the d_raw the native trainer holds)."""
    s = dict(flat=tr.flat, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq, log_alpha=tr.log_alpha, alpha_exp_avg=tr.alpha_exp_avg,
             alpha_exp_avg_sq=tr.alpha_exp_avg_sq, grad_norms=tr.last_grad_norms)
    out = {k: v.detach().cpu().clone() for k, v in s.items()}
    out["steps"] = torch.tensor([tr.alpha_step, tr.opt_step])
    if rows_of_d_raw:
        d = torch.empty((len(tr.agents), rows_of_d_raw, tr.trainer.n_raw), device=DEV)
        torch.cuda.synchronize()
        tr.trainer.read_d_raw(rows_of_d_raw, d.data_ptr())
        out["d_raw"] = d.cpu()
    return out


def assert_same(a, b, what, nets=None):
    """Two state dictionaries hold the same bits; with ``nets`` = (i, j), net i of a and net j of b."""
    assert set(a) == set(b)
    for name in a:
        x, y = a[name], b[name]
        if nets is not None and x.dim() > 0:
            x, y = x[nets[0]], y[nets[1]]
        assert torch.equal(x, y), f"{what}: {name} differs"


# ------------------------------------------------------------------------------------------------ the host files' CPU agents
# HOST_ROWS is a multiple of 16, the float32 lanes of the widest CPU vector unit: torch's CPU kernels compute an element in their vector
# body or in their scalar tail depending on where it sits in the tensor, and the two differ in the last bit of exp / log.  With whole
# vectors per net, an element of net k is computed the same way in the agent's [B, ...] tensors and in the population's [K * B, ...].
HOST_ROWS, HOST_ACTIONS = 32, 5
HOST_HEADS = {"discrete": dict(), "normal": dict(num_components=1), "gmm2": dict(num_components=2)}


def make_agent(head, loss="a0c_tuned", seed=0, hidden=(32, 32), layernorm=False, optimizer=None, grad_clip=0, device="cpu"):
    torch.manual_seed(seed)
    opt = optimizer or run.RMSPROP
    if head == "discrete":
        cfg = run.DISCRETE_DEFAULTS
        pol = dict(cfg["policy"], hidden_dimensions=list(hidden), representation_dim=4, action_dim=1, num_actions=HOST_ACTIONS,
                   layernorm=layernorm)
        return DiscreteAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=device, num_actions=HOST_ACTIONS), loss_cfg=LOSSES[loss],
                             optimizer_cfg=opt, device=device, **dict(cfg["agent"], grad_clip=grad_clip))
    cfg = run.CONTINUOUS_DEFAULTS
    pol = dict(cfg["policy"], hidden_dimensions=list(hidden), representation_dim=3, action_dim=1, action_bound=2.0, layernorm=layernorm,
               **HOST_HEADS[head])
    return ContinuousAgent(policy_cfg=pol, mcts_cfg=dict(cfg["mcts"], device=device), loss_cfg=LOSSES[loss], optimizer_cfg=opt,
                           device=device, **dict(cfg["agent"], grad_clip=grad_clip))


def make_batch(head, seed):
    """(states, actions, counts, values) of HOST_ROWS rows for a make_agent(head) agent, as numpy float32."""
    B, A = HOST_ROWS, HOST_ACTIONS
    rng = np.random.RandomState(seed)
    if head == "discrete":
        states = rng.randn(B, 4).astype(np.float32)
        actions = np.tile(np.arange(A, dtype=np.float32), (B, 1))
    else:
        states = rng.randn(B, 3).astype(np.float32)
        actions = rng.uniform(-1.9, 1.9, (B, A)).astype(np.float32)
    counts = rng.randint(0 if head == "discrete" else 1, 9, (B, A)).astype(np.float32)
    values = rng.randn(B).astype(np.float32)
    return states, actions, counts, values


def normal_agent(seed=0, hidden=(512, 272), layernorm=False, optimizer=None, grad_clip=0):
    """make_agent's Normal-head, tuned-loss agent with the seed first: the layernorm, wide and wide_layernorm host files' agent,
    each with its own defaults for ``hidden`` and ``layernorm`` (functools.partial)."""
    return make_agent("normal", seed=seed, hidden=hidden, layernorm=layernorm, optimizer=optimizer, grad_clip=grad_clip)


def refused(agents, reason, **kw):
    """PopulationTrainer(agents, **kw) raises a ValueError naming ``reason`` and leaves the agents as they were: the same values in the
    same storage, and optimisers without state."""
    from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
    before = copy.deepcopy([a.nn.state_dict() for a in agents])
    ptrs = [[p.data_ptr() for p in a.nn.parameters()] for a in agents]
    with pytest.raises(ValueError, match=re.escape(reason)):
        PopulationTrainer(agents, **kw)
    for a, sd, pp in zip(agents, before, ptrs):
        now = a.nn.state_dict()
        assert list(now) == list(sd) and all(torch.equal(now[name], sd[name]) for name in sd)
        assert [p.data_ptr() for p in a.nn.parameters()] == pp and not a.optimizer.state
