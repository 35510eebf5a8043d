"""GPU: the population trainer's network kernels at the edges of their inputs (trainer_edges.py): every hidden pre-activation of
sixteen units on a kink of the activation's derivative, dead units and an all-zero d_raw through the optimisers, a LayerNorm row of
equal values, and 257 rows (17 tiles, the last with one live row) through the forms that the other files stop at 128 rows."""
import numpy as np
import pytest
import torch

import trainer_edges as E
import trainer_util as TU
from alphazero_gym_amd import _capi
from alphazero_gym_amd.network.policies import make_policy
from trainer_util import ADAM, DEV, OPT

pytestmark = pytest.mark.gpu


def _fused(tr, pol, obs, d_raw, sq0=0.0):
    """forward + backward_step (RMSprop, no weight decay): CPU copies of (grads, params, square_avg)."""
    params, sq = TU.flat([pol]), torch.full((1, tr.n_params), sq0, device=DEV)
    grads = torch.full_like(params, float("nan"))
    TU.forward(tr, params, obs)
    tr.backward_step(params.data_ptr(), d_raw.data_ptr(), obs.shape[1], _capi.rmsprop_opt(**OPT), sq.data_ptr(), grads.data_ptr())
    return grads[0].cpu(), params[0].cpu(), sq[0].cpu()


def _deferred(tr, pol, obs, d_raw, kind, clip=0.0, m0=0.0, v0=0.0):
    """forward + backward_step_opt with grad_norms: CPU copies of (grads, params, state0 = square_avg | exp_avg_sq, exp_avg, norm)."""
    params = TU.flat([pol])
    s0, s1 = torch.full((1, tr.n_params), v0, device=DEV), torch.full((1, tr.n_params), m0, device=DEV)
    grads, norms = torch.full_like(params, float("nan")), torch.full((1,), -1.0, device=DEV)
    TU.forward(tr, params, obs)
    if kind == "adam":
        opt = _capi.optim("adam", ADAM["lr"], s0.data_ptr(), s1.data_ptr(), eps=ADAM["eps"], betas=ADAM["betas"], grad_clip=clip,
                          grad_norms=norms.data_ptr())
    else:
        opt = _capi.optim("rmsprop", OPT["lr"], s0.data_ptr(), alpha=OPT["alpha"], eps=OPT["eps"], grad_clip=clip, grad_norms=norms.data_ptr())
    tr.backward_step_opt(params.data_ptr(), d_raw.data_ptr(), obs.shape[1], opt, grads.data_ptr())
    return grads[0].cpu(), params[0].cpu(), s0[0].cpu(), s1[0].cpu(), float(norms[0])


def _dev(obs, d_raw):
    return obs[None].to(DEV).contiguous(), d_raw[None].to(DEV).contiguous()


def _per_tensor(pol, flat):
    out, off = [], 0
    for t in _capi.policy_tensors(pol)[1]:
        out.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    assert off == flat.numel()
    return out


def _hold_to_autograd(tag, pol, grads, g64, g32, factor=4.0):
    """test_gradients_against_autograd's rule: per parameter tensor max|g - g64| / max|g64| at most ``factor`` x float32 autograd's;
    a tensor whose float64 gradient is identically 0 (no scale to divide by) must be identically 0."""
    assert torch.isfinite(grads).all()
    names = [n for n, _ in pol.named_parameters()]
    fails = []
    for name, gk, a64, a32 in zip(names, _per_tensor(pol, grads), g64, g32):
        scale = float(a64.abs().max())
        if scale == 0.0:
            assert bool((gk == 0).all()), name
            continue
        e32, ek = float((a32.double() - a64).abs().max()) / scale, float((gk.double() - a64).abs().max()) / scale
        print(f"{tag} {name}: float32 autograd error {e32:.3g}, kernel error {ek:.3g}")
        if not ek <= factor * e32:
            fails.append((name, e32, ek))
    assert not fails, (tag, fails)


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the kinks of act'
@pytest.mark.parametrize("act", E.ACTIVATIONS)
def test_kink_nets(act):
    """The first trainer's fused form, its deferred form and the wide trainer on a net whose units 0-15 of both hidden layers sit on
    trainer_edges.kink_table(act) for every row.  Gradients against float64 autograd per tensor; the bias gradient of a kink unit
    is zero exactly where float64's is (ReLU at +-0, ReLU6 at 0 and 6, Hardswish at and below -3), so at ELU's and LeakyReLU's 0
    and one float32 step inside Hardswish's +-3 it is not, and there the tensor's tolerance holds it to float64's derivatives 1,
    0.01, -0.5 and 1.5 (torch's own value at -3 is 0 and at 3 is 1: test_trainer_edges_host.py); the three forms give the same bits."""
    N = TU.native()
    pol = E.kink_net(act)
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = E.kink_data()
    g64, g32 = TU.autograd(pol, obs, d_raw, torch.float64), TU.autograd(pol, obs, d_raw, torch.float32)
    o, d = _dev(obs, d_raw)
    tr = N.HipTrainer(desc, 1, 32)
    fused = _fused(tr, pol, o, d)
    deferred = _deferred(tr, pol, o, d, "rmsprop")
    tr.close()
    tw = N.HipTrainer(desc, 1, 32, wide=True)
    wide = _fused(tw, pol, o, d)
    tw.close()
    _hold_to_autograd(f"kink {act}", pol, fused[0], g64, g32)
    rep = torch.from_numpy(E.representable_derivative(act))
    want_zero = torch.from_numpy(E.dact64(act, E.kink_table(act)) == 0)
    got = _per_tensor(pol, fused[0])
    for layer, i in enumerate((1, 3)):
        db, db64 = got[i][:E.KINK_UNITS], g64[i][:E.KINK_UNITS]
        assert torch.equal(db64 == 0, want_zero), layer                     # (the CPU test's)
        assert torch.equal((db == 0)[rep], want_zero[rep]), (act, layer, db, db64)
    assert torch.equal(_bits(fused[0]), _bits(deferred[0])), "the deferred form's gradients differ from the fused form's"
    for a, b, name in zip(fused, deferred[:3], ("grads", "params", "square_avg")):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: deferred RMSprop and the fused form differ"
    for a, b, name in zip(fused, wide, ("grads", "params", "square_avg")):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: the wide trainer's bits differ"


# ------------------------------------------------------------------------------------------------ zero gradients, zero norms
@pytest.mark.parametrize("wide", [False, True], ids=["first", "wide"])
def test_dead_rows_keep_their_bits(wide):
    """The ReLU kink net: nine units of either layer are dead for every row, so their weight rows, their biases, the next layer's
    columns that read them and the heads' have a gradient of exactly 0 in float64.  On the device those gradients are 0, and after one
    RMSprop step (weight_decay 0, square_avg 0) and one Adam step (both moments 0) those parameters keep their bits, their state
    stays 0 and nothing is NaN: 0 / (sqrt(0) + eps) is 0."""
    N = TU.native()
    pol = E.kink_net("relu")
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = E.kink_data()
    dead = torch.cat([g.reshape(-1) == 0 for g in TU.autograd(pol, obs, d_raw, torch.float64)])
    assert int(dead.sum()) >= 9 * 4 + 9 + 9 * 32 + 23 * 9 + 9 + 3 * 9 and not bool(dead.all())
    o, d = _dev(obs, d_raw)
    before = TU.flat([pol])[0].cpu()
    tr = N.HipTrainer(desc, 1, 32, wide=True) if wide else N.HipTrainer(desc, 1, 32)
    runs = {"fused rmsprop": _fused(tr, pol, o, d), "deferred rmsprop": _deferred(tr, pol, o, d, "rmsprop")[:3],
            "deferred adam": _deferred(tr, pol, o, d, "adam")[:4]}
    tr.close()
    for name, (grads, params, *state) in runs.items():
        assert all(torch.isfinite(t).all() for t in (grads, params, *state)), name
        assert bool((grads[dead] == 0).all()), name
        assert torch.equal(_bits(params)[dead], _bits(before)[dead]), f"{name}: a parameter with a zero gradient moved"
        assert bool((params[~dead] != before[~dead]).any()), name
        for s in state:
            assert bool((s[dead] == 0).all()) and bool((s[~dead] != 0).any()), name


@pytest.mark.parametrize("wide", [False, True], ids=["first", "wide"])
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_zero_d_raw_zero_norm(kind, wide):
    """An all-zero d_raw with grad_clip 1 and grad_norms: the norm is exactly 0, the clip coefficient min(1 / (0 + 1e-6), 1) is 1,
    no parameter moves and no state is NaN -- clip_grad_norm_'s own behaviour."""
    N = TU.native()
    pol = E.kink_net("relu")
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = E.kink_data()
    o, d = _dev(obs, torch.zeros_like(d_raw))
    tr = N.HipTrainer(desc, 1, 32, wide=True) if wide else N.HipTrainer(desc, 1, 32)
    grads, params, s0, s1, norm = _deferred(tr, pol, o, d, kind, clip=1.0)
    tr.close()
    assert norm == 0.0
    assert bool((grads == 0).all())
    assert torch.equal(_bits(params), _bits(TU.flat([pol])[0].cpu()))
    assert bool((s0 == 0).all()) and bool((s1 == 0).all())


# ------------------------------------------------------------------------------------------------ LayerNorm's constant row
@pytest.mark.parametrize("form", ["fused", "deferred"])
def test_layernorm_constant_row(form):
    """[48, 80] with LayerNorm, 17 rows of which one leaves every first-layer unit at 0 (var = 0, rstd = 1 / sqrt(1e-5), X = 0):
    every tensor's gradient, gamma's and beta's included, against float64 autograd by test_population_trainer_layernorm.py's rule,
    and everything finite."""
    N = TU.native()
    pol = E.layernorm_net()
    desc = _capi.policy_tensors(pol)[0]
    obs, d_raw = E.layernorm_data()
    g64, g32 = TU.autograd(pol, obs, d_raw, torch.float64), TU.autograd(pol, obs, d_raw, torch.float32)
    assert len(g64) == 12
    o, d = _dev(obs, d_raw)
    tr = N.HipTrainer(desc, 1, 32, layernorm=True)
    raw = TU.forward(tr, TU.flat([pol]), o)
    out = _fused(tr, pol, o, d) if form == "fused" else _deferred(tr, pol, o, d, "adam")[:4]
    tr.close()
    assert torch.isfinite(raw).all() and all(torch.isfinite(t).all() for t in out)
    _hold_to_autograd(f"LayerNorm constant row {form}", pol, out[0], g64, g32)
    assert not torch.equal(out[1], TU.flat([pol])[0].cpu())


# ------------------------------------------------------------------------------------------------ 257 rows
def _wide_policy():
    torch.manual_seed(971)
    return make_policy(3, 1, "normal", [528, 272], "elu", num_components=2, action_bound=2.0)


def _adam_policy():
    torch.manual_seed(972)
    return make_policy(4, 1, "discrete", [64, 32], "relu", num_actions=16)


ROWS_CASES = {
    # name: (policy, trainer keywords, run, the file's factor on float32 autograd's error)
    "layernorm_48x80_fused": (E.layernorm_net, dict(layernorm=True), lambda tr, pol, o, d: _fused(tr, pol, o, d, sq0=0.25), 4.0),
    "adam_clip_64x32_deferred": (_adam_policy, dict(), lambda tr, pol, o, d: _deferred(tr, pol, o, d, "adam", clip=1e-3, m0=0.01, v0=0.25), 4.0),
    "wide_528x272_fused": (_wide_policy, dict(wide=True), lambda tr, pol, o, d: _fused(tr, pol, o, d, sq0=0.25),
                           4.0 * float(np.sqrt(528 / 256.0))),
}


@pytest.mark.parametrize("case", list(ROWS_CASES))
def test_257_rows(case):
    """257 rows: gradients against float64 autograd by the form's own file's rule (the wide trainer's factor is 4 sqrt(528 / 256)).
    And rows 0-255 padded to 257 with a row whose d_raw is 0 give the 256-row call's gradients bit for bit (so the same step): the
    17th tile adds zeros to every chain."""
    N = TU.native()
    make, kw, run, factor = ROWS_CASES[case]
    pol = make()
    desc = _capi.policy_tensors(pol)[0]
    g = torch.Generator().manual_seed(79)
    obs = torch.randn((257, pol.state_dim), generator=g)
    d_raw = torch.randn((257, 1 + desc.n_dist), generator=g) / 257
    g64, g32 = TU.autograd(pol, obs, d_raw, torch.float64), TU.autograd(pol, obs, d_raw, torch.float32)
    padded = d_raw.clone()
    padded[256] = 0.0
    tr = N.HipTrainer(desc, 1, 512, **kw)
    full = run(tr, pol, *_dev(obs, d_raw))
    pad = run(tr, pol, *_dev(obs, padded))
    short = run(tr, pol, *_dev(obs[:256], d_raw[:256]))
    tr.close()
    _hold_to_autograd(f"257 rows {case}", pol, full[0], g64, g32, factor)
    if "adam" in case:
        want = float(torch.sqrt((full[0].double() ** 2).sum()))
        assert want > 1e-3 and abs(full[4] - want) <= float(np.spacing(np.float32(want)))       # large enough to clip
        assert pad[4] == short[4]
    names = ("grads", "params", "state0", "state1")
    for a, b, name in zip(pad[:4], short[:4], names):
        assert torch.equal(a, b), f"{name}: 256 rows and the same rows padded to 257 differ"
    assert not torch.equal(full[0], short[0]) and not torch.equal(short[1], TU.flat([pol])[0].cpu())
