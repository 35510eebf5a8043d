"""CPU: the tables and networks of trainer_edges.py are what they claim to be.  For every table the float64 reference
(population_loss, or float64 autograd on the policy) is finite and so is its float32 cast, and each edge a table is about occurs in
it, asserted on the reference.  The reference itself is pinned at the squash's pole against a 50-digit restatement."""
import numpy as np
import pytest
import torch

import trainer_edges as E
import trainer_util as TU
from device_loss_util import LOG_ALPHA0, make_loss, torch_loss

F32_MAX = float(np.finfo(np.float32).max)


def _reference(head, loss_name, reduction):
    policy = E.head_policy(head)
    tuned = loss_name == "a0c_tuned"
    la = torch.tensor(LOG_ALPHA0[:2], dtype=torch.float64, requires_grad=True) if tuned else None
    return policy, torch_loss(policy, make_loss(loss_name, reduction), E.table(head), torch.float64, la)


def _finite_in_float32(x):
    return bool(torch.isfinite(x).all()) and bool(torch.isfinite(x.float()).all()) and float(x.abs().max()) <= F32_MAX


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("loss_name", ["a0c", "a0c_tuned"])
@pytest.mark.parametrize("head", list(E.CONT_HEADS))
def test_continuous_table(head, loss_name, reduction):
    C, A = E.CONT_HEADS[head]
    t = E.continuous_table(head)
    raw, actions, counts = t["raw"], t["actions"], t["counts"]
    assert raw.shape[2] == 1 + (2 if C == 1 else 3 * C) and actions.shape == counts.shape == raw.shape[:2] + (A,)
    policy, (truth, g64) = _reference(head, loss_name, reduction)
    assert _finite_in_float32(g64) and all(_finite_in_float32(v) for v in truth.values())
    # the ingredients
    for k in range(2):
        have = set(np.float32(actions[k].numpy()).view(np.uint32).ravel().tolist())
        for a in (E.BOUND, -E.BOUND, E.B_IN, E.NB_IN, 0.0, -0.0, 0.5):
            assert int(np.float32(-a if k else a).view(np.uint32)) in have, a     # (net 1 is the mirror image)
        assert abs(E.B_IN) < E.BOUND and abs(E.NB_IN) < E.BOUND
        assert {1.0, 25.0} <= set(counts[k].ravel().tolist()) and float(t["values"][k].abs().max()) == (1e6, 2.5e5)[k]
        mus = set(raw[k, :, 1:1 + C].ravel().tolist())
        assert {0.0, E.MU_HI, E.MU_LO} <= mus or {0.0, -E.MU_HI, -E.MU_LO} <= mus
        dx0 = (raw[k, :, 1] == 0) & (actions[k] == 0).any(dim=1)     # mu on the exact pre-image of an action of its row
        assert bool(dx0.any())
    # the clamp's gate: true on the ends and one step inside, false one step outside and beyond
    cols = E.log_std_columns(head)
    ls = raw[..., cols]
    mask = (ls >= policy.log_param_min) & (ls <= policy.log_param_max)
    assert torch.equal(mask, t["gate"])
    for v, want in zip(E.LS_LOW + E.LS_HIGH, E.LS_GATE + E.LS_GATE):
        at = ls == v
        assert bool(at.any()) and bool((mask[at] == want).all()), v
    assert E.LS_LOW[2] < E.LMIN == E.LS_LOW[0] < E.LS_LOW[1] and E.LS_HIGH[1] < E.LMAX == E.LS_HIGH[0] < E.LS_HIGH[2]
    # ... and the float64 gradient is zero exactly where the gate is closed (float32 rounding turns no open element into 0)
    assert torch.equal(g64[..., cols] == 0, ~mask)
    assert torch.equal(g64[..., cols].float() == 0, ~mask)
    if C > 1:
        share = torch.softmax(raw[..., 1 + 2 * C:].double(), dim=-1)
        for k in range(2):
            pats = t["pattern"][k]
            assert {"equal", "far", "gone", "interior"} <= set(pats)
            for b, p in enumerate(pats):
                s = share[k, b]
                if p == "gone":
                    assert float(s.min()) == 0.0
                elif p == "far":
                    assert 0.0 < float(s.min()) < 1e-30
                elif p == "equal":
                    assert bool((s == s[0]).all())
            assert any(p == "far" and float(share[k, b].max()) == 1.0 for b, p in enumerate(pats))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("loss_name", ["alphazero", "a0c", "a0c_tuned"])
@pytest.mark.parametrize("head", list(E.DISCRETE_HEADS))
def test_discrete_table(head, loss_name, reduction):
    n = E.DISCRETE_HEADS[head]
    t = E.discrete_table(head)
    _, (truth, g64) = _reference(head, loss_name, reduction)
    assert _finite_in_float32(g64) and all(_finite_in_float32(v) for v in truth.values())
    assert bool((t["actions"] == torch.arange(n, dtype=torch.float32)).all())
    prob = torch.softmax(t["raw"][..., 1:].double(), dim=-1)
    for k in range(2):
        for b, (lp, cp) in enumerate(zip(t["logit_pattern"][k], t["count_pattern"][k])):
            p, c = prob[k, b], t["counts"][k, b]
            if lp == "gone":
                assert float(p.min()) == 0.0 and float(p.max()) == 1.0
            elif lp == "far":
                assert 0.0 < float(p.min()) < 1e-30
            elif lp == "equal":
                assert bool((p == p[0]).all())
            if cp == "zero":
                assert bool((c == 0).all())
            elif cp == "tied":
                assert int((c == c.max()).sum()) == 2 and (n == 2 or int(c.argmax()) > 0)
            elif cp == "big":
                assert float(c.max()) == 2.0 ** 24
        assert set(zip(t["logit_pattern"][k], t["count_pattern"][k])) == {(a, b) for a in E.LOGIT_PATTERNS for b in E.COUNT_PATTERNS}


@pytest.mark.parametrize("act", E.ACTIVATIONS)
def test_kink_net(act):
    """In a float32 CPU forward pass Z of units 0-15 of both hidden layers is the bias bit for bit (a -0.0 bias: +-0, since
    -0 + +0 = +0 and the zero products have either sign), and float64 autograd is finite."""
    pol = E.kink_net(act)
    obs, d_raw = E.kink_data()
    assert obs.shape == (18, 4) and bool((obs[17] == 0).all()) and bool((obs[:17] != 0).all())
    table = E.kink_table(act)
    want = {"relu6": [6.0], "hardswish": [3.0, -3.0]}.get(act, []) + [0.0]
    for v in want:
        for x in (v, E.nxt(v, E.INF), E.nxt(v, -E.INF)):
            assert np.float32(x) in table, x
    assert np.signbit(table[1]) and table[1] == 0 and not np.signbit(table[0])
    for s in (20.0, 88.0, 104.0):
        assert s in table and -s in table
    with torch.no_grad():
        z1 = pol.trunk[0](obs)
        z2 = pol.trunk[2](pol.trunk[1](z1))
    signed = np.arange(E.KINK_UNITS) != 1
    for z in (z1, z2):
        zk = z[:, :E.KINK_UNITS].numpy()
        assert (zk[:, signed].view(np.uint32) == table[signed].view(np.uint32)).all()
        assert (zk[:, 1] == 0).all()
    for dtype in (torch.float64, torch.float32):
        assert all(bool(torch.isfinite(g).all()) for g in TU.autograd(pol, obs, d_raw, dtype))
    # the zero pattern of float64's bias gradients on the kink units is the derivative's
    g64 = TU.autograd(pol, obs, d_raw, torch.float64)
    zero = E.dact64(act, table) == 0
    for db in (g64[1], g64[3]):
        assert ((db[:E.KINK_UNITS].numpy() == 0) == zero).all()
    if act in ("relu", "relu6"):
        assert zero.sum() >= 6


@pytest.mark.parametrize("act", E.ACTIVATIONS)
def test_kink_conventions_are_autograd_s(act):
    """trainer_edges.dact64 restates act' with torch's conventions: on the kink table, float64 autograd through the activation's
    module gives it (bit for bit for the piecewise-linear ones, to 1e-15 of the derivative's scale for ELU and SiLU), and float32
    autograd has the same zeros on every unit of representable_derivative.  The conventions themselves, stated once: ReLU' (+-0) =
    0, LeakyReLU' (+-0) = 0.01, ELU' (+-0) = 1, ReLU6' (0) = ReLU6' (6) = 0, Hardswish' (-3) = 0 and Hardswish' (3) = 1 (the inner
    neighbours: -0.5 + 2^-24 / 3 and 1.5 - 2^-23 / 3)."""
    from alphazero_gym_amd.network.policies import _ACTIVATIONS
    table = E.kink_table(act)
    want = E.dact64(act, table)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        x = torch.from_numpy(table).to(dtype).requires_grad_(True)
        _ACTIVATIONS[act]()(x).sum().backward()
        grads[dtype] = x.grad.double().numpy()
    if act in ("elu", "silu"):
        assert np.abs(grads[torch.float64] - want).max() <= 1e-15
    else:
        assert (grads[torch.float64] == want).all()
    rep = E.representable_derivative(act)
    assert ((grads[torch.float32] == 0) == (want == 0))[rep].all()
    at = lambda v: want[list(table.view(np.uint32)).index(np.float32(v).view(np.uint32))]
    expect = {"relu": {0.0: 0.0, -0.0: 0.0, E.SUB: 1.0}, "leakyrelu": {0.0: 0.01, -0.0: 0.01, E.SUB: 1.0, -E.SUB: 0.01},
              "elu": {0.0: 1.0, -0.0: 1.0}, "relu6": {0.0: 0.0, E.SUB: 1.0, 6.0: 0.0, E.nxt(6.0, 0.0): 1.0, E.nxt(6.0, E.INF): 0.0},
              "silu": {0.0: 0.5, 104.0: 1.0},
              "hardswish": {-3.0: 0.0, 3.0: 1.0, E.nxt(-3.0, -E.INF): 0.0, E.nxt(3.0, E.INF): 1.0, 0.0: 0.5}}[act]
    for v, d in expect.items():
        assert at(v) == d, (v, at(v), d)
    if act == "hardswish":
        assert abs(at(E.nxt(-3.0, 0.0)) + 0.5) < 1e-6 and abs(at(E.nxt(3.0, 0.0)) - 1.5) < 1e-6


def test_layernorm_net():
    pol = E.layernorm_net()
    obs, d_raw = E.layernorm_data()
    assert bool((pol.trunk[0].bias <= 0).all()) and bool((obs[E.LN_ZERO_ROW] == 0).all())
    with torch.no_grad():
        a1 = pol.trunk[1](pol.trunk[0](obs))
    assert bool((a1[E.LN_ZERO_ROW] == 0).all())                       # a LayerNorm row of equal values: var == 0
    others = [r for r in range(obs.shape[0]) if r != E.LN_ZERO_ROW]
    assert bool((a1[others].var(dim=1) > 0).all())
    for dtype in (torch.float64, torch.float32):
        assert all(bool(torch.isfinite(g).all()) for g in TU.autograd(pol, obs, d_raw, dtype))


# ------------------------------------------------------------------------------------------------ the reference at the pole
PIN_BOUND = 2.0 ** -32


def squashed_normal_pin():
    """The largest |float64 PyTorch - 50-digit value| of the squashed Normal's log-probability derivatives by mu and log sigma over
    the normal table's (row, action) pairs, in units of the row's largest derivative; and the same for the log-probability itself
    in units of the row's largest |log-probability|."""
    import mpmath as mp
    mp.mp.dps = 50
    t = E.continuous_table("normal")
    policy = E.head_policy("normal")
    raw, actions = t["raw"].double().reshape(-1, 3), t["actions"].double().reshape(-1, 8)
    mu = raw[:, 1:2].expand(-1, 8).clone().requires_grad_(True)
    ls = raw[:, 2:3].expand(-1, 8).clone().requires_grad_(True)
    lp = policy._dist(mu, torch.clamp(ls, min=policy.log_param_min, max=policy.log_param_max).exp()).log_prob(actions)
    lp.sum().backward()
    lp = lp.detach()
    worst_d, worst_lp = 0.0, 0.0
    b, eps = mp.mpf(E.BOUND), mp.mpf(1e-6)
    for r in range(raw.shape[0]):
        m, l = mp.mpf(float(raw[r, 1])), mp.mpf(float(raw[r, 2]))
        open_ = policy.log_param_min <= l <= policy.log_param_max
        lc = min(max(l, mp.mpf(policy.log_param_min)), mp.mpf(policy.log_param_max))
        rows_d, rows_lp = [], []
        for i in range(8):
            x = mp.atanh(mp.mpf(float(actions[r, i])) / (b + eps))
            cx = (1 + eps / b) * x
            ladj = 8 * mp.log(b) + 2 * (mp.log(2) - cx - mp.log1p(mp.exp(-2 * cx)))
            q = (x - m) ** 2 * mp.exp(-2 * lc)
            rows_lp.append((-q / 2 - lc - mp.log(mp.sqrt(2 * mp.pi)) - ladj, float(lp[r, i])))
            rows_d.append(((x - m) * mp.exp(-2 * lc), float(mu.grad[r, i])))
            rows_d.append(((q - 1) if open_ else mp.mpf(0), float(ls.grad[r, i])))
        scale_d, scale_lp = max(abs(w) for w, _ in rows_d), max(abs(w) for w, _ in rows_lp)
        worst_d = max(worst_d, max(float(abs(mp.mpf(g) - w) / scale_d) for w, g in rows_d))
        worst_lp = max(worst_lp, max(float(abs(mp.mpf(g) - w) / scale_lp) for w, g in rows_lp))
    return worst_d, worst_lp


def test_reference_at_the_pole():
    """float64 PyTorch's squashed-Normal log-probability and its derivatives on the normal table against network/distributions.py
    restated at 50 digits: within 2^-32 of the row's largest.  (atanh at y = bound / (bound + 1e-6) has absolute conditioning
    1 / (1 - y^2), about 1e6, so the 2^-53 of y's rounding grows to about 1e-10, 2^-34 of x = 7.6.)  The device tests allow the
    reference 2^-30: four times this."""
    worst_d, worst_lp = squashed_normal_pin()
    print(f"squashed Normal pin: derivatives {worst_d:.3g} (2^{np.log2(worst_d):.1f}), log-probability {worst_lp:.3g} of the row's largest")
    assert worst_d <= PIN_BOUND and worst_lp <= PIN_BOUND
