"""Policy rollouts at the edges of the policy heads: hand-built networks whose head outputs are exact floats -- tied logits, a softmax
share of exactly 0 or 1, log sigma on and beside both clamps, a saturated squash, a head sum that depends on its order -- and two
bang-bang policies whose games terminate at many different steps.  Each case states its game, head and rule, builds its network for
any hidden shape, and carries a condition on the CPU rollout's trace (rollout_ref.cpu_rollout(trace=...)) that proves, without a GPU,
that the case contains what its name says.  tests/test_rollout_edges_host.py asserts the conditions; tests/test_rollout_edges.py
compares every kernel form with the CPU rollout bit for bit.  numpy and the CPU oracle only.

The nets are edge_values.net_blob's zero networks (ReLU trunks) with a chosen value bias, head biases and a few trunk / head weights.
Where a case needs signal from the trunk it comes from the first, the middle and the last TRUE unit of every layer (0, H // 2, H - 1),
carried through the later layers by unit weights: three different 64-unit slices of a wide layer (three workgroups of a team) and three
different chunks of the head's sum at every width.

Finite head outputs only.  azg_expf is specified for finite arguments (include/azg_math.h), so the largest logit gap here is
float32 max, where `x - max` is still finite; a gap that overflows to -inf is not an input of these kernels and is not built.

What IEEE arithmetic does to a bias of -0.0: a head output is `bias + chunk partials`, every partial of a zero row is +0.0, and
-0.0 + +0.0 = +0.0 (round to nearest).  So a -0.0 bias reaches the action rule, and first_value, as +0.0 -- on the CPU and on the
device alike -- and azg_tanhf(+-0.0) is +0.0.  The cases with a -0.0 bias assert exactly that."""
import functools

import numpy as np

import edge_values as E
import oracle_lib as O
import rollout_ref as R

G = 33                  # one full 32-game team (two full 16-game groups) and one game more
BASE = 1000             # game ids, as in the other rollout tests
ACT = "relu"
NARROW, STREAMED, WIDE, WIDE_1024 = (64, 64), (64, 64, 64, 64), (500, 500), (1024, 1024)
F32_MAX = E.F32_MAX
SUB = np.float32(np.finfo(np.float32).smallest_subnormal)
N_DIST = {"discrete": None, "normal": 2, "gmm2": 6}
BOUND = {"pendulum_v0": 2.0, "pendulum_v1": 2.0, "mcc": 1.0}
X = np.float32(1e30)


def f32_next(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def expf(x):
    """azg_expf(x) as float32 (the oracle's export of the shared math header)."""
    return np.float32(O.math_eval(0, np.array([float(np.float32(x))]))[0])


def ls_bounds(game, head):
    """(log_sigma_min, log_sigma_max) as float32, read from the descriptor the engines are given."""
    d = R.net_desc(game, NARROW, head, ACT)
    return np.float32(d.log_std_min), np.float32(d.log_std_max)


def clamp(ls, lo, hi):
    return lo if ls < lo else (hi if ls > hi else np.float32(ls))


def n_dist(game, head):
    return R.GAMES[game]["num_actions"] if head == "discrete" else N_DIST[head]


def signal_units(hidden):
    """The first, the middle and the last true unit of a layer (every layer of a case's net has the same width)."""
    assert len(set(hidden)) == 1
    H = hidden[0]
    return 0, H // 2, H - 1


def carried(hidden, first):
    """trunk weights: ``first`` = {unit: {input: weight}} for layer 0, every such unit handed on by a unit weight in the later layers
    (ReLU of a non-negative number: itself)."""
    trunk = {(0, u, i): w for u, row in first.items() for i, w in row.items()}
    for li in range(1, len(hidden)):
        for u in first:
            trunk[(li, u, u)] = 1.0
    return trunk


def head_chunk(hidden, unit):
    """The chunk of the head's sum that hidden unit ``unit`` falls into (oracle mlp_forward / mlp.cuh head_output): padded widths up
    to 256 sum 8 chunks of HP/8 POSITIONS, position i holding unit 16 (i >> 4) + 4 (i & 3) + ((i >> 2) & 3); wider layers sum chunks
    of 64 units."""
    HP = -(-hidden[-1] // 64) * 64
    if HP > 256:
        return unit // 64
    t, g, r = unit >> 4, (unit & 15) >> 2, unit & 3
    return (16 * t + 4 * r + g) // (HP // 8)


def head_sum(bias, partials, order):
    """bias and {chunk: partial} added in float32: "forward" (the engine's: bias first, chunks ascending), "chunks_reversed" (bias
    first, chunks descending) or "reversed" (chunks descending, bias last)."""
    chunks = sorted(partials, reverse=order != "forward")
    terms = [np.float32(partials[c]) for c in chunks]
    terms = terms + [np.float32(bias)] if order == "reversed" else [np.float32(bias)] + terms
    total = terms[0]
    for v in terms[1:]:
        total = np.float32(total + v)
    return total


class Case:
    """name, game, head ("discrete" / "normal" / "gmm2"), rule, max_episode_length, the value bias, ``net(hidden)`` -> the keyword
    arguments of edge_values.net_blob beyond the shape, and ``check(case, out, trace)``: the condition on the CPU rollout."""

    def __init__(self, name, game, head, rule, max_len, net, check, value_bias=0.75):
        self.name, self.game, self.head, self.rule, self.max_len, self.net, self.check = name, game, head, rule, max_len, net, check
        self.value_bias = np.float32(value_bias)

    def desc(self, hidden):
        return R.net_desc(self.game, hidden, self.head, ACT)

    def blob(self, hidden):
        return E.net_blob(R.IN_DIM[self.game], list(hidden), n_dist(self.game, self.head), value_bias=self.value_bias, **self.net(tuple(hidden)))

    @property
    def bound(self):
        return np.float32(BOUND[self.game])


def bias_net(dist_bias):
    return lambda hidden: dict(dist_bias=dist_bias)


def by_game(trace):
    out = {}
    for e in trace:
        out.setdefault(e["game"], []).append(e)
    return out


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ conditions

def _all(trace, pred):
    assert trace and all(pred(e) for e in trace), next(e for e in trace if not pred(e))


def check_logits(want):
    want = np.asarray(want, np.float32)

    def check(case, out, trace):
        _all(trace, lambda e: bits32(e["raw"][1:]).tolist() == bits32(want + np.float32(0.0)).tolist())
    return check


def check_actions_all(a):
    def check(case, out, trace):
        _all(trace, lambda e: float(e["action"]) == a)
    return check


def check_every_action_occurs(case, out, trace):
    A = R.GAMES[case.game]["num_actions"]
    assert {int(e["action"]) for e in trace} == set(range(A))


def check_dist(pred):
    def check(case, out, trace):
        _all(trace, lambda e: pred(e["dist"]))
    return check


def check_draws_spread(case, out, trace):
    """the draws reach both ends of [0, 1): the action is the same whatever the draw"""
    u = [e["u"] for e in trace]
    assert min(u) < 0.05 and max(u) > 0.95, (min(u), max(u))


def both(*checks):
    def check(case, out, trace):
        for c in checks:
            c(case, out, trace)
    return check


def check_terminating(case, out, trace):
    """every game terminates; at least 3 distinct lengths inside the full 32-game team"""
    assert out["terminated"].all(), out["terminated"]
    assert (out["lengths"] < case.max_len).all(), out["lengths"]
    assert len(set(out["lengths"][:32].tolist())) >= 3, out["lengths"]


def check_d5(case, out, trace):
    check_terminating(case, out, trace)
    for e in trace:
        if e["t"] == 0:
            assert bits32(e["raw"][1:]).tolist() == [0, 0, 0], e           # the reset velocity is 0: a three-way tie of +0.0
    other = reference("D5_bangbang_sample" if case.rule == "mode" else "D5_bangbang_mode")
    assert (other["lengths"] != out["lengths"]).any()                       # the two rules play different games


def check_pump(case, out, trace):
    """D2 with consequences: every step is either a push to the left or the tie (2, 2) above logit 0, resolved to action 1; both occur
    in every game, and the games do not all end alike"""
    for e in trace:
        tie = bits32(e["raw"][2:4]).tolist() == bits32([2.0, 2.0]).tolist() and e["raw"][1] < 2.0
        assert (float(e["action"]) == 1.0 and tie) or (float(e["action"]) == 0.0 and e["raw"][1] > 2.0), e
    for steps in by_game(trace).values():
        assert {float(e["action"]) for e in steps} == {0.0, 1.0}
    assert len(set(out["lengths"][:32].tolist())) >= 3 or not out["terminated"].all(), out["lengths"]


def check_sigma(case, out, trace):
    """N1: sigma is azg_expf of the clamped log sigma (the raw output is the bias, the bounds are the descriptor's)"""
    lo, hi = ls_bounds(case.game, case.head)
    ls = np.float32(case.net(NARROW)["dist_bias"][1])
    want = expf(clamp(ls, lo, hi))
    _all(trace, lambda e: bits32(e["raw"][2]) == bits32(ls) and bits32(e["dist"][1]) == bits32(want))


def check_saturated(sign):
    def check(case, out, trace):
        lo, hi = ls_bounds(case.game, case.head)
        want = bits32(sign * case.bound)
        _all(trace, lambda e: bits32(e["action"]) == want and bits32(e["dist"][1]) == bits32(expf(hi)))
        assert len({e["eps"] for e in trace}) > len(trace) // 2 and min(e["eps"] for e in trace) < -1.0 < 1.0 < max(e["eps"] for e in trace)
    return check


def check_small_mu(case, out, trace):
    """N3: mu is the bias (+ 0.0f: see the module's note on -0.0), the action sample_action(mu, sigma, 0, bound) to the bit"""
    mu = np.float32(case.net(NARROW)["dist_bias"][0])
    seen = np.float32(mu + np.float32(0.0))
    for e in trace:
        assert bits32(e["dist"][0]) == bits32(seen), e
        want = O.sample_action(e["dist"][0], e["dist"][1], 0.0, case.bound)
        assert bits32(e["action"]) == bits32(want) and e["eps"] == 0.0, e
    if float(mu) == 0.0:
        _all(trace, lambda e: bits32(e["action"]) == 0)                     # +0.0 and -0.0 alike: +0.0
    else:
        _all(trace, lambda e: float(e["action"]) > 0.0)                     # a subnormal mu does not vanish on the way


def n5_partials(hidden):
    first, mid, last = signal_units(hidden)
    return {head_chunk(hidden, first): X, head_chunk(hidden, mid): -X, head_chunk(hidden, last): np.float32(0.25)}


def check_chunk_order(case, out, trace):
    """N5: mu = 0.5 + X - X + 0.25 with the three terms in three chunks: 0.25 in the engine's order, 0 with the chunks in the opposite
    order, 0.5 with the whole sum reversed"""
    for hidden in (NARROW, STREAMED, WIDE, WIDE_1024):
        p = n5_partials(hidden)
        ks = sorted(p)
        assert len(ks) == 3 and (p[ks[0]], p[ks[1]], p[ks[2]]) == (X, -X, np.float32(0.25)), (hidden, p)    # three different chunks
        fwd, rev_chunks, rev = (head_sum(0.5, p, o) for o in ("forward", "chunks_reversed", "reversed"))
        assert (float(fwd), float(rev_chunks), float(rev)) == (0.25, 0.0, 0.5)
    _all(trace, lambda e: bits32(e["dist"][0]) == bits32(np.float32(0.25)))
    _all(trace, lambda e: bits32(e["action"]) == bits32(O.sample_action(np.float32(0.25), e["dist"][1], 0.0, case.bound)))


def check_gmm(comps, extra=None):
    """the components taken are ``comps``; every action is sample_action of ITS component's mu and sigma with the step's eps"""
    def check(case, out, trace):
        assert {e["comp"] for e in trace} == set(comps), {e["comp"] for e in trace}
        for e in trace:
            c = e["comp"]
            assert bits32(e["action"]) == bits32(O.sample_action(e["dist"][c], e["dist"][2 + c], e["eps"], case.bound)), e
            assert e["dist"][0] != e["dist"][1]                             # the components' means differ: the pick shows
        if extra:
            extra(case, out, trace)
    return check


def _g1_extra(case, out, trace):
    _all(trace, lambda e: bits32(e["raw"][5:7]).tolist() == [0, 0])         # equal mixture logits (-0.0 + 0.0f = +0.0)


def _g2_extra(gap):
    def extra(case, out, trace):
        other = expf(-gap)
        assert (float(other) > 0.0) == (gap <= 87.0)                        # gap 30: a share of 9e-14 beside 1.0f; beyond 87: exactly 0
        _all(trace, lambda e: bits32(e["dist"][4]) == bits32(np.float32(1.0)) and bits32(e["dist"][5]) == bits32(np.float32(1.0)))
        assert max(float(e["u"]) for e in trace) > 0.95                     # draws next to 1 still fall below a share of exactly 1.0f
    return extra


def _g3_extra(case, out, trace):
    lo, hi = ls_bounds(case.game, case.head)
    _all(trace, lambda e: bits32(e["dist"][2]) == bits32(expf(lo)) and bits32(e["dist"][3]) == bits32(expf(hi)))
    _all(trace, lambda e: e["raw"][3] < lo and e["raw"][4] > hi and bits32(e["dist"][4]) == bits32(np.float32(0.5)))


# ------------------------------------------------------------------------------------------------ nets with trunk signal

def mountaincar_bangbang(hidden):
    """logits (1e3 relu(-1e3 v), 0, 1e3 relu(+1e3 v)): push the way the car is moving"""
    first, _, last = signal_units(hidden)
    return dict(trunk=carried(hidden, {first: {1: 1e3}, last: {1: -1e3}}), dist_w={(2, first): 1e3, (0, last): 1e3})


def mountaincar_pump(hidden):
    """logits (-1 + 1e3 relu(-1e3 v), 2, 2): push left while the car moves left, else a tie between "no push" and "push right" """
    _, _, last = signal_units(hidden)
    return dict(trunk=carried(hidden, {last: {1: -1e3}}), dist_w={(0, last): 1e3}, dist_bias=[-1.0, 2.0, 2.0])


def mcc_bangbang(hidden):
    """mu = 1e30 relu(v) - 1e30 relu(-v), log sigma 0: full force the way the car is moving"""
    first, _, last = signal_units(hidden)
    return dict(trunk=carried(hidden, {first: {1: 1.0}, last: {1: -1.0}}), dist_w={(0, first): float(X), (0, last): -float(X)})


def chunk_order_net(hidden):
    """three constant units (bias 1, no inputs) at the first, middle and last place; mu = 0.5 + X u_first - X u_mid + 0.25 u_last"""
    first, mid, last = signal_units(hidden)
    trunk = carried(hidden, {first: {}, mid: {}, last: {}})
    return dict(trunk=trunk, trunk_bias={(0, first): 1.0, (0, mid): 1.0, (0, last): 1.0},
                dist_w={(0, first): float(X), (0, mid): -float(X), (0, last): 0.25}, dist_bias=[0.5, 0.0])


# ------------------------------------------------------------------------------------------------ the cases

def _cases():
    c = []
    cut = f32_next(-87.0, up=False)
    e87 = expf(-87.0)
    # D1: all logits equal
    # (CartPole for 12 steps: always pushing one way drops the pole after 9 to 11, so which index a tie takes shows in the lengths)
    for game, bias in (("cartpole", [0.0, -0.0]), ("mountaincar", [-0.0, 0.0, -0.0])):
        c.append(Case(f"D1_tie_{game}_mode", game, "discrete", "mode", 12 if game == "cartpole" else 8, bias_net(bias), both(check_logits(bias), check_actions_all(0.0))))
        c.append(Case(f"D1_tie_{game}_sample", game, "discrete", "sample", 8, bias_net(bias), both(check_logits(bias), check_every_action_occurs)))
    # D2: a tie that is not at index 0
    c.append(Case("D2_tie_at_1_mode", "mountaincar", "discrete", "mode", 8, bias_net([-1.0, 2.0, 2.0]),
                  both(check_logits([-1.0, 2.0, 2.0]), check_actions_all(1.0))))
    # ... and the same tie deciding a game: MountainCar pays -1 whatever the action and a few steps never reach the flag, so the
    # bias-only net above cannot show its action in any output; this one pumps only while the car moves left and coasts (the tie's
    # first index, action 1) otherwise, where taking the tie's last index would push right as well and arrive much earlier
    c.append(Case("D2_tie_at_1_pump_mode", "mountaincar", "discrete", "mode", 200, mountaincar_pump, check_pump))
    # D3: on and beside azg_expf's cut
    c.append(Case("D3_on_cut_sample", "cartpole", "discrete", "sample", 8, bias_net([0.0, -87.0]),
                  check_dist(lambda d: bits32(d[1]) == bits32(e87) and float(d[1]) > 0.0 and float(d[0]) == 1.0)))
    c.append(Case("D3_below_cut_sample", "cartpole", "discrete", "sample", 8, bias_net([0.0, cut]),
                  both(check_dist(lambda d: bits32(d).tolist() == bits32([1.0, 0.0]).tolist()), check_actions_all(0.0))))
    c.append(Case("D3_mountaincar_cut_sample", "mountaincar", "discrete", "sample", 8, bias_net([-87.0, 0.0, cut]),
                  both(check_dist(lambda d: bits32(d).tolist() == bits32([e87, 1.0, 0.0]).tolist()), check_actions_all(1.0))))
    # D4: the largest finite gap: a one-hot softmax
    c.append(Case("D4_onehot_lo_sample", "cartpole", "discrete", "sample", 8, bias_net([0.0, -F32_MAX]),
                  both(check_dist(lambda d: bits32(d).tolist() == bits32([1.0, 0.0]).tolist()), check_actions_all(0.0), check_draws_spread),
                  value_bias=F32_MAX))
    c.append(Case("D4_onehot_hi_sample", "cartpole", "discrete", "sample", 8, bias_net([F32_MAX, 0.0]),
                  both(check_dist(lambda d: bits32(d).tolist() == bits32([1.0, 0.0]).tolist()), check_actions_all(0.0), check_draws_spread)))
    # D5: bang-bang MountainCar-v0
    for rule in ("mode", "sample"):
        c.append(Case(f"D5_bangbang_{rule}", "mountaincar", "discrete", rule, 200, mountaincar_bangbang, check_d5))
    # N1: log sigma below / on / one float32 inside each clamp
    for end, game in (("min", "pendulum_v0"), ("max", "mcc")):
        lo, hi = ls_bounds(game, "normal")
        b = lo if end == "min" else hi
        for where, ls in (("below" if end == "min" else "above", f32_next(b, up=end == "max")), ("on", b), ("inside", f32_next(b, up=end == "min"))):
            c.append(Case(f"N1_ls_{end}_{where}", game, "normal", "sample", 8, bias_net([0.25, ls]), check_sigma,
                          value_bias=SUB if (end, where) == ("min", "below") else 0.75))
    # N2: a saturated squash
    for lab, game, mu in (("p1e30", "pendulum_v1", 1e30), ("m1e30", "pendulum_v1", -1e30), ("p3e38", "mcc", 3e38), ("m3e38", "mcc", -3e38)):
        hi = ls_bounds(game, "normal")[1]
        c.append(Case(f"N2_mu_{lab}_sample", game, "normal", "sample", 8, bias_net([mu, hi]),
                      check_saturated(np.float32(np.sign(mu)))))
    # N3: mu at and next to zero
    for lab, mu in (("p0", 0.0), ("m0", -0.0), ("subnormal", SUB), ("1e-38", 1e-38)):
        c.append(Case(f"N3_mu_{lab}_mode", "pendulum_v0" if lab in ("p0", "subnormal") else "mcc", "normal", "mode", 8, bias_net([mu, 0.0]),
                      check_small_mu))
    # N4: bang-bang MountainCarContinuous; N5: a head sum that depends on its order
    c.append(Case("N4_bangbang_mode", "mcc", "normal", "mode", 200, mcc_bangbang, check_terminating))
    c.append(Case("N5_chunk_order_mode", "pendulum_v0", "normal", "mode", 8, chunk_order_net, check_chunk_order))
    # G1 .. G3: the mixture head (mu0, mu1, ls0, ls1, lc0, lc1)
    lo, hi = ls_bounds("pendulum_v1", "gmm2")
    c.append(Case("G1_equal_shares_mode", "pendulum_v1", "gmm2", "mode", 8, bias_net([0.5, -0.5, 0.0, 0.0, -0.0, 0.0]), check_gmm({0}, _g1_extra),
                  value_bias=-0.0))
    c.append(Case("G2_gap30_sample", "pendulum_v1", "gmm2", "sample", 12, bias_net([0.5, -0.5, 0.0, 0.0, 0.0, -30.0]), check_gmm({0}, _g2_extra(30.0))))
    c.append(Case("G2_gap88_sample", "pendulum_v1", "gmm2", "sample", 12, bias_net([0.5, -0.5, 0.0, 0.0, 0.0, -88.0]), check_gmm({0}, _g2_extra(88.0))))
    c.append(Case("G3_both_clamps_sample", "pendulum_v1", "gmm2", "sample", 8,
                  bias_net([0.5, -0.5, float(lo) - 1.0, float(hi) + 1.0, 0.0, 0.0]), check_gmm({0, 1}, _g3_extra)))
    assert len({x.name for x in c}) == len(c)
    return {x.name: x for x in c}


CASES = _cases()
# one case per head that also runs at (1024, 1024) in the team form (NU = 16, two games per workgroup)
AT_1024 = ("D3_mountaincar_cut_sample", "N1_ls_max_above", "G3_both_clamps_sample")
# the cases whose arrays the CPU suite shows to be the same at the narrow and the wide shape (the added width is zeros)
SAME_AT_EVERY_WIDTH = ("D5_bangbang_sample", "N5_chunk_order_mode")


def check_common(case, out, trace):
    """every case: nothing is NaN, and first_value carries the value bias's bits (+ 0.0f: the head's sum, see the module's note)"""
    assert not np.isnan(out["returns"]).any() and not np.isnan(out["first_value"]).any()
    assert (bits32(out["first_value"]) == bits32(case.value_bias + np.float32(0.0))).all(), out["first_value"]
    assert len(trace) == int(out["lengths"].sum()) and set(by_game(trace)) == set(range(G))


def run(case, hidden, max_len=None, episode=0, trace=None):
    out = R.cpu_rollout(R.GAMES[case.game], case.desc(hidden), case.blob(hidden), G, max_len or case.max_len, case.rule, BASE, episode, trace=trace)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, hidden=NARROW, max_len=None, episode=0):
    """The CPU rollout of case ``name`` at a hidden shape: computed once per process, shared, read-only."""
    return run(CASES[name], tuple(hidden), max_len, episode)


@functools.lru_cache(maxsize=None)
def traced(name):
    """(arrays, trace) of case ``name`` at the narrow shape."""
    trace = []
    out = run(CASES[name], NARROW, trace=trace)
    return out, trace


def assert_same_bits(got, want, what):
    """returns as uint64, first_value as uint32, lengths and flags exact; and nothing is NaN (equal bits alone would let a NaN that
    both sides produce pass)."""
    for k, view in (("returns", np.uint64), ("first_value", np.uint32)):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert not np.isnan(g).any() and not np.isnan(w).any(), (what, k)
        bad = np.argwhere(g.view(view) != w.view(view))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"
    for k in ("lengths", "terminated"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"
