"""Device self-play at the edges of the agents' final-action rule: hand-built networks (edge_values.net_blob: exact value biases, exact
logits) whose searches end in tied counts, an arg-max tie that is not at index 0, unvisited edges, a largest root Q of exactly 0
(every pi entry NaN: the reference raises), ratios above 1, powers that underflow, a cdf with repeated values, episodes that end on
their first step, by `done` and by length at once, and carried root counts that are kept and dropped.  Each case states its game, its
search, selfplay_begin's settings and its net for any hidden shape, and carries a condition on the trace of the numpy restatement
(selfplay_ref.cpu_selfplay(trace=...)) that proves, without a GPU, that the case contains what its name says.
tests/test_selfplay_edges_host.py asserts the conditions, holds the oracle's azo_selfplay_step to the restatement and checks that
every deliberately wrong variant of the rule (selfplay_ref.MUTANTS) is caught; tests/test_selfplay_edges.py compares every kernel form
with the restatement bit for bit.  numpy and the CPU oracle only.

Sizes: 33 games (two full 16-lane groups of selfplay_kernel16 and one game), at most 16 simulations, at most 6 steps.  Exceptions:
temperature_table_ends_2048 (2048 simulations, 16 games: the temperature table's documented limit) and many_children_* (65 games: two
blocks of selfplay_kernel's 64 threads, the second with one game).

Two facts about the games that shape the cases:
  * MountainCar-v0 at [0.44, 0.04] is TWO steps from the flag whatever the action (one step reaches 0.4804 at most): the hand-placed
    games of ends_at_once_mountaincar alternate between that root, which must end on step 1, and [0.47, 0.04], one step away, which
    must end on step 0.
  * many_children_*: Kmax = 20 with 16 simulations is c_pw = 5; the root then holds 17 children (the first unvisited, every other
    visited once): the condition's "more than 16 root children in every row"."""
import functools
import math

import numpy as np

import edge_values as E
import oracle_lib as O
import rollout_edges as RE
import selfplay_ref as SR
from alphazero_gym_amd import _capi

G = 33
BASE = 100              # global id of game 0
SEED = 77
ACT = "relu"
NARROW, W256, WIDE = (64, 64), (256, 256), (512, 512)
GROUPS = ("ties", "nan", "temperature", "books", "continuous")
GAMES = {
    "cartpole": dict(env_id=0, mode=0, in_dim=4, A=2),
    "mountaincar": dict(env_id=3, mode=0, in_dim=2, A=3),
    "acrobot": dict(env_id=5, mode=0, in_dim=6, A=3),
    "pendulum_v0": dict(env_id=1, mode=1, in_dim=3, bound=2.0),
    "pendulum_v1": dict(env_id=2, mode=1, in_dim=3, bound=2.0),
    "mcc": dict(env_id=4, mode=1, in_dim=2, bound=1.0),
}
TEMPERATURES = {"1e-3": 1e-3, "0.5": 0.5, "3": 3.0, "60": 60.0, "1e4": 1e4}


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    """name, group, game, n_sims, steps, selfplay_begin's settings, the engine's other settings (c_uct, v_target, c_pw, ...), the net:
    value bias and ``net(hidden)`` -> edge_values.net_blob's keyword arguments beyond the shape, the hand-placed roots
    ``place`` {game: root} (uploaded after selfplay_begin), ``uploads`` {step: f(states) -> (roots, carry or None)} and
    ``check(case, out, trace)``: the condition on the restatement's trace."""

    def __init__(self, name, group, game, n_sims, check, steps=3, begin=None, value_bias=0.0, net=None, kw=None, place=None, uploads=None,
                 n_games=G):
        assert group in GROUPS
        self.name, self.group, self.game, self.n_sims, self.check, self.steps = name, group, game, n_sims, check, steps
        self.begin = dict(SR.BEGIN, **(begin or {}))
        self.value_bias, self.net, self.extra = np.float32(value_bias), net or (lambda hidden: {}), dict(kw or {})
        self.place, self.uploads, self.n_games = dict(place or {}), dict(uploads or {}), n_games

    @property
    def cont(self):
        return GAMES[self.game]["mode"] == 1

    def kw(self, base=BASE):
        g = GAMES[self.game]
        kw = dict(env_id=g["env_id"], mode=g["mode"], n_sims=self.n_sims, c_uct=0.05 if self.cont else 1.0, gamma=1.0, seed=SEED, tree_id_base=base)
        if self.cont:
            kw.update(c_pw=1.0, kappa=0.5, action_bound=g["bound"])
        else:
            kw.update(num_actions=g["A"])
        kw.update(self.extra)
        return kw

    def desc(self, hidden):
        g = GAMES[self.game]
        return _capi.make_desc(g["in_dim"], list(hidden), 2 if self.cont else g["A"], ACT)

    def blob(self, hidden):
        g = GAMES[self.game]
        return E.net_blob(g["in_dim"], list(hidden), 2 if self.cont else g["A"], value_bias=self.value_bias, **self.net(tuple(hidden)))

    def first_roots(self, n_games, base=BASE):
        """The roots uploaded after selfplay_begin: the games' own reset states with the hand-placed games put over them; None if
        the case places none."""
        if not self.place:
            return None
        env_id = GAMES[self.game]["env_id"]
        roots = np.stack([O.reset_state(SEED, base + i, 0, False, env_id=env_id) for i in range(n_games)])
        for i, r in self.place.items():
            if i < n_games:
                roots[i] = r
        return roots

    def placed(self, n_games=G):
        return sorted(i for i in self.place if i < n_games)


def bias_net(dist_bias):
    return lambda hidden: dict(dist_bias=dist_bias)


# ------------------------------------------------------------------------------------------------ conditions

def _all(trace, pred, step=None):
    es = [e for e in trace if step is None or e["step"] == step]
    assert es and all(pred(e) for e in es), next(e for e in es if not pred(e))


def _some(trace, pred):
    assert any(pred(e) for e in trace)


def _picks(trace):
    return {e["pick"] for e in trace}


def check_counts_all_tied(det):
    def check(case, out, trace):
        _all(trace, lambda e: e["counts"].tolist() == [3, 3, 3])
        if det:
            _all(trace, lambda e: e["pick"] == 0)
        else:
            assert _picks(trace) == {0, 1, 2}
    return check


def check_top_tie_not_first(case, out, trace):
    _all(trace, lambda e: e["counts"][1] == e["counts"][2] > e["counts"][0] and e["pick"] == 1)


def check_unvisited_edges(case, out, trace):
    """an edge with count 0 and no child node; its pi entry is exactly 0; the sampled rule never picks it, though its draws reach both ends"""
    _all(trace, lambda e: e["counts"].tolist() == [case.n_sims, 0] and e["child_n"][1] == -1 and bits64(e["pi"]).tolist() == bits64([1.0, 0.0]).tolist())
    _all(trace, lambda e: e["pick"] == 0 and not e["reference_raises"])
    u = [e["u"] for e in trace]
    assert min(u) < 0.05 and max(u) > 0.95


def check_unvisited_picked(case, out, trace):
    """the unvisited edge's Q (the root's V) is the largest: it is picked, nothing is carried, and the next root is one env step on"""
    for e in trace:
        k = e["pick"]
        assert e["counts"][k] == 0 and e["child_n"][k] == -1 and e["Q"][k] == np.max(e["Q"]) == float(case.value_bias), e
        assert (e["Q"][:k] < e["Q"][k]).all() and e["carry_out"] == 0 and not e["ended"], e
        assert bits64(e["root_after"]).tolist() == bits64(e["next_state"]).tolist(), e
    by_game = {}
    for e in trace:
        by_game.setdefault(e["game"], []).append(e)
    for es in by_game.values():
        for a, b in zip(es, es[1:]):
            assert bits64(b["state"]).tolist() == bits64(a["next_state"]).tolist() and b["carry_in"] == 0


def check_negative_q(case, out, trace):
    """every Q < 0: every ratio Q / max Q is >= 1, and the smallest |Q| gets pi's smallest entry"""
    _all(trace, lambda e: (e["Q"] < 0).all() and (e["Q"] / np.max(e["Q"]) >= 1.0).all() and not e["reference_raises"])
    _all(trace, lambda e: e["pi"][int(np.argmin(np.abs(e["Q"])))] == np.min(e["pi"]))
    _some(trace, lambda e: len(set(e["Q"].tolist())) > 1)
    assert len(_picks(trace)) > 1


def check_mixed_signs(case, out, trace):
    _all(trace, lambda e: e["Q"][0] > 0 > e["Q"][1] and float(np.sum(e["pi"])) > 1.0 and not e["reference_raises"])
    sums = {round(float(np.sum(e["pi"])), 2) for e in trace}
    assert sums & {1.76, 1.8}, sums
    assert _picks(trace) == {0, 1}


def check_qmax_zero(det, last):
    def check(case, out, trace):
        _all(trace, lambda e: np.max(e["Q"]) == 0.0 and np.isnan(e["pi"]).all() and e["reference_raises"])
        _all(trace, lambda e: e["pick"] == (0 if det else last))
        assert int(out["reference_raises"]) == len(trace)
    return check


def check_temperature(label, visited):
    T = TEMPERATURES[label]

    def check(case, out, trace):
        for e in trace:
            c, pi = e["counts"], e["pi"]
            assert (c > 0).sum() == visited and not e["reference_raises"], e
            if visited == 3:
                assert len(set(c.tolist())) == 3, e
            assert (pi[c == 0] == 0.0).all(), e
            top = c == c.max()
            if label == "1e-3":
                assert (np.abs(pi[c > 0] * visited - 1.0) < 0.01).all(), e
            if label == "1e4":
                assert (pi[~top] == 0.0).all() and (pi[top] == 1.0).all(), e
            if label == "60" and visited == 3:
                assert ((pi > 0.0) & (pi < 1e-10)).any(), e
            if visited == 3 and label not in ("1e4",):
                assert (pi > 0).all() and len(set(pi.tolist())) == 3, e
            # the table's entry: libm's pow of the ratio, as Python's float power gives it
            y = np.array([math.pow(float(n) / float(c.max()), T) for n in c])
            assert bits64(pi).tolist() == bits64(np.abs(y / np.sum(y))).tolist(), e
        if visited == 3 and label in ("1e-3", "0.5"):
            assert _picks(trace) == {0, 1, 2}
    return check


def check_table_ends(case, out, trace):
    """some root's largest count is its total: the last entry of the table's last row, index cmax (cmax + 1) / 2 + cmax"""
    _some(trace, lambda e: e["counts"].max() == e["counts"].sum() == case.n_sims)
    _all(trace, lambda e: not e["reference_raises"])


def check_cdf_repeats(case, out, trace):
    _all(trace, lambda e: e["counts"][1] == 0 and e["counts"][0] > 0 and e["counts"][2] > 0)
    _all(trace, lambda e: bits64(e["cdf"][0]) == bits64(e["cdf"][1]) and e["cdf"][0] < 1.0 and e["cdf"][2] == 1.0)
    picks = _picks(trace)
    assert 2 in picks and 0 in picks and 1 not in picks


def check_q_ties_discrete(case, out, trace):
    """every edge visited once: three equal, non-zero Qs, pi = (1/3, 1/3, 1/3): the first index"""
    _all(trace, lambda e: len(set(bits64(e["Q"]).tolist())) == 1 and e["Q"][0] != 0.0 and len(set(bits64(e["pi"]).tolist())) == 1 and e["pick"] == 0)


HIT_GAME, EPS_GAME = 7, 1              # the games whose draw a case's setting is made to meet exactly


def temperature_hitting(u, a, b):
    """A temperature at which the cdf of counts (a, b), a > b > 0, has cdf[0] == u exactly (0.5 < u < 1): the float64 neighbours of
    log(1 / u - 1) / log(b / a) are tried in turn -- a temperature moves cdf[0] by less than the cdf's own spacing, so one of them fits."""
    def cdf0(T):
        return float(SR.discrete_rule(np.array([a, b]), None, dict(SR.BEGIN, temperature=T), 0.5)[2][0])
    lo = hi = math.log(1.0 / u - 1.0) / math.log(b / a)
    lo, hi = lo * (1.0 - 1e-9), hi * (1.0 + 1e-9)                # cdf[0] rises with the temperature
    assert cdf0(lo) < u < cdf0(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        lo, hi = (mid, hi) if cdf0(mid) < u else (lo, mid)
    T = lo
    for _ in range(64):
        T = float(np.nextafter(T, -np.inf))
    for _ in range(256):
        if cdf0(T) == u:
            return T
        T = float(np.nextafter(T, np.inf))
    raise AssertionError("no temperature puts cdf[0] on the draw")


def check_draw_on_a_cdf_value(case, out, trace):
    """game HIT_GAME's first draw IS cdf[0]: searchsorted(side="right") -- first index with u < cdf -- takes index 1"""
    e = next(e for e in trace if e["game"] == HIT_GAME and e["step"] == 0)
    assert e["counts"].tolist() == [6, 2] and bits64(e["cdf"][0]) == bits64(e["u"]) and e["pick"] == 1, e
    _all(trace, lambda e: e["counts"].min() > 0 and not e["reference_raises"])
    assert _picks(trace) == {0, 1}


def check_eps_on_the_draw(case, out, trace):
    """game EPS_GAME's first u01 IS the agent's epsilon: `u01 < epsilon` is false, the greedy child is taken, and w % n_children is another"""
    eps = case.begin["agent_epsilon"]
    e = next(e for e in trace if e["game"] == EPS_GAME and e["step"] == 0)
    assert float(e["u01"]) == eps and e["pick"] == e["greedy"] != e["w"] % len(e["counts"]), e
    check_agent_eps(eps)(case, out, trace)


def check_on_policy_ties(case, out, trace):
    _all(trace, lambda e: len(set(e["counts"].tolist())) == 1 and len(e["counts"]) >= 3)
    So = 3 if case.cont else 2
    K = (out["rows"].shape[1] - So - 1) // 3
    col = out["rows"][:, So + 3 * K]
    assert np.isfinite(col).all() and (col != 0).all()
    if case.cont:
        # the K x K sum is not the maximum: the two targets differ in some row
        qmax = out["rows"][:, So + 2 * K:So + 3 * K].max(1)
        assert (bits32(col) != bits32(qmax)).any()


def check_max_len_1(case, out, trace):
    env_id = GAMES[case.game]["env_id"]
    for e in trace:
        assert e["ended"] and e["why"] in ("length", "both") and e["carry_out"] == 0 and e["carry_in"] == 0, e
        want = O.reset_state(SEED, BASE + e["game"], e["step"] + 1, False, env_id=env_id)
        assert bits64(e["root_after"]).tolist() == bits64(want).tolist(), e
    assert (out["fcnt"] == case.steps).all()
    by = {(e["game"], e["step"]): e for e in trace}
    for (g, s), e in by.items():
        if s > 0:
            assert bits64(e["state"]).tolist() == bits64(by[(g, s - 1)]["root_after"]).tolist()


def check_ends_at_once(ret=None, late=()):
    """every hand-placed game is `done` on step 0 (those of ``late``: on step 1) and restarts; ret: the finished episode's return"""
    def check(case, out, trace):
        placed = case.placed()
        assert len(placed) >= 3 and {p // 16 for p in placed} == {0, 1, 2}      # in both full lane groups and the last game
        by = {(e["game"], e["step"]): e for e in trace}
        for g in placed:
            s = 1 if g in late else 0
            e = by[(g, s)]
            assert e["done"] and e["ended"] and e["why"] == "done" and e["carry_out"] == 0, e
            assert all(not by[(g, k)]["ended"] for k in range(s))
            assert out["fcnt"][g] >= 1
            if ret is not None:
                assert e["reward"] == ret(case, e), e
        others = [e for e in trace if e["game"] not in placed and e["step"] == 0]
        assert others and not any(e["ended"] for e in others)
    return check


def check_done_and_length(case, out, trace):
    """max_episode_length is the step on which the hand-placed games terminate: one episode is counted, not two"""
    L = case.begin["max_episode_length"]
    for g in case.placed():
        es = [e for e in trace if e["game"] == g]
        assert [e["why"] for e in es[:L]] == [None] * (L - 1) + ["both"], [e["why"] for e in es]
    assert (out["fcnt"] == case.steps // L).all(), out["fcnt"]
    _some(trace, lambda e: e["why"] == "length")


def check_carry(case, out, trace):
    """the carry is the picked child's node count: positive inside an episode, 0 after an end; uploaded roots (before step 2 without a
    carry, moving game 5; before step 3 with a carry of 5) are where the games go on from; the episode that ends on step 3 drops the
    uploaded carry, and the last step hands a carry on"""
    for e in trace:
        k = e["pick"]
        if e["ended"]:
            assert e["carry_out"] == 0, e
        else:
            assert e["carry_out"] == e["child_n"][k] > 0 and e["carry_out"] != e["counts"][k], e
    by = {(e["game"], e["step"]): e for e in trace}
    games = range(case.n_games)
    assert sorted(case.uploads) == [2, 3]
    for (g, s), e in by.items():
        if s in case.uploads:
            want_roots, want_carry = case.uploads[s](np.stack([by[(i, s - 1)]["root_after"] for i in games]))
            assert bits64(e["state"]).tolist() == bits64(want_roots[g]).tolist()
            assert e["carry_in"] == (0 if want_carry is None else want_carry[g])
        elif s > 0:
            assert e["carry_in"] == by[(g, s - 1)]["carry_out"]
    assert [g for g in games if bits64(by[(g, 2)]["state"]).tolist() != bits64(by[(g, 1)]["root_after"]).tolist()] == [5]   # the game the upload moved
    assert all(by[(g, 1)]["carry_out"] > 0 and by[(g, 2)]["carry_in"] == 0 and by[(g, 3)]["carry_in"] == 5 for g in games)
    assert all(by[(g, 3)]["ended"] and by[(g, 4)]["carry_in"] == 0 and by[(g, 5)]["carry_out"] > 0 for g in games)
    assert (out["carry"] > 0).all()


def check_visit_ties_first(many):
    def check(case, out, trace):
        if many:
            # 17 children, the first unvisited and every other visited once: the first index of the largest count is 1
            _all(trace, lambda e: len(e["counts"]) > 16 and e["counts"].tolist() == [0] + [1] * (len(e["counts"]) - 1) and e["pick"] == 1)
        else:
            _all(trace, lambda e: len(set(e["counts"].tolist())) == 1 and len(e["counts"]) >= 3 and e["pick"] == 0)
            _some(trace, lambda e: len(set(e["Q"].tolist())) > 1)
    return check


def check_q_ties_first(case, out, trace):
    bound = np.float32(GAMES[case.game]["bound"])
    So = 3
    K = (out["rows"].shape[1] - So - 1) // 3
    acts = out["rows"][:, So:So + K]
    assert (bits32(acts) == bits32(bound)).all() or (bits32(acts) == bits32(-bound)).all()
    _all(trace, lambda e: len(set(bits64(e["Q"]).tolist())) == 1 and len(e["Q"]) >= 3 and e["pick"] == 0)


def check_agent_eps(eps, many=False):
    def check(case, out, trace):
        if many:
            _all(trace, lambda e: len(e["counts"]) > 16)
        if eps == 1.0:
            _all(trace, lambda e: e["pick"] == e["w"] % len(e["counts"]))
            _some(trace, lambda e: e["pick"] != e["greedy"])
        else:
            _some(trace, lambda e: e["u01"] < eps and e["pick"] == e["w"] % len(e["counts"]) != e["greedy"])
            _some(trace, lambda e: e["u01"] >= eps and e["pick"] == e["greedy"])
            _all(trace, lambda e: e["pick"] == (e["w"] % len(e["counts"]) if e["u01"] < eps else e["greedy"]))
    return check


def check_many_max_len_1(case, out, trace):
    _all(trace, lambda e: len(e["counts"]) > 16 and e["ended"] and e["why"] == "length" and e["carry_out"] == 0)
    assert (out["fcnt"] == case.steps).all()


# ------------------------------------------------------------------------------------------------ the cases

def _upload_move_5(carry):
    def f(states):
        roots = np.array(states, np.float64)
        roots[5] = [0.1, 0.0, 0.01, 0.0]
        return roots, (None if carry is None else np.full(len(roots), carry, np.int32))
    return f


def _keep(carry):
    def f(states):
        return np.array(states, np.float64), (None if carry is None else np.full(len(states), carry, np.int32))
    return f


PLACES = (0, 7, 16, 31, 32)            # hand-placed games: both full lane groups and the last game


def _place(root, alt=None):
    return {g: (alt if (alt is not None and i % 2) else root) for i, g in enumerate(PLACES)}


def _mcc_flag_reward(case, e):
    """mu saturated at +bound: the flag pays 100 - 0.1 a^2 with a = the bound"""
    a = GAMES[case.game]["bound"]
    assert bits32(e["action"]) == bits32(np.float32(a)), e
    return 100.0 - 0.1 * a * a


def _cases():
    c = []
    det, mv = dict(deterministic=True), dict(final_selection="max_value")
    # ---- ties
    c.append(Case("counts_all_tied_det", "ties", "mountaincar", 9, check_counts_all_tied(True), begin=det))
    c.append(Case("counts_all_tied_sampled", "ties", "mountaincar", 9, check_counts_all_tied(False)))
    c.append(Case("top_tie_not_first", "ties", "mountaincar", 8, check_top_tie_not_first, begin=det, net=bias_net([-1.0, 2.0, 2.0])))
    for n in (1, 2):
        c.append(Case(f"unvisited_edges_{n}", "ties", "cartpole", n, check_unvisited_edges, steps=4))
    # MountainCar pays -1: a visited edge's Q is V - 1, an unvisited edge's is the root's V = 2: ratios (1/2, 1/2, 1)
    c.append(Case("unvisited_picked", "ties", "mountaincar", 2, check_unvisited_picked, begin=dict(det, **mv), value_bias=2.0))
    for game in ("mountaincar", "acrobot"):
        c.append(Case(f"negative_q_{game}", "ties", game, 8, check_negative_q, begin=mv, value_bias=-0.5))
    c.append(Case("negative_q_cartpole", "ties", "cartpole", 1, check_negative_q, begin=mv, value_bias=-3.0))
    c.append(Case("cdf_repeats", "ties", "mountaincar", 8, check_cdf_repeats, net=bias_net([3.0, -200.0, 2.0]), kw=dict(c_uct=1e6)))
    c.append(Case("q_ties_discrete", "ties", "mountaincar", 3, check_q_ties_discrete, begin=dict(det, **mv), value_bias=0.5))
    T = temperature_hitting(O.act_draw(SEED, BASE + HIT_GAME, 0)[1], 6, 2)
    c.append(Case("draw_on_a_cdf_value", "ties", "cartpole", 8, check_draw_on_a_cdf_value, steps=2, begin=dict(temperature=T),
                  net=bias_net([1.0, 0.0]), kw=dict(c_uct=1e6)))
    c.append(Case("on_policy_ties_discrete", "ties", "mountaincar", 9, check_on_policy_ties, kw=dict(v_target="on_policy"), value_bias=0.3))
    # ---- NaN and what lies beside it
    c.append(Case("mixed_signs", "nan", "cartpole", 8, check_mixed_signs, begin=mv, value_bias=-1.0))
    c.append(Case("qmax_zero_det", "nan", "cartpole", 1, check_qmax_zero(True, 1), begin=dict(det, **mv), value_bias=-1.0))
    c.append(Case("qmax_zero_sampled", "nan", "cartpole", 1, check_qmax_zero(False, 1), begin=mv, value_bias=-1.0))
    # (Acrobot pays -1 too: with V = 1 every edge visited once has Q exactly 0)
    c.append(Case("qmax_zero_acrobot", "nan", "acrobot", 3, check_qmax_zero(False, 2), begin=mv, value_bias=1.0))
    # ---- the temperature table
    for label, T in TEMPERATURES.items():
        for game in ("mountaincar", "acrobot") if label == "60" else ("mountaincar",):
            c.append(Case(f"temperature_{label}_{game}", "temperature", game, 12, check_temperature(label, 3), begin=dict(temperature=T),
                          net=bias_net([2.0, 1.0, 0.0])))
        c.append(Case(f"temperature_{label}_cartpole", "temperature", "cartpole", 8, check_temperature(label, 1), begin=dict(temperature=T)))
    c.append(Case("temperature_table_ends_1", "temperature", "cartpole", 1, check_table_ends, begin=dict(temperature=0.5)))
    c.append(Case("temperature_table_ends_2048", "temperature", "cartpole", 2048, check_table_ends, steps=2, begin=dict(temperature=0.5),
                  net=bias_net([80.0, 0.0]), kw=dict(c_uct=1e9), n_games=16))
    # ---- the episode books
    c.append(Case("max_len_1", "books", "cartpole", 8, check_max_len_1, steps=4, begin=dict(det, max_episode_length=1)))
    c.append(Case("ends_at_once_cartpole", "books", "cartpole", 8, check_ends_at_once(lambda case, e: 1.0), begin=det,
                  place=_place([2.39, 1.5, 0.0, 0.0])))
    c.append(Case("ends_at_once_mountaincar", "books", "mountaincar", 8, check_ends_at_once(lambda case, e: -1.0, late=PLACES[0::2]), begin=det,
                  net=RE.mountaincar_bangbang, place=_place([0.44, 0.04], [0.47, 0.04])))
    c.append(Case("ends_at_once_acrobot", "books", "acrobot", 8, check_ends_at_once(lambda case, e: 0.0), begin=det,
                  place=_place([1.9, 0.2, 2.0, 1.0])))
    c.append(Case("ends_at_once_mcc", "books", "mcc", 8, check_ends_at_once(_mcc_flag_reward), begin=det, net=bias_net([1e30, 0.0]),
                  place=_place([0.44, 0.03])))
    c.append(Case("done_and_length", "books", "cartpole", 8, check_done_and_length, steps=4, begin=dict(det, max_episode_length=2),
                  place=_place([2.35, 1.5, 0.0, 0.0])))
    c.append(Case("carry_kept_and_dropped", "books", "cartpole", 8, check_carry, steps=6, begin=dict(det, max_episode_length=4),
                  uploads={2: _upload_move_5(None), 3: _keep(5)}))
    # ---- continuous
    c.append(Case("visit_ties_first", "continuous", "pendulum_v1", 16, check_visit_ties_first(False), net=bias_net([0.25, 0.0])))
    c.append(Case("q_ties_first", "continuous", "pendulum_v1", 16, check_q_ties_first, begin=mv, value_bias=0.5, net=bias_net([1e30, 0.0])))
    c.append(Case("on_policy_ties_continuous", "continuous", "pendulum_v0", 16, check_on_policy_ties, kw=dict(v_target="on_policy"),
                  value_bias=0.3, net=bias_net([0.25, 0.0])))
    c.append(Case("agent_eps_1", "continuous", "pendulum_v0", 16, check_agent_eps(1.0), begin=dict(agent_epsilon=1.0), net=bias_net([0.25, 0.0])))
    c.append(Case("agent_eps_half", "continuous", "pendulum_v0", 16, check_agent_eps(0.5), begin=dict(agent_epsilon=0.5), net=bias_net([0.25, 0.0])))
    c.append(Case("agent_eps_on_the_draw", "continuous", "pendulum_v0", 16, check_eps_on_the_draw,
                  begin=dict(agent_epsilon=float(O.act_draw(SEED, BASE + EPS_GAME, 0)[0])), net=bias_net([0.25, 0.0])))
    many = dict(kw=dict(c_pw=5.0), net=bias_net([0.25, 0.0]), n_games=65)
    c.append(Case("many_children_visit_ties_first", "continuous", "pendulum_v1", 16, check_visit_ties_first(True), **many))
    c.append(Case("many_children_agent_eps_1", "continuous", "pendulum_v1", 16, check_agent_eps(1.0, many=True), begin=dict(agent_epsilon=1.0), **many))
    c.append(Case("many_children_max_len_1", "continuous", "pendulum_v1", 16, check_many_max_len_1, steps=4, begin=dict(max_episode_length=1), **many))
    assert len({x.name for x in c}) == len(c)
    return {x.name: x for x in c}


CASES = _cases()

# ------------------------------------------------------------------------------------------------ which case runs in which device form

# the cases every form takes: at least one of each group, and the seven the forms must always see
SUBSET = ("qmax_zero_sampled", "qmax_zero_det", "counts_all_tied_det", "temperature_1e4_mountaincar", "max_len_1", "ends_at_once_cartpole",
          "unvisited_picked", "agent_eps_1", "visit_ties_first", "carry_kept_and_dropped")
ALWAYS = ("qmax_zero", "counts_all_tied", "temperature_1e4", "max_len_1", "ends_at_once", "unvisited_picked", "agent_eps_1")
# the 8-wave shapes exist for continuous mode only (dispatch.cuh): more of the continuous cases run at (256, 256)
CONT_256 = ("q_ties_first", "on_policy_ties_continuous", "agent_eps_on_the_draw", "agent_eps_half")
ACROBOT = ("qmax_zero_acrobot", "negative_q_acrobot", "temperature_60_acrobot", "ends_at_once_acrobot")
# three CartPole nets, one simulation, max_value sampled: Q = (0, -1): NaN;  (-2, -3): ratios (1, 1.5);  (6, 5): an unvisited edge's V
POPULATION = ("qmax_zero_sampled", "negative_q_cartpole", "unvisited_value_cartpole")
CASES["unvisited_value_cartpole"] = Case("unvisited_value_cartpole", "ties", "cartpole", 1,
                                         lambda case, out, trace: (_all(trace, lambda e: e["Q"].tolist() == [6.0, 5.0] and e["child_n"][1] == -1),
                                                                   _some(trace, lambda e: e["pick"] == 1 and e["carry_out"] == 0)),
                                         begin=dict(final_selection="max_value"), value_bias=5.0)
# three MountainCar nets with their own c_uct in one launch (8 simulations, sampled): counts (3, 3, 2), (a, 0, b) and (2, 3, 3)
NET_SEARCH = (("counts_near_tied", 1.0), ("cdf_repeats", 1e6), ("top_tie_sampled", 2.0))
CASES["counts_near_tied"] = Case("counts_near_tied", "ties", "mountaincar", 8,
                                 lambda case, out, trace: _all(trace, lambda e: sorted(e["counts"].tolist()) == [2, 3, 3]))
CASES["top_tie_sampled"] = Case("top_tie_sampled", "ties", "mountaincar", 8,
                                lambda case, out, trace: _all(trace, lambda e: e["counts"][1] == e["counts"][2] > e["counts"][0], step=0),
                                net=bias_net([-1.0, 2.0, 2.0]), kw=dict(c_uct=2.0))

# form: (hidden shape, games where the case leaves them open, the cases)
FORMS = {
    "lds": (NARROW, None, tuple(CASES)),
    "global_tree": (NARROW, None, SUBSET),
    "w256": (W256, None, SUBSET + CONT_256),
    "wide_team": (WIDE, 64, SUBSET),
    "wide_layers": (WIDE, 64, SUBSET),
    "wide_acrobot": (WIDE, 64, ACROBOT),
    "population": (NARROW, None, POPULATION),
    "net_search": (NARROW, None, tuple(n for n, _ in NET_SEARCH)),
}
EVERY_GROUP = ("lds", "global_tree", "w256", "wide_team", "wide_layers")


def form_games(form, case):
    """33 games (the case's own number where it sets one); the wide forms need a multiple of 32: 64."""
    n = FORMS[form][1]
    return case.n_games if (n is None or case.n_games != G) else n


# ------------------------------------------------------------------------------------------------ running a case

def run_cpu(case, hidden=NARROW, n_games=None, trace=None, mutant=None, base=BASE):
    n = n_games or case.n_games
    out = SR.cpu_selfplay(case.kw(base), case.desc(hidden), case.blob(hidden), n, case.steps, begin=case.begin, first_roots=case.first_roots(n, base),
                          uploads=case.uploads, trace=trace, mutant=mutant)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, hidden=NARROW, n_games=None, base=BASE):
    """The restatement's run of case ``name``: computed once per process, shared, read-only."""
    return run_cpu(CASES[name], tuple(hidden), n_games, base=base)


@functools.lru_cache(maxsize=None)
def traced(name):
    """(arrays, trace) of case ``name`` at the narrow shape."""
    trace = []
    return run_cpu(CASES[name], NARROW, trace=trace), trace


def carried(e):
    """The root counts an engine would hand to its next search.  The C ABI has no getter: one more search from the resident roots puts
    them into the root's record, whose visit count is the carried count plus the search's simulations."""
    e.search_resident()
    return (e.dump_tree()["node_n"][:, 0] - e.n_sims).astype(np.int32)


def play(e, steps, begin, first_roots=None, uploads=None, population=False):
    """``steps`` self-play steps on a prepared engine (weights set): the restatement's dict, plus the ring's books."""
    (e.population_selfplay_begin if population else e.selfplay_begin)(capacity_steps=steps, **begin)
    if first_roots is not None:
        e.upload_roots(first_roots)
    for s in range(steps):
        if uploads and s in uploads:
            e.upload_roots(*uploads[s](e.selfplay_stats()[2]))
        e.selfplay_step()
    rows = e.selfplay_rows(clear=False)
    fsum, fcnt, state = e.selfplay_stats()
    ring = e.selfplay_ring()
    return dict(rows=rows, fsum=fsum, fcnt=fcnt, state=state, ring=ring, carry=carried(e))


def run_engine(cls, case, hidden=NARROW, n_games=None):
    n = n_games or case.n_games
    e = cls(**dict(case.kw(), n_trees=n))
    try:
        e.set_weights(case.desc(hidden), case.blob(hidden))
        out = play(e, case.steps, case.begin, case.first_roots(n), case.uploads)
        if hasattr(e, "search_info"):
            out["info"] = e.search_info()
    finally:
        e.close()
    return out


def assert_same_bits(got, want, what):
    """rows by their uint32 view, fsum and the env states by their uint64 view, fcnt and the carried counts exact, the ring's books:
    every step stored, none overwritten."""
    for k, view in (("rows", np.uint32), ("fsum", np.uint64), ("state", np.uint64), ("fcnt", None), ("carry", None)):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere((g.view(view) != w.view(view)) if view else (g != w))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"
    if "ring" in got:
        steps = want["rows"].shape[0] // want["fcnt"].shape[0]
        assert got["ring"] == (steps, 0, steps), (what, got["ring"])


def stack_nets(refs):
    """K one-net runs as one population's: rows [step][net][game], the rest net after net."""
    steps = refs[0]["rows"].shape[0] // refs[0]["fcnt"].shape[0]
    rows = np.concatenate([r["rows"].reshape(steps, -1, r["rows"].shape[1]) for r in refs], 1)
    out = {k: np.concatenate([r[k] for r in refs]) for k in ("fsum", "fcnt", "state", "carry")}
    out["rows"] = rows.reshape(-1, rows.shape[2])
    return out
