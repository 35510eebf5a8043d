"""GPU (-m gpu): policy rollouts at the edges of the policy heads, every kernel form against the CPU rollout, by bit pattern.

The cases are tests/rollout_edges.py's hand-built nets (tied logits, softmax shares of exactly 0 and 1, log sigma on and beside both
clamps, a saturated squash, mu at and next to zero, a head sum that depends on its order, a mixture at its limits, two bang-bang
policies whose games all terminate); what each contains is asserted on the CPU in tests/test_rollout_edges_host.py.  Here each runs
in every form of the rollout that takes it, G = 33 games (one full team or two full groups, and one game more):

  resident   (64, 64):           rollout_kernel<64, 1>, the hidden->hidden layer in registers (azg_policy_rollout's entry)
  streamed   (64, 64, 64, 64):   rollout_kernel<64, 0> -- three hidden->hidden layers: engine_weights.hip's resident_layers keeps up
                                 to two in registers at this width, so three hidden layers would still be the resident form
  group      (500, 500), AZG_LS_TEAM=0: rollout_kernel<512, 0>
  team       (500, 500):         rollout_team_kernel<512>, or a counted fall-back
  team1024   (1024, 1024):       rollout_team_kernel<1024> (NU = 16, two games per workgroup), one case per head

and is compared with the CPU rollout OF THE SAME SHAPE: returns as uint64, first_value as uint32, lengths and flags exact, nothing
NaN (rollout_edges.assert_same_bits).  No tolerance anywhere.  One engine per (game, head, form) serves its cases in turn."""
import os
import re

import numpy as np
import pytest

import rollout_edges as RE
import rollout_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("returns", "lengths", "terminated", "first_value")
FORMS = {"resident": RE.NARROW, "streamed": RE.STREAMED, "group": RE.WIDE, "team": RE.WIDE, "team1024": RE.WIDE_1024}
W512 = (512, 512)


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _create(game, n_trees, group):
    """A HIP engine; group: created under AZG_LS_TEAM=0 (the engine reads its switches when it is created)."""
    old = os.environ.get("AZG_LS_TEAM")
    if group:
        os.environ["AZG_LS_TEAM"] = "0"
    try:
        return _hip()(**dict(R.GAMES[game], n_trees=n_trees))
    finally:
        if group:
            if old is None:
                del os.environ["AZG_LS_TEAM"]
            else:
                os.environ["AZG_LS_TEAM"] = old


@pytest.fixture(scope="module")
def engines():
    """One-net engines by (game, head, form), created on first use and closed with the module."""
    made = {}

    def get(game, head, form):
        if (game, head, form) not in made:
            made[(game, head, form)] = _create(game, 1, form == "group")
        return made[(game, head, form)]
    yield get
    for e in made.values():
        e.close()


def _assert_form(e, form, what):
    """test_policy_rollout_wide's _assert_form: the team form, or a counted fall-back (its workgroups were not all resident); every
    other form is the group kernel's, without one"""
    info = e.last_rollout_info
    if form.startswith("team"):
        print(f"{what}: {info}")
        assert info["form"] == "team" or info["team_fallbacks"] > 0, (what, info)
    else:
        assert info["form"] == "group" and info["team_fallbacks"] == 0, (what, info)
    assert info["launches"] >= 1


def _stack(refs):
    return {k: np.stack([r[k] for r in refs]) for k in KEYS}


def _device_cases():
    out = [(form, name) for form in ("resident", "streamed", "group", "team") for name in RE.CASES]
    return out + [("team1024", name) for name in RE.AT_1024]


@pytest.mark.parametrize("form,name", _device_cases())
def test_edge_case_equals_cpu_rollout(engines, form, name):
    case, hidden = RE.CASES[name], FORMS[form]
    want = RE.reference(name, hidden)
    e = engines(case.game, case.head, form)
    e.set_weights(case.desc(hidden), case.blob(hidden))
    got = e.policy_rollout(RE.G, case.max_len, rule=case.rule, game_id_base=RE.BASE)
    _assert_form(e, form, f"{name} {form}")
    RE.assert_same_bits(got, _stack([want]), f"{name} {form}")


@pytest.mark.parametrize("form,nreg", [("resident", "1"), ("streamed", "0")])
def test_narrow_shapes_take_the_forms_they_are_named_for(form, nreg):
    """dispatch_rollout picks rollout_kernel<HP, NREG> by the engine's count of register-resident layers, the one its searches use:
    search_info's kernel name (search_kernel<ENV, HP, NREG, ...>) after a search of the same net shows it."""
    case, hidden = RE.CASES["D2_tie_at_1_mode"], FORMS[form]
    e = _create(case.game, 1, False)
    try:
        e.set_weights(case.desc(hidden), case.blob(hidden))
        e.set_search_index(3)
        e.search(e.synthetic_roots())
        name = e.search_info()["kernel_name"]
    finally:
        e.close()
    m = re.fullmatch(r"search_kernel<(.*)>", name)
    assert m, name
    args = [a.strip() for a in m.group(1).split(",")]
    assert args[1:3] == ["64", nreg], name


def test_population_of_edges_in_one_call():
    """K = 3 CartPole nets at (512, 512) in one call, 32 trees each, sample rule: a one-hot net (D4), a tie net (D1) and a
    make_weights net, against three one-net CPU rollouts.  Their longest games differ, so the nets' teams leave at different steps."""
    game, max_len = "cartpole", 60
    one_hot, tie = RE.CASES["D4_onehot_lo_sample"], RE.CASES["D1_tie_cartpole_sample"]
    desc = one_hot.desc(W512)
    refs = [RE.reference(one_hot.name, W512, max_len), RE.reference(tie.name, W512, max_len),
            R.reference(game, W512, "discrete", RE.ACT, False, 214, 1.0, RE.G, max_len, "sample", RE.BASE, 0)]
    longest = [int(r["lengths"].max()) for r in refs]
    assert len(set(longest)) == 3 and max(longest) < max_len, longest
    e = _create(game, 3 * 32, False)
    try:
        e.set_population(3)
        for k, blob in enumerate((one_hot.blob(W512), tie.blob(W512), R.net_blob(game, W512, "discrete", False, 214))):
            e.set_net_weights(k, desc, blob)
        got = e.policy_rollout(RE.G, max_len, rule="sample", game_id_base=RE.BASE)
        _assert_form(e, "team", f"population of edges, longest games {longest}")
    finally:
        e.close()
    RE.assert_same_bits(got, _stack(refs), "population of edges")


@pytest.mark.parametrize("game,edge,head", [("cartpole", "D1_tie_cartpole_sample", "discrete"), ("pendulum_v0", "N1_ls_min_below", "normal")])
@pytest.mark.parametrize("max_len", [1, 2, 3])
def test_short_loops_in_the_team_form(game, edge, head, max_len):
    """max_episode_length 1, 2, 3 at (512, 512), K = 2 (an edge net and a make_weights net), G = 33: the live counts' parity words are
    used once (1), both once (2), the first one again (3).  Nothing terminates."""
    case = RE.CASES[edge]
    refs = [RE.reference(edge, W512, max_len), R.reference(game, W512, head, RE.ACT, False, 507, 1.0, RE.G, max_len, case.rule, RE.BASE, 0)]
    for r in refs:
        assert (r["lengths"] == max_len).all() and not r["terminated"].any()
    e = _create(game, 2 * 32, False)
    try:
        e.set_population(2)
        e.set_net_weights(0, case.desc(W512), case.blob(W512))
        e.set_net_weights(1, case.desc(W512), R.net_blob(game, W512, head, False, 507))
        got = e.policy_rollout(RE.G, max_len, rule=case.rule, game_id_base=RE.BASE)
        _assert_form(e, "team", f"short loop {game} {max_len}")
    finally:
        e.close()
    assert (got["lengths"] == max_len).all() and not got["terminated"].any()
    RE.assert_same_bits(got, _stack(refs), f"short loop {game} {max_len}")


def test_second_call_and_another_episode_on_one_team_engine():
    """The rollout's counters and buffers are grow-only and re-used: after a 200-step call whose games all terminate, a second, shorter
    call with another episode (other start states) on the same engine equals its own CPU rollout, and so does the first call again."""
    name = "D5_bangbang_sample"
    case = RE.CASES[name]
    first, second = RE.reference(name, RE.WIDE), RE.reference(name, RE.WIDE, 60, 3)
    assert (second["lengths"] != first["lengths"]).any() and (~second["terminated"]).any()
    e = _create(case.game, 1, False)
    try:
        e.set_weights(case.desc(RE.WIDE), case.blob(RE.WIDE))
        got = []
        for max_len, episode in ((case.max_len, 0), (60, 3), (case.max_len, 0)):
            got.append(e.policy_rollout(RE.G, max_len, rule=case.rule, game_id_base=RE.BASE, episode=episode))
            _assert_form(e, "team", f"call {len(got)} on one engine")
    finally:
        e.close()
    for g, want, what in zip(got, (first, second, first), ("first call", "second call, episode 3", "first call again")):
        RE.assert_same_bits(g, _stack([want]), what)
