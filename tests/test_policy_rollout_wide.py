"""Policy rollouts of wide nets (padded width >= 512) on the device: azg_policy_rollout_ex (include/azgym_eval.h), its group form
(rollout_kernel at widths 512 / 1024) and its team form (rollout_team.cuh: 32-game teams of HP/64 workgroups).

The truth is rollout_ref.reference, the CPU rollout composed from the oracle's exports, used as it stands.  Returns, lengths,
terminated flags and first values must be EQUAL: the project's rule, no tolerance.  Where the team form is expected an engine either
reports it or has counted a fall-back (its workgroups were not all resident), the shape of test_population_wide's
_assert_team_or_fell_back."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rollout_ref as R
from alphazero_gym_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

KEYS = ("returns", "lengths", "terminated", "first_value")
BASE = 1000   # game ids of the rollouts here


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _lockstep_shaped(game, net):
    hidden, _, _, ln = net
    return bool(_capi.lockstep_shaped(R.IN_DIM[game], list(hidden), ln))


def _engine(game, net, wseeds, scale=1.0, n_trees=None):
    """A HIP engine of len(wseeds) nets of shape ``net`` = (hidden, head, act, layernorm), net k with weights wseeds[k].  (Several
    nets the engine searches as teams need a multiple of 32 trees each.)"""
    hidden, head, act, ln = net
    K = len(wseeds)
    if n_trees is None:
        n_trees = 32 * K if K > 1 and _lockstep_shaped(game, net) else K
    e = _hip()(**dict(R.GAMES[game], n_trees=n_trees))
    desc = R.net_desc(game, hidden, head, act, ln)
    if K == 1:
        e.set_weights(desc, R.net_blob(game, hidden, head, ln, wseeds[0], scale))
    else:
        e.set_population(K)
        for k, ws in enumerate(wseeds):
            e.set_net_weights(k, desc, R.net_blob(game, hidden, head, ln, ws, scale))
    return e


def _reference(game, net, wseeds, scale, G, max_len, rule, episode=0):
    hidden, head, act, ln = net
    per_net = [R.reference(game, tuple(hidden), head, act, ln, ws, scale, G, max_len, rule, BASE, episode) for ws in wseeds]
    return {k: np.stack([r[k] for r in per_net]) for k in KEYS}


def _assert_equal(got, want, what):
    """Equal by bit pattern (-0.0 is not +0.0), and no float is NaN (a NaN that both sides produce would have equal bits)."""
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.dtype.kind == "f":
            assert not np.isnan(g).any() and not np.isnan(w).any(), f"{what}: {k} holds a NaN"
            g, w = g.view(f"u{g.dtype.itemsize}"), w.view(f"u{w.dtype.itemsize}")
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8].tolist()}: {got[k][tuple(bad[0])]!r} != {want[k][tuple(bad[0])]!r}"


def _assert_form(e, form, what, fallbacks_before=0):
    info = e.last_rollout_info
    print(f"{what}: {info}")
    if form == "team":
        assert info["form"] == "team" or info["team_fallbacks"] > fallbacks_before, (what, info)
    else:
        assert info["form"] == "group" and info["team_fallbacks"] == fallbacks_before, (what, info)
    assert info["launches"] >= 1


# name: game, (hidden, head, activation, layernorm), K, G, max_episode_length, rules, expected form
SHAPES = {
    "r01_cartpole_2x512_relu_K3_G33": ("cartpole", ((512, 512), "discrete", "relu", False), 3, 33, 12, ("sample",), "team"),
    "r02_pendulum_v1_3x1024_elu_K1_G33": ("pendulum_v1", ((1024, 1024, 1024), "normal", "elu", False), 1, 33, 6, ("sample",), "team"),
    "r03_pendulum_v1_4x1024_gmm2_K2_G33": ("pendulum_v1", ((1024,) * 4, "gmm2", "elu", False), 2, 33, 5, ("sample", "mode"), "team"),
    "r04_mountaincar_2x512_relu_K1_G32": ("mountaincar", ((512, 512), "discrete", "relu", False), 1, 32, 8, ("sample",), "team"),
    "r05_mcc_3x512_elu_K3_G40": ("mcc", ((512, 512, 512), "normal", "elu", False), 3, 40, 10, ("sample",), "team"),
    "r06_mcc_2x512_elu_K1_G64": ("mcc", ((512, 512), "normal", "elu", False), 1, 64, 10, ("mode",), "team"),
    # (true width 500: the widest the engine takes below 512 is 449 .. 512, padded to 512; 400 pads to 448, which it refuses)
    "r07_pendulum_v0_2x500_silu_K1_G33": ("pendulum_v0", ((500, 500), "normal", "silu", False), 1, 33, 6, ("sample",), "team"),
    "r08_acrobot_2x512_relu_K3_G17": ("acrobot", ((512, 512), "discrete", "relu", False), 3, 17, 8, ("sample",), "group"),
    "r09_cartpole_2x512_ln_relu_K3_G17": ("cartpole", ((512, 512), "discrete", "relu", True), 3, 17, 10, ("sample",), "group"),
    "r10_pendulum_v0_1x1024_elu_K1_G17": ("pendulum_v0", ((1024,), "normal", "elu", False), 1, 17, 6, ("mode",), "group"),
    "r11_pendulum_v1_3x1024_elu_K2_G1": ("pendulum_v1", ((1024, 1024, 1024), "normal", "elu", False), 2, 1, 6, ("mode",), "team"),
}


def _run_shape(name):
    """(per rule: the engine's arrays and its rollout info) of a row of SHAPES, on a fresh engine"""
    game, net, K, G, max_len, rules, _ = SHAPES[name]
    wseeds = [500 + 7 * k for k in range(K)]
    e = _engine(game, net, wseeds)
    out = {}
    for rule in rules:
        got = e.policy_rollout(G, max_len, rule=rule, game_id_base=BASE)
        out[rule] = (got, dict(e.last_rollout_info))
    return e, out


@pytest.mark.parametrize("name", list(SHAPES))
def test_wide_rollout_equals_cpu_rollout(name):
    game, net, K, G, max_len, rules, form = SHAPES[name]
    assert _lockstep_shaped(game, net) == (form == "team")
    wseeds = [500 + 7 * k for k in range(K)]
    e, out = _run_shape(name)
    try:
        for rule in rules:
            got, info = out[rule]
            print(f"{name} {rule}: {info}")
            _assert_equal(got, _reference(game, net, wseeds, 1.0, G, max_len, rule), f"{name} {rule}")
        _assert_form(e, form, name)
        assert e.search_info()["team_fallbacks"] == 0
    finally:
        e.close()


CARTPOLE_512 = ("cartpole", ((512, 512), "discrete", "relu", False))


def test_frozen_games_inside_one_team():
    """Inside ONE 32-game team some games end early, at several different steps, while others run to the length limit."""
    game, net = CARTPOLE_512
    want = _reference(game, net, [200], 1.0, 32, 14, "sample")
    lengths, term = want["lengths"][0], want["terminated"][0]
    assert len(set(lengths.tolist())) >= 3, lengths
    assert term.any() and (~term).any(), term
    assert (lengths[~term] == 14).all() and (lengths[term] <= 14).all()
    e = _engine(game, net, [200])
    got = e.policy_rollout(32, 14, rule="sample", game_id_base=BASE)
    _assert_form(e, "team", "frozen")
    e.close()
    _assert_equal(got, want, "frozen")


@pytest.mark.parametrize("wseed,G,maxima,at_limit", [(214, 64, (51, 37), 0), (200, 96, (54, 80, 46), 1)])
def test_teams_leave_early_at_different_steps(wseed, G, maxima, at_limit):
    """Every team leaves its loop at its own longest game's end, well before max_episode_length where no game reaches it."""
    game, net = CARTPOLE_512
    max_len = 80
    want = _reference(game, net, [wseed], 1.0, G, max_len, "sample")
    lengths, term = want["lengths"][0], want["terminated"][0]
    assert tuple(int(lengths[i:i + 32].max()) for i in range(0, G, 32)) == maxima, lengths
    assert int((lengths == max_len).sum()) == at_limit, lengths
    if at_limit == 0:
        assert term.all() and lengths.max() < max_len, (lengths, term)   # every game ends by itself, none at the limit
    e = _engine(game, net, [wseed])
    got = e.policy_rollout(G, max_len, rule="sample", game_id_base=BASE)
    _assert_form(e, "team", f"early exit {wseed}")
    e.close()
    _assert_equal(got, want, f"early exit {wseed}")


@pytest.mark.parametrize("name", ["r01_cartpole_2x512_relu_K3_G33", "r02_pendulum_v1_3x1024_elu_K1_G33"])
def test_forms_agree(name, monkeypatch):
    """AZG_LS_TEAM=0 forces the group form: the same arrays as the team run's."""
    rule = SHAPES[name][5][0]
    e, out = _run_shape(name)
    _assert_form(e, "team", name)
    e.close()
    monkeypatch.setenv("AZG_LS_TEAM", "0")
    g, out_g = _run_shape(name)
    _assert_form(g, "group", name + " AZG_LS_TEAM=0")
    assert g.last_rollout_info["launches"] == 1
    g.close()
    _assert_equal(out_g[rule][0], out[rule][0], name)


def test_orderly_give_up(monkeypatch):
    """AZG_TEAM_SPIN_LIMIT=0: every wait of the team kernel counts as timed out, it leaves through its abort flag, the call is replayed
    in the group form and the engine's later rollouts take that form; the search's own fall-back count is not touched."""
    name = "r01_cartpole_2x512_relu_K3_G33"
    game, net, K, G, max_len, rules, _ = SHAPES[name]
    wseeds = [500 + 7 * k for k in range(K)]
    want = _reference(game, net, wseeds, 1.0, G, max_len, rules[0])
    monkeypatch.setenv("AZG_TEAM_SPIN_LIMIT", "0")
    e = _engine(game, net, wseeds)
    got = e.policy_rollout(G, max_len, rule=rules[0], game_id_base=BASE)
    first = dict(e.last_rollout_info)
    again = e.policy_rollout(G, max_len, rule=rules[0], game_id_base=BASE)
    second = dict(e.last_rollout_info)
    fallbacks = e.search_info()["team_fallbacks"]
    e.close()
    print(first, second)
    _assert_equal(got, want, "give-up")
    _assert_equal(again, want, "after the give-up")
    assert first["form"] == "group" and first["team_fallbacks"] == 1 and first["launches"] >= 2, first
    assert second == {"form": "group", "team_fallbacks": 1, "launches": 1}, second
    assert fallbacks == 0


def test_several_launches(monkeypatch):
    """AZG_ROLLOUT_TEAMS=n caps the teams of one launch: row 1's six teams run as successive launches with the same outputs."""
    name = "r01_cartpole_2x512_relu_K3_G33"
    game, net, K, G, max_len, rules, _ = SHAPES[name]
    wseeds = [500 + 7 * k for k in range(K)]
    want = _reference(game, net, wseeds, 1.0, G, max_len, rules[0])
    for cap, launches in (("4", 2), ("1", 6)):
        monkeypatch.setenv("AZG_ROLLOUT_TEAMS", cap)
        e = _engine(game, net, wseeds)
        got = e.policy_rollout(G, max_len, rule=rules[0], game_id_base=BASE)
        info = dict(e.last_rollout_info)
        e.close()
        print(cap, info)
        _assert_equal(got, want, f"cap {cap}")
        assert info["form"] == "group" and info["team_fallbacks"] == 1 or (info["form"] == "team" and info["launches"] == launches), info


@pytest.mark.parametrize("game,net,rule", [("cartpole", ((512, 512), "discrete", "relu", False), "sample"),
                                           ("pendulum_v0", ((512, 512, 512), "gmm2", "elu", False), "sample"),
                                           ("mcc", ((512, 512), "normal", "elu", False), "mode")])
def test_population_invariance(game, net, rule):
    """Net k of a K = 3 rollout is what a one-net engine with net k's weights plays under the same config."""
    wseeds = [500, 507, 514]
    pop = _engine(game, net, wseeds)
    got = pop.policy_rollout(17, 9, rule=rule, game_id_base=BASE, episode=2)
    _assert_form(pop, "team", "population")
    pop.close()
    for k, ws in enumerate(wseeds):
        one = _engine(game, net, [ws])
        alone = one.policy_rollout(17, 9, rule=rule, game_id_base=BASE, episode=2)
        one.close()
        for key in KEYS:
            np.testing.assert_array_equal(got[key][k], alone[key][0], err_msg=f"net {k} {key}")


def test_common_start_states():
    """Game j starts from the same state for every net: identical weights give identical arrays; different weights differ in the
    value of that common start state.  Another ``episode`` is another set of start states."""
    game, net = "pendulum_v1", ((512, 512), "normal", "elu", False)
    same = _engine(game, net, [510, 510, 510])
    got = same.policy_rollout(17, 8, rule="sample", game_id_base=BASE)
    other = same.policy_rollout(17, 8, rule="sample", game_id_base=BASE, episode=1)
    same.close()
    for k in KEYS:
        for n in (1, 2):
            np.testing.assert_array_equal(got[k][n], got[k][0], err_msg=k)
    assert (other["first_value"] != got["first_value"]).all()
    diff = _engine(game, net, [510, 517, 524])
    got_d = diff.policy_rollout(17, 8, rule="sample", game_id_base=BASE)
    diff.close()
    np.testing.assert_array_equal(got_d["first_value"][0], got["first_value"][0])
    assert (got_d["first_value"][1] != got_d["first_value"][0]).all() and (got_d["first_value"][2] != got_d["first_value"][0]).all()


def test_no_side_effects_on_search():
    """A wide search's results and its launch record are still there after a team rollout, and the same search gives them again."""
    game, net = "pendulum_v1", ((512, 512), "normal", "elu", False)
    e = _engine(game, net, [500, 507], n_trees=64)
    roots = e.synthetic_roots()
    e.set_search_index(3)
    e.search(roots)
    before, info_before = e.results(), e.search_info()
    e.policy_rollout(33, 6, rule="sample", game_id_base=BASE)
    _assert_form(e, "team", "between searches")
    after, info_after = e.results(), e.search_info()
    e.set_search_index(3)
    e.search(roots)
    again, info_again = e.results(), e.search_info()
    e.close()
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
        np.testing.assert_array_equal(again[k], before[k], err_msg=k)
    drop = ("last_ms",)
    assert {k: v for k, v in info_after.items() if k not in drop} == {k: v for k, v in info_before.items() if k not in drop}
    assert {k: v for k, v in info_again.items() if k not in drop} == {k: v for k, v in info_before.items() if k not in drop}


def test_no_side_effects_on_selfplay():
    """Two wide self-play populations with the same seeds play 3 steps; one evaluates between step 1 and step 2: same rows, ring, stats."""
    import torch
    from alphazero_gym_amd import run
    from selfplay_train import build_agent
    _hip()

    def make():
        nets = []
        for s in (3, 11):
            torch.manual_seed(s)
            nets.append(build_agent("CartPole-v0", [512, 512], 6, "cpu", 1e-3)[0].nn)
        return run.PopulationSelfPlay(nets, game="CartPole-v0", games_per_net=32, n_rollouts=6, c_uct=1.0, max_episode_length=2,
                                      capacity_steps=4, seed=5)
    a, b = make(), make()
    a.play(1)
    b.play(1)
    ev = a.evaluate(33, rule="sample", max_episode_length=20)
    _assert_form(a.engine, "team", "between self-play steps")
    assert ev["returns"].shape == (2, 33) and ev["mean_return"].shape == (2,)
    np.testing.assert_array_equal(ev["returns"], ev["lengths"].astype(np.float64))   # CartPole pays 1 per step
    a.play(2)
    b.play(2)
    assert a.engine.selfplay_ring() == b.engine.selfplay_ring()
    np.testing.assert_array_equal(a.engine.selfplay_rows(clear=False), b.engine.selfplay_rows(clear=False))
    for x, y in zip(a.finished_returns(), b.finished_returns()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.engine.selfplay_stats(), b.engine.selfplay_stats()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


def test_abi_errors_of_the_new_entry():
    """Every refusal of azg_policy_rollout holds for azg_policy_rollout_ex but the width one; a wrong info size is refused, a NULL
    info accepted; nothing is written on an error.  The old entry still refuses the wide engine."""
    from alphazero_gym_amd import _native
    f = _native.fns()
    rollout_ex, rollout_old, last_error = f["policy_rollout_ex"], f["policy_rollout"], f["last_error"]
    G = 4
    out = None

    def sentinels():
        return (np.full((3, G), -7.5), np.full((3, G), -7, np.int32), np.full((3, G), -7, np.int32), np.full((3, G), -7.5, np.float32))

    def cfg(**over):
        c = _capi.AzgRolloutConfig()
        c.struct_size = C.sizeof(_capi.AzgRolloutConfig)
        c.episodes_per_net, c.max_episode_length, c.action_rule, c.game_id_base, c.episode = G, 5, 0, BASE, 0
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def new_info(size=None):
        i = _capi.AzgRolloutInfo()
        i.struct_size = C.sizeof(_capi.AzgRolloutInfo) if size is None else size
        i.form, i.launches, i.team_fallbacks = -7, -7, -7
        return i

    def call(e, c, skip=(), info=None, fn=None):
        nonlocal out
        out = sentinels()
        ptrs = [_capi._ptr(out[0], C.c_double), _capi._ptr(out[1], C.c_int32), _capi._ptr(out[2], C.c_int32), _capi._ptr(out[3], C.c_float)]
        for i in skip:
            ptrs[i] = None
        args = [e._h if e is not None else None, C.byref(c) if c is not None else None, *ptrs]
        if fn is not None:
            return fn(*args)
        return rollout_ex(*args, C.byref(info) if info is not None else None)

    def refused(e, code, c, skip=(), message=True, info=None, fn=None):
        assert call(e, c, skip, info, fn) == code
        if message:
            assert (last_error(e._h) or b"").decode() != ""
        for arr, s in zip(out, sentinels()):
            np.testing.assert_array_equal(arr, s)
        if info is not None:
            assert (info.form, info.launches, info.team_fallbacks) == (-7, -7, -7)

    game, net = CARTPOLE_512
    e = _engine(game, net, [500, 507, 514])
    refused(None, _capi.AZG_E_INVALID, cfg(), message=False, info=new_info())
    refused(e, _capi.AZG_E_INVALID, None, info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(), skip=(0,), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(), skip=(1,), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(struct_size=8), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(episodes_per_net=0), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(max_episode_length=0), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(action_rule=2), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(action_rule=-1), info=new_info())
    refused(e, _capi.AZG_E_INVALID, cfg(), info=new_info(size=12))
    refused(e, _capi.AZG_E_INVALID, cfg(), info=new_info(size=0))
    # the old entry still refuses this engine's width
    refused(e, _capi.AZG_E_UNSUPPORTED, cfg(), fn=rollout_old)
    # terminated, first_value and info may be NULL
    assert call(e, cfg(), skip=(2, 3)) == 0
    assert (out[1] > 0).all() and (out[2] == -7).all() and (out[3] == -7.5).all()
    info = new_info()
    assert call(e, cfg(), info=info) == 0
    assert info.form in (0, 1) and info.launches >= 1 and info.team_fallbacks in (0, 1)
    assert (out[1] > 0).all() and (out[3] != -7.5).all()
    # a net without weights: a fresh population, two of three nets uploaded
    e.set_population(1)
    e.set_population(3)
    desc = R.net_desc(game, *net)
    for k in (0, 1):
        e.set_net_weights(k, desc, R.net_blob(game, net[0], net[1], net[3], 500 + k))
    refused(e, _capi.AZG_E_STATE, cfg(), info=new_info())
    e.close()
    fresh = _hip()(**dict(R.GAMES[game], n_trees=3))
    refused(fresh, _capi.AZG_E_STATE, cfg(), info=new_info())
    # widths up to 256: the new entry does what the old one does, in the group form
    narrow = ((128, 128), "discrete", "relu", False)
    fresh.set_weights(R.net_desc(game, *narrow), R.net_blob(game, narrow[0], narrow[1], False, 500))
    small = lambda: (np.full((1, G), -7.5), np.full((1, G), -7, np.int32), np.full((1, G), -7, np.int32), np.full((1, G), -7.5, np.float32))  # noqa: E731
    a, b = small(), small()
    info = new_info()
    pa = [_capi._ptr(a[0], C.c_double), _capi._ptr(a[1], C.c_int32), _capi._ptr(a[2], C.c_int32), _capi._ptr(a[3], C.c_float)]
    pb = [_capi._ptr(b[0], C.c_double), _capi._ptr(b[1], C.c_int32), _capi._ptr(b[2], C.c_int32), _capi._ptr(b[3], C.c_float)]
    assert rollout_old(fresh._h, C.byref(cfg()), *pa) == 0 and rollout_ex(fresh._h, C.byref(cfg()), *pb, C.byref(info)) == 0
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert (info.form, info.launches, info.team_fallbacks) == (0, 1, 0)
    fresh.close()


def test_example_wide_eval_return():
    _hip()
    import population_selfplay_train as P
    a = P.parse_args(["--game", "CartPole-v0", "--hidden", "512", "512", "--wide", "--seeds", "3", "11", "--games-per-seed", "32",
                      "--eval-episodes", "32", "--n-rollouts", "6", "--iters", "2", "--steps-per-iter", "6", "--train-rows", "20",
                      "--batch-size", "8", "--max-episode-length", "8", "--device", "cpu"])
    hist = P.train(a, log=None)
    assert len(hist) == 2
    for rec in hist:
        assert len(rec["eval_return"]) == 2 and np.isfinite(rec["eval_return"]).all()
        assert all(1.0 <= x <= 8.0 for x in rec["eval_return"])   # CartPole: one per step, at most max_episode_length steps
