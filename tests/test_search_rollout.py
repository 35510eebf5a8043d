"""Search rollouts (azg_search_rollout, run.PopulationSelfPlay.evaluate_search) on the GPU: bit equality with the CPU truth, independence
of the polling interval, non-interference with device self-play, population invariance, repeatability, the refusals and the Python
layer.  Cases, sizes and the CPU truth: tests/search_rollout_util.py."""
import numpy as np
import pytest

import reanalyse_util as R
import search_rollout_util as U
from alphazero_gym_amd import _capi
from selfplay_ref import assert_stats_bits

ALL = sorted(U.CASES)
RES_KEYS = ("counts", "n_children", "actions", "Q", "v_target")


def _hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _engine(name, monkeypatch):
    case = U.CASES[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    return case, R.make_engine(_hip(), case)


def _call(e, name, poll_steps=1, **over):
    cfg = U.config(name, **over)
    return e.search_rollout(cfg.pop("episodes_per_game"), cfg.pop("max_episode_length"), poll_steps=poll_steps, **cfg)


def _code(fn, *a, **kw):
    with pytest.raises(_capi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_rollouts_equal_the_cpu_truth(name, monkeypatch):
    """1.  returns, lengths, terminated and, looking at the count of unfinished games after every step, the number of searches (the
    largest game total) equal the CPU truth bit for bit, on an engine that never began self-play.  The call's last search is the
    engine's last search: results() are the oracle's for it, parked games' trees (searched from their parked roots) included."""
    want = U.truth(name)
    case, e = _engine(name, monkeypatch)
    got = _call(e, name, poll_steps=1)
    info = e.search_info()
    res = {k: np.array(v) for k, v in e.results().items()}
    e.close()
    U.assert_same(got, want, name)
    assert got["steps"] == want["steps"] == int(want["totals"].max())
    assert got["polls"] == min(got["steps"], U.E * U.config(name)["max_episode_length"] - 1)
    if name.endswith("_team"):
        assert info["kernel_form"] in ("team", "per_layer"), info
    else:
        assert info["kernel_form"] == "persistent", info
    if name == "many_children":
        assert info["max_children"] == 20 and (info["tree_storage"], info["lds_exit"]) == ("global", "children"), info
    if name.endswith("_global_tree"):
        assert (info["tree_storage"], info["lds_exit"]) == ("global", "forced"), info
    if "last" in want:
        for k in RES_KEYS:
            a, b = res[k], want["last"][k]
            if a.ndim == 2:
                a = a[:, :b.shape[1]]
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: last search, {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole_falls", "pendulum"])
def test_outputs_do_not_depend_on_the_polling_interval(name, monkeypatch):
    """2.  poll_steps 1, 3 and 1000 give identical outputs; only the number of searches differs (1000: the hard bound)."""
    want = U.truth(name)
    case, e = _engine(name, monkeypatch)
    bound = U.E * U.config(name)["max_episode_length"]
    for poll, steps, polls in ((1, want["steps"], None), (3, min(-(-want["steps"] // 3) * 3, bound), None), (1000, bound, 0)):
        got = _call(e, name, poll_steps=poll)
        U.assert_same(got, want, f"{name} poll_steps {poll}")
        assert got["steps"] == steps, (poll, got["steps"])
        assert polls is None or got["polls"] == polls
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cartpole", "pendulum", "population", "wide_team"])
def test_a_rollout_does_not_disturb_the_selfplay(name, monkeypatch):
    """3.  Self-play of 4 steps with an evaluation between steps 2 and 3 against a run without it, bit for bit: the ring's rows, the
    episode statistics and the games' states, the ring's books, the kept states -- and the next search (the running index came
    back).  cartpole: carried counts are in flight when the evaluation runs."""
    engines = []
    for with_eval in (False, True):
        case, e = _engine(name, monkeypatch)
        R.begin(e, case, 4)
        for s in range(4):
            if with_eval and s == 2:
                U.assert_same(_call(e, name, poll_steps=3), U.truth(name), name)
                assert e.selfplay_ring() == (2, 0, 2)
            e.selfplay_step()
        engines.append(e)
    a, b = engines
    np.testing.assert_array_equal(R.bits32(R.ring(b, case)), R.bits32(R.ring(a, case)))
    assert_stats_bits(b.selfplay_stats(), a.selfplay_stats(), name)
    assert a.selfplay_ring() == b.selfplay_ring() == (4, 0, 4)
    np.testing.assert_array_equal(R.bits64(b.selfplay_states()), R.bits64(a.selfplay_states()))
    for e in engines:
        e.search_resident()
    ra, rb = a.results(), b.results()
    for k in RES_KEYS:
        np.testing.assert_array_equal(np.array(rb[k]), np.array(ra[k]), err_msg=k)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["population", "population_wide"])
def test_net_k_of_a_population_is_a_one_net_engine(name, monkeypatch):
    """4.  On the engine alone: net k's games of the K-net call equal the call of a one-net engine created with net_kw(k) -- its
    tree ids, table entry and budget -- over the same start states."""
    case, e = _engine(name, monkeypatch)
    got = _call(e, name)
    e.close()
    T = case.T
    for k in range(case.nets):
        one = _hip()(**dict(case.net_kw(k), n_trees=T))
        one.set_weights(case.desc(), case.blob(k))
        solo = _call(one, name)
        one.close()
        U.assert_same({key: got[key][k * T:(k + 1) * T] for key in ("returns", "lengths", "terminated")}, solo, f"{name} net {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pendulum", "cartpole_falls"])
def test_calls_repeat_and_their_keys_matter(name, monkeypatch):
    """5.  The same index_base gives the same results, with other searches in between; another episode (other start states) or another
    index_base (other draws) changes them."""
    case, e = _engine(name, monkeypatch)
    first = _call(e, name, poll_steps=8)
    e.search_resident()
    again = _call(e, name, poll_steps=8)
    U.assert_same(again, first, name)
    assert not U.same(_call(e, name, episode=U.CFG["episode"] + U.E), first)
    assert not U.same(_call(e, name, index_base=U.INDEX_BASE + 1000), first)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "population"])
def test_refusals_leave_everything_alone(name, monkeypatch):
    """6.  Every refusal returns its code and leaves the outputs, the ring and the stats untouched."""
    case, e = _engine(name, monkeypatch)
    R.begin(e, case, 4, keep=False)
    for _ in range(2):
        e.selfplay_step()
    rows, stats, ring = R.ring(e, case).copy(), e.selfplay_stats(), e.selfplay_ring()
    shape = (case.games, U.E)
    out = (np.full(shape, -7.5), np.full(shape, -7, np.int32), np.full(shape, -7, np.int32))
    bad = [(dict(episodes_per_game=0), _capi.AZG_E_INVALID), (dict(max_episode_length=0), _capi.AZG_E_INVALID),
           (dict(final_selection=2), _capi.AZG_E_INVALID), (dict(temperature=0.0), _capi.AZG_E_INVALID),
           (dict(temperature=-1.0), _capi.AZG_E_INVALID), (dict(agent_epsilon=-0.01), _capi.AZG_E_INVALID),
           (dict(agent_epsilon=1.01), _capi.AZG_E_INVALID)]
    if not case.cont:
        bad.append((dict(final_selection="max_value", temperature=0.5), _capi.AZG_E_UNSUPPORTED))
    for over, code in bad:
        cfg = U.config(name, **over)
        E = cfg.pop("episodes_per_game")
        o = out if E == U.E else None
        assert _code(e.search_rollout, E, cfg.pop("max_episode_length"), out=o, **cfg) == code, over
    cfg = U.config(name)
    assert _code(e.search_rollout, cfg.pop("episodes_per_game"), cfg.pop("max_episode_length"), poll_steps=0, out=out, **cfg) == _capi.AZG_E_INVALID
    fn = e._f["search_rollout"]   # NULL arguments and struct sizes, below the Python layer
    import ctypes as C
    c, info = _capi.AzgSearchRolloutConfig(), _capi.AzgSearchRolloutInfo()
    c.struct_size, c.episodes_per_game, c.max_episode_length, c.poll_steps, c.temperature = C.sizeof(c), U.E, 3, 1, 1.0
    info.struct_size = C.sizeof(info)
    ptrs = (_capi._ptr(out[0], C.c_double), _capi._ptr(out[1], C.c_int32), _capi._ptr(out[2], C.c_int32))
    assert fn(e._h, None, *ptrs, C.byref(info)) == _capi.AZG_E_INVALID
    assert fn(e._h, C.byref(c), None, ptrs[1], ptrs[2], C.byref(info)) == _capi.AZG_E_INVALID
    assert fn(e._h, C.byref(c), ptrs[0], None, ptrs[2], C.byref(info)) == _capi.AZG_E_INVALID
    c.struct_size -= 4
    assert fn(e._h, C.byref(c), *ptrs, C.byref(info)) == _capi.AZG_E_INVALID
    c.struct_size += 4
    info.struct_size += 4
    assert fn(e._h, C.byref(c), *ptrs, C.byref(info)) == _capi.AZG_E_INVALID
    assert (out[0] == -7.5).all() and (out[1] == -7).all() and (out[2] == -7).all()
    np.testing.assert_array_equal(R.bits32(R.ring(e, case)), R.bits32(rows))
    assert_stats_bits(e.selfplay_stats(), stats, name)
    assert e.selfplay_ring() == ring
    U.assert_same(_call(e, name), U.truth(name), name)   # (the engine still works)
    e.close()


@pytest.mark.gpu
def test_refusals_of_the_search_come_through(monkeypatch):
    """6, last items: temperature != 1 beyond 2048 simulations, weights not set, and a settings table on nets of width 512 that came
    without the wide flag are refused with their codes before anything is written; once the table is gone the call runs."""
    shape = (2, 1)
    out = (np.full(shape, -7.5), np.full(shape, -7, np.int32), np.full(shape, -7, np.int32))
    big = _hip()(env_id=0, mode=0, n_trees=2, n_sims=2049, c_uct=1.5, gamma=1.0, num_actions=2)
    assert _code(big.search_rollout, 1, 3, out=out) == _capi.AZG_E_STATE            # no weights
    big.set_weights(_capi.make_desc(4, [64], 2, "relu"), U.O.make_weights(1, 4, [64], 2))
    assert _code(big.search_rollout, 1, 3, deterministic=False, temperature=0.5, out=out) == _capi.AZG_E_UNSUPPORTED
    big.close()
    assert (out[0] == -7.5).all() and (out[1] == -7).all() and (out[2] == -7).all()
    case, e = _engine("population_wide", monkeypatch)
    shape = (case.games, U.E)
    out = (np.full(shape, -7.5), np.full(shape, -7, np.int32), np.full(shape, -7, np.int32))
    e.set_net_search([dict(c_uct=0.05, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)] * case.nets)
    cfg = U.config("population_wide")
    assert _code(e.search_rollout, cfg.pop("episodes_per_game"), cfg.pop("max_episode_length"), out=out, **cfg) == _capi.AZG_E_UNSUPPORTED
    assert (out[0] == -7.5).all() and (out[1] == -7).all() and (out[2] == -7).all()
    e.set_net_search(None)
    U.assert_same(_call(e, "population_wide"), U.truth("population_wide"), "population_wide")
    e.close()


@pytest.mark.gpu
def test_population_selfplay_evaluate_search():
    """7.  run.PopulationSelfPlay.evaluate_search, two CartPole seeds: the shapes, mean_return is the row mean, the default call
    repeats, it is the engine's call under EVAL_SEARCH_INDEX_BASE over evaluate's start states, weights changed on the host are
    picked up, and a following play continues as if no evaluation had run."""
    import torch
    from alphazero_gym_amd import run
    from alphazero_gym_amd.network.policies import make_policy

    def nets():
        out = []
        for s in range(2):
            torch.manual_seed(60 + s)
            out.append(make_policy(4, 1, "discrete", [64, 64], "relu", num_actions=2))
        return out
    T, E, L = 11, 2, 6
    kw = dict(game="CartPole-v0", games_per_net=T, n_rollouts=8, c_uct=1.5, max_episode_length=L, capacity_steps=4, seed=21)
    plain, sp = run.PopulationSelfPlay(nets(), **kw), run.PopulationSelfPlay(nets(), **kw)
    for x in (plain, sp):
        x.play(2)
    ev = sp.evaluate_search(E)
    assert ev["returns"].shape == ev["lengths"].shape == ev["terminated"].shape == (2, T, E)
    assert ev["returns"].dtype == np.float64 and ev["terminated"].dtype == bool
    np.testing.assert_array_equal(ev["mean_return"], ev["returns"].reshape(2, -1).mean(axis=1))
    assert 1 <= ev["steps"] <= E * L and (ev["lengths"] >= 1).all() and (ev["lengths"] <= L).all()
    np.testing.assert_array_equal(ev["returns"], ev["lengths"].astype(np.float64))   # (CartPole pays 1 per step)
    again = sp.evaluate_search(E)
    np.testing.assert_array_equal(R.bits64(again["returns"]), R.bits64(ev["returns"]))
    raw = sp.engine.search_rollout(E, L, game_id_base=run.EVAL_GAME_ID_BASE, index_base=run.EVAL_SEARCH_INDEX_BASE)
    np.testing.assert_array_equal(R.bits64(raw["returns"].reshape(2, T, E)), R.bits64(ev["returns"]))
    for x in (plain, sp):
        x.play(2)
    np.testing.assert_array_equal(R.bits32(sp.engine.selfplay_rows(clear=False)), R.bits32(plain.engine.selfplay_rows(clear=False)))
    assert_stats_bits(sp.engine.selfplay_stats(), plain.engine.selfplay_stats(), "evaluate_search")
    long = sp.evaluate_search(E, max_episode_length=32)   # (long enough for the poles to fall: the lengths tell the nets apart)
    with torch.no_grad():
        for p in sp.policies[1].parameters():
            p.mul_(-1.5)
    new = sp.evaluate_search(E, max_episode_length=32)
    assert sp.last_weight_sync is not None
    np.testing.assert_array_equal(new["lengths"][0], long["lengths"][0])   # (net 0 is unchanged)
    assert not np.array_equal(new["lengths"][1], long["lengths"][1])
    with pytest.raises(ValueError):
        sp.evaluate_search(0)
    plain.close()
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("example,extra", [("selfplay_train", ["--games", "16"]),
                                           ("population_selfplay_train", ["--seeds", "0", "1", "--games-per-seed", "8", "--eval-episodes", "8"])])
def test_examples_report_the_return_under_search(example, extra):
    """--eval-search-episodes 1: every iteration's record carries eval_search_return (per seed in the population example, beside the
    raw policy's eval_return)."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    mod = importlib.import_module(example)
    a = mod.parse_args(["--game", "CartPole-v0", "--n-rollouts", "8", "--iters", "2", "--steps-per-iter", "2", "--hidden", "16", "16",
                        "--train-rows", "32", "--batch-size", "8", "--max-episode-length", "5", "--eval-search-episodes", "1", "--device", "cuda"] + extra)
    hist = mod.train(a, log=None)
    assert len(hist) == 2
    for h in hist:
        got = np.atleast_1d(np.asarray(h["eval_search_return"], np.float64))
        assert got.shape == ((2,) if example.startswith("population") else (1,)) and ((got >= 1.0) & (got <= 5.0)).all()
        if example.startswith("population"):
            assert len(h["eval_return"]) == 2
