"""CPU: population-based training's host pieces (alphazero_gym_amd.pbt) -- truncation selection and perturbation on fixed inputs with
their draws reproduced by hand, their refusals, the argument check both ``copy_nets`` share, and the example's --pbt-* flags."""
import os
import sys

import numpy as np
import pytest

from alphazero_gym_amd import pbt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _untouched(rng, twin):
    """The generator's next output is its untouched twin's: it has made no draw."""
    return rng.bit_generator.state == twin.bit_generator.state and rng.integers(1 << 30) == twin.integers(1 << 30)


# ---------------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_select_on_fixed_scores(seed):
    """K = 8, a quarter: the top is nets {5, 7} (9 and 6), the bottom nets {1, 3} (the tie at 1 stays in index order); their sources
    are two integers(2) draws, net 1's first."""
    src = pbt.select([3, 1, 4, 1, 5, 9, 2, 6], 0.25, np.random.default_rng(seed))
    twin = np.random.default_rng(seed)
    top = [5, 7]
    want = np.arange(8)
    want[1] = top[twin.integers(2)]
    want[3] = top[twin.integers(2)]
    assert src.dtype == np.int64 and src.tolist() == want.tolist()


def test_select_draws_once_per_replaced_net():
    rng, twin = np.random.default_rng(5), np.random.default_rng(5)
    pbt.select([3, 1, 4, 1, 5, 9, 2, 6], 0.25, rng)
    twin.integers(2), twin.integers(2)
    assert _untouched(rng, twin)


def test_select_with_equal_scores_ranks_by_index():
    """All equal, K = 4, a half: the stable sort keeps the index order, so the top is {0, 1} and the bottom {2, 3}."""
    for seed in range(8):
        src = pbt.select(np.zeros(4), 0.5, np.random.default_rng(seed))
        twin = np.random.default_rng(seed)
        assert src.tolist() == [0, 1, int(twin.integers(2)), int(twin.integers(2))]


@pytest.mark.parametrize("scores,fraction", [([2.0], 0.5), ([4.0, 3.0, 2.0, 1.0], 0.2)])
def test_select_that_replaces_nobody_is_the_identity_and_draws_nothing(scores, fraction):
    rng, twin = np.random.default_rng(11), np.random.default_rng(11)
    assert pbt.select(scores, fraction, rng).tolist() == list(range(len(scores)))
    assert _untouched(rng, twin)


def test_select_never_replaces_a_source():
    cases = np.random.default_rng(2024)
    for _ in range(200):
        K = int(cases.integers(2, 65))
        fraction = float(cases.uniform(0.01, 0.5))
        scores = np.round(cases.normal(size=K), 1)   # (rounded: ties occur)
        src = pbt.select(scores, fraction, np.random.default_rng(int(cases.integers(1 << 30))))
        assert np.array_equal(src[src], src)
        assert int((src != np.arange(K)).sum()) == int(np.floor(K * fraction))
        assert pbt.check_src(src, K).tolist() == src.tolist()


@pytest.mark.parametrize("scores,fraction", [([1.0, np.nan, 2.0, 3.0], 0.25), ([1.0, np.inf, 2.0, 3.0], 0.25), ([1.0, 2.0, 3.0, 4.0], 0.0),
                                             ([1.0, 2.0, 3.0, 4.0], 0.6), ([1.0, 2.0, 3.0, 4.0], -0.25), ([1.0, 2.0, 3.0, 4.0], np.nan),
                                             ([[1.0, 2.0], [3.0, 4.0]], 0.5)])
def test_select_refusals_draw_nothing(scores, fraction):
    rng, twin = np.random.default_rng(3), np.random.default_rng(3)
    with pytest.raises(ValueError):
        pbt.select(scores, fraction, rng)
    assert _untouched(rng, twin)


# ---------------------------------------------------------------------------------------------------------------- perturb
def test_perturb_draws_one_factor_and_clips():
    spec = {"factors": [0.5, 2.0, 10.0], "min": 0.25, "max": 3.0}
    for seed in range(12):
        rng, twin = np.random.default_rng(seed), np.random.default_rng(seed)
        got = pbt.perturb(1.0, spec, rng)
        want = min(max(1.0 * spec["factors"][twin.integers(3)], 0.25), 3.0)
        assert isinstance(got, float) and got == want
        assert _untouched(rng, twin)
    rng = np.random.default_rng(0)
    assert pbt.perturb(1.0, {"factors": [100.0], "min": 0.0, "max": 3.0}, rng) == 3.0     # the clip at the top
    assert pbt.perturb(1.0, {"factors": [0.001], "min": 0.25, "max": 3.0}, rng) == 0.25   # and at the bottom
    assert pbt.perturb(0.3, {"factors": [0.1], "min": 0.0, "max": 1.0}, rng) == 0.3 * 0.1   # Python float64 arithmetic


def test_perturb_integer_rule():
    rng = np.random.default_rng(0)
    one = {"factors": [1.0], "min": 1, "max": 10, "integer": True}
    assert pbt.perturb(2.5, one, rng) == 3 and isinstance(pbt.perturb(2.5, one, rng), int)   # floor(x + 0.5): halves go up
    assert pbt.perturb(3.5, one, rng) == 4
    assert pbt.perturb(2.4, one, rng) == 2
    assert pbt.perturb(0.4, one, rng) == 1      # rounds to 0, clipped to min again
    assert pbt.perturb(8, dict(one, factors=[1.25]), rng) == 10
    assert pbt.perturb(9, dict(one, factors=[1.25]), rng) == 10   # 11.25 clipped to max


@pytest.mark.parametrize("spec", [{"factors": [], "min": 0, "max": 1}, {"factors": [1.0, 0.0], "min": 0, "max": 1},
                                  {"factors": [-1.0], "min": 0, "max": 1}, {"factors": [1.0], "min": 2, "max": 1},
                                  {"factors": [1.0], "max": 1}, {"factors": [np.nan], "min": 0, "max": 1}])
def test_perturb_refusals_draw_nothing(spec):
    rng, twin = np.random.default_rng(3), np.random.default_rng(3)
    with pytest.raises(ValueError):
        pbt.perturb(1.0, spec, rng)
    assert _untouched(rng, twin)


# ---------------------------------------------------------------------------------------------------------------- copy_nets' src
def test_check_src():
    assert pbt.check_src([0, 1, 0, 1], 4).tolist() == [0, 1, 0, 1]
    assert pbt.check_src(np.array([2, 1, 2], np.int32), 3).dtype == np.int64
    assert pbt.check_src([0.0, 0.0], 2).tolist() == [0, 0]
    for bad, K, why in [([0, 1, 4, 1], 4, "outside"), ([0, -1, 0, 1], 4, "outside"), ([0, 1, 0], 4, "one entry per net"),
                        ([[0, 1], [0, 1]], 2, "one entry per net"), ([1, 2, 2], 3, "itself replaced"), ([0.5, 1.0], 2, "integers"),
                        (["a", "b"], 2, "integers")]:
        with pytest.raises(ValueError, match=why):
            pbt.check_src(bad, K)


def test_the_module_imports_without_torch():
    import subprocess
    code = "import sys; import alphazero_gym_amd.pbt; assert 'torch' not in sys.modules, 'pbt pulled torch in'"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# ---------------------------------------------------------------------------------------------------------------- the example's flags
# the parser's fields before the --pbt-* flags
PARENT_FIELDS = {"game", "seeds", "games_per_seed", "n_rollouts", "iters", "steps_per_iter", "train_rows", "batch_size", "hidden",
                 "max_episode_length", "lr", "lrs", "c_ucts", "gammas", "search_epsilons", "c_pws", "kappas", "n_rollouts_per_seed",
                 "optimizer", "grad_clip", "layernorm", "wide", "engine_seed", "device", "trainer", "eval_episodes", "eval_rule",
                 "eval_search_episodes", "replay_steps", "reanalyse_slots", "n_step", "n_steps", "td_lambda", "td_lambdas",
                 "prioritized_alpha", "prioritized_eps", "prioritized_beta", "prioritized_feedback", "prioritized_online"}
PBT_OFF = {"pbt_every": 0, "pbt_fraction": 0.25, "pbt_explore": None, "pbt_score": "selfplay"}
BASE = ["--seeds", "1", "2", "3", "4", "--trainer", "device-epoch", "--device", "cpu"]


def test_parser_without_pbt_is_the_parser_as_it_was():
    import population_selfplay_train as P
    a = P.parse_args(["--device", "cpu"])
    fields = vars(a)
    assert PARENT_FIELDS <= set(fields)
    assert {k: v for k, v in fields.items() if k.startswith("pbt_")} == PBT_OFF
    assert P.pbt_names(a) == [] and P.search_kwargs(a) == {} and P.pbt_target_rule(a) == P.target_rule(a)
    b = P.parse_args(BASE + ["--n-step", "3"])
    assert P.pbt_target_rule(b) == {"n_step": 3, "td_lambda": None}


def test_parser_reads_explore_specs():
    import population_selfplay_train as P
    a = P.parse_args(BASE + ["--n-rollouts", "16", "--n-step", "3", "--td-lambda", "0.9", "--pbt-every", "2", "--pbt-fraction", "0.5",
                             "--pbt-explore", "lr", "c_uct:0.5,2", "n_rollouts:0.5,2:2:8", "n_step", "td_lambda", "target_gamma"])
    assert P.pbt_explore(a) == {"lr": {"factors": [0.8, 1.25], "min": 1e-6, "max": 1.0},
                                "c_uct": {"factors": [0.5, 2.0], "min": 0.0, "max": 100.0},
                                "n_rollouts": {"factors": [0.5, 2.0], "min": 2.0, "max": 8.0, "integer": True},
                                "n_step": {"factors": [0.8, 1.25], "min": 0, "max": 20, "integer": True},
                                "td_lambda": {"factors": [0.8, 1.25], "min": 0.0, "max": 1.0},
                                "target_gamma": {"factors": [0.8, 1.25], "min": 0.0, "max": 1.0}}
    assert list(P.pbt_explore(a)) == ["lr", "c_uct", "n_rollouts", "n_step", "td_lambda", "target_gamma"]
    # search names and budgets give the engine its tables from iteration 0, filled with the shared values
    assert P.search_kwargs(a) == {"net_settings": [{}, {}, {}, {}], "net_rollouts": [16, 16, 16, 16]}
    assert P.pbt_target_rule(a) == {"n_step": [3] * 4, "td_lambda": [0.9] * 4, "target_gamma": [None] * 4}
    for spec in P.pbt_explore(a).values():
        pbt.check_spec("spec", spec)


@pytest.mark.parametrize("argv,why", [
    (BASE + ["--pbt-every", "-1"], "--pbt-every must be >= 0"),
    (BASE + ["--pbt-explore", "lr"], "it needs --pbt-every N"),
    (["--seeds", "1", "2", "--device", "cpu", "--pbt-every", "2"], "use --trainer device, device-fused or device-epoch"),
    (["--seeds", "1", "--trainer", "device", "--device", "cpu", "--pbt-every", "2"], "two --seeds entries or more"),
    (BASE + ["--pbt-every", "2", "--pbt-fraction", "0"], "--pbt-fraction must lie in (0, 0.5]"),
    (BASE + ["--pbt-every", "2", "--pbt-fraction", "0.6"], "--pbt-fraction must lie in (0, 0.5]"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "momentum"], "is not a hyper-parameter it can perturb"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr", "lr:0.5,2"], "names 'lr' twice"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr:0.5,2:1e-5"], "the forms are NAME"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr:0.5,x"], "the factors are positive numbers"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr:0.5,-2"], "the factors are positive numbers"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr:0.5,2:1:0.1"], "0 <= min <= max"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "lr:0.5,2:a:b"], "0 <= min <= max"),
    (["--seeds", "1", "2", "--trainer", "device", "--device", "cpu", "--pbt-every", "2", "--pbt-explore", "tau"],
     "use --trainer device-fused or"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "n_step"], "it needs --n-step N or --n-steps"),
    (BASE + ["--pbt-every", "2", "--pbt-explore", "target_gamma"], "it needs --n-step N or --n-steps"),
    (BASE + ["--pbt-every", "2", "--n-step", "3", "--pbt-explore", "td_lambda"], "it needs --td-lambda L or --td-lambdas"),
    (BASE + ["--pbt-every", "2", "--pbt-score", "eval"], "it needs --eval-episodes N"),
    (BASE + ["--pbt-every", "2", "--pbt-score", "eval-search"], "it needs --eval-search-episodes E"),
])
def test_parser_refusals(argv, why, capsys):
    import population_selfplay_train as P
    with pytest.raises(SystemExit):
        P.parse_args(argv)
    assert why in capsys.readouterr().err.replace("\n", " ")
