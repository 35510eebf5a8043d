"""No GPU: the host-side rules of wide populations -- the example's argument check (several nets that the engine searches as teams of
32 trees need a multiple of 32 games each, said before anything is built) and the latency tool's wide configurations."""
import os
import sys

import pytest

from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("examples", "tools"):
    sys.path.insert(0, os.path.join(ROOT, d))

WIDE = ["--wide", "--seeds", "3", "11", "--hidden", "512", "512"]


def test_lockstep_shaped_is_the_engines_rule():
    """engine_host.h: azg_lockstep_shaped -- padded width >= 512, two or more hidden layers, no LayerNorm, at most four inputs."""
    assert _capi.lockstep_shaped(3, [512, 512]) and _capi.lockstep_shaped(4, [1024] * 4) and _capi.lockstep_shaped(2, [64, 449])
    assert not _capi.lockstep_shaped(3, [448, 448])                   # pads to 448
    assert not _capi.lockstep_shaped(4, [512])                        # one hidden layer
    assert not _capi.lockstep_shaped(6, [512, 512])                   # Acrobot's six observations
    assert not _capi.lockstep_shaped(3, [512, 512], layernorm=True)


def test_example_refuses_ragged_teams_before_it_builds_anything(capsys):
    import population_selfplay_train as X
    with pytest.raises(SystemExit) as ei:
        X.parse_args(WIDE + ["--games-per-seed", "20"])
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "--games-per-seed must be a multiple of 32 (got 20)" in err and "teams of 32 trees" in err and "2 seeds" in err


@pytest.mark.parametrize("args", [WIDE + ["--games-per-seed", "32"], WIDE + ["--games-per-seed", "64"],
                                  ["--wide", "--seeds", "0", "--hidden", "512", "512", "--games-per-seed", "20"],              # one seed
                                  WIDE + ["--games-per-seed", "20", "--layernorm"],                                              # search kernel
                                  ["--wide", "--seeds", "3", "11", "--hidden", "512", "--games-per-seed", "20"],                # one layer
                                  WIDE + ["--games-per-seed", "20", "--game", "Acrobot-v1"],                                    # six inputs
                                  ["--seeds", "3", "11", "--hidden", "128", "128", "--games-per-seed", "20"]],
                         ids=["32", "64", "one_seed", "layernorm", "one_layer", "acrobot", "narrow"])
def test_example_passes_the_check(args):
    import population_selfplay_train as X
    a = X.parse_args(args)
    assert X.check_population_shape(a) is None and a.games_per_seed == int(args[args.index("--games-per-seed") + 1])


def test_latency_tool_wide_configurations_parse():
    import population_latency as L
    a = L.parse_args(["--wide"])
    assert a.wide and a.configs.split(",") == ["pendulum_4x1024_200", "cartpole_2x512_100"] and (a.steps, a.warmup) == (5, 2)
    assert L.parse_splits(a.splits) == [(1, 1024), (2, 512), (4, 256), (8, 128), (16, 64), (32, 32)]
    for name in a.configs.split(","):
        kw, (in_dim, hidden, n_dist, act) = L.WIDE_CONFIGS[name]
        assert _capi.lockstep_shaped(in_dim, hidden) and act in _capi.ACT and kw["n_sims"] in (100, 200)
        desc = _capi.make_desc(in_dim, hidden, n_dist, act)
        assert desc.n_hidden == len(hidden) and desc.in_dim == in_dim
    assert L.parse_args(["--wide", "--splits", "3x96", "--configs", "cartpole_2x512_100", "--steps", "2"]).steps == 2
    for bad in (["--wide", "--splits", "2x48"], ["--wide", "--splits", "0x32"], ["--wide", "--configs", "cartpole_2x128_8"]):
        with pytest.raises(SystemExit):
            L.parse_args(bad)
    b = L.parse_args([])                                              # the narrow tool as it was
    assert not b.wide and b.configs.split(",") == list(L.CONFIGS) and (b.steps, b.warmup) == (20, 3)
