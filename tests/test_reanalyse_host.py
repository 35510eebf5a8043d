"""Reanalysis of the replay ring, the part that runs without a GPU: the expected-row builder of tests/reanalyse_util.py pinned to the
oracle's self-play, the search-index range run.py uses, the ABI's additions, and the sizes of the GPU file's cases."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import reanalyse_util as R
from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("selfplay_keep_states", "selfplay_states", "selfplay_reanalyse")


@pytest.mark.parametrize("name", ["pendulum", "mcc", "cartpole", "cartpole_onpolicy", "population"])
def test_expected_rows_are_the_rows_selfplay_writes(name):
    """A self-play step's row is the row of an ordinary search's results(): expected_rows at search index s from the trace's root
    states equals cpu_selfplay's rows of step s, bit for bit -- every (step, game) of the continuous cases, and every discrete
    (step, game) whose search carried no count (a reused root has visits an ordinary search does not start with)."""
    case, ref = R.CASES[name], R.reference(name)
    assert case.games == 33 and case.n_sims <= 16
    steps = ref["rows"].shape[0]
    assert steps >= 5
    kws, blobs = ([case.net_kw(k) for k in range(case.nets)], case.blobs()) if case.nets > 1 else (case.net_kw(0), case.blob(0))
    checked = 0
    for s in range(steps):
        got = R.expected_rows(kws, case.desc(), blobs, ref["states"], s, s, ref["rows"])
        fresh = ref["carry_in"][s] == 0
        if case.cont:
            assert fresh.all()
        np.testing.assert_array_equal(R.bits32(got[fresh]), R.bits32(ref["rows"][s][fresh]), err_msg=f"{name} step {s}")
        checked += int(fresh.sum())
    # (discrete: every game's first step, and the steps after an episode's end, start from a fresh root)
    assert checked >= (steps * case.games if case.cont else 2 * case.games)
    if not case.cont:
        assert (ref["carry_in"] > 0).any()   # ... and the others do carry: the condition above excludes something


def test_reanalysis_search_indices_are_searchable_and_distinct():
    """run.REANALYSE_INDEX_BASE = 2^31: an oracle search under that index runs, and draws other numbers than index 0's."""
    from alphazero_gym_amd import run
    assert run.REANALYSE_INDEX_BASE == R.NEW_INDEX == 1 << 31
    case, ref = R.CASES["pendulum"], R.reference("pendulum")
    a = R.oracle_search(case.net_kw(0), case.desc(), case.blob(0), ref["states"][0], 0)
    b = R.oracle_search(case.net_kw(0), case.desc(), case.blob(0), ref["states"][0], run.REANALYSE_INDEX_BASE)
    assert (b["counts"].sum(1) == case.n_sims).all()
    assert not np.array_equal(a["actions"], b["actions"])


def test_abi_additions_are_optional_symbols(tmp_path):
    for s in NEW_SYMBOLS:
        assert s in _capi.OPTIONAL_SYMBOLS and s not in _capi.SYMBOLS
        assert s not in O.fns()   # (the CPU oracle has no reanalysis: the expected row is an ordinary search's)
    src = tmp_path / "use.c"
    src.write_text('#include "azgym_reanalyse.h"\n'
                   "int use(azg_engine* e, const int32_t* slots, double* states) {\n"
                   "    return azg_selfplay_keep_states(e, 1) + azg_selfplay_states(e, states, 4) + azg_selfplay_reanalyse(e, slots, 0, 1u << 31);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert _capi.ABI_VERSION == 1


def test_an_engine_without_the_symbols_says_so():
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.5, gamma=1.0, num_actions=2)
    e.set_weights(_capi.make_desc(4, [64], 2, "relu"), O.make_weights(1, 4, [64], 2))
    e.selfplay_begin(5)
    for call in (e.selfplay_keep_states, e.selfplay_states, e.selfplay_reanalyse):
        with pytest.raises(NotImplementedError):
            call()
    e.close()


def test_gpu_cases_stay_small():
    import test_reanalyse as T
    assert set(T.ALL) == set(R.CASES)
    for name, case in R.CASES.items():
        assert case.n_sims <= 32 and case.games <= 96, name
    assert max(R.STEPS + 1, T.STEPS_A, T.STEPS_C, T.STEPS_D) <= 6


@pytest.mark.parametrize("example", ["selfplay_train", "population_selfplay_train"])
def test_examples_refuse_reanalysis_where_no_row_stays_in_the_ring(example, capsys):
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    mod = importlib.import_module(example)
    assert mod.parse_args(["--device", "cpu"]).reanalyse_slots == 0
    for argv in (["--reanalyse-slots", "2", "--device", "cuda"],                                   # the ring is cleared every iteration
                 ["--reanalyse-slots", "2", "--replay-steps", "40", "--device", "cpu"],          # no device ring to train from
                 ["--replay-steps", "5", "--steps-per-iter", "20", "--device", "cuda"]):         # shorter than one iteration
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
        assert "--re" in capsys.readouterr().err
    a = mod.parse_args(["--reanalyse-slots", "2", "--replay-steps", "40", "--device", "cuda"])
    assert (a.reanalyse_slots, a.replay_steps) == (2, 40)
    if example == "population_selfplay_train":
        assert mod.parse_args(["--reanalyse-slots", "2", "--trainer", "device-epoch", "--device", "cuda"]).reanalyse_slots == 2
