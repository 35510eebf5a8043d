"""CPU: the self-play edge cases (tests/selfplay_edges.py) contain what their names say, the oracle's azo_selfplay_step equals the numpy
restatement (tests/selfplay_ref.py) on every one of them, every deliberately wrong variant of the rule is caught by a named case, and
the GPU file runs every case and every group in every form.  The device comparison is tests/test_selfplay_edges.py (-m gpu)."""
import ast
import os

import numpy as np
import pytest

import oracle_lib as O
import selfplay_edges as SE
import selfplay_ref as SR


_oracle = {}


def oracle_run(name):
    """The oracle's selfplay_begin / selfplay_step run of a case at the narrow shape: computed once, shared, read-only."""
    if name not in _oracle:
        out = SE.run_engine(O.OracleEngine, SE.CASES[name])
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle[name] = out
    return _oracle[name]


def test_sizes():
    for name, case in SE.CASES.items():
        assert case.steps <= 6, name
        assert case.n_sims <= 16 or name == "temperature_table_ends_2048", name
        want = 16 if name == "temperature_table_ends_2048" else 65 if name.startswith("many_children_") else 33
        assert case.n_games == want, name
    assert SE.CASES["temperature_table_ends_2048"].n_sims == 2048


@pytest.mark.parametrize("name", sorted(SE.CASES))
def test_case_contains_what_its_name_says(name):
    case = SE.CASES[name]
    out, trace = SE.traced(name)
    assert len(trace) == case.steps * case.n_games and out["rows"].shape[0] == case.steps * case.n_games
    assert not np.isnan(out["rows"]).any() and not np.isnan(out["fsum"]).any() and not np.isnan(out["state"]).any()
    if case.group != "nan" or name == "mixed_signs":
        assert int(out["reference_raises"]) == 0
    if name.startswith("many_children_"):
        K = (out["rows"].shape[1] - 3 - 1) // 3
        assert K == 20 and all(len(e["counts"]) > 16 for e in trace)           # selfplay_kernel's side of the switch
    case.check(case, out, trace)


@pytest.mark.parametrize("name", sorted(SE.CASES))
def test_oracle_equals_the_restatement(name):
    """azo_selfplay_begin / azo_selfplay_step against cpu_selfplay: rows by uint32 view, fsum and states by uint64 view, fcnt, the ring
    and the carried counts equal."""
    SE.assert_same_bits(oracle_run(name), SE.reference(name), name)


def _differs(a, b):
    return any(np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes() for k in ("rows", "fsum", "fcnt", "state", "carry"))


# mutant: the cases that must catch it
TEETH = {
    "count_ties_last": ("counts_all_tied_det", "top_tie_not_first", "visit_ties_first", "many_children_visit_ties_first"),
    "q_ties_last": ("q_ties_discrete",),
    "side_left": ("draw_on_a_cdf_value",),
    "no_power": ("temperature_0.5_mountaincar", "temperature_3_mountaincar", "temperature_60_mountaincar"),
    "no_abs": ("mixed_signs",),
    "carry_kept_over_end": ("max_len_1",),
    "carry_from_edge_count": ("carry_kept_and_dropped",),
    "done_and_length_twice": ("done_and_length",),
    "nan_sampled_first": ("qmax_zero_sampled", "qmax_zero_acrobot"),
    "eps_le": ("agent_eps_on_the_draw",),
}


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """Each wrong variant of the rule differs from the oracle on the cases named for it (and the right rule does not:
    test_oracle_equals_the_restatement)."""
    assert set(TEETH) == set(SR.MUTANTS)
    caught = [name for name in TEETH[mutant] if _differs(SE.run_cpu(SE.CASES[name], mutant=mutant), oracle_run(name))]
    print(f"{mutant}: caught by {caught}")
    assert caught == list(TEETH[mutant]), (mutant, caught)


def _gpu_file_forms():
    """The FORMS keys tests/test_selfplay_edges.py runs, read from its source (importing it would need nothing more, but the file is
    marked gpu as a whole)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_selfplay_edges.py")
    tree = ast.parse(open(path).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value in SE.FORMS:
            names.add(node.value)
    return names


def test_coverage():
    """Every case runs on the device, every form the GPU file runs is one of FORMS and the other way round, and every form that can
    takes at least one case of each group -- the seven named cases among them."""
    assert _gpu_file_forms() == set(SE.FORMS)
    ran = {n for _, _, names in SE.FORMS.values() for n in names}
    assert ran == set(SE.CASES) == set(SE.FORMS["lds"][2])
    for form in SE.EVERY_GROUP:
        names = SE.FORMS[form][2]
        assert {SE.CASES[n].group for n in names} == set(SE.GROUPS), form
        for stem in SE.ALWAYS:
            assert any(n.startswith(stem) for n in names), (form, stem)
    assert {SE.CASES[n].group for n in SE.ACROBOT} == set(SE.GROUPS) - {"continuous"}       # (Acrobot is a discrete game)
    assert all(SE.CASES[n].game == "acrobot" for n in SE.ACROBOT)
    assert len(set(SE.POPULATION)) == 3 and len({n for n, _ in SE.NET_SEARCH}) == 3
    for names in (SE.POPULATION, tuple(n for n, _ in SE.NET_SEARCH)):
        cs = [SE.CASES[n] for n in names]
        assert len({(c.game, c.n_sims, c.steps, tuple(sorted(c.begin.items()))) for c in cs}) == 1      # one engine can play them
    assert len({c_uct for _, c_uct in SE.NET_SEARCH}) == 3
    for n, c_uct in SE.NET_SEARCH:
        assert SE.CASES[n].kw()["c_uct"] == c_uct
