"""GPU (-m gpu): the device self-play step at the edges of the agents' final-action rule, every kernel form against the numpy
restatement (tests/selfplay_ref.py), by bit pattern.

The cases are tests/selfplay_edges.py's hand-built nets and hand-placed roots; what each contains, that the CPU oracle plays them as
the restatement does, and that every wrong variant of the rule is caught by one of them is asserted on the CPU in
tests/test_selfplay_edges_host.py.  Here every case runs on the register-resident LDS-tree kernel (2x64), and selfplay_edges.SUBSET
-- at least one case of each group -- in the other forms:

  lds           (64, 64):   search_kernel with its trees in LDS; return_results from the kernel's epilogue, then selfplay_kernel16
                            (many_children_*: trees in global memory, selfplay_kernel)
  global_tree   (64, 64), AZG_FORCE_GLOBAL_TREE=1
  w256          (256, 256): the 8-wave shapes (continuous mode; the discrete cases run the family's 4-wave kernel of that width)
  wide_team     (512, 512): the team kernel (or a counted fall-back), results_kernel, then selfplay_kernel16
  wide_layers   (512, 512), AZG_LS_TEAM=0: the per-layer launches
  wide_acrobot  (512, 512): Acrobot's six inputs take the one-launch kernel
  population    three CartPole nets, each a different edge case, in one engine (azg_population_selfplay_begin)
  net_search    three MountainCar nets with their own c_uct (azg_set_net_search: search_kernel_nets)

Rows as uint32, fsum and the env states as uint64, fcnt, the ring and the carried counts exact (selfplay_edges.assert_same_bits).  No
tolerance anywhere."""
import time

import pytest

import selfplay_edges as SE
import selfplay_ref as SR
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

FORM_ENV = {"global_tree": ("AZG_FORCE_GLOBAL_TREE", "1"), "wide_layers": ("AZG_LS_TEAM", "0")}
SWITCHES = ("AZG_FORCE_GLOBAL_TREE", "AZG_LS_TEAM", "AZG_FORCE_PERSISTENT", "AZG_TEAM_SPIN_LIMIT", "AZG_WAVES", "AZG_NO_SPEC", "AZG_TILE_TREES")


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_selfplay_edges.py: {time.perf_counter() - t0:.1f} s wall time")


@pytest.fixture(scope="module")
def hip():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def _set_form(monkeypatch, form):
    """The engine reads its switches when it is created."""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if form in FORM_ENV:
        monkeypatch.setenv(*FORM_ENV[form])


def _assert_form(form, case, info):
    what = (form, case.name, info)
    if form in ("lds", "population", "net_search"):
        assert info["kernel_form"] == "persistent", what
        if case.name.startswith("many_children_"):
            assert info["max_children"] == 20 and (info["tree_storage"], info["lds_exit"]) == ("global", "children"), what
        elif case.n_sims > 509:
            assert (info["tree_storage"], info["lds_exit"]) == ("global", "records"), what
        else:
            assert info["tree_storage"] in ("lds8", "lds9") and info["lds_exit"] == "resident", what
        assert " 64," in info["kernel_name"], what
        assert info["kernel_name"].startswith("search_kernel_nets<" if form == "net_search" else "search_kernel<"), what
    elif form == "global_tree":
        assert info["kernel_form"] == "persistent" and (info["tree_storage"], info["lds_exit"]) == ("global", "forced"), what
    elif form == "w256":
        # (the discrete family has no 8-wave shape: dispatch.cuh)
        assert info["kernel_form"] == "persistent" and " 256," in info["kernel_name"] and info["waves"] == (8 if case.cont else 4), what
    elif form == "wide_team":
        assert info["kernel_form"] == "team" or (info["kernel_form"] == "per_layer" and info["team_fallbacks"] >= 1), what
    elif form == "wide_layers":
        assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, what
    elif form == "wide_acrobot":
        assert info["kernel_form"] == "persistent" and " 512, 0," in info["kernel_name"], what
    else:
        raise AssertionError(form)


def _form_cases():
    return [(form, name) for form in ("lds", "global_tree", "w256", "wide_team", "wide_layers", "wide_acrobot") for name in SE.FORMS[form][2]]


@pytest.mark.parametrize("form,name", _form_cases())
def test_edge_case_equals_the_restatement(hip, form, name, monkeypatch):
    case = SE.CASES[name]
    hidden, n = SE.FORMS[form][0], SE.form_games(form, case)
    want = SE.reference(name, hidden, n)
    _set_form(monkeypatch, form)
    got = SE.run_engine(hip, case, hidden, n)
    print(f"{form} {name}: {got['info']['kernel_name']} waves {got['info']['waves']} trees {got['info']['tree_storage']}")
    _assert_form(form, case, got["info"])
    SE.assert_same_bits(got, want, f"{name} {form}")


def _population(hip, names, T, net_search=None):
    """K nets of one game in one engine, net k playing case names[k] as games BASE + k T ..: (the engine's run, the K restatements)."""
    cases = [SE.CASES[n] for n in names]
    c0 = cases[0]
    refs = [SE.reference(n, SE.NARROW, T, SE.BASE + k * T) for k, n in enumerate(names)]
    e = hip(**dict(c0.kw(), n_trees=len(cases) * T))
    try:
        e.set_population(len(cases))
        for k, c in enumerate(cases):
            e.set_net_weights(k, c.desc(SE.NARROW), c.blob(SE.NARROW))
        if net_search:
            e.set_net_search([dict(c_uct=c.kw()["c_uct"], gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5) for c in cases])
        got = SE.play(e, c0.steps, c0.begin, population=True)
        info = e.search_info()
    finally:
        e.close()
    return got, refs, info


def test_population_of_three_edge_cases_in_one_engine(hip, monkeypatch):
    """CartPole, one simulation, max_value sampled: a net whose largest root Q is 0 (every pi entry NaN), one whose Qs are all negative
    (ratios 1 and 1.5) and one whose unvisited edge carries the root's V, side by side in the lanes of one selfplay_kernel16 launch."""
    _set_form(monkeypatch, "population")
    got, refs, info = _population(hip, SE.FORMS["population"][2], SE.G)
    assert int(refs[0]["reference_raises"]) > 0 and int(refs[1]["reference_raises"]) == int(refs[2]["reference_raises"]) == 0
    _assert_form("population", SE.CASES[SE.POPULATION[0]], info)
    SE.assert_same_bits(got, SE.stack_nets(refs), "population of edges")


def test_three_nets_under_a_per_net_search_table(hip, monkeypatch):
    """MountainCar, 8 simulations, sampled, c_uct 1, 1e6 and 2 from azg_set_net_search: counts (3, 3, 2), (a, 0, b) with its repeated
    cdf value, and (2, 3, 3), each net against the restatement searched with ITS c_uct."""
    _set_form(monkeypatch, "net_search")
    got, refs, info = _population(hip, SE.FORMS["net_search"][2], SE.G, net_search=True)
    _assert_form("net_search", SE.CASES[SE.NET_SEARCH[0][0]], info)
    SE.assert_same_bits(got, SE.stack_nets(refs), "per-net search table")


def test_temperature_table_refuses_2049_simulations(hip):
    """The (c / m)^temperature table ends at 2048 simulations: one more with a temperature other than 1 is AZG_E_UNSUPPORTED from
    selfplay_begin, and temperature 1 (no table) is taken."""
    case = SE.CASES["temperature_table_ends_2048"]
    e = hip(**dict(case.kw(), n_sims=2049, n_trees=16))
    try:
        e.set_weights(case.desc(SE.NARROW), case.blob(SE.NARROW))
        with pytest.raises(_capi.EngineError) as err:
            e.selfplay_begin(capacity_steps=1, **case.begin)
        assert err.value.code == _capi.AZG_E_UNSUPPORTED, err.value
        e.selfplay_begin(capacity_steps=1, **dict(case.begin, temperature=1.0))
    finally:
        e.close()
    assert SR.BEGIN["temperature"] == 1.0 and case.begin["temperature"] != 1.0
