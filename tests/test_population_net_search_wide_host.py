"""CPU: per-net search settings at padded widths >= 512 (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE) -- that the GPU matrix
(test_population_net_search_wide.py) cannot pass by accident, the Python layer against a CPU double of the engine, and the binding."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import net_search_util as N
import net_search_wide_util as NW
import oracle_lib as O
import test_population_net_search_host as H
import test_population_wide as W
from alphazero_gym_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------- the matrix cannot pass by accident

# every row at the number of trees per net the GPU matrix gives it, and the one-launch rows at 32 as well (one net with a table)
ROW_T = [(row, NW.trees_per_net(row)) for row in NW.matrix_rows()] + [(row, 32) for row in NW.matrix_rows() if isinstance(row, int) and not NW.lockstep_shaped(row)]


def test_the_rows_are_the_wide_rows():
    rows = NW.matrix_rows()
    assert rows[:-1] == [18, 19, 20, 21, 29, 34, 40] and rows[-1] is W.PENDULUM_2x512_LN
    assert [NW.trees_per_net(r) for r in rows] == [32, 32, 32, 19, 32, 32, 19, 19]
    by = {}
    for row, v in NW.cases():
        by.setdefault(NW.row_id(row), []).append(v)
    for row in rows:
        assert by[NW.row_id(row)] == (W.VARIANTS if NW.lockstep_shaped(row) else ["default", "global_tree"]), (row, by)


@pytest.mark.parametrize("row,T", ROW_T, ids=[f"{NW.row_id(r)}-T{t}" for r, t in ROW_T])
def test_the_settings_of_nets_1_and_2_change_their_trees(row, T):
    """On the oracle alone: nets 1 and 2 (their own weights, roots and tree ids) under their own settings differ from the same nets
    under net 0's settings in at least T // 2 of their trees, in edge_n or edge_Q; net 0 in none.  An engine that ignored its table, or
    read another net's record, would therefore fail the matrix on this row."""
    cfg = NW.cfg_of(row)
    st = NW.net_settings(row)
    kw, desc, blobs, roots, carry = W._inputs(cfg, T)
    assert len({tuple(sorted(s.items())) for s in st}) == 3 and st[0] == N.shared_settings(cfg)
    if cfg[1] == 1:   # net 1's widening fits the engine the row's own pair creates
        ks = [N.kmax_of(s, kw["n_sims"]) for s in st]
        assert ks[1] < ks[0] == ks[2], ks
    own = NW.oracle(row, T)
    shared = W._oracle(kw, desc, blobs, roots, carry, W.SIDX)
    for key in own[1]:
        np.testing.assert_array_equal(own[1][key][:T], shared[1][key][:T], err_msg=f"net 0 {key}")   # (its settings ARE the row's)
    changed = []
    for k in (1, 2):
        changed.append(sum(own[1]["edge_n"][i].tobytes() != shared[1]["edge_n"][i].tobytes() or
                           own[1]["edge_Q"][i].tobytes() != shared[1]["edge_Q"][i].tobytes() for i in range(k * T, (k + 1) * T)))
    print(f"{NW.row_id(row)} T={T}: changed trees of nets 1 / 2: {changed[0]} / {changed[1]}")
    assert min(changed) >= T // 2, f"{NW.row_id(row)}: the settings change only {changed} of the nets' {T} trees"


def test_net_1_leaves_result_columns_empty():
    """Kmax 3 against 6 on 2x512 (30 simulations), 2 against 4 on 4x1024 (12): the matrix covers the empty result columns."""
    for row, want in ((18, (6, 3)), (20, (4, 2))):
        st, n_sims = NW.net_settings(row), NW.cfg_of(row)[4]
        assert (N.kmax_of(st[0], n_sims), N.kmax_of(st[1], n_sims)) == want


# ------------------------------------------------------------------------------------------------------------------ Python layer


class OracleNetSearchWide(H.OracleNetSearch):
    """OracleNetSearch whose set_net_search takes ``wide=`` and records it."""

    wide_calls = []

    def set_net_search(self, entries, wide=False):
        type(self).wide_calls.append(bool(wide))
        super().set_net_search(entries)


def test_population_mcts_wide_opt_in(monkeypatch):
    from alphazero_gym_amd import _native
    from alphazero_gym_amd.search.mcts import PopulationMCTS
    monkeypatch.setattr(_native, "HipEngine", OracleNetSearchWide)
    H.OracleNetSearch.tables, OracleNetSearchWide.wide_calls = [], []
    kw = dict(env_id=0, mode=0, n_rollouts=4, c_uct=1.5, gamma=1.0, epsilon=0.1, num_actions=2)
    wide = H._policies(3, [512, 512])
    with pytest.raises(ValueError, match="at most 256"):                      # without the opt-in the refusal stands
        PopulationMCTS(wide, trees_per_model=32, net_settings=[{}] * 3, **kw)
    with pytest.raises(ValueError, match="at most 256"):
        PopulationMCTS(wide, trees_per_model=32, net_settings=[{}] * 3, net_settings_wide=False, **kw)
    with pytest.raises(ValueError, match="multiple of 32"):                  # lock-step shaped: whole teams per model
        PopulationMCTS(wide, trees_per_model=16, net_settings=[{}] * 3, net_settings_wide=True, **kw)
    assert H.OracleNetSearch.tables == [] and OracleNetSearchWide.wide_calls == []
    st = [{}, {"c_uct": 6.0}, {"gamma": 0.9, "epsilon": 0.0}]
    pop = PopulationMCTS(wide, trees_per_model=32, net_settings=st, net_settings_wide=True, **kw)
    assert OracleNetSearchWide.wide_calls == [True] and pop.net_settings_wide
    assert [s["c_uct"] for s in H.OracleNetSearch.tables[-1]] == [1.5, 6.0, 1.5] and pop.net_settings == H.OracleNetSearch.tables[-1]
    pop.set_net_settings([{"c_uct": 3.0}, {}, {}])                            # wide=None: what the constructor was given
    assert OracleNetSearchWide.wide_calls == [True, True] and H.OracleNetSearch.tables[-1][0]["c_uct"] == 3.0
    with pytest.raises(ValueError, match="at most 256"):
        pop.set_net_settings([{}] * 3, wide=False)
    pop.set_net_settings(None)
    assert H.OracleNetSearch.tables[-1] is None and pop.net_settings is None
    pop.close()
    # one hidden layer of 512 is not lock-step shaped: any number of trees per model
    pop = PopulationMCTS(H._policies(3, [512]), trees_per_model=5, net_settings=st, net_settings_wide=True, **kw)
    assert OracleNetSearchWide.wide_calls[-1] is True
    pop.close()
    # narrow nets: the flag permits and changes nothing else; without it the plain call, as before
    pop = PopulationMCTS(H._policies(3, [16, 16]), trees_per_model=2, net_settings=st, net_settings_wide=True, **kw)
    assert OracleNetSearchWide.wide_calls[-1] is True
    pop.set_net_settings(st, wide=False)
    assert OracleNetSearchWide.wide_calls[-1] is False
    pop.close()


def test_selfplay_forwards_the_keyword_only_when_given(monkeypatch):
    from alphazero_gym_amd import run
    seen = {}

    class Stop(Exception):
        pass

    def search(policies, games_per_net, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(run.PopulationSelfPlay, "_search", staticmethod(search))
    st = [{"c_uct": 1.0}, {"c_uct": 2.0}]
    args = dict(game="CartPole-v0", games_per_net=32, n_rollouts=5, c_uct=1.5)
    with pytest.raises(Stop):
        run.PopulationSelfPlay(H._policies(2, [512, 512]), net_settings=st, net_settings_wide=True, **args)
    assert seen["net_settings"] == st and seen["net_settings_wide"] is True
    seen.clear()
    with pytest.raises(Stop):
        run.PopulationSelfPlay(H._policies(2, [16, 16]), net_settings=st, **args)
    assert seen["net_settings"] == st and "net_settings_wide" not in seen   # today's call as it was
    seen.clear()
    with pytest.raises(Stop):
        run.PopulationSelfPlay(H._policies(2, [16, 16]), **args)
    assert "net_settings" not in seen and "net_settings_wide" not in seen


def test_agent_population_wide_search(monkeypatch):
    """AgentPopulation(per_agent_search=True, wide_search=True) builds its PopulationMCTS with the opt-in; without it, without."""
    import test_population as TP
    from alphazero_gym_amd.agent import population
    agents, _ = TP._agents("discrete")
    agents[1].mcts.c_uct = 2.0
    with pytest.raises(ValueError, match="per_agent_search=True"):
        population.AgentPopulation(agents, wide_search=True)
    seen = []

    class Stop(Exception):
        pass

    def fake(models, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(population, "PopulationMCTS", fake)
    for wide in (True, False):
        pop = population.AgentPopulation(agents, per_agent_search=True, wide_search=wide)
        with pytest.raises(Stop):
            pop._engine(0)
    assert seen[0]["net_settings_wide"] is True and seen[0]["net_settings"][1]["c_uct"] == 2.0
    assert "net_settings_wide" not in seen[1] and seen[1]["net_settings"][1]["c_uct"] == 2.0


def test_example_wide_sweep_builds_the_opt_in_call():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import population_selfplay_train as X
    wide = ["--wide", "--seeds", "3", "11", "--hidden", "512", "512", "--games-per-seed", "32"]
    kw = X.search_kwargs(X.parse_args(wide + ["--c-ucts", "1", "2"]))
    assert kw == dict(net_settings=[dict(c_uct=1.0), dict(c_uct=2.0)], net_settings_wide=True)
    for flag in ("--gammas", "--search-epsilons"):
        assert X.search_kwargs(X.parse_args(wide + [flag, "0.5", "0.25"]))["net_settings_wide"] is True
    for flag in ("--c-pws", "--kappas"):
        assert X.search_kwargs(X.parse_args(wide + ["--game", "Pendulum-v0", flag, "0.5", "0.25"]))["net_settings_wide"] is True
    assert X.search_kwargs(X.parse_args(wide)) == {}                                      # no sweep: no keyword
    assert X.search_kwargs(X.parse_args(["--seeds", "0", "1", "--c-ucts", "1", "2"])) == dict(net_settings=[dict(c_uct=1.0), dict(c_uct=2.0)])


# --------------------------------------------------------------------------------------------------------------------------- ABI


def test_binding():
    """set_net_search_ex is optional for a library (the oracle has none): the clear error, not an AttributeError."""
    assert "set_net_search_ex" in _capi.OPTIONAL_SYMBOLS and "set_net_search_ex" not in O.fns()
    e = O.OracleEngine(env_id=0, mode=0, n_trees=2, n_sims=4, c_uct=1.0, gamma=1.0, num_actions=2)
    with pytest.raises(NotImplementedError, match="no set_net_search_ex entry point"):
        e.set_net_search([dict(c_uct=1.0, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)] * 2, wide=True)
    with pytest.raises(NotImplementedError, match="no set_net_search entry point"):
        e.set_net_search([dict(c_uct=1.0, gamma=1.0, epsilon=0.0, c_pw=1.0, kappa=0.5)] * 2)
    e.close()
    so = os.path.join(ROOT, "alphazero_gym_amd", "csrc", "libazgym_hip.so")
    if os.path.exists(so):   # (loads without a GPU)
        from alphazero_gym_amd import _native
        f = _native.fns()
        assert list(f["set_net_search_ex"].argtypes) == [C.c_void_p, C.POINTER(_capi.AzgNetSearch), C.c_int32, C.c_uint32]


def test_prototype_and_flag_match_the_header(tmp_path):
    """The header's prototype takes (engine, const azg_net_search*, int32_t, uint32_t) -- a function pointer of exactly that type is
    assigned under -Werror -- its flag has the binding's value, and the argument types have the ctypes sizes."""
    src = tmp_path / "proto.c"
    src.write_text('#include <stdio.h>\n#include <stdint.h>\n#include "azgym_population.h"\n'
                   'int main(void) { int (*fn)(azg_engine*, const azg_net_search*, int32_t, uint32_t) = azg_set_net_search_ex; (void)fn;\n'
                   ' printf("%u %zu %zu %zu", (unsigned)AZG_NET_SEARCH_WIDE, sizeof(int32_t), sizeof(uint32_t), sizeof(azg_net_search)); return 0; }\n')
    obj = tmp_path / "proto.o"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])
    # (compiled only: the entry point lives in the HIP library; the constants are read from a program that does not call it)
    vals = tmp_path / "vals.c"
    vals.write_text('#include <stdio.h>\n#include <stdint.h>\n#include "azgym_population.h"\n'
                    'int main(void) { printf("%u %zu %zu %zu", (unsigned)AZG_NET_SEARCH_WIDE, sizeof(int32_t), sizeof(uint32_t), sizeof(azg_net_search)); return 0; }\n')
    exe = tmp_path / "vals"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(vals), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [_capi.NET_SEARCH_WIDE, C.sizeof(C.c_int32), C.sizeof(C.c_uint32), C.sizeof(_capi.AzgNetSearch)]
