"""Error behaviour of the C ABI (codes + messages), identical for the oracle (CPU) and the HIP engine (gpu)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from alphazero_gym_amd import _capi

BACKENDS = ["oracle", pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def engine_cls(request):
    if request.param == "oracle":
        return O.OracleEngine
    from alphazero_gym_amd import _native
    _native.lib()
    return _native.HipEngine


def test_create_rejects_bad_configs(engine_cls):
    with pytest.raises(_capi.EngineError) as ei:
        engine_cls(env_id=2, mode=0, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0, num_actions=2)      # discrete MCTS on Pendulum
    assert ei.value.code == _capi.AZG_E_UNSUPPORTED
    with pytest.raises(_capi.EngineError) as ei:
        engine_cls(env_id=0, mode=1, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0)                     # continuous MCTS on CartPole
    assert ei.value.code == _capi.AZG_E_UNSUPPORTED
    with pytest.raises(_capi.EngineError) as ei:
        engine_cls(env_id=2, mode=1, n_trees=0, n_sims=4, c_uct=1.0, gamma=1.0)
    assert ei.value.code == _capi.AZG_E_INVALID
    with pytest.raises(_capi.EngineError):
        engine_cls(env_id=7, mode=1, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0)
    for bad in (dict(c_pw=0.0), dict(c_pw=-1.0), dict(kappa=-0.5)):                                 # no node would ever be entitled to a child
        with pytest.raises(_capi.EngineError) as ei:
            engine_cls(env_id=2, mode=1, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0, **bad)
        assert ei.value.code == _capi.AZG_E_INVALID and "c_pw" in str(ei.value)
    for env_id, bad in ((0, 3), (3, 2), (3, 4)):                                                    # num_actions is the env's: CartPole 2, MountainCar 3
        with pytest.raises(_capi.EngineError) as ei:
            engine_cls(env_id=env_id, mode=0, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0, num_actions=bad)
        assert ei.value.code == _capi.AZG_E_INVALID
    with pytest.raises(_capi.EngineError) as ei:
        engine_cls(env_id=3, mode=1, n_trees=1, n_sims=4, c_uct=1.0, gamma=1.0)                     # continuous MCTS on MountainCar
    assert ei.value.code == _capi.AZG_E_UNSUPPORTED
    e = engine_cls(env_id=3, mode=0, n_trees=2, n_sims=4, c_uct=1.0, gamma=1.0, num_actions=3)
    e.set_weights(_capi.make_desc(2, [64], 3, "relu"), O.make_weights(1, 2, [64], 3))
    with pytest.raises(ValueError):
        e.search(np.array([[-0.5, 0.0], [0.55, 0.01]]))                                             # a root at the flag is terminal
    e.close()


def test_search_needs_weights_and_results_need_a_search(engine_cls):
    e = engine_cls(env_id=2, mode=1, n_trees=2, n_sims=4, c_uct=0.05, gamma=1.0)
    with pytest.raises(_capi.EngineError) as ei:
        e.search(np.zeros((2, 2)))
    assert ei.value.code == _capi.AZG_E_STATE and "set_weights" in str(ei.value)
    with pytest.raises(_capi.EngineError) as ei:
        e.results()
    assert ei.value.code == _capi.AZG_E_STATE
    with pytest.raises(_capi.EngineError):
        e.selfplay_step()
    e.close()


def test_set_weights_validates_the_descriptor(engine_cls):
    e = engine_cls(env_id=2, mode=1, n_trees=2, n_sims=4, c_uct=0.05, gamma=1.0)
    good = O.make_weights(1, 3, [64], 2)
    with pytest.raises(_capi.EngineError):
        e.set_weights(_capi.make_desc(4, [64], 2, "elu"), good)                    # wrong observation size
    with pytest.raises(_capi.EngineError):
        e.set_weights(_capi.make_desc(3, [64], 2, "elu"), good[:-1])               # blob too short
    with pytest.raises(_capi.EngineError):
        e.set_weights(_capi.make_desc(3, [64], 3, "elu"), O.make_weights(1, 3, [64], 3))   # n_dist does not match num_components
    d = _capi.make_desc(3, [64], 2, "elu")
    d.activation = 17
    with pytest.raises(_capi.EngineError):
        e.set_weights(d, good)
    e.set_weights(_capi.make_desc(3, [64], 2, "elu"), good)
    e.search(np.array([[0.1, 0.2], [0.3, -0.1]]))
    assert (e.results()["counts"].sum(1) == 4).all()
    with pytest.raises(_capi.EngineError):
        e.search(np.zeros((2, 2)), carry=np.array([-1, 0]))                          # negative carried count
    with pytest.raises(_capi.EngineError) as ei:
        e.search(np.zeros((2, 2)), carry=np.array([0, 3]))                           # a carried count in continuous mode (mcts.py:589-600: fresh root)
    assert ei.value.code == _capi.AZG_E_INVALID and "fresh root" in str(ei.value)
    e.search(np.zeros((2, 2)), carry=np.array([0, 0]))
    e.close()


@pytest.mark.gpu
def test_search_info_reports_form_and_residency_through_the_abi(capfd, monkeypatch):
    """azg_search_info (include/azgym.h), called the way a C caller would: plain struct, struct_size checked.  It names the kernel form and
    where the trees lived; a search whose trees do not fit LDS residency (600 simulations: 602 records > 511) still gives the right
    visit totals, reports AZG_TREES_GLOBAL with AZG_LDS_EXIT_RECORDS and prints ONE line to stderr for the engine, not one per search."""
    from alphazero_gym_amd import _native
    monkeypatch.delenv("AZG_QUIET", raising=False)   # (the warning this test counts is what AZG_QUIET=1 silences)
    lib = _native.lib()
    info = _native.AzgSearchInfo()
    e = _native.HipEngine(env_id=2, mode=1, n_trees=64, n_sims=40, c_uct=0.05, gamma=1.0)
    h = C.c_void_p(e._h.value)
    info.struct_size = 4
    assert lib.azg_search_info(h, C.byref(info)) == _capi.AZG_E_INVALID            # wrong struct size: refused, nothing written
    info.struct_size = C.sizeof(_native.AzgSearchInfo)
    assert lib.azg_search_info(h, C.byref(info)) == 0 and info.kernel_form == -1   # AZG_FORM_NONE before the first search
    e.set_weights(_capi.make_desc(3, [256, 256], 2, "elu"), O.make_weights(34, 3, [256, 256], 2))
    e.search(e.synthetic_roots())
    assert lib.azg_search_info(h, C.byref(info)) == 0
    assert info.kernel_form == 0 and info.tree_storage == 1 and info.lds_exit == 0 and info.spec == 1      # persistent, LDS8, resident, SPEC
    assert (info.waves, info.groups, info.tile_trees) == (8, 1, 16) and info.max_records == 42
    assert info.kernel_name.decode() == "search_kernel<2, 256, 1, 1, false, 8, 1, 16, 1>" and info.last_ms > 0
    assert e.search_info()["tree_storage"] == "lds8"
    e.close()
    assert "LDS residency" not in capfd.readouterr().err
    # beyond 511 records: global-memory trees, one warning for the engine
    e = _native.HipEngine(env_id=2, mode=1, n_trees=32, n_sims=600, c_uct=0.05, gamma=1.0, kappa=0.3)   # (601^0.3: 7 children at most)
    e.set_weights(_capi.make_desc(3, [64], 2, "elu"), O.make_weights(34, 3, [64], 2))
    for _ in range(2):
        e.search(e.synthetic_roots())
    assert (e.results()["counts"].sum(1) == 600).all()
    d = e.search_info()
    assert d["kernel_form"] == "persistent" and d["tree_storage"] == "global" and d["lds_exit"] == "records" and d["max_records"] == 602
    e.close()
    assert capfd.readouterr().err.count("do not fit LDS residency (more than 511 records") == 1
    # ... and the other residency limit: 600 simulations with the default widening law give the root 25 children (> 16)
    e = _native.HipEngine(env_id=2, mode=1, n_trees=32, n_sims=600, c_uct=0.05, gamma=1.0)
    e.set_weights(_capi.make_desc(3, [64], 2, "elu"), O.make_weights(34, 3, [64], 2))
    e.search(e.synthetic_roots())
    assert e.search_info()["lds_exit"] == "children" and e.search_info()["max_children"] == 25
    e.close()
    assert "more than 16 children per node" in capfd.readouterr().err
    # wide networks: the team kernel (or, on a shared GPU, the per-layer launches), trees in HBM by design -- no warning
    e = _native.HipEngine(env_id=2, mode=1, n_trees=64, n_sims=6, c_uct=0.05, gamma=1.0)
    e.set_weights(_capi.make_desc(3, [1024] * 4, 2, "elu"), O.make_weights(34, 3, [1024] * 4, 2))
    e.search(e.synthetic_roots())
    d = e.search_info()
    assert d["kernel_form"] in ("team", "per_layer") and d["lds_exit"] == "not_applicable" and d["team_fallbacks"] in (0, 1)
    if d["kernel_form"] == "team":
        assert d["team_trees"] == 32 and d["team_parts"] == 1 and d["kernel_name"].startswith("ls_team_kernel<2, 1024")
    e.close()
    assert "LDS residency" not in capfd.readouterr().err


@pytest.mark.gpu
def test_search_info_names_the_residency_limit_that_applied(capfd, monkeypatch):
    """The two limits besides "more than 511 records": a mixture head has no 9-bit-id kernels, so its trees of 256 .. 511 records leave
    LDS at 255 records (AZG_LDS_EXIT_RECORDS, and the stderr line says 255); a carried root count of 65536 or more overflows the 8-bit-id
    records' 16-bit counters (AZG_LDS_EXIT_COUNTS)."""
    from alphazero_gym_amd import _native
    monkeypatch.delenv("AZG_QUIET", raising=False)
    # 300 simulations: 302 records, at most 6 children per node (301^0.3 < 6); 2x256 with three mixture components
    e = _native.HipEngine(env_id=2, mode=1, n_trees=32, n_sims=300, c_uct=0.05, gamma=1.0, kappa=0.3)
    e.set_weights(_capi.make_desc(3, [256, 256], 9, "elu", num_components=3), O.make_weights(34, 3, [256, 256], 9))
    e.search(e.synthetic_roots())
    assert (e.results()["counts"].sum(1) == 300).all()
    d = e.search_info()
    assert d["kernel_form"] == "persistent" and d["tree_storage"] == "global" and d["lds_exit"] == "records" and d["max_records"] == 302
    e.close()
    err = capfd.readouterr().err
    assert "do not fit LDS residency (more than 255 records" in err and "511" not in err
    # CartPole, 100 simulations (203 records) from roots that carry 70 000 visits
    e = _native.HipEngine(env_id=0, mode=0, n_trees=32, n_sims=100, c_uct=1.5, gamma=1.0, num_actions=2)
    e.set_weights(_capi.make_desc(4, [64, 64], 2, "relu"), O.make_weights(34, 4, [64, 64], 2))
    e.search(e.synthetic_roots(), np.full(32, 70000, dtype=np.int32))
    d = e.search_info()
    assert d["kernel_form"] == "persistent" and d["tree_storage"] == "global" and d["lds_exit"] == "counts" and d["max_records"] == 203
    e.close()
    assert "do not fit LDS residency (the root's visit count" in capfd.readouterr().err
