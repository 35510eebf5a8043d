"""The trainer's moving average and the engine's target weight set, the part that runs without a GPU: the ABI's additions
(include/azgym_train_ema.h, include/azgym_target.h), the Python layer's refusals, the CPU double's answer to ``nets="target"``, and the
numpy restatement of the rule (tests/ema_util.py) held to two closed forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ema_util as E
import oracle_lib as O
from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent import population_trainer as PT
from alphazero_gym_amd.network.policies import make_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NEW_SYMBOLS = ("trainer_set_ema", "trainer_ema_info", "use_weights", "weights_info")


def test_abi_additions_are_optional_symbols(tmp_path):
    for s in NEW_SYMBOLS:
        assert s in _capi.OPTIONAL_SYMBOLS and s not in _capi.SYMBOLS
        assert s not in O.fns()   # (the CPU oracle has neither a trainer nor a second weight set)
    src = tmp_path / "use.c"
    src.write_text('#include "azgym_train_ema.h"\n'
                   '#include "azgym_target.h"\n'
                   "int use(azg_trainer* t, azg_engine* e, float* ema, const double* decay) {\n"
                   "    azg_ema_cfg c = {sizeof(azg_ema_cfg), 1, 1, 0, ema, decay};\n"
                   "    int64_t steps, updates;\n"
                   "    int32_t in_use, ready;\n"
                   "    return azg_trainer_set_ema(t, &c) + azg_trainer_set_ema(t, NULL) + azg_trainer_ema_info(t, &steps, &updates)\n"
                   "           + azg_use_weights(e, AZG_WEIGHTS_TARGET) + azg_use_weights(e, AZG_WEIGHTS_LIVE) + azg_weights_info(e, &in_use, &ready);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert _capi.ABI_VERSION == 1
    assert (_capi.WEIGHTS_LIVE, _capi.WEIGHTS_TARGET) == (0, 1)


def test_the_library_exports_the_symbols():
    from alphazero_gym_amd import _native
    lib = _native.lib()   # (loads without a GPU)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, "azg_" + s), s
        assert s in _native.fns()


def test_struct_size_matches_the_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "azgym_train_ema.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(azg_ema_cfg), offsetof(azg_ema_cfg, ema), offsetof(azg_ema_cfg, decay)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-o", str(exe)])
    size, at_ema, at_decay = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert C.sizeof(_capi.AzgEmaCfg) == size
    assert (_capi.AzgEmaCfg.ema.offset, _capi.AzgEmaCfg.decay.offset) == (at_ema, at_decay)


def test_ema_settings_and_their_refusals():
    assert PT._ema_settings(0.99, 3) == (0.99, 1)
    assert PT._ema_settings(0, 3) == (0.0, 1)
    assert PT._ema_settings([0.5, 0.0, 0.9], 3) == ([0.5, 0.0, 0.9], 1)
    assert PT._ema_settings(np.asarray([0.5, 0.25], np.float32), 2) == ([0.5, 0.25], 1)
    assert PT._ema_settings({"decay": 0.9, "every": 8}, 2) == (0.9, 8)
    assert PT._ema_settings({"decay": [0.9, 0.5]}, 2) == ([0.9, 0.5], 1)
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), [0.5, 1.0], [0.5, float("nan")]):
        with pytest.raises(ValueError, match=r"finite and in \[0, 1\)"):
            PT._ema_settings(bad, 2)
    for bad in ([0.5], [0.5, 0.5, 0.5], []):
        with pytest.raises(ValueError, match="entries for 2 nets"):
            PT._ema_settings(bad, 2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="every must be an int >= 1"):
            PT._ema_settings({"decay": 0.9, "every": bad}, 2)
    with pytest.raises(ValueError, match="takes decay and every"):
        PT._ema_settings({"decay": 0.9, "warmup": 10}, 2)
    with pytest.raises(ValueError, match="needs a decay"):
        PT._ema_settings({"every": 2}, 2)
    with pytest.raises(ValueError, match="a number or one number per net"):
        PT._ema_settings([[0.5, 0.5]], 2)
    with pytest.raises(ValueError, match="a number or one number per net"):
        PT._ema_settings("0.9", 2)


def test_the_constructor_refuses_before_it_touches_anything():
    """A bad ``ema`` is refused before the agents are looked at (no GPU, no native trainer needed to see it)."""
    with pytest.raises(ValueError, match=r"finite and in \[0, 1\)"):
        PT.PopulationTrainer([object(), object()], ema=1.0)
    with pytest.raises(ValueError, match="entries for 2 nets"):
        PT.PopulationTrainer([object(), object()], ema=[0.5])
    with pytest.raises(ValueError, match="every must be an int >= 1"):
        PT.PopulationTrainer([object(), object()], ema={"decay": 0.5, "every": 0})


@pytest.fixture
def cpu_selfplay(monkeypatch):
    """A one-policy ``PopulationSelfPlay`` on the tests' CPU double of the engine, which lacks the new symbols."""
    from alphazero_gym_amd import _native
    monkeypatch.setattr(_native, "HipEngine", O.OracleEngine)
    torch.manual_seed(0)
    pol = make_policy(4, 1, "discrete", [16], "relu", num_actions=2)
    sp = run.PopulationSelfPlay([pol], game="CartPole-v0", games_per_net=2, n_rollouts=4, c_uct=1.5, capacity_steps=3, max_episode_length=3)
    yield sp
    sp.close()


def test_an_engine_without_the_symbols_says_so(cpu_selfplay):
    sp = cpu_selfplay
    for call in (lambda: sp.engine.use_weights("target"), sp.engine.weights_info):
        with pytest.raises(NotImplementedError, match="no (use_weights|weights_info) entry point"):
            call()
    with pytest.raises(NotImplementedError, match="weights_info"):
        sp.evaluate(1, nets="target")
    with pytest.raises(NotImplementedError, match="weights_info"):
        sp.evaluate_search(1, nets="target")
    sp.reanalysing = True   # (the double keeps no states: only the check in front of the searches is reached)
    with pytest.raises(NotImplementedError, match="weights_info"):
        sp.reanalyse(slots=[0], nets="target")
    with pytest.raises(NotImplementedError, match="weights_info"):
        with sp.mcts.target_weights():
            pass
    assert sp.mcts._in_target is False
    for call in (lambda: sp.evaluate(1, nets="ema"), lambda: sp.evaluate_search(1, nets=None), lambda: sp.reanalyse(slots=[0], nets="both")):
        with pytest.raises(ValueError, match="nets must be 'live' or 'target'"):
            call()
    sp.play(1)   # the live path is what it was
    assert sp.engine.selfplay_ring()[0] == 1


def test_upload_target_flat_checks_its_tensor(cpu_selfplay):
    sp = cpu_selfplay
    desc = _capi.policy_tensors(sp.policies[0])[0]
    for flat in (torch.zeros(2, 8), torch.zeros(8), torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 16)[:, ::2]):
        with pytest.raises(ValueError, match="contiguous float32"):
            sp.upload_target_flat(desc, flat)
    with pytest.raises(ValueError, match="must live on the engine's GPU"):
        sp.upload_target_flat(desc, torch.zeros(1, 8))


def test_sync_weights_writes_nothing_inside_target_weights(cpu_selfplay):
    """Inside ``target_weights()`` a changed model is not uploaded (it would land in the target set); afterwards it is."""
    m = cpu_selfplay.mcts
    m.sync_weights()
    assert m.last_weight_sync is None   # (nothing changed since the constructor's upload)
    before = list(m._versions)
    with torch.no_grad():
        next(m.models[0].parameters()).add_(1.0)
    m._in_target = True
    m.sync_weights()
    m.sync_weights(force=True)
    assert m._versions == before and m.last_weight_sync is None
    m._in_target = False
    m.sync_weights()
    assert m.last_weight_sync == "host" and m._versions != before


def test_numpy_rule_constant_parameters_stay_put():
    rng = np.random.RandomState(0)
    p = (rng.randn(3, 37) * np.float32(10.0) ** rng.randint(-20, 20, (3, 37))).astype(np.float32)
    ema, made = E.ema_after(p, [p] * 7, [0.0, 0.5, 0.999], every=2)
    assert made == 3
    np.testing.assert_array_equal(ema.view(np.int32), p.view(np.int32))


def test_numpy_rule_matches_the_closed_form_on_exact_values():
    """decay 0.5 over small integers: every difference, product and sum is exactly representable, so after n updates towards a
    constant p the average is p + (ema0 - p) / 2^n exactly."""
    assert E.one_minus(0.5, 2).tolist() == [0.5, 0.5] and E.one_minus([0.0, 0.75], 2).tolist() == [1.0, 0.25]
    assert E.one_minus(0.9, 1)[0] == np.float32(1.0 - 0.9) and E.one_minus(0.9, 1).dtype == np.float32
    ema0 = np.asarray([[0.0, 64.0, -128.0, 3.0], [1024.0, -5.0, 0.5, 96.0]], np.float32)
    p = np.asarray([[32.0, 0.0, 128.0, 3.0], [0.0, 11.0, -0.5, 32.0]], np.float32)
    ema = ema0
    for n in range(1, 6):
        ema = E.ema_step(ema, p, 0.5)
        assert ema.dtype == np.float32
        np.testing.assert_array_equal(ema, (p.astype(np.float64) + (ema0.astype(np.float64) - p) / 2.0 ** n).astype(np.float32))
        assert ((p.astype(np.float64) + (ema0.astype(np.float64) - p) / 2.0 ** n) == ema.astype(np.float64)).all()   # (nothing was rounded)
    got, made = E.ema_after(ema0, [p] * 6, 0.5, every=3)
    assert made == 2
    np.testing.assert_array_equal(got, E.ema_step(E.ema_step(ema0, p, 0.5), p, 0.5))
    got, made = E.ema_after(ema0, [p] * 2, 0.5, every=3, first_step=5)   # steps 5 and 6: one update
    assert made == 1
    np.testing.assert_array_equal(got, E.ema_step(ema0, p, 0.5))
