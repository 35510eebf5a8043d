"""The online epoch on the CPU (include/azgym_train_online.h): the ctypes struct against the header as gcc lays it out, the library's
entry points, the Python refusals raised before any native call, and the numpy side of tests/test_online_replay.py's first claim --
what the first minibatch draws from the planted errors."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import nstep_util as N
import online_replay_util as U
import priority_feedback_util as F
import priority_util as P
from alphazero_gym_amd import _capi
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "n_minibatches", "batch_size", "sample_index", "beta", "prio", "drawn")


def test_the_struct_is_the_headers(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc, "a C compiler"
    src = tmp_path / "layout.c"
    prints = "".join(f'printf("%zu ", offsetof(azg_online_epoch, {f}));' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "azgym_train_online.h"\n'
                   f'int main(void) {{ printf("%zu ", sizeof(azg_online_epoch)); {prints} return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.AzgOnlineEpoch)] + [getattr(_capi.AzgOnlineEpoch, f).offset for f in FIELDS]
    assert [n for n, _ in _capi.AzgOnlineEpoch._fields_] == list(FIELDS)
    assert _capi.AzgOnlineEpoch.prio.size == C.sizeof(_capi.AzgTrainedPriorityConfig)
    c = _capi.trained_priority_config(0.6, 1e-3, 0.75)
    assert (c.struct_size, c.unseen, c.unseen_d) == (C.sizeof(c), _capi.UNSEEN_CONSTANT, 0.75)
    assert _capi.trained_priority_config(1.0, 1e-3, "value_gap").unseen == _capi.UNSEEN_VALUE_GAP


def test_the_library_has_the_entry_points():
    from alphazero_gym_amd import _native
    f = _native.fns()
    for name in ("trainer_epoch_online", "trainer_epoch_online_nets"):
        assert name in f and len(f[name].argtypes) == 8
    # without them the binding says what is missing
    tr = _capi.Trainer.__new__(_capi.Trainer)
    tr._f, tr._h, tr.n_nets = {}, C.c_void_p(), 1
    with pytest.raises(NotImplementedError, match="azg_trainer_epoch_online"):
        tr.epoch_online(None, 0, 1, 1, 0, 0.0, _capi.trained_priority_config(0.6, 1e-3), None, None, None, 0)


def _trainer(losses="device", max_batch=64, agents=2):
    """A PopulationTrainer as far as train_online_ring's own checks read it."""
    t = PopulationTrainer.__new__(PopulationTrainer)
    t.losses, t.max_batch, t.agents = losses, max_batch, [None] * agents
    t.device = types.SimpleNamespace(index=0)
    return t


def _selfplay(prioritized, device_id=0, n_nets=2):
    engine = types.SimpleNamespace(cfg=types.SimpleNamespace(device_id=device_id))
    return types.SimpleNamespace(prioritized=prioritized, engine=engine, n_nets=n_nets, _sample_index=0)


def test_python_refusals_before_any_native_call():
    full = {"alpha": 0.6, "eps": 1e-3, "beta": 0.4, "feedback": "max"}
    with pytest.raises(ValueError, match='losses="device"'):
        _trainer(losses="torch").train_online_ring(_selfplay(full), 2)
    for prioritized in (None, {"alpha": 0.6, "eps": 1e-3, "beta": 0.4}):
        with pytest.raises(ValueError, match='"feedback"'):
            _trainer().train_online_ring(_selfplay(prioritized), 2)
    for M, batch in ((0, 8), (-1, 8), (2, 0), (2, 65)):
        with pytest.raises(ValueError, match="n_minibatches >= 1 and a batch_size of 1..64"):
            _trainer().train_online_ring(_selfplay(full), M, batch_size=batch)
    with pytest.raises(ValueError, match="another GPU"):
        _trainer().train_online_ring(_selfplay(full, device_id=1), 2)
    with pytest.raises(ValueError, match="3 nets, the trainer 2"):
        _trainer().train_online_ring(_selfplay(full, n_nets=3), 2)


@pytest.mark.parametrize("name,size", [("cartpole", 16), ("population", 10)])
def test_what_the_first_minibatch_draws_from_the_planted_errors(name, size):
    """tests/test_online_replay.py's planted errors under alpha 1, unseen "max": the unseen rows take their net's largest seen error
    (+inf in net 0, 10 elsewhere), so the first 16 draws of every net fall on its planted rows, some row more than once, and never on
    the NaN row."""
    case = N.CASES[name]
    K, G, T = case.nets, case.games, case.T
    planted, spots = U.plant(size, G, K, 30)
    assert (planted == U.SEEN).sum() == size * G - 14 * K - 2
    q, first = U.numpy_draw(planted, K, 1.0, 1e-3, "max", case.kw["seed"], case.kw.get("tree_id_base", 0), 7, 16)
    q_net, err_net = U.per_net(q, K), U.per_net(planted, K)
    assert (q_net[0][(err_net[0] == F.UNSEEN) | np.isinf(err_net[0])] == P.Q_MAX).all() and (q_net[0] == P.Q_MAX).sum() == 7
    assert (q_net[0][np.isnan(err_net[0])] == 1).all()
    for k in range(1, K):
        assert (q_net[k][err_net[k] == F.UNSEEN] == q_net[k][err_net[k] == U.LARGE][0]).all()
    assert first.shape == (K, 16)
    for k in range(K):
        assert set(first[k].tolist()) <= set(spots[k].tolist()), f"net {k}"
        assert len(set(first[k].tolist())) < 16
        assert not np.isnan(err_net[k][first[k]]).any()
    # net 0's draws all fall on the seven rows at 2^40
    assert (q_net[0][first[0]] == P.Q_MAX).all()
