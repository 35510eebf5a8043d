"""CPU: the host half of the population trainer's epoch call (azg_trainer_epoch) -- the minibatch boundaries, the row addressing
that ``_capi.epoch_rows`` describes, and the ``losses="device"`` guard.  The kernels are tested on the GPU in
test_population_train_epoch.py."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent import population_trainer as PT


def _while_loop(n, batch_size):
    """PopulationTrainer.train_on_rows's loop, transcribed."""
    out, i = [], 0
    while i < n:
        j = n if i + 2 * batch_size > n else i + batch_size
        out.append((i, j))
        i = j
    return out


@pytest.mark.parametrize("batch_size", [1, 2, 7, 32, 64])
def test_minibatch_bounds(batch_size):
    for n in range(1, 201):
        got = PT.minibatch_bounds(n, batch_size)
        assert got == _while_loop(n, batch_size), n
        assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        assert all(1 <= j - i <= 2 * batch_size - 1 for i, j in got)
    assert PT.minibatch_bounds(0, batch_size) == []
    with pytest.raises(ValueError):
        PT.minibatch_bounds(5, 0)


def _address(r, k, i):
    """include/azgym_train.h: the float offset of row i of net k."""
    return ((i // r.group) * r.group_stride + k * r.net_stride + i % r.group) * r.row_len


def test_epoch_rows_plain_layout():
    K, n, S, A = 3, 10, 4, 2
    r = _capi.epoch_rows(0x1000, S, A, n)
    assert r.struct_size == C.sizeof(_capi.AzgEpochRows) == 48
    assert (r.row_len, r.state_dim, r.n_actions, r.rows_per_net, r.rows) == (S + 3 * A + 1, S, A, n, 0x1000)
    assert (r.group, r.net_stride) == (n, n)
    flat = np.arange(K * n * r.row_len, dtype=np.float32)
    rows = flat.reshape(K, n, r.row_len)
    for k in range(K):
        for i in range(n):
            at = _address(r, k, i)
            np.testing.assert_array_equal(flat[at:at + r.row_len], rows[k, i])
    assert _capi.epoch_rows(None, S, A, n).rows is None


def test_epoch_rows_ring_layout_is_splits_numbering():
    steps, K, T, S, A = 5, 3, 4, 3, 4
    r = _capi.epoch_rows(0x2000, S, A, steps * T, ring_trees=K * T, games_per_net=T)
    assert r.struct_size == C.sizeof(_capi.AzgEpochRows)
    assert (r.row_len, r.rows_per_net, r.group, r.group_stride, r.net_stride) == (S + 3 * A + 1, steps * T, T, K * T, T)
    flat = np.random.RandomState(0).randn(steps * K * T * r.row_len).astype(np.float32)
    ring = torch.from_numpy(flat).reshape(steps * K * T, r.row_len)       # [S][K * T][row], as azg_selfplay_rows_device lays it
    sp = types.SimpleNamespace(n_nets=K, games_per_net=T)
    split = run.PopulationSelfPlay._split(sp, ring, steps)
    assert len(split) == K
    for k in range(K):
        assert split[k].shape == (steps * T, r.row_len)
        for i in range(steps * T):
            at = _address(r, k, i)
            np.testing.assert_array_equal(flat[at:at + r.row_len], split[k][i].numpy())


def test_epoch_needs_device_losses():
    with pytest.raises(ValueError, match=re.escape('losses="device"')):
        PT._need_device_losses("torch", "train_epoch")
    PT._need_device_losses("device", "train_epoch")
    # the guard comes first: a trainer with nothing else in it is not looked at
    tr = PT.PopulationTrainer.__new__(PT.PopulationTrainer)
    tr.losses = "torch"
    with pytest.raises(ValueError, match=re.escape('losses="device"')):
        tr.train_epoch([torch.zeros(4, 11)], 4, 2)
    with pytest.raises(ValueError, match=re.escape('losses="device"')):
        tr.train_epoch_ring(None, np.zeros((1, 4), np.int64), 2)
