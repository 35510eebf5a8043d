"""Priorities fed back from the trainer's value errors (azg_selfplay_keep_errors / _priorities_trained, include/azgym_priority.h;
the *_errors entry points of include/azgym_train_errors.h): the numpy restatement of the rules, on top of priority_util.  TEST
INFRASTRUCTURE ONLY.  Importing it needs neither a GPU nor the native library.

The rules are exact.  The error of a trained row is float32(|float64(V) - float64(z)|).  A kept error is that, or the sentinel
-1.0f.  The d of a row: a seen entry (anything but the sentinel, NaN included) is its own d; an unseen one takes the largest seen
error of its net over the entries >= 0 (as the maximum of their bit patterns; 1.0f where the net has none), the value gap, or a
constant.  q follows by priority_util.priorities for a finite d; with alpha != 0 a NaN d has q = 1 and a +inf d q = 2^40."""
import numpy as np

import priority_util as P

UNSEEN = np.float32(-1.0)
UNSEEN_BITS = 0xBF800000
MAX, VALUE_GAP, CONSTANT = 0, 1, 2          # AZG_UNSEEN_*


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def loss_errors(raw0, z):
    """e = (float)fabs((double)raw[0] - (double)z) of every row."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(np.asarray(raw0, np.float32).astype(np.float64) - np.asarray(z, np.float32).astype(np.float64)).astype(np.float32)


def seen_max(err):
    """The largest entry >= 0 of ``err`` as the maximum of the bit patterns (-0.0f counts as +0.0f); None if there is none."""
    err = np.asarray(err, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = err >= 0
    if not ok.any():
        return None
    return np.abs(err[ok]).view(np.uint32).max().reshape(1).view(np.float32)[0]


def trained_d(err, n_nets, unseen, unseen_d=0.0, gap=None):
    """err [size_steps, n_trees] float32 -> the rows' d, float32 of the same shape.  ``gap``: AZG_UNSEEN_VALUE_GAP's d of every row."""
    err = np.asarray(err, np.float32)
    d = err.copy()
    T = err.shape[1] // n_nets
    for k in range(n_nets):
        block = err[:, k * T:(k + 1) * T]
        miss = block == UNSEEN
        if unseen == MAX:
            m = seen_max(block)
            fill = np.float32(1.0) if m is None else m
        elif unseen == VALUE_GAP:
            fill = np.asarray(gap, np.float32)[:, k * T:(k + 1) * T][miss]
        else:
            fill = np.float32(unseen_d)
        d[:, k * T:(k + 1) * T][miss] = fill
    return d


def trained_priorities(err, n_nets, alpha, eps, unseen, unseen_d=0.0, gap=None):
    """azg_selfplay_priorities_trained: err [size_steps, n_trees] -> q uint64 of the same shape."""
    d = trained_d(err, n_nets, unseen, unseen_d, gap)
    q = P.priorities(d, alpha, eps)
    if np.float32(alpha) != 0:   # outside azg_logf's domain: decided before it
        q[np.isnan(d)] = 1
        q[np.isposinf(d)] = P.Q_MAX
    return q
