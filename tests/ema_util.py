"""The moving average of the trainer's parameters (include/azgym_train_ema.h) restated in numpy float32, for the tests of the device
kernel: ema' = ema + om * (p - ema) with om = float32(1 - decay), every operation rounded by itself.  Needs neither a GPU nor the
native library."""
import numpy as np


def one_minus(decay, K):
    """om[K] float32: float32(1.0 - decay_k), the subtraction in float64 (the host's); ``decay`` a number or K numbers."""
    d = np.full(K, decay, np.float64) if np.ndim(decay) == 0 else np.asarray(decay, np.float64)
    assert d.shape == (K,)
    return (1.0 - d).astype(np.float32)


def ema_step(ema, params, decay):
    """One update of ema [K, P] towards params [K, P] (float32 arrays); a new array."""
    ema, params = np.asarray(ema), np.asarray(params)
    assert ema.dtype == params.dtype == np.float32 and ema.shape == params.shape and ema.ndim == 2
    om = one_minus(decay, ema.shape[0])[:, None]
    diff = params - ema            # float32, rounded
    prod = om * diff               # float32, rounded
    return ema + prod              # float32, rounded


def ema_after(start, snapshots, decay, every=1, first_step=1):
    """The average after the optimiser steps first_step, first_step + 1, ... whose parameters are ``snapshots`` (a sequence of [K, P]
    float32 arrays, the parameters after each step), from ``start``: it moves after every step whose number is a multiple of
    ``every``.  Returns (ema, updates made)."""
    ema, made = np.array(start, np.float32, copy=True), 0
    for s, p in enumerate(snapshots, start=first_step):
        if s % every == 0:
            ema = ema_step(ema, p, decay)
            made += 1
    return ema, made
