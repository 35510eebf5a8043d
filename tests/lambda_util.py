"""Lambda-return value targets for the device replay ring (azg_selfplay_lambda_targets / _nets, include/azgym_lambda.h): the CPU
truth of tests/test_lambda_targets.py.  TEST INFRASTRUCTURE ONLY.

The truth is numpy over the same kept transitions as nstep_util's: the window of nstep_util.nstep_returns, folded from its far end in
float64 scalars with every product and sum rounded by itself.  tests/test_lambda_host.py pins it on hand-written sequences, against
the explicit mixture of m-step returns and against nstep_util.nstep_returns at its edges."""
import numpy as np

import nstep_util as N

LAMBDAS = (0.0, 0.5, 0.95, 1.0)
# the least share of stored rows whose float32 target at lambda 0.5, n_step 3 must differ in bits from BOTH the n-step and the
# 1-step target: measured 0.429 .. 0.816 on nstep_util's five cases, so a call that wrote either of them could not pass for lambda's
MIN_SHARE = 0.4


def per_game(x, G, dtype):
    """A scalar or [G] -> [G]."""
    return np.broadcast_to(np.asarray(x, dtype), (G,))


def window(end, s, n_step):
    """(L, terminal) of the row at chronological position s of one game column (end [S]): nstep_util.nstep_returns' window."""
    S = end.shape[0]
    for i in range(s, min(s + n_step, S)):
        if end[i] != N.END_NONE:
            return i, bool(end[i] == N.END_TERMINAL)
    return min(s + n_step, S - 1), False


def lambda_returns(reward, value, end, n_step, lam, gamma):
    """The float64 lambda-returns of a stored range: reward, value, end [S, G] in chronological order; n_step, lam and gamma a scalar
    or [G].  n_step 0: the value itself."""
    reward, value, end = np.asarray(reward, np.float64), np.asarray(value, np.float64), np.asarray(end)
    S, G = reward.shape
    ns, lams, gam = per_game(n_step, G, np.int64), per_game(lam, G, np.float64), per_game(gamma, G, np.float64)
    out = np.zeros((S, G), np.float64)
    for g in range(G):
        lm, gm = np.float64(lams[g]), np.float64(gam[g])
        om = np.float64(1.0) - lm
        for s in range(S):
            L, terminal = window(end[:, g], s, int(ns[g]))
            acc, i = (np.float64(0.0), L) if terminal else (value[L, g], L - 1)
            if i >= s:
                prod = gm * acc              # (rounded by itself: no fused multiply-add)
                acc = reward[i, g] + prod
                i -= 1
            while i >= s:
                a = om * value[i + 1, g]
                b = lm * acc
                mix = a + b
                prod = gm * mix
                acc = reward[i, g] + prod
                i -= 1
            out[s, g] = acc
    return out


def mixture_returns(reward, value, end, n_step, lam, gamma):
    """The same targets as the explicit mixture  (1 - lam) sum_{m < M} lam^(m-1) G^(m) + lam^(M-1) G^(M),  G^(m) nstep_util's m-step
    return as the explicit sum (direct_returns) and M the length of the row's window: equal to lambda_returns bit for bit only where
    every product and sum is exact."""
    reward, value, end = np.asarray(reward, np.float64), np.asarray(value, np.float64), np.asarray(end)
    S, G = reward.shape
    out = np.zeros((S, G), np.float64)
    if n_step == 0:
        return value.copy()
    Gm = [None] + [N.direct_returns(reward, value, end, m, gamma) for m in range(1, min(n_step, S) + 1)]
    for g in range(G):
        for s in range(S):
            L, terminal = window(end[:, g], s, n_step)
            M = L - s + 1 if terminal else L - s   # the window's length in steps (0: the row bootstraps from its own value)
            if M == 0:
                out[s, g] = value[s, g]
                continue
            tot, w = 0.0, 1.0
            for m in range(1, M):
                tot += (1.0 - lam) * w * Gm[m][s, g]
                w *= lam
            out[s, g] = tot + w * Gm[M][s, g]
    return out


def ring_lambda_targets(reward, value, end, held, n_step, lam, gamma):
    """The float32 V_target column of a ring [slots, G] whose slot j holds step held[j] of the run (nstep_util.ring_targets' form)."""
    order = np.argsort(held)   # chronological position -> slot
    st = np.asarray(held)[order]
    assert np.array_equal(st, np.arange(st[0], st[0] + len(st)))
    z = lambda_returns(reward[st], value[st], end[st], n_step, lam, gamma)
    out = np.zeros(z.shape, np.float32)
    out[order] = z.astype(np.float32)
    return out


def share_apart(reward, value, end, held, n_step, lam, gamma):
    """The share of a ring's rows whose lambda target differs in bits from both the n-step and the 1-step target."""
    z = N.bits32(ring_lambda_targets(reward, value, end, held, n_step, lam, gamma))
    a = N.bits32(N.ring_targets(reward, value, end, held, n_step, gamma))
    b = N.bits32(N.ring_targets(reward, value, end, held, 1, gamma))
    return float(((z != a) & (z != b)).mean())
