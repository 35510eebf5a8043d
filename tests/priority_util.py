"""Prioritised sampling from the device replay ring (azg_selfplay_priorities / _sample_rows / _sample_slots,
include/azgym_priority.h): the numpy truth of tests/test_priority_host.py and tests/test_priority_sample.py.  TEST INFRASTRUCTURE ONLY.

The rule is exact, so the truth is plain: a numpy Philox4x32-10 (pinned against the oracle's own draw on the CPU), the priority with
exp and log through the oracle's azg_expf / azg_logf (oracle_lib.math_eval fn 0 and fn 3), prefix sums in Python integers, the target
as (x * total) >> 64 and a bisection for the least index whose prefix sum exceeds it."""
import bisect

import numpy as np

import oracle_lib as O

STREAM_ACT, STREAM_SAMPLE, STREAM_SLOT = 3, 5, 6
Q_ONE = 1 << 20          # p = 1 in q's fixed point
Q_MAX = 1 << 40
P_MIN, P_MAX = np.float32(2.0 ** -20), np.float32(2.0 ** 20)
ALPHAS = (0.0, 0.6, 1.0)
EPS = 1e-3
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ Philox4x32-10

def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays (or scalars) of counters under one key: the four output words, uint64 arrays
    holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & _M32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]    # (32 x 32 bits: fits 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def draw(seed, tree, search, d, stream):
    """azg_draw: counter (tree, search, d, stream), key the seed's two halves."""
    return philox4x32(tree, search, d, stream, int(seed) & 0xFFFFFFFF, int(seed) >> 32)


def draw_x(seed, tree, search, d, stream):
    """The 64 bits a sampling draw uses, as Python ints: word 0 high, word 1 low."""
    w = draw(seed, tree, search, d, stream)
    return [(int(a) << 32) | int(b) for a, b in zip(w[0], w[1])]


# ------------------------------------------------------------------------------------------------ the priority rule

def gap(value, z):
    """AZG_PRIO_VALUE_GAP's d: (float)fabs(v - (double)z), v float64, z the float32 of the V_target column."""
    return np.abs(np.asarray(value, np.float64) - np.asarray(z, np.float32).astype(np.float64)).astype(np.float32)


def p_of_d(d, alpha, eps):
    """p = azg_expf(alpha * azg_logf(d + eps)) in float32, every step rounded by itself; alpha == 0: 1."""
    d = np.asarray(d, np.float32)
    alpha, eps = np.float32(alpha), np.float32(eps)
    if alpha == 0:
        return np.ones(d.shape, np.float32)
    with np.errstate(all="ignore"):
        s = (d + eps).astype(np.float32)
        log = O.math_eval(3, s.reshape(-1)).astype(np.float32)
        prod = (alpha * log).astype(np.float32)
        return O.math_eval(0, prod).astype(np.float32).reshape(d.shape)


def q_of_p(p):
    """The fixed-point priority: 1 unless p >= 2^-20 (NaN: 1), 2^40 from 2^20 on, else (uint64)((double)p * 2^20)."""
    p = np.asarray(p, np.float32)
    q = np.ones(p.shape, np.uint64)
    with np.errstate(invalid="ignore"):
        ok, big = p >= P_MIN, p >= P_MAX
    mid = ok & ~big
    q[mid] = (p[mid].astype(np.float64) * 1048576.0).astype(np.uint64)
    q[big] = Q_MAX
    return q


def priorities(d, alpha, eps=EPS):
    return q_of_p(p_of_d(d, alpha, eps))


# ------------------------------------------------------------------------------------------------ the draws

def prefix(q):
    """Inclusive prefix sums of q as Python ints."""
    out, acc = [], 0
    for v in np.asarray(q).reshape(-1):
        acc += int(v)
        out.append(acc)
    return out


def pick(csum, x):
    """The least i with csum[i] > target, target the high 64 bits of x * total."""
    target = (int(x) * csum[-1]) >> 64
    return bisect.bisect_right(csum, target)


def row_draws(q_net, seed, first_tree, sample_index, n_order):
    """n_order draws over one net's rows: q_net in the net's own numbering (slot * T + game)."""
    csum = prefix(q_net)
    xs = draw_x(seed, first_tree, sample_index, np.arange(n_order, dtype=np.uint64), STREAM_SAMPLE)
    return np.asarray([pick(csum, x) for x in xs], np.int32)


def sample_rows(q, n_nets, seed, tree_id_base, sample_index, n_order):
    """azg_selfplay_sample_rows: q [size_steps, n_trees] -> int32 [n_nets, n_order]."""
    q = np.asarray(q)
    T = q.shape[1] // n_nets
    return np.stack([row_draws(q[:, k * T:(k + 1) * T].reshape(-1), seed, tree_id_base + k * T, sample_index, n_order) for k in range(n_nets)])


def sample_slots(q, seed, tree_id_base, sample_index):
    """azg_selfplay_sample_slots: q [size_steps, n_trees] -> int32 [n_trees]."""
    q = np.asarray(q)
    B = q.shape[1]
    xs = draw_x(seed, tree_id_base + np.arange(B, dtype=np.uint64), sample_index, 0, STREAM_SLOT)
    return np.asarray([pick(prefix(q[:, t]), xs[t]) for t in range(B)], np.int32)
