"""Refreshing the replay ring's bootstrap values from the value head (azg_selfplay_refresh_values, include/azgym_refresh.h): the truth
of tests/test_value_refresh.py.  TEST INFRASTRUCTURE ONLY.

The truth of a row's value is the path test_population_eval.py / test_oracle_mlp.py pin bit for bit: the CPU oracle's MLP evaluation of
net k's weights on the row's downloaded float32 observation columns (where the oracle cannot take the shape: ``mlp_eval`` of a one-net
engine holding those weights), widened to float64.  The builders below only say WHICH rows get WHOSE value and in what order the
targets see them; tests/test_value_refresh_host.py pins them on a hand-written example."""
import numpy as np

import nstep_util as N
import oracle_lib as O
from alphazero_gym_amd import _capi

CASES, STEPS, RINGS, RING_IDS = N.CASES, N.STEPS, N.RINGS, N.RING_IDS


def net_values(obs, T, evaluate):
    """float64 [S, G]: net k's value of every observation of its own games.  obs [S, G, S_obs] float32, the ring's observation columns
    slot by slot; net k owns games k*T .. k*T+T-1; ``evaluate(k, x)``: float32 [n] values of x [n, S_obs] under net k's weights."""
    obs = np.asarray(obs)
    assert obs.dtype == np.float32 and obs.ndim == 3 and obs.shape[1] % T == 0
    S, G, So = obs.shape
    out = np.zeros((S, G), np.float64)
    for k in range(G // T):
        x = np.ascontiguousarray(obs[:, k * T:(k + 1) * T]).reshape(S * T, So)
        v = np.asarray(evaluate(k, x))
        assert v.dtype == np.float32 and v.shape == (S * T,)
        out[:, k * T:(k + 1) * T] = v.reshape(S, T).astype(np.float64)
    return out


def refreshed(old, truth, slots=None):
    """The kept value column [S, G] after a refresh of ``slots`` (None: every slot; a slot may be listed twice): the listed slots take
    the truth, the others keep what they held."""
    old, truth = np.asarray(old, np.float64), np.asarray(truth, np.float64)
    assert old.shape == truth.shape
    out = old.copy()
    idx = np.arange(old.shape[0]) if slots is None else np.asarray(list(slots), np.int64)
    out[idx] = truth[idx]
    return out


def slot_targets(reward, value, end, held, returns):
    """The float32 V_target column [slots, G] of a ring whose slot j holds step held[j] of the run, from columns given SLOT BY SLOT
    (the ring's downloads; nstep_util.ring_targets takes the whole run's instead): ``returns(reward, value, end)`` -- nstep_util.
    nstep_returns or lambda_util.lambda_returns with their settings bound -- sees the stored steps in chronological order."""
    order = np.argsort(held)   # chronological position -> slot
    st = np.asarray(held)[order]
    assert np.array_equal(st, np.arange(st[0], st[0] + len(st)))
    z = returns(np.asarray(reward)[order], np.asarray(value)[order], np.asarray(end)[order])
    out = np.zeros(z.shape, np.float32)
    out[order] = z.astype(np.float32)
    return out


def refresh_blob(case, k):
    """Net k's weights of a refresh in the tests: other weights than the games were played with, with a value head that depends on
    every input (a refresh with stale weights, or one that reads the wrong columns, cannot pass)."""
    in_dim, hidden, n_dist, _, _ = case.net
    return O.make_weights(900 + 7 * k, in_dim, list(hidden), n_dist, scale=2.0)


def oracle_evaluator(kws, desc, blobs, fallback=None):
    """``evaluate`` of net_values: the oracle's MLP evaluation under blobs[k] (settings kws[k]); ``fallback(k)``: a one-net engine with
    those weights, asked where the oracle refuses the shape."""
    def evaluate(k, x):
        try:
            o = O.OracleEngine(**dict(kws[k], n_trees=1))
        except _capi.EngineError:
            o = None
        if o is not None:
            try:
                o.set_weights(desc, blobs[k])
                return o.mlp_eval(x)[0]
            except _capi.EngineError:
                if fallback is None:
                    raise
            finally:
                o.close()
        e = fallback(k)
        try:
            return e.mlp_eval(x)[0]
        finally:
            e.close()
    return evaluate


def case_truth(case, obs, blobs, fallback=None):
    """float64 [S, G]: the refreshed value of every row of ``case``'s ring under ``blobs`` (one per net)."""
    return net_values(obs, case.T, oracle_evaluator([case.net_kw(k) for k in range(case.nets)], case.desc(), blobs, fallback))


bits32, bits64 = N.bits32, N.bits64
