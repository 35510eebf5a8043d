"""N-step return value targets for the device replay ring (azg_selfplay_keep_transitions / _transitions / _nstep_targets,
include/azgym_nstep.h): the cases of tests/test_nstep_targets.py and the CPU truth.  TEST INFRASTRUCTURE ONLY.

The truth is numpy over the trace of selfplay_ref.cpu_selfplay: per game and step the reward (continuous mode: divided by
reward_scale, the units a tree node holds), the float64 value target (selfplay_ref.value_target), the action and the end kind; the
target is the float64 recurrence acc = r + gamma * acc folded from the window's far end.  tests/test_nstep_host.py pins the builder on
hand-written sequences on the CPU."""
import functools

import numpy as np

import reanalyse_util as R
import selfplay_ref as SR
from alphazero_gym_amd import _capi

END_NONE, END_TERMINAL, END_LENGTH = 0, 1, 2
END_OF = {None: END_NONE, "done": END_TERMINAL, "both": END_TERMINAL, "length": END_LENGTH}
N_STEPS = (0, 1, 3, 1000)
GAMMAS = (None, 0.9)          # None: the search's gamma
POP_GAMMAS = (1.0, 0.97, 0.5)


def _cases():
    """The settings of reanalyse_util's cases with the episode limits and sizes the n-step windows need."""
    c, steps = {}, {}
    base = R.CASES["cartpole"]
    c["cartpole"] = R.Case(base.kw, base.net, games=33, max_len=12)
    steps["cartpole"] = 24
    base = R.CASES["pendulum"]
    c["pendulum"] = R.Case(base.kw, base.net, games=17, max_len=5)
    steps["pendulum"] = 24
    base = R.CASES["many_children"]
    c["many_children"] = R.Case(base.kw, base.net, games=base.games, max_len=4, blob=base._blob)
    steps["many_children"] = 7
    base = R.CASES["wide"]
    c["wide"] = R.Case(base.kw, base.net, games=32, max_len=4)
    steps["wide"] = 7
    base = R.CASES["population"]
    settings = [dict(s, gamma=g) for s, g in zip(base.net_settings, POP_GAMMAS)]
    c["population"] = R.Case(base.kw, base.net, games=33, max_len=6, nets=3, net_settings=settings, net_rollouts=base.net_rollouts)
    steps["population"] = 10
    return c, steps


CASES, STEPS = _cases()
# (case, ring capacity, fifo): the CartPole ring wraps in FIFO mode; every other case runs a STOP ring with one unused slot
RINGS = [("cartpole", 16, True), ("cartpole", 24, False)] + [(n, STEPS[n] + 1, False) for n in ("pendulum", "many_children", "wide", "population")]
RING_IDS = [f"{n}-{'fifo' if f else 'stop'}{c}" for n, c, f in RINGS]


def search_gamma(case):
    """[games]: the gamma each game's net searches with."""
    if case.net_settings is None:
        return np.full(case.games, float(case.kw["gamma"]))
    return np.repeat(np.asarray([s["gamma"] for s in case.net_settings], np.float64), case.T)


# ------------------------------------------------------------------------------------------------ the CPU truth

def nstep_returns(reward, value, end, n_step, gamma):
    """The float64 n-step returns of a stored range: reward, value, end [S, G] in chronological order (row 0: the oldest stored step,
    S - 1: the newest), gamma a scalar or [G].  Walk forward from s at most n_step steps, stopping at the first step that ended its
    episode or at the newest one.  A terminal end inside the window: no bootstrap, the rewards s .. e.  Otherwise the bootstrap is the
    value of step L = min(s + n_step, newest, a time-limit end inside the window) and the rewards are s .. L - 1."""
    reward, value, end = np.asarray(reward, np.float64), np.asarray(value, np.float64), np.asarray(end)
    S, G = reward.shape
    gam = np.broadcast_to(np.asarray(gamma, np.float64), (G,))
    out = np.zeros((S, G), np.float64)
    for g in range(G):
        ended = [i for i in range(S) if end[i, g] != END_NONE]
        for s in range(S):
            e = min([i for i in ended if i >= s] + [S - 1])
            inside = e < s + n_step and end[e, g] != END_NONE
            if inside and end[e, g] == END_TERMINAL:
                acc, first = np.float64(0.0), e
            else:
                L = min(s + n_step, S - 1, e if inside else S - 1)
                acc, first = value[L, g], L - 1
            for i in range(first, s - 1, -1):
                prod = gam[g] * acc          # (rounded by itself: no fused multiply-add)
                acc = reward[i, g] + prod
            out[s, g] = acc
    return out


def direct_returns(reward, value, end, n_step, gamma):
    """The same targets as the explicit sum  r_s + g r_{s+1} + ... + g^m v_{s+m}  (added up from the near end, powers by repeated
    multiplication): equal to nstep_returns bit for bit only where every product and sum is exact (gamma 1 and small integers)."""
    reward, value, end = np.asarray(reward, np.float64), np.asarray(value, np.float64), np.asarray(end)
    S, G = reward.shape
    out = np.zeros((S, G), np.float64)
    for g in range(G):
        for s in range(S):
            tot, w, i = 0.0, 1.0, s
            while True:
                if i == s + n_step or (i == S - 1 and end[i, g] != END_TERMINAL) or end[i, g] == END_LENGTH:
                    tot += w * value[i, g]
                    break
                tot += w * reward[i, g]
                w *= gamma
                if end[i, g] == END_TERMINAL:
                    break
                i += 1
            out[s, g] = tot
    return out


def ring_layout(capacity, fifo, total):
    """ReplayBuffer.store in steps (buffers.py:75-82), as azg_selfplay_step keeps its books: after ``total`` steps, (held, oldest) --
    held[slot] the step each used slot holds, oldest the slot of the oldest one."""
    held, insert = [], 0
    for s in range(total):
        if len(held) < capacity:
            held.append(s)
        else:
            assert fifo
            held[insert] = s
            insert = (insert + 1) % len(held)
    return np.asarray(held, np.int64), insert


def ring_targets(reward, value, end, held, n_step, gamma):
    """The float32 V_target column of a ring [slots, G] whose slot j holds step held[j] of the run (reward, value, end [steps, G] of
    the whole run): windows see the stored steps only."""
    order = np.argsort(held)   # chronological position -> slot
    st = np.asarray(held)[order]
    assert np.array_equal(st, np.arange(st[0], st[0] + len(st)))
    z = nstep_returns(reward[st], value[st], end[st], n_step, gamma)
    out = np.zeros(z.shape, np.float32)
    out[order] = z.astype(np.float32)
    return out


def window_kinds(end, n_step):
    """How many rows of a stored range (end [S, G], chronological) have a window of each kind at ``n_step`` >= 1: closed by a terminal
    end, stopped at a time-limit end, cut by the newest step, or of full length."""
    S, G = end.shape
    k = dict(terminal_inside=0, length_inside=0, cut_by_newest=0, full=0)
    for g in range(G):
        for s in range(S):
            hit = [i for i in range(s, min(s + n_step, S)) if end[i, g] != END_NONE]
            if hit:
                k["terminal_inside" if end[hit[0], g] == END_TERMINAL else "length_inside"] += 1
            else:
                k["cut_by_newest" if s + n_step > S - 1 else "full"] += 1
    return k


def transitions_of(trace, steps, games, cont, on_policy, reward_scale):
    """reward, value [steps, games] float64, action float32, end int32 from cpu_selfplay's trace; both: the env's done and the length
    limit fell on the same step (END_TERMINAL)."""
    t = dict(reward=np.zeros((steps, games)), value=np.zeros((steps, games)), action=np.zeros((steps, games), np.float32),
             end=np.zeros((steps, games), np.int32), both=np.zeros((steps, games), bool))
    for r in trace:
        s, g = r["step"], r["game"]
        t["reward"][s, g] = np.float64(r["reward"]) / np.float64(reward_scale) if cont else np.float64(r["reward"])
        t["value"][s, g] = SR.value_target(r["counts"], r["Q"], on_policy, cont)
        t["action"][s, g] = r["action"]
        t["end"][s, g] = END_OF[r["why"]]
        t["both"][s, g] = r["why"] == "both"
    return t


@functools.lru_cache(maxsize=None)
def reference(name, steps=None):
    """The restatement's self-play of case ``name`` (net by net): rows [steps, G, row_len], states [steps, G, S] and the transitions
    [steps, G].  Computed once per process, read-only.  (The first ``s`` steps of a run are the run of ``s`` steps.)"""
    case = CASES[name]
    steps = STEPS[name] + 3 if steps is None else steps
    parts = []
    for k in range(case.nets):
        kw = case.net_kw(k)
        trace = []
        out = SR.cpu_selfplay(kw, case.desc(), case.blob(k), case.T, steps, begin=dict(max_episode_length=case.max_len), trace=trace)
        t = transitions_of(trace, steps, case.T, case.cont, kw.get("v_target", "off_policy") == "on_policy",
                           kw.get("reward_scale", _capi.PENDULUM_R_SCALE))
        t["rows"] = out["rows"].reshape(steps, case.T, -1)
        t["states"] = np.zeros((steps, case.T, len(trace[0]["state"])))
        for r in trace:
            t["states"][r["step"], r["game"]] = r["state"]
        parts.append(t)
    out = {k: np.concatenate([p[k] for p in parts], 1) for k in parts[0]}
    for v in out.values():
        v.setflags(write=False)
    return out


bits32, bits64 = R.bits32, R.bits64
