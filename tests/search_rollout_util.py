"""Search rollouts (azg_search_rollout, include/azgym_search_rollout.h): the cases of tests/test_search_rollout.py and the CPU truth
of a call.  TEST INFRASTRUCTURE ONLY.

``cpu_search_rollout`` restates the header's contract from the pieces tests/selfplay_ref.py composes a self-play step from: a
search-only ``OracleEngine`` (``set_search_index``, ``search(roots, carry)``, ``results()``, ``root_children()``), selfplay_ref's
``discrete_rule`` / ``continuous_rule``, and ``env_step`` / ``reset_state`` / ``act_draw``; the oracle library has no search rollout.
A population runs net by net with ``Case.net_kw(k)`` (``truth``), as in reanalyse_util.  tests/test_search_rollout_host.py pins the
restatement to ``cpu_selfplay`` on the CPU.

The cases reuse reanalyse_util.CASES' settings and nets at the smallest shapes that reach every code path: 33 games per one-net case
(two full 16-game blocks and a ragged one), 65 for the one-thread kernel, 32 / 64 for the wide nets, three nets of 11 games with
per-net settings and budgets 16 / 9 / 1, the AZG_FORCE_GLOBAL_TREE pair; n_sims <= 16, episodes of 3 to 5 steps, two per game.
``cartpole_falls`` is there so that games end by ``done`` at different steps and park while others play on."""
import functools

import numpy as np

import oracle_lib as O
import reanalyse_util as R
import selfplay_ref as SR

MUTANTS = ("parked_keeps_root", "carry_kept_over_end", "step_restarts_per_episode")
INDEX_BASE = 3 << 30   # run.EVAL_SEARCH_INDEX_BASE
E = 2

CFG = dict(episodes_per_game=E, max_episode_length=4, final_selection="max_visit", deterministic=True, temperature=1.0, agent_epsilon=0.0,
           game_id_base=1000, episode=3, index_base=INDEX_BASE)

# the final-action rule of the cases that do not take the greedy default: every branch of the pick is walked by some case
RULES = {
    "pendulum": dict(agent_epsilon=0.25),
    "cartpole_onpolicy": dict(deterministic=False, temperature=0.5),
    "mcc": dict(final_selection="max_value"),
    "many_children": dict(agent_epsilon=0.25),
    "population": dict(deterministic=False),
}

# cartpole_falls: CartPole, 8 simulations, the sampled rule.  Weight seed and length limit were picked on the CPU among seeds 1 .. 7
# at 30 steps (test_search_rollout_host.py asserts what they are there for).  Found with seed 7: 58 of the 66 episodes end by done, 8
# at the limit, 23 distinct step totals among the 33 games, and the last game finishes at step 54 of the 60 the call may run
FALLS_SEED, FALLS_MAX_LEN = 7, 30


def _cases():
    c = dict(R.CASES)
    cart = R.CASES["cartpole"]
    c["cartpole_falls"] = R.Case(dict(cart.kw, n_sims=8), cart.net, games=33, max_len=FALLS_MAX_LEN,
                                 blob=lambda k, new: O.make_weights(FALLS_SEED, 4, [64, 64], 2, scale=2.0))
    return c


CASES = _cases()


def config(name, **over):
    """The call's settings for case ``name`` (CFG's keys)."""
    case = CASES[name]
    cfg = dict(CFG, max_episode_length=case.max_len, **RULES.get(name, {}))
    if name == "cartpole_falls":
        cfg.update(deterministic=False)
    cfg.update(over)
    assert set(cfg) == set(CFG), cfg
    return cfg


def _rule(cfg):
    return dict(SR.BEGIN, max_episode_length=cfg["max_episode_length"], deterministic=cfg["deterministic"],
                final_selection=cfg["final_selection"], temperature=cfg["temperature"], agent_epsilon=cfg["agent_epsilon"])


# ------------------------------------------------------------------------------------------------ the CPU truth

def cpu_search_rollout(kw, desc, blob, T, cfg, mutant=None):
    """One net's games of a search rollout: ``T`` games (tree ids kw["tree_id_base"] + j, start states of global games
    cfg["game_id_base"] + j) play cfg["episodes_per_game"] episodes each.  Returns a dict: returns / lengths / terminated [T, E], totals
    [T] (the steps each game played), steps (the searches of a call that looks at the count of unfinished games after every step:
    the largest total), roots [T, S] and carry [T] as the call leaves them (parked), and last (``results()`` of the last search).
    mutant: one deliberately wrong variant of the contract (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert set(cfg) == set(CFG), cfg
    b = _rule(cfg)
    o = O.OracleEngine(**dict(kw, n_trees=T))
    o.set_weights(desc, blob)
    env_id, seed, base = kw["env_id"], kw.get("seed", 34), kw.get("tree_id_base", 0)
    cont = kw["mode"] == R._capi.MODE_CONTINUOUS
    S = o.s_env
    n_ep, L, gid, ep0, idx0 = cfg["episodes_per_game"], cfg["max_episode_length"], cfg["game_id_base"], cfg["episode"], cfg["index_base"]

    def reset(j, episode):
        out = np.zeros(4)
        r = O.reset_state(seed, gid + j, ep0 + episode, False, env_id=env_id)
        out[:len(r)] = r
        return out

    state = np.stack([reset(j, 0) for j in range(T)])
    carry = np.zeros(T, np.int32)
    t, ep, totals = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32)
    ret = np.zeros(T)
    returns, lengths, terminated = np.zeros((T, n_ep)), np.zeros((T, n_ep), np.int32), np.zeros((T, n_ep), bool)
    s, last = 0, None
    while (ep < n_ep).any():
        assert s < n_ep * L
        step = idx0 + (s % L if mutant == "step_restarts_per_episode" else s)
        o.set_search_index(step)
        o.search(state[:, :S], carry)
        res = o.results()
        last = {k: np.array(v) for k, v in res.items()}
        child_n, _ = o.root_children()
        for j in range(T):
            if ep[j] >= n_ep:   # parked: searched, and the result ignored
                continue
            nc = int(res["n_children"][j])
            counts, Q = res["counts"][j, :nc], res["Q"][j, :nc]
            acts = res["actions"][j, :nc] if cont else np.arange(nc, dtype=np.float32)
            u01, u, w = O.act_draw(seed, base + j, step)
            if cont:
                pick, _ = SR.continuous_rule(counts, Q, b, u01, w)
            else:
                pick, _, _, _ = SR.discrete_rule(counts, Q, b, u)
            nxt, r, done, _ = O.env_step(env_id, state[j], float(acts[pick]))
            nxt[S:] = 0.0
            ret[j] = ret[j] + r
            t[j] += 1
            totals[j] += 1
            node_n = 0 if cont else max(int(child_n[j, pick]), 0)
            if done or t[j] >= L:
                i = ep[j]
                returns[j, i], lengths[j, i], terminated[j, i] = ret[j], t[j], done
                ret[j], t[j] = 0.0, 0
                ep[j] += 1
                if not (mutant == "parked_keeps_root" and ep[j] == n_ep):
                    nxt = reset(j, int(ep[j]))
                if mutant != "carry_kept_over_end":
                    node_n = 0
            state[j] = nxt
            carry[j] = node_n
        s += 1
    o.close()
    return dict(returns=returns, lengths=lengths, terminated=terminated, totals=totals, steps=int(totals.max()), roots=state[:, :S].copy(),
                carry=carry, last=last)


def _side_by_side(parts):
    out = {}
    for key in ("returns", "lengths", "terminated", "totals", "roots", "carry"):
        out[key] = np.concatenate([p[key] for p in parts])
    out["steps"] = max(p["steps"] for p in parts)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, mutant=None):
    """The truth of case ``name`` under ``config(name)``, net by net, the nets' games side by side in tree order.  Computed once per
    process, read-only.  (``last`` is left out for a population: its nets stop at different steps.)"""
    case, cfg = CASES[name], config(name)
    parts = [cpu_search_rollout(case.net_kw(k), case.desc(), case.blob(k), case.T, cfg, mutant) for k in range(case.nets)]
    out = _side_by_side(parts)
    if case.nets == 1:
        out["last"] = parts[0]["last"]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def same(a, b):
    """Two truths / outputs agree bit for bit on returns, lengths and terminated."""
    return (np.array_equal(R.bits64(a["returns"]), R.bits64(b["returns"])) and np.array_equal(a["lengths"], b["lengths"])
            and np.array_equal(a["terminated"], b["terminated"]))


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(R.bits64(got["returns"]), R.bits64(want["returns"]), err_msg=f"{what}: returns")
    np.testing.assert_array_equal(got["lengths"], want["lengths"], err_msg=f"{what}: lengths")
    np.testing.assert_array_equal(got["terminated"], want["terminated"], err_msg=f"{what}: terminated")
