"""CPU truth of azg_policy_rollout (include/azgym_eval.h), composed from the oracle's existing exports.  TEST INFRASTRUCTURE ONLY.

The network is a single-net ``OracleEngine``'s ``mlp_eval`` (``raw``: the head outputs; ``dist``: the float32 softmax / mu, sigma /
mixture parameters the heads derive from them), the draws are ``act_draw`` / ``normal`` / ``gmm_u``, the squashing function is
``sample_action``, and ``env_step`` / ``reset_state`` / the oracle's ``azo_env_obs`` (prototype set up by ``oracle_lib.lib()``) are
the game.  The action rules are restated here in numpy."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from alphazero_gym_amd import _capi

GMM_MAXC = 5


def _obs(env_id, state, n_obs):
    out = np.zeros(8, np.float32)
    O.lib().azo_env_obs(env_id, _capi._ptr(state, C.c_double), _capi._ptr(out, C.c_float))
    return out[:n_obs].copy()


def _action(kw, ncomp, rule, raw, dist, seed, gid, t, rec=None):
    """The action of one game from its head outputs at step t.  rec (a dict, optional) receives the draws used: ``u`` (the float64
    draw of the discrete walk, or the float32 draw that picks a mixture's component), ``eps`` and, with a mixture head, ``comp``."""
    rec = {} if rec is None else rec
    sample = rule == "sample"
    if kw["mode"] == _capi.MODE_DISCRETE:
        logits = raw[1:]
        if not sample:
            return float(int(np.argmax(logits)))   # (first index on ties)
        u = rec["u"] = O.act_draw(seed, gid, t)[1]
        c = 0.0
        for a, p in enumerate(dist):
            c = c + float(p)   # float64 sum of the float32 probabilities, in index order
            if u < c:
                return float(a)
        return float(len(dist) - 1)
    bound = kw.get("action_bound", 2.0)
    if ncomp >= 2:
        mu, sigma, cum = dist[:ncomp], dist[ncomp:2 * ncomp], dist[2 * ncomp:3 * ncomp]
        if sample:
            u = rec["u"] = np.float32(O.gmm_u(seed, gid, t, 0))
            comp = ncomp - 1
            for i in range(ncomp):
                if u < cum[i]:
                    comp = i
                    break
        else:
            comp = int(np.argmax(raw[1 + 2 * ncomp:1 + 3 * ncomp]))
        m, s = mu[comp], sigma[comp]
        rec["comp"] = comp
    else:
        m, s = dist[0], dist[1]
    eps = rec["eps"] = O.normal(seed, gid, t, 0) if sample else 0.0
    return float(O.sample_action(m, s, eps, bound))


def cpu_rollout(kw, desc, blob, G, max_len, rule, game_id_base, episode, trace=None):
    """One net's G episodes: dict of returns [G] float64, lengths, terminated, first_value.
    trace (a list, optional) receives one dict per game and step, in step order: ``game``, ``t``, ``raw`` (the head outputs), ``dist``
    (what the heads derive from them), the draws used (``u`` / ``eps`` / ``comp``, see _action), ``action``, ``state`` (before the
    step), ``next_state``, ``reward`` and ``done``."""
    o = O.OracleEngine(**dict(kw, n_trees=1, tree_id_base=0))
    o.set_weights(desc, blob)
    env_id, seed, n_obs = kw["env_id"], kw.get("seed", 34), o.s_obs
    ncomp = int(desc.num_components)
    states = np.zeros((G, 4))
    for j in range(G):
        r = O.reset_state(seed, game_id_base + j, episode, False, env_id=env_id)
        states[j, :len(r)] = r
    returns, lengths = np.zeros(G), np.zeros(G, np.int32)
    terminated, first_value = np.zeros(G, bool), np.zeros(G, np.float32)
    live = list(range(G))
    t = 0
    while live:
        obs = np.stack([_obs(env_id, states[j], n_obs) for j in live])
        value, dist, raw = o.mlp_eval(obs)
        nxt_live = []
        for i, j in enumerate(live):
            if t == 0:
                first_value[j] = raw[i, 0]
            rec = {}
            a = _action(kw, ncomp, rule, raw[i], dist[i], seed, game_id_base + j, t, rec)
            nxt, r, done, _ = O.env_step(env_id, states[j], a)
            if o.s_env < 4:
                nxt[o.s_env:] = 0.0
            if trace is not None:
                trace.append(dict(rec, game=j, t=t, raw=raw[i].copy(), dist=dist[i].copy(), action=np.float32(a), state=states[j].copy(),
                                  next_state=nxt.copy(), reward=r, done=done))
            states[j] = nxt
            returns[j] = returns[j] + r
            lengths[j] = t + 1
            if done or t + 1 >= max_len:
                terminated[j] = done
            else:
                nxt_live.append(j)
        live = nxt_live
        t += 1
    o.close()
    return {"returns": returns, "lengths": lengths, "terminated": terminated, "first_value": first_value}


# name: engine kwargs, network (in_dim, hidden, n_dist, activation, mixture components, LayerNorm)
GAMES = {
    "cartpole": dict(env_id=0, mode=0, num_actions=2, n_sims=4, c_uct=1.0, gamma=1.0, seed=41),
    "pendulum_v0": dict(env_id=1, mode=1, n_sims=4, c_uct=0.05, gamma=1.0, seed=42),
    "pendulum_v1": dict(env_id=2, mode=1, n_sims=4, c_uct=0.05, gamma=1.0, seed=43),
    "mountaincar": dict(env_id=3, mode=0, num_actions=3, n_sims=4, c_uct=1.0, gamma=1.0, seed=44),
    "mcc": dict(env_id=4, mode=1, n_sims=4, c_uct=0.05, gamma=1.0, action_bound=1.0, seed=45),
    "acrobot": dict(env_id=5, mode=0, num_actions=3, n_sims=4, c_uct=1.0, gamma=1.0, seed=46),
}
IN_DIM = {"cartpole": 4, "pendulum_v0": 3, "pendulum_v1": 3, "mountaincar": 2, "mcc": 2, "acrobot": 6}


def net_desc(game, hidden, head, act, layernorm=False):
    """(desc, n_dist) of a net for ``game``: head "discrete", "normal" or "gmm2"."""
    n_dist = GAMES[game].get("num_actions", 0) if head == "discrete" else (2 if head == "normal" else 6)
    return _capi.make_desc(IN_DIM[game], list(hidden), n_dist, act, num_components=2 if head == "gmm2" else 0, layernorm=layernorm)


def net_blob(game, hidden, head, layernorm, seed, scale=1.0):
    n_dist = GAMES[game].get("num_actions", 0) if head == "discrete" else (2 if head == "normal" else 6)
    blob = O.make_weights(seed, IN_DIM[game], list(hidden), n_dist, scale=scale)
    return O.add_layernorm(blob, IN_DIM[game], list(hidden), n_dist, seed + 1) if layernorm else blob


@functools.lru_cache(maxsize=None)
def reference(game, hidden, head, act, layernorm, wseed, scale, G, max_len, rule, game_id_base, episode):
    """cpu_rollout of the net (game, hidden, head, act, layernorm) with weights ``wseed``: computed once, shared, read-only."""
    out = cpu_rollout(GAMES[game], net_desc(game, hidden, head, act, layernorm), net_blob(game, hidden, head, layernorm, wseed, scale),
                      G, max_len, rule, game_id_base, episode)
    for v in out.values():
        v.setflags(write=False)
    return out
