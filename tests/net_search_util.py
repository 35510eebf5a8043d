"""Shared by the per-net search settings tests (azg_set_net_search): the three nets' settings of the matrix, and the expected result --
K oracle engines, net k created with its OWN settings and tree_id_base + k*T -- brought to the population's result width."""
import math

import numpy as np

import oracle_lib as O
import parity_util as P

NARROW_PW = (0.6, 0.45)   # net 1's widening in continuous mode: never entitles a node to more children than any row's own pair


def matrix_rows():
    """The rows of parity_util.CONFIGS a population with per-net settings runs: padded hidden width <= 256."""
    return [ci for ci, cfg in enumerate(P.CONFIGS) if max(cfg[2]) <= 256]


def shared_settings(cfg):
    """The row's own five settings, complete (the engine's defaults where the row names none)."""
    _, mode, _, _, _, extra, _, _ = P.split_config(cfg)
    s = dict(c_uct=extra["c_uct"], gamma=extra["gamma"], epsilon=extra.get("epsilon", 0.0))
    if mode == 1:
        s.update(c_pw=extra.get("c_pw", 1.0), kappa=extra.get("kappa", 0.5))
    return s


# Rows where the rule below leaves a net with the trees it has under net 0's settings, found on the oracle
# (test_population_net_search_host.py), and what that net takes instead.  Row 1 (c_pw 2.5, kappa 0.7, 64 simulations: a node is
# entitled to a new child at nearly every visit, so selection among children hardly ever decides anything) already has gamma 0.97, and no
# c_uct multiplier from 0.01 to 100 changes more than 2 of net 2's 19 trees: net 2 takes gamma 0.9 there, still c_uct x 0.25.
OVERRIDES = {1: {2: dict(gamma=0.9)}}


def net_settings(cfg):
    """Net 0: the row's settings.  Net 1: c_uct x 4, gamma 0.9 if the row's is 1.0 else 1.0, epsilon 0.25 if the row's is 0 else 0, and in
    continuous mode the narrow widening pair.  Net 2: c_uct x 0.25 and gamma 0.97.  So one launch always mixes gamma == 1 (the closed-form
    backup) with the general chain, and in discrete mode cached selections with epsilon-greedy descents."""
    s0 = shared_settings(cfg)
    s1 = dict(s0, c_uct=s0["c_uct"] * 4.0, gamma=0.9 if s0["gamma"] == 1.0 else 1.0, epsilon=0.25 if s0["epsilon"] == 0.0 else 0.0)
    if "c_pw" in s0:
        s1.update(c_pw=NARROW_PW[0], kappa=NARROW_PW[1])
    s2 = dict(s0, c_uct=s0["c_uct"] * 0.25, gamma=0.97)
    out = [s0, s1, s2]
    for k, over in OVERRIDES.get(P.CONFIGS.index(cfg), {}).items():
        out[k].update(over)
    return out


def full(s):
    """All five keys (Engine.set_net_search wants them; discrete mode ignores the widening pair)."""
    return dict(dict(c_pw=1.0, kappa=0.5), **s)


def kmax_of(s, n_sims):
    """The most children a node reaches within n_sims simulations under s's widening (the engine's Kmax; 0: discrete, no widening)."""
    if "c_pw" not in s:
        return 0
    return max([1] + [math.ceil(s["c_pw"] * math.pow(n + 1, s["kappa"])) for n in range(n_sims)])


# what return_results / root_children hold in the slot of a child that does not exist
EMPTY = {"actions": 0.0, "counts": 0, "Q": 0.0, "child_n": -1, "child_state": 0.0}


def _widen(a, width, fill):
    if a.ndim < 2 or a.shape[1] == width:
        return a
    out = np.full((a.shape[0], width) + a.shape[2:], fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def oracle_nets(kw, desc, blobs, roots, carry, sidx, settings, width=None):
    """(results, dump, (child_n, child_state)) of K oracle engines concatenated -- net k created with kw overridden by settings[k] and
    tree_id_base + k*T.  A net whose own Kmax is below `width` (the population engine's) has its per-child arrays filled up with EMPTY:
    its first Kmax_k columns are its own engine's, the others must be empty slots."""
    nets = len(blobs)
    T = kw["n_trees"] // nets
    parts = []
    for k in range(nets):
        o = O.OracleEngine(**dict(kw, n_trees=T, tree_id_base=kw.get("tree_id_base", 0) + k * T, **settings[k]))
        o.set_weights(desc, blobs[k])
        o.set_search_index(sidx)
        sl = slice(k * T, (k + 1) * T)
        o.search(roots[sl], None if carry is None else carry[sl])
        res, dump, (cn, cs) = dict(o.results()), dict(o.dump_tree()), o.root_children()
        w = o.kmax if width is None else width
        assert o.kmax <= w, (k, o.kmax, w)
        for key in ("actions", "counts", "Q"):
            res[key] = _widen(res[key], w, EMPTY[key])
        parts.append((res, dump, (_widen(cn, w, EMPTY["child_n"]), _widen(cs, w, EMPTY["child_state"]))))
        o.close()
    res = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    dump = {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
    return res, dump, (np.concatenate([p[2][0] for p in parts]), np.concatenate([p[2][1] for p in parts]))
