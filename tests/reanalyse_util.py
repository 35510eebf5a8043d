"""Reanalysis of the device replay ring (azg_selfplay_reanalyse, include/azgym_reanalyse.h): the cases of tests/test_reanalyse.py and
the CPU truth of a reanalysed row.  TEST INFRASTRUCTURE ONLY.

The expected row of a reanalysis is MCTS.return_results of an ORDINARY oracle search -- ``OracleEngine.search`` of the kept state under
the reanalysis' search index, no carried count -- put into a row by selfplay_ref's column rule (``value_target`` and the columns of
``cpu_selfplay``); the oracle library has no reanalysis entry point.  tests/test_reanalyse_host.py pins that builder to the oracle's
self-play on the CPU."""
import functools

import numpy as np

import oracle_lib as O
import selfplay_edges as SE
import selfplay_ref as SR
from alphazero_gym_amd import _capi

STEPS = 5          # steps a case plays at most before / between its reanalyses (checks c and d: 4 and 6)
NEW_INDEX = 1 << 31   # run.REANALYSE_INDEX_BASE: the first search index run.py hands to a reanalysis


class Case:
    """kw: the engine's settings without n_trees; net: (in_dim, hidden, n_dist, activation, mixture components); games: all games of
    the engine (nets * games per net); nets / net_settings / net_rollouts / wide_table: a population and its per-net table;
    blob(k, new): net k's weights, ``new``: the ones loaded before a reanalysis."""

    def __init__(self, kw, net, games=33, max_len=4, nets=1, net_settings=None, net_rollouts=None, wide_table=False, slope=False, blob=None,
                 env=None):
        self.kw, self.net, self.games, self.max_len, self.nets = dict(kw), net, games, max_len, nets
        self.net_settings, self.net_rollouts, self.wide_table, self.slope = net_settings, net_rollouts, wide_table, slope
        self._blob = blob
        self.env = dict(env or {})   # environment variables the engine is created under
        assert games % nets == 0

    @property
    def cont(self):
        return self.kw["mode"] == _capi.MODE_CONTINUOUS

    @property
    def T(self):
        return self.games // self.nets

    @property
    def n_sims(self):
        return self.kw["n_sims"]

    def desc(self):
        in_dim, hidden, n_dist, act, ncomp = self.net
        return _capi.make_desc(in_dim, list(hidden), n_dist, act, num_components=ncomp)

    def blob(self, k=0, new=False):
        if self._blob is not None:
            return self._blob(k, new)
        in_dim, hidden, n_dist, _, _ = self.net
        return O.make_weights((500 if new else 3) + 7 * k, in_dim, list(hidden), n_dist, scale=2.0)

    def blobs(self, new=False):
        return [self.blob(k, new) for k in range(self.nets)]

    def net_kw(self, k):
        """The settings of the one-net engine that computes net k's trees: its own tree ids, table entry and budget."""
        kw = dict(self.kw, tree_id_base=self.kw.get("tree_id_base", 0) + k * self.T)
        if self.net_settings is not None:
            s = self.net_settings[k]
            kw.update(c_uct=s["c_uct"], gamma=s["gamma"], epsilon=s["epsilon"])
            if self.cont:
                kw.update(c_pw=s["c_pw"], kappa=s["kappa"])
        if self.net_rollouts is not None:
            kw["n_sims"] = self.net_rollouts[k]
        return kw

    def budget(self):
        """[games]: the simulations a search of each game's tree runs."""
        per = self.net_rollouts if self.net_rollouts is not None else [self.n_sims] * self.nets
        return np.repeat(np.asarray(per, np.int64), self.T)

    def first_roots(self, e):
        if not self.slope:
            return None
        from test_selfplay_device import slope_roots
        return slope_roots(e)


def _settings(c_uct):
    return dict(c_uct=c_uct, gamma=0.97, epsilon=0.0, c_pw=1.0, kappa=0.5)


def _cases():
    pend = dict(env_id=2, mode=1, n_sims=16, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=11, tree_id_base=5)
    cart = dict(env_id=0, mode=0, n_sims=16, c_uct=20.0, gamma=0.97, num_actions=2, seed=12)
    c = {}
    c["pendulum"] = Case(pend, (3, [64, 64], 2, "elu", 0))
    c["cartpole"] = Case(cart, (4, [64, 64], 2, "relu", 0), max_len=3)
    c["cartpole_onpolicy"] = Case(dict(cart, v_target="on_policy"), (4, [64, 64], 2, "relu", 0), max_len=3)
    c["acrobot"] = Case(dict(env_id=5, mode=0, n_sims=16, c_uct=1.0, gamma=0.99, num_actions=3, seed=13, tree_id_base=2), (6, [64, 64], 3, "relu", 0))
    c["mcc"] = Case(dict(env_id=4, mode=1, n_sims=16, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=14, tree_id_base=9, action_bound=1.0),
                    (2, [64, 64], 2, "elu", 0), max_len=5, slope=True)
    c["gmm"] = Case(dict(pend, seed=15), (3, [64, 64], 6, "elu", 2))
    # more than 16 root children (selfplay_kernel's side of the switch, the reanalysis' one-thread-per-tree kernel): the settings and the
    # net of selfplay_edges' many_children_* cases
    many = SE.CASES["many_children_visit_ties_first"]
    assert many.n_games == 65 and many.n_sims == 16
    g = SE.GAMES[many.game]
    c["many_children"] = Case(many.kw(), (g["in_dim"], list(SE.NARROW), 2, SE.ACT, 0), games=many.n_games, max_len=3,
                              blob=lambda k, new: (SE.E.net_blob(g["in_dim"], list(SE.NARROW), 2, value_bias=0.5, dist_bias=[0.4, 0.1]) if new
                                                   else many.blob(SE.NARROW)))
    # one hidden layer of 512: the wide one-launch kernel; two: the team kernel / the per-layer launches
    c["wide"] = Case(dict(pend, n_sims=8, seed=16), (3, [512], 2, "elu", 0), games=32)
    c["wide_team"] = Case(dict(pend, n_sims=8, seed=17), (3, [512, 512], 2, "elu", 0), games=32)
    c["population"] = Case(cart, (4, [64, 64], 2, "relu", 0), max_len=3, nets=3, net_settings=[_settings(x) for x in (20.0, 1.5, 0.3)],
                           net_rollouts=[16, 9, 1])
    c["population_wide"] = Case(dict(pend, n_sims=8, seed=18), (3, [512], 2, "elu", 0), games=64, nets=2)
    c["population_wide_team"] = Case(dict(pend, n_sims=8, seed=19), (3, [512, 512], 2, "elu", 0), games=64, nets=2)
    for name in ("pendulum", "cartpole"):
        base = c[name]
        c[name + "_global_tree"] = Case(base.kw, base.net, games=base.games, max_len=base.max_len, env={"AZG_FORCE_GLOBAL_TREE": "1"})
    return c


CASES = _cases()


# ------------------------------------------------------------------------------------------------ the CPU truth

def oracle_search(case_kw, desc, blobs, roots, search_index):
    """One ordinary oracle search of ``roots`` [G, S] under ``search_index``, fresh roots: ``results()``.  ``case_kw`` / ``blobs``: one
    engine's settings and weights, or lists of them, one per net of a population (net k: the block k*T .. k*T+T-1 of the roots, an
    engine of its own with its tree ids, settings and budget); the nets' results are put side by side in game order."""
    kws, blobs = (case_kw, blobs) if isinstance(case_kw, (list, tuple)) else ([case_kw], [blobs])
    roots = np.ascontiguousarray(roots, np.float64)
    T = roots.shape[0] // len(kws)
    parts = []
    for k, (kw, blob) in enumerate(zip(kws, blobs)):
        o = O.OracleEngine(**dict(kw, n_trees=T))
        o.set_weights(desc, blob)
        o.set_search_index(search_index)
        o.search(roots[k * T:(k + 1) * T])
        parts.append({key: np.array(v) for key, v in o.results().items()})
        o.close()
    K = max(p["counts"].shape[1] for p in parts)

    def pad(a):   # (a net with a smaller budget may reach fewer children: its remaining columns are empty slots)
        return a if a.ndim == 1 or a.shape[1] == K else np.concatenate([a, np.zeros((a.shape[0], K - a.shape[1]), a.dtype)], 1)
    return {key: np.concatenate([pad(p[key]) for p in parts]) for key in parts[0]}


def expected_rows(kw, desc, blob, states, slots, search_index, old_rows, results=None):
    """The rows (slots[t], t) after a reanalysis under ``search_index``: [G, row_len] float32.  states [steps, G, S]: the kept states;
    old_rows [steps, G, row_len]: the ring before (its observation columns stay).  ``results`` (optional dict): filled with the oracle's
    ``results()`` of the search."""
    kw0 = kw[0] if isinstance(kw, (list, tuple)) else kw
    cont = kw0["mode"] == _capi.MODE_CONTINUOUS
    on_policy = kw0.get("v_target", "off_policy") == "on_policy"
    states, old_rows = np.asarray(states), np.asarray(old_rows)
    G = states.shape[1]
    slots = np.broadcast_to(np.asarray(slots, np.int64), (G,))
    res = oracle_search(kw, desc, blob, states[slots, np.arange(G)], search_index)
    if results is not None:
        results.update(res)
    row_len = old_rows.shape[2]
    K = res["counts"].shape[1]
    So = row_len - 3 * K - 1
    rows = np.zeros((G, row_len), np.float32)
    for i in range(G):
        nc = int(res["n_children"][i])
        counts, Q = res["counts"][i, :nc], res["Q"][i, :nc]
        acts = res["actions"][i, :nc] if cont else np.arange(nc, dtype=np.float32)
        row = rows[i]
        row[:So] = old_rows[slots[i], i, :So]
        row[So:So + nc] = acts
        row[So + K:So + K + nc] = counts
        row[So + 2 * K:So + 2 * K + nc] = Q
        row[So + 3 * K] = SR.value_target(counts, Q, on_policy, cont)
    return rows


@functools.lru_cache(maxsize=None)
def reference(name, steps=STEPS + 1):
    """The restatement's self-play of case ``name`` (selfplay_ref.cpu_selfplay, net by net): rows [steps, G, row_len], the states every
    step's search started from [steps, G, S] and the counts it carried [steps, G].  Computed once per process, read-only.  (The
    first ``s`` steps of a run are the run of ``s`` steps.)"""
    case = CASES[name]
    rows, states, carry = [], [], []
    for k in range(case.nets):
        kw = case.net_kw(k)
        first = None
        if case.slope:
            o = O.OracleEngine(**dict(kw, n_trees=case.T))
            first = case.first_roots(o)
            o.close()
        trace = []
        out = SR.cpu_selfplay(kw, case.desc(), case.blob(k), case.T, steps, begin=dict(max_episode_length=case.max_len), first_roots=first,
                              trace=trace)
        rows.append(out["rows"].reshape(steps, case.T, -1))
        st, ci = np.zeros((steps, case.T, len(trace[0]["state"]))), np.zeros((steps, case.T), np.int64)
        for r in trace:
            st[r["step"], r["game"]] = r["state"]
            ci[r["step"], r["game"]] = r["carry_in"]
        states.append(st)
        carry.append(ci)
    out = dict(rows=np.concatenate(rows, 1), states=np.concatenate(states, 1), carry_in=np.concatenate(carry, 1))
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the engine under test

def make_engine(cls, case, new=False):
    e = cls(**dict(case.kw, n_trees=case.games))
    if case.nets > 1:
        e.set_population(case.nets)
    set_weights(e, case, new)
    if case.net_settings is not None:
        e.set_net_search(case.net_settings, wide=case.wide_table, n_sims=case.net_rollouts)
    return e


def set_weights(e, case, new=False):
    if case.nets == 1:
        e.set_weights(case.desc(), case.blob(0, new))
    else:
        for k in range(case.nets):
            e.set_net_weights(k, case.desc(), case.blob(k, new))


def begin(e, case, capacity, fifo=False, keep=True):
    start = e.selfplay_begin if case.nets == 1 else e.population_selfplay_begin
    start(case.max_len, False, capacity_steps=capacity, fifo=fifo)
    if keep:
        e.selfplay_keep_states(True)
    first = case.first_roots(e)
    if first is not None:
        e.upload_roots(first)


def ring(e, case):
    """The stored rows as [steps, G, row_len]."""
    rows = e.selfplay_rows(clear=False)
    return rows.reshape(-1, case.games, rows.shape[1])


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
