"""Shared by the per-net simulation budget tests (azg_net_search.n_sims): the three nets' budgets of the matrix, and the expected result
-- K oracle engines, net k CREATED with its own n_sims (and settings) and tree_id_base + k*T -- brought to the population's widths.

An oracle engine created with a smaller n_sims has fewer records per tree and, in continuous mode, a smaller Kmax: its per-child
result columns are filled up with empty slots (net_search_util.EMPTY) and its dumped trees with zero records -- what azg_dump_tree
writes beyond a tree's n_rec -- before the nets are concatenated.  Comparing the padded arrays whole therefore compares every tree's
first n_rec records AND holds the population engine to zeros beyond them."""
import numpy as np

import net_search_util as N
import oracle_lib as O


def budgets(n_sims):
    """Net 0 keeps the capacity, net 1 runs one simulation, net 2 a middle value."""
    return [n_sims, 1, n_sims // 3 + 1]


def with_budgets(settings, sims):
    """settings[k] with net k's budget as its n_sims: the kwargs its oracle engine is created with (net_search_util.oracle_nets)."""
    return [dict(s, n_sims=int(n)) for s, n in zip(settings, sims)]


def _pad_records(a, R):
    """[T, R_k] -> [T, R]: zero records behind the engine's own."""
    if a.ndim < 2 or a.shape[1] == R:
        return a
    assert a.shape[1] < R, (a.shape, R)
    out = np.zeros((a.shape[0], R) + a.shape[2:], dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def oracle_nets(kw, desc, blobs, roots, carry, sidx, settings, sims, width=None, records=None):
    """(results, dump, (child_n, child_state)) of K oracle engines concatenated -- net k created with kw overridden by settings[k],
    n_sims = sims[k] and tree_id_base + k*T.  width: the population engine's Kmax (None: the largest of the K engines'); records: its
    records per tree (None: those of an oracle engine created with kw itself, the capacity)."""
    nets = len(blobs)
    T = kw["n_trees"] // nets
    if records is None:
        o = O.OracleEngine(**dict(kw, n_trees=T))
        records = o.max_records
        if width is None and kw["mode"] == 1:
            width = o.kmax
        o.close()
    parts = []
    for k in range(nets):
        own = dict(kw, n_trees=T, tree_id_base=kw.get("tree_id_base", 0) + k * T, **dict(settings[k], n_sims=int(sims[k])))
        o = O.OracleEngine(**own)
        o.set_weights(desc, blobs[k])
        o.set_search_index(sidx)
        sl = slice(k * T, (k + 1) * T)
        o.search(roots[sl], None if carry is None else carry[sl])
        res, dump, (cn, cs) = dict(o.results()), dict(o.dump_tree()), o.root_children()
        w = o.kmax if width is None else width
        assert o.kmax <= w and o.max_records <= records, (k, o.kmax, w, o.max_records, records)
        for key in ("actions", "counts", "Q"):
            res[key] = N._widen(res[key], w, N.EMPTY[key])
        dump = {key: _pad_records(a, records) for key, a in dump.items()}
        parts.append((res, dump, (N._widen(cn, w, N.EMPTY["child_n"]), N._widen(cs, w, N.EMPTY["child_state"]))))
        o.close()
    res = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    dump = {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
    return res, dump, (np.concatenate([p[2][0] for p in parts]), np.concatenate([p[2][1] for p in parts]))


def assert_root_counts(got, sims, T, carry=None, what=""):
    """Every tree ran its own net's budget: each trace passes through exactly one of the root's child edges, so the root's child counts
    sum to the budget, and the root's own count is the budget plus what it carried (discrete mode; continuous roots start fresh)."""
    res, dump, _ = got
    for k, n in enumerate(sims):
        sl = slice(k * T, (k + 1) * T)
        c = 0 if carry is None else carry[sl]
        np.testing.assert_array_equal(res["counts"][sl].sum(axis=1), np.full(T, n), err_msg=f"{what} net {k}: root child counts")
        np.testing.assert_array_equal(dump["node_n"][sl, 0], c + n, err_msg=f"{what} net {k}: root count")
