"""GPU (-m gpu): the eight-wave / 16-tree continuous search kernels finish a leaf in two halves -- the walking waves take its value and
back it up, a non-walking wave computes its policy (mu, sigma) and hands it over through an LDS mailbox (tree_phases.cuh: PolicyMailbox,
policy_finish_helper).  Everything a search leaves behind must stay bit for bit what the CPU oracle computes.

Shapes: the 2x256 ELU Pendulum-v1 network; 16 trees (one full workgroup) and 40 (the last workgroup has 8 live columns: helper lanes
beside padding trees); 1, 17 and 48 simulations (none, one and three blocks of 16 widening draws beyond the root's); two searches on one
engine (search index, mailbox flags from a used state); populations of 2 x 16 and 2 x 5 trees (the helper reads its net's head bias).
Default c_pw / kappa: a fresh node widens at its first visit, so a trace that reaches the leaf of its own step takes that leaf's policy
from the mailbox -- asserted from the dumped trees.  Every case asserts from search_info() that the persistent eight-wave form with
16-tree tiles and LDS trees ran."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from alphazero_gym_amd import _capi, synthetic

pytestmark = pytest.mark.gpu

IN_DIM, HIDDEN, N_DIST, ACT = 3, [256, 256], 2, "elu"
BASE = 11   # tree_id_base


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _kw(n_trees, n_sims):
    # (c_pw, kappa: the engine's defaults)
    return dict(env_id=2, mode=1, n_trees=n_trees, n_sims=n_sims, c_uct=0.05, gamma=1.0, seed=34, tree_id_base=BASE)


def _desc():
    return _capi.make_desc(IN_DIM, HIDDEN, N_DIST, ACT)


def _blob(wseed):
    return synthetic.make_weights(wseed, IN_DIM, HIDDEN, N_DIST)


def _collect(e):
    return dict(e.results()), dict(e.dump_tree())


def _run(e, roots, indices):
    """One search per search index on the same engine; what each left behind."""
    out = []
    for sidx in indices:
        e.set_search_index(sidx)
        e.search(roots)
        out.append(_collect(e))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(n_trees, n_sims, wseed, base, indices):
    o = O.OracleEngine(**dict(_kw(n_trees, n_sims), tree_id_base=base))
    o.set_weights(_desc(), _blob(wseed))
    roots = o.synthetic_roots()
    out = _run(o, roots, indices)
    o.close()
    return roots, out


def _assert_same(got, want, what):
    for (rg, dg), (rw, dw) in zip(got, want):
        assert set(rg) == set(rw) and set(dg) == set(dw)
        for name, a, b in [("results " + k, rg[k], rw[k]) for k in rw] + [("dump " + k, dg[k], dw[k]) for k in dw]:
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
            rows = [i for i in range(a.shape[0]) if a[i].tobytes() != b[i].tobytes()]
            np.testing.assert_array_equal(a, b, err_msg=f"{what} {name}: trees {rows[:8]} differ")


def _assert_form(info, spec):
    assert info["kernel_form"] == "persistent" and info["waves"] == 8 and info["groups"] == 1 and info["tile_trees"] == 16, info
    assert info["tree_storage"] == "lds8" and info["spec"] == spec, info


def _fresh_leaf_widened(dump):
    """Trees with a node whose first child is the very next record: the node was widened by the trace that followed its own
    evaluation, i.e. in the step whose leaf it was."""
    hits = 0
    for t in range(dump["n_records"].shape[0]):
        n = int(dump["n_records"][t])
        par = dump["parent"][t, :n]
        j = np.arange(1, n - 1)
        hits += bool((par[j + 1] == j).any())
    return hits


@pytest.mark.parametrize("n_sims", [1, 17, 48])
@pytest.mark.parametrize("n_trees", [16, 40])
def test_bit_exact_vs_oracle(native, n_trees, n_sims):
    roots, want = _oracle(n_trees, n_sims, 34, BASE, (0,))
    e = native.HipEngine(**_kw(n_trees, n_sims))
    e.set_weights(_desc(), _blob(34))
    got = _run(e, roots, (0,))
    info = e.search_info()
    e.close()
    _assert_form(info, 1)
    _assert_same(got, want, f"{n_trees} trees x {n_sims} sims")
    if n_sims == 48:
        hits = _fresh_leaf_widened(got[0][1])
        print(f"{n_trees} trees: {hits} widened a leaf in the step that evaluated it")
        assert hits >= 1


def test_general_kernel(native, monkeypatch):
    """The SPEC = 0 form of the same kernel (AZG_NO_SPEC=1)."""
    monkeypatch.setenv("AZG_NO_SPEC", "1")
    roots, want = _oracle(40, 48, 34, BASE, (0,))
    e = native.HipEngine(**_kw(40, 48))
    e.set_weights(_desc(), _blob(34))
    got = _run(e, roots, (0,))
    info = e.search_info()
    e.close()
    _assert_form(info, 0)
    _assert_same(got, want, "general kernel")
    assert _fresh_leaf_widened(got[0][1]) >= 1


def test_two_searches_on_one_engine(native):
    """Search indices 3 and 4, one after the other: the index enters the widening draws; the second launch starts from LDS and cold
    records the first one used."""
    roots, want = _oracle(40, 48, 34, BASE, (3, 4))
    e = native.HipEngine(**_kw(40, 48))
    e.set_weights(_desc(), _blob(34))
    got = _run(e, roots, (3, 4))
    info = e.search_info()
    e.close()
    _assert_form(info, 1)
    _assert_same(got, want, "two searches")
    assert any(got[0][1][k].tobytes() != got[1][1][k].tobytes() for k in got[0][1])   # (the two searches differ)


@pytest.mark.parametrize("T", [16, 5])
def test_population_equals_single_net_engines(native, T):
    """K = 2 nets x T trees in one launch against two single-net engines (net k: its own weights, tree_id_base + k*T), and against
    the oracle."""
    n_sims, seeds = 48, (34, 35)
    o = O.OracleEngine(**_kw(2 * T, n_sims))
    roots = o.synthetic_roots()
    o.close()
    e = native.HipEngine(**_kw(2 * T, n_sims))
    e.set_population(2)
    for k in range(2):
        e.set_net_weights(k, _desc(), _blob(seeds[k]))
    got = _run(e, roots, (2,))
    info = e.search_info()
    e.close()
    _assert_form(info, 1)
    singles, oracles = [], []
    for k in range(2):
        kw = dict(_kw(T, n_sims), tree_id_base=BASE + k * T)
        for cls, sink in ((native.HipEngine, singles), (O.OracleEngine, oracles)):
            s = cls(**kw)
            s.set_weights(_desc(), _blob(seeds[k]))
            sink.append(_run(s, roots[k * T:(k + 1) * T], (2,))[0])
            if cls is native.HipEngine:
                _assert_form(s.search_info(), 1)
            s.close()
    for parts, what in ((singles, "single-net engines"), (oracles, "oracle")):
        want = [tuple({k: np.concatenate([p[i][k] for p in parts]) for k in parts[0][i]} for i in range(2))]
        _assert_same(got, want, f"population 2 x {T} against {what}")
