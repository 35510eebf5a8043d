"""GPU (-m gpu): the HIP search against the CPU oracle on continuous trees deeper than the 16 levels a tree's lanes hold, bit for bit.

Every other continuous parity test runs c_pw >= 0.5 with kappa >= 0.3: trees of 3 or 4 levels, whatever the number of simulations.  The deep
continuous backup has code of its own that those never reach -- backup_path's travelling return (`else` arm) and its float32 first
product, the hand-over of the 16th return and of the shallowest record's parent, backup_from<CONT> with the widen-at-next-visit
bits, the path slots wrapping (slot 0, the root's, is overwritten at depth 16) in the scored descent, the deferred-expansion and
helper-wave forms of the 2x256 kernel, the lock-step and team kernels' tree phase.  The cases (tests/deep_paths.py) use two narrow
widening laws: CHAIN (kappa 0: one child per node, a path of n_sims levels, Kmax = 1) and NARROW (c_pw 0.15: branching, 45 to 48
levels).  What each case contains is asserted on the oracle's run alone in tests/test_deep_paths_host.py (CPU), where the oracle's
backup is also replayed in float64 numpy; here the device must reproduce that run: results, every record, the root's children, the
root evaluation."""
import numpy as np
import pytest

import deep_paths as D
import edge_values as E
import net_search_util as N
import oracle_lib as O
import parity_util as P
from selfplay_ref import assert_stats_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _force(monkeypatch, form):
    if form != "default":
        monkeypatch.setenv(*P.VARIANT_ENV[form])


def _assert_form(cid, form, info):
    """search_info names the kernel form the case is there for."""
    shape, law, n_sims, opts = D.CASES[cid]
    what = (cid, form, info)
    hidden = D.SHAPES[shape]["hidden"]
    if max(hidden) <= 256:
        assert info["kernel_form"] == "persistent" and info["kernel_name"].startswith("search_kernel<"), what
        assert info["tree_storage"] == D.expected_storage(shape, law, n_sims, form), what
        assert info["max_children"] == D.kmax_of(law, n_sims), what
    if shape == "p64":
        half = info["tree_storage"] == "lds8" and form not in ("tile16", "stream_weights")
        assert info["tile_trees"] == (8 if half else 16), what      # 37 trees: half-filled tiles (register-resident nets, 8-bit ids)
        assert info["spec"] == (1 if form == "tile16" else 0), what                            # (the specialised kernels: full tiles)
        assert (" 64, 0," in info["kernel_name"]) == (form == "stream_weights"), what          # no layer in registers
    if shape in ("p256", "mcc256"):
        assert info["waves"] == (4 if form in ("waves4", "global_tree") else 8), what
        assert info["groups"] == (2 if form == "groups2" else 1), what
        assert info["spec"] == (0 if form in ("no_spec", "global_tree") else 1), what
    if shape == "ln100":
        assert " 128, 0," in info["kernel_name"], what                                         # LayerNorm: weights streamed
    if shape == "gmm128":
        assert ", true," in info["kernel_name"], what                                          # the mixture head's kernel
    if max(hidden) >= 512:
        if form == "persistent":
            assert info["kernel_form"] == "persistent" and f" {max(hidden)}, 0," in info["kernel_name"], what
        elif form == "launches":
            assert info["kernel_form"] == "per_layer" and info["team_fallbacks"] == 0, what
        else:
            # 32 trees: the team kernel's workgroups are all resident, so it must not have handed over to the per-layer launches
            assert info["kernel_form"] == "team" and info["team_fallbacks"] == 0, what
            if shape == "p1024":
                assert info["spec"] == (0 if form == "no_spec" else 1), what


@pytest.mark.parametrize("cid,form", [pytest.param(*c[1:], id=c[0]) for c in D.device_cases()])
def test_deep_continuous_bit_exact_vs_oracle(native, cid, form, monkeypatch):
    """Every (shape, law, form) of deep_paths.device_cases(): identical to the oracle's run of the case."""
    shape, law, n_sims, opts = D.CASES[cid]
    want = D.oracle(shape, law, n_sims, **opts)
    kw, desc, blob, roots = D.case(shape, law, n_sims, **opts)
    _force(monkeypatch, form)
    got = E.run_engine(native.HipEngine, kw, desc, blob, roots, None, sidx=D.SIDX)
    E.assert_same(got, want)
    _assert_form(cid, form, got["info"])


@pytest.mark.parametrize("shape", D.POP_SHAPES)
def test_population_of_chains_in_one_launch(native, shape):
    """Three nets of distinct weights, 19 trees each (a full workgroup and a ragged one per net), CHAIN 60 with shared settings:
    one launch against three one-net oracle engines."""
    kw, desc, blobs, roots = D.population_case(shape)
    got = E.run_engine(native.HipEngine, kw, desc, blobs, roots, None, sidx=D.SIDX)
    E.assert_same(got, E.concat_runs(D.oracle_population(shape)))
    info = got["info"]
    assert info["kernel_form"] == "persistent" and info["kernel_name"].startswith("search_kernel<") and info["max_children"] == 1, info


def test_three_laws_in_one_launch(native):
    """search_kernel_nets: net 0 CHAIN (120 levels), net 1 c_pw 1 / kappa 0.5 (5 levels), net 2 NARROW (46 levels), the engine
    created with the widest law (Kmax 11, so net 0's one-child nodes sit in trees laid out for eleven).  A workgroup belongs to one net
    (search_kernel_body.inc: wnet), so one launch runs workgroups that take backup_from at nearly every trace next to workgroups
    that never do.  Against net_search_util.oracle_nets: each net on an oracle engine created with its own settings."""
    kw, desc, blobs, roots, settings = D.net_search_case()
    e = native.HipEngine(**kw)
    e.set_population(len(blobs))
    for k, b in enumerate(blobs):
        e.set_net_weights(k, desc, b)
    e.set_net_search(settings)
    e.set_search_index(D.SIDX)
    e.search(roots, None)
    got = dict(e.results()), dict(e.dump_tree()), e.root_children()
    info = e.search_info()
    e.close()
    want = N.oracle_nets(kw, desc, blobs, roots, None, D.SIDX, settings, width=N.kmax_of(settings[1], D.NET_SIMS))
    for g, w in zip(got[:2], want[:2]):
        assert set(g) == set(w)
        for k in w:
            x, y = np.asarray(g[k]), np.asarray(w[k])
            assert x.dtype == y.dtype and x.shape == y.shape, k
            assert x.tobytes() == y.tobytes(), f"{k}: trees {[i for i in range(x.shape[0]) if x[i].tobytes() != y[i].tobytes()][:8]} differ"
    for x, y in zip(got[2], want[2]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert info["kernel_name"].startswith("search_kernel_nets<") and D.POP_T % info["tile_trees"] != 0, info


def test_selfplay_from_one_child_roots(native):
    """Device self-play under CHAIN: the step kernel picks the final action from a root with one child (one-column replay rows)."""
    a_rows, a_stats = D.selfplay_play(native.HipEngine)
    b_rows, b_stats = D.selfplay_play(O.OracleEngine)
    assert a_rows.shape == b_rows.shape == (D.SELFPLAY["steps"] * D.SELFPLAY["games"], 7)
    np.testing.assert_array_equal(a_rows.view(np.uint32), b_rows.view(np.uint32))
    assert_stats_bits(a_stats, b_stats, "deep self-play")
