"""GPU (-m gpu): populations (azg_set_population) against the CPU oracle on every search-kernel shape a population can run.

A K-net engine must compute, bit for bit, what K oracle engines compute -- net k with its own weights and tree_id_base + k*T, under
the population's search index: results, root children and every record of every tree.  The matrix takes test_hip_parity's
configurations (those a population accepts: padded hidden width <= 256) crossed with its variants, and asserts from search_info()
that the forced shape really ran and that every net spans a full workgroup and a ragged one (search_kernel.cuh: wnet, wj0, n_live).
Then the CU-count edges where the padded tree count flips the tile / group choice (engine_host.h: azg_padded_trees), and engines used
more than once."""
import functools
import math
import re

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from alphazero_gym_amd import _capi

pytestmark = pytest.mark.gpu

K = 3                   # nets of the matrix's populations
BASE, SIDX = 77, 3      # tree_id_base, search index
VARIANTS = ["default", "stream_weights", "global_tree", "waves8", "waves4", "groups2", "trace_cap1", "trace_cap64", "tile16", "tile8",
            "no_spec"]


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _shape(cfg, variant):
    """The search_info a population of this configuration must report under the variant: dispatch.cuh's choices (and engine_weights.hip's
    register residency, resident_layers) for a batch of fewer workgroups than the device has CUs."""
    env, mode, hidden, act, n_sims, extra, ncomp, ln = P.split_config(cfg)
    HP = -(-max(hidden) // 64) * 64
    nhh = len(hidden) - 1
    nreg = nhh if 1 <= nhh <= 2 and nhh * HP * HP // 256 <= 288 and act in ("relu", "elu") and not ln else 0
    if variant == "stream_weights":
        nreg = 0
    A = extra.get("num_actions", 0)
    if mode == 1:
        R = n_sims + 2
        kmax = max([1] + [math.ceil(extra.get("c_pw", 1.0) * math.pow(n + 1, extra.get("kappa", 0.5))) for n in range(n_sims)])
    else:
        R, kmax = 1 + A * (n_sims + 1), A
    nmax = (6 if mode == 0 else 0) + n_sims + 2          # (carried root counts: tree % 7)
    ts = "global"
    if kmax <= 16 and variant != "global_tree":
        if R <= 255 and nmax < 65536:
            ts = "lds8"
        elif R <= 511 and nmax < 2048 and ncomp < 2:
            ts = "lds9"
    waves, groups, tile = 4, 1, 16
    if HP == 256 and nreg == 1 and mode == 1 and ts == "lds8" and ncomp < 2 and variant != "waves4":
        waves, groups = 8, 2 if variant == "groups2" else 1
    elif HP <= 128 and nreg == 1 and ts == "lds8" and ncomp < 2 and variant != "tile16":
        tile = 8
    common = extra.get("epsilon", 0.0) == 0.0 and env != 1 and (mode == 1 or (env == 0 and A == 2))
    spec = int(nreg == 1 and ts == "lds8" and tile == 16 and ncomp < 2 and env != 5 and common and variant != "no_spec")
    return dict(HP=HP, nreg=nreg, tree_storage=ts, waves=waves, groups=groups, tile_trees=tile, spec=spec)


def _matrix():
    """Every (configuration, variant) a population runs; a variant is left out where test_hip_parity calls it moot and where it would
    only re-run the default's kernel (its forced shape is already the default's)."""
    cases, left_out = [], []
    for ci, cfg in enumerate(P.CONFIGS):
        if max(cfg[2]) > 256:
            continue                                          # (populations refuse the team / per-layer forms)
        for v in VARIANTS:
            same = v not in ("default", "trace_cap1", "trace_cap64") and _shape(cfg, v) == _shape(cfg, "default")
            (left_out if P.moot(cfg, v) or same else cases).append(pytest.param(ci, v, id=f"cfg{ci}-{v}"))
    return cases, left_out


CASES, LEFT_OUT = _matrix()


def _inputs(ci, T, nets=K):
    """Engine kwargs, descriptor, one blob per net (distinct weights and LayerNorm parameters), roots and carried counts of a
    population of `nets` x T trees: every net's segment gets the configuration's hand-placed roots."""
    env, mode, hidden, act, n_sims, extra, ncomp, ln = P.split_config(P.CONFIGS[ci])
    kw = dict(env_id=env, mode=mode, n_trees=nets * T, n_sims=n_sims, seed=1234, tree_id_base=BASE, **extra)
    desc = P.config_net(P.CONFIGS[ci], 99)[0]
    blobs = [P.config_net(P.CONFIGS[ci], 99 + k, ln_seed=7 + k)[1] for k in range(nets)]
    o = O.OracleEngine(**kw)
    roots = o.synthetic_roots()
    o.close()
    for k in range(nets):
        roots[k * T:(k + 1) * T] = P.config_roots(env, roots[k * T:(k + 1) * T])
    carry = (np.arange(nets * T) % 7).astype(np.int32) if mode == 0 else None
    return kw, desc, blobs, roots, carry


def _collect(e):
    return dict(e.results()), dict(e.dump_tree()), e.root_children()


def _oracle(kw, desc, blobs, roots, carry, sidx):
    """K oracle engines, net k with tree_id_base + k*T, concatenated: what the population must compute."""
    nets = len(blobs)
    T = kw["n_trees"] // nets
    parts = []
    for k in range(nets):
        o = O.OracleEngine(**dict(kw, n_trees=T, tree_id_base=kw.get("tree_id_base", 0) + k * T))
        o.set_weights(desc, blobs[k])
        o.set_search_index(sidx)
        sl = slice(k * T, (k + 1) * T)
        o.search(roots[sl], None if carry is None else carry[sl])
        parts.append(_collect(o))
        o.close()
    res = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    dump = {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
    return res, dump, (np.concatenate([p[2][0] for p in parts]), np.concatenate([p[2][1] for p in parts]))


@functools.lru_cache(maxsize=2)
def _oracle_case(ci, T):
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    return _oracle(kw, desc, blobs, roots, carry, SIDX)


def _population(native, kw, desc, blobs, order=None):
    e = native.HipEngine(**kw)
    e.set_population(len(blobs))
    for k in (range(len(blobs)) if order is None else order):
        e.set_net_weights(k, desc, blobs[k])
    return e


def _assert_same(got, want, T, what=""):
    """Every array of (results, dump_tree, root_children) identical (test_hip_parity's strictness); a failure names the nets whose
    trees differ."""
    (rg, dg, cg), (rw, dw, cw) = got, want
    assert set(rg) == set(rw) and set(dg) == set(dw)
    arrays = [("results " + k, rg[k], rw[k]) for k in rw] + [("dump " + k, dg[k], dw[k]) for k in dw]
    arrays += [("child_n", cg[0], cw[0]), ("child_state", cg[1], cw[1])]
    for name, a, b in arrays:
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        rows = [i for i in range(a.shape[0]) if a[i].tobytes() != b[i].tobytes()]
        msg = f"{what} {name}: trees {rows[:8]} of nets {sorted({i // T for i in rows})} differ"
        np.testing.assert_array_equal(a, b, err_msg=msg)


def _kernel_args(info):
    """search_kernel<ENV, HP, NREG, tree storage, GMM, waves, groups, tile trees, SPEC> of search_info's kernel name."""
    m = re.fullmatch(r"search_kernel<(.*)>", info["kernel_name"])
    assert m, info["kernel_name"]
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("ci,variant", CASES)
def test_population_bit_exact_vs_oracle(native, ci, variant, monkeypatch):
    """K = 3 nets of distinct weights on the configuration's shape under the variant: every record of every tree identical to K
    oracle engines; the forced shape ran (a variant that falls back to another kernel fails), and every net covers at least one full
    workgroup and a ragged one."""
    cfg = P.CONFIGS[ci]
    if variant in P.VARIANT_ENV:
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    want_shape = _shape(cfg, variant)
    T = 35 if want_shape["groups"] == 2 else 19           # 32 + 3 trees, 16 + 3, 8 + 8 + 3
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    e = _population(native, kw, desc, blobs)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    got = _collect(e)
    info = e.search_info()
    e.close()
    _assert_same(got, _oracle_case(ci, T), T, f"cfg{ci}-{variant}")
    args = _kernel_args(info)
    shape = dict(HP=int(args[1]), nreg=int(args[2]), tree_storage=info["tree_storage"], waves=info["waves"], groups=info["groups"],
                 tile_trees=info["tile_trees"], spec=info["spec"])
    print(f"cfg{ci}-{variant}: K={K} T={T} {shape}")
    assert info["kernel_form"] == "persistent" and shape == want_shape, (variant, shape, want_shape)
    tpw = shape["tile_trees"] * shape["groups"]
    assert -(-T // tpw) >= 2 and T % tpw != 0, (T, tpw)   # every net: a full workgroup and a ragged one
    env, n_sims = cfg[0], cfg[4]
    if env == 4:   # terminal nodes, and traces that ended in an existing one (no new record)
        d, B = got[1], K * T
        assert ((d["node_flags"] & 2) != 0).any(1).sum() >= B // 3 and (d["n_records"] < n_sims + 1).sum() >= B // 3
    if cfg[1] == 0:
        np.testing.assert_array_equal(got[1]["node_n"][:, 0], carry + n_sims)   # carried root counts


def test_the_matrix_reaches_every_shape():
    """The matrix is not silently thin: each variant keeps cases, and together they reach every shape the variants force (the shapes
    the other test asserts each case ran)."""
    by = {}
    for p in CASES:
        ci, v = p.values
        by.setdefault(v, []).append(_shape(P.CONFIGS[ci], v))
    # (AZG_WAVES=8 and AZG_TILE_TREES=8 force what a population of K x 19 trees picks by itself: its default cases run those shapes)
    assert set(by) == set(VARIANTS) - {"waves8", "tile8"}, sorted(by)
    shapes = [s for v in by.values() for s in v]
    for key, values in (("waves", {4, 8}), ("groups", {1, 2}), ("tile_trees", {8, 16}), ("tree_storage", {"lds8", "lds9", "global"}),
                        ("spec", {0, 1}), ("nreg", {0, 1, 2}), ("HP", {64, 128, 256})):
        assert {s[key] for s in shapes} == values, key


# ---------------------------------------------------------------------------------------------------------------- CU-count edges


@pytest.mark.parametrize("net", ["cartpole_2x128_relu", "pendulum_2x256_elu"])
def test_shape_flips_at_the_cu_count(native, net):
    """T = 1 at K = n_cus and K = n_cus + 1 nets: the padded tree count crosses the device's CU count there, which moves CartPole's
    2x128 net from half-filled 8-tree tiles to full 16-tree ones and Pendulum's 2x256 net from one 16-tree group per workgroup to
    two (32 trees, one live).  Both sides against K one-tree oracle engines."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    if net == "cartpole_2x128_relu":
        kw = dict(env_id=0, mode=0, n_sims=20, c_uct=1.5, gamma=1.0, num_actions=2, seed=34, tree_id_base=5)
        dims, key, flip = (4, [128, 128], 2, "relu"), "tile_trees", (8, 16)
    else:
        kw = dict(env_id=2, mode=1, n_sims=20, c_uct=0.05, gamma=1.0, c_pw=1.0, kappa=0.5, seed=34, tree_id_base=5)
        dims, key, flip = (3, [256, 256], 2, "elu"), "groups", (1, 2)
    in_dim, hidden, n_dist, act = dims
    desc = _capi.make_desc(in_dim, hidden, n_dist, act)
    seen = []
    for nets in (n_cus, n_cus + 1):
        kwn = dict(kw, n_trees=nets)
        blobs = [O.make_weights(500 + k, in_dim, hidden, n_dist) for k in range(nets)]
        o = O.OracleEngine(**kwn)
        roots = o.synthetic_roots()
        o.close()
        carry = (np.arange(nets) % 7).astype(np.int32) if kw["mode"] == 0 else None
        e = _population(native, kwn, desc, blobs)
        e.set_search_index(2)
        e.search(roots, carry)
        got = _collect(e)
        info = e.search_info()
        e.close()
        _assert_same(got, _oracle(kwn, desc, blobs, roots, carry, 2), 1, f"{net} K={nets}")
        seen.append(info[key])
        print(f"{net} K={nets} T=1: waves {info['waves']} groups {info['groups']} tile_trees {info['tile_trees']} spec {info['spec']}")
    assert tuple(seen) == flip, (key, seen)


# ---------------------------------------------------------------------------------------------------------------- engine reuse


@pytest.mark.parametrize("ci", [6, 13], ids=["cartpole_2x128_relu", "pendulum_100x60_elu_ln"])
def test_one_net_gets_new_weights(native, ci):
    """Search; re-upload net 1 only; search again under the same index: nets 0 and 2 are what their old weights give, net 1 what
    its new ones give (and not what the old ones gave)."""
    T = 19
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    e = _population(native, kw, desc, blobs)
    e.set_search_index(SIDX)
    e.search(roots, carry)
    first = _collect(e)
    _assert_same(first, _oracle(kw, desc, blobs, roots, carry, SIDX), T, "before")
    new = list(blobs)
    new[1] = P.config_net(P.CONFIGS[ci], 150, ln_seed=40)[1]
    e.set_net_weights(1, desc, new[1])
    e.set_search_index(SIDX)
    e.search(roots, carry)
    second = _collect(e)
    e.close()
    _assert_same(second, _oracle(kw, desc, new, roots, carry, SIDX), T, "after")
    sl = slice(T, 2 * T)
    assert not np.array_equal(first[0]["Q"][sl], second[0]["Q"][sl])


@pytest.mark.parametrize("ci", [6, 13], ids=["cartpole_2x128_relu", "pendulum_100x60_elu_ln"])
def test_population_resplit(native, ci):
    """One engine of 45 trees: 3 nets, search; then 5 nets, upload, search.  Each against its oracle engines: no workgroup count per
    net or weight stride of the first split survives into the second."""
    e = None
    for nets in (3, 5):
        kw, desc, blobs, roots, carry = _inputs(ci, 45 // nets, nets=nets)
        if e is None:
            e = native.HipEngine(**kw)
        e.set_population(nets)
        for k in range(nets):
            e.set_net_weights(k, desc, blobs[k])
        e.set_search_index(SIDX + nets)
        e.search(roots, carry)
        _assert_same(_collect(e), _oracle(kw, desc, blobs, roots, carry, SIDX + nets), 45 // nets, f"{nets} nets")
    e.close()


class _DevArr:
    """A raw device pointer as a CUDA-array-interface object (torch.as_tensor wraps it without a copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def test_resident_path_equals_search(native):
    """The bench's path on a population: upload_roots + search_resident, then results() and the device buffers of
    results_resident() -- both equal search()'s results, and the oracle's."""
    import torch
    ci, T = 0, 19
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    want = _oracle(kw, desc, blobs, roots, carry, SIDX)
    a = _population(native, kw, desc, blobs)
    a.set_search_index(SIDX)
    a.search(roots, carry)
    via_search = _collect(a)
    a.close()
    _assert_same(via_search, want, T, "search()")
    e = _population(native, kw, desc, blobs)
    e.set_search_index(SIDX)
    e.upload_roots(roots, carry)
    e.search_resident()
    p = e.results_resident()
    e.sync()
    B, Kc = e.n_trees, e.kmax
    dev = {"actions": torch.as_tensor(_DevArr(p["actions"], (B, Kc), "<f4"), device="cuda").cpu().numpy(),
           "counts": torch.as_tensor(_DevArr(p["counts"], (B, Kc), "<i4"), device="cuda").cpu().numpy(),
           "Q": torch.as_tensor(_DevArr(p["Q"], (B, Kc), "<f8"), device="cuda").cpu().numpy(),
           "v_target": torch.as_tensor(_DevArr(p["v_target"], (B,), "<f8"), device="cuda").cpu().numpy(),
           "n_children": torch.as_tensor(_DevArr(p["n_children"], (B,), "<i4"), device="cuda").cpu().numpy()}
    resident = _collect(e)
    e.close()
    _assert_same(resident, via_search, T, "search_resident")
    for k in via_search[0]:
        np.testing.assert_array_equal(dev[k], via_search[0][k], err_msg=f"results_resident {k}")


@pytest.mark.parametrize("ci", [2, 15], ids=["pendulum_v0_3x128_elu", "cartpole_3x128_silu_ln"])
def test_nets_uploaded_in_reverse_order(native, ci):
    """Net weights uploaded last net first: the first upload allocates every net's block, the others fill theirs in."""
    T = 19
    kw, desc, blobs, roots, carry = _inputs(ci, T)
    e = _population(native, kw, desc, blobs, order=range(K - 1, -1, -1))
    e.set_search_index(SIDX)
    e.search(roots, carry)
    got = _collect(e)
    e.close()
    _assert_same(got, _oracle(kw, desc, blobs, roots, carry, SIDX), T, "reverse upload")
