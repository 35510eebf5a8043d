"""Continuous searches deeper than the 16 levels a tree's lanes hold: the cases (an engine configuration, a net, roots and a widening
law each), the conditions their oracle runs must meet before a device is compared with them, an independent float64 replay of the
backup, and the table of device runs (case x kernel form) that tests/test_deep_paths.py takes.

Progressive widening gives a node ceil(c_pw (n + 1)^kappa) children.  Under every configuration of the other suites (c_pw 1, kappa 0.5)
a 200-simulation tree is 4 levels deep; the deep continuous backup -- backup_path's `else` arm, the hand-over of the 16th return,
backup_from<CONT>, the path slots' wrap in the scored descent (csrc/tree.cuh, csrc/tree_phases.cuh) -- needs a narrow law:
  CHAIN   c_pw 1, kappa 0: one child per node, so a tree of n_sims simulations IS a path of n_sims levels (and Kmax = 1);
  NARROW  c_pw 0.15, kappa 0.5: a node is entitled to a second child at its 45th visit, so a chain of 44 levels grows first and
          then branches, two children per node, along its upper levels.  (c_pw 0.2, the law of the narrow golden fixture, branches
          at the 25th visit and ends at 26 to 35 levels whatever the number of simulations: too few traces reach level 33.)

Shared by the CPU tests (test_deep_paths_host.py) and the GPU tests (test_deep_paths.py); numpy and the CPU oracle only."""
import functools
import math

import numpy as np

import edge_values as E
import oracle_lib as O
from alphazero_gym_amd import _capi

CHAIN = (1.0, 0.0)
NARROW = (0.15, 0.5)
GOLDEN_NARROW = (0.2, 0.5)           # tests/golden/t1_pendulum_v1_narrow200.npz
LAWS = {"chain": CHAIN, "narrow": NARROW}

SEED, BASE, SIDX = 4321, 55, 3       # engine seed, tree_id_base, search index of every case

# name -> env, net and batch.  trees: ragged (19 = 16 + 3, 37 = 2 x 16 + 5) except where the team kernels want 32.
SHAPES = {
    "p64": dict(env_id=2, hidden=(64, 64), trees=37, wseed=65),                          # Pendulum-v1, the register-resident 4-wave kernels
    "p256": dict(env_id=2, hidden=(256, 256), trees=37, wseed=72),                       # ... config C's eight-wave kernel
    "gmm128": dict(env_id=1, hidden=(128, 128, 128), ncomp=2, trees=19, wseed=73),       # Pendulum-v0, a mixture head of two components
    "ln100": dict(env_id=2, hidden=(100, 60), ln=True, trees=19, wseed=74),              # LayerNorm: the weight-streaming kernels
    "mcc64": dict(env_id=4, hidden=(64, 64), trees=19, wseed=75),                        # MountainCarContinuous: terminal nodes
    "mcc256": dict(env_id=4, hidden=(256, 256), trees=19, wseed=76),
    "p512": dict(env_id=2, hidden=(512, 512), trees=32, wseed=77),                       # wide nets: team kernel / per-layer launches / one launch
    "p1024": dict(env_id=2, hidden=(1024, 1024, 1024, 1024), trees=32, wseed=78),        # BASELINE config E's net
    "mcc512": dict(env_id=4, hidden=(512, 512), trees=32, wseed=79),
}


def in_dim(shape):
    return 2 if SHAPES[shape]["env_id"] == 4 else 3


def lower_slope_roots(n):
    """MountainCarContinuous roots on the lower slope, moving towards the flag: it is 17 to 30 steps away, so terminal nodes sit deeper
    than the 16 levels of the lanes."""
    u = np.arange(n) / 18.0
    return np.stack([-0.35 + 0.5 * (u % 1.0), 0.035 + 0.03 * ((7.0 * u) % 1.0)], 1)


def case(shape, law, n_sims, gamma=None, epsilon=0.0, v_target="off_policy", trees=None, tree_id_base=BASE, wseed=None):
    """(engine kwargs, descriptor, blob, roots) of a case.  gamma (None): 0.99 under CHAIN -- the float32 first-level product gamma_f V and
    the float64 gamma R above it on every level -- and 1 under a NARROW law (the configs' own)."""
    sh = SHAPES[shape]
    c_pw, kappa = LAWS[law]
    hidden, C = list(sh["hidden"]), sh.get("ncomp", 0)
    n_dist = 3 * C if C else 2
    n = trees or sh["trees"]
    if gamma is None:
        gamma = 0.99 if law == "chain" else 1.0
    kw = dict(env_id=sh["env_id"], mode=1, n_trees=n, n_sims=n_sims, c_uct=0.05, gamma=gamma, epsilon=epsilon, c_pw=c_pw, kappa=kappa,
              v_target=v_target, seed=SEED, tree_id_base=tree_id_base, action_bound=1.0 if sh["env_id"] == 4 else 2.0)
    desc = _capi.make_desc(in_dim(shape), hidden, n_dist, "elu", num_components=C, layernorm=sh.get("ln", False))
    blob = O.make_weights(sh["wseed"] if wseed is None else wseed, in_dim(shape), hidden, n_dist, scale=1.0)
    if sh.get("ln"):
        blob = O.add_layernorm(blob, in_dim(shape), hidden, n_dist, 7)
    if sh["env_id"] == 4:
        roots = lower_slope_roots(n)
    else:
        o = O.OracleEngine(**kw)
        roots = np.array(o.synthetic_roots(), np.float64)
        o.close()
    return kw, desc, blob, roots


@functools.lru_cache(maxsize=None)
def _oracle_cached(shape, law, n_sims, opts):
    kw, desc, blob, roots = case(shape, law, n_sims, **dict(opts))
    return E.run_engine(O.OracleEngine, kw, desc, blob, roots, None, sidx=SIDX, trace=True)


def oracle(shape, law, n_sims, **opts):
    """The oracle's run of case(...), with the traces' leaves, computed once per process (treat as read-only)."""
    return _oracle_cached(shape, law, n_sims, tuple(sorted(opts.items())))


# ------------------------------------------------------------------------------------------------ the matrix
# CASES: id -> (shape, law, n_sims, options of case()).  Every distinct oracle run of the single-net device matrix.
_GMM = dict(gamma=0.97, epsilon=0.2, v_target="on_policy")     # the `pick` path on a one-child node
CASES = {
    "p64-chain60": ("p64", "chain", 60, {}),
    "p64-chain253": ("p64", "chain", 253, {}),        # 255 records: the 8-bit id limit
    "p64-chain300": ("p64", "chain", 300, {}),        # 302 records: 9-bit ids
    "p64-chain600": ("p64", "chain", 600, {}),        # 602 records: global trees
    "p64-narrow200": ("p64", "narrow", 200, {}),
    "p256-chain60": ("p256", "chain", 60, {}),
    "p256-narrow200": ("p256", "narrow", 200, {}),
    "gmm128-chain60": ("gmm128", "chain", 60, _GMM),
    "ln100-chain40": ("ln100", "chain", 40, {}),
    "mcc64-chain80": ("mcc64", "chain", 80, {}),
    "mcc64-narrow200": ("mcc64", "narrow", 200, {}),
    "mcc256-chain80": ("mcc256", "chain", 80, {}),
    "mcc256-narrow200": ("mcc256", "narrow", 200, {}),
    "p512-chain40": ("p512", "chain", 40, {}),
    "p512-narrow120": ("p512", "narrow", 120, {}),
    "p1024-chain40": ("p1024", "chain", 40, {}),
    "mcc512-chain80": ("mcc512", "chain", 80, {}),
    "p64-chain40-greedy": ("p64", "chain", 40, dict(v_target="greedy")),          # the value targets over a one-column result
    "p64-chain40-on_policy": ("p64", "chain", 40, dict(v_target="on_policy")),
}
# Every case is asked for leaf depths <= 15, == 16, >= 17 and >= 33 (backup_from's second round): check_run.

# the kernel forms each shape's cases run on (parity_util.VARIANT_ENV); a form that does not exist for a shape is not listed
FORMS = {
    "p64": ["default", "global_tree", "stream_weights", "tile16"],
    "p256": ["default", "no_spec", "waves4", "groups2", "global_tree"],
    "gmm128": ["default"], "ln100": ["default"],
    "mcc64": ["default", "global_tree"], "mcc256": ["default", "global_tree"],
    "p512": ["default", "launches", "persistent"],
    "p1024": ["default", "no_spec"],
    "mcc512": ["default"],
}


def device_cases():
    """[(id, case id, form)]: every device run of the single-net matrix.  A form is left out where its forcing variable is moot, so that
    it would only run the default's kernel again: global_tree on trees that are in global memory already (600 simulations), tile16
    on trees that are not in LDS with 8-bit ids (half-filled tiles exist there only: dispatch.cuh); the value-target cases run
    the default only."""
    out = []
    for cid, (shape, law, n_sims, opts) in CASES.items():
        for form in FORMS[shape]:
            if form == "global_tree" and n_sims + 2 > 511 or form == "tile16" and n_sims + 2 > 255:
                continue
            if "v_target" in opts and shape == "p64" and form != "default":
                continue
            out.append((f"{cid}-{form}", cid, form))
    return out


def kmax_of(law, n_sims):
    c_pw, kappa = LAWS[law]
    return max([1] + [math.ceil(c_pw * math.pow(n + 1, kappa)) for n in range(n_sims)])


def expected_storage(shape, law, n_sims, form):
    """Where dispatch keeps the trees of a single-net case (engine_host.h): LDS with 8-bit ids up to 255 records, 9-bit ids up to 511
    (not for a mixture head), global memory beyond or when forced."""
    R = n_sims + 2
    if form == "global_tree" or R > 511:
        return "global"
    return "lds8" if R <= 255 else "lds9"


# ------------------------------------------------------------------------------------------------ populations

POP_T, POP_K = 19, 3
POP_SHAPES = ["p64", "p256"]
POP_SIMS = 60


def population_case(shape):
    """Three nets of distinct weights on POP_T trees each, CHAIN 60 with shared settings, in one launch."""
    cases = [case(shape, "chain", POP_SIMS, trees=POP_T, tree_id_base=BASE + k * POP_T, wseed=SHAPES[shape]["wseed"] + 100 * k)
             for k in range(POP_K)]
    kw = dict(cases[0][0], n_trees=POP_K * POP_T, tree_id_base=BASE)
    return kw, cases[0][1], [c[2] for c in cases], np.concatenate([c[3] for c in cases])


def oracle_population(shape):
    """One single-net oracle engine per net of population_case(shape)."""
    return [oracle(shape, "chain", POP_SIMS, trees=POP_T, tree_id_base=BASE + k * POP_T, wseed=SHAPES[shape]["wseed"] + 100 * k)
            for k in range(POP_K)]


# per-net settings in one launch (azg_set_net_search): net 0 a 120-deep chain, net 1 the configs' law (4-level trees), net 2 NARROW
NET_LAWS = [CHAIN, (1.0, 0.5), NARROW]
NET_GAMMAS = (0.99, 1.0, 1.0)
NET_SIMS = 120


def net_search_case():
    """(engine kwargs, descriptor, blobs, roots, per-net settings): the engine is created with the widest law (net 1's: Kmax 11)."""
    kw, desc, blobs, roots = population_case("p64")
    kw = dict(kw, n_sims=NET_SIMS, gamma=1.0, c_pw=1.0, kappa=0.5)
    settings = [dict(c_uct=kw["c_uct"], gamma=g, epsilon=0.0, c_pw=law[0], kappa=law[1]) for law, g in zip(NET_LAWS, NET_GAMMAS)]
    return kw, desc, blobs, roots, settings


def oracle_net(k):
    """Net k of net_search_case() on a one-net oracle engine created with its own settings, with the traces' leaves (what
    net_search_util.oracle_nets runs, which keeps no traces)."""
    kw, desc, blobs, roots, settings = net_search_case()
    kw = dict(kw, n_trees=POP_T, tree_id_base=BASE + k * POP_T, **{key: settings[k][key] for key in ("gamma", "c_pw", "kappa")})
    return E.run_engine(O.OracleEngine, kw, desc, blobs[k], roots[k * POP_T:(k + 1) * POP_T], None, sidx=SIDX, trace=True)


# device self-play (azg_selfplay_*): the step kernel reads a one-child root -- Pendulum-v1 2x64, CHAIN, 24 simulations per move
SELFPLAY = dict(kw=dict(env_id=2, mode=1, n_sims=24, c_uct=0.05, gamma=0.99, c_pw=CHAIN[0], kappa=CHAIN[1], seed=SEED, tree_id_base=BASE),
                games=6, steps=3, max_len=2)


def selfplay_play(engine_cls):
    """(replay rows, (episode return sums, episode counts, env states)) of the self-play case on an engine class."""
    e = engine_cls(n_trees=SELFPLAY["games"], **SELFPLAY["kw"])
    e.set_weights(_capi.make_desc(3, [64, 64], 2, "elu"), O.make_weights(SHAPES["p64"]["wseed"], 3, [64, 64], 2, scale=1.0))
    e.selfplay_begin(SELFPLAY["max_len"], False, capacity_steps=SELFPLAY["steps"])
    for _ in range(SELFPLAY["steps"]):
        e.selfplay_step()
    rows, stats = e.selfplay_rows(clear=True), e.selfplay_stats()
    e.close()
    return rows, stats


# ------------------------------------------------------------------------------------------------ conditions

def leaf_depths(out):
    """Per tree: the depth of every trace's leaf, from the dump's parent links and trace_get's leaves."""
    dump, trace = out["dump"], out["trace"]
    return [E.depths(dump["parent"][t], dump["n_records"][t])[trace[t] & 0xffff] for t in range(trace.shape[0])]


def children_per_node(dump, t):
    n = int(dump["n_records"][t])
    return np.bincount(dump["parent"][t][1:n], minlength=n)


def replay(dump, trace, t, gamma):
    """Tree t's (edge_W, edge_Q) recomputed in numpy from the dump and the traces' leaves, in trace order: R = float64(float32(gamma) V)
    at the leaf's edge (V = 0 at a terminal leaf), R = r_k + gamma R up the path; W += R, Q = W / n.  edge_values.replay_W with
    per-edge rewards (node_r) and continuous mode's float32 first product."""
    n = int(dump["n_records"][t])
    par, r = dump["parent"][t][:n].tolist(), dump["node_r"][t][:n].tolist()      # (python floats are IEEE float64: the same arithmetic)
    V, flags = dump["node_V"][t], dump["node_flags"][t]
    W, cnt = [0.0] * n, [0] * n
    g32, g64 = np.float32(gamma), float(gamma)
    for leaf in (trace[t] & 0xffff).tolist():
        j = leaf
        v = np.float32(0.0) if flags[j] & 2 else np.float32(V[j])
        gR = float(np.float32(g32 * v))                # the float32 product, widened
        while j != 0:
            R = r[j] + gR
            W[j] += R
            cnt[j] += 1
            gR = g64 * R
            j = par[j]
    W, cnt = np.array(W, np.float64), np.array(cnt, np.int64)
    Q = np.zeros(n, np.float64)
    Q[cnt > 0] = W[cnt > 0] / cnt[cnt > 0]
    return W, Q, cnt


def check_conditions(cid, out):
    """What the oracle's run of CASES[cid] must contain before a device is compared with it.  Returns a few figures for the records."""
    shape, law, n_sims, opts = CASES[cid]
    return check_run(out, law, n_sims, opts.get("gamma", 0.99 if law == "chain" else 1.0), mcc=SHAPES[shape]["env_id"] == 4)


def check_run(out, law, n_sims, gamma, mcc=False):
    dump, trace, res = out["dump"], out["trace"], out["results"]
    nt = trace.shape[0]
    ld = leaf_depths(out)
    all_ld = np.concatenate(ld)
    assert (all_ld <= 15).any() and (all_ld == 16).any() and (all_ld >= 17).any(), np.bincount(all_ld)
    assert (all_ld >= 33).sum() >= nt, all_ld.max()                   # backup_from loops twice: at least a trace per tree's worth
    fig = dict(max_depth=int(all_ld.max()), traces_ge17=int((all_ld >= 17).sum()), traces_ge33=int((all_ld >= 33).sum()))
    if law == "chain":
        assert res["counts"].shape[1] == res["actions"].shape[1] == res["Q"].shape[1] == 1           # Kmax = 1
        assert (res["n_children"] == 1).all()
        for t in range(nt):
            n = int(dump["n_records"][t])
            kids = children_per_node(dump, t)
            assert (dump["parent"][t][1:n] == np.arange(n - 1)).all() and (kids[:n - 1] == 1).all() and kids[n - 1] == 0, t
        if not mcc:
            assert fig["max_depth"] == n_sims and (dump["n_records"] == n_sims + 1).all()
    else:
        # a node below the root, itself at depth >= 1, with two or more children, on the path of a trace of 17 or more levels
        branched = 0
        for t in range(nt):
            n = int(dump["n_records"][t])
            d = E.depths(dump["parent"][t], n)
            wide = (children_per_node(dump, t) >= 2) & (d >= 1)
            for s in np.nonzero(ld[t] >= 17)[0]:
                j = int(trace[t, s]) & 0xffff
                j = int(dump["parent"][t][j])                          # (the leaf itself has no children on this trace's path)
                while j != 0:
                    branched += int(wide[j])
                    j = int(dump["parent"][t][j])
        assert branched >= 1
        fig["deep_traces_through_branches"] = branched
    if mcc:
        # a terminal node at depth >= 17 that is the leaf of two or more traces: the later ones end in the existing node, V = 0, no record
        revisits = []
        for t in range(nt):
            n = int(dump["n_records"][t])
            d = E.depths(dump["parent"][t], n)
            leaves = np.bincount(trace[t] & 0xffff, minlength=n)
            term = (dump["node_flags"][t][:n] & 2) != 0
            revisits += [(t, int(d[j]), int(leaves[j])) for j in np.nonzero(term & (d >= 17) & (leaves >= 2))[0]]
        assert revisits, "no terminal node at depth >= 17 is the leaf of two traces"
        assert (dump["n_records"] < n_sims + 1).any()
        fig["deep_terminal_revisits"] = revisits[:6]
        if law == "chain":
            assert fig["max_depth"] == int(dump["n_records"].max()) - 1
    # the independent replay: float64 numpy against the oracle's own chain, bit for bit
    for t in range(nt):
        n = int(dump["n_records"][t])
        W, Q, cnt = replay(dump, trace, t, gamma)
        assert (cnt == dump["edge_n"][t][:n]).all(), t
        assert W.tobytes() == dump["edge_W"][t][:n].tobytes(), (t, np.nonzero(W != dump["edge_W"][t][:n])[0][:8])
        assert Q.tobytes() == dump["edge_Q"][t][:n].tobytes(), (t, np.nonzero(Q != dump["edge_Q"][t][:n])[0][:8])
    return fig
