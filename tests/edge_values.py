"""Values at the edges of the float32 range for the search: the backup's closed form restated in numpy, the float32 values on which
closed form and serial chain differ (TEETH), hand-built networks that put a chosen value / prior / log sigma / mu into every node,
and the cases (with the conditions their oracle runs must meet) that tests/test_edge_values.py compares on the device.

Shared by the CPU tests (test_backup_closed_form.py) and the GPU tests (test_edge_values.py); numpy and the CPU oracle only."""
import functools

import numpy as np

import oracle_lib as O
import parity_util as P
from alphazero_gym_amd import _capi

F32_MAX = np.float32(3.4028234663852886e38)
LO, HI = np.float32(2.0 ** -25), np.float32(2.0 ** 30)      # tree.cuh: the closed form's range is V == 0 or LO <= |V| < HI

# (r_first, r_uniform) of a path (tree.cuh backup_path): the edge into the leaf carries r_first, every other edge r_uniform
REWARDS = {"cartpole": (1.0, 1.0), "mountaincar": (-1.0, -1.0), "acrobot": (0.0, -1.0)}
# what a NON-terminal leaf's path carries in each env (Acrobot pays 0 on the terminal step only, and a terminal leaf's V is 0)
LEAF_REWARDS = {"cartpole": (1.0, 1.0), "mountaincar": (-1.0, -1.0), "acrobot": (-1.0, -1.0)}
ENV = {"cartpole": dict(env_id=0, in_dim=4, A=2), "mountaincar": dict(env_id=3, in_dim=2, A=3), "acrobot": dict(env_id=5, in_dim=6, A=3)}


def f32(bits):
    """The float32 with these bits."""
    return np.array([bits], np.uint32).view(np.float32)[0]


def bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def in_range(V):
    """tree.cuh backup_path, the gamma == 1 arm: `av == 0.0f || (av >= 0x1p-25f && av < 0x1p30f)`."""
    av = np.abs(np.asarray(V, np.float32))
    return (av == 0) | ((av >= LO) & (av < HI))


def chain(V, r_first, r_uniform, levels=16):
    """The serial chain of tree.cuh (gamma == 1): R = (double)V; R = (d == 0 ? r_first : r_uniform) + R -- [levels, ...] float64."""
    R = np.asarray(V, np.float32).astype(np.float64)
    out = []
    for d in range(levels):
        R = np.float64(r_first if d == 0 else r_uniform) + R
        out.append(R)
    return np.stack(out)


def closed(V, r_first, r_uniform, levels=16):
    """The closed form of tree.cuh: (r_first + (double)dl * r_uniform) + (double)V for dl = 0 .. levels - 1."""
    Vd = np.asarray(V, np.float32).astype(np.float64)
    return np.stack([(np.float64(r_first) + np.float64(dl) * np.float64(r_uniform)) + Vd for dl in range(levels)])


def differs(V, rewards, levels=16):
    """Whether chain and closed form differ at some level 1..levels for the float32 value(s) V."""
    a, b = chain(V, *rewards, levels), closed(V, *rewards, levels)
    return (a.view(np.uint64) != b.view(np.uint64)).any(0)


def line_W_differs(V, rewards, visits=8):
    """Whether an edge's W would differ after 2..visits visits along one line (the returns of levels 1, 2, ... added in this order,
    as on the first edge of a path that grows by one node per trace): a difference in a return that the sum's rounding swallows
    at once would change no record."""
    a, b = chain(V, *rewards, visits), closed(V, *rewards, visits)
    Wa, Wb, ne = np.zeros_like(a[0]), np.zeros_like(a[0]), np.zeros(a[0].shape, bool)
    for d in range(visits):
        Wa, Wb = Wa + a[d], Wb + b[d]
        ne |= Wa.view(np.uint64) != Wb.view(np.uint64)
    return ne


def _find_teeth(env):
    """Float32 values outside the closed form's range on which it differs from the chain under every reward pattern the env's paths
    carry, within the first four levels and in the W of an edge visited up to eight times (so that many records of a tree show
    it): two below 2^-25 and two at or above 2^30, one of each sign, nearest to the thresholds (a fixed, seeded search)."""
    rng = np.random.Generator(np.random.PCG64(2025))
    mant = np.concatenate([[0x555555, 0x7fffff, 0x2aaaaa, 1, 0x400001], rng.integers(0, 1 << 23, 64)]).astype(np.uint32)
    pats = {REWARDS[env], LEAF_REWARDS[env]}
    out = []
    for exps in (range(-26, -70, -1), range(30, 70)):          # nearest to the thresholds first
        found = []
        for e in exps:
            for sign in (0, 1):
                if len(found) >= 2:
                    break
                if found and (bits(found[-1]) >> 31) == sign:
                    continue                                    # one of each sign
                v = ((np.uint32(sign) << 31) | (np.uint32(e + 127) << 23) | mant).view(np.float32)
                ok = np.logical_and.reduce([differs(v, p, 4) & line_W_differs(v, p) for p in pats])
                if ok.any():
                    found.append(v[np.argmax(ok)])
        out += found
    return [np.float32(v) for v in out]


TEETH = {env: _find_teeth(env) for env in ENV}


# ------------------------------------------------------------------------------------------------ hand-built networks
# blob layout (synthetic.make_weights): per trunk layer W [h, k] and b [h]; value W [1, k], b [1]; dist W [n_dist, k], b [n_dist]

def net_blob(in_dim, hidden, n_dist, value_bias=0.0, dist_bias=None, trunk=None, dist_w=None, trunk_bias=None):
    """A network of zeros with the given value bias and distribution bias; trunk: {(layer, unit, input): weight}, dist_w:
    {(output, unit): weight}, trunk_bias: {(layer, unit): bias}.  With a zero value row the value head returns the bias itself, bit
    for bit (a subnormal included)."""
    parts, k = [], in_dim
    for li, h in enumerate(hidden):
        W, b = np.zeros((h, k), np.float32), np.zeros(h, np.float32)
        for (l, u, i), w in (trunk or {}).items():
            if l == li:
                W[u, i] = w
        for (l, u), v in (trunk_bias or {}).items():
            if l == li:
                b[u] = v
        parts += [W.ravel(), b]
        k = h
    parts += [np.zeros(k, np.float32), np.array([value_bias], np.float32)]
    Wd = np.zeros((n_dist, k), np.float32)
    for (o, u), w in (dist_w or {}).items():
        Wd[o, u] = w
    parts += [Wd.ravel(), np.zeros(n_dist, np.float32) if dist_bias is None else np.asarray(dist_bias, np.float32)]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def peaked_net(env, hidden, V):
    """Constant value V, priors peaked on action 0 (logit bias 12): with c_uct = 50 the search follows one line deep."""
    d = ENV[env]
    return net_blob(d["in_dim"], hidden, d["A"], V, dist_bias=[12.0] + [0.0] * (d["A"] - 1))


def balancing_net(hidden, V, g=40.0):
    """CartPole: units 0 / 1 carry relu(+-(g theta + g/4 theta_dot)) through an identity second layer (one-layer trunks: straight)
    into the logits -+(h0 - h1): push towards the side the pole falls to.  Constant value V."""
    trunk = {(0, 0, 2): g, (0, 0, 3): g / 4, (0, 1, 2): -g, (0, 1, 3): -g / 4}
    for li in range(1, len(hidden)):
        trunk[(li, 0, 0)] = 1.0
        trunk[(li, 1, 1)] = 1.0
    return net_blob(4, hidden, 2, V, trunk=trunk, dist_w={(0, 0): -1.0, (0, 1): 1.0, (1, 0): 1.0, (1, 1): -1.0})


# ------------------------------------------------------------------------------------------------ discrete cases

def discrete_values(env):
    """[(label, float32 value)] of the discrete cases: in range first, then out of range."""
    inr = [0.0, -0.0, 2.0 ** -25, -2.0 ** -25, float(f32(0x337fffff)), -float(f32(0x337fffff)), 0.75, float(f32(0x4e7fffff)),
           -float(f32(0x4e7fffff))]
    out = [float(f32(0x32ffffff)), -float(f32(0x32ffffff))] + [float(v) for v in TEETH[env]] + [2.0 ** 30, float(F32_MAX), 1e-40]
    vals = [np.float32(v) for v in inr + out]
    assert f32(0x337fffff) == np.float32(float.fromhex("0x1.fffffep-25")) and f32(0x4e7fffff) == np.float32(float.fromhex("0x1.fffffep+29"))
    assert f32(0x32ffffff) == np.float32(float.fromhex("0x1.fffffep-26"))
    assert all(in_range(v) for v in vals[:len(inr)]) and not any(in_range(v) for v in vals[len(inr):])
    return [(f"{bits(v):08x}", v) for v in vals]


def is_tooth(env, V):
    return any(bits(V) == bits(t) for t in TEETH[env])


def short_list(env):
    """One in-range and two out-of-range values for the variants: 0.75, a TEETH value below 2^-25 and one at or above 2^30."""
    return [np.float32(0.75), TEETH[env][0], TEETH[env][2]]


# CartPole with |V| >= 2^53 ("sharp"): Q's unit in the last place is 2 or more there, and it grows with |V| (2^104 at float32 max), so
# the prior term c_uct * prior * sqrt(N + 1) / (n + 1) is seen only if the constant grows with |V| too: c_uct = max(CUCT_BIG, CUCT_PER_V |V|),
# 2.6e33 at float32 max (a float32 like every c_uct).  With that constant the priors decide, so they are made sharp (gain G_BIG
# instead of 40): the search follows the balancing line one node deeper per trace instead of spreading over both actions.
CUCT_BIG, CUCT_PER_V, G_BIG = 5e4, 2.0 ** -17, 4000.0


def sharp_c_uct(V):
    return float(np.float32(max(CUCT_BIG, CUCT_PER_V * abs(float(V)))))


B = 37    # ragged: neither a multiple of the 16-tree workgroup nor of the 8-tree half tile


def default_sims(env):
    return 100 if env == "cartpole" else 60


def discrete_case(env, V, hidden=(64, 64), gamma=1.0, n_sims=None, n_trees=B, sharp=None, tree_id_base=55, c_uct=None):
    """(engine kwargs, descriptor, blob, roots, carried root counts) of a discrete case with constant value V.
    sharp (CartPole; None: from |V|): the large exploration constant with the sharp balancing priors.  c_uct: the constant, where the
    case's own choice will not do (a population's nets share the engine's)."""
    d = ENV[env]
    hidden = list(hidden)
    n_sims = n_sims or default_sims(env)
    if env == "cartpole":
        sharp = abs(float(V)) >= 2.0 ** 53 if sharp is None else sharp
        kw = dict(c_uct=sharp_c_uct(V) if sharp else 5.0)
        blob = balancing_net(hidden, V, G_BIG if sharp else 40.0)
    else:
        kw = dict(c_uct=50.0)
        blob = peaked_net(env, hidden, V)
    if gamma != 1.0 and abs(float(V)) >= 2.0 ** 30:
        # discounting separates the Q of one level from the next by 3 % of V: a constant far above V keeps the search on the priors' line
        kw = dict(c_uct=float(np.float32(1e6 * abs(float(V)))))
    if c_uct is not None:
        kw = dict(c_uct=c_uct)
    kw = dict(env_id=d["env_id"], mode=0, n_trees=n_trees, n_sims=n_sims, gamma=gamma, num_actions=d["A"], seed=4321,
              tree_id_base=tree_id_base, **kw)
    desc = _capi.make_desc(d["in_dim"], hidden, d["A"], "relu")
    o = O.OracleEngine(**kw)
    roots = np.array(o.synthetic_roots(), np.float64)
    o.close()
    if env == "cartpole":
        roots[:, :] = 0.0
        roots[:, 2] = np.linspace(-0.02, 0.02, n_trees)       # near upright: the balancing line is long
        roots[3] = [2.35, 1.5, 0.0, 0.0]                      # leaves the track after a few steps: terminal leaves (V = 0) beside the others
    elif env == "acrobot":
        roots = P.upswing_roots(roots)
        for i in range(n_trees):
            if O.env_step(5, roots[i], 1)[2] or (-np.cos(roots[i][0]) - np.cos(roots[i][1] + roots[i][0])) > 0.9:
                roots[i] = [0.05, -0.03, 0.02, 0.01]          # (already near the line: hang at rest instead)
        roots[5] = [1.373, -0.681, 2.48, 1.698]               # three steps below the line: terminal leaves
    else:
        roots[5] = [0.44, 0.04]                               # the flag is two steps away: terminal leaves
    carry = (np.arange(n_trees) % 7).astype(np.int32)
    return kw, desc, blob, roots, carry


def run_engine(cls, kw, desc, blobs, roots, carry=None, sidx=3, trace=False):
    """One search on an engine class; blobs: one weight blob, or a list of them (a population, one net per blob).  Returns
    results, the whole tree dump, the root's children and evaluation -- and the traces' leaves (trace: oracle only) / search_info
    (every engine class but the oracle's, which has none)."""
    e = cls(**kw)
    if isinstance(blobs, (list, tuple)):
        e.set_population(len(blobs))
        for k, b in enumerate(blobs):
            e.set_net_weights(k, desc, b)
    else:
        e.set_weights(desc, blobs)
    e.set_search_index(sidx)
    if trace:
        e.trace_enable()
    e.search(roots, carry)
    out = dict(results=e.results(), dump=e.dump_tree(), children=e.root_children())
    if not isinstance(blobs, (list, tuple)):
        out["root_eval"] = e.root_eval()                       # (the C ABI has no root evaluation for populations)
    if trace:
        out["trace"] = e.trace_get()[0]
    if cls is not O.OracleEngine:
        out["info"] = e.search_info()
    e.close()
    return out


def assert_same(a, b):
    """Every result, every record, the root's children and its evaluation: identical bits."""
    for part in ("results", "dump"):
        assert set(a[part]) == set(b[part])
        for k in b[part]:
            x, y = np.asarray(a[part][k]), np.asarray(b[part][k])
            assert x.dtype == y.dtype and x.shape == y.shape, (part, k)
            assert x.tobytes() == y.tobytes(), f"{part} {k}: trees {[i for i in range(x.shape[0]) if x[i].tobytes() != y[i].tobytes()][:8]} differ"
    extras = {"info", "trace", "mlp_eval"}                      # (what only one side records)
    assert set(a) - extras == set(b) - extras
    for part in ("children", "root_eval"):
        if part in b:
            assert len(a[part]) == len(b[part]) > 0, part
            for x, y in zip(a[part], b[part]):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), part


def concat_runs(parts):
    """The runs of K engines over consecutive tree segments as one batch's."""
    out = {p: {k: np.concatenate([q[p][k] for q in parts]) for k in parts[0][p]} for p in ("results", "dump")}
    out["children"] = tuple(np.concatenate([q["children"][i] for q in parts]) for i in range(len(parts[0]["children"])))
    return out                                                 # (without root_eval: a population engine has none to compare)


@functools.lru_cache(maxsize=None)
def _oracle_discrete_cached(env, vbits, hidden, gamma, n_sims, n_trees, sharp, tree_id_base, c_uct):
    kw, desc, blob, roots, carry = discrete_case(env, f32(vbits), hidden, gamma, n_sims, n_trees, sharp, tree_id_base, c_uct)
    return run_engine(O.OracleEngine, kw, desc, blob, roots, carry, trace=True)


def oracle_discrete(env, V, hidden=(64, 64), gamma=1.0, n_sims=None, n_trees=B, sharp=None, tree_id_base=55, c_uct=None):
    """The oracle's run of discrete_case(...), computed once per process (treat as read-only)."""
    return _oracle_discrete_cached(env, bits(V), tuple(hidden), gamma, n_sims, n_trees, sharp, tree_id_base, c_uct)


# The discrete matrix.  DISCRETE_SETUPS: the network / search settings a value list runs on (each its own oracle run);
# DISCRETE_VARIANTS: engine variants (parity_util.VARIANT_ENV) that run a setup's oracle result on another device path.
DISCRETE_SETUPS = {
    "base": dict(),                                            # 2x64 ReLU, gamma 1: the whole value list
    "sims200": dict(n_sims=200),                               # CartPole: 403 records, 9-bit ids in LDS
    "gamma097": dict(gamma=0.97),                              # control: the discounted chain, whatever V
    "wide512": dict(hidden=(512,)),                            # the wide path: weights streamed from L2, trees in LDS or global memory
}


def discrete_oracle_cases():
    """[(id, env, V, setup)]: every distinct oracle run of the discrete matrix."""
    out = []
    for env in ENV:
        out += [(f"{env}-base-{lab}", env, V, "base") for lab, V in discrete_values(env)]
        for setup in ("sims200", "gamma097", "wide512"):
            if setup == "sims200" and env != "cartpole":
                continue
            out += [(f"{env}-{setup}-{bits(V):08x}", env, V, setup) for V in short_list(env)]
    return out


def discrete_device_cases():
    """[(id, env, V, setup, variant)]: the device runs.  The whole value list on the default kernel (37 trees of a 2x64 network: half-filled
    8-tree tiles, general kernel) and, CartPole, on full tiles, where the compile-time specialised kernel runs (tile16); the short list
    on the other variants and setups.  no_spec: the general kernel on full tiles, CartPole only (the other two envs have no
    specialised kernel to switch off).  The [512] net runs the wide one-launch kernel (a single hidden layer never takes the
    lock-step path, so AZG_FORCE_PERSISTENT / AZG_LS_TEAM have nothing to force) in both of its forms: trees in LDS (default) and
    in global memory (global_tree)."""
    out = [(i, env, V, setup, "default") for i, env, V, setup in discrete_oracle_cases()]
    out += [(f"cartpole-base-{lab}-tile16", "cartpole", V, "base", "tile16") for lab, V in discrete_values("cartpole")]
    for env in ENV:
        for variant in ("tile16", "no_spec", "global_tree", "trace_cap1", "trace_cap64"):
            if env == "cartpole" and variant == "tile16" or env != "cartpole" and variant == "no_spec":
                continue
            out += [(f"{env}-base-{bits(V):08x}-{variant}", env, V, "base", variant) for V in short_list(env)]
        out += [(f"{env}-wide512-{bits(V):08x}-global_tree", env, V, "wide512", "global_tree") for V in short_list(env)]
    return out


POP_T = 19                                                     # trees per net of the populations: 16 + 3, 8 + 8 + 3


def population_c_uct(env):
    """The one constant of a population's engine: CartPole's sharp one for the largest |V| among the nets, 50 elsewhere."""
    return sharp_c_uct(max(abs(float(V)) for V in short_list(env))) if env == "cartpole" else 50.0


def population_case(env):
    """Three nets in one launch: an in-range V, one below 2^-25 and one at or above 2^30 (short_list), each on POP_T trees with
    tree_id_base 55 + k POP_T (CartPole: the sharp priors and the large constant for all three, the constant being the engine's)."""
    cases = [discrete_case(env, V, n_trees=POP_T, sharp=True, tree_id_base=55 + k * POP_T, c_uct=population_c_uct(env))
             for k, V in enumerate(short_list(env))]
    assert len({c[0]["c_uct"] for c in cases}) == 1
    kw = dict(cases[0][0], n_trees=3 * POP_T, tree_id_base=55)
    return kw, cases[0][1], [c[2] for c in cases], np.concatenate([c[3] for c in cases]), np.concatenate([c[4] for c in cases])


def oracle_population(env):
    """Three single-net oracle engines, one per net of population_case(env)."""
    return [oracle_discrete(env, V, n_trees=POP_T, sharp=True, tree_id_base=55 + k * POP_T, c_uct=population_c_uct(env))
            for k, V in enumerate(short_list(env))]


def depths(parent, n_rec):
    d = np.zeros(int(n_rec), np.int64)
    for j in range(1, int(n_rec)):
        d[j] = d[parent[j]] + 1            # (a record's parent always precedes it)
    return d


def replay_W(dump, trace, t, n_sims, gamma, closed_form):
    """Tree t's edge_W recomputed from its dump and its traces' leaves, in trace order: the serial chain (oracle backup; tree.cuh's
    `else` loop) or, closed_form (gamma == 1 only), the one-addition form whatever V is (what a device that took the closed form's
    arm for this V would store)."""
    par, r, V = dump["parent"][t], dump["node_r"][t], dump["node_V"][t]
    W = np.zeros(int(dump["n_records"][t]), np.float64)
    for s in range(n_sims):
        j = int(trace[t, s]) & 0xffff
        Vd = np.float64(V[j])              # (0 for a terminal leaf)
        path = []
        while j != 0:
            path.append(j)
            j = int(par[j])
        R = Vd
        r_first, r_uni = r[path[0]], (r[path[1]] if len(path) > 1 else r[path[0]])
        for dl, k in enumerate(path):
            if closed_form and dl < 16:       # (beyond the 16 levels the lanes hold, backup_from chains on from the 16th return)
                R = (np.float64(r_first) + np.float64(dl) * np.float64(r_uni)) + Vd
            else:
                R = np.float64(r[k]) + (np.float64(gamma) * R)
            W[k] += R
    return W


def check_discrete_conditions(env, V, out, n_sims, gamma=1.0, need_33=None):
    """What an oracle run of a discrete case must contain before the device is compared with it (the case would otherwise miss,
    silently, what it is there for).  Returns a few figures for the records."""
    dump, trace = out["dump"], out["trace"]
    nt = trace.shape[0]
    leaf_depth = []
    for t in range(nt):
        d = depths(dump["parent"][t], dump["n_records"][t])
        leaf_depth.append(d[trace[t] & 0xffff])
    leaf_depth = np.concatenate(leaf_depth)
    assert (leaf_depth <= 15).any() and (leaf_depth == 16).any() and (leaf_depth >= 17).any(), np.bincount(leaf_depth)
    if env == "cartpole" if need_33 is None else need_33:
        assert (leaf_depth >= 33).any(), leaf_depth.max()             # backup_from loops twice
    # every expanded, non-terminal node carries the intended bits; terminal ones +0 -- and both kinds are leaves of some trace
    exp_nonterm = np.zeros_like(dump["node_flags"], bool)
    for t in range(nt):
        n = int(dump["n_records"][t])
        fl = dump["node_flags"][t][:n]
        exp_nonterm[t, :n] = ((fl & 1) != 0) & ((fl & 2) == 0)
    vb = dump["node_V"].view(np.uint32)
    assert (vb[exp_nonterm] == bits(np.float32(V) + np.float32(0.0))).all() and exp_nonterm.sum() > nt   # (bias -0.0: the head's sum is +0)
    assert (vb[~exp_nonterm] == 0).all()
    assert ((dump["node_flags"] & 2) != 0).any()                      # terminal leaves beside the others
    # the dump's W is the chain's; on a TEETH value the closed form would have stored something else
    n_diff = 0
    for t in range(nt):
        Wc = replay_W(dump, trace, t, n_sims, gamma, False)
        n = Wc.shape[0]
        assert Wc.tobytes() == dump["edge_W"][t][:n].tobytes(), t
        if gamma == 1.0:
            n_diff += int((replay_W(dump, trace, t, n_sims, gamma, True).view(np.uint64) != Wc.view(np.uint64)).sum())
    if gamma == 1.0 and in_range(V):
        assert n_diff == 0
    if gamma == 1.0 and is_tooth(env, V):
        assert n_diff >= 1
    return dict(max_depth=int(leaf_depth.max()), edges_closed_form_would_change=n_diff)


# ------------------------------------------------------------------------------------------------ continuous cases

CONT_SHAPES = {
    # Pendulum-v1, 2x256 ELU: config C's eight-wave kernel with the helper-wave policy finish (and its waves4 / global_tree / no_spec forms)
    "pendulum256": dict(env_id=2, in_dim=3, hidden=(256, 256), ncomp=0, bound=2.0, wseed=61),
    "mcc64": dict(env_id=4, in_dim=2, hidden=(64, 64), ncomp=0, bound=1.0, wseed=62),          # MountainCarContinuous: terminal nodes
    "gmm128": dict(env_id=2, in_dim=3, hidden=(128, 128, 128), ncomp=2, bound=2.0, wseed=63),  # a mixture head of two components
}
CONT_SETTINGS = ["v_subnormal", "v_max", "v_negzero", "ls_hi", "ls_lo", "mu_hi", "mu_lo"]
CONT_SIMS = 60
LS_MIN, LS_MAX = -5.0, 2.0       # _capi.make_desc's defaults (the policies' log_param_min / log_param_max)


def cont_settings(shape):
    return CONT_SETTINGS + (["coeff_lo"] if CONT_SHAPES[shape]["ncomp"] else [])


def cont_value(setting):
    return np.float32({"v_subnormal": 1e-40, "v_max": float(F32_MAX), "v_negzero": -0.0}.get(setting, 0.5))


def continuous_case(shape, setting, n_trees=B):
    """(engine kwargs, descriptor, blob, roots) of a continuous case: a seeded random ELU trunk under hand-set heads.  The value row
    is zero with the wanted bias (a constant-value net); a setting about the policy head zeroes the rows it is about and sets
    their biases, so that the head's output IS the bias in every node:
      v_subnormal  V = 1e-40 with gamma 0.97: the first level's float32 product gamma V is subnormal
      v_max        V = float32 max, gamma 1        v_negzero  value bias -0.0
      ls_hi/ls_lo  log sigma = +20 / -20: the clamp to [log_param_min, log_param_max] engages in every node
      mu_hi/mu_lo  mu = +40 / -40 (log sigma 0): tanh saturates, every sampled action is exactly +-bound
      coeff_lo     (mixture) the second component's log coefficient is -80"""
    sh = CONT_SHAPES[shape]
    hidden, C, k_in = list(sh["hidden"]), sh["ncomp"], sh["in_dim"]
    n_dist = 3 * C if C else 2
    blob = O.make_weights(sh["wseed"], k_in, hidden, n_dist, scale=1.0).copy()
    off, k = 0, k_in
    for h in hidden:
        off += h * k + h
        k = h
    vW, vb, dW, db = off, off + k, off + k + 1, off + k + 1 + n_dist * k
    blob[vW:vW + k] = 0.0
    blob[vb] = cont_value(setting)
    nc = max(C, 1)

    def head(row, bias):
        blob[dW + row * k:dW + (row + 1) * k] = 0.0
        blob[db + row] = bias

    if setting in ("ls_hi", "ls_lo"):
        for c in range(nc):
            head(nc + c, 20.0 if setting == "ls_hi" else -20.0)
    if setting in ("mu_hi", "mu_lo"):
        for c in range(nc):
            head(c, 40.0 if setting == "mu_hi" else -40.0)
            head(nc + c, 0.0)
    if setting == "coeff_lo":
        head(2 * C + 1, -80.0)
    kw = dict(env_id=sh["env_id"], mode=1, n_trees=n_trees, n_sims=CONT_SIMS, c_uct=0.05, gamma=0.97 if setting == "v_subnormal" else 1.0,
              c_pw=1.0, kappa=0.5, seed=4321, tree_id_base=55, action_bound=sh["bound"])
    desc = _capi.make_desc(k_in, hidden, n_dist, "elu", num_components=C)
    o = O.OracleEngine(**kw)
    roots = np.array(o.synthetic_roots(), np.float64)
    o.close()
    if sh["env_id"] == 4:
        roots = P.config_roots(4, roots)
    return kw, desc, blob, roots


@functools.lru_cache(maxsize=None)
def oracle_continuous(shape, setting):
    """The oracle's run of continuous_case(shape, setting), once per process (read-only), with the head's outputs on a seeded
    batch of observations (mlp_eval: value, dist, raw)."""
    kw, desc, blob, roots = continuous_case(shape, setting)
    out = run_engine(O.OracleEngine, kw, desc, blob, roots, None)
    e = O.OracleEngine(**kw)
    e.set_weights(desc, blob)
    obs = np.random.Generator(np.random.PCG64(17)).uniform(-8.0, 8.0, (128, CONT_SHAPES[shape]["in_dim"])).astype(np.float32)
    out["mlp_eval"] = e.mlp_eval(obs)
    e.close()
    return out


def check_continuous_conditions(shape, setting, out):
    """What the oracle's run of a continuous case must show before the device is compared with it.
    "In every node" is an argument by construction, not a walk over the tree (the dump keeps no per-node sigma or mu): the head rows a
    setting is about are zero, so their outputs are the biases whatever the observation.  What is checked is that the builder did
    that: the raw head outputs and the derived sigma / mixture share on 128 seeded observations and at every tree's root, the value in
    every expanded node of the dump, and for the saturated squash every sampled action of every tree."""
    sh = CONT_SHAPES[shape]
    dump, res = out["dump"], out["results"]
    C = sh["ncomp"]
    nc = max(C, 1)
    V = cont_value(setting)
    expanded = (dump["node_flags"] & 1) != 0
    nonterm = expanded & ((dump["node_flags"] & 2) == 0)
    assert nonterm.sum() > B and (dump["node_V"].view(np.uint32)[nonterm] == bits(V + np.float32(0.0))).all()
    value, dist, raw = out["mlp_eval"]
    assert (value.view(np.uint32) == bits(V + np.float32(0.0))).all()
    if sh["env_id"] == 4:
        assert ((dump["node_flags"] & 2) != 0).any()                    # terminal nodes beside the others
    if setting == "v_subnormal":
        prod = np.float32(0.97) * V
        assert 0.0 < float(prod) < float(np.finfo(np.float32).tiny) and 0.0 < float(V) < float(np.finfo(np.float32).tiny)
    if setting in ("ls_hi", "ls_lo"):
        ls = LS_MAX if setting == "ls_hi" else LS_MIN
        sigma = np.float32(O.math_eval(0, np.array([ls]))[0])           # azg_expf of the clamped log sigma
        assert (raw[:, 1 + nc:1 + 2 * nc] == (20.0 if setting == "ls_hi" else -20.0)).all()
        assert (dist[:, nc:2 * nc] == sigma).all() and (out["root_eval"][1][:, nc:2 * nc] == sigma).all()
    if setting in ("mu_hi", "mu_lo"):
        want = np.float32(sh["bound"] if setting == "mu_hi" else -sh["bound"])
        n_kids = res["n_children"]
        assert (n_kids >= 2).all()
        for t in range(B):
            assert (res["actions"][t, :n_kids[t]] == want).all(), (t, res["actions"][t])
        n = dump["n_records"]
        for t in range(B):
            assert (dump["edge_action"][t, 1:n[t]] == want).all()       # ... and every other sampled action of the tree
    if setting == "coeff_lo":
        assert (raw[:, 1 + 2 * C + 1] == -80.0).all()
        assert (dist[:, 2 * C] == 1.0).all()      # exp(-80 - l0) / sum is below half an ulp of 1: the first component's share rounds to 1


# ------------------------------------------------------------------------------------------------ edge domains of the math header

def _f32_around(x, n=4):
    """x as float32 with its n float32 neighbours on each side, as float64."""
    out = [np.float32(x)]
    lo = hi = np.float32(x)
    with np.errstate(over="ignore"):
        for _ in range(n):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            out += [lo, hi]
    return np.sort(np.array(out, np.float32)).astype(np.float64)


def _f64_around(x, n=4):
    out = [np.float64(x)]
    lo = hi = np.float64(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.sort(np.array(out, np.float64))


_F32_TINY, _F32_SUB = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).smallest_subnormal)
_F32_ZEROS = np.array([0.0, -0.0, _F32_SUB, -_F32_SUB, 1e-40, -1e-40, float(f32(0x007fffff)), -float(f32(0x007fffff)), _F32_TINY, -_F32_TINY,
                       1e-30, -1e-30, 1e-7, -1e-7])
_F32_FAR = np.array([89.0, 100.0, 1e10, float(F32_MAX), -88.0, -100.0, -1e10, -float(F32_MAX)])
_TWO_PI = 2.0 * 3.141592653589793
_F64_SUB = 5e-324


def _sincos_edges():
    k = np.round(np.array([1e5, 99999.0, 5e4, 1e3]) / (np.pi / 4))        # the octant boundaries and axis crossings nearest the domain's end
    pts = np.concatenate([_f64_around(kk * np.pi / 4, 3) for kk in np.concatenate([k, k + 1, k + 2, -k, -k - 1])])
    ends = np.concatenate([_f64_around(1e5, 3)[:4], -_f64_around(1e5, 3)[:4], [99999.5, -99999.5]])
    zeros = np.array([0.0, -0.0, _F64_SUB, -_F64_SUB, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, 1e-20, -1e-20, 1e-8, -1e-8])
    return np.concatenate([pts, ends, zeros, _f64_around(np.pi / 4, 3), _f64_around(-np.pi / 4, 3), _f64_around(np.pi / 2, 3)])


def _pymod_edges():
    lim = 2.0 ** 20 * _TWO_PI                                              # documented: |x / y| < 2^20
    k = np.array([1.0, 2.0, 3.0, 1000.0, 2.0 ** 20 - 1.0, 2.0 ** 19])
    mult = np.concatenate([_f64_around(kk * _TWO_PI, 3) for kk in k] + [-_f64_around(kk * _TWO_PI, 3) for kk in k])
    ends = np.concatenate([_f64_around(lim, 3)[:3], -_f64_around(lim, 3)[:3]])
    zeros = np.array([0.0, -0.0, _F64_SUB, -_F64_SUB, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, -1e-300, 1e-17, -1e-17])
    return np.concatenate([mult, ends, zeros])


# fn id (azo_math_eval / azg_math_selftest) -> inputs: each function's own thresholds with their neighbours, +-0, subnormals, the ends
# of its documented domain and, where the behaviour beyond it is documented (azg_expf, azg_expm1f, azg_tanhf), points far outside
MATH_EDGES = {
    0: np.concatenate([_f32_around(-87.0), _f32_around(88.0), _F32_ZEROS, _F32_FAR, _f32_around(0.5 * 0.6931471805599453), _f32_around(-0.5 * 0.6931471805599453)]),
    1: np.concatenate([_f32_around(-87.0), _f32_around(88.0), _F32_ZEROS, _F32_FAR, _f32_around(0.5 * 0.6931471805599453), _f32_around(-0.5 * 0.6931471805599453)]),
    2: np.concatenate([_f32_around(9.0), _f32_around(-9.0), _F32_ZEROS, _F32_FAR, _f32_around(44.0), [1e-4, -1e-4, 1e-3, 0.01, 0.1]]),
    3: np.concatenate([_f32_around(np.sqrt(2.0)), _f32_around(np.sqrt(2.0) * 2.0 ** -126), _f32_around(np.sqrt(2.0) * 2.0 ** 127), _f32_around(1.0),
                       _f32_around(2.0), _f32_around(0.5), _f32_around(np.sqrt(0.5)), _f32_around(_F32_TINY)[4:], _f32_around(float(F32_MAX))[:5],
                       [_F32_SUB, 1e-40, float(f32(0x007fffff))]]),
    4: np.concatenate([_f32_around(0.25), _f32_around(0.5), _f32_around(0.75), _f32_around(0.125), _f32_around(0.375), _f32_around(0.625),
                       _f32_around(0.875), _f32_around(1.0)[:4], [0.0, -0.0, _F32_SUB, 1e-40, _F32_TINY, 1e-30, 1e-7]]),
    5: _sincos_edges(), 6: _sincos_edges(), 7: _pymod_edges(),
    9: np.array([0.0, -0.0, _F32_SUB, -_F32_SUB, 1e-40, 3 * _F32_SUB, _F32_TINY, 3 * _F32_TINY, float(F32_MAX), -float(F32_MAX)]),
    10: np.array([0.0, -0.0, _F32_SUB, 1e-40, _F32_TINY, float(f32(0x007fffff)), float(F32_MAX), 1.0, 2.0]),
    11: np.array([0.0, -0.0, _F64_SUB, -_F64_SUB, 3 * _F64_SUB, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308]),
    12: np.array([0.0, -0.0, _F64_SUB, 2.2250738585072014e-308, 1.7976931348623157e308, 1.0, 2.0]),
}
# the documented domain of each function, as a mask over its edge inputs (the accuracy claim of include/azg_math.h holds there)
MATH_DOMAIN = {
    0: lambda x: (x >= -87.0) & (x <= 88.0),
    1: lambda x: x <= 88.0,                                    # (below -87 the clamp's value, e^-87 - 1, is the answer to within 1e-38)
    2: lambda x: np.isfinite(x),
    3: lambda x: x >= _F32_TINY,                               # normal positive floats
    4: lambda x: (x >= 0.0) & (x < 1.0),
    5: lambda x: np.abs(x) < 1e5, 6: lambda x: np.abs(x) < 1e5,
}
