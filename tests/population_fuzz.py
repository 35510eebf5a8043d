"""Seeded random populations with a per-net table (azg_set_net_search: settings AND simulation budgets per net): the generator, the
expected result on the CPU oracle, and the hand-made cases that put the 16-level path boundary at a different depth for each net of
one launch.  Shared by test_population_fuzz_host.py (CPU: what the seeds cover), test_population_fuzz.py (GPU: bit for bit) and the
soak fuzz_population.py; numpy and the CPU oracle only.

case(seed) draws everything from PCG64(5000 + seed).  Network, env and mode are test_hip_parity._random_case's (one fuzz space for
single nets and populations), with re-weightings the single-net space has no use for -- half of the capacities below 7 are drawn
again from {33, 64, 120} (a budget needs room below the capacity), a fifth of the cases takes a wide shape (padded width 512 / 1024:
the three wide table kernels), and a forced variant whose path the drawn shape does not have mostly re-shapes the net to one that
has it (2x256 for the 8-wave workgroups, 2x64 / 2x128 for half-filled tiles, a lock-step shape for the per-layer launches) -- and
clamps that keep a case quick on the oracle: capacity <= 120, wide nets <= two hidden layers and capacity <= 24.  Then K nets x T
trees, a table entry per net (c_uct, gamma, epsilon, widening law, budget), one forced kernel variant, roots, carried counts, a
search index and a tree id base.  The engine is created with the case's own law at capacity; a net's law is re-drawn while its Kmax
AT ITS OWN BUDGET exceeds the engine's (engine_weights.hip: set_net_search counts the same).  The weights below were set so that the
48 seeds meet test_population_fuzz_host.py's coverage conditions."""
import types

import numpy as np

import deep_paths as D
import edge_values as E
import net_rollouts_util as R
import net_search_util as N
import net_search_wide_util as NW
import oracle_lib as O
import parity_util as P
from alphazero_gym_amd import _capi

SEEDS = range(48)                       # the suite's seeds (the soak runs beyond them)
SECOND_SEARCH = 8                       # seeds that search twice, budgets rotated by one net
KS, TS = [1, 2, 3, 4, 6, 9], [1, 5, 16, 17, 33]
KS_LOCKSTEP, TS_LOCKSTEP = [1, 2, 3], [32, 64]      # a multiple of 32 trees per lock-step shaped net (one or two teams)
VARIANTS = ["default", "global_tree", "stream_weights", "waves8", "groups2", "tile8", "trace_cap1", "launches", "persistent"]
VARIANT_WEIGHTS = [0.12, 0.09, 0.09, 0.10, 0.10, 0.10, 0.14, 0.08, 0.18]     # (trace_cap1 and persistent lose half their draws to the mode and the env)
CHAIN = (1.0, 0.0)
GAMES = {0: "CartPole-v0", 1: "Pendulum-v0", 2: "Pendulum-v1", 3: "MountainCar-v0", 4: "MountainCarContinuous-v0", 5: "Acrobot-v1"}
CAP, CAP_WIDE = 120, 24
# (hidden, act, layernorm, mixture components in continuous mode): the wide shapes of parity_util.CONFIGS and test_population_wide,
# at most two hidden layers
WIDE_SHAPES = [([512, 512], "elu", False, 0), ([512], "relu", False, 0), ([1024, 1024], "elu", False, 0), ([512, 512], "elu", True, 0),
               ([512, 512], "elu", False, 2), ([1024], "relu", False, 0), ([512, 512], "relu", False, 0)]


def _random_case(rng):
    import test_hip_parity as HP        # (a GPU test module: imported for its generator only)
    return HP._random_case(rng)


def wider(law):
    """The pool's pair wider than the case's own: twice the children at every count."""
    return (2.0 * law[0], law[1])


def _segment_roots(env, seg):
    """One net's roots, made to reach the game's edges: parity_util.config_roots where the segment holds its hand-placed roots (eight
    trees), else the single-net fuzz's roots with one hand-placed root that reaches a terminal node within two or three steps."""
    T = seg.shape[0]
    if T >= 8:
        return P.config_roots(env, seg)
    seg = np.array(seg, dtype=np.float64)
    if env == 4:
        seg = P.slope_roots(seg)
    if env == 5:
        seg = P.upswing_roots(seg)
        for i in range(T):
            if (-np.cos(seg[i][0]) - np.cos(seg[i][1] + seg[i][0])) > 0.98:
                seg[i] = [1.0, 0.0, 0.5, 0.0]
    j = min(3, T - 1)
    if env == 0:
        seg[j] = [2.35, 1.5, 0.0, 0.0]
    if env == 4:
        seg[j] = [0.44, 0.03]
    return seg


def _budget(rng, cap):
    """One of the classes 0 (the engine's), 1, 2, capacity - 1, capacity, uniform -- as the value the ABI takes, in 0 .. capacity."""
    cls = int(rng.integers(0, 6))
    b = [0, 1, 2, cap - 1, cap, int(rng.integers(1, cap + 1))][cls]
    return min(max(b, 0), cap)


def _no_path(env, mode, hidden, act, ln, ncomp, extra, variant):
    """Why the forced variant would only re-run the default's kernel (None: its path exists): parity_util.moot, and the rules of
    test_population_wide's matrix -- wide nets stream their weights anyway, and only lock-step shaped ones leave the search kernel."""
    if variant == "default":
        return None
    cfg = (env, mode, list(hidden), act, 0, dict(extra, _ncomp=ncomp, _ln=ln))
    wide = max(hidden) >= 512
    if wide and variant == "stream_weights":
        return "wide nets stream their weights"
    if wide and not NW.lockstep_shaped(cfg) and variant in ("launches", "persistent"):
        return "not lock-step shaped"
    return P.moot(cfg, variant)


def case(seed):
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    env, mode, hidden, act, ln, n_sims, extra, ncomp, in_dim, n_dist = _random_case(rng)
    # re-weightings (module docstring): small capacities, wide shapes, and -- with the variant drawn first -- the variant's home shape
    if n_sims < 7 and rng.random() < 0.5:
        n_sims = int(rng.choice([33, 64, 120]))
    if rng.random() < 0.2:
        hidden, act, ln, ncomp = WIDE_SHAPES[int(rng.integers(0, len(WIDE_SHAPES)))]
        ncomp = ncomp if mode == 1 else 0
    variant = str(rng.choice(VARIANTS, p=VARIANT_WEIGHTS))
    if _no_path(env, mode, hidden, act, ln, ncomp, extra, variant) and rng.random() < 0.75:
        if variant in ("waves8", "groups2") and mode == 1:
            hidden, ln, ncomp = [256, 256], False, 0
        elif variant == "tile8":
            hidden, ln, ncomp = [int(rng.choice([64, 128]))] * 2, False, 0
        elif variant == "trace_cap1" and mode == 0:
            hidden = [128, 128]
        elif variant in ("launches", "persistent") and env != 5:
            hidden, act, ln = [int(rng.choice([512, 1024]))] * 2, "elu", False
    hidden = list(hidden)
    if mode == 1:
        n_dist = 3 * ncomp if ncomp else 2
    wide = max(hidden) >= 512
    cap = min(n_sims, CAP_WIDE if wide else CAP)
    extra = dict(extra)
    cfg = (env, mode, hidden, act, cap, dict(extra, _ncomp=ncomp, _ln=ln))
    lockstep = wide and NW.lockstep_shaped(cfg)
    if _no_path(env, mode, hidden, act, ln, ncomp, extra, variant):
        variant = "default"             # the variant's path does not exist for the shape

    K = int(rng.choice(KS_LOCKSTEP if lockstep else KS))
    T = int(rng.choice(TS_LOCKSTEP if lockstep else TS))

    own = (extra["c_pw"], extra["kappa"]) if mode == 1 else None
    kmax = N.kmax_of(dict(c_pw=own[0], kappa=own[1]), cap) if mode == 1 else 0

    # budgets: a class per net, with K >= 3 now and then a duplicate, then the largest moved to a drawn position
    raw = [_budget(rng, cap) for _ in range(K)]
    if K >= 3 and rng.random() < 0.4:
        a, b = rng.choice(K, 2, replace=False)
        raw[int(a)] = raw[int(b)]
    eff = [b if b else cap for b in raw]
    top, pos = int(np.argmax(eff)), int(rng.integers(0, K))
    raw[top], raw[pos] = raw[pos], raw[top]
    sims = [b if b else cap for b in raw]

    # settings
    pool = [own, N.NARROW_PW, CHAIN, wider(own)] if mode == 1 else None
    settings, redraws = [], 0
    for k in range(K):
        s = dict(c_uct=extra["c_uct"] * float(rng.choice([0.25, 1.0, 4.0])), gamma=float(rng.choice([1.0, 0.97, 0.9])),
                 epsilon=float(rng.choice([0.0, 0.25])))
        if mode == 1:
            law = pool[int(rng.integers(0, 4))]
            while N.kmax_of(dict(c_pw=law[0], kappa=law[1]), sims[k]) > kmax:
                law = pool[int(rng.integers(0, 4))]
                redraws += 1
                assert redraws <= 20, (seed, k, law, sims[k], kmax)
            s.update(c_pw=float(law[0]), kappa=float(law[1]))
        settings.append(s)
    if K >= 2 and all(s == settings[0] for s in settings):
        settings[1]["gamma"] = 0.9 if settings[0]["gamma"] != 0.9 else 0.97

    kw = dict(env_id=env, mode=mode, n_trees=K * T, n_sims=cap, seed=int(rng.integers(1, 1 << 30)), tree_id_base=int(rng.integers(0, 1000)), **extra)
    desc = _capi.make_desc(in_dim, hidden, n_dist, act, num_components=ncomp, layernorm=ln)
    wseed, scale = int(rng.integers(1, 1000)), float(rng.choice([1.0, 2.0, 3.0]))
    blobs = []
    for k in range(K):
        blob = O.make_weights(wseed + k, in_dim, hidden, n_dist, scale=scale)
        blobs.append(O.add_layernorm(blob, in_dim, hidden, n_dist, 7 + k) if ln else blob)
    o = O.OracleEngine(**kw)
    roots = np.array(o.synthetic_roots(), dtype=np.float64)
    o.close()
    roots = np.concatenate([_segment_roots(env, roots[k * T:(k + 1) * T]) for k in range(K)])
    carry = (np.arange(K * T) % 5).astype(np.int32) if mode == 0 else None
    sidx = int(rng.integers(0, 50))
    return types.SimpleNamespace(seed=seed, env=env, mode=mode, hidden=hidden, act=act, ln=ln, ncomp=ncomp, in_dim=in_dim, n_dist=n_dist, cap=cap,
                                 wide=wide, lockstep=lockstep, K=K, T=T, variant=variant, own=own, kmax=kmax, budgets=raw, sims=sims,
                                 settings=settings, redraws=redraws, kw=kw, cfg=cfg, desc=desc, blobs=blobs, roots=roots, carry=carry, sidx=sidx,
                                 wseed=wseed, scale=scale)


def describe(c):
    return (f"seed {c.seed}: env {c.env} {'x'.join(map(str, c.hidden))} {c.act}{' ln' if c.ln else ''}{f' gmm{c.ncomp}' if c.ncomp else ''} "
            f"cap {c.cap} K={c.K} T={c.T} budgets {c.budgets} {c.variant}{' random-tie' if c.kw.get('tie_break') == 'random' else ''}")


def table(c, settings=None):
    return [N.full(s) for s in (c.settings if settings is None else settings)]


def law_of(s):
    return (s["c_pw"], s["kappa"])


def oracle(c, settings=None, sims=None, sidx=None):
    """What the population must compute: net k on an oracle engine CREATED with its settings and its budget (net_rollouts_util)."""
    return R.oracle_nets(c.kw, c.desc, c.blobs, c.roots, c.carry, c.sidx if sidx is None else sidx, c.settings if settings is None else settings,
                         c.sims if sims is None else sims, width=c.kmax if c.mode == 1 else None)


def rotated(c):
    """(budgets as the ABI takes them, effective budgets) rotated by one net, or None where a net's law would not fit its new budget."""
    raw = c.budgets[-1:] + c.budgets[:-1]
    sims = c.sims[-1:] + c.sims[:-1]
    if c.mode == 1 and any(N.kmax_of(s, n) > c.kmax for s, n in zip(c.settings, sims)):
        return None
    return raw, sims


def second_search_seeds():
    """The first SECOND_SEARCH seeds of two or more nets whose budgets differ and still fit when rotated."""
    out = []
    for seed in SEEDS:
        c = case(seed)
        if c.K >= 2 and len(set(c.sims)) > 1 and rotated(c) is not None:
            out.append(seed)
        if len(out) == SECOND_SEARCH:
            break
    return out


# ------------------------------------------------------------------------------------------- budgets across the 16-level boundary
# Four nets under the chain law (a tree of n simulations IS a path of n levels: deep_paths.py), budgets 15, 16, 17 and 33 at capacity
# 40: in one launch a net whose paths stay inside the 16 levels a tree's lanes hold, one that fills them, one that hands the 16th
# return over to backup_from, and one that takes backup_from's second round.

BOUNDARY_SIMS, BOUNDARY_CAP = [15, 16, 17, 33], 40
# name -> (deep_paths shape, trees per net, forced variant)
BOUNDARY = {"p64-lds": ("p64", 19, "default"), "p64-global_tree": ("p64", 19, "global_tree"), "p512-team": ("p512", 32, "default"),
            "p512-launches": ("p512", 32, "launches"), "p512-persistent": ("p512", 32, "persistent")}


def boundary_case(name):
    """(engine kwargs, descriptor, blobs, roots, settings, budgets, trees per net, variant)."""
    shape, T, variant = BOUNDARY[name]
    nets = len(BOUNDARY_SIMS)
    cases = [D.case(shape, "chain", BOUNDARY_CAP, trees=T, tree_id_base=D.BASE + k * T, wseed=D.SHAPES[shape]["wseed"] + 100 * k) for k in range(nets)]
    kw = dict(cases[0][0], n_trees=nets * T, tree_id_base=D.BASE)
    gammas = [0.99, 1.0, 0.97, 0.99]
    settings = [dict(c_uct=kw["c_uct"], gamma=g, epsilon=0.0, c_pw=CHAIN[0], kappa=CHAIN[1]) for g in gammas]
    return kw, cases[0][1], [c[2] for c in cases], np.concatenate([c[3] for c in cases]), settings, list(BOUNDARY_SIMS), T, variant


def boundary_oracle(name):
    kw, desc, blobs, roots, settings, sims, T, _ = boundary_case(name)
    return R.oracle_nets(kw, desc, blobs, roots, None, D.SIDX, settings, sims, width=1)


def boundary_traces(name):
    """Per net: the leaf depths of every trace of every tree, from a one-net oracle engine created with the net's budget."""
    kw, desc, blobs, roots, settings, sims, T, _ = boundary_case(name)
    out = []
    for k, n in enumerate(sims):
        own = dict(kw, n_trees=T, tree_id_base=kw["tree_id_base"] + k * T, n_sims=n, **settings[k])
        out.append(np.concatenate(D.leaf_depths(E.run_engine(O.OracleEngine, own, desc, blobs[k], roots[k * T:(k + 1) * T], None, sidx=D.SIDX, trace=True))))
    return out


# The discrete counterpart: edge_values.population_case("cartpole") -- the CartPole setup of edge_values.discrete_device_cases whose
# trees follow the balancing line one node deeper per trace (sharp priors), three nets of 19 trees, capacity 100.  The budgets come from
# the oracle's leaf depths at capacity: net 0 gets the most simulations after which no trace of its trees has a leaf at level 16 or
# deeper, net 1 the fewest after which some trace of its trees has one at level 17 or deeper, net 2 the capacity.

def discrete_boundary_case():
    kw, desc, blobs, roots, carry = E.population_case("cartpole")
    full = E.oracle_population("cartpole")
    T, cap = E.POP_T, kw["n_sims"]

    def depth_by_sim(run):       # [T, n_sims]: the leaf depth of simulation s of tree t
        return np.stack(D.leaf_depths(run))

    d0, d1 = depth_by_sim(full[0]), depth_by_sim(full[1])
    below = int(np.argmax((d0 >= 16).any(axis=0)))                  # the first simulation with a leaf at level >= 16: that many fit below
    beyond = int(np.argmax((d1 >= 17).any(axis=0))) + 1
    assert (d0 >= 16).any() and (d1 >= 17).any() and 2 <= below < beyond <= cap, (below, beyond)
    c = kw["c_uct"]
    settings = [dict(c_uct=c, gamma=1.0, epsilon=0.0), dict(c_uct=c, gamma=0.97, epsilon=0.0), dict(c_uct=c, gamma=1.0, epsilon=0.0)]
    return kw, desc, blobs, roots, carry, settings, [below, beyond, cap], T


def discrete_boundary_traces():
    kw, desc, blobs, roots, carry, settings, sims, T = discrete_boundary_case()
    out = []
    for k, n in enumerate(sims):
        own = dict(kw, n_trees=T, tree_id_base=kw["tree_id_base"] + k * T, n_sims=n, **settings[k])
        sl = slice(k * T, (k + 1) * T)
        out.append(np.concatenate(D.leaf_depths(E.run_engine(O.OracleEngine, own, desc, blobs[k], roots[sl], carry[sl], sidx=3, trace=True))))
    return out


def discrete_boundary_oracle():
    kw, desc, blobs, roots, carry, settings, sims, T = discrete_boundary_case()
    return R.oracle_nets(kw, desc, blobs, roots, carry, 3, settings, sims)


# ------------------------------------------------------------------------------------------------------------------- self-play
# Six seeds of the generator (beyond the suite's 48, narrow nets, capacity clamped to 24) chosen so that Acrobot,
# MountainCarContinuous, T == 1 and K == 6 occur; each draws its own final action rule from PCG64(6000 + seed).

SELFPLAY_CAP, SELFPLAY_STEPS, SELFPLAY_MAX_LEN = 24, 4, 3
# 61: MountainCarContinuous, K 6, T 1, on_policy, max_value; 97: Pendulum-v0 with LayerNorm, T 1; 106: CartPole, K 6, temperature 2;
# 170: Acrobot, K 6, max_value; 212: Pendulum-v1 2x256, K 6; 240: MountainCar, K 6, temperature 2
SELFPLAY_SEEDS = [61, 97, 106, 170, 212, 240]


def selfplay_case(seed):
    """A self-play population from case(seed): game, K, T, the nets' shape, capacity min(the case's, 24), every net's settings and
    budget (clamped to the capacity), and the agents' rule."""
    c = case(seed)
    assert not c.wide
    rng = np.random.Generator(np.random.PCG64(6000 + seed))
    cap = min(c.cap, SELFPLAY_CAP)
    sims = [min(n, cap) for n in c.sims]
    settings = [dict(s) for s in c.settings]        # (PopulationMCTS creates the engine with the widest of the nets' laws)
    # (the temperature belongs to the discrete max_visit rule: the device's max_value takes 1 only, continuous agents have none)
    rule = dict(final_selection=str(rng.choice(["max_visit", "max_value"])), temperature=float(rng.choice([1.0, 0.5, 2.0])))
    if rule["final_selection"] == "max_value" or c.mode == 1:
        rule["temperature"] = 1.0
    shared = dict(c_uct=c.kw["c_uct"], gamma=c.kw["gamma"], epsilon=c.kw["epsilon"])
    if c.mode == 1:
        shared.update(c_pw=c.own[0], kappa=c.own[1])
    return types.SimpleNamespace(seed=seed, case=c, game=GAMES[c.env], K=c.K, T=c.T, cap=cap, sims=sims, settings=settings, rule=rule, shared=shared,
                                 v_target=c.kw["v_target"], engine_seed=c.kw["seed"] % 100000, action_bound=c.kw.get("action_bound", 2.0))


def selfplay_policies(sp, device):
    """K torch policies of the case's shape, seeded by the case."""
    import torch
    from alphazero_gym_amd.network.policies import make_policy
    c = sp.case
    nets = []
    for k in range(sp.K):
        torch.manual_seed(c.wseed + k)
        if c.mode == 1:
            pol = make_policy(representation_dim=c.in_dim, action_dim=1, distribution="normal", hidden_dimensions=c.hidden, nonlinearity=c.act,
                              num_components=max(c.ncomp, 1), action_bound=sp.action_bound, layernorm=c.ln)
        else:
            pol = make_policy(representation_dim=c.in_dim, action_dim=1, distribution="discrete", hidden_dimensions=c.hidden, nonlinearity=c.act,
                              num_actions=c.n_dist, layernorm=c.ln)
        nets.append(pol.to(device))
    return nets
