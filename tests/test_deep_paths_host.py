"""CPU: continuous searches deeper than 16 levels (tests/deep_paths.py) on the oracle alone -- the conditions every case of
tests/test_deep_paths.py must meet before the device is compared with it, the oracle's deep backup against an independent float64
replay in numpy, and what the three deep golden fixtures (captured from the reference) contain.

The oracle itself is held to the reference on these paths by tests/test_oracle_golden.py through parity_util.T1_NAMES."""
import numpy as np
import pytest

import deep_paths as D
import edge_values as E
import net_search_util as N
import oracle_lib as O
import parity_util as P


@pytest.mark.parametrize("cid", sorted(D.CASES))
def test_case_conditions(cid):
    """Leaf depths <= 15, == 16, >= 17 and >= 33; CHAIN: one child per node, one result column, the
    deepest leaf at n_sims; NARROW: a branching node below the root on a path of 17 or more levels; MountainCarContinuous: a terminal
    node at depth >= 17 that later traces end in; and every edge's W and Q equal to the float64 replay, bit for bit."""
    shape, law, n_sims, opts = D.CASES[cid]
    fig = D.check_conditions(cid, D.oracle(shape, law, n_sims, **opts))
    print(cid, fig)


@pytest.mark.parametrize("shape", D.POP_SHAPES)
def test_population_case_conditions(shape):
    """Each net of the three-net launch on its own oracle engine: the same conditions per net, and three different trees."""
    outs = D.oracle_population(shape)
    for out in outs:
        D.check_run(out, "chain", D.POP_SIMS, 0.99)
    assert len({o["dump"]["edge_W"].tobytes() for o in outs}) == D.POP_K


def test_net_search_case_conditions():
    """One launch, three laws: net 0's trees are 120-deep chains, net 1's (c_pw 1, kappa 0.5) stay within the lanes' 16 levels, net 2's
    (NARROW) lie between.  The engine's own law is the widest of the three.  Nets 0 and 2 meet the conditions of every other case
    (leaf depths, children, the float64 replay) on one-net oracle engines with their own settings, whose trees are the ones
    net_search_util.oracle_nets hands to the device comparison."""
    kw, desc, blobs, roots, settings = D.net_search_case()
    res, dump, _ = N.oracle_nets(kw, desc, blobs, roots, None, D.SIDX, settings, width=N.kmax_of(settings[1], D.NET_SIMS))
    T = D.POP_T
    deepest = [max(int(E.depths(dump["parent"][t], dump["n_records"][t]).max()) for t in range(k * T, (k + 1) * T)) for k in range(D.POP_K)]
    print("deepest record per net", deepest)
    assert deepest[0] == D.NET_SIMS and deepest[1] <= 15 and deepest[0] > deepest[2] > deepest[1]
    assert (res["n_children"][:T] == 1).all() and (res["n_children"][T:2 * T] == N.kmax_of(settings[1], D.NET_SIMS)).all()
    assert N.kmax_of(settings[1], D.NET_SIMS) == max(N.kmax_of(s, D.NET_SIMS) for s in settings) == res["counts"].shape[1]
    for k, law in ((0, "chain"), (2, "narrow")):
        out = D.oracle_net(k)
        print("net", k, D.check_run(out, law, D.NET_SIMS, D.NET_GAMMAS[k]))
        for key in out["dump"]:
            assert out["dump"][key].tobytes() == dump[key][k * T:(k + 1) * T].tobytes(), (k, key)


def test_every_family_has_device_cases():
    """The GPU file's parameters come from these tables: none of them may be empty, every shape and every form must occur."""
    cases = D.device_cases()
    assert len({c[0] for c in cases}) == len(cases) >= len(D.CASES)
    assert {c[1] for c in cases} == set(D.CASES)
    for shape, forms in D.FORMS.items():
        assert {f for _, cid, f in cases if D.CASES[cid][0] == shape} == set(forms), shape
    laws = {D.CASES[cid][1] for _, cid, _ in cases}
    assert laws == set(D.LAWS)
    assert D.POP_SHAPES and D.POP_K == 3 and len(D.NET_LAWS) == D.POP_K
    for cid, (shape, law, n_sims, opts) in D.CASES.items():
        assert D.kmax_of(law, n_sims) == (1 if law == "chain" else 2 if n_sims < 178 else 3), cid     # (0.15 sqrt(178) > 2)
    # no listed form is moot for its shape (parity_util.moot): a moot form would be asserted around, not run
    for _, cid, form in cases:
        shape, law, n_sims, opts = D.CASES[cid]
        sh = D.SHAPES[shape]
        extra = dict(c_uct=0.05, gamma=1.0, epsilon=opts.get("epsilon", 0.0))
        if sh.get("ncomp"):
            extra["_ncomp"] = sh["ncomp"]
        if sh.get("ln"):
            extra["_ln"] = True
        if form != "default":
            assert P.moot((sh["env_id"], 1, list(sh["hidden"]), "elu", n_sims, extra), form) is None, (cid, form)


def test_selfplay_case_plays_from_one_child_roots():
    """The device self-play case on the oracle: every replay row holds one child with all the visits."""
    rows, stats = D.selfplay_play(O.OracleEngine)
    kw = D.SELFPLAY["kw"]
    assert rows.shape == (D.SELFPLAY["steps"] * D.SELFPLAY["games"], 3 + 3 * 1 + 1)      # observation, action, count, Q, value target
    assert (rows[:, 3 + 1] == float(kw["n_sims"])).all()


# ------------------------------------------------------------------------------------------------ the golden fixtures

GOLDEN = {"t1_pendulum_v1_chain40": D.CHAIN, "t1_pendulum_v1_narrow200": D.GOLDEN_NARROW, "t1_mcc_chain80": D.CHAIN}


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_deep_goldens_are_deep(name):
    """What the reference's own trees hold (the fixture alone, no engine): the chain of 40, a branching tree beyond 16 and beyond 24
    levels, MountainCarContinuous terminal nodes at depth >= 17 with most of the tree's traces ending in them."""
    assert name in P.T1_NAMES
    case, z = P.load_case(name)
    assert (case["c_pw"], case["kappa"]) == GOLDEN[name] and case["c_pw"] <= 1
    deepest, deep_term = [], 0
    for row in range(z["parent"].shape[0]):
        n = int(z["n_records"][row])
        d = E.depths(z["parent"][row], n)
        deepest.append(int(d.max()))
        kids = np.bincount(z["parent"][row][1:n], minlength=n)
        if GOLDEN[name] == D.CHAIN:
            assert (kids[:n - 1] == 1).all() and z["counts"].shape[1] == 1
        else:
            assert ((kids >= 2) & (d >= 1)).any()
        term = np.nonzero((z["node_flags"][row][:n] & 2) != 0)[0]
        for j in term:
            # every trace that does not create a record ends in the terminal node: n_sims - (n - 1) of them
            if d[j] >= 17 and case["n_sims"] - (n - 1) >= 2:
                deep_term += 1
    print(name, "deepest record per tree", deepest)
    if name == "t1_pendulum_v1_chain40":
        assert deepest == [40] * len(deepest) and case["gamma"] == 0.99
    if name == "t1_pendulum_v1_narrow200":
        assert min(deepest) >= 24
    if name == "t1_mcc_chain80":
        assert deep_term >= 2 and max(deepest) == 80
