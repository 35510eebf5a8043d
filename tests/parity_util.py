"""Shared helpers for the parity tests: rebuild an engine from a golden case, compare tree dumps."""
import ast
import os

import numpy as np

import oracle_lib as O
from alphazero_gym_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

T1_NAMES = [
    "t1_pendulum_v1_default", "t1_pendulum_v0_gamma", "t1_pendulum_v1_epsgreedy", "t1_cartpole_default",
    "t1_cartpole_epsgreedy", "t1_cartpole_explore", "t1_cartpole_reuse", "t1_mountaincar_default", "t1_mountaincar_epsgreedy_reuse",
    "t1_mcc_terminal", "t1_mcc_terminal_eps",   # MCTSContinuous with terminal nodes (MountainCarContinuous-v0; mcts.py:619-623, 682)
    "t1_acrobot_default", "t1_acrobot_epsgreedy_reuse",   # six observations, reward 0 on the terminal step (Acrobot-v1)
    # MCTSContinuous deeper than 16 levels: a chain of 40 (kappa 0), a branching tree of ~30 levels (c_pw 0.2), terminal nodes below level 16
    "t1_pendulum_v1_chain40", "t1_pendulum_v1_narrow200", "t1_mcc_chain80",
]

DUMP_INT = ("n_records", "parent", "edge_n", "node_n", "node_flags")
DUMP_F32 = ("edge_action", "node_V")
DUMP_F64 = ("edge_W", "edge_Q", "node_r")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = ast.literal_eval(str(z["case"]))
    return case, z


def engine_kwargs(case, n_trees, tree_id_base=None):
    return dict(env_id=case["env_id"], mode=case["mode"], n_trees=n_trees, n_sims=case["n_sims"], c_uct=case["c_uct"],
                gamma=case["gamma"], epsilon=case["epsilon"], num_actions=case.get("num_actions", 0), c_pw=case.get("c_pw", 1.0),
                kappa=case.get("kappa", 0.5), v_target=case["v_target"], action_bound=case.get("action_bound", 2.0),
                seed=case["seed"], tree_id_base=case.get("tree_id_base", 0) if tree_id_base is None else tree_id_base)


def case_weights(case):
    cont = case["mode"] == 1
    in_dim = (2 if case["env_id"] == 4 else 3) if cont else {3: 2, 5: 6}.get(case["env_id"], 4)
    n_dist = 2 if cont else case["num_actions"]
    blob = O.make_weights(case["wseed"], in_dim, case["hidden"], n_dist, scale=case.get("wscale", 1.0))
    return _capi.make_desc(in_dim, case["hidden"], n_dist, case["act"]), blob


def run_case(engine_cls, case, z):
    """Replay a golden T1 case on an engine class; returns a list of (results, dump, child_n) per golden row."""
    n_roots = len(case["roots"])
    steps = case.get("reuse_steps", 1)
    rows = z["root_state"].shape[0]
    out = []
    if steps == 1:
        eng = engine_cls(**engine_kwargs(case, n_roots))
        eng.set_weights(*case_weights(case))
        eng.set_search_index(case.get("search_idx", 0))
        eng.search(z["root_state"], z["carry_in"])
        res, dump = eng.results(), eng.dump_tree()
        cn, _ = eng.root_children()
        for i in range(n_roots):
            out.append(({k: v[i] for k, v in res.items()}, {k: v[i] for k, v in dump.items()}, cn[i]))
        eng.close()
    else:
        # tree reuse (MCTSDiscrete.forward): one single-tree engine per root, successive searches with the carried root count
        per_tree = rows // n_roots
        for ti in range(n_roots):
            eng = engine_cls(**engine_kwargs(case, 1, tree_id_base=case.get("tree_id_base", 0) + ti))
            eng.set_weights(*case_weights(case))
            for s in range(per_tree):
                row = ti * per_tree + s
                eng.set_search_index(case.get("search_idx", 0) + s)
                eng.search(z["root_state"][row:row + 1], z["carry_in"][row:row + 1])
                res, dump = eng.results(), eng.dump_tree()
                cn, _ = eng.root_children()
                out.append(({k: v[0] for k, v in res.items()}, {k: v[0] for k, v in dump.items()}, cn[0]))
            eng.close()
    return out


def compare_rows(out, z, float_tol=0.0, check_v_target=True):
    """Assert engine rows == golden rows.  Integers exactly; floats exactly when float_tol == 0."""
    for row, (res, dump, cn) in enumerate(out):
        nc = int(z["n_children"][row])
        assert int(res["n_children"]) == nc, (row, res["n_children"], nc)
        np.testing.assert_array_equal(res["counts"][:nc], z["counts"][row][:nc], err_msg=f"row {row} counts")
        for k in DUMP_INT:
            np.testing.assert_array_equal(dump[k], z[k][row], err_msg=f"row {row} {k}")
        np.testing.assert_array_equal(cn[:nc], z["child_n"][row][:nc], err_msg=f"row {row} child_n")
        for k in DUMP_F32 + DUMP_F64:
            if float_tol == 0.0:
                np.testing.assert_array_equal(dump[k], z[k][row], err_msg=f"row {row} {k}")
            else:
                np.testing.assert_allclose(dump[k], z[k][row], rtol=float_tol, atol=float_tol, err_msg=f"row {row} {k}")
        if float_tol == 0.0:
            np.testing.assert_array_equal(res["actions"][:nc], z["actions"][row][:nc])
            np.testing.assert_array_equal(res["Q"][:nc], z["Q"][row][:nc])
        else:
            np.testing.assert_allclose(res["actions"][:nc], z["actions"][row][:nc], rtol=float_tol, atol=float_tol)
            np.testing.assert_allclose(res["Q"][:nc], z["Q"][row][:nc], rtol=float_tol, atol=float_tol)
        if check_v_target:
            np.testing.assert_allclose(res["v_target"], z["v_target"][row], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------ the configuration matrix of the HIP parity tests
# (test_hip_parity.test_hip_bit_exact_vs_oracle: single-network engines; test_population_parity: populations of the same shapes)

CONFIGS = [
    # (env, mode, hidden, act, n_sims, extra)
    (2, 1, [256, 256], "elu", 200, dict(c_uct=0.05, gamma=1.0)),
    (2, 1, [256, 256], "elu", 64, dict(c_uct=0.3, gamma=0.97, c_pw=2.5, kappa=0.7, epsilon=0.2, v_target="on_policy")),
    (1, 1, [128, 128, 128], "elu", 90, dict(c_uct=0.1, gamma=0.99, c_pw=1.0, kappa=0.5)),
    (2, 1, [64], "relu", 50, dict(c_uct=0.05, gamma=1.0, c_pw=3.0, kappa=0.9)),
    (2, 1, [100, 60], "elu", 40, dict(c_uct=0.05, gamma=1.0)),
    (2, 1, [128, 128, 128, 128, 128], "relu", 30, dict(c_uct=0.05, gamma=1.0)),
    (0, 0, [128, 128], "relu", 100, dict(c_uct=1.5, gamma=1.0, num_actions=2)),
    (0, 0, [64, 64], "elu", 60, dict(c_uct=20.0, gamma=0.95, epsilon=0.1, num_actions=2, v_target="on_policy")),
    (0, 0, [256, 256], "relu", 80, dict(c_uct=5.0, gamma=0.99, num_actions=2)),
    # the other trunk nonlinearities
    (2, 1, [64, 64], "leakyrelu", 30, dict(c_uct=0.05, gamma=1.0)),
    (2, 1, [128, 128], "silu", 30, dict(c_uct=0.05, gamma=1.0)),
    (0, 0, [64, 64], "hardswish", 40, dict(c_uct=4.0, gamma=1.0, num_actions=2)),
    (0, 0, [64], "relu6", 40, dict(c_uct=4.0, gamma=1.0, num_actions=2)),
    # LayerNorm trunks (widths that are not multiples of 64 exercise the padded-unit mask)
    (2, 1, [100, 60], "elu", 30, dict(c_uct=0.05, gamma=1.0, _ln=True)),
    (2, 1, [256, 256], "relu", 30, dict(c_uct=0.05, gamma=1.0, _ln=True)),
    (0, 0, [128, 128, 128], "silu", 30, dict(c_uct=4.0, gamma=1.0, num_actions=2, _ln=True)),
    # Gaussian-mixture policy heads (the reference's default continuous config: 2 components, 3x128 ELU)
    (2, 1, [128, 128, 128], "elu", 60, dict(c_uct=0.05, gamma=1.0, _ncomp=2)),
    (1, 1, [64, 64], "elu", 40, dict(c_uct=0.2, gamma=0.95, c_pw=1.5, kappa=0.6, _ncomp=3)),
    # wide MLPs (BASELINE config E is 4x1024): weights streamed from L2, activation buffers up to 128 KB of LDS
    (2, 1, [512, 512], "elu", 30, dict(c_uct=0.05, gamma=1.0)),
    (2, 1, [512, 512, 512], "elu", 20, dict(c_uct=0.05, gamma=1.0, _ncomp=2)),
    (2, 1, [1024, 1024, 1024, 1024], "elu", 12, dict(c_uct=0.05, gamma=1.0)),
    (0, 0, [512], "relu", 40, dict(c_uct=3.0, gamma=1.0, num_actions=2)),
    # trees too large for LDS residency (> 255 records): global-memory tree storage
    (2, 1, [64, 64], "elu", 300, dict(c_uct=0.05, gamma=1.0)),
    (0, 0, [64, 64], "relu", 200, dict(c_uct=8.0, gamma=0.98, num_actions=2)),
    # up to 16 children per node: the LDS child-list pool grows through all its block sizes (4, 8, 16)
    (2, 1, [256, 256], "relu", 120, dict(c_uct=0.2, gamma=0.98, c_pw=1.4, kappa=0.5)),
    (1, 1, [64, 64], "elu", 254, dict(c_uct=0.02, gamma=1.0, c_pw=1.0, kappa=0.5)),
    # three actions (gym MountainCar-v0): the generic-A paths of evaluation, selection, re-scoring; LDS trees of 8- and 9-bit ids,
    # global trees, a 2x256 network (8-wave variants), a wide one (lock-step path), epsilon-greedy
    (3, 0, [64, 64], "relu", 60, dict(c_uct=0.8, gamma=0.99, num_actions=3)),
    (3, 0, [128, 128], "elu", 120, dict(c_uct=2.0, gamma=1.0, num_actions=3, epsilon=0.2, v_target="on_policy")),
    (3, 0, [256, 256], "relu", 50, dict(c_uct=1.5, gamma=0.97, num_actions=3)),
    (3, 0, [512, 512], "relu", 25, dict(c_uct=1.5, gamma=1.0, num_actions=3)),
    (3, 0, [64], "relu", 200, dict(c_uct=3.0, gamma=0.98, num_actions=3, v_target="greedy")),
    # MCTSContinuous over an env whose episodes END (gym MountainCarContinuous-v0; mcts.py:619-623, 682): terminal nodes in the continuous
    # descent -- 4-wave LDS kernels, the 8-wave shapes of 2x256 networks (lean walkers), a mixture head, a wide network (team kernel /
    # per-layer launches / one-launch kernel), trees in global memory (> 255 records), > 16 children per node
    (4, 1, [64, 64], "elu", 120, dict(c_uct=0.05, gamma=1.0, action_bound=1.0)),
    (4, 1, [256, 256], "elu", 150, dict(c_uct=0.1, gamma=0.98, epsilon=0.15, v_target="on_policy", action_bound=1.0)),
    (4, 1, [128, 128, 128], "elu", 60, dict(c_uct=0.05, gamma=1.0, action_bound=1.0, _ncomp=2)),
    (4, 1, [512, 512], "elu", 30, dict(c_uct=0.05, gamma=1.0, action_bound=1.0)),
    (4, 1, [64, 64], "relu", 300, dict(c_uct=0.05, gamma=0.99, action_bound=1.0)),
    (4, 1, [128, 128], "elu", 90, dict(c_uct=0.2, gamma=1.0, c_pw=2.0, kappa=0.6, action_bound=1.0, v_target="greedy")),
    # six observations (gym Acrobot-v1): two k-steps in the network's first layer, Runge-Kutta dynamics, reward 0 on the terminal step --
    # LDS trees of 8- and 9-bit ids, global trees, epsilon-greedy, 2x256 and a wide network (one-launch kernel: the team kernels take
    # at most four inputs), LayerNorm (weight-streaming kernels)
    (5, 0, [64, 64], "relu", 60, dict(c_uct=1.0, gamma=0.99, num_actions=3)),
    (5, 0, [128, 128], "elu", 120, dict(c_uct=2.0, gamma=1.0, num_actions=3, epsilon=0.2, v_target="on_policy")),
    (5, 0, [256, 256], "relu", 50, dict(c_uct=1.5, gamma=0.97, num_actions=3)),
    (5, 0, [512, 512], "relu", 20, dict(c_uct=1.5, gamma=1.0, num_actions=3)),
    (5, 0, [64], "relu", 200, dict(c_uct=3.0, gamma=0.98, num_actions=3, v_target="greedy")),
    (5, 0, [100, 60], "silu", 30, dict(c_uct=2.0, gamma=1.0, num_actions=3, _ln=True)),
]


# the environment variable (engine_host.h: EngineOptions) that forces each variant of the matrix
VARIANT_ENV = {"stream_weights": ("AZG_FORCE_STREAM_WEIGHTS", "1"), "global_tree": ("AZG_FORCE_GLOBAL_TREE", "1"), "waves8": ("AZG_WAVES", "8"),
               "waves4": ("AZG_WAVES", "4"), "groups2": ("AZG_GROUPS", "2"), "trace_cap1": ("AZG_TRACE_CAP", "1"),
               "trace_cap64": ("AZG_TRACE_CAP", "64"), "no_spec": ("AZG_NO_SPEC", "1"), "tile16": ("AZG_TILE_TREES", "16"),
               "tile8": ("AZG_TILE_TREES", "8"), "persistent": ("AZG_FORCE_PERSISTENT", "1"), "launches": ("AZG_LS_TEAM", "0")}


def split_config(cfg):
    """(env, mode, hidden, act, n_sims, engine extras, mixture components, layernorm) of a CONFIGS row."""
    env, mode, hidden, act, n_sims, extra = cfg
    extra = dict(extra)
    ncomp = extra.pop("_ncomp", 0)
    ln = extra.pop("_ln", False)
    return env, mode, hidden, act, n_sims, extra, ncomp, ln


def config_dims(cfg):
    """(network inputs, distribution outputs) of a CONFIGS row."""
    env, mode, _, _, _, _, ncomp, _ = split_config(cfg)
    return (2 if env == 4 else 3, 3 * ncomp if ncomp else 2) if mode == 1 else {3: (2, 3), 5: (6, 3)}.get(env, (4, 2))


def config_net(cfg, wseed, ln_seed=7):
    """(descriptor, weight blob) of a CONFIGS row's network: make_weights(wseed) at scale 2, LayerNorm parameters from ln_seed."""
    _, _, hidden, act, _, _, ncomp, ln = split_config(cfg)
    in_dim, n_dist = config_dims(cfg)
    desc = _capi.make_desc(in_dim, hidden, n_dist, act, num_components=ncomp, layernorm=ln)
    blob = O.make_weights(wseed, in_dim, hidden, n_dist, scale=2.0)
    if ln:
        blob = O.add_layernorm(blob, in_dim, hidden, n_dist, ln_seed)
    return desc, blob


def moot(cfg, variant):
    """Why a variant's path does not exist for a CONFIGS row (None: it does)."""
    env, mode, hidden, act, n_sims, extra, ncomp, ln = split_config(cfg)
    if variant in ("waves8", "waves4", "groups2"):
        if hidden != [256, 256] or ln or ncomp or mode != 1:
            return "the 8-wave workgroups exist for 2x256 squashed-Normal networks (continuous mode)"
    if variant in ("trace_cap1", "trace_cap64"):
        if mode != 0 or max(hidden) > 256:
            return "several traces per step: the discrete persistent search kernels"
    if variant == "no_spec":
        # register-resident one-layer networks with common parameters run kernels specialised at compile time (dispatch.cuh: SPEC);
        # this variant forces the general kernels on the same inputs
        # (SPEC kernels keep their trees in LDS with 8-bit ids: at most 255 records per tree -- n_sims + 2 in continuous mode, the root
        # plus two edges per evaluated node in CartPole's discrete mode; cfg0, the headline shape with its 202 records, is one of them)
        # -- and so do the team kernels of 1024-wide Pendulum-v1 networks (team_dispatch.cuh: the BASELINE config E shape)
        records = n_sims + 2 if mode == 1 else 1 + 2 * (n_sims + 1)
        one_launch = not (len(hidden) != 2 or max(hidden) > 256 or ln or ncomp or extra.get("epsilon", 0.0) != 0.0 or records > 255 or env in (3, 5))
        team = env == 2 and len(hidden) >= 2 and max(hidden) == 1024 and not ln and not ncomp and extra.get("epsilon", 0.0) == 0.0 and records <= 255
        if not (one_launch or team):
            return "no compile-time specialised kernel exists for this configuration"
    if variant in ("tile16", "tile8"):
        if max(hidden) > 128 or len(hidden) != 2 or ln or ncomp:
            return "half-filled tiles exist for register-resident networks up to 128 wide"
    if variant in ("persistent", "launches"):
        if max(hidden) <= 256:
            return "lock-step kernels only exist for hidden widths >= 512"
    return None


def upswing_roots(roots):
    """Acrobot roots on the upswing (the synthetic ones hang at rest, hundreds of steps from the episode's end)."""
    return np.stack([1.4 + 6.0 * roots[:, 0], 8.0 * roots[:, 1], 3.0 + 20.0 * roots[:, 2], 20.0 * roots[:, 3]], 1)


def slope_roots(roots):
    """MountainCarContinuous roots on the slope below the flag (the synthetic ones rest in the valley, out of the flag's reach)."""
    u = (roots[:, 0] + 0.6) / 0.2
    return np.stack([0.25 + 0.199 * u, 0.02 + 0.05 * ((17.0 * u) % 1.0)], 1)


def config_roots(env, roots):
    """A batch's synthetic roots made to reach the game's edges: Acrobot on the upswing, MountainCarContinuous on the slope, and
    hand-placed roots 3, 5, 7: a quick terminal, a wall, a flag within reach (the batch must hold at least eight trees)."""
    roots = np.array(roots, dtype=np.float64)
    if env == 0:
        roots[3] = [2.35, 1.5, 0.0, 0.0]      # terminates quickly
        roots[5] = [0.0, 0.0, 0.2, 1.0]
    if env == 3:
        roots[3] = [0.44, 0.04]               # the flag is two steps away
        roots[5] = [-1.195, -0.05]            # into the left wall
    if env == 5:
        roots = upswing_roots(roots)
        for i in range(roots.shape[0]):
            if O.env_step(5, roots[i], 1)[2] and (-np.cos(roots[i][0]) - np.cos(roots[i][1] + roots[i][0])) > 1.0:
                roots[i] = [1.0, 0.0, 0.5, 0.0]           # (already above the line)
        roots[3] = [1.9, 0.2, 2.0, 1.0]           # every torque swings the tip over the line: terminal children, reward 0
        roots[5] = [1.373, -0.681, 2.48, 1.698]   # three steps below it
        roots[7] = [0.05, -0.03, 0.02, 0.01]      # hanging at rest
    if env == 4:
        roots = slope_roots(roots)
        roots[3] = [0.44, 0.03]               # every action reaches the flag: a search of traces that end in terminal nodes
        roots[5] = [-1.195, -0.05]            # into the left wall
        roots[7] = [-0.5, 0.0]                # the valley: no terminal node within reach
    return roots
