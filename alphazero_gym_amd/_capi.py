"""ctypes binding of the C ABI declared in include/azgym.h.

``Engine`` wraps one ``azg_engine*``.  The symbol prefix is a parameter only so that the test-suite can
bind the CPU oracle (prefix ``azo_``) through the same code; the product always binds ``azg_`` from
``csrc/libazgym_hip.so`` (see ``_native.py``).
"""
import ctypes as C
import math

import numpy as np

ABI_VERSION = 1

AZG_OK = 0
AZG_E_INVALID = -1
AZG_E_TERMINAL_ROOT = -2
AZG_E_DEVICE = -3
AZG_E_STATE = -4
AZG_E_UNSUPPORTED = -5

ENV_CARTPOLE, ENV_PENDULUM_V0, ENV_PENDULUM_V1, ENV_MOUNTAINCAR, ENV_MOUNTAINCAR_CONT, ENV_ACROBOT = 0, 1, 2, 3, 4, 5
MODE_DISCRETE, MODE_CONTINUOUS = 0, 1
VT = {"off_policy": 0, "on_policy": 1, "greedy": 2}
TIE = {"first": 0, "random": 1}   # helpers.argmax on exactly equal scores: lowest index (parity) or a Philox-keyed uniform pick
ACT = {"relu": 0, "elu": 1, "leakyrelu": 2, "relu6": 3, "silu": 4, "swish": 4, "hardswish": 5}
_ACT_MODULES = {"ReLU": 0, "ELU": 1, "LeakyReLU": 2, "ReLU6": 3, "SiLU": 4, "Hardswish": 5}
MAX_HIDDEN = 8

PENDULUM_R_SCALE = 16.2736044  # alphazero/search/mcts.py:20


class AzgConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("device_id", C.c_int32),
        ("env_id", C.c_int32),
        ("mode", C.c_int32),
        ("n_trees", C.c_int32),
        ("n_sims", C.c_int32),
        ("num_actions", C.c_int32),
        ("v_target", C.c_int32),
        ("tree_id_base", C.c_int32),
        ("tie_break", C.c_int32),
        ("c_uct", C.c_double),
        ("gamma", C.c_double),
        ("epsilon", C.c_double),
        ("c_pw", C.c_double),
        ("kappa", C.c_double),
        ("reward_scale", C.c_double),
        ("action_bound", C.c_double),
        ("seed", C.c_uint64),
    ]


class AzgMlpDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("in_dim", C.c_int32),
        ("n_hidden", C.c_int32),
        ("hidden", C.c_int32 * MAX_HIDDEN),
        ("n_dist", C.c_int32),
        ("activation", C.c_int32),
        ("log_std_min", C.c_float),
        ("log_std_max", C.c_float),
        ("num_components", C.c_int32),
        ("layernorm", C.c_int32),
    ]


class AzgSelfplayConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("max_episode_length", C.c_int32),
        ("deterministic", C.c_int32),
        ("capacity_steps", C.c_int32),
        ("final_selection", C.c_int32),
        ("ring_mode", C.c_int32),
        ("temperature", C.c_double),
        ("agent_epsilon", C.c_double),
    ]


class AzgRolloutConfig(C.Structure):
    """include/azgym_eval.h: azg_rollout_config"""
    _fields_ = [("struct_size", C.c_int32), ("episodes_per_net", C.c_int32), ("max_episode_length", C.c_int32),
                ("action_rule", C.c_int32), ("game_id_base", C.c_uint32), ("episode", C.c_uint32)]


class AzgRolloutInfo(C.Structure):
    """include/azgym_eval.h: azg_rollout_info"""
    _fields_ = [("struct_size", C.c_int32), ("form", C.c_int32), ("launches", C.c_int32), ("team_fallbacks", C.c_int32)]


class AzgEvalInfo(C.Structure):
    """include/azgym_eval.h: azg_eval_info"""
    _fields_ = [("struct_size", C.c_int32), ("resident", C.c_int32), ("groups", C.c_int32), ("tiles", C.c_int32)]


class AzgNstepConfig(C.Structure):
    """include/azgym_nstep.h: azg_nstep_config"""
    _fields_ = [("struct_size", C.c_int32), ("n_step", C.c_int32), ("gamma", C.c_double), ("flags", C.c_int32)]


class AzgReturnRule(C.Structure):
    """include/azgym_lambda.h: azg_return_rule"""
    _fields_ = [("struct_size", C.c_int32), ("n_step", C.c_int32), ("lambda_", C.c_double), ("gamma", C.c_double), ("flags", C.c_int32)]


NSTEP_SEARCH_GAMMA = 1   # AZG_NSTEP_SEARCH_GAMMA: discount with the search's own gamma (the row's net's where a per-net table is set)
END_NONE, END_TERMINAL, END_LENGTH = 0, 1, 2   # AZG_END_*: how a stored self-play step ended


class AzgPriorityConfig(C.Structure):
    """include/azgym_priority.h: azg_priority_config"""
    _fields_ = [("struct_size", C.c_int32), ("source", C.c_int32), ("alpha", C.c_float), ("eps", C.c_float),
                ("given", C.POINTER(C.c_float))]


class AzgSampleConfig(C.Structure):
    """include/azgym_priority.h: azg_sample_config"""
    _fields_ = [("struct_size", C.c_int32), ("n_order", C.c_int32), ("sample_index", C.c_uint32)]


PRIO_VALUE_GAP, PRIO_GIVEN = 0, 1   # AZG_PRIO_*: a row's priority from |search value - V_target|, or from the caller's array


class AzgTrainedPriorityConfig(C.Structure):
    """include/azgym_priority.h: azg_trained_priority_config"""
    _fields_ = [("struct_size", C.c_int32), ("unseen", C.c_int32), ("alpha", C.c_float), ("eps", C.c_float), ("unseen_d", C.c_float)]


UNSEEN_MAX, UNSEEN_VALUE_GAP, UNSEEN_CONSTANT = 0, 1, 2   # AZG_UNSEEN_*: the d of a row never trained on since it was stored
ERR_UNSEEN = np.float32(-1.0)                             # ... and its entry in the kept errors


def trained_priority_config(alpha, eps, unseen="max"):
    """azg_trained_priority_config of (alpha, eps) and an ``unseen`` setting (``unseen_mode``)."""
    c = AzgTrainedPriorityConfig()
    c.struct_size = C.sizeof(AzgTrainedPriorityConfig)
    c.unseen, c.unseen_d = unseen_mode(unseen)
    c.alpha, c.eps = float(alpha), float(eps)
    return c


class AzgOnlineEpoch(C.Structure):
    """include/azgym_train_online.h: azg_online_epoch"""
    _fields_ = [("struct_size", C.c_int32), ("n_minibatches", C.c_int32), ("batch_size", C.c_int32), ("sample_index", C.c_uint32),
                ("beta", C.c_float), ("prio", AzgTrainedPriorityConfig), ("drawn", C.POINTER(C.c_int32))]


def unseen_mode(feedback):
    """(AZG_UNSEEN_*, unseen_d) of a ``feedback`` setting: "max", "value_gap" or a finite number >= 0 (the constant d)."""
    if isinstance(feedback, str):
        modes = {"max": UNSEEN_MAX, "value_gap": UNSEEN_VALUE_GAP}
        if feedback not in modes:
            raise ValueError(f"feedback: \"max\", \"value_gap\" or a number >= 0, got {feedback!r}")
        return modes[feedback], 0.0
    if isinstance(feedback, bool) or not isinstance(feedback, (int, float, np.integer, np.floating)):
        raise ValueError(f"feedback: \"max\", \"value_gap\" or a number >= 0, got {feedback!r}")
    d = float(feedback)
    if not (d >= 0.0 and np.isfinite(d)):
        raise ValueError(f"feedback: the constant d of unseen rows must be finite and >= 0, got {feedback!r}")
    return UNSEEN_CONSTANT, d


class AzgSearchRolloutConfig(C.Structure):
    """include/azgym_search_rollout.h: azg_search_rollout_config"""
    _fields_ = [("struct_size", C.c_int32), ("episodes_per_game", C.c_int32), ("max_episode_length", C.c_int32),
                ("final_selection", C.c_int32), ("deterministic", C.c_int32), ("poll_steps", C.c_int32),
                ("game_id_base", C.c_uint32), ("episode", C.c_uint32), ("index_base", C.c_uint32),
                ("temperature", C.c_double), ("agent_epsilon", C.c_double)]


class AzgSearchRolloutInfo(C.Structure):
    """include/azgym_search_rollout.h: azg_search_rollout_info"""
    _fields_ = [("struct_size", C.c_int32), ("steps", C.c_int32), ("polls", C.c_int32)]


ROLLOUT_RULE = {"mode": 0, "sample": 1}   # include/azgym_eval.h: AZG_ROLLOUT_*
ROLLOUT_FORM = {0: "group", 1: "team"}    # include/azgym_eval.h: AZG_ROLLOUT_FORM_*
FINAL_SELECTION = {"max_visit": 0, "max_visits": 0, "max_value": 1}   # the reference's configs spell it both ways


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"azgym error {code}: {msg}")
        self.code = code


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


SYMBOLS = [
    "abi_version", "engine_create", "engine_destroy", "last_error", "set_weights", "set_weights_device", "set_search_index", "search",
    "results", "results_resident", "root_children", "root_eval", "dump_tree", "max_children", "max_records", "env_state_dim", "obs_dim",
    "synthetic_roots", "last_search_ms", "upload_roots", "search_resident", "sync",
    "selfplay_begin", "selfplay_begin_ex", "selfplay_step", "selfplay_row_len", "selfplay_rows", "selfplay_stats",
    "selfplay_ring", "selfplay_rows_device", "mlp_eval",
]
# entry points a library may lack (the tests' CPU oracle binds SYMBOLS only): bound when present, else the methods that need
# them raise
OPTIONAL_SYMBOLS = ["set_population", "set_net_weights", "set_net_weights_device", "set_population_weights_device", "set_net_search",
                    "set_net_search_ex",
                    "population_selfplay_begin", "selfplay_keep_states", "selfplay_states", "selfplay_reanalyse",
                    "selfplay_keep_transitions", "selfplay_transitions", "selfplay_nstep_targets",
                    "selfplay_lambda_targets", "selfplay_lambda_targets_nets",
                    "selfplay_keep_priorities", "selfplay_priorities", "selfplay_priority_values", "selfplay_sample_rows",
                    "selfplay_sample_slots", "selfplay_is_weights", "selfplay_is_weights_device", "selfplay_is_weight_values",
                    "selfplay_keep_errors", "selfplay_errors_device", "selfplay_error_values", "selfplay_set_error_values",
                    "selfplay_priorities_trained",
                    "policy_rollout", "policy_rollout_ex", "search_rollout",
                    "population_mlp_eval", "population_mlp_eval_device", "population_root_eval",
                    "trainer_create", "trainer_destroy", "trainer_last_error", "trainer_param_count", "trainer_forward",
                    "trainer_backward_step", "trainer_loss", "trainer_step", "trainer_read_d_raw", "trainer_epoch",
                    "trainer_backward_step_opt", "trainer_step_opt", "trainer_epoch_opt", "trainer_create_ex", "trainer_create_wide",
                    "trainer_create_wide_ex",
                    "trainer_backward_step_nets", "trainer_loss_nets", "trainer_step_nets", "trainer_epoch_nets",
                    "trainer_loss_weighted", "trainer_loss_nets_weighted", "trainer_step_opt_weighted", "trainer_step_nets_weighted",
                    "trainer_epoch_opt_weighted", "trainer_epoch_nets_weighted",
                    "trainer_loss_errors", "trainer_loss_nets_errors", "trainer_epoch_opt_errors", "trainer_epoch_nets_errors",
                    "trainer_epoch_online", "trainer_epoch_online_nets",
                    "trainer_set_ema", "trainer_ema_info", "use_weights", "weights_info", "selfplay_refresh_values"]


class AzgNetSearch(C.Structure):
    """include/azgym_population.h: azg_net_search"""
    _fields_ = [("struct_size", C.c_int32), ("n_sims", C.c_int32), ("c_uct", C.c_double), ("gamma", C.c_double), ("epsilon", C.c_double),
                ("c_pw", C.c_double), ("kappa", C.c_double)]


NET_SEARCH_WIDE = 1   # AZG_NET_SEARCH_WIDE: the table may be searched by nets of padded width >= 512 (azg_set_net_search_ex)
NET_SEARCH_KEYS = ("c_uct", "gamma", "epsilon", "c_pw", "kappa")   # the MCTS settings a population's nets may each have their own of


def net_search_entries(settings, n_nets, shared):
    """The per-net settings of a population as K complete dicts: ``settings`` is a list of K dicts whose keys are a subset of
    NET_SEARCH_KEYS; a missing key takes its value from ``shared`` (the engine's own settings)."""
    settings = list(settings)
    if len(settings) != n_nets:
        raise ValueError(f"net_settings has {len(settings)} entries for {n_nets} nets: one per net")
    out = []
    for k, st in enumerate(settings):
        unknown = sorted(set(st) - set(NET_SEARCH_KEYS))
        if unknown:
            raise ValueError(f"net_settings[{k}]: unknown keys {unknown}; per-net search settings are {list(NET_SEARCH_KEYS)}")
        out.append({key: float(st.get(key, shared[key])) for key in NET_SEARCH_KEYS})
    return out


def widest_pw(entries, n_sims):
    """The (c_pw, kappa) pair among ``entries`` (dicts) whose progressive widening reaches the most children within n_sims simulations
    (the engine's Kmax): the pair an engine is created with so that every net fits.  The first such pair on a tie."""
    best, best_k = None, -1
    for st in entries:
        k = max(pw_table(st["c_pw"], st["kappa"], n_sims))
        if k > best_k:
            best, best_k = (st["c_pw"], st["kappa"]), k
    return best


class AzgRmsprop(C.Structure):
    """include/azgym_train.h: azg_rmsprop"""
    _fields_ = [("struct_size", C.c_int32), ("centered", C.c_int32), ("lr", C.c_double), ("alpha", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("momentum", C.c_double), ("grad_clip", C.c_double)]


class AzgTrainerOptions(C.Structure):
    """include/azgym_train.h: azg_trainer_options"""
    _fields_ = [("struct_size", C.c_int32), ("layernorm", C.c_int32)]


OPT_RMSPROP, OPT_ADAM = 0, 1


class AzgOptim(C.Structure):
    """include/azgym_train.h: azg_optim"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("lr", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("alpha", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("grad_clip", C.c_double),
                ("state0", C.c_void_p), ("state1", C.c_void_p), ("grad_norms", C.c_void_p), ("step", C.c_int32)]


LOSS_ALPHAZERO, LOSS_A0C, LOSS_A0C_TUNED = 0, 1, 2
HEAD_DISCRETE, HEAD_NORMAL, HEAD_GMM = 0, 1, 2
REDUCE = {"mean": 0, "sum": 1}
LOSS_KEYS = ("loss", "policy_loss", "value_loss", "entropy_loss", "alpha_loss")   # the slots of losses[k][5]
# the keys of population_loss's dictionary per loss kind, in its order
LOSS_KEYS_OF = {LOSS_ALPHAZERO: ("loss", "policy_loss", "value_loss"), LOSS_A0C: ("loss", "policy_loss", "entropy_loss", "value_loss"),
                LOSS_A0C_TUNED: ("loss", "policy_loss", "entropy_loss", "value_loss", "alpha_loss")}


class AzgLossCfg(C.Structure):
    """include/azgym_train.h: azg_loss_cfg"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("head", C.c_int32), ("reduction", C.c_int32),
                ("tau", C.c_double), ("policy_coeff", C.c_double), ("value_coeff", C.c_double), ("alpha", C.c_double),
                ("target_entropy", C.c_double), ("alpha_lr", C.c_double), ("alpha_beta1", C.c_double), ("alpha_beta2", C.c_double),
                ("alpha_eps", C.c_double), ("alpha_weight_decay", C.c_double), ("alpha_clip", C.c_double), ("action_bound", C.c_double)]


class AzgAlphaState(C.Structure):
    """include/azgym_train.h: azg_alpha_state"""
    _fields_ = [("struct_size", C.c_int32), ("step", C.c_int32), ("log_alpha", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p)]


class AzgEpochRows(C.Structure):
    """include/azgym_train.h: azg_epoch_rows"""
    _fields_ = [("struct_size", C.c_int32), ("row_len", C.c_int32), ("state_dim", C.c_int32), ("n_actions", C.c_int32),
                ("rows_per_net", C.c_int32), ("group", C.c_int32), ("group_stride", C.c_int64), ("net_stride", C.c_int64),
                ("rows", C.c_void_p)]


class AzgEmaCfg(C.Structure):
    """include/azgym_train_ema.h: azg_ema_cfg"""
    _fields_ = [("struct_size", C.c_int32), ("n_decay", C.c_int32), ("every", C.c_int32), ("reserved", C.c_int32),
                ("ema", C.c_void_p), ("decay", C.POINTER(C.c_double))]


WEIGHTS_LIVE, WEIGHTS_TARGET = 0, 1   # include/azgym_target.h: AZG_WEIGHTS_*


def bind(lib, prefix):
    """Resolve every entry point of include/azgym.h on ``lib`` and set its prototype."""
    f = {}
    for s in SYMBOLS:
        f[s] = getattr(lib, prefix + s)
    vp = C.c_void_p
    f["abi_version"].restype = C.c_int
    f["engine_create"].argtypes = [C.POINTER(AzgConfig), C.POINTER(vp)]
    f["engine_destroy"].argtypes = [vp]
    f["engine_destroy"].restype = None
    f["last_error"].argtypes = [vp]
    f["last_error"].restype = C.c_char_p
    f["set_weights"].argtypes = [vp, C.POINTER(AzgMlpDesc), C.POINTER(C.c_float), C.c_size_t]
    f["set_weights_device"].argtypes = [vp, C.POINTER(AzgMlpDesc), C.c_void_p, C.c_size_t]
    f["results_resident"].argtypes = [vp] + [C.POINTER(C.c_void_p)] * 5
    f["set_search_index"].argtypes = [vp, C.c_uint32]
    f["search"].argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    f["results"].argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    f["root_children"].argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    f["root_eval"].argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    f["dump_tree"].argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                               C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    for s in ("max_children", "max_records", "env_state_dim", "obs_dim"):
        f[s].argtypes = [vp]
    f["synthetic_roots"].argtypes = [vp, C.POINTER(C.c_double)]
    f["last_search_ms"].argtypes = [vp, C.POINTER(C.c_float)]
    f["upload_roots"].argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    f["search_resident"].argtypes = [vp]
    f["sync"].argtypes = [vp]
    f["selfplay_begin"].argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    f["selfplay_begin_ex"].argtypes = [vp, C.POINTER(AzgSelfplayConfig)]
    f["selfplay_ring"].argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    f["selfplay_rows_device"].argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    f["selfplay_step"].argtypes = [vp]
    f["selfplay_row_len"].argtypes = [vp]
    f["selfplay_rows"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int32]
    f["selfplay_stats"].argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    f["mlp_eval"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for s in OPTIONAL_SYMBOLS:
        fn = getattr(lib, prefix + s, None)
        if fn is not None:
            f[s] = fn
    if "set_population" in f:
        f["set_population"].argtypes = [vp, C.c_int32]
    if "set_net_search" in f:
        f["set_net_search"].argtypes = [vp, C.POINTER(AzgNetSearch), C.c_int32]
    if "set_net_search_ex" in f:
        f["set_net_search_ex"].argtypes = [vp, C.POINTER(AzgNetSearch), C.c_int32, C.c_uint32]
    if "set_net_weights" in f:
        f["set_net_weights"].argtypes = [vp, C.c_int32, C.POINTER(AzgMlpDesc), C.POINTER(C.c_float), C.c_size_t]
    if "set_net_weights_device" in f:
        f["set_net_weights_device"].argtypes = [vp, C.c_int32, C.POINTER(AzgMlpDesc), C.c_void_p, C.c_size_t]
    if "set_population_weights_device" in f:
        f["set_population_weights_device"].argtypes = [vp, C.POINTER(AzgMlpDesc), C.c_void_p, C.c_size_t, C.c_int32]
    if "population_selfplay_begin" in f:
        f["population_selfplay_begin"].argtypes = [vp, C.POINTER(AzgSelfplayConfig)]
    if "selfplay_reanalyse" in f:   # include/azgym_reanalyse.h
        f["selfplay_keep_states"].argtypes = [vp, C.c_int32]
        f["selfplay_states"].argtypes = [vp, C.POINTER(C.c_double), C.c_size_t]
        f["selfplay_reanalyse"].argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, C.c_uint32]
    if "selfplay_nstep_targets" in f:   # include/azgym_nstep.h
        f["selfplay_keep_transitions"].argtypes = [vp, C.c_int32]
        f["selfplay_transitions"].argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                              C.c_size_t]
        f["selfplay_nstep_targets"].argtypes = [vp, C.POINTER(AzgNstepConfig)]
    if "selfplay_refresh_values" in f:   # include/azgym_refresh.h
        f["selfplay_refresh_values"].argtypes = [vp, C.POINTER(C.c_int32), C.c_int32]
    if "selfplay_lambda_targets" in f:   # include/azgym_lambda.h
        f["selfplay_lambda_targets"].argtypes = [vp, C.POINTER(AzgReturnRule)]
        f["selfplay_lambda_targets_nets"].argtypes = [vp, C.POINTER(AzgReturnRule)]
    if "selfplay_sample_rows" in f:   # include/azgym_priority.h
        f["selfplay_keep_priorities"].argtypes = [vp, C.c_int32]
        f["selfplay_priorities"].argtypes = [vp, C.POINTER(AzgPriorityConfig)]
        f["selfplay_priority_values"].argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
        f["selfplay_sample_rows"].argtypes = [vp, C.POINTER(AzgSampleConfig), C.POINTER(C.c_int32)]
        f["selfplay_sample_slots"].argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32)]
    if "selfplay_is_weights" in f:   # include/azgym_priority.h: the importance-sampling weights
        f["selfplay_is_weights"].argtypes = [vp, C.c_float]
        f["selfplay_is_weights_device"].argtypes = [vp, C.POINTER(C.c_void_p)]
        f["selfplay_is_weight_values"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
    if "selfplay_priorities_trained" in f:   # include/azgym_priority.h: priorities fed back from the trainer's value errors
        f["selfplay_keep_errors"].argtypes = [vp, C.c_int32]
        f["selfplay_errors_device"].argtypes = [vp, C.POINTER(C.c_void_p)]
        f["selfplay_error_values"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
        f["selfplay_set_error_values"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
        f["selfplay_priorities_trained"].argtypes = [vp, C.POINTER(AzgTrainedPriorityConfig)]
    if "search_rollout" in f:   # include/azgym_search_rollout.h
        f["search_rollout"].argtypes = [vp, C.POINTER(AzgSearchRolloutConfig), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(AzgSearchRolloutInfo)]
    if "policy_rollout" in f:   # include/azgym_eval.h
        f["policy_rollout"].argtypes = [vp, C.POINTER(AzgRolloutConfig), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    if "policy_rollout_ex" in f:
        f["policy_rollout_ex"].argtypes = [vp, C.POINTER(AzgRolloutConfig), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(AzgRolloutInfo)]
    if "population_mlp_eval" in f:
        f["population_mlp_eval"].argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), C.POINTER(AzgEvalInfo)]
    if "population_mlp_eval_device" in f:
        f["population_mlp_eval_device"].argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, C.POINTER(AzgEvalInfo)]
    if "population_root_eval" in f:
        f["population_root_eval"].argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if "trainer_create" in f:   # include/azgym_train.h
        f["trainer_create"].argtypes = [C.c_int32, C.POINTER(AzgMlpDesc), C.c_int32, C.c_int32, C.POINTER(vp)]
        f["trainer_destroy"].argtypes = [vp]
        f["trainer_destroy"].restype = None
        f["trainer_last_error"].argtypes = [vp]
        f["trainer_last_error"].restype = C.c_char_p
        f["trainer_param_count"].argtypes = [vp]
        f["trainer_param_count"].restype = C.c_size_t
        f["trainer_forward"].argtypes = [vp, vp, vp, C.c_int32, vp]
        f["trainer_backward_step"].argtypes = [vp, vp, vp, C.c_int32, C.POINTER(AzgRmsprop), vp, vp]
    if "trainer_loss" in f:
        f["trainer_loss"].argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(AzgLossCfg), C.POINTER(AzgAlphaState), vp, vp]
        f["trainer_step"].argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(AzgLossCfg), C.POINTER(AzgAlphaState),
                                      C.POINTER(AzgRmsprop), vp, vp, vp, vp]
        f["trainer_read_d_raw"].argtypes = [vp, C.c_int32, vp]
    if "trainer_epoch" in f:
        f["trainer_epoch"].argtypes = [vp, vp, C.POINTER(AzgEpochRows), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(AzgLossCfg),
                                       C.POINTER(AzgAlphaState), C.POINTER(AzgRmsprop), vp, vp, C.POINTER(C.c_int32)]
    if "trainer_backward_step_opt" in f:
        f["trainer_backward_step_opt"].argtypes = [vp, vp, vp, C.c_int32, C.POINTER(AzgOptim), vp]
        f["trainer_step_opt"].argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(AzgLossCfg), C.POINTER(AzgAlphaState),
                                          C.POINTER(AzgOptim), vp, vp, vp]
        f["trainer_epoch_opt"].argtypes = [vp, vp, C.POINTER(AzgEpochRows), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(AzgLossCfg),
                                           C.POINTER(AzgAlphaState), C.POINTER(AzgOptim), vp, C.POINTER(C.c_int32)]
    if "trainer_create_ex" in f:
        f["trainer_create_ex"].argtypes = [C.c_int32, C.POINTER(AzgMlpDesc), C.c_int32, C.c_int32, C.POINTER(AzgTrainerOptions), C.POINTER(vp)]
    if "trainer_create_wide" in f:
        f["trainer_create_wide"].argtypes = [C.c_int32, C.POINTER(AzgMlpDesc), C.c_int32, C.c_int32, C.POINTER(vp)]
    if "trainer_create_wide_ex" in f:
        f["trainer_create_wide_ex"].argtypes = [C.c_int32, C.POINTER(AzgMlpDesc), C.c_int32, C.c_int32, C.POINTER(AzgTrainerOptions),
                                                C.POINTER(vp)]
    if "trainer_backward_step_nets" in f:   # the *_opt prototypes with arrays of n_nets entries
        f["trainer_backward_step_nets"].argtypes = f["trainer_backward_step_opt"].argtypes
        f["trainer_loss_nets"].argtypes = f["trainer_loss"].argtypes
        f["trainer_step_nets"].argtypes = f["trainer_step_opt"].argtypes
        f["trainer_epoch_nets"].argtypes = f["trainer_epoch_opt"].argtypes
    if "trainer_loss_weighted" in f:   # include/azgym_train_weighted.h: the namesake's prototype with `weights` added
        def with_weights(name, at):
            args = list(f[name].argtypes)
            return args[:at] + [vp] + args[at:]
        f["trainer_loss_weighted"].argtypes = f["trainer_loss_nets_weighted"].argtypes = with_weights("trainer_loss", 5)
        f["trainer_step_opt_weighted"].argtypes = f["trainer_step_nets_weighted"].argtypes = with_weights("trainer_step_opt", 6)
        f["trainer_epoch_opt_weighted"].argtypes = f["trainer_epoch_nets_weighted"].argtypes = with_weights("trainer_epoch_opt", 3)
    if "trainer_loss_errors" in f:   # include/azgym_train_errors.h: the weighted prototype with `errors` after `weights`
        def with_errors(name, at):
            args = list(f[name].argtypes)
            return args[:at] + [vp] + args[at:]
        f["trainer_loss_errors"].argtypes = f["trainer_loss_nets_errors"].argtypes = with_errors("trainer_loss_weighted", 6)
        f["trainer_epoch_opt_errors"].argtypes = f["trainer_epoch_nets_errors"].argtypes = with_errors("trainer_epoch_opt_weighted", 4)
    if "trainer_epoch_online" in f:   # include/azgym_train_online.h
        f["trainer_epoch_online"].argtypes = f["trainer_epoch_online_nets"].argtypes = [
            vp, vp, vp, C.POINTER(AzgOnlineEpoch), C.POINTER(AzgLossCfg), C.POINTER(AzgAlphaState), C.POINTER(AzgOptim), vp]
    if "trainer_set_ema" in f:   # include/azgym_train_ema.h
        f["trainer_set_ema"].argtypes = [vp, C.POINTER(AzgEmaCfg)]
        f["trainer_ema_info"].argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if "use_weights" in f:   # include/azgym_target.h
        f["use_weights"].argtypes = [vp, C.c_int32]
        f["weights_info"].argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return f


def policy_tensors(policy):
    """(AzgMlpDesc, [tensors in blob order]) of a torch policy: per trunk layer weight, bias (, LayerNorm weight, bias), then the
    value head and the distribution head (= state_dict order).  Works for this package's policies and for the reference's
    DiscretePolicy / DiagonalNormalPolicy objects alike (same attribute names: trunk, value_head, dist_head, hidden_dimensions,
    state_dim; alphazero/network/policies.py:101-120, 238-259)."""
    hidden = list(policy.hidden_dimensions)
    linears, norms, acts = [], [], set()
    for mod in policy.trunk:
        name = type(mod).__name__
        if name == "Linear":
            linears.append(mod)
        elif name == "LayerNorm":
            norms.append(mod)
        elif name in _ACT_MODULES:
            acts.add(_ACT_MODULES[name])
        else:
            raise NotImplementedError(f"trunk module {name}: the engine implements Linear + activation (+ LayerNorm) trunks")
    if len(acts) != 1 or len(linears) != len(hidden) or len(norms) not in (0, len(hidden)):
        raise NotImplementedError("unsupported trunk structure")
    if any(abs(n.eps - 1e-5) > 1e-12 or not n.elementwise_affine for n in norms):
        raise NotImplementedError("LayerNorm must use eps=1e-5 and elementwise_affine=True (the torch defaults)")
    desc = AzgMlpDesc()
    desc.struct_size = C.sizeof(AzgMlpDesc)
    desc.in_dim = policy.state_dim
    desc.n_hidden = len(hidden)
    for i, h in enumerate(hidden):
        desc.hidden[i] = h
    desc.n_dist = policy.dist_head.out_features
    desc.activation = acts.pop()
    desc.log_std_min = float(getattr(policy, "log_param_min", -5.0))
    desc.log_std_max = float(getattr(policy, "log_param_max", 2.0))
    desc.num_components = int(getattr(policy, "num_components", 0) or 0)
    desc.layernorm = 1 if norms else 0
    tensors = []
    for i, mod in enumerate(linears):
        tensors += [mod.weight, mod.bias]
        if norms:
            tensors += [norms[i].weight, norms[i].bias]
    for mod in (policy.value_head, policy.dist_head):
        tensors += [mod.weight, mod.bias]
    return desc, tensors


def policy_blob(policy):
    """Flatten a torch policy into (AzgMlpDesc, float32 host blob) in state_dict order (see policy_tensors)."""
    desc, tensors = policy_tensors(policy)
    blob = np.ascontiguousarray(np.concatenate([t.detach().cpu().numpy().ravel() for t in tensors]), dtype=np.float32)
    return desc, blob


def make_desc(in_dim, hidden, n_dist, activation, log_std_min=-5.0, log_std_max=2.0, num_components=0, layernorm=False):
    desc = AzgMlpDesc()
    desc.struct_size = C.sizeof(AzgMlpDesc)
    desc.in_dim = in_dim
    desc.n_hidden = len(hidden)
    for i, h in enumerate(hidden):
        desc.hidden[i] = h
    desc.n_dist = n_dist
    desc.activation = ACT[activation] if isinstance(activation, str) else activation
    desc.log_std_min = log_std_min
    desc.log_std_max = log_std_max
    desc.num_components = num_components
    desc.layernorm = int(bool(layernorm))
    return desc


def lockstep_shaped(in_dim, hidden, layernorm=False):
    """The engine's rule (engine_host.h: azg_lockstep_shaped) for a network it searches as team / per-layer launches: padded width
    >= 512, at least two hidden layers, no LayerNorm, at most four inputs.  A population of such nets needs a multiple of 32 trees
    per net (azg_set_net_weights refuses others with AZG_E_UNSUPPORTED); every other shape takes any number."""
    return -(-max(hidden) // 64) * 64 >= 512 and len(hidden) >= 2 and not layernorm and in_dim <= 4


class Engine:
    """One batched MCTS engine (B trees).  Mirrors MCTS*.__init__ kwargs (alphazero/search/mcts.py:316-327, 537-549)."""

    last_rollout_info = None   # what the last policy_rollout ran as (azg_rollout_info as a dict)
    last_eval_info = None      # what the last population_mlp_eval* ran as (azg_eval_info as a dict)
    _sp_cap = 0                # the replay ring's capacity in steps (selfplay_begin; 0: no begin yet, the engine refuses the ring's calls)

    def __init__(self, fns, *, env_id, mode, n_trees, n_sims, c_uct, gamma, epsilon=0.0, num_actions=0, c_pw=1.0,
                 kappa=0.5, v_target="off_policy", reward_scale=PENDULUM_R_SCALE, action_bound=2.0, seed=34,
                 tree_id_base=0, device_id=0, tie_break="first"):
        self._f = fns
        self._h = C.c_void_p()
        cfg = AzgConfig()
        cfg.struct_size = C.sizeof(AzgConfig)
        cfg.device_id = device_id
        cfg.env_id = env_id
        cfg.mode = mode
        cfg.n_trees = n_trees
        cfg.n_sims = n_sims
        cfg.num_actions = num_actions
        cfg.v_target = VT[v_target] if isinstance(v_target, str) else v_target
        cfg.tree_id_base = tree_id_base
        cfg.tie_break = TIE[tie_break] if isinstance(tie_break, str) else int(tie_break)
        cfg.c_uct = float(c_uct)
        cfg.gamma = float(gamma)
        cfg.epsilon = float(epsilon)
        cfg.c_pw = float(c_pw)
        cfg.kappa = float(kappa)
        cfg.reward_scale = float(reward_scale)
        cfg.action_bound = float(action_bound)
        cfg.seed = int(seed)
        self.cfg = cfg
        rc = fns["engine_create"](C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise EngineError(rc, (fns["last_error"](None) or b"").decode())
        self.n_trees = n_trees
        self.n_sims = n_sims
        self.mode = mode
        self.kmax = fns["max_children"](self._h)
        self.max_records = fns["max_records"](self._h)
        self.s_env = fns["env_state_dim"](self._h)
        self.s_obs = fns["obs_dim"](self._h)
        self.n_dist = num_actions if mode == MODE_DISCRETE else 2   # 3 * num_components after set_weights with a mixture head

    def _check(self, rc):
        if rc != 0:
            msg = (self._f["last_error"](self._h) or b"").decode()
            if rc == AZG_E_TERMINAL_ROOT:
                raise ValueError(msg or "Can't do tree search from a terminal node")
            raise EngineError(rc, msg)

    def close(self):
        if self._h:
            self._f["engine_destroy"](self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _weights_set(self, rc, desc):
        """Check a set_*weights* call; a continuous head's n_dist is then the net's (3 * num_components with a mixture)."""
        self._check(rc)
        if self.mode == MODE_CONTINUOUS:
            self.n_dist = desc.n_dist

    def set_weights(self, desc, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._weights_set(self._f["set_weights"](self._h, C.byref(desc), _ptr(blob, C.c_float), blob.size), desc)

    def set_weights_device(self, desc, device_ptr, n_floats):
        """azg_set_weights_device: the flat float32 blob already lives on the engine's GPU (complete: producer stream synchronised)."""
        self._weights_set(self._f["set_weights_device"](self._h, C.byref(desc), C.c_void_p(int(device_ptr)), int(n_floats)), desc)

    def _flat_on_device(self, policies):
        """(desc, [K, n] float32 tensor) of K torch policies flattened on the engine's GPU (one torch.cat per policy; the torch stream
        is synchronised), or None when some parameter lives elsewhere."""
        pars = [p for pol in policies for p in pol.parameters()]
        if not pars or not all(p.is_cuda and p.device.index == self.cfg.device_id for p in pars):
            return None
        import torch
        parts = [policy_tensors(pol) for pol in policies]
        with torch.no_grad():
            rows = [torch.cat([t.detach().reshape(-1).to(torch.float32) for t in tensors]) for _, tensors in parts]
        flat = rows[0][None] if len(rows) == 1 else torch.stack(rows)
        torch.cuda.current_stream(pars[0].device).synchronize()
        return parts[0][0], flat

    def set_policy(self, policy):
        """Push a torch policy's weights.  Parameters on the engine's GPU are flattened there and re-laid-out by the engine's gather
        kernel: nothing crosses PCIe ("device"); CPU parameters take the host path ("host").  Returns which path was taken."""
        on_device = self._flat_on_device([policy])
        if on_device is not None:
            desc, flat = on_device
            self.set_weights_device(desc, flat.data_ptr(), flat.shape[1])
            return "device"
        self.set_weights(*policy_blob(policy))
        return "host"

    def _optional(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise NotImplementedError(f"this engine library has no {name} entry point")
        return fn

    def set_population(self, n_nets):
        """azg_set_population: trees k*T .. k*T+T-1 (T = n_trees / n_nets) are searched with net k's weights.  Drops every weight
        when n_nets changes; 1 is the single-network engine."""
        self._check(self._optional("set_population")(self._h, int(n_nets)))
        if int(n_nets) != getattr(self, "n_nets", 1):   # (the engine dropped its per-net search table with the old split)
            self._net_search_gamma = None
        self.n_nets = int(n_nets)

    def set_net_search(self, settings, wide=False, n_sims=None):
        """azg_set_net_search: net k searches with settings[k], a dict with all of c_uct, gamma, epsilon, c_pw, kappa (discrete mode
        ignores the last two), instead of the engine's shared settings; None returns to those.  One entry per net of the population.
        ``wide=True``: azg_set_net_search_ex with AZG_NET_SEARCH_WIDE -- the table may be searched by nets of padded width >= 512.
        ``n_sims`` (optional): one int per net, net k's own simulation budget (azg_net_search.n_sims: 0 = the engine's, else 1 .. the
        engine's n_sims, which stays the capacity)."""
        if wide:
            ex = self._optional("set_net_search_ex")

            def fn(h, arr, n):
                return ex(h, arr, n, NET_SEARCH_WIDE)
        else:
            fn = self._optional("set_net_search")
        if settings is None:
            self._check(fn(self._h, None, 0))
            self._net_search_gamma = None
            return
        settings = list(settings)
        if n_sims is not None:
            n_sims = [int(n) for n in n_sims]
            if len(n_sims) != len(settings):
                raise ValueError(f"set_net_search: n_sims has {len(n_sims)} entries for {len(settings)} nets: one per net")
        arr = (AzgNetSearch * max(len(settings), 1))()
        for k, st in enumerate(settings):
            arr[k].struct_size = C.sizeof(AzgNetSearch)
            arr[k].n_sims = 0 if n_sims is None else n_sims[k]
            for key in NET_SEARCH_KEYS:
                setattr(arr[k], key, float(st[key]))
        self._check(fn(self._h, arr, len(settings)))
        self._net_search_gamma = [float(arr[k].gamma) for k in range(len(settings))]   # (selfplay_lambda_targets resolves a None among numbers from it)

    def set_net_weights(self, net, desc, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._weights_set(self._optional("set_net_weights")(self._h, int(net), C.byref(desc), _ptr(blob, C.c_float), blob.size), desc)

    def set_net_policy(self, net, policy):
        """Push a torch policy's weights as net ``net`` of the population (host blob: one H2D copy per net)."""
        desc, blob = policy_blob(policy)
        self.set_net_weights(net, desc, blob)

    def set_net_weights_device(self, net, desc, device_ptr, n_floats):
        """azg_set_net_weights_device: net ``net``'s flat float32 blob already lives on the engine's GPU (complete)."""
        fn = self._optional("set_net_weights_device")
        self._weights_set(fn(self._h, int(net), C.byref(desc), C.c_void_p(int(device_ptr)), int(n_floats)), desc)

    def set_population_weights_device(self, desc, device_ptr, n_floats_per_net, n_nets):
        """azg_set_population_weights_device: every net from one device array [n_nets][n_floats_per_net] (complete), one gather
        launch."""
        fn = self._optional("set_population_weights_device")
        self._weights_set(fn(self._h, C.byref(desc), C.c_void_p(int(device_ptr)), int(n_floats_per_net), int(n_nets)), desc)

    def set_population_policies(self, policies):
        """Push K torch policies as nets 0..K-1 (K = the engine's n_nets).  When every parameter lives on the engine's GPU they are
        flattened there into one [K, n] tensor, the torch stream is synchronised once and one call gathers them all ("device");
        otherwise each net is uploaded from a host blob ("host").  Returns which path was taken."""
        policies = list(policies)
        self._optional("set_population_weights_device")
        on_device = self._flat_on_device(policies)
        if on_device is not None:
            desc, flat = on_device
            self.set_population_weights_device(desc, flat.data_ptr(), flat.shape[1], flat.shape[0])
            return "device"
        for k, pol in enumerate(policies):
            self.set_net_policy(k, pol)
        return "host"

    def use_weights(self, which):
        """azg_use_weights: ``which`` "live" or "target" (or AZG_WEIGHTS_*) becomes the weight set every upload writes and every
        network evaluation reads (include/azgym_target.h)."""
        which = {"live": WEIGHTS_LIVE, "target": WEIGHTS_TARGET}.get(which, which)
        self._check(self._optional("use_weights")(self._h, int(which)))

    def weights_info(self):
        """azg_weights_info: {"in_use": "live" | "target", "target_ready": bool}."""
        in_use, ready = C.c_int32(0), C.c_int32(0)
        self._check(self._optional("weights_info")(self._h, C.byref(in_use), C.byref(ready)))
        return {"in_use": "target" if in_use.value == WEIGHTS_TARGET else "live", "target_ready": bool(ready.value)}

    def results_resident(self):
        """azg_results_resident: launch return_results into the engine's device buffers; their addresses as a dict of ints."""
        ptrs = [C.c_void_p() for _ in range(5)]
        self._check(self._f["results_resident"](self._h, *[C.byref(p) for p in ptrs]))
        return dict(zip(("actions", "counts", "Q", "v_target", "n_children"), (p.value for p in ptrs)))

    def set_search_index(self, idx):
        self._check(self._f["set_search_index"](self._h, int(idx)))

    def _roots(self, roots, carry):
        roots = np.ascontiguousarray(roots, dtype=np.float64).reshape(self.n_trees, self.s_env)
        if carry is not None:
            carry = np.ascontiguousarray(carry, dtype=np.int32).reshape(self.n_trees)
        return roots, carry

    def search(self, roots, carry=None):
        roots, carry = self._roots(roots, carry)
        self._check(self._f["search"](self._h, _ptr(roots, C.c_double), _ptr(carry, C.c_int32)))

    def upload_roots(self, roots, carry=None):
        roots, carry = self._roots(roots, carry)
        self._check(self._f["upload_roots"](self._h, _ptr(roots, C.c_double), _ptr(carry, C.c_int32)))

    def search_resident(self):
        self._check(self._f["search_resident"](self._h))

    def sync(self):
        self._check(self._f["sync"](self._h))

    def last_search_ms(self):
        ms = C.c_float()
        self._check(self._f["last_search_ms"](self._h, C.byref(ms)))
        return ms.value

    def synthetic_roots(self):
        roots = np.empty((self.n_trees, self.s_env), dtype=np.float64)
        self._check(self._f["synthetic_roots"](self._h, _ptr(roots, C.c_double)))
        return roots

    def results(self):
        B, K = self.n_trees, self.kmax
        actions = np.empty((B, K), np.float32)
        counts = np.empty((B, K), np.int32)
        Q = np.empty((B, K), np.float64)
        vt = np.empty((B,), np.float64)
        nc = np.empty((B,), np.int32)
        self._check(self._f["results"](self._h, _ptr(actions, C.c_float), _ptr(counts, C.c_int32), _ptr(Q, C.c_double),
                                       _ptr(vt, C.c_double), _ptr(nc, C.c_int32)))
        return {"actions": actions, "counts": counts, "Q": Q, "v_target": vt, "n_children": nc}

    def root_children(self):
        B, K = self.n_trees, self.kmax
        child_n = np.empty((B, K), np.int32)
        child_state = np.empty((B, K, self.s_env), np.float64)
        self._check(self._f["root_children"](self._h, _ptr(child_n, C.c_int32), _ptr(child_state, C.c_double)))
        return child_n, child_state

    def root_eval(self):
        value = np.empty((self.n_trees,), np.float32)
        dist = np.empty((self.n_trees, self.n_dist), np.float32)
        self._check(self._f["root_eval"](self._h, _ptr(value, C.c_float), _ptr(dist, C.c_float)))
        return value, dist

    def mlp_eval(self, obs):
        """Batched network inference (policies.py predict_V / predict_pi / forward) of observations [n, obs_dim] with the
        search's own arithmetic: (value [n], dist [n, n_dist], raw head outputs [n, 1 + n_dist])."""
        obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, self.s_obs)
        n = obs.shape[0]
        value = np.empty((n,), np.float32)
        dist = np.empty((n, self.n_dist), np.float32)
        raw = np.empty((n, 1 + self.n_dist), np.float32)
        self._check(self._f["mlp_eval"](self._h, _ptr(obs, C.c_float), n, _ptr(value, C.c_float), _ptr(dist, C.c_float),
                                        _ptr(raw, C.c_float)))
        return value, dist, raw

    def _eval_rows(self, who, shape, shared):
        """n of a population_mlp_eval* call with observations of ``shape``; a wrong shape raises before anything native is touched."""
        K = int(getattr(self, "n_nets", 1))
        shape = tuple(int(s) for s in shape)
        if len(shape) != (2 if shared else 3) or shape[-1] != self.s_obs or not (shared or shape[0] == K):
            expected = f"[n, {self.s_obs}]" if shared else f"[{K}, n, {self.s_obs}]"
            raise ValueError(f"{who}: obs has shape {list(shape)}, expected {expected}" + (" (shared=True)" if shared else ""))
        return shape[-2]

    def _eval_info(self, info):
        self.last_eval_info = {"resident": int(info.resident), "groups": int(info.groups), "tiles": int(info.tiles)}

    def population_mlp_eval(self, obs, shared=False):
        """azg_population_mlp_eval (include/azgym_eval.h): every net of the engine evaluated in ONE launch, net k on ``obs[k]`` (obs
        [n_nets, n, obs_dim]), or with ``shared`` every net on the same rows (obs [n, obs_dim]).  Returns (value [n_nets, n], dist
        [n_nets, n, n_dist], raw [n_nets, n, 1 + n_dist]) with mlp_eval's bits per net; ``self.last_eval_info`` is then what ran
        (``resident``, ``groups``, ``tiles``)."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n = self._eval_rows("population_mlp_eval", obs.shape, shared)
        fn = self._optional("population_mlp_eval")
        K = int(getattr(self, "n_nets", 1))
        value = np.empty((K, n), np.float32)
        dist = np.empty((K, n, self.n_dist), np.float32)
        raw = np.empty((K, n, 1 + self.n_dist), np.float32)
        info = AzgEvalInfo()
        info.struct_size = C.sizeof(AzgEvalInfo)
        self._check(fn(self._h, _ptr(obs, C.c_float), n, 1 if shared else 0, _ptr(value, C.c_float), _ptr(dist, C.c_float),
                       _ptr(raw, C.c_float), C.byref(info)))
        self._eval_info(info)
        return value, dist, raw

    def population_mlp_eval_device(self, obs, shared=False, out=None):
        """azg_population_mlp_eval_device: ``obs`` is a float32 torch tensor on the engine's GPU (shapes as population_mlp_eval); the
        torch stream is synchronised once, then the kernel reads it in place and writes torch tensors (value, dist, raw) --
        ``out``, a triple of contiguous float32 tensors of those shapes on the same GPU, or new ones.  Nothing crosses PCIe."""
        import torch
        n = self._eval_rows("population_mlp_eval_device", obs.shape, shared)
        fn = self._optional("population_mlp_eval_device")
        if not obs.is_cuda or obs.device.index != self.cfg.device_id or obs.dtype != torch.float32:
            raise ValueError("population_mlp_eval_device: obs must be a float32 tensor on the engine's GPU")
        obs = obs.contiguous()
        K = int(getattr(self, "n_nets", 1))
        shapes = ((K, n), (K, n, self.n_dist), (K, n, 1 + self.n_dist))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=obs.device) for s in shapes)
        else:
            out = tuple(out)
            for t, s in zip(out, shapes):
                if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != obs.device or not t.is_contiguous():
                    raise ValueError(f"population_mlp_eval_device: out must be contiguous float32 tensors of shapes {shapes} on the engine's GPU")
        torch.cuda.current_stream(obs.device).synchronize()
        info = AzgEvalInfo()
        info.struct_size = C.sizeof(AzgEvalInfo)
        self._check(fn(self._h, C.c_void_p(obs.data_ptr()), n, 1 if shared else 0, *[C.c_void_p(t.data_ptr()) for t in out],
                       C.byref(info)))
        self._eval_info(info)
        return out

    def population_root_eval(self):
        """azg_population_root_eval: root_eval for any number of nets -- (value [n_trees], dist [n_trees, n_dist]) of the last search,
        rows in tree order k*T + j."""
        fn = self._optional("population_root_eval")
        value = np.empty((self.n_trees,), np.float32)
        dist = np.empty((self.n_trees, self.n_dist), np.float32)
        self._check(fn(self._h, _ptr(value, C.c_float), _ptr(dist, C.c_float)))
        return value, dist

    def policy_rollout(self, episodes_per_net, max_episode_length, rule="mode", game_id_base=0, episode=0):
        """azg_policy_rollout_ex (include/azgym_eval.h; a library without it: azg_policy_rollout, widths up to 256 only):
        ``episodes_per_net`` whole episodes per net played by the network alone, on the device.  Game j of every net starts at the
        reset state of global game ``game_id_base + j``, episode ``episode``.
        Returns a dict of [n_nets, episodes_per_net] arrays: returns (float64), lengths, terminated (bool), first_value.
        ``self.last_rollout_info`` is then what ran: ``form`` ("group" / "team"), ``launches``, ``team_fallbacks`` (None after the
        old entry point, which does not report)."""
        fn_ex = self._f.get("policy_rollout_ex")
        fn = fn_ex if fn_ex is not None else self._optional("policy_rollout")
        c = AzgRolloutConfig()
        c.struct_size = C.sizeof(AzgRolloutConfig)
        c.episodes_per_net, c.max_episode_length = int(episodes_per_net), int(max_episode_length)
        c.action_rule = ROLLOUT_RULE[rule] if isinstance(rule, str) else int(rule)
        c.game_id_base, c.episode = int(game_id_base), int(episode)
        shape = (int(getattr(self, "n_nets", 1)), max(int(episodes_per_net), 0))
        returns = np.empty(shape, np.float64)
        lengths = np.empty(shape, np.int32)
        terminated = np.empty(shape, np.int32)
        first_value = np.empty(shape, np.float32)
        outs = (_ptr(returns, C.c_double), _ptr(lengths, C.c_int32), _ptr(terminated, C.c_int32), _ptr(first_value, C.c_float))
        if fn_ex is not None:
            info = AzgRolloutInfo()
            info.struct_size = C.sizeof(AzgRolloutInfo)
            self._check(fn_ex(self._h, C.byref(c), *outs, C.byref(info)))
            self.last_rollout_info = {"form": ROLLOUT_FORM.get(info.form, str(info.form)), "launches": int(info.launches),
                                      "team_fallbacks": int(info.team_fallbacks)}
        else:
            self._check(fn(self._h, C.byref(c), *outs))
            self.last_rollout_info = None
        return {"returns": returns, "lengths": lengths, "terminated": terminated.astype(bool), "first_value": first_value}

    def search_rollout(self, episodes_per_game, max_episode_length, final_selection="max_visit", deterministic=True, temperature=1.0,
                       agent_epsilon=0.0, game_id_base=0, episode=0, index_base=0, poll_steps=8, out=None):
        """azg_search_rollout (include/azgym_search_rollout.h): every game of the engine plays ``episodes_per_game`` whole episodes
        under MCTS on the device, on evaluation state of its own: self-play, the ring and the running search index are left as they
        were.  Game j of every net starts its i-th episode at the reset state of global game ``game_id_base + j``, episode
        ``episode + i``; step s of the call searches under RNG search index ``index_base + s``.  final_selection / deterministic /
        temperature / agent_epsilon: the final-action rule, as selfplay_begin's.
        Returns a dict of [n_trees, episodes_per_game] arrays: returns (float64), lengths, terminated (bool), and ``steps`` /
        ``polls`` (the searches run; the times the host read the device's count of unfinished games).  ``out``: (returns, lengths,
        terminated int32) arrays to write into."""
        fn = self._optional("search_rollout")
        c = AzgSearchRolloutConfig()
        c.struct_size = C.sizeof(AzgSearchRolloutConfig)
        c.episodes_per_game, c.max_episode_length = int(episodes_per_game), int(max_episode_length)
        c.final_selection = FINAL_SELECTION[final_selection] if isinstance(final_selection, str) else int(final_selection)
        c.deterministic, c.poll_steps = int(bool(deterministic)), int(poll_steps)
        c.game_id_base, c.episode, c.index_base = int(game_id_base) & 0xFFFFFFFF, int(episode) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF
        c.temperature, c.agent_epsilon = float(temperature), float(agent_epsilon)
        shape = (self.n_trees, max(int(episodes_per_game), 0))
        if out is None:
            out = (np.empty(shape, np.float64), np.empty(shape, np.int32), np.empty(shape, np.int32))
        returns, lengths, terminated = out
        for a, dt in zip(out, (np.float64, np.int32, np.int32)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError(f"search_rollout: out must be contiguous float64 / int32 / int32 arrays of shape {shape}")
        info = AzgSearchRolloutInfo()
        info.struct_size = C.sizeof(AzgSearchRolloutInfo)
        self._check(fn(self._h, C.byref(c), _ptr(returns, C.c_double), _ptr(lengths, C.c_int32), _ptr(terminated, C.c_int32), C.byref(info)))
        return {"returns": returns, "lengths": lengths, "terminated": terminated.astype(bool), "steps": int(info.steps),
                "polls": int(info.polls)}

    def dump_tree(self):
        B, R = self.n_trees, self.max_records
        d = {
            "n_records": np.empty((B,), np.int32),
            "parent": np.empty((B, R), np.int32),
            "edge_n": np.empty((B, R), np.int32),
            "edge_W": np.empty((B, R), np.float64),
            "edge_Q": np.empty((B, R), np.float64),
            "edge_action": np.empty((B, R), np.float32),
            "node_n": np.empty((B, R), np.int32),
            "node_r": np.empty((B, R), np.float64),
            "node_V": np.empty((B, R), np.float32),
            "node_flags": np.empty((B, R), np.uint8),
        }
        self._check(self._f["dump_tree"](
            self._h, _ptr(d["n_records"], C.c_int32), _ptr(d["parent"], C.c_int32), _ptr(d["edge_n"], C.c_int32),
            _ptr(d["edge_W"], C.c_double), _ptr(d["edge_Q"], C.c_double), _ptr(d["edge_action"], C.c_float),
            _ptr(d["node_n"], C.c_int32), _ptr(d["node_r"], C.c_double), _ptr(d["node_V"], C.c_float),
            _ptr(d["node_flags"], C.c_uint8)))
        return d


def _selfplay_methods():
    def selfplay_begin(self, max_episode_length, deterministic=False, capacity_steps=64, final_selection="max_visit",
                       temperature=1.0, agent_epsilon=0.0, fifo=False, _symbol="selfplay_begin_ex"):
        """Start device-resident self-play: games reset to their fixed-seed initial states (include/azgym.h).
        final_selection / temperature / agent_epsilon: the agents' final action rule (agents.py:294-301, 524-535);
        fifo: the ring overwrites its oldest step like ReplayBuffer.store (buffers.py:75-82) instead of refusing when full."""
        c = AzgSelfplayConfig()
        c.struct_size = C.sizeof(AzgSelfplayConfig)
        c.max_episode_length = int(max_episode_length)
        c.deterministic = int(bool(deterministic))
        c.capacity_steps = int(capacity_steps)
        c.final_selection = FINAL_SELECTION[final_selection] if isinstance(final_selection, str) else int(final_selection)
        c.ring_mode = 1 if fifo else 0
        c.temperature = float(temperature)
        c.agent_epsilon = float(agent_epsilon)
        self._check(self._optional(_symbol)(self._h, C.byref(c)))
        self._sp_cap = int(capacity_steps)

    def population_selfplay_begin(self, *args, **kw):
        """selfplay_begin for an engine with any number of nets (azg_population_selfplay_begin): net k plays games k*T .. k*T+T-1,
        and its rows of a step are that block of the step's n_trees rows."""
        selfplay_begin(self, *args, _symbol="population_selfplay_begin", **kw)

    def selfplay_ring(self):
        """(size, insert_index, total) of the replay ring in steps: ReplayBuffer.size / .insert_index (buffers.py:56-82)."""
        size, ins, tot = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._f["selfplay_ring"](self._h, C.byref(size), C.byref(ins), C.byref(tot)))
        return size.value, ins.value, tot.value

    def selfplay_rows_device(self):
        """(device pointer, capacity in rows, row length) of the replay ring, for consumers on the same GPU."""
        ptr, cap, rl = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self._f["selfplay_rows_device"](self._h, C.byref(ptr), C.byref(cap), C.byref(rl)))
        return ptr.value, cap.value, rl.value

    def selfplay_step(self):
        """One search + final action + env step + bookkeeping for all games, entirely on the device (asynchronous)."""
        self._check(self._f["selfplay_step"](self._h))

    def _ring_download(self, fn, columns, *extra):
        """The ring's row-aligned downloads: fn(engine, one array per column..., max_rows, extra...) fills arrays that hold the ring's
        capacity in rows and returns the stored rows n; the arrays' first n rows, in order.  columns: (dtype, ctypes type, shape of a
        row).  Before any begin the capacity is 0: nothing to hold, the engine refuses."""
        cap = self._sp_cap * self.n_trees
        arrays = [np.empty((cap,) + tuple(shape), dt) for dt, _, shape in columns]
        n = fn(self._h, *(_ptr(a, ct) for a, (_, ct, _) in zip(arrays, columns)), cap, *extra)
        if n < 0:
            self._check(n)
        return [a[:n] for a in arrays]

    def selfplay_rows(self, clear=True):
        """Replay rows [steps*B, row_len] float32 of the steps since the last clear: obs | actions[K] | counts[K] | Q[K] | V."""
        rl = self._f["selfplay_row_len"](self._h)
        return _ring_download(self, self._f["selfplay_rows"], [(np.float32, C.c_float, (rl,))], int(bool(clear)))[0]

    def selfplay_clear(self):
        """ReplayBuffer.clear (buffers.py:56-60) for the device ring, without downloading anything."""
        n = self._f["selfplay_rows"](self._h, None, 0, 1)
        if n < 0:
            self._check(n)

    def selfplay_stats(self):
        fsum = np.empty((self.n_trees,), np.float64)
        fcnt = np.empty((self.n_trees,), np.int32)
        state = np.empty((self.n_trees, self.s_env), np.float64)
        self._check(self._f["selfplay_stats"](self._h, _ptr(fsum, C.c_double), _ptr(fcnt, C.c_int32), _ptr(state, C.c_double)))
        return fsum, fcnt, state

    def selfplay_keep_states(self, on=True):
        """azg_selfplay_keep_states: keep every stored step's float64 env states beside the replay ring (what selfplay_reanalyse
        searches from).  Right after a begin, while the ring is empty; the next begin drops it."""
        self._check(self._optional("selfplay_keep_states")(self._h, int(bool(on))))

    def selfplay_states(self):
        """The kept env states of the stored steps, [steps*B, S_env] float64, ordered like selfplay_rows."""
        return _ring_download(self, self._optional("selfplay_states"), [(np.float64, C.c_double, (self.s_env,))])[0]

    def selfplay_reanalyse(self, slots=None, search_index=0):
        """azg_selfplay_reanalyse: search stored positions again with the current weights and settings, under RNG search index
        ``search_index``, and overwrite their rows' actions | counts | Q | V_target columns (asynchronous).  ``slots``: an int --
        every game re-searches its position in that ring slot -- or one slot per game, length n_trees (game t rewrites row
        (slots[t], t)); None is slot 0."""
        fn = self._optional("selfplay_reanalyse")
        if slots is None or np.ndim(slots) == 0:
            self._check(fn(self._h, None, int(0 if slots is None else slots), int(search_index) & 0xFFFFFFFF))
            return
        arr = np.ascontiguousarray(slots, dtype=np.int32)
        if arr.shape != (self.n_trees,):
            raise ValueError(f"slots: an int or one slot per game (length {self.n_trees}), got shape {arr.shape}")
        self._check(fn(self._h, _ptr(arr, C.c_int32), 0, int(search_index) & 0xFFFFFFFF))

    def selfplay_keep_transitions(self, on=True):
        """azg_selfplay_keep_transitions: keep every stored step's reward, float64 value target, action and end kind beside the
        replay ring (what selfplay_nstep_targets reads).  Right after a begin, while the ring is empty; the next begin drops it."""
        self._check(self._optional("selfplay_keep_transitions")(self._h, int(bool(on))))

    def selfplay_transitions(self):
        """The kept transitions of the stored steps, ordered like selfplay_rows: a dict of [steps*B] arrays "reward" float64 (in a
        tree node's units: continuous mode divided by reward_scale), "value" float64 (the value target before its rounding to the
        row), "action" float32 and "end" int32 (END_NONE / END_TERMINAL / END_LENGTH)."""
        columns = [(np.float64, C.c_double, ()), (np.float64, C.c_double, ()), (np.float32, C.c_float, ()), (np.int32, C.c_int32, ())]
        return dict(zip(("reward", "value", "action", "end"), _ring_download(self, self._optional("selfplay_transitions"), columns)))

    def selfplay_nstep_targets(self, n_step, gamma=None):
        """azg_selfplay_nstep_targets: rewrite every stored row's V_target column as the n-step return of its game column from the
        kept transitions -- discounted rewards up to the first terminal step, else bootstrapped from the search value n_step steps
        on, at the first time-limit step or at the newest stored step, whichever comes first (include/azgym_nstep.h; asynchronous).
        ``gamma`` None: the search's own gamma, the row's net's where a per-net table is set."""
        c = AzgNstepConfig()
        c.struct_size = C.sizeof(AzgNstepConfig)
        c.n_step = int(n_step)
        c.gamma = 0.0 if gamma is None else float(gamma)
        c.flags = NSTEP_SEARCH_GAMMA if gamma is None else 0
        self._check(self._optional("selfplay_nstep_targets")(self._h, C.byref(c)))

    def selfplay_refresh_values(self, slots=None):
        """azg_selfplay_refresh_values (include/azgym_refresh.h): overwrite the kept float64 value of every row of the ring slots
        ``slots`` (an iterable of ints; None: every stored slot) with the value head's output for the row's stored observation --
        net k's weights of the weight set in use on net k's rows, mlp_eval's float32 value widened (asynchronous: one small copy
        and one launch).  Nothing else is written: selfplay_nstep_targets / selfplay_lambda_targets turn the values into targets."""
        fn = self._optional("selfplay_refresh_values")
        if slots is None:
            self._check(fn(self._h, None, 0))
            return
        arr = np.ascontiguousarray([int(s) for s in slots], dtype=np.int32).reshape(-1)
        buf = arr if arr.size else np.zeros(1, np.int32)   # (an empty list is a list: never the NULL that means every slot)
        self._check(fn(self._h, _ptr(buf, C.c_int32), arr.shape[0]))

    def selfplay_lambda_targets(self, n_step, td_lambda, gamma=None):
        """azg_selfplay_lambda_targets / _nets: rewrite every stored row's V_target column as the lambda-return of its game column
        from the kept transitions -- selfplay_nstep_targets' window of ``n_step`` steps, inside which the returns of the windows 1 ..
        n_step are mixed with weights (1 - lambda) lambda^(m-1), the longest taking the rest (include/azgym_lambda.h; asynchronous).
        ``td_lambda`` 1 is the n-step return, 0 the 1-step return.  Each argument is a scalar or a sequence with one value per net;
        any sequence selects the per-net call, in which net k's games follow entry k.  ``gamma`` None: the search's own gamma, the
        row's net's where a per-net table is set; a sequence may hold None beside numbers (that net: its search's gamma)."""
        K = int(getattr(self, "n_nets", 1))

        def seq(x):
            return x is not None and np.ndim(x) > 0

        if not (seq(n_step) or seq(td_lambda) or seq(gamma)):
            c = AzgReturnRule()
            c.struct_size = C.sizeof(AzgReturnRule)
            c.n_step, c.lambda_ = int(n_step), float(td_lambda)
            c.gamma = 0.0 if gamma is None else float(gamma)
            c.flags = NSTEP_SEARCH_GAMMA if gamma is None else 0
            self._check(self._optional("selfplay_lambda_targets")(self._h, C.byref(c)))
            return
        cols = {}
        for name, x in (("n_step", n_step), ("td_lambda", td_lambda), ("gamma", gamma)):
            cols[name] = list(x) if seq(x) else [x] * K
            if len(cols[name]) != K:
                raise ValueError(f"selfplay_lambda_targets: {name} has {len(cols[name])} entries for {K} nets: a scalar or one per net")
        gammas = cols["gamma"]
        search = all(g is None for g in gammas)
        if not search and any(g is None for g in gammas):   # (the flag is one for the call: resolve the search's gammas here)
            own = getattr(self, "_net_search_gamma", None)
            gammas = [(float(self.cfg.gamma) if own is None else own[k]) if g is None else g for k, g in enumerate(gammas)]
        arr = (AzgReturnRule * K)()
        for k in range(K):
            arr[k].struct_size = C.sizeof(AzgReturnRule)
            arr[k].n_step, arr[k].lambda_ = int(cols["n_step"][k]), float(cols["td_lambda"][k])
            arr[k].gamma = 0.0 if search else float(gammas[k])
            arr[k].flags = NSTEP_SEARCH_GAMMA if search else 0
        self._check(self._optional("selfplay_lambda_targets_nets")(self._h, arr))

    def selfplay_keep_priorities(self, on=True):
        """azg_selfplay_keep_priorities: keep a fixed-point priority per stored row beside the replay ring, and the scratch of the
        proportional draws (include/azgym_priority.h).  After a begin, at any ring size; the next begin drops it."""
        self._check(self._optional("selfplay_keep_priorities")(self._h, int(bool(on))))

    def selfplay_priorities(self, alpha, eps, given=None):
        """azg_selfplay_priorities: the priority of every stored row, (d + eps)^alpha in fixed point (asynchronous: one launch).
        ``given`` None: d is |kept search value - the row's V_target| (needs selfplay_keep_transitions); else d is ``given``, a
        float32 array with one entry >= 0 per stored row, ordered like selfplay_rows."""
        c = AzgPriorityConfig()
        c.struct_size = C.sizeof(AzgPriorityConfig)
        c.source = PRIO_VALUE_GAP if given is None else PRIO_GIVEN
        c.alpha, c.eps = float(alpha), float(eps)
        if given is not None:
            given = np.ascontiguousarray(given, np.float32).reshape(-1)
            size = self.selfplay_ring()[0] if self._sp_cap else 0
            if given.shape[0] != size * self.n_trees:
                raise ValueError(f"given: one entry per stored row ({size * self.n_trees}), got {given.shape[0]}")
            c.given = _ptr(given, C.c_float)
        self._check(self._optional("selfplay_priorities")(self._h, C.byref(c)))

    def selfplay_priority_values(self):
        """The stored rows' priorities as the draws see them: uint64 [steps*B] with 20 fractional bits, ordered like selfplay_rows."""
        return _ring_download(self, self._optional("selfplay_priority_values"), [(np.uint64, C.c_uint64, ())])[0]

    def selfplay_sample_rows(self, n_order, sample_index):
        """azg_selfplay_sample_rows: ``n_order`` row numbers per net drawn in proportion to the priorities, with replacement, on the
        device: int32 [n_nets, n_order], net k's rows numbered slot * T + game as a training epoch over the ring numbers them.  The
        same ``sample_index`` gives the same draws.  Needs selfplay_priorities since the last step, clear or begin."""
        c = AzgSampleConfig()
        c.struct_size = C.sizeof(AzgSampleConfig)
        c.n_order, c.sample_index = int(n_order), int(sample_index) & 0xFFFFFFFF
        order = np.empty((int(getattr(self, "n_nets", 1)), max(int(n_order), 1)), np.int32)
        self._check(self._optional("selfplay_sample_rows")(self._h, C.byref(c), _ptr(order, C.c_int32)))
        return order

    def selfplay_sample_slots(self, sample_index):
        """azg_selfplay_sample_slots: one stored slot per game drawn in proportion to the priorities of the game's column: int32
        [n_trees], what selfplay_reanalyse takes as ``slots``."""
        slots = np.empty(self.n_trees, np.int32)
        self._check(self._optional("selfplay_sample_slots")(self._h, int(sample_index) & 0xFFFFFFFF, _ptr(slots, C.c_int32)))
        return slots

    def selfplay_is_weights(self, beta):
        """azg_selfplay_is_weights: the importance-sampling weight (q_min / q)^beta of every stored row, q_min the least priority of
        the row's net, into a device array slot-aligned with the rows (asynchronous).  Needs selfplay_priorities since the last
        step, clear or begin."""
        self._check(self._optional("selfplay_is_weights")(self._h, float(beta)))

    def selfplay_is_weights_device(self):
        """azg_selfplay_is_weights_device: the device address of the weights [capacity_steps, n_trees] float32, for a trainer on the
        same GPU.  Refused until selfplay_is_weights has run since the stored rows or their priorities last changed."""
        ptr = C.c_void_p()
        self._check(self._optional("selfplay_is_weights_device")(self._h, C.byref(ptr)))
        return int(ptr.value)

    def selfplay_is_weight_values(self):
        """The stored rows' weights as the array holds them: float32 [steps*B], ordered like selfplay_rows."""
        return _ring_download(self, self._optional("selfplay_is_weight_values"), [(np.float32, C.c_float, ())])[0]

    def selfplay_keep_errors(self, on=True):
        """azg_selfplay_keep_errors: keep the trainer's value error per stored row beside the priorities (-1: never trained on since
        it was stored); every step then resets the entries of the slot it stores into.  Needs selfplay_keep_priorities."""
        self._check(self._optional("selfplay_keep_errors")(self._h, int(bool(on))))

    def selfplay_errors_device(self):
        """azg_selfplay_errors_device: the device address of the errors [capacity_steps, n_trees] float32, for a trainer on the same
        GPU to write (PopulationTrainer.train_epoch_ring(errors=True))."""
        ptr = C.c_void_p()
        self._check(self._optional("selfplay_errors_device")(self._h, C.byref(ptr)))
        return int(ptr.value)

    def selfplay_error_values(self):
        """The stored rows' errors as the array holds them: float32 [steps*B], ordered like selfplay_rows."""
        return _ring_download(self, self._optional("selfplay_error_values"), [(np.float32, C.c_float, ())])[0]

    def selfplay_set_error_values(self, err):
        """azg_selfplay_set_error_values: upload one error per stored row, ordered like selfplay_rows; every entry -1, NaN or >= 0."""
        err = np.ascontiguousarray(err, np.float32).reshape(-1)
        self._check(self._optional("selfplay_set_error_values")(self._h, _ptr(err, C.c_float), err.shape[0]))

    def selfplay_priorities_trained(self, alpha, eps, unseen="max"):
        """azg_selfplay_priorities_trained: the priority of every stored row from the kept errors, (d + eps)^alpha in fixed point with
        d the row's error; a row never trained on takes ``unseen``: "max" (the largest seen error of its net, 1 if none),
        "value_gap" (|kept search value - V_target|, needs selfplay_keep_transitions) or a constant d >= 0.  Asynchronous."""
        c = trained_priority_config(alpha, eps, unseen)
        self._check(self._optional("selfplay_priorities_trained")(self._h, C.byref(c)))

    for fn in (selfplay_keep_errors, selfplay_errors_device, selfplay_error_values, selfplay_set_error_values, selfplay_priorities_trained):
        setattr(Engine, fn.__name__, fn)

    for fn in (selfplay_begin, population_selfplay_begin, selfplay_ring, selfplay_rows_device, selfplay_step, selfplay_rows, selfplay_clear, selfplay_stats,
               selfplay_keep_states, selfplay_states, selfplay_reanalyse, selfplay_keep_transitions, selfplay_transitions,
               selfplay_nstep_targets, selfplay_refresh_values, selfplay_lambda_targets, selfplay_keep_priorities, selfplay_priorities, selfplay_priority_values, selfplay_sample_rows,
               selfplay_sample_slots, selfplay_is_weights, selfplay_is_weights_device, selfplay_is_weight_values):
        setattr(Engine, fn.__name__, fn)


_selfplay_methods()


def rmsprop_opt(lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, grad_clip=0.0):
    """azg_rmsprop with torch.optim.RMSprop's keyword names and defaults."""
    o = AzgRmsprop()
    o.struct_size = C.sizeof(AzgRmsprop)
    o.centered = int(bool(centered))
    o.lr, o.alpha, o.eps, o.weight_decay = float(lr), float(alpha), float(eps), float(weight_decay)
    o.momentum, o.grad_clip = float(momentum), float(grad_clip)
    return o


def optim(kind, lr, state0, state1=None, *, eps=None, weight_decay=0.0, alpha=0.99, betas=(0.9, 0.999), grad_clip=0.0, step=0,
          grad_norms=None):
    """azg_optim.  ``kind``: "rmsprop" / "adam" (or OPT_*), with torch.optim.RMSprop's / torch.optim.Adam's keyword names and defaults
    (eps 1e-8); ``state0`` / ``state1`` / ``grad_norms``: device addresses ([n_nets, P] square_avg or exp_avg_sq; [n_nets, P]
    exp_avg; optional [n_nets]); ``step``: the Adam steps taken so far."""
    o = AzgOptim()
    o.struct_size = C.sizeof(AzgOptim)
    o.kind = {"rmsprop": OPT_RMSPROP, "adam": OPT_ADAM}.get(kind, kind)
    o.lr, o.eps, o.weight_decay = float(lr), float(1e-8 if eps is None else eps), float(weight_decay)
    o.alpha, (o.beta1, o.beta2), o.grad_clip = float(alpha), (float(b) for b in betas), float(grad_clip)
    o.state0, o.state1, o.grad_norms = state0 or None, state1 or None, grad_norms or None
    o.step = int(step)
    return o


def loss_cfg(policy, loss):
    """azg_loss_cfg of a policy and loss pairing (one of a population's: all nets share them).  The head kind comes from the
    policy's class, the loss kind from the loss's; names, not isinstance, so that the reference's objects work alike.  Raises
    ``ValueError`` for what ``population_loss`` refuses."""
    head = {"DiscretePolicy": HEAD_DISCRETE, "DiagonalNormalPolicy": HEAD_NORMAL, "DiagonalGMMPolicy": HEAD_GMM}.get(type(policy).__name__)
    kind = {"AlphaZeroLoss": LOSS_ALPHAZERO, "A0CLoss": LOSS_A0C, "A0CLossTuned": LOSS_A0C_TUNED}.get(type(loss).__name__)
    if head is None:
        raise ValueError(f"loss_cfg: {type(policy).__name__} heads are not supported")
    if kind is None:
        raise ValueError(f"loss_cfg: {type(loss).__name__} is not supported")
    if kind == LOSS_ALPHAZERO and head != HEAD_DISCRETE:
        raise ValueError("loss_cfg: AlphaZeroLoss needs a discrete policy")
    if loss.reduction not in REDUCE:
        raise ValueError("loss_cfg: reduction must be 'mean' or 'sum'")
    if head == HEAD_GMM and policy.num_components > 5:
        raise ValueError("loss_cfg: at most 5 mixture components")
    c = AzgLossCfg()
    c.struct_size = C.sizeof(AzgLossCfg)
    c.kind, c.head, c.reduction = kind, head, REDUCE[loss.reduction]
    c.policy_coeff, c.value_coeff = float(loss.policy_coeff), float(loss.value_coeff)
    c.action_bound = float(getattr(policy, "action_bound", 0.0) or 0.0) if head != HEAD_DISCRETE else 0.0
    if kind != LOSS_ALPHAZERO:
        c.tau = float(loss.tau)
    if kind == LOSS_A0C:
        c.alpha = float(loss.alpha)
    if kind == LOSS_A0C_TUNED:
        g = loss.optimizer.param_groups[0]
        if type(loss.optimizer).__name__ != "Adam" or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("loss_cfg: the learned temperature's optimiser must be plain torch.optim.Adam")
        c.target_entropy = float(loss.target_entropy)
        c.alpha_lr, (c.alpha_beta1, c.alpha_beta2) = float(g["lr"]), (float(b) for b in g["betas"])
        c.alpha_eps, c.alpha_weight_decay, c.alpha_clip = float(g["eps"]), float(g["weight_decay"]), float(loss.clip or 0.0)
    return c


def alpha_state(step, log_alpha, exp_avg, exp_avg_sq):
    """azg_alpha_state: ``step`` Adam steps taken so far, and the device addresses of the three [n_nets] float32 arrays."""
    s = AzgAlphaState()
    s.struct_size = C.sizeof(AzgAlphaState)
    s.step = int(step)
    s.log_alpha, s.exp_avg, s.exp_avg_sq = log_alpha or None, exp_avg or None, exp_avg_sq or None
    return s


def epoch_rows(rows, state_dim, n_actions, rows_per_net, *, ring_trees=None, games_per_net=None):
    """azg_epoch_rows: where a population's replay rows lie (``rows``: their device address).  Default: a plain
    [n_nets, rows_per_net, row_len] array.  With ``ring_trees`` (the engine's n_trees) and ``games_per_net`` (T): the self-play
    ring [capacity_steps, n_trees, row_len], where net k's row i is step i // T, game k * T + i % T -- the numbering of
    ``PopulationSelfPlay._split``'s copies."""
    r = AzgEpochRows()
    r.struct_size = C.sizeof(AzgEpochRows)
    r.state_dim, r.n_actions = int(state_dim), int(n_actions)
    r.row_len = r.state_dim + 3 * r.n_actions + 1
    r.rows_per_net = int(rows_per_net)
    if ring_trees is None:
        r.group, r.group_stride, r.net_stride = r.rows_per_net, r.rows_per_net, r.rows_per_net
    else:
        r.group, r.group_stride, r.net_stride = int(games_per_net), int(ring_trees), int(games_per_net)
    r.rows = rows or None
    return r


def _ref(x):
    """``byref(x)``; None stays NULL."""
    return C.byref(x) if x is not None else None


def _require(fns, symbol, what=None):
    """The library's ``symbol``, or the refusal that names what it lacks."""
    if symbol not in fns:
        raise NotImplementedError(f"this engine library has no azg_{what or symbol}")
    return fns[symbol]


class Trainer:
    """One ``azg_trainer*`` (include/azgym_train.h): forward and backward + RMSprop step of n_nets nets of shape ``desc`` in two
    launches.  Every array argument is a device address (int) of float32 memory on the trainer's GPU, complete when the call is
    made; outputs are complete when it returns.  ``layernorm=True`` creates it with azg_trainer_create_ex, which also takes
    descriptors of LayerNorm trunks (per trunk layer weight, bias, ln.weight, ln.bias in ``params``).  ``wide=True`` creates it with
    azg_trainer_create_wide: 1-8 hidden layers of widths up to 1024 (no LayerNorm), a launch per layer; every method works the same.
    ``wide_layernorm=True`` creates it with azg_trainer_create_wide_ex and options.layernorm set: the wide trainer that also takes
    descriptors of LayerNorm trunks."""

    # which azg_trainer_create* a constructor flag asks for, in the order they are looked at: (flag, symbol, with options)
    _CREATE = (("wide_layernorm", "trainer_create_wide_ex", True), ("wide", "trainer_create_wide", False),
               ("layernorm", "trainer_create_ex", True))

    def __init__(self, fns, desc, n_nets, max_batch, device_id=0, layernorm=False, wide=False, wide_layernorm=False):
        if wide and layernorm:
            raise ValueError("Trainer: wide=True does not take LayerNorm trunks (layernorm=True)")
        if wide_layernorm and layernorm:
            raise ValueError("Trainer: wide_layernorm=True and layernorm=True ask for two different trainers")
        _require(fns, "trainer_create", "trainer_* entry points")
        flags = {"wide_layernorm": wide_layernorm, "wide": wide, "layernorm": layernorm}
        asked = [(symbol, options) for flag, symbol, options in self._CREATE if flags[flag]] + [("trainer_create", False)]
        for symbol, _ in asked:   # (every refusal before any native call)
            _require(fns, symbol)
        symbol, options = asked[0]
        self._f = fns
        self._h = C.c_void_p()
        args = [int(device_id), _ref(desc), int(n_nets), int(max_batch)]
        if options:
            opts = AzgTrainerOptions(C.sizeof(AzgTrainerOptions), 1)
            args.append(C.byref(opts))
        rc = fns[symbol](*args, C.byref(self._h))
        if rc != 0:
            raise EngineError(rc, (fns["trainer_last_error"](None) or b"").decode())
        self.n_nets, self.max_batch, self.device_id = int(n_nets), int(max_batch), int(device_id)
        self.n_params = int(fns["trainer_param_count"](self._h))
        self.n_raw = 1 + desc.n_dist
        self.in_dim = desc.in_dim

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, (self._f["trainer_last_error"](self._h) or b"").decode())

    def close(self):
        if self._h:
            self._f["trainer_destroy"](self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _order(self, who, order):
        """An epoch's ``order`` as (n_order, pointer to its int32 copy); None stays NULL."""
        if order is None:
            return 0, None
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.ndim != 2 or order.shape[0] != self.n_nets:
            raise ValueError(f"Trainer.{who}: order must be [n_nets, n_order]")
        return order.shape[1], _ptr(order, C.c_int32)

    # The three forms of every call differ in the native symbol, in ``cfg`` (a reference to one azg_loss_cfg, or the array of
    # ``_entries``) and in ``opt``, the optimiser's arguments as the symbol takes them: (azg_rmsprop, square_avg), (azg_optim,) or
    # (the array of azg_optim,).

    def _backward_step(self, symbol, params, d_raw, n_rows, opt, grads):
        self._check(_require(self._f, symbol)(self._h, params or None, d_raw or None, int(n_rows), *opt, grads or None))

    # ``weights``: () for the unweighted symbols, (address,) for the *_weighted ones, whose extra argument follows the row arrays.

    def _loss(self, symbol, raw, actions, counts, values, n_rows, n_actions, cfg, alpha, d_raw, losses, weights=()):
        self._check(_require(self._f, symbol)(self._h, raw or None, actions or None, counts or None, values or None, *weights, int(n_rows),
                                              int(n_actions), cfg, _ref(alpha), d_raw or None, losses or None))

    def _step(self, symbol, params, obs, actions, counts, values, n_rows, n_actions, cfg, alpha, opt, grads, raw_out, losses, weights=()):
        self._check(_require(self._f, symbol)(self._h, params or None, obs or None, actions or None, counts or None, values or None,
                                              *weights, int(n_rows), int(n_actions), cfg, _ref(alpha), *opt, grads or None, raw_out or None,
                                              losses or None))

    def _epoch(self, symbol, who, params, rows, order, batch_size, cfg, alpha, opt, loss_sums, weights=()):
        fn = _require(self._f, symbol)
        n_order, ptr = self._order(who, order)
        n_mb = C.c_int32(0)
        self._check(fn(self._h, params or None, _ref(rows), *weights, ptr, n_order, int(batch_size), cfg, _ref(alpha), *opt, loss_sums or None,
                       C.byref(n_mb)))
        return n_mb.value

    def forward(self, params, obs, n_rows, raw):
        """azg_trainer_forward: params [n_nets, P], obs [n_nets, n_rows, in_dim] -> raw [n_nets, n_rows, 1 + n_dist]."""
        self._check(self._f["trainer_forward"](self._h, params or None, obs or None, int(n_rows), raw or None))

    def backward_step(self, params, d_raw, n_rows, opt, square_avg, grads=None):
        """azg_trainer_backward_step: back from d_raw, RMSprop update of params / square_avg in place; grads (optional) filled."""
        self._backward_step("trainer_backward_step", params, d_raw, n_rows, (_ref(opt), square_avg or None), grads)

    def loss(self, raw, actions, counts, values, n_rows, n_actions, cfg, alpha, d_raw, losses):
        """azg_trainer_loss: the loss kernel alone.  raw [n_nets, n_rows, 1 + n_dist], actions / counts [n_nets, n_rows, n_actions],
        values [n_nets, n_rows] -> d_raw (raw's shape) and losses [n_nets, 5] (``LOSS_KEYS``); ``alpha`` (``alpha_state``, for
        A0CLossTuned) is stepped in place."""
        self._loss("trainer_loss", raw, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha, d_raw, losses)

    def step(self, params, obs, actions, counts, values, n_rows, n_actions, cfg, alpha, opt, square_avg, grads, raw_out, losses):
        """azg_trainer_step: forward, loss and backward + RMSprop of every net, three launches and one synchronisation."""
        self._step("trainer_step", params, obs, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha,
                   (_ref(opt), square_avg or None), grads, raw_out, losses)

    def epoch(self, params, rows, order, batch_size, cfg, alpha, opt, square_avg, loss_sums):
        """azg_trainer_epoch: one epoch of ``step``s of every net, the minibatches gathered on the device from ``rows``
        (``epoch_rows``) by ``order`` (a HOST int array [n_nets, n_order]; consecutive slices of ``batch_size``, the last one
        absorbing the remainder); one synchronisation.  ``loss_sums``: device float64 [n_nets, 5].  Returns the number of
        minibatches (= Adam steps of a tuned alpha)."""
        return self._epoch("trainer_epoch", "epoch", params, rows, order, batch_size, _ref(cfg), alpha, (_ref(opt), square_avg or None),
                           loss_sums)

    def backward_step_opt(self, params, d_raw, n_rows, opt, grads=None):
        """azg_trainer_backward_step_opt: ``backward_step`` with an ``optim`` (RMSprop or Adam, optional gradient clipping; the
        optimiser state's addresses are in ``opt``)."""
        self._backward_step("trainer_backward_step_opt", params, d_raw, n_rows, (_ref(opt),), grads)

    def step_opt(self, params, obs, actions, counts, values, n_rows, n_actions, cfg, alpha, opt, grads, raw_out, losses):
        """azg_trainer_step_opt: ``step`` with an ``optim``."""
        self._step("trainer_step_opt", params, obs, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha, (_ref(opt),), grads,
                   raw_out, losses)

    def epoch_opt(self, params, rows, order, batch_size, cfg, alpha, opt, loss_sums):
        """azg_trainer_epoch_opt: ``epoch`` with an ``optim``; minibatch m is Adam step ``opt.step + m + 1``.  Returns the number of
        minibatches."""
        return self._epoch("trainer_epoch_opt", "epoch_opt", params, rows, order, batch_size, _ref(cfg), alpha, (_ref(opt),), loss_sums)

    # ---- per-net settings: the *_opt calls with one azg_optim / azg_loss_cfg per net ----

    def _entries(self, who, items, ctype):
        """A sequence of n_nets ``ctype`` structures as the contiguous array the *_nets entry points read (None stays NULL)."""
        _require(self._f, "trainer_step_nets", "trainer_*_nets entry points")
        if items is None:
            return None
        if isinstance(items, C.Array) and items._type_ is ctype and len(items) == self.n_nets:   # (ready: no copy)
            return items
        items = list(items)
        if len(items) != self.n_nets:
            raise ValueError(f"Trainer.{who}: one {ctype.__name__} per net ({self.n_nets}), not {len(items)}")
        return (ctype * len(items))(*items)

    def backward_step_nets(self, params, d_raw, n_rows, opts, grads=None):
        """azg_trainer_backward_step_nets: ``backward_step_opt`` with ``opts``, a sequence of n_nets ``optim``s whose numeric
        settings (lr, eps, weight_decay, alpha, betas, grad_clip) may differ; kind, state addresses and step must be equal."""
        arr = self._entries("backward_step_nets", opts, AzgOptim)
        self._backward_step("trainer_backward_step_nets", params, d_raw, n_rows, (arr,), grads)

    def loss_nets(self, raw, actions, counts, values, n_rows, n_actions, cfgs, alpha, d_raw, losses):
        """azg_trainer_loss_nets: ``loss`` with ``cfgs``, a sequence of n_nets ``loss_cfg``s whose numeric settings may differ;
        kind, head, reduction and action_bound must be equal."""
        arr = self._entries("loss_nets", cfgs, AzgLossCfg)
        self._loss("trainer_loss_nets", raw, actions, counts, values, n_rows, n_actions, arr, alpha, d_raw, losses)

    def step_nets(self, params, obs, actions, counts, values, n_rows, n_actions, cfgs, alpha, opts, grads, raw_out, losses):
        """azg_trainer_step_nets: ``step_opt`` with one ``loss_cfg`` and one ``optim`` per net."""
        carr, oarr = self._entries("step_nets", cfgs, AzgLossCfg), self._entries("step_nets", opts, AzgOptim)
        self._step("trainer_step_nets", params, obs, actions, counts, values, n_rows, n_actions, carr, alpha, (oarr,), grads, raw_out,
                   losses)

    def epoch_nets(self, params, rows, order, batch_size, cfgs, alpha, opts, loss_sums):
        """azg_trainer_epoch_nets: ``epoch_opt`` with one ``loss_cfg`` and one ``optim`` per net.  Returns the number of
        minibatches."""
        carr, oarr = self._entries("epoch_nets", cfgs, AzgLossCfg), self._entries("epoch_nets", opts, AzgOptim)
        return self._epoch("trainer_epoch_nets", "epoch_nets", params, rows, order, batch_size, carr, alpha, (oarr,), loss_sums)

    # ---- weighted losses (include/azgym_train_weighted.h): the namesake with ``weights``, a device address of float32 ----

    def loss_weighted(self, raw, actions, counts, values, weights, n_rows, n_actions, cfg, alpha, d_raw, losses):
        """azg_trainer_loss_weighted: ``loss`` with a weight per row, weights [n_nets, n_rows], multiplied into the row's summands of
        every loss and into its d_raw in float64; the reductions stay.  Weights of 1 give ``loss``'s bits."""
        self._loss("trainer_loss_weighted", raw, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha, d_raw, losses,
                   (weights or None,))

    def loss_nets_weighted(self, raw, actions, counts, values, weights, n_rows, n_actions, cfgs, alpha, d_raw, losses):
        """azg_trainer_loss_nets_weighted: ``loss_nets`` with a weight per row."""
        arr = self._entries("loss_nets_weighted", cfgs, AzgLossCfg)
        self._loss("trainer_loss_nets_weighted", raw, actions, counts, values, n_rows, n_actions, arr, alpha, d_raw, losses,
                   (weights or None,))

    def step_opt_weighted(self, params, obs, actions, counts, values, weights, n_rows, n_actions, cfg, alpha, opt, grads, raw_out, losses):
        """azg_trainer_step_opt_weighted: ``step_opt`` with a weight per row, weights [n_nets, n_rows]."""
        self._step("trainer_step_opt_weighted", params, obs, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha, (_ref(opt),),
                   grads, raw_out, losses, (weights or None,))

    def step_nets_weighted(self, params, obs, actions, counts, values, weights, n_rows, n_actions, cfgs, alpha, opts, grads, raw_out,
                           losses):
        """azg_trainer_step_nets_weighted: ``step_nets`` with a weight per row."""
        carr, oarr = self._entries("step_nets_weighted", cfgs, AzgLossCfg), self._entries("step_nets_weighted", opts, AzgOptim)
        self._step("trainer_step_nets_weighted", params, obs, actions, counts, values, n_rows, n_actions, carr, alpha, (oarr,), grads,
                   raw_out, losses, (weights or None,))

    def epoch_opt_weighted(self, params, rows, weights, order, batch_size, cfg, alpha, opt, loss_sums):
        """azg_trainer_epoch_opt_weighted: ``epoch_opt`` with a weight per replay row.  ``weights`` is addressed like ``rows`` with a
        row length of 1: [n_nets, rows_per_net] beside a plain rows array, [capacity_steps, n_trees] beside the self-play ring
        (``Engine.selfplay_is_weights_device``)."""
        return self._epoch("trainer_epoch_opt_weighted", "epoch_opt_weighted", params, rows, order, batch_size, _ref(cfg), alpha,
                           (_ref(opt),), loss_sums, (weights or None,))

    def epoch_nets_weighted(self, params, rows, weights, order, batch_size, cfgs, alpha, opts, loss_sums):
        """azg_trainer_epoch_nets_weighted: ``epoch_nets`` with a weight per replay row."""
        carr, oarr = self._entries("epoch_nets_weighted", cfgs, AzgLossCfg), self._entries("epoch_nets_weighted", opts, AzgOptim)
        return self._epoch("trainer_epoch_nets_weighted", "epoch_nets_weighted", params, rows, order, batch_size, carr, alpha, (oarr,),
                           loss_sums, (weights or None,))

    # ---- value errors out of the loss launch (include/azgym_train_errors.h): the weighted namesake with ``errors``, a device
    # address of float32 that receives |V - z| of every row; ``weights`` may be None (unweighted) ----

    def loss_errors(self, raw, actions, counts, values, weights, errors, n_rows, n_actions, cfg, alpha, d_raw, losses):
        """azg_trainer_loss_errors: ``loss_weighted`` that also writes errors [n_nets, n_rows]."""
        self._loss("trainer_loss_errors", raw, actions, counts, values, n_rows, n_actions, _ref(cfg), alpha, d_raw, losses,
                   (weights or None, errors or None))

    def loss_nets_errors(self, raw, actions, counts, values, weights, errors, n_rows, n_actions, cfgs, alpha, d_raw, losses):
        """azg_trainer_loss_nets_errors: ``loss_nets_weighted`` that also writes errors [n_nets, n_rows]."""
        arr = self._entries("loss_nets_errors", cfgs, AzgLossCfg)
        self._loss("trainer_loss_nets_errors", raw, actions, counts, values, n_rows, n_actions, arr, alpha, d_raw, losses,
                   (weights or None, errors or None))

    def epoch_opt_errors(self, params, rows, weights, errors, order, batch_size, cfg, alpha, opt, loss_sums):
        """azg_trainer_epoch_opt_errors: ``epoch_opt_weighted`` whose loss launches also write every trained row's error into
        ``errors``, addressed like ``weights``: [n_nets, rows_per_net] beside a plain rows array, [capacity_steps, n_trees] beside
        the self-play ring (``Engine.selfplay_errors_device``).  Rows not drawn keep their entries."""
        return self._epoch("trainer_epoch_opt_errors", "epoch_opt_errors", params, rows, order, batch_size, _ref(cfg), alpha,
                           (_ref(opt),), loss_sums, (weights or None, errors or None))

    def epoch_nets_errors(self, params, rows, weights, errors, order, batch_size, cfgs, alpha, opts, loss_sums):
        """azg_trainer_epoch_nets_errors: ``epoch_nets_weighted`` that also writes the trained rows' errors."""
        carr, oarr = self._entries("epoch_nets_errors", cfgs, AzgLossCfg), self._entries("epoch_nets_errors", opts, AzgOptim)
        return self._epoch("trainer_epoch_nets_errors", "epoch_nets_errors", params, rows, order, batch_size, carr, alpha, (oarr,),
                           loss_sums, (weights or None, errors or None))

    # ---- the online epoch (include/azgym_train_online.h): every minibatch redrawn from the engine's refreshed priorities ----

    def _epoch_online(self, symbol, engine, params, n_minibatches, batch_size, sample_index, beta, prio, cfg, alpha, opt, loss_sums,
                      return_drawn):
        fn = _require(self._f, symbol, "azg_trainer_epoch_online")
        c = AzgOnlineEpoch()
        c.struct_size = C.sizeof(AzgOnlineEpoch)
        c.n_minibatches, c.batch_size = int(n_minibatches), int(batch_size)
        c.sample_index, c.beta = int(sample_index) & 0xFFFFFFFF, float(beta)
        c.prio = prio
        drawn = None
        if return_drawn:
            drawn = np.empty((max(c.n_minibatches, 0), self.n_nets, max(c.batch_size, 0)), np.int32)
            c.drawn = _ptr(drawn, C.c_int32)
        self._check(fn(self._h, engine._h if engine is not None else None, params or None, C.byref(c), cfg, _ref(alpha), opt,
                       loss_sums or None))
        return drawn

    def epoch_online(self, engine, params, n_minibatches, batch_size, sample_index, beta, prio, cfg, alpha, opt, loss_sums,
                     return_drawn=False):
        """azg_trainer_epoch_online: ``n_minibatches`` minibatches of ``batch_size`` rows per net over ``engine``'s replay ring, each
        drawn under ``sample_index + m`` from priorities refreshed (``prio``: ``trained_priority_config``) with the errors of the
        minibatches before it and weighted by (q_min / q)^beta; one synchronisation.  Equal, bit for bit, to the loop of
        selfplay_priorities_trained, selfplay_sample_rows, selfplay_is_weights and epoch_opt_errors.  Returns the drawn rows, int32
        [n_minibatches, n_nets, batch_size], when asked."""
        return self._epoch_online("trainer_epoch_online", engine, params, n_minibatches, batch_size, sample_index, beta, prio, _ref(cfg),
                                  alpha, _ref(opt), loss_sums, return_drawn)

    def epoch_online_nets(self, engine, params, n_minibatches, batch_size, sample_index, beta, prio, cfgs, alpha, opts, loss_sums,
                          return_drawn=False):
        """azg_trainer_epoch_online_nets: ``epoch_online`` with one ``loss_cfg`` and one ``optim`` per net."""
        carr, oarr = self._entries("epoch_online_nets", cfgs, AzgLossCfg), self._entries("epoch_online_nets", opts, AzgOptim)
        return self._epoch_online("trainer_epoch_online_nets", engine, params, n_minibatches, batch_size, sample_index, beta, prio, carr,
                                  alpha, oarr, loss_sums, return_drawn)

    def read_d_raw(self, n_rows, d_raw):
        """azg_trainer_read_d_raw: the last ``step``'s d_raw [n_nets, n_rows, 1 + n_dist] into the caller's device array."""
        self._check(self._f["trainer_read_d_raw"](self._h, int(n_rows), d_raw or None))

    # ---- the moving average of the parameters (include/azgym_train_ema.h) ----

    def set_ema(self, ema, decay=None, every=1):
        """azg_trainer_set_ema: from now on every ``every``-th optimiser step is followed by ema += (1 - decay) * (params - ema) on
        the device.  ``ema``: the device address of the caller's float32 [n_nets, P] array, which must stay alive; ``decay``: one
        number or one per net, each in [0, 1).  ``ema`` None detaches."""
        fn = _require(self._f, "trainer_set_ema")
        if ema is None:
            self._check(fn(self._h, None))
            return
        decays = [float(d) for d in (decay if np.ndim(decay) else [decay])]
        arr = (C.c_double * max(len(decays), 1))(*decays)
        cfg = AzgEmaCfg(C.sizeof(AzgEmaCfg), len(decays), int(every), 0, ema or None, arr)
        self._check(fn(self._h, C.byref(cfg)))

    def ema_info(self):
        """azg_trainer_ema_info: (optimiser steps seen, launches of the average's kernel) since the last attach."""
        steps, updates = C.c_int64(0), C.c_int64(0)
        self._check(_require(self._f, "trainer_ema_info")(self._h, C.byref(steps), C.byref(updates)))
        return steps.value, updates.value


# Which ``Trainer`` method serves a (family, variant) call of a trainer whose optimiser arguments have the form "rmsprop" (an
# azg_rmsprop and square_avg), "opt" (one azg_optim) or "nets" (an array of azg_optim, and of azg_loss_cfg), and the form in which
# that method takes them.  azg_rmsprop has no weighted, errors or online entry point: those calls of its trainer go to the *_opt ones.
_T = Trainer
TRAINER_CALLS = {
    "opt": {("backward_step", "plain"): (_T.backward_step_opt, "opt"), ("step", "plain"): (_T.step_opt, "opt"),
            ("step", "weighted"): (_T.step_opt_weighted, "opt"), ("epoch", "plain"): (_T.epoch_opt, "opt"),
            ("epoch", "weighted"): (_T.epoch_opt_weighted, "opt"), ("epoch", "errors"): (_T.epoch_opt_errors, "opt"),
            ("epoch", "online"): (_T.epoch_online, "opt")},
    "nets": {("backward_step", "plain"): (_T.backward_step_nets, "nets"), ("step", "plain"): (_T.step_nets, "nets"),
             ("step", "weighted"): (_T.step_nets_weighted, "nets"), ("epoch", "plain"): (_T.epoch_nets, "nets"),
             ("epoch", "weighted"): (_T.epoch_nets_weighted, "nets"), ("epoch", "errors"): (_T.epoch_nets_errors, "nets"),
             ("epoch", "online"): (_T.epoch_online_nets, "nets")},
}
TRAINER_CALLS["rmsprop"] = {**TRAINER_CALLS["opt"], ("backward_step", "plain"): (_T.backward_step, "rmsprop"),
                            ("step", "plain"): (_T.step, "rmsprop"), ("epoch", "plain"): (_T.epoch, "rmsprop")}
del _T


def pw_table(c_pw, kappa, n):
    """NodeContinuous.check_pw's threshold (alphazero/search/states.py:271-273) for visit counts 0..n-1."""
    return [math.ceil(c_pw * ((i + 1) ** kappa)) for i in range(n)]
