"""MCTS with the reference's class surface (alphazero/search/mcts.py), executed by the MI355X engine.

``MCTSDiscrete`` / ``MCTSContinuous`` keep the reference's constructor kwargs (mcts.py:316-327, 537-549), the
attributes the agents poke (``root_node``, ``root_state``, ``n_rollouts``, ``c_uct``, ``gamma``), ``search(Env)``,
``return_results(final_selection)`` and (discrete) ``forward(action, state)``; ``model`` is the torch policy whose
weights the engine evaluates on the GPU.  One ``search`` call is ONE kernel launch that runs all ``n_rollouts`` traces.

``BatchedMCTS`` is the native interface: B independent trees per call (``Env`` may also be a list of environments
for the two classes above).  ``PopulationMCTS`` searches the trees of K models, each with its own weights, in one launch.
There is no CPU fallback; constructing an engine without the HIP library or a GPU raises.
"""
import contextlib
import warnings
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from .. import _capi

PENDULUM_R_SCALE = _capi.PENDULUM_R_SCALE  # scales the step reward between -1 and 0 (mcts.py:19-20)


def env_signature(env) -> Tuple[int, np.ndarray]:
    """(engine env id, float64 internal state) of a supported environment object."""
    u = getattr(env, "unwrapped", env)
    if hasattr(u, "azg_env_id"):
        return int(u.azg_env_id), np.asarray(u.azg_state(), dtype=np.float64)
    name = type(u).__name__
    if name == "CartPoleEnv":
        return _capi.ENV_CARTPOLE, np.asarray(u.state, dtype=np.float64)
    if name == "MountainCarEnv":
        return _capi.ENV_MOUNTAINCAR, np.asarray(u.state, dtype=np.float64)
    if name == "AcrobotEnv":
        return _capi.ENV_ACROBOT, np.asarray(u.state, dtype=np.float64)
    if name == "Continuous_MountainCarEnv":
        return _capi.ENV_MOUNTAINCAR_CONT, np.asarray(u.state, dtype=np.float64)
    if name == "PendulumEnv":
        spec = getattr(getattr(u, "spec", None), "id", "") or ""
        return (_capi.ENV_PENDULUM_V0 if spec.endswith("v0") else _capi.ENV_PENDULUM_V1), np.asarray(u.state, dtype=np.float64)
    raise NotImplementedError(
        f"{name}: the engine steps CartPole, MountainCar, MountainCarContinuous, Acrobot and Pendulum in closed form on the GPU; other "
        "environments are not supported")


def env_observation(env_id: int, st: np.ndarray) -> np.ndarray:
    """float32 observation the reference's nodes keep as ``state`` for an engine state: Acrobot observes (cos, sin) of both joint
    angles and the two velocities (gym acrobot.py _get_ob), Pendulum (cos, sin, thdot); the others observe their state."""
    st = np.asarray(st, dtype=np.float64)
    if env_id == _capi.ENV_ACROBOT:
        return np.array([np.cos(st[0]), np.sin(st[0]), np.cos(st[1]), np.sin(st[1]), st[2], st[3]], dtype=np.float32)
    if env_id in (_capi.ENV_PENDULUM_V0, _capi.ENV_PENDULUM_V1):
        return np.array([np.cos(st[0]), np.sin(st[0]), st[1]], dtype=np.float32)
    return st.astype(np.float32)


def _weights_version(model) -> Tuple:
    """Changes whenever a parameter is written in place (optimiser step, copy_, broadcast: ``_version``) or rebound to
    new storage (``p.data = ...``, ``load_state_dict(assign=True)``: ``data_ptr``)."""
    return tuple((id(p), p._version, p.data_ptr()) for p in model.parameters())


def device_ordinal(device) -> int:
    """GPU ordinal for the reference's ``device`` kwarg (mcts.py:316-327).  "cuda:N" -> N; "cuda" -> torch's current device;
    anything else (the reference's configs say "cpu": that is where ITS network ran) -> LOCAL_RANK, so that one agent per
    rank lands on its own GPU, else 0."""
    import os
    try:
        import torch
        d = torch.device(device) if device is not None else None
        if d is not None and d.type == "cuda":
            if d.index is not None:
                return int(d.index)
            if torch.cuda.is_available():
                return int(torch.cuda.current_device())
    except (RuntimeError, TypeError):
        pass
    return int(os.environ.get("LOCAL_RANK", "0"))


class PopulationMCTS:
    """K models (same network shape, own weights) searched in ONE launch: trees k*T .. k*T+T-1 (T = ``trees_per_model``) use
    ``models[k]``, with the RNG streams of global trees ``tree_id_base + k*T + j`` -- what K ``BatchedMCTS`` engines with
    ``tree_id_base + k*T`` compute, one launch and one synchronisation instead of K (azg_set_population).  kwargs = the reference's
    MCTS kwargs + batch geometry; the search index is shared, and so are the search settings unless ``net_settings`` is given.  Each
    model's weights are re-uploaded only when they changed (models train at different times).  One model is the plain single-net engine.

    ``net_settings`` (opt-in; None: shared settings): a list of K dicts with keys among ``c_uct``, ``gamma``, ``epsilon``, ``c_pw``,
    ``kappa`` -- model k searches with its own values, a missing key takes the shared kwarg -- still in one launch, bit for bit what a
    one-model engine with those kwargs computes (azg_set_net_search).  The engine is created with the (c_pw, kappa) pair that widens
    furthest, so that every model's trees fit; ``set_net_settings`` changes the settings between searches.  Networks of padded hidden
    width >= 512 need ``net_settings_wide=True`` (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE: the team, per-layer and wide
    one-launch kernels' table forms); without it they search with shared settings only: ValueError.

    ``net_rollouts`` (opt-in; None: every model runs ``n_rollouts``): K ints in 1 .. ``n_rollouts`` -- model k runs its own number of
    simulations per search, in the same launch, bit for bit what a one-model engine created with that ``n_rollouts`` computes
    (azg_net_search.n_sims).  ``n_rollouts`` stays the engine's capacity: storage, tables and the kernel form follow it.  With or
    without ``net_settings`` (without: every model's five settings are the shared ones); the same width and ``net_settings_wide``
    rules apply.  ``set_net_rollouts`` changes the budgets between searches."""

    def __init__(self, models: Sequence[Any], *, trees_per_model: int = 1, env_id: int, mode: int, n_rollouts: int, c_uct: float,
                 gamma: float, epsilon: float = 0.0, num_actions: int = 0, c_pw: float = 1.0, kappa: float = 0.5,
                 V_target_policy: str = "off_policy", action_bound: float = 2.0, seed: int = 34, tree_id_base: int = 0,
                 device_id: int = 0, net_settings: Optional[Sequence[dict]] = None, net_settings_wide: bool = False,
                 net_rollouts: Optional[Sequence[int]] = None):
        from .. import _native   # raises if libazgym_hip.so is missing

        self.models = list(models)
        if not self.models or trees_per_model < 1:
            raise ValueError("PopulationMCTS needs at least one model and trees_per_model >= 1")
        self.n_models = len(self.models)
        self.n_rollouts = int(n_rollouts)
        self._shared = dict(c_uct=c_uct, gamma=gamma, epsilon=epsilon, c_pw=c_pw, kappa=kappa)
        self.net_settings: Optional[List[dict]] = None
        self.net_settings_wide = bool(net_settings_wide)
        self.net_rollouts: Optional[List[int]] = None
        self.trees_per_model = int(trees_per_model)
        rollouts = None if net_rollouts is None else self._net_budgets(net_rollouts, self.net_settings_wide)
        if net_settings is not None:
            entries = self._net_entries(net_settings, self.net_settings_wide)
            if mode == _capi.MODE_CONTINUOUS:
                c_pw, kappa = _capi.widest_pw(entries, self.n_rollouts)
        self.n_trees = self.n_models * self.trees_per_model
        self.engine = _native.HipEngine(env_id=env_id, mode=mode, n_trees=self.n_trees, n_sims=n_rollouts, c_uct=c_uct, gamma=gamma,
                                        epsilon=epsilon, num_actions=num_actions, c_pw=c_pw, kappa=kappa, v_target=V_target_policy,
                                        action_bound=action_bound, seed=seed, tree_id_base=tree_id_base, device_id=device_id)
        if self.n_models > 1:   # (one model: the plain engine, which the tests' CPU oracle -- no population entry points -- also is)
            self.engine.set_population(self.n_models)
        self._versions: List[Any] = [None] * self.n_models
        self._in_target = False   # inside target_weights(): the engine's TARGET weight set is in use
        self._cliff_warned = False
        self.last_weight_sync: Optional[str] = None
        if net_settings is not None or rollouts is not None:
            self._push_net_settings(entries if net_settings is not None else None, self.net_settings_wide, rollouts)
        self.sync_weights()

    def _net_entries(self, net_settings, wide: bool) -> List[dict]:
        """``net_settings`` completed with the shared kwargs and checked: one entry per model, known keys; widths up to 256, or
        (``wide``) any width, with whole 32-tree teams per model where the models are searched as teams."""
        entries = _capi.net_search_entries(net_settings, self.n_models, self._shared)
        for m in self.models:
            if wide:
                norm = any(type(mod).__name__ == "LayerNorm" for mod in m.trunk)
                if self.n_models > 1 and self.trees_per_model % 32 and _capi.lockstep_shaped(m.state_dim, list(m.hidden_dimensions), norm):
                    raise ValueError(f"net_settings: models of this shape are searched as teams of 32 trees, so trees_per_model must be a multiple "
                                     f"of 32 (got {self.trees_per_model}) for every team to serve one model")
                continue
            width = max(m.hidden_dimensions)
            if (width + 63) // 64 * 64 >= 512:
                raise ValueError(f"net_settings: per-model search settings need a hidden width of at most 256 (padded to a multiple of 64); "
                                 f"this model's is {width}. Wider networks search with shared settings only, or with net_settings_wide=True")
        return entries

    def _net_budgets(self, net_rollouts, wide: bool) -> List[int]:
        """``net_rollouts`` checked: one int per model in 1 .. n_rollouts, and the width rules of ``net_settings``."""
        budgets = list(net_rollouts)
        if len(budgets) != self.n_models:
            raise ValueError(f"net_rollouts has {len(budgets)} entries for {self.n_models} models: one per model")
        for k, n in enumerate(budgets):
            if int(n) != n or not 1 <= int(n) <= self.n_rollouts:
                raise ValueError(f"net_rollouts[{k}] = {n!r}: a model's own budget is an int in 1 .. n_rollouts ({self.n_rollouts}, the "
                                 "engine's capacity)")
        self._net_entries([{}] * self.n_models, wide)
        return [int(n) for n in budgets]

    def _push_net_settings(self, entries: Optional[List[dict]], wide: bool, rollouts: Optional[List[int]] = None) -> None:
        """The table as it now stands goes to the engine: ``entries`` (None: every model's five settings are the shared ones) and
        ``rollouts`` (None: no budgets -- the calls are those of a table without them)."""
        table = entries if entries is not None else [dict(self._shared) for _ in range(self.n_models)]
        kw = {} if rollouts is None else {"n_sims": rollouts}
        if wide:
            self.engine.set_net_search(table, wide=True, **kw)
        else:
            self.engine.set_net_search(table, **kw)
        self.net_settings, self.net_settings_wide, self.net_rollouts = entries, wide, rollouts

    def set_net_settings(self, net_settings: Optional[Sequence[dict]], wide: Optional[bool] = None) -> None:
        """Change the per-model search settings between searches (same rules as the constructor's ``net_settings``); None returns to
        the shared settings (per-model budgets, ``net_rollouts``, stay).  ``wide``: as the constructor's ``net_settings_wide`` (None:
        what the constructor was given).  Every model's widening must fit the engine as it was created (azg_max_children): EngineError
        otherwise."""
        if net_settings is None:
            if self.net_rollouts is not None:
                self._push_net_settings(None, self.net_settings_wide, self.net_rollouts)
                return
            self.engine.set_net_search(None)
            self.net_settings = None
            return
        wide = self.net_settings_wide if wide is None else bool(wide)
        self._push_net_settings(self._net_entries(net_settings, wide), wide, self.net_rollouts)

    def set_net_rollouts(self, net_rollouts: Optional[Sequence[int]]) -> None:
        """Change the per-model simulation budgets between searches (same rules as the constructor's ``net_rollouts``); None: every
        model runs ``n_rollouts`` again (per-model settings, ``net_settings``, stay)."""
        if net_rollouts is None:
            if self.net_settings is not None:
                self._push_net_settings(self.net_settings, self.net_settings_wide)
            else:
                self.engine.set_net_search(None)
                self.net_rollouts = None
            return
        self._push_net_settings(self.net_settings, self.net_settings_wide, self._net_budgets(net_rollouts, self.net_settings_wide))

    def set_net_table(self, net_settings: Optional[Sequence[dict]], net_rollouts: Optional[Sequence[int]]) -> None:
        """``set_net_settings`` and ``set_net_rollouts`` in one: both setters' checks run first, then the table goes to the engine
        once, so a refusal -- a budget above ``n_rollouts``, a widening beyond azg_max_children -- leaves both as they were (an
        exploit/explore step changes settings and budgets together).  None for either: that part returns to the shared values."""
        if net_settings is None and net_rollouts is None:
            self.engine.set_net_search(None)
            self.net_settings, self.net_rollouts = None, None
            return
        wide = self.net_settings_wide
        entries = None if net_settings is None else self._net_entries(net_settings, wide)
        rollouts = None if net_rollouts is None else self._net_budgets(net_rollouts, wide)
        self._push_net_settings(entries, wide, rollouts)

    def sync_weights(self, force: bool = False) -> None:
        """Upload the weights of every model that changed since its last upload (net k = models[k]; after every optimiser step).
        ``last_weight_sync`` says how: "device" when every parameter lives on the engine's GPU (flattened there; K > 1: one gather
        launch for all nets), "host" (K > 1: one host upload per changed net), None when nothing changed."""
        if self._in_target:   # (the models are the live set's: inside ``target_weights()`` nothing of theirs is written)
            return
        versions = [_weights_version(m) for m in self.models]
        changed = [k for k in range(self.n_models) if force or versions[k] != self._versions[k]]
        self.last_weight_sync = None
        if not changed:
            return
        if self.n_models == 1:
            self.last_weight_sync = self.engine.set_policy(self.models[0])
        elif all(p.is_cuda and p.device.index == self.engine.cfg.device_id for m in self.models for p in m.parameters()):
            self.last_weight_sync = self.engine.set_population_policies(self.models)
        else:
            for k in changed:
                self.engine.set_net_policy(k, self.models[k])
            self.last_weight_sync = "host"
        self._versions = versions

    def upload_flat(self, desc, flat) -> None:
        """Upload every net from ``flat`` [n_models, P], the device tensor the models' parameters are views of
        (agent.population_trainer.bind_flat): one gather launch, no per-net flattening.  For parameters a HIP kernel wrote in place
        (PopulationTrainer): that does not bump torch's ``_version``, so ``sync_weights`` would not see it.  The models' current
        versions are recorded, so that the next plain ``sync_weights()`` uploads nothing."""
        import torch
        if tuple(flat.shape[:1]) != (self.n_models,) or flat.dim() != 2 or not flat.is_contiguous() or flat.dtype != torch.float32:
            raise ValueError("upload_flat: flat must be a contiguous float32 [n_models, P] tensor")
        if not flat.is_cuda or flat.device.index != self.engine.cfg.device_id:
            raise ValueError("upload_flat: flat must live on the engine's GPU")
        torch.cuda.current_stream(flat.device).synchronize()
        self._set_flat(desc, flat)
        self._versions = [_weights_version(m) for m in self.models]
        self.last_weight_sync = "device"

    def _set_flat(self, desc, flat) -> None:
        """One gather launch from ``flat`` [n_models, P] (checked, complete) into the weight set in use."""
        if self.n_models == 1:
            self.engine.set_weights_device(desc, flat.data_ptr(), flat.shape[1])
        else:
            self.engine.set_population_weights_device(desc, flat.data_ptr(), flat.shape[1], self.n_models)

    def upload_target_flat(self, desc, flat) -> None:
        """Upload every net of the engine's TARGET weight set (include/azgym_target.h) from ``flat`` [n_models, P] -- a
        ``PopulationTrainer``'s ``ema``, say -- with ``upload_flat``'s checks and its one gather launch; the live weights, which the
        games are played with, are not touched and are in use again when this returns.  ``target_weights()`` then runs anything with
        the target set.  A ``desc`` that differs from the live set's empties the live set (the sets share one descriptor)."""
        import torch
        if tuple(flat.shape[:1]) != (self.n_models,) or flat.dim() != 2 or not flat.is_contiguous() or flat.dtype != torch.float32:
            raise ValueError("upload_target_flat: flat must be a contiguous float32 [n_models, P] tensor")
        if not flat.is_cuda or flat.device.index != self.engine.cfg.device_id:
            raise ValueError("upload_target_flat: flat must live on the engine's GPU")
        torch.cuda.current_stream(flat.device).synchronize()
        self.engine.use_weights("target")
        try:
            self._set_flat(desc, flat)
        finally:
            self.engine.use_weights("live")

    @contextlib.contextmanager
    def target_weights(self):
        """Everything inside runs with the engine's TARGET weight set (``upload_target_flat`` first: ``RuntimeError`` otherwise);
        LIVE is in use again on exit, exceptions included.  Pending uploads of the models' own (live) weights are not applied
        inside -- ``sync_weights()`` does nothing there -- so apply them before."""
        if self._in_target:
            raise RuntimeError("target_weights: already inside target_weights()")
        if not self.engine.weights_info()["target_ready"]:
            raise RuntimeError("target_weights: the engine has no target weights: upload_target_flat(desc, flat) first (an upload of "
                               "another network descriptor empties them)")
        self.engine.use_weights("target")
        self._in_target = True
        try:
            yield self
        finally:
            self._in_target = False
            self.engine.use_weights("live")

    def search(self, root_states: np.ndarray, root_n_carry: Optional[np.ndarray] = None) -> None:
        """root_states [n_trees, S] (or [n_models, trees_per_model, S]); tree k*T + j belongs to models[k]."""
        self.sync_weights()
        self.engine.search(root_states, root_n_carry)
        if not self._cliff_warned and hasattr(self.engine, "search_info"):   # (the tests' CPU double of the engine has no kernel forms)
            info = self.engine.search_info()
            if info["kernel_form"] == "persistent" and info["tree_storage"] == "global" and info["lds_exit"] != "forced":
                self._cliff_warned = True
                warnings.warn(f"the trees of this search do not fit LDS residency ({info['lds_exit']}: {info['max_records']} records per tree, up to "
                              f"{info['max_children']} children per node): they are kept in global memory -- same results, slower tree walk "
                              "(last_search_info)", RuntimeWarning, stacklevel=2)

    @property
    def last_search_info(self) -> dict:
        """What the last search ran as (azg_search_info): ``kernel_form`` "persistent" / "per_layer" / "team", ``tree_storage`` "lds8" /
        "lds9" / "global" with ``lds_exit`` saying which residency limit pushed the trees out of LDS, ``spec``, the workgroup shape,
        ``team_fallbacks``, ``last_ms`` and the kernel's name."""
        return self.engine.search_info()

    def results(self):
        """return_results of every tree, rows in tree order k*T + j."""
        return self.engine.results()

    def root_children(self):
        return self.engine.root_children()

    def root_eval(self):
        """(value [n_trees], dist [n_trees, n_dist]) of the roots of the last search as their nets evaluated them, rows in tree order."""
        return self.engine.root_eval() if self.n_models == 1 else self.engine.population_root_eval()   # (one model: the plain entry point)

    def evaluate_observations(self, obs, shared: bool = False):
        """Value and policy heads of EVERY model on given observations, in one launch and with the search's own arithmetic:
        ``obs`` [n_models, n, obs_dim] (model k on ``obs[k]``), or with ``shared`` [n, obs_dim] (every model on the same rows).
        A numpy array takes the host form and returns numpy arrays; a torch tensor on the engine's GPU is read in place and torch
        tensors come back.  Returns (value [n_models, n], dist [n_models, n, n_dist], raw [n_models, n, 1 + n_dist])."""
        self.sync_weights()
        if hasattr(obs, "is_cuda"):
            if obs.is_cuda:
                return self.engine.population_mlp_eval_device(obs, shared=shared)
            obs = obs.detach().numpy()
        return self.engine.population_mlp_eval(obs, shared=shared)

    def close(self):
        self.engine.close()


class BatchedMCTS(PopulationMCTS):
    """B independent trees of one model searched in one launch: a population of one (``PopulationMCTS`` kwargs)."""

    def __init__(self, model, *, n_trees: int, **kwargs):
        super().__init__([model], trees_per_model=n_trees, **kwargs)

    @property
    def model(self):
        return self.models[0]

    @property
    def _version(self):
        """The model's weights version (_weights_version) at its last upload."""
        return self._versions[0]


class _Root:
    """What remains of the reference's root Node object on the host: the visit count a reused root carries."""

    def __init__(self, n: int, state):
        self.n = n
        self.state = state
        self.terminal = False
        self.parent_action = None


class MCTS:
    """Shared surface of mcts.py:23-307."""

    _mode = None

    def __init__(self, model, n_rollouts: int, c_uct: float, gamma: float, epsilon: float, device: str, V_target_policy: str,
                 root_state: np.ndarray, seed: int = 34, tree_id_base: int = 0):
        self.device = device
        self.tree_id_base = tree_id_base   # global id of the (first) tree: keys its RNG streams
        self.root_node = None
        self.root_state = root_state
        self.model = model
        self.n_rollouts = n_rollouts
        self.c_uct = c_uct
        self.gamma = gamma
        self.epsilon = epsilon
        self.V_target_policy = V_target_policy
        self.seed = seed
        self._batched: Optional[BatchedMCTS] = None
        self._key = None
        self._res = None
        self._children = None
        self._envs: List[Any] = []

    # ---- engine management
    def _engine_kwargs(self) -> dict:
        raise NotImplementedError

    def _ensure_engine(self, env_id: int, n_trees: int) -> BatchedMCTS:
        device_id = device_ordinal(self.device)
        key = (env_id, n_trees, self.n_rollouts, self.c_uct, self.gamma, self.epsilon, self.V_target_policy, id(self.model),
               device_id, self.tree_id_base, tuple(sorted(self._engine_kwargs().items())))
        if self._batched is None or key != self._key:
            if self._batched is not None:
                self._batched.close()
            self._batched = BatchedMCTS(self.model, env_id=env_id, mode=self._mode, n_trees=n_trees, n_rollouts=self.n_rollouts,
                                        c_uct=self.c_uct, gamma=self.gamma, epsilon=self.epsilon,
                                        V_target_policy=self.V_target_policy, seed=self.seed, tree_id_base=self.tree_id_base,
                                        device_id=device_id, **self._engine_kwargs())
            self._key = key
        return self._batched

    def _carry(self, n_trees: int) -> Optional[np.ndarray]:
        return None

    # ---- the reference's interface
    def search(self, Env) -> None:
        """Run n_rollouts traces from the state of ``Env`` (mcts.py:418-462 / 656-702).  ``Env`` is not mutated.
        A list/tuple of environments searches one tree per environment in the same launch."""
        envs: Sequence[Any] = list(Env) if isinstance(Env, (list, tuple)) else [Env]
        sigs = [env_signature(e) for e in envs]
        env_id = sigs[0][0]
        if any(s[0] != env_id for s in sigs):
            raise ValueError("all environments of one batched search must be of the same kind")
        roots = np.stack([s[1] for s in sigs])
        eng = self._ensure_engine(env_id, len(envs))
        eng.search(roots, self._carry(len(envs)))   # raises ValueError on a terminal root (mcts.py:382-383, 599-600)
        self._adopt(envs, eng.results(), eng.root_children())

    def _adopt(self, envs: Sequence[Any], res: dict, children) -> None:
        """Take the results of a search of ``envs`` (one tree each) as this object's last search: what search() does once the
        engine has run (AgentPopulation hands each agent its rows of a population search this way)."""
        self._envs = list(envs)
        self._res = res
        self._children = children
        carried = 0 if self.root_node is None else self.root_node.n
        self.root_node = _Root(carried + self.n_rollouts, self.root_state)

    def _row(self, i: int):
        raise NotImplementedError

    def return_results(self, final_selection: str):
        """(root state, actions, counts, Q, V_target) with the reference's shapes and dtypes (mcts.py:269-307).
        After a batched search, a list with one such tuple per environment."""
        assert self._res is not None, "search() has not been called"
        rows = [self._row(i) for i in range(len(self._envs))]
        return rows[0] if len(rows) == 1 else rows

    # ---- value targets kept for API parity (mcts.py:92-131); the engine computes them on the device
    @staticmethod
    def get_on_policy_value_target(Q: np.ndarray, counts: np.ndarray) -> np.ndarray:
        return np.sum((counts / np.sum(counts)) * Q)

    @staticmethod
    def get_off_policy_value_target(Q: np.ndarray) -> Any:
        return Q.max()


class MCTSDiscrete(MCTS):
    """mcts.py:310-526.  Tree "reuse" keeps only the root's visit count, exactly as in the reference."""

    _mode = _capi.MODE_DISCRETE

    def __init__(self, model, num_actions: int, n_rollouts: int, c_uct: float, gamma: float, epsilon: float, V_target_policy: str,
                 device: str, root_state: np.ndarray, seed: int = 34, tree_id_base: int = 0):
        super().__init__(model=model, n_rollouts=n_rollouts, c_uct=c_uct, gamma=gamma, epsilon=epsilon, device=device,
                         V_target_policy=V_target_policy, root_state=root_state, seed=seed, tree_id_base=tree_id_base)
        self.num_actions = num_actions

    def _engine_kwargs(self) -> dict:
        return dict(num_actions=self.num_actions)

    def _carry(self, n_trees: int):
        if self.root_node is None:
            return None
        return np.full((n_trees,), int(self.root_node.n), dtype=np.int32)

    def _row(self, i: int):
        r = self._res
        k = int(r["n_children"][i])
        state = self.root_state if (len(self._envs) == 1 and self.root_state is not None) else env_observation(
            *env_signature(self._envs[i]))
        return (state, np.arange(k), r["counts"][i, :k].astype(np.int64), r["Q"][i, :k].copy(), float(r["v_target"][i]))

    def forward(self, action: int, state: np.ndarray) -> None:
        """Move the root to the child reached by ``action`` (mcts.py:495-526)."""
        assert self._children is not None
        child_n, child_state = self._children
        if child_n[0, action] < 0:
            self.root_node = None
            self.root_state = state
        elif np.linalg.norm(env_observation(env_signature(self._envs[0])[0], child_state[0, action])
                            - np.asarray(state, dtype=np.float32)) > 0.01:
            print("Warning: this domain seems stochastic. Not re-using the subtree for next search. "
                  + "To deal with stochastic environments, implement progressive widening.")
            self.root_node = None
            self.root_state = state
        else:
            self.root_node = _Root(int(child_n[0, action]), state)
            self.root_state = state


class MCTSContinuous(MCTS):
    """mcts.py:529-741: progressive widening; a new root every search (no tree reuse).  Nodes of environments whose episodes end
    (MountainCarContinuous) are terminal as in mcts.py:619-623, 682: value 0, no evaluation, the trace stops there; a terminal root
    state raises ValueError (mcts.py:599-600)."""

    _mode = _capi.MODE_CONTINUOUS

    def __init__(self, model, n_rollouts: int, c_uct: float, c_pw: float, kappa: float, gamma: float, epsilon: float,
                 V_target_policy: str, device: str, root_state: np.ndarray, seed: int = 34, tree_id_base: int = 0):
        super().__init__(model=model, n_rollouts=n_rollouts, c_uct=c_uct, gamma=gamma, epsilon=epsilon, device=device,
                         V_target_policy=V_target_policy, root_state=root_state, seed=seed, tree_id_base=tree_id_base)
        self.c_pw = c_pw
        self.kappa = kappa

    def _engine_kwargs(self) -> dict:
        bound = getattr(self.model, "action_bound", None)
        if not bound:
            raise NotImplementedError("the engine samples squashed-Normal actions: the policy needs a finite action_bound")
        return dict(c_pw=self.c_pw, kappa=self.kappa, action_bound=float(bound))

    def search(self, Env) -> None:
        self.root_node = None   # initialize_search always builds a fresh root (mcts.py:589-600)
        super().search(Env)

    def _adopt(self, envs, res, children) -> None:
        self.root_node = None
        super()._adopt(envs, res, children)

    def _row(self, i: int):
        r = self._res
        k = int(r["n_children"][i])
        if len(self._envs) == 1 and self.root_state is not None:
            state = self.root_state
        else:
            env_id, st = env_signature(self._envs[i])
            if env_id == _capi.ENV_MOUNTAINCAR_CONT:
                state = np.array(st)                       # (position, velocity): the observation is the state
            else:
                th, thdot = st
                state = np.array([np.cos(th), np.sin(th), thdot])
        actions = r["actions"][i, :k].copy()
        if k == 1:
            actions = actions.reshape(())   # np.squeeze of a single action (mcts.py:307)
        return (state, actions, r["counts"][i, :k].astype(np.int64), r["Q"][i, :k].reshape(k, 1).copy(), np.float64(r["v_target"][i]))
