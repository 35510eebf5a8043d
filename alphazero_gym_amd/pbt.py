"""Population-based training (Jaderberg et al. 2017) for a device population: the exploit/explore step that the per-net pieces were
built for -- ``PopulationTrainer(per_net=True)`` and ``reload_settings()``, ``PopulationMCTS`` ``net_settings`` / ``net_rollouts``,
per-net ``n_step`` / ``td_lambda`` / ``target_gamma``, and the fitness signals ``evaluate`` / ``evaluate_search`` /
``finished_returns``.

``select`` picks who copies whom (truncation selection), ``perturb`` moves one hyper-parameter, and ``PopulationBasedTraining.step``
does a whole step: the losers take the winners' parameters, optimiser state, learned temperature and settings
(``PopulationTrainer.copy_nets``, ``PopulationSelfPlay.copy_nets``), their inherited hyper-parameters are perturbed, and the result
is handed back to the engine (``upload_flat``).  A step moves at most K * P floats by row copies on tensors the trainer owns and
runs once per many training iterations: there is no kernel of its own.  Experience does not move: a replaced net keeps its games,
ring rows and counters (``PopulationSelfPlay.reanalyse`` refreshes those rows' targets with the new weights).

This module is pure numpy: importing it needs neither torch nor a GPU."""
import math
from typing import Any, Dict, List, Optional

import numpy as np

TRAINER_OPT_NAMES = ("lr", "weight_decay", "grad_clip")          # optimizer.param_groups[0] / agent.clip
TRAINER_LOSS_NAMES = ("tau", "policy_coeff", "value_coeff", "alpha")   # agent.loss
SEARCH_NAMES = ("c_uct", "gamma", "epsilon", "c_pw", "kappa")    # PopulationMCTS.net_settings
BUDGET_NAME = "n_rollouts"                                       # PopulationMCTS.net_rollouts
TARGET_NAMES = ("n_step", "td_lambda", "target_gamma")           # PopulationSelfPlay's per-net lists
NAMES = TRAINER_OPT_NAMES + TRAINER_LOSS_NAMES + SEARCH_NAMES + (BUDGET_NAME,) + TARGET_NAMES
INTEGER_NAMES = (BUDGET_NAME, "n_step")


def check_src(src, K: int) -> np.ndarray:
    """``src`` as int64 [K] after the checks every ``copy_nets`` makes: K integers in 0 .. K-1 with ``src[src[k]] == src[k]`` (a
    net that is copied from is not itself replaced, so the copies can be made in any order).  ``ValueError`` otherwise."""
    arr = np.asarray(src)
    if arr.ndim != 1 or arr.shape[0] != int(K):
        raise ValueError(f"copy_nets: src must have one entry per net ({int(K)}), got shape {tuple(arr.shape)}")
    if arr.dtype.kind not in "iu":
        if arr.dtype.kind != "f" or not np.all(np.isfinite(arr)) or np.any(arr != np.floor(arr)):
            raise ValueError("copy_nets: src must hold integers (net indices)")
    arr = arr.astype(np.int64)
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= int(K)):
        raise ValueError(f"copy_nets: src names nets outside 0 .. {int(K) - 1}: {arr.tolist()}")
    if np.any(arr[arr] != arr):
        bad = int(np.nonzero(arr[arr] != arr)[0][0])
        raise ValueError(f"copy_nets: net {bad} copies net {int(arr[bad])}, which is itself replaced (by net {int(arr[arr[bad]])}): "
                         "a source must stay (src[src[k]] == src[k])")
    return arr


def select(scores, fraction: float, rng: np.random.Generator) -> np.ndarray:
    """Truncation selection.  ``scores`` [K] float, higher is better.  Returns ``src`` int64 [K]: ``src[k] == k``, net k stays;
    ``src[k] == j``, net k becomes a copy of net j.

    ``n = floor(K * fraction)`` nets are replaced (0: the identity, no draw).  ``order = np.argsort(-scores, kind="stable")`` ranks
    the nets, ties to the lower index; the top set is ``order[:n]``, the bottom set ``order[K - n:]``.  For the bottom nets in
    ascending net index, ``src[k] = top[rng.integers(n)]``: one draw per replaced net and no other.  ``fraction`` lies in (0, 0.5],
    so the two sets are disjoint and ``src[src[k]] == src[k]``.  A non-finite score, a ``scores`` that is not one-dimensional or a
    ``fraction`` outside (0, 0.5] raise ``ValueError`` before anything is drawn."""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 1:
        raise ValueError(f"select: scores must be one-dimensional [K], got shape {tuple(scores.shape)}")
    if not np.all(np.isfinite(scores)):
        raise ValueError("select: every score must be finite")
    fraction = float(fraction)
    if not 0.0 < fraction <= 0.5:   # (NaN fails both)
        raise ValueError(f"select: fraction must lie in (0, 0.5], got {fraction}")
    K = scores.shape[0]
    src = np.arange(K, dtype=np.int64)
    n = int(math.floor(K * fraction))
    if n == 0:
        return src
    order = np.argsort(-scores, kind="stable")
    top, bottom = order[:n], order[K - n:]
    for k in sorted(int(b) for b in bottom):
        src[k] = top[int(rng.integers(n))]
    return src


def check_spec(name: str, spec) -> None:
    """A perturbation spec: ``factors`` non-empty, finite and positive, ``min <= max``, both finite.  ``ValueError`` otherwise."""
    try:
        factors = [float(f) for f in spec["factors"]]
        lo, hi = float(spec["min"]), float(spec["max"])
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"perturb: the spec of {name!r} needs 'factors' (a sequence of numbers), 'min' and 'max'") from None
    if not factors or not all(math.isfinite(f) and f > 0.0 for f in factors):
        raise ValueError(f"perturb: the factors of {name!r} must be non-empty, finite and positive, got {list(spec['factors'])}")
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"perturb: {name!r} needs finite min <= max, got min {spec['min']!r}, max {spec['max']!r}")


def perturb(value, spec: dict, rng: np.random.Generator):
    """``clip(value * spec["factors"][rng.integers(len(factors))], spec["min"], spec["max"])`` in Python float64: one draw per call.
    With ``spec.get("integer")`` the result is ``int(floor(x + 0.5))``, clipped again.  ``factors`` must be non-empty and positive
    and ``min <= max``: ``ValueError`` otherwise, before the draw."""
    check_spec("value", spec)
    factors = [float(f) for f in spec["factors"]]
    lo, hi = float(spec["min"]), float(spec["max"])
    x = float(value) * factors[int(rng.integers(len(factors)))]
    x = min(max(x, lo), hi)
    if spec.get("integer"):
        x = int(np.floor(x + 0.5))
        return int(min(max(x, int(math.ceil(lo))), int(math.floor(hi))))
    return x


def _identity(src: np.ndarray) -> bool:
    return bool(np.all(src == np.arange(src.shape[0])))


class PopulationBasedTraining:
    """The exploit/explore driver of a ``run.PopulationSelfPlay`` ``sp`` and the ``PopulationTrainer`` ``trainer`` of the same K agents.

    ``explore``: an ordered dict, hyper-parameter name -> spec (``perturb``: ``{"factors": [...], "min": a, "max": b}`` and, for
    ``n_rollouts`` and ``n_step``, ``"integer": True``).  The names, and where their values live:

    * trainer settings ``lr``, ``weight_decay`` (the agents' ``optimizer.param_groups[0]``), ``grad_clip`` (``agent.clip``) and the
      loss's ``tau``, ``policy_coeff``, ``value_coeff``, ``alpha`` (``agent.loss``; ``alpha`` is A0CLoss's constant, a tuned loss
      learns its own).  They need ``PopulationTrainer(per_net=True)``; the loss ones also ``losses="device"``.
    * search settings ``c_uct``, ``gamma``, ``epsilon``, ``c_pw``, ``kappa`` (``sp.mcts.net_settings``) and ``n_rollouts``
      (``sp.mcts.net_rollouts``).  They need an engine created with ``net_settings=`` / ``net_rollouts=``: the table exists and the
      kernel form was picked for it.  ``c_pw`` and ``kappa`` are a continuous game's.
    * target rules ``n_step``, ``td_lambda``, ``target_gamma``: ``sp``'s per-net lists.  They need the lambda rule in force with
      that setting given as a list.

    A name whose precondition is not met raises ``ValueError`` naming the constructor argument to pass; unknown names, an invalid
    spec and a K that differs between ``sp`` and ``trainer`` are refused too.  What the engine itself limits -- a widening beyond
    azg_max_children, a budget above the capacity -- is refused by the existing setters' checks when a step reaches it.

    ``step(scores)``, ``scores`` [K] with higher better, in this order:

    1. ``src = select(scores, fraction, rng)``.
    2. ``src`` the identity: the record says so, nothing is written and no further draw is made.
    3. Explore draws: for every replaced net in ascending index, for every name in ``explore``'s insertion order, one ``perturb``
       draw on the value the net inherits (net ``src[k]``'s; a ``target_gamma`` entry None counts as that net's search gamma).
    4. ``sp.copy_nets(src, explored=...)``: the engine's copied and explored search table, budgets and target rules, every check
       first and then one push each -- the only part that can refuse, so it goes first: a refusal leaves trainer, agents, engine
       and this object's generator as they were.
    5. ``trainer.copy_nets(src)``; the explored trainer settings are written into the agents; ``trainer.reload_settings()``.
    6. ``sp.upload_flat(trainer.desc, trainer.flat)``.

    The draw protocol: ONE ``np.random.Generator(np.random.PCG64(seed))`` (``self.rng``) is kept across steps; a step's draws are
    ``select``'s (one ``rng.integers(n)`` per replaced net, ascending net index), then the explore draws in the order of 3 (one
    ``rng.integers(len(factors))`` each).  Nothing else draws.

    Returns, and appends to ``self.history``, the record ``{"src": [K ints], "identity": bool, "replaced": [nets],
    "explored": {net: {name: {"old": inherited value, "new": value written}}}}``."""

    def __init__(self, sp, trainer, explore: Optional[Dict[str, dict]] = None, fraction: float = 0.25, seed: int = 0):
        self.sp, self.trainer = sp, trainer
        self.explore = dict(explore or {})
        self.fraction = float(fraction)
        if not 0.0 < self.fraction <= 0.5:
            raise ValueError(f"PopulationBasedTraining: fraction must lie in (0, 0.5], got {fraction}")
        self.K = int(sp.n_nets)
        if len(trainer) != self.K:
            raise ValueError(f"PopulationBasedTraining: the self-play engine has {self.K} nets, the trainer {len(trainer)}")
        for name, spec in self.explore.items():
            self._check_name(name, spec)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.history: List[dict] = []

    def _check_name(self, name: str, spec) -> None:
        who = "PopulationBasedTraining"
        if name not in NAMES:
            raise ValueError(f"{who}: {name!r} is not a hyper-parameter it can explore ({list(NAMES)})")
        check_spec(name, spec)
        if float(spec["min"]) < 0.0:
            raise ValueError(f"{who}: {name!r} is never negative: its spec needs min >= 0")
        if name in INTEGER_NAMES and not spec.get("integer"):
            raise ValueError(f'{who}: {name!r} is an integer: its spec needs "integer": True')
        sp, tr = self.sp, self.trainer
        if name in TRAINER_OPT_NAMES + TRAINER_LOSS_NAMES:
            if not tr.per_net:
                raise ValueError(f"{who}: exploring {name!r} needs a trainer whose nets have their own settings: build it with "
                                 'PopulationTrainer(..., optimizers="agents", per_net=True)')
            if name in TRAINER_LOSS_NAMES:
                if tr.losses != "device":
                    raise ValueError(f"{who}: exploring the loss setting {name!r} needs per-net loss settings: build the trainer with "
                                     'PopulationTrainer(..., losses="device")')
                loss = type(tr.loss).__name__
                if name == "alpha" and loss != "A0CLoss":
                    raise ValueError(f"{who}: 'alpha' is A0CLoss's constant temperature; the agents' loss is {loss}")
                if name == "tau" and loss == "AlphaZeroLoss":
                    raise ValueError(f"{who}: 'tau' is the A0C losses' setting; the agents' loss is {loss}")
        elif name in SEARCH_NAMES:
            if sp.mcts.net_settings is None:
                raise ValueError(f"{who}: exploring {name!r} needs the per-net search table: create the engine with "
                                 "PopulationSelfPlay(..., net_settings=[...]) (one dict per net; the shared values will do)")
            if name in ("c_pw", "kappa") and not sp.continuous:
                raise ValueError(f"{who}: {name!r} is progressive widening's, a continuous game's setting")
        elif name == BUDGET_NAME:
            if sp.mcts.net_rollouts is None:
                raise ValueError(f"{who}: exploring 'n_rollouts' needs per-net budgets: create the engine with "
                                 "PopulationSelfPlay(..., net_rollouts=[...]) (one int per net; n_rollouts stays the capacity)")
            if float(spec["min"]) < 1.0:
                raise ValueError(f"{who}: a net runs at least one simulation: the spec of 'n_rollouts' needs min >= 1")
        else:
            if not getattr(sp, "_lambda_rule", False) or not isinstance(getattr(sp, name), list):
                raise ValueError(f"{who}: exploring {name!r} needs per-net target rules: create the engine with "
                                 f"PopulationSelfPlay(..., {name}=[...]) (a list, one entry per net)")
            if name == "td_lambda" and float(spec["max"]) > 1.0:
                raise ValueError(f"{who}: td_lambda lies in [0, 1]: its spec needs max <= 1")

    # ---- where the values live
    def _read(self, name: str, k: int):
        """Net k's current value of ``name``."""
        sp = self.sp
        if name in TRAINER_OPT_NAMES + TRAINER_LOSS_NAMES:
            a = self.trainer.agents[k]
            if name == "grad_clip":
                return float(a.clip or 0.0)
            if name in TRAINER_OPT_NAMES:
                return float(a.optimizer.param_groups[0][name])
            return float(getattr(a.loss, name))
        if name in SEARCH_NAMES:
            return float(sp.mcts.net_settings[k][name])
        if name == BUDGET_NAME:
            return int(sp.mcts.net_rollouts[k])
        v = getattr(sp, name)[k]
        if v is None:   # (a target_gamma entry None: that net's search gamma)
            return float(sp.mcts.net_settings[k]["gamma"] if sp.mcts.net_settings is not None else sp.mcts._shared["gamma"])
        return v

    def _write_trainer(self, name: str, k: int, value) -> None:
        a = self.trainer.agents[k]
        if name == "grad_clip":
            a.clip = float(value)
        elif name in TRAINER_OPT_NAMES:
            a.optimizer.param_groups[0][name] = float(value)
        else:
            setattr(a.loss, name, float(value))

    def _scores(self, scores) -> np.ndarray:
        scores = np.asarray(scores, dtype=np.float64)
        if scores.ndim != 1 or scores.shape[0] != self.K:
            raise ValueError(f"PopulationBasedTraining.step: scores must be [K = {self.K}], got shape {tuple(scores.shape)}")
        return scores

    def step(self, scores) -> Dict[str, Any]:
        """One exploit/explore step on ``scores`` [K] (higher is better); see the class for the order, the draws and the record."""
        scores = self._scores(scores)
        before = self.rng.bit_generator.state
        src = select(scores, self.fraction, self.rng)
        record: Dict[str, Any] = {"src": [int(s) for s in src], "identity": _identity(src), "replaced": [], "explored": {}}
        if record["identity"]:
            self.history.append(record)
            return record
        replaced = [k for k in range(self.K) if int(src[k]) != k]
        record["replaced"] = replaced
        engine_side: Dict[int, Dict[str, Any]] = {}
        for k in replaced:
            mine = record["explored"].setdefault(k, {})
            for name, spec in self.explore.items():
                old = self._read(name, int(src[k]))
                new = perturb(old, spec, self.rng)
                mine[name] = {"old": old, "new": new}
                if name not in TRAINER_OPT_NAMES + TRAINER_LOSS_NAMES:
                    engine_side.setdefault(k, {})[name] = new
        try:
            self.sp.copy_nets(src, explored=engine_side)
        except Exception:
            self.rng.bit_generator.state = before   # (a refused step drew nothing)
            raise
        self.trainer.copy_nets(src)
        wrote = False
        for k in replaced:
            for name, change in record["explored"][k].items():
                if name in TRAINER_OPT_NAMES + TRAINER_LOSS_NAMES:
                    self._write_trainer(name, k, change["new"])
                    wrote = True
        if wrote:
            self.trainer.reload_settings()
        self.sp.upload_flat(self.trainer.desc, self.trainer.flat)
        self.history.append(record)
        return record
