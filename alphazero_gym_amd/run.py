"""Training drivers with the reference's loop shape, without hydra / wandb / gym.

``run_continuous_agent`` / ``run_discrete_agent`` mirror run_continuous.py:15-165 / run_discrete.py:16-146: one game, one
tree, ``act -> buffer.store -> Env.step -> reset_mcts | mcts_forward`` per step, ``agent.train(buffer)`` per episode.
``run_population`` is the same loop for K seeds at once: every step searches all K agents' trees in one launch
(AgentPopulation); training stays each agent's own optimiser step.  ``BatchedSelfPlay`` is the scaled-out form the engine is
built for: B games per GPU advance in lock step, one search launch per environment step, replay rows gathered across ranks,
weights broadcast after the optimiser step.  ``PopulationSelfPlay`` keeps the games, searches and replay rows of K policies on the
GPU, in one engine; ``DeviceSelfPlay`` is its one-policy form.

Default hyper-parameters are the reference's (config/*.yaml), except that the continuous policy uses
one squashed-Normal component (num_components: 1) instead of the 2-component GMM.
"""
import argparse
import contextlib
import copy
import functools
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import _capi, distributed as D
from .agent.agents import ContinuousAgent, DiscreteAgent
from .agent.buffers import DeviceReplay, ReplayBuffer
from .agent.population import AgentPopulation
from .envs import VecCartPole, VecMountainCarContinuous, VecPendulum, make_game
from .helpers import check_space, stable_normalizer
from .pbt import check_src
from .search.mcts import BatchedMCTS, PopulationMCTS

LOSS_TUNED = dict(_target_="alphazero_gym_amd.agent.losses.A0CLossTuned", action_dim=1, alpha_init=1.0, lr=0.001, tau=0.1,
                  policy_coeff=0.1, value_coeff=1.0, reduction="mean", grad_clip=0, device="cpu")
RMSPROP = dict(_target_="torch.optim.RMSprop", lr=0.001, alpha=0.9, eps=1e-10, weight_decay=0, momentum=0)
ADAM = dict(_target_="torch.optim.Adam", lr=0.001, betas=(0.9, 0.99), weight_decay=0, eps=1e-07, amsgrad=False)   # config/optimizer/Adam.yaml

CONTINUOUS_DEFAULTS = dict(
    game="Pendulum-v0", seed=34, num_train_episodes=45, max_episode_length=200, device="cpu",
    buffer=dict(max_size=3000, batch_size=32),
    policy=dict(_target_="alphazero_gym_amd.network.policies.make_policy", distribution="normal", num_components=1,
                hidden_dimensions=[128, 128, 128], nonlinearity="elu", layernorm=False, log_param_min=-5, log_param_max=2),
    mcts=dict(_target_="alphazero_gym_amd.search.mcts.MCTSContinuous", n_rollouts=25, c_pw=1, kappa=0.5, c_uct=0.05, gamma=1, epsilon=0,
              V_target_policy="off_policy", root_state=None),
    loss=LOSS_TUNED, optimizer=RMSPROP,
    agent=dict(final_selection="max_visit", epsilon=0, train_epochs=1, grad_clip=0),
)
DISCRETE_DEFAULTS = dict(
    game="CartPole-v0", seed=34, num_train_episodes=200, max_episode_length=200, device="cpu",
    buffer=dict(max_size=1000, batch_size=32),
    policy=dict(_target_="alphazero_gym_amd.network.policies.make_policy", distribution="discrete", hidden_dimensions=[128, 128],
                nonlinearity="relu", layernorm=False),
    mcts=dict(_target_="alphazero_gym_amd.search.mcts.MCTSDiscrete", n_rollouts=8, c_uct=1.5, gamma=1, epsilon=0.1,
              V_target_policy="off_policy", root_state=None),
    loss=LOSS_TUNED, optimizer=RMSPROP,
    agent=dict(final_selection="max_visits", temperature=1.0, train_epochs=1, grad_clip=0),
)


def _merge(base: dict, over: Optional[dict]) -> dict:
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _merge(out[k], v)
        else:
            out[k] = v
    return out


def run_continuous_agent(cfg: Optional[dict] = None, log: Optional[Callable[[Dict, int], None]] = None) -> List[float]:
    """run_continuous.py:15-165"""
    cfg = _merge(CONTINUOUS_DEFAULTS, cfg)
    Env = make_game(cfg["game"])
    np.random.seed(cfg["seed"])
    Env.seed(cfg["seed"])
    buffer = ReplayBuffer(**cfg["buffer"])
    state_dim, _ = check_space(Env.observation_space)
    action_dim, discrete = check_space(Env.action_space)
    assert not discrete, "Using continuous agent for a discrete action space!"
    policy = dict(cfg["policy"], representation_dim=state_dim[0], action_dim=action_dim[0], action_bound=float(Env.action_space.high[0]))
    agent = ContinuousAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=cfg["device"]), loss_cfg=cfg["loss"],
                            optimizer_cfg=cfg["optimizer"], device=cfg["device"], **cfg["agent"])
    returns = []
    for ep in range(cfg["num_train_episodes"]):
        state = Env.reset()
        R = 0.0
        agent.reset_mcts(root_state=state)
        for t in range(cfg["max_episode_length"]):
            action, s, actions, counts, Qs, V = agent.act(Env=Env)
            buffer.store((s, actions, counts, Qs, V))
            state, step_reward, terminal, _ = Env.step(action)
            R += float(np.asarray(step_reward).reshape(-1)[0])
            if terminal or t == cfg["max_episode_length"] - 1:
                break
            agent.reset_mcts(root_state=state)   # the continuous tree cannot be reused
        returns.append(R)
        info = agent.train(buffer)
        info["Episode reward"] = R
        if log:
            log(dict(info), ep)
    return returns


def run_discrete_agent(cfg: Optional[dict] = None, log: Optional[Callable[[Dict, int], None]] = None) -> List[float]:
    """run_discrete.py:16-146"""
    cfg = _merge(DISCRETE_DEFAULTS, cfg)
    Env = make_game(cfg["game"])
    np.random.seed(cfg["seed"])
    Env.seed(cfg["seed"])
    buffer = ReplayBuffer(**cfg["buffer"])
    state_dim, _ = check_space(Env.observation_space)
    action_dim, discrete = check_space(Env.action_space)
    assert discrete, "Can't use discrete agent for continuous action spaces!"
    policy = dict(cfg["policy"], representation_dim=state_dim[0], action_dim=1, num_actions=action_dim[0])
    agent = DiscreteAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=cfg["device"], num_actions=action_dim[0]),
                          loss_cfg=cfg["loss"], optimizer_cfg=cfg["optimizer"], device=cfg["device"], **cfg["agent"])
    returns = []
    for ep in range(cfg["num_train_episodes"]):
        state = Env.reset()
        R = 0.0
        agent.reset_mcts(root_state=state)
        for t in range(cfg["max_episode_length"]):
            action, s, actions, counts, Qs, V = agent.act(Env=Env, deterministic=False)
            buffer.store((s, actions, counts, Qs, V))
            new_state, step_reward, terminal, _ = Env.step(action)
            R += step_reward
            if terminal or t == cfg["max_episode_length"] - 1:
                break
            agent.mcts_forward(action, new_state)
        returns.append(R)
        info = agent.train(buffer)
        info["Episode reward"] = R
        if log:
            log(dict(info), ep)
    return returns


def make_agent(kind: str, cfg: dict, Env, tree_id_base: int = 0):
    """The agent run_continuous_agent / run_discrete_agent build for ``Env`` (cfg: merged defaults), searching tree ``tree_id_base``."""
    state_dim, _ = check_space(Env.observation_space)
    action_dim, discrete = check_space(Env.action_space)
    if kind == "continuous":
        assert not discrete, "Using continuous agent for a discrete action space!"
        policy = dict(cfg["policy"], representation_dim=state_dim[0], action_dim=action_dim[0], action_bound=float(Env.action_space.high[0]))
        return ContinuousAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=cfg["device"], tree_id_base=tree_id_base),
                               loss_cfg=cfg["loss"], optimizer_cfg=cfg["optimizer"], device=cfg["device"], **cfg["agent"])
    assert discrete, "Can't use discrete agent for continuous action spaces!"
    policy = dict(cfg["policy"], representation_dim=state_dim[0], action_dim=1, num_actions=action_dim[0])
    return DiscreteAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device=cfg["device"], num_actions=action_dim[0], tree_id_base=tree_id_base),
                         loss_cfg=cfg["loss"], optimizer_cfg=cfg["optimizer"], device=cfg["device"], **cfg["agent"])


def run_population(kind: str, seeds: List[int], cfg: Optional[dict] = None, log: Optional[Callable[[Dict, int, int], None]] = None,
                   agents: Optional[List] = None, sweep: Optional[Dict[str, List[float]]] = None,
                   rollouts: Optional[List[int]] = None) -> List[List[float]]:
    """run_continuous.py / run_discrete.py for K seeds at once (kind "continuous" / "discrete"; cfg as for run_*_agent, its
    ``seed`` replaced by ``seeds``).  Agent k plays its own game (env seeded with seeds[k]) with its own network, buffer,
    optimiser and np.random / random streams (seeded with seeds[k]); every environment step searches all agents' trees in ONE
    launch (AgentPopulation; agent k is tree k).  Agents whose episode has ended sit the remaining steps of that episode out.
    ``agents``: K agents built beforehand (default: built here from cfg).  Returns per seed its episode returns;
    ``log(info, episode, k)`` gets agent k's training losses and its "Episode reward".
    ``sweep``: search settings swept over the seeds, {"c_uct": [...], "gamma": [...], "epsilon": [...], "c_pw": [...], "kappa": [...]}
    (any subset; one list entry per seed): agent k is built with its own values in place of cfg["mcts"]'s, and all agents are still
    searched in one launch (AgentPopulation(per_agent_search=True)).
    ``rollouts``: simulation budgets swept over the seeds, one int >= 1 per seed: agent k is built with ``n_rollouts = rollouts[k]``
    and all agents are still searched in one launch, in an engine created for the largest budget
    (AgentPopulation(per_agent_rollouts=True)).  It combines with ``sweep``; ``sweep={"n_rollouts": ...}`` is not the way in."""
    cfg = _merge(CONTINUOUS_DEFAULTS if kind == "continuous" else DISCRETE_DEFAULTS, cfg)
    K = len(seeds)
    sweep = dict(sweep or {})
    for key, vals in sweep.items():
        if key not in _capi.NET_SEARCH_KEYS or (kind != "continuous" and key in ("c_pw", "kappa")):
            raise ValueError(f"sweep: {key!r} is not a per-agent search setting of a {kind} agent ({list(_capi.NET_SEARCH_KEYS)})")
        if len(vals) != K:
            raise ValueError(f"sweep[{key!r}] has {len(vals)} entries for {K} seeds: one per seed")
    if sweep and agents is not None:
        raise ValueError("sweep builds the agents itself: pass either sweep or agents")
    if rollouts is not None:
        if agents is not None:
            raise ValueError("rollouts builds the agents itself: pass either rollouts or agents")
        if len(rollouts) != K:
            raise ValueError(f"rollouts has {len(rollouts)} entries for {K} seeds: one per seed")
        if any(int(n) != n or int(n) < 1 for n in rollouts):
            raise ValueError(f"rollouts: every seed's budget is an int >= 1, got {list(rollouts)}")
    envs = []
    for s in seeds:
        Env = make_game(cfg["game"])
        Env.seed(s)
        envs.append(Env)
    if agents is None:
        own = [dict({key: vals[k] for key, vals in sweep.items()}, **({} if rollouts is None else {"n_rollouts": int(rollouts[k])}))
               for k in range(K)]
        agents = [make_agent(kind, dict(cfg, mcts=dict(cfg["mcts"], **own[k])), envs[k], tree_id_base=k) for k in range(K)]
    assert len(agents) == K
    buffers = [ReplayBuffer(**cfg["buffer"]) for _ in range(K)]
    if rollouts is not None:   # (opt-in: the agents' budgets differ; with or without swept settings)
        pop = AgentPopulation(agents, seeds=seeds, per_agent_search=True, per_agent_rollouts=True)
    else:
        pop = AgentPopulation(agents, seeds=seeds, per_agent_search=bool(sweep))
    returns: List[List[float]] = [[] for _ in range(K)]
    try:
        for ep in range(cfg["num_train_episodes"]):
            R = [0.0] * K
            for k in range(K):
                agents[k].reset_mcts(root_state=envs[k].reset())
            active = [True] * K
            for t in range(cfg["max_episode_length"]):
                outs = pop.act([envs[k] if active[k] else None for k in range(K)], deterministic=False)
                for k in range(K):
                    if not active[k]:
                        continue
                    action, s, actions, counts, Qs, V = outs[k]
                    buffers[k].store((s, actions, counts, Qs, V))
                    state, step_reward, terminal, _ = envs[k].step(action)
                    R[k] += float(np.asarray(step_reward).reshape(-1)[0])
                    if terminal or t == cfg["max_episode_length"] - 1:
                        active[k] = False
                    elif kind == "continuous":
                        agents[k].reset_mcts(root_state=state)   # the continuous tree cannot be reused
                    else:
                        agents[k].mcts_forward(action, state)
                if not any(active):
                    break
            for k in range(K):
                returns[k].append(R[k])
                info = pop.train(k, buffers[k])
                info["Episode reward"] = R[k]
                if log:
                    log(dict(info), ep, k)
    finally:
        pop.close()
    return returns


def _game_engine_kwargs(game: str, policy, c_pw: float = 1.0, kappa: float = 0.5) -> dict:
    """The engine's env_id, mode and head keywords for ``game`` (make_game's names; ValueError for others) and nets shaped like
    ``policy``: ``num_actions`` for a discrete game, ``c_pw`` / ``kappa`` / ``action_bound`` for a continuous one."""
    env_id = make_game(game).azg_env_id
    if env_id in (_capi.ENV_PENDULUM_V0, _capi.ENV_PENDULUM_V1, _capi.ENV_MOUNTAINCAR_CONT):
        return dict(env_id=env_id, mode=_capi.MODE_CONTINUOUS, c_pw=c_pw, kappa=kappa, action_bound=float(policy.action_bound))
    return dict(env_id=env_id, mode=_capi.MODE_DISCRETE, num_actions=policy.num_actions)


class BatchedSelfPlay:
    """B games per process in lock step: one search launch per environment step.
    Final action rules are the agents': continuous -> most visited root action (first index on ties),
    discrete -> sampled in proportion to (counts/max)^temperature."""

    def __init__(self, policy, *, game: str, n_games: int, n_rollouts: int, c_uct: float, gamma: float = 1.0, epsilon: float = 0.0,
                 c_pw: float = 1.0, kappa: float = 0.5, V_target_policy: str = "off_policy", max_episode_length: int = 200,
                 temperature: float = 1.0, seed: int = 34, rank: int = 0, world: int = 1, device_id: int = 0):
        self.policy = policy
        kw = _game_engine_kwargs(game, policy, c_pw, kappa)
        self.continuous = kw["mode"] == _capi.MODE_CONTINUOUS
        self.n = n_games
        self.max_len = max_episode_length
        self.temperature = temperature
        self.rng = np.random.RandomState(seed + 1000 * rank)
        env_id = kw["env_id"]
        if env_id == _capi.ENV_CARTPOLE:
            self.env = VecCartPole(n_games, seed=seed + rank)
        elif env_id == _capi.ENV_MOUNTAINCAR_CONT:
            self.env = VecMountainCarContinuous(n_games, seed=seed + rank)
        elif env_id in (_capi.ENV_PENDULUM_V0, _capi.ENV_PENDULUM_V1):
            self.env = VecPendulum(n_games, version=0 if env_id == _capi.ENV_PENDULUM_V0 else 1, seed=seed + rank)
        else:
            # (this host-stepped loop has vectorised numpy envs for CartPole, Pendulum and MountainCarContinuous only)
            raise NotImplementedError(f"BatchedSelfPlay steps CartPole, Pendulum and MountainCarContinuous on the host; {game} plays "
                                      "its own dynamics on the device: use DeviceSelfPlay")
        self.mcts = BatchedMCTS(policy, n_trees=n_games, n_rollouts=n_rollouts, c_uct=c_uct, gamma=gamma, epsilon=epsilon,
                                V_target_policy=V_target_policy, seed=seed, tree_id_base=rank * n_games, device_id=device_id, **kw)
        self.t = np.zeros(n_games, np.int64)
        self.ep_return = np.zeros(n_games)
        self.finished_returns: List[float] = []

    def step(self):
        """One environment step of all games; returns the replay rows (obs, actions, counts, Q, V_target) of this step."""
        obs = self.env.obs()
        self.mcts.search(self.env.state)
        r = self.mcts.results()
        K = int(r["n_children"].max())
        counts, Q, actions = r["counts"][:, :K], r["Q"][:, :K], r["actions"][:, :K]
        if self.continuous:
            act = actions[np.arange(self.n), counts.argmax(1)]
        else:
            pi = np.stack([stable_normalizer(c.astype(np.float64), self.temperature) for c in counts])
            act = np.array([self.rng.choice(K, p=p) for p in pi])
        reward, done = self.env.step(act)
        self.ep_return += reward
        self.t += 1
        over = done | (self.t >= self.max_len)
        if over.any():
            self.finished_returns += self.ep_return[over].tolist()
            self.ep_return[over] = 0.0
            self.t[over] = 0
            self.env.reset(over)
        return obs, actions, counts, Q, r["v_target"]

    def collect(self, n_steps: int) -> torch.Tensor:
        """Play n_steps and return this rank's replay rows packed as float32 [n_steps * B, row]."""
        rows = [D.pack_replay_rows(*self.step()) for _ in range(n_steps)]
        return torch.cat(rows, 0)


# evaluate()'s default game ids start here: far above any self-play game, and the same for every engine and rank, so that
# separately evaluated nets see the same start states too
EVAL_GAME_ID_BASE = 1 << 30
# reanalysis searches draw their RNG search indices from a counter of their own that starts here, far above any self-play step's
# (a step's search runs under the engine's running index, which counts up from 0): no reanalysis shares an index with a self-play
# search of the same tree
REANALYSE_INDEX_BASE = 1 << 31
# evaluate_search()'s searches run under RNG search indices from here on: above self-play's and apart from the reanalyses' first
# 2^30.  The default is the same at every call, so the same nets give the same number
EVAL_SEARCH_INDEX_BASE = 3 << 30


def _nets_keyword(method):
    """Gives a ``PopulationSelfPlay`` method the keyword ``nets``: "live" (the default) is the call as it always was; "target" runs it
    with the engine's TARGET weight set (``upload_target_flat``).  The method keeps its own parameters and signature; where it applies
    pending weight uploads it enters ``self._with_nets(...)``, which reads what was asked for here."""
    @functools.wraps(method)
    def call(self, *args, nets: str = "live", **kw):
        if nets not in ("live", "target"):
            raise ValueError(f"{method.__name__}: nets must be 'live' or 'target', not {nets!r}")
        self._nets = nets
        try:
            return method(self, *args, **kw)
        finally:
            self._nets = "live"
    return call


class PopulationSelfPlay:
    """Self-play with everything but the optimiser on the GPU (azg_selfplay_* in include/azgym.h), for K policies in ONE engine:
    games, final action rule, env step, episode resets and the replay ring live on the device; the host only downloads rows to
    train on.  ``policies[k]`` plays games k*T .. k*T+T-1 (T = ``games_per_net``) with global ids ``tree_id_base + k*T + j``, the
    games ``DeviceSelfPlay(policies[k], n_games=T, rank=k)`` plays, bit for bit, with one search launch and one self-play launch
    per step for the whole population.  The game, search and self-play settings are shared by every net, except that
    ``net_settings`` (``PopulationMCTS``: a list of K dicts) gives net k its own c_uct / gamma / epsilon / c_pw / kappa;
    ``net_settings_wide=True`` lets nets of padded hidden width >= 512 search with them; ``net_rollouts`` (K ints in 1 ..
    ``n_rollouts``) gives net k its own simulation budget, ``n_rollouts`` staying the engine's capacity.  The agents' final
    action rules run on the device too: ``final_selection`` "max_visit" / "max_value", discrete ``temperature`` and
    ``deterministic``, continuous ``agent_epsilon`` (agents.py:294-301, 524-535; include/azgym.h).  ``fifo=True`` turns the
    replay ring into the reference's overwrite-the-oldest buffer (buffers.py:75-82).  Weights are re-uploaded only when some
    policy changed (``PopulationMCTS.sync_weights``; ``last_weight_sync``: "device", "host" or None when nothing changed).
    ``reanalyse=True`` keeps every stored step's env states beside the ring, so that ``reanalyse()`` can search stored positions
    again with the current weights and overwrite their rows' targets.
    ``n_step`` (an integer >= 0; None: off, nothing is kept and the rows are today's) turns the rows' value targets into n-step
    returns: the engine keeps every stored step's reward, search value and end kind beside the ring, and ``play`` and
    ``reanalyse`` end with ``nstep_targets()``, which rewrites the ring's V_target column as the discounted rewards of the next
    ``n_step`` steps plus the discounted search value after them (include/azgym_nstep.h: a terminal step closes the window with
    no bootstrap; a time-limit step and the newest stored step bootstrap from their own search value).  ``target_gamma`` None:
    the search's gamma, net k's own where ``net_settings`` gives it one.
    ``td_lambda`` (a number in [0, 1]; None: off, every call made is the one above) turns them into lambda-returns
    (include/azgym_lambda.h): inside the window of ``n_step`` steps the returns of the windows 1 .. ``n_step`` are mixed with weights
    ``(1 - td_lambda) td_lambda**(m-1)``, the longest taking the rest -- 1 is the n-step return, 0 the 1-step return.  ``n_step``,
    ``td_lambda`` and ``target_gamma`` may each be a list with one entry per net (a ``target_gamma`` entry None: that net's search
    gamma): net k's rows then follow rule k, one launch for the population; a list for ``n_step`` or ``target_gamma`` with
    ``td_lambda`` None means lambda 1.  ``play`` and ``reanalyse`` then end with ``lambda_targets()`` instead.  ``prioritized``
    needs nothing else: the priority reads the V_target column, so it follows the lambda targets.
    ``prioritized`` (``{"alpha": 0.6, "eps": 1e-3}``; None: off, nothing is kept and behaviour is today's) keeps a priority per
    stored row beside the ring (include/azgym_priority.h): ``(|search value - V_target| + eps) ** alpha``, MuZero's, which needs
    ``n_step``.  ``sample_order(n)`` then draws training rows per net in proportion to it, on the device, in the form
    ``PopulationTrainer.train_epoch_ring`` takes as its order, and ``reanalyse(by="priority")`` draws the reanalysed position of
    every game the same way.  The draws are biased towards surprising rows; with ``"beta"`` in ``prioritized`` (optional; absent:
    no weight is ever computed) ``is_weights()`` computes the importance-sampling weight ``(q_min / q) ** beta`` of every stored
    row on the device, q_min the least priority of the row's net, and ``PopulationTrainer.train_epoch_ring(sp, order,
    weights="priority")`` multiplies it into the row's losses.  With ``"feedback"`` in ``prioritized`` (optional; absent: every
    call is what it was) the engine also keeps the trainer's value error of every stored row, ``|V - z|`` as
    ``PopulationTrainer.train_epoch_ring(sp, order, errors=True)`` writes it from its loss launch, and ``priorities()`` takes a
    row's d from it; a row not trained on since it was stored takes the largest trained error of its net (``"max"``; 1 while the
    net has none), ``|search value - V_target|`` (``"value_gap"``) or a constant d >= 0 (a number).  ``errors()`` downloads the
    kept errors, ``set_errors(array)`` uploads them (-1: not trained on)."""

    def __init__(self, policies, *, game: str, games_per_net: int, n_rollouts: int, c_uct: float, gamma: float = 1.0, epsilon: float = 0.0,
                 c_pw: float = 1.0, kappa: float = 0.5, V_target_policy: str = "off_policy", max_episode_length: int = 200,
                 deterministic: bool = False, capacity_steps: int = 64, seed: int = 34, tree_id_base: int = 0, device_id: int = 0,
                 final_selection: str = "max_visit", temperature: float = 1.0, agent_epsilon: float = 0.0, fifo: bool = False,
                 net_settings: Optional[List[dict]] = None, net_settings_wide: Optional[bool] = None,
                 net_rollouts: Optional[List[int]] = None, reanalyse: bool = False, n_step=None,
                 target_gamma=None, prioritized: Optional[dict] = None, td_lambda=None):
        policies = list(policies)
        if not policies or games_per_net < 1:
            raise ValueError(f"{type(self).__name__} needs at least one policy and games_per_net >= 1")
        n_step, td_lambda, target_gamma, self._lambda_rule = self._return_rule(len(policies), n_step, td_lambda, target_gamma)
        if prioritized is not None:
            if set(prioritized) - {"alpha", "eps", "beta", "feedback"}:
                raise ValueError(f"{type(self).__name__}: prioritized takes alpha, eps and beta, and feedback, not "
                                 f"{sorted(set(prioritized) - {'alpha', 'eps', 'beta', 'feedback'})}")
            if prioritized.get("feedback") is not None:
                _capi.unseen_mode(prioritized["feedback"])   # (ValueError: neither "max", "value_gap" nor a number >= 0)
            if prioritized.get("beta") is not None:
                if "alpha" not in prioritized:
                    raise ValueError(f"{type(self).__name__}: prioritized takes alpha and eps, and beta only beside alpha (the weights "
                                     "correct a draw by priority)")
                if not (float(prioritized["beta"]) >= 0.0 and np.isfinite(float(prioritized["beta"]))):
                    raise ValueError(f"{type(self).__name__}: prioritized beta must be finite and >= 0")
            if n_step is None:
                raise ValueError(f"{type(self).__name__}: prioritized needs n_step (the priority is |search value - n-step target|, and "
                                 "both are kept only then)")
        kw = _game_engine_kwargs(game, policies[0], c_pw, kappa)
        if net_settings is not None:   # (opt-in: net k searches with its own c_uct / gamma / epsilon / c_pw / kappa, PopulationMCTS)
            kw["net_settings"] = net_settings
        if net_settings_wide is not None:   # (opt-in: the table may be searched by nets of width >= 512)
            kw["net_settings_wide"] = net_settings_wide
        if net_rollouts is not None:   # (opt-in: net k runs its own number of simulations per search, PopulationMCTS)
            kw["net_rollouts"] = net_rollouts
        self.continuous = kw["mode"] == _capi.MODE_CONTINUOUS
        self.mcts = self._search(policies, games_per_net, n_rollouts=n_rollouts, c_uct=c_uct, gamma=gamma, epsilon=epsilon,
                                 V_target_policy=V_target_policy, seed=seed, tree_id_base=tree_id_base, device_id=device_id, **kw)
        self.engine, self.policies = self.mcts.engine, self.mcts.models
        self.n_nets, self.games_per_net, self.n_games = self.mcts.n_models, self.mcts.trees_per_model, self.mcts.n_trees
        self.capacity = capacity_steps
        self.fifo = fifo
        self.max_episode_length, self.tree_id_base = max_episode_length, tree_id_base
        self._replay = None
        # (one net: the plain engine's entry point, which the tests' CPU oracle also has)
        begin = self.engine.selfplay_begin if self.n_nets == 1 else self.engine.population_selfplay_begin
        begin(max_episode_length, deterministic, capacity_steps, final_selection=final_selection, temperature=temperature,
              agent_epsilon=agent_epsilon, fifo=fifo)
        self.reanalysing = bool(reanalyse)
        self._reanalyse_index = REANALYSE_INDEX_BASE
        self._reanalyse_rng = np.random.default_rng(seed)
        if self.reanalysing:
            self.engine.selfplay_keep_states(True)
        if n_step is not None and not isinstance(n_step, list) and n_step < 0:
            raise ValueError(f"{type(self).__name__}: n_step must be >= 0 or None")
        self.n_step, self.td_lambda, self.target_gamma = n_step, td_lambda, target_gamma
        if self.n_step is not None:
            self.engine.selfplay_keep_transitions(True)
        self.prioritized = None if prioritized is None else dict(alpha=float(prioritized.get("alpha", 0.6)),
                                                                 eps=float(prioritized.get("eps", 1e-3)))
        if self.prioritized is not None and prioritized.get("beta") is not None:
            self.prioritized["beta"] = float(prioritized["beta"])
        # the row draws and the slot draws take their sample indices from a counter each, both from 0: the streams differ
        self._sample_index = 0
        self._slot_sample_index = 0
        if self.prioritized is not None:
            self.engine.selfplay_keep_priorities(True)
            if prioritized.get("feedback") is not None:
                self.prioritized["feedback"] = prioritized["feedback"]
                self.engine.selfplay_keep_errors(True)

    @classmethod
    def _return_rule(cls, K: int, n_step, td_lambda, target_gamma):
        """The value-target settings as they are kept: (n_step, td_lambda, target_gamma, lambda rule in force).  A scalar stays a
        scalar (an int / a float; None stays None), a sequence becomes a list with one entry per net.  The lambda rule is in force
        when ``td_lambda`` is given or any setting is a list; ``td_lambda`` None is then lambda 1.  Raises ValueError for what no
        engine call could accept."""
        who = cls.__name__

        def listed(name, x, conv):
            if x is None or np.ndim(x) == 0:
                return x if x is None else conv(x)
            x = [conv(v) for v in x]
            if len(x) != K:
                raise ValueError(f"{who}: {name} has {len(x)} entries for {K} nets: a scalar or one per net")
            return x

        n_step = listed("n_step", n_step, int)
        td_lambda = listed("td_lambda", td_lambda, float)
        target_gamma = listed("target_gamma", target_gamma, lambda g: None if g is None else float(g))
        in_force = td_lambda is not None or isinstance(n_step, list) or isinstance(target_gamma, list)
        if in_force and n_step is None:
            raise ValueError(f"{who}: td_lambda (and per-net target settings) need n_step: the window the returns are mixed in")
        for lam in td_lambda if isinstance(td_lambda, list) else [] if td_lambda is None else [td_lambda]:
            if not 0.0 <= lam <= 1.0:   # (NaN fails both)
                raise ValueError(f"{who}: td_lambda must be in [0, 1], got {lam}")
        if isinstance(n_step, list) and min(n_step) < 0:
            raise ValueError(f"{who}: every n_step entry must be >= 0, got {n_step}")
        return n_step, td_lambda, target_gamma, in_force

    @staticmethod
    def _search(policies, games_per_net: int, **kw) -> PopulationMCTS:
        return PopulationMCTS(policies, trees_per_model=games_per_net, **kw)

    @property
    def last_weight_sync(self) -> Optional[str]:
        return self.mcts.last_weight_sync

    def sync_weights(self, force: bool = False) -> None:
        self.mcts.sync_weights(force)

    def upload_flat(self, desc, flat) -> None:
        """``PopulationMCTS.upload_flat``: the hand-off of parameters trained in place by ``PopulationTrainer``."""
        self.mcts.upload_flat(desc, flat)

    def upload_target_flat(self, desc, flat) -> None:
        """``PopulationMCTS.upload_target_flat``: the engine's TARGET weight set from a ``[K, P]`` tensor such as
        ``PopulationTrainer.ema``; the games go on with the live weights.  ``reanalyse``, ``refresh_values``, ``evaluate`` and ``evaluate_search``
        take ``nets="target"`` to run with it."""
        self.mcts.upload_target_flat(desc, flat)

    _nets = "live"   # what the call in progress was asked to run with (_nets_keyword)

    def _with_nets(self, who: str):
        """The context the network launches of a ``_nets_keyword`` method run under, pending live uploads applied first: nothing for
        "live" (the path as it always was), ``mcts.target_weights()`` for "target"."""
        self.sync_weights()
        if self._nets == "live":
            return contextlib.nullcontext()
        if not self.engine.weights_info()["target_ready"]:
            raise RuntimeError(f"{type(self).__name__}.{who}(nets='target'): no target weights yet: upload_target_flat(desc, flat) first")
        return self.mcts.target_weights()

    def copy_nets(self, src, reset_errors: bool = True, explored: Optional[Dict[int, dict]] = None) -> None:
        """The engine side of population-based training's exploit step (``alphazero_gym_amd.pbt``): net k's settings become those of
        net ``src[k]`` -- its entry in ``mcts.net_settings``, in ``mcts.net_rollouts`` and in the per-net ``n_step``, ``td_lambda``
        and ``target_gamma`` lists, each where that table or list exists.  Net k keeps its own games, carried subtrees, ring rows,
        kept states and transitions, priorities and counters: weights and hyper-parameters move, experience does not
        (``reanalyse()`` refreshes those rows' targets with the new weights).  The weights themselves arrive through
        ``upload_flat``.  ``src``: K ints in range with ``src[src[k]] == src[k]`` (``pbt.check_src``).

        ``reset_errors``: with ``prioritized={"feedback": ...}`` the kept trainer errors of the replaced nets' rows are set to -1
        ("not trained on"): they were another net's errors.
        ``explored`` ({net: {name: value}}, names among the search settings, ``n_rollouts`` and the target rules): values written
        over net k's copied ones, the explore half of the same step (``pbt.PopulationBasedTraining``).
        Every check -- this method's, ``PopulationMCTS.set_net_table``'s and the target rule's -- runs before the first write, and
        the search table is pushed once: a refusal leaves the engine and this object as they were."""
        src = check_src(src, self.n_nets)
        explored = {int(k): dict(v) for k, v in (explored or {}).items()}
        replaced = [k for k in range(self.n_nets) if int(src[k]) != k]
        if not replaced and not explored:
            return
        who = f"{type(self).__name__}.copy_nets"
        m = self.mcts
        settings = None if m.net_settings is None else [dict(m.net_settings[int(s)]) for s in src]
        rollouts = None if m.net_rollouts is None else [int(m.net_rollouts[int(s)]) for s in src]
        rule = {name: [getattr(self, name)[int(s)] for s in src] if isinstance(getattr(self, name), list) else getattr(self, name)
                for name in ("n_step", "td_lambda", "target_gamma")}
        for k, values in explored.items():
            if not 0 <= k < self.n_nets:
                raise ValueError(f"{who}: explored names net {k} of {self.n_nets}")
            for name, value in values.items():
                if name in _capi.NET_SEARCH_KEYS and settings is not None:
                    settings[k][name] = float(value)
                elif name == "n_rollouts" and rollouts is not None:
                    rollouts[k] = value
                elif name in rule and isinstance(rule[name], list):
                    rule[name][k] = value
                else:
                    raise ValueError(f"{who}: explored[{k}][{name!r}] has no per-net table or list in this engine to be written to")
        self._return_rule(self.n_nets, rule["n_step"], rule["td_lambda"], rule["target_gamma"])   # (its refusals, before any write)
        if settings is not None or rollouts is not None:
            m.set_net_table(settings, rollouts)
        self.n_step, self.td_lambda, self.target_gamma, _ = self._return_rule(self.n_nets, rule["n_step"], rule["td_lambda"],
                                                                              rule["target_gamma"])
        if reset_errors and replaced and self.prioritized is not None and "feedback" in self.prioritized \
                and self.engine.selfplay_ring()[0]:
            errors = self.errors().reshape(-1, self.n_games).copy()
            T = self.games_per_net
            for k in replaced:
                errors[:, k * T:(k + 1) * T] = -1.0
            self.set_errors(errors.reshape(-1))

    def play(self, n_steps: int) -> None:
        """n_steps self-play steps of every game of every net (asynchronous: launches only); rows accumulate in the device ring."""
        assert self.fifo or n_steps <= self.capacity
        self.sync_weights()
        for _ in range(n_steps):
            self.engine.selfplay_step()
        self._value_targets()

    def _value_targets(self) -> None:
        """What ``play`` and ``reanalyse`` end with: the value targets asked for at creation, if any."""
        if self.n_step is None:
            return
        if self._lambda_rule:
            self.lambda_targets()
        else:
            self.nstep_targets()

    def nstep_targets(self, n_step: Optional[int] = None, gamma: Optional[float] = None) -> None:
        """Rewrite the V_target column of every stored row as its n-step return (``Engine.selfplay_nstep_targets``; asynchronous:
        one launch).  ``n_step`` / ``gamma`` None: the ones given at creation (``target_gamma`` None: the search's gamma).
        Idempotent: ``play`` and ``reanalyse`` already end with it."""
        if self.n_step is None:
            raise RuntimeError(f"{type(self).__name__}.nstep_targets needs the stored steps' rewards and ends: create it with n_step=...")
        n_step = self.n_step if n_step is None else int(n_step)
        gamma = self.target_gamma if gamma is None else float(gamma)
        if isinstance(n_step, list) or isinstance(gamma, list):
            raise ValueError(f"{type(self).__name__}.nstep_targets takes one n_step and one gamma: per-net settings go through lambda_targets()")
        self.engine.selfplay_nstep_targets(n_step, gamma)

    def lambda_targets(self, n_step=None, td_lambda=None, gamma=None) -> None:
        """Rewrite the V_target column of every stored row as its lambda-return (``Engine.selfplay_lambda_targets``; asynchronous:
        one small copy and one launch).  Each argument is a scalar or a list with one entry per net; None: the one given at
        creation (``td_lambda`` None there: 1, the n-step return; ``target_gamma`` None: the search's gamma).  Idempotent: created
        with ``td_lambda`` or a list, ``play`` and ``reanalyse`` already end with it."""
        if self.n_step is None:
            raise RuntimeError(f"{type(self).__name__}.lambda_targets needs the stored steps' rewards and ends: create it with n_step=...")
        n_step, td_lambda, gamma, _ = self._return_rule(self.n_nets, self.n_step if n_step is None else n_step,
                                                        self.td_lambda if td_lambda is None else td_lambda,
                                                        self.target_gamma if gamma is None else gamma)
        self.engine.selfplay_lambda_targets(n_step, 1.0 if td_lambda is None else td_lambda, gamma)

    def priorities(self, given=None) -> None:
        """Compute the priority of every stored row (``Engine.selfplay_priorities`` with the ``alpha`` and ``eps`` given at
        creation; asynchronous: one launch).  ``given`` None: from |kept search value - V_target|; else from ``given``, a float32
        array with one entry >= 0 per stored row ordered like the ring ([size_steps, n_games]): a training loop's own TD errors.
        Created with ``"feedback"`` and ``given`` None: from the kept errors of the trainer (``Engine.selfplay_priorities_trained``)."""
        if self.prioritized is None:
            raise RuntimeError(f"{type(self).__name__}.priorities needs a priority per stored row: create it with prioritized={{...}}")
        if given is None and "feedback" in self.prioritized:
            self.engine.selfplay_priorities_trained(self.prioritized["alpha"], self.prioritized["eps"], self.prioritized["feedback"])
            return
        self.engine.selfplay_priorities(self.prioritized["alpha"], self.prioritized["eps"], given)

    def _feedback_refusal(self, what: str) -> None:
        if self.prioritized is None or "feedback" not in self.prioritized:
            raise RuntimeError(f'{type(self).__name__}.{what} needs an error per stored row: create it with prioritized={{..., "feedback": ...}}')

    def errors(self) -> np.ndarray:
        """The kept value errors of the stored rows, float32 [size_steps * n_games] ordered like the ring; -1: not trained on since
        the row was stored (``Engine.selfplay_error_values``; synchronises)."""
        self._feedback_refusal("errors")
        return self.engine.selfplay_error_values()

    def set_errors(self, errors) -> None:
        """Upload one error per stored row, ordered like the ring; every entry -1 (not trained on), NaN or >= 0
        (``Engine.selfplay_set_error_values``): a caller's own errors, a restored checkpoint."""
        self._feedback_refusal("set_errors")
        self.engine.selfplay_set_error_values(errors)

    def sample_order(self, n_order: int, given=None) -> np.ndarray:
        """``n_order`` training rows per net drawn on the device in proportion to the rows' priorities, with replacement: int32
        [K, n_order], what ``PopulationTrainer.train_epoch_ring(sp, order)`` takes.  The priorities are recomputed first
        (``priorities(given)``); every call takes the next index of a counter that starts at 0.  The draw is biased towards large
        priorities; ``is_weights()`` after it computes the weights that correct the loss."""
        self.priorities(given)
        order = self.engine.selfplay_sample_rows(int(n_order), self._sample_index)
        self._sample_index += 1
        return order

    def is_weights(self, beta: Optional[float] = None) -> None:
        """Compute the importance-sampling weight of every stored row from the priorities that stand
        (``Engine.selfplay_is_weights``; asynchronous: three launches): ``(q_min / q) ** beta`` with q_min the least priority of the
        row's net.  ``beta`` None: the one given at creation.  Call it after ``sample_order`` (which recomputes the priorities);
        ``PopulationTrainer.train_epoch_ring(sp, order, weights="priority")`` then reads the weights where they lie."""
        if self.prioritized is None:
            raise RuntimeError(f"{type(self).__name__}.is_weights needs a priority per stored row: create it with prioritized={{...}}")
        if beta is None:
            beta = self.prioritized.get("beta")
        if beta is None:
            raise ValueError(f'{type(self).__name__}.is_weights needs a beta: pass one, or create it with prioritized={{..., "beta": b}}')
        if not (float(beta) >= 0.0 and np.isfinite(float(beta))):
            raise ValueError(f"{type(self).__name__}.is_weights: beta must be finite and >= 0")
        self.engine.selfplay_is_weights(float(beta))

    @_nets_keyword
    def reanalyse(self, slots=None, n: int = 1, rng: Optional[np.random.Generator] = None, by: str = "uniform") -> list:
        """MuZero's Reanalyse on the device ring: search stored positions again with the CURRENT weights (pending uploads are
        applied first, as ``play`` does) and overwrite their rows' actions | counts | Q | V_target; observations, the live games
        and the ring's books stay as they are (asynchronous: launches only).  ``slots`` None: ``n`` stored slots (at most the
        ring's size) chosen uniformly without replacement by ``rng`` (default: this object's generator, seeded from the engine
        seed); a list of slots: each is reanalysed for every game; one ``[n_games]`` integer array: a single search in which game
        t re-searches its position in slot ``slots[t]``.  Every search takes the next index of a counter that starts at
        ``REANALYSE_INDEX_BASE``.  Returns the slots used (the per-game array: a one-element list holding it).
        ``by="priority"`` (with ``prioritized`` and ``slots`` None): one search in which game t re-searches the slot drawn for it
        on the device in proportion to the priorities of its column (recomputed first); the draws take the next index of a second
        counter that starts at 0.  ``by="uniform"`` is the rest of this description.
        ``nets="target"``: the searches run with the engine's TARGET weight set (``upload_target_flat``; MuZero's target network)
        instead of the live weights, which are in use again when the call returns; "live" is the call as it always was."""
        if by not in ("uniform", "priority"):
            raise ValueError(f"reanalyse: by must be 'uniform' or 'priority', not {by!r}")
        if not self.reanalysing:
            raise RuntimeError(f"{type(self).__name__}.reanalyse needs the stored positions' env states: create it with reanalyse=True")
        with self._with_nets("reanalyse"):
            used = self._reanalyse_searches(slots, n, rng, by)
        self._value_targets()   # (the reanalysed rows hold plain search values again: back to the returns, from the fresh values)
        return used

    @_nets_keyword
    def refresh_values(self, slots=None) -> list:
        """Refresh the bootstrap values of stored steps from the value head (``Engine.selfplay_refresh_values``,
        include/azgym_refresh.h): the kept value of every row of the ring slots ``slots`` (an iterable of ints; None: every stored
        slot) becomes net k's value of the row's stored observation -- one forward pass per row where ``reanalyse`` runs a whole
        search, one launch for the population (asynchronous; pending uploads are applied first, as ``play`` does) -- and the value
        targets asked for at creation are computed again from the fresh values.  The rows' policy targets, the live games and the
        ring's books stay as they are.  A window that bootstraps from its own row (the newest stored step, a time-limit step,
        ``n_step=0``) then has the net's own value as its target.  Returns the slots used.
        ``nets="target"``: the values come from the engine's TARGET weight set (``upload_target_flat``; MuZero Reanalyse's value
        targets), and the live weights are in use again when the call returns; "live" runs the live weights."""
        if self.n_step is None:
            raise RuntimeError(f"{type(self).__name__}.refresh_values needs the stored steps' kept values: create it with n_step=...")
        used = list(range(self.engine.selfplay_ring()[0])) if slots is None else [int(s) for s in slots]
        with self._with_nets("refresh_values"):
            self.engine.selfplay_refresh_values(None if slots is None else used)
        self._value_targets()
        return used

    def _reanalyse_searches(self, slots, n: int, rng, by: str) -> list:
        """``reanalyse``'s choice of slots and its searches, with the weight set in use; the slots used."""
        if by == "priority":
            if slots is not None:
                raise ValueError("reanalyse: by='priority' draws the slots itself")
            self.priorities()
            used = [self.engine.selfplay_sample_slots(self._slot_sample_index)] if self.engine.selfplay_ring()[0] else []
            self._slot_sample_index += 1
        elif slots is None:
            size = self.engine.selfplay_ring()[0]
            gen = self._reanalyse_rng if rng is None else rng
            used = [int(s) for s in gen.choice(size, size=min(int(n), size), replace=False)] if size else []
        elif isinstance(slots, np.ndarray) and slots.ndim == 1 and slots.shape[0] == self.n_games:
            used = [np.ascontiguousarray(slots, dtype=np.int32)]
        else:
            used = [int(s) for s in slots]
        for s in used:
            self.engine.selfplay_reanalyse(s, search_index=self._reanalyse_index)
            self._reanalyse_index += 1
        return used

    def play_device(self, n_steps: int):
        """``play`` for a consumer that reads the ring where it lies (``PopulationTrainer.train_epoch_ring``): returns the ring's
        (size_steps, insert_step) after the n_steps; nothing is copied and nothing cleared (``engine.selfplay_clear()`` is the
        caller's, once it is done with the rows)."""
        self.play(n_steps)
        size, insert, _ = self.engine.selfplay_ring()
        return size, insert

    def _split(self, rows, n_steps: int) -> List[torch.Tensor]:
        """[n_steps * n_games, row] in step-major order -> copies of net k's [n_steps * T, row] (the order of its DeviceSelfPlay)."""
        blocks = rows.reshape(n_steps, self.n_nets, self.games_per_net, rows.shape[-1])
        return [blocks[:, k].reshape(n_steps * self.games_per_net, -1).clone() for k in range(self.n_nets)]

    def collect(self, n_steps: int) -> List[torch.Tensor]:
        """Play n_steps (<= capacity) and return every net's replay rows since the last clear as host float32 tensors
        [steps * T, row] (net k's games in DeviceSelfPlay.collect's order); the ring is cleared."""
        assert n_steps <= self.capacity
        self.play(n_steps)
        rows = torch.from_numpy(self.engine.selfplay_rows(clear=True))
        return self._split(rows, rows.shape[0] // self.n_games)

    def collect_device(self, n_steps: int, replay: Optional[DeviceReplay] = None) -> List[torch.Tensor]:
        """Play n_steps and return every net's NEW rows as device tensors [n_steps * T, row] (copies in HBM, read through
        ``replay``, default: a view of this engine's ring): the ring is cleared, unless it runs in FIFO mode, where it keeps
        accumulating."""
        assert n_steps <= self.capacity, "the ring keeps its newest capacity_steps steps: older ones would already be overwritten"
        if replay is None:
            if self._replay is None:
                self._replay = DeviceReplay(self.engine, 1)
            replay = self._replay
        if not self.fifo:
            self.play(n_steps)
            rows = replay.rows()
            out = self._split(rows, rows.shape[0] // self.n_games)
            self.engine.selfplay_clear()
            return out
        before = self.engine.selfplay_ring()
        self.play(n_steps)
        size, insert, _ = self.engine.selfplay_ring()
        ring = replay.rows().reshape(size, self.n_games, -1)
        # the n_steps newest slots, oldest first: while filling they are the tail; once full they end just before insert_index
        if before[0] + n_steps <= self.capacity:
            new = ring[before[0]:before[0] + n_steps]
        else:
            idx = [(insert - n_steps + i) % size for i in range(n_steps)]
            new = ring[torch.as_tensor(idx, device=ring.device)]
        return self._split(new, n_steps)

    def finished_returns(self):
        """(fsum [K] float64, fcnt [K] int64): the returns and the number of the episodes each net's games finished so far, summed
        over the net's games in tree order."""
        fsum, fcnt, _ = self.engine.selfplay_stats()
        fsum = fsum.reshape(self.n_nets, self.games_per_net)
        fcnt = fcnt.reshape(self.n_nets, self.games_per_net).astype(np.int64)
        s, c = np.zeros(self.n_nets), np.zeros(self.n_nets, np.int64)
        for j in range(self.games_per_net):
            s += fsum[:, j]
            c += fcnt[:, j]
        return s, c

    @_nets_keyword
    def evaluate(self, episodes_per_net: int, rule: str = "mode", max_episode_length: Optional[int] = None, episode: int = 0,
                 game_id_base: Optional[int] = None) -> Dict[str, np.ndarray]:
        """How good each net is by itself: ``episodes_per_net`` whole episodes per net played by the raw policy, no search, on the
        device in one call (azg_policy_rollout_ex: every width the engine accepts).  Game j of EVERY net starts from the same state (that of global game ``game_id_base + j``,
        episode ``episode``), so the nets' returns can be ranked; another ``episode`` draws fresh start states.  ``rule``:
        "mode" (arg-max logit / the squashed mean) or "sample" (the policy's own distribution, the engine's Philox streams).
        ``max_episode_length`` None: the self-play's own limit; ``game_id_base`` None: ``EVAL_GAME_ID_BASE``, or the first id
        above this engine's self-play games where those reach it.  Pending weight uploads are applied first, as ``play`` does;
        self-play, searches and their results are left untouched.  Returns [n_nets, episodes_per_net] arrays "returns",
        "lengths", "terminated", "first_value" (the value head at the start state) and "mean_return" [n_nets].
        ``nets="target"``: the engine's TARGET weight set (``upload_target_flat``) plays instead of the live weights."""
        if rule not in _capi.ROLLOUT_RULE:
            raise ValueError(f"evaluate: rule must be one of {sorted(_capi.ROLLOUT_RULE)}, not {rule!r}")
        if int(episodes_per_net) < 1:
            raise ValueError("evaluate: episodes_per_net must be >= 1")
        if max_episode_length is None:
            max_episode_length = self.max_episode_length
        if int(max_episode_length) < 1:
            raise ValueError("evaluate: max_episode_length must be >= 1")
        if game_id_base is None:
            game_id_base = max(EVAL_GAME_ID_BASE, self.tree_id_base + self.n_games)
        with self._with_nets("evaluate"):
            out = self.engine.policy_rollout(int(episodes_per_net), int(max_episode_length), rule=rule, game_id_base=int(game_id_base),
                                             episode=int(episode))
        out["mean_return"] = out["returns"].mean(axis=1)
        return out

    @_nets_keyword
    def evaluate_search(self, episodes_per_game: int = 1, final_selection: str = "max_visit", deterministic: bool = True,
                        temperature: float = 1.0, agent_epsilon: float = 0.0, max_episode_length: Optional[int] = None, episode: int = 0,
                        game_id_base: Optional[int] = None, index_base: int = EVAL_SEARCH_INDEX_BASE,
                        poll_steps: int = 8) -> Dict[str, np.ndarray]:
        """How good each net is when it acts with its search: every game of the engine plays ``episodes_per_game`` whole episodes
        under MCTS on the device in one call (azg_search_rollout), with the engine's own search -- per-net settings and budgets
        included -- and the final-action rule given here (``evaluate``'s counterpart for ``Agent.act``; the defaults are the greedy
        rule).  Game j of EVERY net starts its i-th episode from the state of global game ``game_id_base + j``, episode
        ``episode + i``: ``evaluate``'s start states, so the nets can be ranked and compared with their raw policies.  Step s
        searches under RNG search index ``index_base + s``: the same nets give the same number at every call.
        ``max_episode_length`` None: the self-play's own limit; ``game_id_base`` None: as ``evaluate``.  Pending weight uploads are
        applied first, as ``play`` does; the self-play's games, ring and search index are left untouched.  Returns
        [n_nets, games_per_net, episodes_per_game] arrays "returns", "lengths", "terminated", plus "mean_return" [n_nets] and
        "steps" (the searches run).  ``nets="target"``: the engine's TARGET weight set (``upload_target_flat``) searches and acts
        instead of the live weights."""
        if final_selection not in _capi.FINAL_SELECTION:
            raise ValueError(f"evaluate_search: final_selection must be one of {sorted(_capi.FINAL_SELECTION)}, not {final_selection!r}")
        if int(episodes_per_game) < 1:
            raise ValueError("evaluate_search: episodes_per_game must be >= 1")
        if max_episode_length is None:
            max_episode_length = self.max_episode_length
        if int(max_episode_length) < 1:
            raise ValueError("evaluate_search: max_episode_length must be >= 1")
        if int(poll_steps) < 1:
            raise ValueError("evaluate_search: poll_steps must be >= 1")
        if not float(temperature) > 0.0:
            raise ValueError("evaluate_search: temperature must be > 0")
        if not 0.0 <= float(agent_epsilon) <= 1.0:
            raise ValueError("evaluate_search: agent_epsilon must be in [0, 1]")
        if not 0 <= int(index_base) < (1 << 32) or not 0 <= int(episode) < (1 << 32):
            raise ValueError("evaluate_search: index_base and episode must fit 32 bits")
        if game_id_base is None:
            game_id_base = max(EVAL_GAME_ID_BASE, self.tree_id_base + self.n_games)
        with self._with_nets("evaluate_search"):
            out = self.engine.search_rollout(int(episodes_per_game), int(max_episode_length), final_selection=final_selection,
                                             deterministic=bool(deterministic), temperature=float(temperature),
                                             agent_epsilon=float(agent_epsilon), game_id_base=int(game_id_base), episode=int(episode),
                                             index_base=int(index_base), poll_steps=int(poll_steps))
        shape = (self.n_nets, self.games_per_net, int(episodes_per_game))
        res = {k: out[k].reshape(shape) for k in ("returns", "lengths", "terminated")}
        res["mean_return"] = res["returns"].reshape(self.n_nets, -1).mean(axis=1)
        res["steps"] = out["steps"]
        return res

    def close(self) -> None:
        self.engine.close()


class DeviceSelfPlay(PopulationSelfPlay):
    """``PopulationSelfPlay`` of one policy: B games (``n_games``) with global ids ``rank * B + j``; rows come back as one tensor."""

    def __init__(self, policy, *, n_games: int, rank: int = 0, **kwargs):
        super().__init__([policy], games_per_net=n_games, tree_id_base=rank * n_games, **kwargs)

    @staticmethod
    def _search(policies, games_per_net: int, **kw) -> BatchedMCTS:
        return BatchedMCTS(policies[0], n_trees=games_per_net, **kw)   # (.mcts stays the single-net search: .model, ._version)

    def collect(self, n_steps: int) -> torch.Tensor:
        """Play n_steps (<= capacity) and return this rank's replay rows as a host float32 tensor [n_steps * B, row]."""
        return super().collect(n_steps)[0]

    def replay(self, batch_size: int, device=None) -> DeviceReplay:
        """The device ring as a replay buffer with the reference's sampling rules; minibatches are device tensors."""
        return DeviceReplay(self.engine, batch_size, device=device)

    def collect_device(self, n_steps: int, replay: DeviceReplay) -> torch.Tensor:
        """Play n_steps and return this rank's NEW rows as a device tensor [n_steps * B, row] (see PopulationSelfPlay.collect_device)."""
        return super().collect_device(n_steps, replay)[0]

    def mean_finished_return(self) -> float:
        fsum, fcnt, _ = self.engine.selfplay_stats()
        return float(fsum.sum() / max(int(fcnt.sum()), 1))


def train_on_rows(agent, rows: torch.Tensor, state_dim: int, K: int, batch_size: int = 32, shuffle_seed: int = 0) -> Dict[str, float]:
    """One epoch of minibatch updates (agent.update) over replay rows gathered from all ranks; the last batch absorbs the
    remainder like ReplayBuffer.__next__."""
    on_device = rows.is_cuda
    if on_device:   # minibatches are gathered on the GPU, nothing goes through the host
        s, a, c, q, v = (rows[:, :state_dim], rows[:, state_dim:state_dim + K], rows[:, state_dim + K:state_dim + 2 * K],
                         rows[:, state_dim + 2 * K:state_dim + 3 * K], rows[:, -1])
    else:
        s, a, c, q, v = D.unpack_replay_rows(rows, state_dim, K)
    n = s.shape[0]
    order = np.random.RandomState(shuffle_seed).permutation(n)
    sums: Dict[str, float] = {}
    i = 0
    while i < n:
        j = n if i + 2 * batch_size > n else i + batch_size
        idx = order[i:j]
        if on_device:
            ti = torch.from_numpy(idx).to(rows.device)
            info = agent.update((s[ti], a[ti], c[ti], q[ti], v[ti]))
        else:
            info = agent.update((s[idx].copy(), a[idx].copy(), c[idx].copy(), q[idx].copy(), v[idx].astype(np.float64)))
        for k_, val in info.items():
            sums[k_] = sums.get(k_, 0.0) + val
        i = j
    return sums


def main():
    ap = argparse.ArgumentParser(description="single-game drivers with the reference's loop shape")
    ap.add_argument("kind", choices=["continuous", "discrete"])
    ap.add_argument("--episodes", type=int, default=None)
    ap.add_argument("--n-rollouts", type=int, default=None)
    a = ap.parse_args()
    over = {}
    if a.episodes is not None:
        over["num_train_episodes"] = a.episodes
    if a.n_rollouts is not None:
        over["mcts"] = {"n_rollouts": a.n_rollouts}
    fn = run_continuous_agent if a.kind == "continuous" else run_discrete_agent
    rets = fn(over, log=lambda info, ep: print(ep, {k: round(float(v), 4) for k, v in info.items()}))
    print("episode returns:", np.round(rets, 2).tolist())


if __name__ == "__main__":
    main()
