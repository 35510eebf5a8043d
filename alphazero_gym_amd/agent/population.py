"""K agents of one game searched together: ``AgentPopulation.act`` is one launch (and one set of ABI round trips) for all of them.

Each agent keeps its own network, optimiser, MCTS object (root node, carried visit count) and host-side random streams; what the
population shares is the engine (PopulationMCTS: one net per agent) and therefore its search index.  The search index of a
population step is the population's step counter, shared by every agent (steps in which an agent sits idle advance it too): a
standalone agent reproduces agent k exactly when it searches from the same weights under the same tree id
(``tree_id_base + k``) and the same search indices.
"""
import contextlib
import random
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .. import _capi
from ..search.mcts import PopulationMCTS, device_ordinal, env_signature
from .agents import ContinuousAgent, DiscreteAgent
from .buffers import ReplayBuffer


class AgentPopulation:
    """K ``DiscreteAgent``s or K ``ContinuousAgent``s of one game with the same MCTS settings (n_rollouts, c_uct, gamma, epsilon,
    V_target_policy, seed, and num_actions or c_pw / kappa) and the same network shape.  Agent k searches one tree, global tree id
    ``tree_id_base + k``.

    ``seeds``: agent k's ``np.random`` / ``random`` streams start as if seeded with seeds[k] (default: as the global streams stand
    now).  Every host-side draw of agent k -- its final action rule in ``act``, its buffer's reshuffle in ``train`` -- runs on its
    own streams, which are saved and restored around it (``rng(k)``), so that K agents' draws do not interleave.

    ``per_agent_search=True`` (opt-in): the agents may differ in ``mcts.c_uct`` / ``gamma`` / ``epsilon`` and (continuous) ``c_pw`` /
    ``kappa``; agent k's tree is searched with its own values, still in the one launch (PopulationMCTS ``net_settings``).  Everything
    else must still agree.  ``wide_search=True`` with it: agents whose networks are 512 or wider (PopulationMCTS
    ``net_settings_wide``).  ``per_agent_rollouts=True`` with it: the agents may also differ in ``mcts.n_rollouts``; the engine is
    created with the largest budget and agent k's tree runs its own (PopulationMCTS ``net_rollouts``), and the visit count a reused
    discrete root carries grows by agent k's own budget."""

    PER_AGENT = _capi.NET_SEARCH_KEYS

    def __init__(self, agents: Sequence[Any], seeds: Optional[Sequence[int]] = None, tree_id_base: int = 0,
                 per_agent_search: bool = False, wide_search: bool = False, per_agent_rollouts: bool = False):
        self.agents = list(agents)
        if not self.agents:
            raise ValueError("AgentPopulation needs at least one agent")
        if all(isinstance(a, DiscreteAgent) for a in self.agents):
            self.discrete = True
        elif all(isinstance(a, ContinuousAgent) for a in self.agents):
            self.discrete = False
        else:
            raise ValueError("AgentPopulation: all agents must be DiscreteAgents or all ContinuousAgents")
        self.per_agent_search = bool(per_agent_search)
        if wide_search and not self.per_agent_search:
            raise ValueError("AgentPopulation: wide_search=True goes with per_agent_search=True (it lets wide networks search with per-agent settings)")
        self.wide_search = bool(wide_search)
        if per_agent_rollouts and not self.per_agent_search:
            raise ValueError("AgentPopulation: per_agent_rollouts=True goes with per_agent_search=True (the budgets travel in the per-agent table)")
        self.per_agent_rollouts = bool(per_agent_rollouts)
        keys = {self._settings(a) for a in self.agents}
        if len(keys) != 1:
            if not self.per_agent_search:
                raise ValueError("AgentPopulation: every agent must have the same MCTS settings (per-agent search hyper-parameters are not "
                                 "supported)")
            if self.per_agent_rollouts:
                raise ValueError("AgentPopulation(per_agent_search=True, per_agent_rollouts=True): the agents may differ in n_rollouts, c_uct, "
                                 "gamma, epsilon, c_pw and kappa only; V_target_policy, seed, device and the other engine settings must agree")
            raise ValueError("AgentPopulation(per_agent_search=True): the agents may differ in c_uct, gamma, epsilon, c_pw and kappa only; "
                             "n_rollouts, V_target_policy, seed, device and the other engine settings must agree")
        self.tree_id_base = int(tree_id_base)
        K = len(self.agents)
        if seeds is not None and len(seeds) != K:
            raise ValueError("AgentPopulation: one seed per agent")
        self._np_states: List[Any] = []
        self._py_states: List[Any] = []
        for k in range(K):
            if seeds is None:
                self._np_states.append(np.random.get_state())
                self._py_states.append(random.getstate())
            else:
                self._np_states.append(np.random.RandomState(int(seeds[k])).get_state())
                self._py_states.append(random.Random(int(seeds[k])).getstate())
        self._pop: Optional[PopulationMCTS] = None
        self._env_id: Optional[int] = None

    def __len__(self) -> int:
        return len(self.agents)

    def _settings(self, agent) -> tuple:
        m = agent.mcts
        key = (type(m), m.n_rollouts, m.c_uct, m.gamma, m.epsilon, m.V_target_policy, m.seed, device_ordinal(m.device))
        if self.per_agent_search:   # (the five settings an agent may have its own of do not have to agree)
            key = (type(m), None if self.per_agent_rollouts else m.n_rollouts, m.V_target_policy, m.seed, device_ordinal(m.device))
        return key + tuple(sorted((k, v) for k, v in m._engine_kwargs().items() if not (self.per_agent_search and k in self.PER_AGENT)))

    def _net_settings(self) -> Optional[List[Dict[str, float]]]:
        """Each agent's own values of the per-agent search settings (None without ``per_agent_search``)."""
        if not self.per_agent_search:
            return None
        return [{k: float(getattr(a.mcts, k)) for k in self.PER_AGENT if hasattr(a.mcts, k)} for a in self.agents]

    def _net_rollouts(self) -> Optional[List[int]]:
        """Each agent's own simulation budget (None without ``per_agent_rollouts``)."""
        if not self.per_agent_rollouts:
            return None
        return [int(a.mcts.n_rollouts) for a in self.agents]

    @contextlib.contextmanager
    def rng(self, k: int):
        """Run a block on agent k's ``np.random`` / ``random`` streams (the global streams are restored afterwards)."""
        outer_np, outer_py = np.random.get_state(), random.getstate()
        np.random.set_state(self._np_states[k])
        random.setstate(self._py_states[k])
        try:
            yield
        finally:
            self._np_states[k] = np.random.get_state()
            self._py_states[k] = random.getstate()
            np.random.set_state(outer_np)
            random.setstate(outer_py)

    def _engine(self, env_id: int) -> PopulationMCTS:
        if self._pop is None or env_id != self._env_id:
            if self._pop is not None:
                self._pop.close()
            m = self.agents[0].mcts
            self._pop = PopulationMCTS([a.nn for a in self.agents], trees_per_model=1, env_id=env_id,
                                       mode=_capi.MODE_DISCRETE if self.discrete else _capi.MODE_CONTINUOUS,
                                       n_rollouts=max(self._net_rollouts()) if self.per_agent_rollouts else m.n_rollouts,
                                       c_uct=m.c_uct, gamma=m.gamma, epsilon=m.epsilon, V_target_policy=m.V_target_policy, seed=m.seed,
                                       tree_id_base=self.tree_id_base, device_id=device_ordinal(m.device), **m._engine_kwargs(),
                                       **({"net_settings": self._net_settings()} if self.per_agent_search else {}),
                                       **({"net_settings_wide": True} if self.wide_search else {}),
                                       **({"net_rollouts": self._net_rollouts()} if self.per_agent_rollouts else {}))
            self._env_id = env_id
        return self._pop

    @property
    def mcts(self) -> Optional[PopulationMCTS]:
        """The population's engine (None before the first ``act``)."""
        return self._pop

    def act(self, envs: Sequence[Any], deterministic: bool = False) -> List[Any]:
        """One search of every agent's environment in one launch, then each agent's own final action rule on its own streams.
        ``envs[k]`` is agent k's environment, or None when agent k sits this step out (its episode is over): its tree then searches
        a placeholder root whose results are dropped.  Returns, per agent, what ``agent.act(envs[k])`` returns (None for idle
        agents)."""
        K = len(self.agents)
        if len(envs) != K:
            raise ValueError("AgentPopulation.act: one environment (or None) per agent")
        sigs = [None if e is None else env_signature(e) for e in envs]
        live = [s for s in sigs if s is not None]
        if not live:
            raise ValueError("AgentPopulation.act: no agent has an environment")
        env_id = live[0][0]
        if any(s[0] != env_id for s in live):
            raise ValueError("all environments of a population must be of the same kind")
        S = live[0][1].size
        roots = np.zeros((K, S), np.float64)          # (idle agents: the all-zero state, a non-terminal root of every game)
        carry = np.zeros((K,), np.int32)
        for k, s in enumerate(sigs):
            if s is None:
                continue
            roots[k] = s[1]
            c = self.agents[k].mcts._carry(1)
            if c is not None:
                carry[k] = c[0]
        pop = self._engine(env_id)
        pop.search(roots, carry if self.discrete else None)   # one launch for all agents (ValueError on a terminal root)
        res = pop.results()
        child_n, child_state = pop.root_children()
        out: List[Any] = [None] * K
        for k, e in enumerate(envs):
            if e is None:
                continue
            agent = self.agents[k]
            agent.mcts._adopt([e], {key: v[k:k + 1] for key, v in res.items()}, (child_n[k:k + 1], child_state[k:k + 1]))
            with self.rng(k):
                out[k] = agent._final_action(deterministic) if self.discrete else agent._final_action()
        return out

    def train(self, k: int, buffer: ReplayBuffer) -> Dict[str, Any]:
        """Agent k's own training pass (its optimiser step) on its own random streams."""
        with self.rng(k):
            return self.agents[k].train(buffer)

    def close(self) -> None:
        if self._pop is not None:
            self._pop.close()
            self._pop = None

