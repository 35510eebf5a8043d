"""Population training: one minibatch optimiser step of K agents' nets in two HIP launches (include/azgym_train.h), with no Python
loop over the nets.

The K policies' parameters live in ONE float32 tensor ``flat[K, P]`` (``bind_flat``; state_dict order, the order of
``_capi.policy_tensors``) that the trainer's kernels update in place and the search engine's gather reads directly
(``PopulationMCTS.upload_flat``).  The boundary between HIP and PyTorch is the heads' raw output ``raw[K, B, 1 + n_dist]``:
trunk, heads, their backward pass and the optimiser step (RMSprop; with ``optimizers="agents"`` also Adam and gradient clipping) are kernels; the losses (``population_loss``: ``DiscreteAgent._loss`` /
``ContinuousAgent._loss`` restated once for a leading K axis, the tuned alpha's Adam step included) stay in PyTorch and give
``d_raw`` by autograd on those small tensors.  ``PopulationTrainer(..., losses="device")`` moves that boundary out of the step:
the same losses, their ``d_raw`` and the tuned alpha's Adam step are one more kernel between the two (``azg_trainer_step``: three
launches, one synchronisation, one copy of ``losses[K, 5]`` to the host).  ``train_epoch`` / ``train_epoch_ring`` take the loop
around that step to the device as well (``azg_trainer_epoch``): the minibatches are gathered by a kernel from the rows where they
lie, the self-play ring included, and a whole epoch costs one synchronisation.  The single-agent path (``Agent.update``) is untouched.

Every native call of a trainer goes through ``PopulationTrainer._call``: the form of the trainer's optimiser arguments, chosen once
in ``__init__``, names a row of ``_capi.TRAINER_CALLS``, which says what ``_capi.Trainer`` method serves each call and how that
method takes the optimiser; ``_call`` adds the loss settings and the learned temperature's state and keeps the step counts.
"""
import ctypes as C
import operator
from collections import namedtuple
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import _capi
from ..network.policies import DiagonalGMMPolicy, DiagonalNormalPolicy, DiscretePolicy
from ..pbt import check_src
from .losses import A0CLoss, A0CLossTuned, AlphaZeroLoss


def bind_flat(policies: Sequence[Any]) -> Tuple[Any, torch.Tensor]:
    """(desc, flat[K, P]): one float32 tensor on the policies' device holding every policy's parameters, row k = policy k in
    ``_capi.policy_tensors`` order (= ``_capi.policy_blob``'s blob).  Every parameter is re-pointed at a view of its row, values
    preserved, so ``state_dict()``, checkpoints and the agents' own torch optimisers keep working on the same storage."""
    policies = list(policies)
    if not policies:
        raise ValueError("bind_flat needs at least one policy")
    parts = [_capi.policy_tensors(p) for p in policies]
    desc, first = parts[0]
    shapes = [tuple(t.shape) for t in first]
    device = first[0].device
    for d_, tensors in parts:
        if [tuple(t.shape) for t in tensors] != shapes or bytes(d_) != bytes(desc):
            raise ValueError("bind_flat: every policy must have the same network shape, activation and head settings")
        if any(t.dtype != torch.float32 or t.device != device for t in tensors):
            raise ValueError("bind_flat: every parameter must be float32 on one device")
    flat = torch.empty((len(policies), sum(t.numel() for t in first)), dtype=torch.float32, device=device)
    with torch.no_grad():
        for k, (_, tensors) in enumerate(parts):
            off = 0
            for t in tensors:
                row = flat[k, off:off + t.numel()]
                row.copy_(t.detach().reshape(-1))
                t.data = row.view_as(t)
                off += t.numel()
    return desc, flat


def _log_probs_entropy(policy, head, actions):
    """``policy.get_train_data``'s log-probs and entropy from the distribution head's raw output ``head`` [N, n_dist] and
    ``actions`` [N, A], N = K * B rows of all nets: policies.py's own lines on a longer batch, so every element and every
    per-row sum is computed as the single agent computes it."""
    if isinstance(policy, DiscretePolicy):
        num_actions = actions.shape[1]
        pi_hat = torch.distributions.Categorical(logits=head.unsqueeze(dim=1).repeat((1, num_actions, 1)))
        return pi_hat.log_prob(actions), pi_hat.entropy()
    if isinstance(policy, DiagonalNormalPolicy):
        mu, log_std = head.chunk(2, dim=-1)
        log_std = torch.clamp(log_std, min=policy.log_param_min, max=policy.log_param_max)
        log_probs = policy._dist(mu, log_std.exp()).log_prob(actions)
        return log_probs, -log_probs.mean(dim=-1)
    if isinstance(policy, DiagonalGMMPolicy):
        C_ = policy.num_components
        dist_params = head[..., :C_ * 2 * policy.action_dim].reshape(head.shape[0], -1)
        log_coeff = head[..., -C_:]
        mu, log_std = dist_params.chunk(2, dim=-1)
        log_std = torch.clamp(log_std, min=policy.log_param_min, max=policy.log_param_max)
        A = actions.shape[-1]
        mu = mu.unsqueeze(dim=1).expand((-1, A, -1))
        sigma = log_std.exp().unsqueeze(dim=1).expand((-1, A, -1))
        log_mix = torch.log_softmax(log_coeff, dim=-1).unsqueeze(dim=1).expand((-1, A, -1))
        comp_lp = policy._component(mu, sigma).log_prob(actions.unsqueeze(-1))
        log_probs = torch.logsumexp(comp_lp + log_mix, dim=-1)
        return log_probs, -log_probs.mean(dim=-1)
    raise ValueError(f"population_loss: {type(policy).__name__} heads are not supported")


def _reduce(x, reduction):
    """Per-net reduction of [K, ...] over everything but K (losses.py: x.mean() / x.sum() of one net's tensor)."""
    dims = tuple(range(1, x.dim()))
    return x.mean(dim=dims) if reduction == "mean" else x.sum(dim=dims)


def population_terms(policy, loss, raw, actions, counts, values) -> Dict[str, torch.Tensor]:
    """The losses' summands before any reduction over the batch: "policy" [K, B] (cross-entropy per row, or the A0C policy term
    sum_i (log pi_i - tau log n_i).detach() * log pi_i per row), "value" [K, B, 1] (squared errors) and, for the A0C losses,
    "entropy" [K, B] or [K, B, A] and the "log_probs" [K, B, A] they come from.  Element for element what the single agent's code computes (the rows of all nets go through
    policies.py's and losses.py's own operations as one batch of K * B rows); only the reductions over B that follow see a
    tensor of another shape."""
    K, B = raw.shape[0], raw.shape[1]
    V_hat, head = raw[..., :1], raw[..., 1:]
    value = F.mse_loss(V_hat, values, reduction="none")
    if type(loss) is AlphaZeroLoss:
        if not isinstance(policy, DiscretePolicy):
            raise ValueError("population_loss: AlphaZeroLoss needs a discrete policy")
        if loss.reduction not in ("mean", "sum"):
            raise ValueError("population_loss: reduction must be 'mean' or 'sum'")
        logits = torch.distributions.Categorical(logits=head.reshape(K * B, -1)).logits
        target = F.softmax(counts.reshape(K * B, -1), dim=-1).argmax(dim=1)
        return {"policy": F.cross_entropy(logits, target, reduction="none").reshape(K, B), "value": value}
    if type(loss) not in (A0CLoss, A0CLossTuned):
        raise ValueError(f"population_loss: {type(loss).__name__} is not supported")
    A = actions.shape[-1]
    log_probs, entropy = _log_probs_entropy(policy, head.reshape(K * B, -1), actions.reshape(K * B, A))
    counts = counts.reshape(K * B, A)
    if isinstance(policy, DiscretePolicy):
        counts = counts + 1   # keeps log(counts) finite (agents.py:364)
    with torch.no_grad():
        log_diff = log_probs - loss.tau * torch.log(counts)
    per_row = torch.einsum("ni, ni -> n", log_diff, log_probs).reshape(K, B)
    return {"policy": per_row, "value": value, "entropy": entropy.reshape((K, B) + entropy.shape[1:]),
            "log_probs": log_probs.reshape(K, B, A)}


def _weighted_terms(terms: Dict[str, torch.Tensor], weights: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Every per-row summand times its row's weight ``weights`` [K, B] (an importance-sampling weight of prioritised replay): the
    value's [K, B, 1] and the discrete head's entropy [K, B, A] carry the row's weight in every element."""
    out = dict(terms)
    for key in ("policy", "value", "entropy"):
        if key in terms:
            t = terms[key]
            out[key] = t * weights.reshape(weights.shape + (1,) * (t.dim() - 2))
    return out


def population_loss(policy, loss, raw, actions, counts, values, log_alpha: Optional[torch.Tensor] = None,
                    alpha_optimizer: Optional[torch.optim.Optimizer] = None,
                    weights: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The K-axis form of ``DiscreteAgent._loss`` / ``ContinuousAgent._loss`` from the heads' raw outputs.

    ``policy`` / ``loss``: one of the K policies / loss objects (all nets share head kind, loss class and hyper-parameters);
    ``raw`` [K, B, 1 + n_dist] (value head first), ``actions`` / ``counts`` [K, B, A], ``values`` [K, B, 1].  With ``A0CLossTuned``,
    ``log_alpha`` [K] holds every net's own learned temperature and ``alpha_optimizer`` (one Adam over that tensor: Adam is
    element-wise, so element k is net k's own Adam) takes the step ``A0CLossTuned.forward`` takes.
    Returns {key: [K] tensor} with the keys of ``Agent.update``'s dictionary; ``out["loss"].sum().backward()`` gives every net's
    own ``d loss_k / d raw[k]`` (the nets are independent).  ``per_net`` turns it into K dictionaries of floats.

    ``weights`` [K, B] (None: unweighted, the code path as it always was): a weight per row multiplies every per-row summand of
    every loss before the reduction, which stays what it is (``mean`` divides by the number of rows); ``alpha_loss`` becomes
    mean(alpha * w * gap).  The truth of the weighted loss kernel (include/azgym_train_weighted.h); weights of 1 give the
    unweighted bits."""
    K = raw.shape[0]
    terms = population_terms(policy, loss, raw, actions, counts, values)
    if weights is not None:
        if tuple(weights.shape) != tuple(raw.shape[:2]):
            raise ValueError("population_loss: weights must be [K, B]")
        if type(loss) is A0CLossTuned:
            gap_w = weights.reshape(weights.shape + (1,) * (terms["entropy"].dim() - 2))
            unweighted_entropy = terms["entropy"]
        terms = _weighted_terms(terms, weights.to(raw.dtype))
    policy_loss = loss.policy_coeff * _reduce(terms["policy"], loss.reduction)
    value_loss = loss.value_coeff * _reduce(terms["value"], loss.reduction)
    if type(loss) is AlphaZeroLoss:
        return {"loss": policy_loss + value_loss, "policy_loss": policy_loss, "value_loss": value_loss}
    entropy = terms["entropy"]
    if type(loss) is A0CLoss:
        entropy_loss = loss.alpha * _reduce(entropy, loss.reduction)
        return {"loss": policy_loss + entropy_loss + value_loss, "policy_loss": policy_loss, "entropy_loss": entropy_loss,
                "value_loss": value_loss}
    if log_alpha is None:
        raise ValueError("population_loss: A0CLossTuned needs log_alpha [K]")
    alpha = log_alpha.exp()
    entropy_loss = alpha.detach() * _reduce(entropy, loss.reduction)
    total = policy_loss + entropy_loss + value_loss
    # A0CLossTuned._update_alpha for every net at once
    if weights is None:
        gap = (entropy - loss.target_entropy).detach()
    else:
        gap = (gap_w.to(raw.dtype) * (unweighted_entropy - loss.target_entropy)).detach()
    alpha_loss = (alpha.reshape((K,) + (1,) * (gap.dim() - 1)) * gap).mean(dim=tuple(range(1, gap.dim())))
    if alpha_optimizer is not None:
        log_alpha.grad = None
        alpha_loss.sum().backward()
        if loss.clip:   # clip_grad_norm_ of a one-element parameter, element by element
            g = log_alpha.grad
            g.mul_(torch.clamp(loss.clip / (g.abs() + 1e-6), max=1.0))
        alpha_optimizer.step()
    return {"loss": total, "policy_loss": policy_loss, "entropy_loss": entropy_loss, "value_loss": value_loss,
            "alpha_loss": alpha_loss.detach()}


def per_net(losses: Dict[str, torch.Tensor]) -> List[Dict[str, float]]:
    """{key: [K]} -> K dictionaries of floats (one device-to-host copy)."""
    keys = list(losses)
    table = torch.stack([losses[k].detach().to(torch.float32) for k in keys]).cpu().tolist()
    return [{k: table[i][n] for i, k in enumerate(keys)} for n in range(len(table[0]))]


def _loss_settings(loss) -> tuple:
    if type(loss) is AlphaZeroLoss:
        return (AlphaZeroLoss, loss.policy_coeff, loss.value_coeff, loss.reduction)
    if type(loss) is A0CLoss:
        return (A0CLoss, loss.tau, loss.policy_coeff, float(loss.alpha), loss.value_coeff, loss.reduction)
    if type(loss) is A0CLossTuned:
        g = loss.optimizer.param_groups[0]
        return (A0CLossTuned, loss.tau, loss.policy_coeff, loss.value_coeff, loss.reduction, loss.target_entropy, loss.clip,
                type(loss.optimizer), g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g.get("amsgrad", False))
    raise ValueError(f"PopulationTrainer: loss {type(loss).__name__} is not supported (AlphaZeroLoss, A0CLoss, A0CLossTuned)")


def _loss_shared(loss) -> tuple:
    """What ``per_net=True`` still asks every agent's loss to share: the class, the reduction and (tuned) the alpha optimiser's kind.
    Everything else in ``_loss_settings`` is a number that azg_loss_cfg carries per net."""
    _loss_settings(loss)   # (its refusal of other loss classes)
    if type(loss) is A0CLossTuned:
        return (A0CLossTuned, loss.reduction, type(loss.optimizer), loss.optimizer.param_groups[0].get("amsgrad", False))
    return (type(loss), loss.reduction)


def _rmsprop_settings(opt) -> tuple:
    if type(opt) is not torch.optim.RMSprop:
        raise ValueError(f"PopulationTrainer: the nets' optimiser must be torch.optim.RMSprop, not {type(opt).__name__}")
    if len(opt.param_groups) != 1:
        raise ValueError("PopulationTrainer: one RMSprop parameter group per agent")
    g = opt.param_groups[0]
    if g["momentum"] != 0 or g["centered"] or g.get("maximize", False):
        raise ValueError("PopulationTrainer: RMSprop with momentum, centered or maximize is not supported")
    return (g["lr"], g["alpha"], g["eps"], g["weight_decay"])


def _optimizer_settings(opt) -> tuple:
    """(class, settings) of an agent's optimiser as ``optimizers="agents"`` takes it: plain RMSprop, or Adam without amsgrad."""
    if type(opt) not in (torch.optim.RMSprop, torch.optim.Adam):
        raise ValueError(f"PopulationTrainer: the nets' optimiser must be torch.optim.RMSprop or torch.optim.Adam, not {type(opt).__name__}")
    if len(opt.param_groups) != 1:
        raise ValueError("PopulationTrainer: one parameter group per agent's optimiser")
    g = opt.param_groups[0]
    if g.get("maximize", False):
        raise ValueError("PopulationTrainer: an optimiser with maximize is not supported")
    if type(opt) is torch.optim.RMSprop:
        if g["momentum"] != 0 or g["centered"]:
            raise ValueError("PopulationTrainer: RMSprop with momentum or centered is not supported")
        return (torch.optim.RMSprop, float(g["lr"]), float(g["alpha"]), float(g["eps"]), float(g["weight_decay"]))
    if g.get("amsgrad", False):
        raise ValueError("PopulationTrainer: Adam with amsgrad is not supported")
    if g.get("capturable", False) or g.get("differentiable", False):
        raise ValueError("PopulationTrainer: Adam with capturable or differentiable is not supported")
    return (torch.optim.Adam, float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"]))


def minibatch_bounds(n: int, batch_size: int) -> List[Tuple[int, int]]:
    """The minibatches [i, j) of an epoch over n shuffled rows: consecutive slices of ``batch_size``, the last one absorbing the
    remainder (``train_on_rows``'s and ``ReplayBuffer.__next__``'s rule; azg_trainer_epoch cuts the same way)."""
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    out, i = [], 0
    while i < n:
        j = n if i + 2 * batch_size > n else i + batch_size
        out.append((i, j))
        i = j
    return out


def _need_device_losses(losses: str, who: str) -> None:
    if losses != "device":
        raise ValueError(f'PopulationTrainer.{who} needs a trainer built with losses="device" (this one has losses="{losses}"): the '
                         "epoch runs on the device from the gather to the loss sums")


def _check_selfplay(who: str, selfplay, device, n_nets: int) -> None:
    """The self-play engine sits on the trainer's GPU and has the trainer's number of nets."""
    if int(selfplay.engine.cfg.device_id) != (device.index or 0):
        raise ValueError(f"PopulationTrainer.{who}: the ring lies on another GPU than the trainer's nets")
    if selfplay.n_nets != n_nets:
        raise ValueError(f"PopulationTrainer.{who}: the self-play engine has {selfplay.n_nets} nets, the trainer {n_nets}")


def _check_device_tensor(who: str, name: str, t, device, shape: tuple, shape_text: str) -> None:
    """``t`` is a contiguous float32 tensor of ``shape`` on the trainer's GPU: one the native call reads or writes where it lies."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or \
            tuple(t.shape) != shape:
        raise ValueError(f"PopulationTrainer.{who}: {name} must be a contiguous float32 tensor {shape_text} on the trainer's GPU")


def _agents_optim(agents, shared: bool) -> Tuple[List[tuple], List[float]]:
    """``optimizers="agents"``: every agent's (class, settings) and grad_clip after the checks -- grad_clip >= 0 and a supported
    optimiser of one class for all; ``shared`` (``per_net=False``): with one grad_clip and one set of settings."""
    clips = [float(a.clip or 0.0) for a in agents]
    if any(c < 0 for c in clips):
        raise ValueError("PopulationTrainer: grad_clip must be >= 0")
    if shared and len(set(clips)) != 1:
        raise ValueError("PopulationTrainer: every agent must have the same grad_clip")
    settings = [_optimizer_settings(a.optimizer) for a in agents]
    if len({st[0] for st in settings}) != 1:
        raise ValueError("PopulationTrainer: every agent must have the same optimiser class")
    if shared and len(set(settings)) != 1:
        raise ValueError(f"PopulationTrainer: every agent must have the same {settings[0][0].__name__} settings")
    return settings, clips


def _check_losses(agents, per_net: bool, losses: str) -> None:
    """The loss objects share everything (``population_loss`` is written for one set of settings) -- with ``per_net=True`` and
    ``losses="device"`` only what they must (``_loss_shared``)."""
    if len({(_loss_shared if per_net and losses == "device" else _loss_settings)(a.loss) for a in agents}) != 1:
        raise ValueError("PopulationTrainer: every agent must have the same loss class and hyper-parameters"
                         + (' (per-net loss settings need losses="device")' if per_net and losses != "device" else ""))


def _ema_settings(ema, K: int) -> Tuple[Any, int]:
    """``PopulationTrainer(ema=...)`` as (decay, every): a decay, a list of K decays, or ``{"decay": either, "every": N}`` (``every``
    absent: 1).  Every decay is finite and in [0, 1), ``every`` an int >= 1: ``ValueError`` otherwise, before anything is touched."""
    every = 1
    if isinstance(ema, dict):
        unknown = sorted(set(ema) - {"decay", "every"})
        if unknown or "decay" not in ema:
            raise ValueError(f"PopulationTrainer: ema takes decay and every, not {unknown}" if unknown else
                             "PopulationTrainer: ema needs a decay")
        every, ema = ema.get("every", 1), ema["decay"]
    if isinstance(every, bool) or int(every) != every or int(every) < 1:
        raise ValueError(f"PopulationTrainer: ema every must be an int >= 1, got {every!r}")
    if np.ndim(ema) > 1 or isinstance(ema, str):
        raise ValueError("PopulationTrainer: ema decay must be a number or one number per net")
    decay = [float(d) for d in ema] if np.ndim(ema) == 1 else float(ema)
    if isinstance(decay, list) and len(decay) != K:
        raise ValueError(f"PopulationTrainer: ema decay has {len(decay)} entries for {K} nets: a number or one per net")
    for d in decay if isinstance(decay, list) else [decay]:
        if not (np.isfinite(d) and 0.0 <= d < 1.0):
            raise ValueError(f"PopulationTrainer: every ema decay must be finite and in [0, 1), got {d}")
    return decay, int(every)


def _same_steps(states: List[dict], whose: str) -> int:
    """The step count of Adam ``states`` (one dictionary per parameter, empty before the first step) that must agree on it."""
    if not any(states):
        return 0
    if not all(states) or len({float(st["step"]) for st in states}) != 1:
        raise ValueError(f"PopulationTrainer: the agents' {whose} must have taken the same number of steps")
    return int(float(states[0]["step"]))


# What the constructor's checks hand to its later steps: the nets' descriptor and device, every agent's optimiser settings
# (``_optimizer_settings``; with ``optimizers="rmsprop"``, ``_rmsprop_settings``) and grad_clip, Adam's step count, the alpha optimisers'
# states (A0CLossTuned) and step count, and with ``losses="device"`` the azg_loss_cfg (``per_net``: one per net too).
_Checked = namedtuple("_Checked", "desc device settings clips opt_step alpha_states alpha_step loss_cfg net_cfgs")


def _check(agents, losses: str, optimizers: str, per_net: bool, layernorm: bool, wide: bool, wide_layernorm: bool) -> _Checked:
    """Every refusal of the constructor, the arguments' and then the agents', in the order the tests know; changes nothing."""
    if losses not in ("torch", "device"):
        raise ValueError("losses must be 'torch' or 'device'")
    if optimizers not in ("rmsprop", "agents"):
        raise ValueError("optimizers must be 'rmsprop' or 'agents'")
    if per_net and optimizers != "agents":
        raise ValueError('PopulationTrainer: per_net=True requires optimizers="agents"')
    if not agents:
        raise ValueError("PopulationTrainer needs at least one agent")
    a0 = agents[0]
    if len({type(a.nn) for a in agents}) != 1:
        raise ValueError("PopulationTrainer: every agent must have the same policy class")
    if not isinstance(a0.nn, (DiscretePolicy, DiagonalNormalPolicy, DiagonalGMMPolicy)):
        raise ValueError(f"PopulationTrainer: policy {type(a0.nn).__name__} is not supported")
    if wide_layernorm and layernorm:
        raise ValueError("PopulationTrainer: wide_layernorm=True and layernorm=True ask for two different trainers")
    if wide and not wide_layernorm and (layernorm or any(a.nn.layernorm for a in agents)):
        raise ValueError("PopulationTrainer: wide=True does not train LayerNorm trunks on the device")
    if not layernorm and not wide_layernorm and any(a.nn.layernorm for a in agents):
        raise ValueError("PopulationTrainer: LayerNorm trunks are not trained on the device")
    opt_step = 0
    if optimizers == "agents":
        settings, clips = _agents_optim(agents, shared=not per_net)
        if settings[0][0] is torch.optim.Adam:
            opt_step = _same_steps([a.optimizer.state.get(p, {}) for a in agents for p in a.nn.parameters()], "Adam optimisers")
    else:
        if any(a.clip for a in agents):
            raise ValueError("PopulationTrainer: grad_clip != 0 is not supported (a per-net global norm needs a pass of its own)")
        settings, clips = [_rmsprop_settings(a.optimizer) for a in agents], [0.0] * len(agents)
        if len(set(settings)) != 1:
            raise ValueError("PopulationTrainer: every agent must have the same RMSprop settings")
    _check_losses(agents, per_net, losses)
    max_layers, max_width = (8, 1024) if (wide or wide_layernorm) else (3, 256)
    unsupported = (f"PopulationTrainer: supported nets have 1-{max_layers} hidden layers of widths 16, 32, ... {max_width}, at most "
                   "8 inputs and 16 distribution outputs")
    if any(len(list(a.nn.hidden_dimensions)) > _capi.MAX_HIDDEN for a in agents):   # (more than a descriptor holds)
        raise ValueError(unsupported)
    descs = [_capi.policy_tensors(a.nn) for a in agents]
    if any([tuple(t.shape) for t in ts] != [tuple(t.shape) for t in descs[0][1]] or bytes(d) != bytes(descs[0][0]) for d, ts in descs):
        raise ValueError("PopulationTrainer: every agent must have the same network shape, activation and head settings")
    d0 = descs[0][0]
    hidden = [d0.hidden[i] for i in range(d0.n_hidden)]
    if not (1 <= d0.n_hidden <= max_layers and all(h % 16 == 0 and 16 <= h <= max_width for h in hidden) and d0.in_dim <= 8
            and d0.n_dist <= 16):
        raise ValueError(unsupported)
    pars = [p for a in agents for p in a.nn.parameters()]
    device = pars[0].device
    if device.type != "cuda" or any(p.device != device for p in pars):
        raise ValueError("PopulationTrainer: every parameter must live on one GPU (there is no CPU form of the trainer's kernels)")
    alpha_states = [a.loss.optimizer.state.get(a.loss.log_alpha, {}) for a in agents] if type(a0.loss) is A0CLossTuned else []
    alpha_step = _same_steps(alpha_states, "alpha optimisers")
    loss_cfg = _capi.loss_cfg(a0.nn, a0.loss) if losses == "device" else None
    net_cfgs = [_capi.loss_cfg(a.nn, a.loss) for a in agents] if (per_net and losses == "device") else None
    return _Checked(d0, device, settings, clips, opt_step, alpha_states, alpha_step, loss_cfg, net_cfgs)


class PopulationTrainer:
    """The optimiser step of K agents of one shape, all at once.  Raises ``ValueError`` naming the reason when the agents cannot be
    trained here (the caller then keeps the per-agent ``agent.update`` loop): different network shapes, LayerNorm (unless
    ``layernorm=True``), gradient clipping or an optimiser other than plain RMSprop (unless ``optimizers="agents"``), different
    losses or hyper-parameters, parameters not on a GPU.

    Binds the agents' parameters to ``self.flat`` [K, P] (``bind_flat``) and their RMSprop ``square_avg`` state to
    ``self.square_avg`` [K, P] (state an agent already has is taken over; the agents' torch optimisers keep working on the same
    storage).  With ``A0CLossTuned`` the learned temperatures live in ``self.log_alpha`` [K] under one Adam; ``export_alpha()``
    (called by ``close()``) writes them and their Adam state back into the agents' loss objects, which are stale until then.  After ``update`` hand the weights to the search with
    ``PopulationMCTS.upload_flat(trainer.desc, trainer.flat)``.

    ``losses``: "torch" computes the losses and ``d_raw`` in PyTorch between the two launches; "device" computes them in a kernel of
    the same step (``_capi.Trainer.step``).  Then ``log_alpha`` and its Adam state (``alpha_exp_avg``, ``alpha_exp_avg_sq``,
    ``alpha_step``) are plain tensors of the trainer that the kernel steps in place, and there is no ``alpha_optimizer``.

    ``optimizers``: "rmsprop" (the default) takes plain RMSprop without gradient clipping and steps it inside the backward kernel
    (its weighted, errors and online calls, for which azg_rmsprop has no entry points, take the ``*_opt`` ones with the same
    RMSprop as an azg_optim, ``_optim``: the same bits; ``opt_step`` stays 0).  "agents" takes what the agents carry -- plain RMSprop
    or ``torch.optim.Adam`` (no amsgrad), and their ``grad_clip`` -- through the ``*_opt`` entry points: the backward launch writes
    the gradients first, then computes every net's global norm, clips and steps.  Every agent must have the same optimiser class, settings and ``grad_clip``, and, with Adam, have taken the same number
    of steps.  Adam's ``exp_avg`` / ``exp_avg_sq`` become ``self.exp_avg`` / ``self.exp_avg_sq`` [K, P] with the agents' optimiser
    state as views of their rows; ``self.opt_step`` counts the steps and ``export_alpha()`` / ``close()`` write it to every
    ``state[p]["step"]``.  ``self.last_grad_norms`` [K] holds every net's gradient norm (before clipping) of the last step.

    ``layernorm``: True also takes agents whose trunks have ``nn.LayerNorm`` after every activation (all of them, or none: a mix is
    a different network shape).  The native trainer is then made by azg_trainer_create_ex and runs the LayerNorm forms of its
    kernels; ``flat``, the optimiser state, ``grads`` and the gradient norm cover ln.weight and ln.bias like every other parameter.

    ``wide``: True takes every network shape the engine can search: 1-8 hidden layers of widths 16, 32, ... 1024 (narrow agents
    too).  The native trainer is then made by azg_trainer_create_wide, whose kernels spread every layer over the chip, one launch
    per layer and direction; a shape the default trainer also takes gets the same bits.  LayerNorm trunks are not among them:
    ``wide=True`` with ``layernorm=True`` or with LayerNorm agents raises.

    ``wide_layernorm``: True is the wide trainer that also takes LayerNorm agents (agents without LayerNorm too): the same 8 x 1024
    limits, checks and behaviour as ``wide=True``, the native trainer made by azg_trainer_create_wide_ex, which adds a row pass per
    LayerNorm and direction to the wide trainer's launches.  Together with ``layernorm=True`` it raises: two different trainers.

    ``per_net``: True (needs ``optimizers="agents"``) lets the agents differ in their optimiser's numeric settings (lr, eps,
    weight_decay, RMSprop's alpha, Adam's betas) and in ``grad_clip``, and with ``losses="device"`` also in their loss's numeric
    settings (tau, the coefficients, A0CLoss's alpha, the tuned loss's target entropy, alpha optimiser settings and clip): a
    learning-rate sweep in one trainer.  Optimiser class, loss class, reduction, network shape and step counts are still shared.
    Every call then goes through the ``*_nets`` entry points, which read one settings entry per net; agents with equal settings
    get the bits of ``per_net=False``.  ``reload_settings()`` reads the agents' settings again, e.g. after a schedule or an
    exploit/explore step changed ``optimizer.param_groups[0]["lr"]``.  ``copy_nets(src)`` is that step's exploit half: net k
    becomes a faithful clone of net ``src[k]`` (``alphazero_gym_amd.pbt.PopulationBasedTraining`` drives the whole step).

    ``ema`` (None: off, every call launches what it always did): a decay in [0, 1), a list of K decays, or ``{"decay": ..., "every":
    N}`` keeps ``self.ema`` [K, P], a slowly moving copy of ``flat`` (include/azgym_train_ema.h): a copy of it to begin with, and after
    every N-th optimiser step -- of ``update`` with either ``losses``, and of every minibatch inside ``train_epoch``,
    ``train_epoch_ring`` and ``train_online_ring`` -- ``ema += (1 - decay_k) * (flat - ema)`` in float32, one more launch behind the
    step's, no synchronisation.  The count of steps carries over from call to call.  ``ema_decay`` / ``ema_every`` are the settings in
    force (``ema_decay`` None: detached), ``ema_updates`` the times it moved; ``set_ema`` re-attaches with other settings or detaches,
    ``reset_ema(nets)`` copies rows of ``flat`` again, ``copy_nets`` clones the row (with a list of decays also the decay) and
    ``close()`` detaches.  Hand it to the search as its target set: ``PopulationSelfPlay.upload_target_flat(trainer.desc, trainer.ema)``."""

    def __init__(self, agents: Sequence[Any], max_batch: int = 512, keep_grads: bool = False, losses: str = "torch",
                 optimizers: str = "rmsprop", layernorm: bool = False, wide: bool = False, wide_layernorm: bool = False,
                 per_net: bool = False, ema=None):
        # 1. checks that touch nothing: the arguments, then the agents
        self.agents = list(agents)
        ema_settings = None if ema is None else _ema_settings(ema, len(self.agents))
        self.per_net, self.losses, self.optimizers = bool(per_net), losses, optimizers
        self.layernorm, self.wide, self.wide_layernorm = bool(layernorm), bool(wide), bool(wide_layernorm)
        c = _check(self.agents, losses, optimizers, self.per_net, self.layernorm, self.wide, self.wide_layernorm)
        # 2. the native trainer: if it cannot be created, the agents are left as they were
        from .. import _native   # raises if libazgym_hip.so is missing
        K = len(self.agents)
        self.max_batch = int(max_batch)
        kind = "wide_layernorm" if self.wide_layernorm else "wide" if self.wide else "layernorm" if self.layernorm else None
        self.trainer = _native.HipTrainer(c.desc, K, self.max_batch, device_id=c.device.index or 0, **({kind: True} if kind else {}))
        self.policy, self.loss, self.device = self.agents[0].nn, self.agents[0].loss, c.device
        self.loss_cfg, self.loss_cfgs = c.loss_cfg, None   # (loss_cfgs: per_net=True, losses="device": one azg_loss_cfg per net)
        # the form of the trainer's calls: the row of _capi.TRAINER_CALLS and the optimiser settings its methods are given
        self.opt, self.last_grad_norms, self.opt_step = None, None, c.opt_step
        if optimizers == "agents":
            self._calls = _capi.TRAINER_CALLS["nets" if self.per_net else "opt"]
            self._opt_settings, self.grad_clip = c.settings[0], c.clips[0]
            self.last_grad_norms = torch.zeros(K, dtype=torch.float32, device=c.device)
        else:
            self._calls = _capi.TRAINER_CALLS["rmsprop"]
            lr, alpha, eps, wd = c.settings[0]
            self.opt = _capi.rmsprop_opt(lr=lr, alpha=alpha, eps=eps, weight_decay=wd)
            self._opt_settings = (torch.optim.RMSprop, lr, alpha, eps, wd)
        # 3. binding: the parameters, the optimiser's moments, the learned temperature
        self.desc, self.flat = bind_flat([a.nn for a in self.agents])
        self._bind_moments(adam=self._opt_settings[0] is torch.optim.Adam)
        self.grads = torch.zeros_like(self.flat) if keep_grads else None
        self._bind_alpha(c.alpha_states, c.alpha_step)
        self.last_raw: Optional[torch.Tensor] = None
        self._last_d_raw: Optional[torch.Tensor] = None
        # 4. the per-net arrays
        if self.per_net:
            self._set_net_entries(c.settings, c.clips, c.net_cfgs)
        # 5. the moving average of the parameters, a copy of them to begin with
        self.ema: Optional[torch.Tensor] = None
        self.ema_decay, self.ema_every = None, 1
        if ema_settings is not None:
            self.ema = self.flat.clone()
            self._attach_ema(*ema_settings)

    def _attach_ema(self, decay, every: int) -> None:
        """azg_trainer_set_ema over ``self.ema`` with checked settings (``_ema_settings``); the native step count starts again."""
        torch.cuda.current_stream(self.device).synchronize()   # (the copies that filled ``ema`` are complete)
        self.trainer.set_ema(self.ema.data_ptr(), decay, every)
        self.ema_decay, self.ema_every = decay, every

    @property
    def ema_updates(self) -> int:
        """How often the average has moved since it was last attached (the constructor, ``set_ema``, ``copy_nets`` with a list of
        decays): one launch per ``every`` optimiser steps.  0 without an average."""
        return self.trainer.ema_info()[1] if self.ema is not None and self.ema_decay is not None else 0

    def set_ema(self, decay=None, every: Optional[int] = None) -> None:
        """Re-attach the average with new settings (None: the one in force); ``set_ema(None)`` with nothing else detaches it: the
        steps after it leave ``ema`` as it stands (the tensor stays readable).  A trainer built without ``ema=`` has no average to
        re-attach: ``ValueError``."""
        if self.ema is None:
            raise ValueError("PopulationTrainer.set_ema needs a trainer built with ema=...")
        if decay is None and every is None:
            self.trainer.set_ema(None)
            self.ema_decay = None
            return
        if decay is None and self.ema_decay is None:
            raise ValueError("PopulationTrainer.set_ema: the average is detached: give a decay")
        self._attach_ema(*_ema_settings({"decay": self.ema_decay if decay is None else decay,
                                         "every": self.ema_every if every is None else every}, len(self.agents)))

    def reset_ema(self, nets=None) -> None:
        """Copy the rows ``nets`` (None: all) of ``flat`` into ``ema`` again: those nets' averages start afresh from where the nets
        stand.  Row copies on the current stream; the step count and the settings stay."""
        if self.ema is None:
            raise ValueError("PopulationTrainer.reset_ema needs a trainer built with ema=...")
        with torch.no_grad():
            if nets is None:
                self.ema.copy_(self.flat)
                return
            rows = [int(k) for k in nets]
            if any(not 0 <= k < len(self.agents) for k in rows):
                raise ValueError(f"PopulationTrainer.reset_ema: nets must be in 0 .. {len(self.agents) - 1}")
            idx = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
            self.ema[idx] = self.flat[idx]

    def _bind_moments(self, adam: bool) -> None:
        """The optimiser's moments as [K, P] tensors of the trainer (``square_avg``, or Adam's ``exp_avg`` and ``exp_avg_sq``), every
        agent's ``optimizer.state`` entries re-pointed at views of its row; state an agent already has is taken over."""
        self.square_avg, self.exp_avg, self.exp_avg_sq = None, None, None
        if adam:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
            bound = (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq))
        else:
            self.square_avg = torch.zeros_like(self.flat)
            bound = (("square_avg", self.square_avg),)
        for k, a in enumerate(self.agents):
            off = 0
            g = a.optimizer.param_groups[0]
            for p in _capi.policy_tensors(a.nn)[1]:
                st = a.optimizer.state[p]
                if "step" not in st:   # (torch keeps the count on the host unless the optimiser is capturable or fused)
                    st["step"] = torch.tensor(0.0, device=p.device if (g.get("capturable") or g.get("fused")) else "cpu")
                for name, table in bound:
                    view = table[k, off:off + p.numel()].view_as(p)
                    if name in st:
                        view.copy_(st[name])
                    st[name] = view
                off += p.numel()

    def _bind_alpha(self, states: List[dict], step: int) -> None:
        """A0CLossTuned: the K learned temperatures as ``log_alpha`` [K] with the agents' alpha optimisers' ``states`` taken over --
        ``losses="device"``: plain float32 tensors that the loss kernel steps, ``alpha_step`` counting; ``losses="torch"``: a leaf
        under one torch Adam, ``alpha_optimizer``, which counts its own steps."""
        self.log_alpha, self.alpha_optimizer = None, None
        self.alpha_exp_avg, self.alpha_exp_avg_sq, self.alpha_step = None, None, 0
        if type(self.loss) is not A0CLossTuned:
            return
        device = self.device
        if self.losses == "device":
            self.log_alpha = torch.stack([a.loss.log_alpha.detach().to(device, dtype=torch.float32) for a in self.agents]).contiguous()
            self.alpha_exp_avg, self.alpha_exp_avg_sq = torch.zeros_like(self.log_alpha), torch.zeros_like(self.log_alpha)
            if any(states):
                self.alpha_step = step
                self.alpha_exp_avg = torch.stack([s["exp_avg"].to(device, dtype=torch.float32) for s in states]).contiguous()
                self.alpha_exp_avg_sq = torch.stack([s["exp_avg_sq"].to(device, dtype=torch.float32) for s in states]).contiguous()
            return
        self.log_alpha = torch.stack([a.loss.log_alpha.detach().to(device) for a in self.agents]).requires_grad_(True)
        g = self.loss.optimizer.param_groups[0]
        self.alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
        if any(states):
            self.alpha_optimizer.state[self.log_alpha] = {
                "step": torch.tensor(float(step)),
                "exp_avg": torch.stack([s["exp_avg"].to(device) for s in states]),
                "exp_avg_sq": torch.stack([s["exp_avg_sq"].to(device) for s in states])}

    @property
    def last_d_raw(self) -> Optional[torch.Tensor]:
        """d loss_k / d raw[k] of the last ``update``, [K, B, 1 + n_dist] (with ``losses="device"`` it stays in the native trainer
        and is copied out when asked for)."""
        if self._last_d_raw is None and self.last_raw is not None and self.losses == "device":
            d = torch.empty_like(self.last_raw)
            torch.cuda.current_stream(self.device).synchronize()
            self.trainer.read_d_raw(d.shape[1], d.data_ptr())
            self._last_d_raw = d
        return self._last_d_raw

    def __len__(self) -> int:
        return len(self.agents)

    def _stacked(self, x) -> torch.Tensor:
        """A batch field as one float32 [K, B, ...] tensor on the trainer's device (a sequence of K per-net fields is stacked)."""
        if not isinstance(x, torch.Tensor):
            x = torch.stack([f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)) for f in x])
        return x.to(self.device, dtype=torch.float32).contiguous()

    def _row_weights(self, who: str, weights, K: int, B: int) -> torch.Tensor:
        """``weights`` as a contiguous float32 [K, B] tensor on the trainer's device."""
        if not isinstance(weights, torch.Tensor):
            weights = torch.as_tensor(np.asarray(weights, dtype=np.float32))
        weights = weights.to(self.device, dtype=torch.float32).contiguous()
        if tuple(weights.shape) != (K, B):
            raise ValueError(f"PopulationTrainer.{who}: weights must be [K = {K}, {B}]")
        return weights

    def update(self, batches, weights=None) -> List[Dict[str, float]]:
        """One optimiser step of every net on its own minibatch.  ``batches``: K tuples (states, actions, counts, Qs, V_target), the
        argument of ``Agent.update``, with equal row counts -- or one such tuple of stacked [K, B, ...] tensors.  Returns what K
        ``agent.update`` calls return.  ``weights``: a [K, B] tensor, one weight per minibatch row (importance-sampling weights of
        prioritised rows), multiplied into the row's summands of every loss (``population_loss``; with ``losses="device"`` the
        weighted loss kernel); None is the unweighted step."""
        K = len(self.agents)
        if isinstance(batches, (list, tuple)) and len(batches) == 5 and isinstance(batches[0], torch.Tensor) and batches[0].dim() == 3:
            states, actions, counts, _, v_target = batches
        else:
            if len(batches) != K:
                raise ValueError("PopulationTrainer.update: one minibatch per net")
            if len({len(b[0]) for b in batches}) != 1:
                raise ValueError("PopulationTrainer.update: every net's minibatch must have the same number of rows")
            states, actions, counts, _, v_target = zip(*batches)
        states, actions, counts = self._stacked(states), self._stacked(actions), self._stacked(counts)
        B = states.shape[1]
        values = self._stacked(v_target).reshape(K, B, 1)
        if states.shape[0] != K or not 1 <= B <= self.max_batch:
            raise ValueError(f"PopulationTrainer.update: needs [K = {K}, 1..{self.max_batch} rows, ...] minibatches")
        states = states.reshape(K, B, -1)
        raw = torch.empty((K, B, self.trainer.n_raw), dtype=torch.float32, device=self.device)
        if weights is not None:
            weights = self._row_weights("update", weights, K, B)
        grads = self.grads.data_ptr() if self.grads is not None else None
        if self.losses == "device":   # one native call (three launches), one copy of losses[K, 5] to the host
            actions, counts = actions.reshape(K, B, -1), counts.reshape(K, B, -1)
            variant, w = ("plain", ()) if weights is None else ("weighted", (weights.data_ptr(),))
            return self._call("step", variant, (self.flat.data_ptr(), states.data_ptr(), actions.data_ptr(), counts.data_ptr(),
                                                values.data_ptr(), *w, B, actions.shape[2]), (grads, raw.data_ptr()), raw=raw)[1]
        torch.cuda.current_stream(self.device).synchronize()
        self.trainer.forward(self.flat.data_ptr(), states.data_ptr(), B, raw.data_ptr())
        raw.requires_grad_(True)
        losses = population_loss(self.policy, self.loss, raw, actions, counts, values, self.log_alpha, self.alpha_optimizer, weights=weights)
        losses["loss"].sum().backward()
        d_raw = raw.grad.contiguous()
        out = per_net(losses)   # (the copy to the host also completes d_raw)
        # (a clip happens inside: PyTorch never sees the parameter gradients)
        self._call("backward_step", "plain", (self.flat.data_ptr(), d_raw.data_ptr(), B), (grads,), raw=raw, d_raw=d_raw)
        return out

    def _call(self, family: str, variant: str, head: tuple, tail: tuple = (), raw=None, d_raw=None, steps: Optional[int] = None, **kw):
        """Every native call that steps the nets, and the bookkeeping after it: (what the method returned, the K loss dictionaries).
        ``family`` ("backward_step", "step", "epoch") and ``variant`` ("plain", "weighted", "errors", "online") name the entry of
        ``self._calls``: the ``_capi.Trainer`` method and the form in which it takes the optimiser.  The method gets ``head``, the
        loss settings and the learned temperature's state, the optimiser's arguments, ``tail`` and the [K, 5] table it writes the
        losses to (float32 for a step, float64 for an epoch's sums) -- "backward_step", with no loss in it, only ``head``, the
        optimiser and ``tail``.  The work queued on the current stream is complete before it.  Afterwards the steps taken
        (``steps``; else what the method returns, an epoch's number of minibatches; else 1) are counted in ``opt_step``, which stays
        0 for ``optimizers="rmsprop"``, and in ``alpha_step`` where the call stepped a learned temperature; ``last_raw`` /
        ``last_d_raw`` become ``raw`` / ``d_raw`` (None: the raw outputs stay in the native trainer)."""
        method, opt_form = self._calls[family, variant]
        with_loss = family != "backward_step"
        tuned = with_loss and self.log_alpha is not None
        if with_loss:
            state = _capi.alpha_state(self.alpha_step, self.log_alpha.data_ptr(), self.alpha_exp_avg.data_ptr(),
                                      self.alpha_exp_avg_sq.data_ptr()) if tuned else None
            head += (self.loss_cfgs if self.per_net else self.loss_cfg, state)
            table = torch.empty((len(self.agents), len(_capi.LOSS_KEYS)), dtype=torch.float32 if family == "step" else torch.float64,
                                device=self.device)
            tail += (table.data_ptr(),)
        if opt_form == "nets":   # (per_net=True: the array of azg_optim, the step count written into all)
            self._net_steps[:] = self.opt_step
        opt = (self._net_opts,) if opt_form == "nets" else (self._optim(),) if opt_form == "opt" else (self.opt, self.square_avg.data_ptr())
        torch.cuda.current_stream(self.device).synchronize()
        out = method(self.trainer, *head, *opt, *tail, **kw)
        n_steps = steps if steps is not None else 1 if out is None else out
        if self.optimizers == "agents":
            self.opt_step += n_steps
        if tuned:
            self.alpha_step += n_steps
        self.last_raw, self._last_d_raw = raw, d_raw
        if not with_loss:
            return out, None
        slots = [(key, _capi.LOSS_KEYS.index(key)) for key in _capi.LOSS_KEYS_OF[self.loss_cfg.kind]]
        return out, [{key: row[i] for key, i in slots} for row in table.cpu().tolist()]

    def reload_settings(self) -> None:
        """Read every agent's ``optimizer.param_groups[0]``, ``clip`` and loss object again (``per_net=True`` only), with the
        constructor's checks; the next ``update`` / epoch uses them.  If a check refuses, it raises ``ValueError`` and the trainer
        keeps the settings it had.  The optimiser state, the step counts and the learned temperatures are the trainer's and are
        not touched."""
        if not self.per_net:
            raise ValueError("PopulationTrainer.reload_settings needs a trainer built with per_net=True")
        settings, clips = _agents_optim(self.agents, shared=False)
        if settings[0][0] is not self._opt_settings[0]:
            raise ValueError("PopulationTrainer.reload_settings: the optimiser class cannot change")
        _check_losses(self.agents, True, self.losses)
        cfgs = None
        if self.losses == "device":
            cfgs = [_capi.loss_cfg(a.nn, a.loss) for a in self.agents]
            fixed = operator.attrgetter("kind", "head", "reduction", "action_bound")
            if any(fixed(c) != fixed(self.loss_cfg) for c in cfgs):
                raise ValueError("PopulationTrainer.reload_settings: loss class, head and reduction cannot change")
        self._set_net_entries(settings, clips, cfgs)

    def copy_nets(self, src) -> None:
        """The exploit half of population-based training (``alphazero_gym_amd.pbt``): row k of every per-net piece of state becomes
        row ``src[k]`` -- ``flat`` and the optimiser's moments (``square_avg``, or ``exp_avg`` and ``exp_avg_sq``: the agents'
        modules, ``state_dict()`` and torch optimisers are views of those rows and see the copy), and with ``A0CLossTuned`` the
        learned temperature with its Adam moments (``losses="device"``: ``log_alpha``, ``alpha_exp_avg``, ``alpha_exp_avg_sq``;
        ``losses="torch"``: ``log_alpha.data`` and the ``alpha_optimizer``'s state).  With ``per_net=True`` agent k also takes agent
        ``src[k]``'s numeric optimiser settings, ``clip`` and numeric loss settings, and ``reload_settings()`` runs; without it the
        settings are shared.  ``opt_step`` and ``alpha_step`` are shared by all nets and stay.  ``src``: K ints in range with
        ``src[src[k]] == src[k]`` (``pbt.check_src``; ``ValueError`` before anything is written).  The copies are row copies on the
        trainer's stream; hand the result to the search with ``upload_flat`` (a copy into views bumps no ``_version``)."""
        src = check_src(src, len(self.agents))
        replaced = [k for k in range(len(self.agents)) if int(src[k]) != k]
        if not replaced:
            return
        to = torch.as_tensor(replaced, dtype=torch.int64, device=self.device)
        frm = torch.as_tensor([int(src[k]) for k in replaced], dtype=torch.int64, device=self.device)
        tables = [self.flat, self.square_avg, self.exp_avg, self.exp_avg_sq, self.alpha_exp_avg, self.alpha_exp_avg_sq, self.ema]
        if self.log_alpha is not None:
            tables.append(self.log_alpha.data)
        if self.alpha_optimizer is not None:
            st = self.alpha_optimizer.state.get(self.log_alpha, {})
            tables += [st.get("exp_avg"), st.get("exp_avg_sq")]
        with torch.no_grad():
            for t in tables:
                if t is not None:
                    t[to] = t[frm]   # (sources are never replaced: the gather is complete before the scatter writes)
        if isinstance(self.ema_decay, list):   # (a clone averages at its source's pace; the native step count starts again)
            self._attach_ema([self.ema_decay[int(s)] for s in src], self.ema_every)
        if not self.per_net:
            return
        for k in replaced:
            a, s = self.agents[k], self.agents[int(src[k])]
            ga, gs = a.optimizer.param_groups[0], s.optimizer.param_groups[0]
            for key in ("lr", "eps", "weight_decay", "alpha", "betas"):
                if key in gs:
                    ga[key] = gs[key]
            a.clip = s.clip
            for key in ("tau", "policy_coeff", "value_coeff", "target_entropy", "clip"):
                if hasattr(s.loss, key):
                    setattr(a.loss, key, getattr(s.loss, key))
            if type(s.loss) is A0CLoss:
                a.loss.alpha = s.loss.alpha
            elif type(s.loss) is A0CLossTuned:
                la, ls = a.loss.optimizer.param_groups[0], s.loss.optimizer.param_groups[0]
                for key in ("lr", "betas", "eps", "weight_decay"):
                    la[key] = ls[key]
        self.reload_settings()

    def _set_net_entries(self, settings: List[tuple], clips: List[float], cfgs: Optional[list]) -> None:
        """``per_net=True``: the arrays the ``*_nets`` calls read, built once per set of settings -- one azg_optim per net (its
        agent's settings over the shared state tensors; ``_call`` writes the step count into all of them) and, with
        ``losses="device"``, one azg_loss_cfg per net."""
        out = [self._azg_optim(st, clip) for st, clip in zip(settings, clips)]
        opts = (_capi.AzgOptim * len(out))(*out)
        words = C.sizeof(_capi.AzgOptim) // 4
        steps = np.frombuffer(opts, dtype=np.int32).reshape(len(out), words)[:, _capi.AzgOptim.step.offset // 4]
        self._net_opt_settings, self._net_clips = settings, clips
        self._net_opts, self._net_steps = opts, steps
        self.loss_cfgs = (_capi.AzgLossCfg * len(cfgs))(*cfgs) if cfgs is not None else None

    def _azg_optim(self, st: tuple, clip: float):
        """azg_optim of an ``_optimizer_settings`` tuple and a grad_clip over the trainer's state tensors and step count."""
        norms = self.last_grad_norms
        common = dict(grad_clip=clip, step=self.opt_step, grad_norms=norms.data_ptr() if norms is not None else None)
        if st[0] is torch.optim.Adam:
            _, lr, betas, eps, wd = st
            return _capi.optim("adam", lr, self.exp_avg_sq.data_ptr(), self.exp_avg.data_ptr(), eps=eps, weight_decay=wd, betas=betas,
                               **common)
        _, lr, alpha, eps, wd = st
        return _capi.optim("rmsprop", lr, self.square_avg.data_ptr(), eps=eps, weight_decay=wd, alpha=alpha, **common)

    def _optim(self):
        """azg_optim of the next step over the trainer's state tensors and step count.  ``optimizers="agents"``: the agents' settings
        and grad_clip.  ``optimizers="rmsprop"``: the trainer's RMSprop restated for the ``*_opt`` entry points that serve its
        weighted, errors and online calls (azg_rmsprop has none): no clip, no grad_norms, step 0 -- the same bits."""
        return self._azg_optim(self._opt_settings, self.grad_clip if self.optimizers == "agents" else 0.0)

    def train_on_rows(self, rows_per_net, state_dim: int, K: int, batch_size: int = 32,
                      shuffle_seeds: Optional[Sequence[int]] = None, weights=None) -> List[Dict[str, float]]:
        """``run.train_on_rows`` for every net at once: one epoch of minibatch updates over ``rows_per_net`` (K tensors [n, row] with
        the same n, or one [K, n, row] tensor; row = obs | actions[K] | counts[K] | Q[K] | V), net k's rows shuffled with
        ``shuffle_seeds[k]``; the last minibatch absorbs the remainder.  Returns per net the per-key sums.  ``weights``: a [K, n]
        tensor, one weight per row, gathered with every minibatch and passed to ``update`` (None: unweighted)."""
        rows = rows_per_net if isinstance(rows_per_net, torch.Tensor) else torch.stack(list(rows_per_net))
        rows = rows.to(self.device, dtype=torch.float32)
        N, n = rows.shape[0], rows.shape[1]
        if N != len(self.agents):
            raise ValueError("PopulationTrainer.train_on_rows: one block of rows per net")
        if weights is not None:
            weights = self._row_weights("train_on_rows", weights, N, n)
        seeds = [0] * N if shuffle_seeds is None else list(shuffle_seeds)
        order = torch.from_numpy(np.stack([np.random.RandomState(int(s)).permutation(n) for s in seeds])).to(self.device)
        net = torch.arange(N, device=self.device)[:, None]
        sums: List[Dict[str, float]] = [{} for _ in range(N)]
        for i, j in minibatch_bounds(n, batch_size):
            b = rows[net, order[:, i:j]]
            batch = (b[..., :state_dim], b[..., state_dim:state_dim + K], b[..., state_dim + K:state_dim + 2 * K],
                     b[..., state_dim + 2 * K:state_dim + 3 * K], b[..., -1])
            infos = self.update(batch, weights=None if weights is None else weights[net, order[:, i:j]])
            for s, info in zip(sums, infos):
                for key, val in info.items():
                    s[key] = s.get(key, 0.0) + val
        return sums

    def _epoch(self, who: str, where, order: np.ndarray, batch_size: int, weights: Optional[int] = None,
               errors: Optional[int] = None) -> List[Dict[str, float]]:
        """azg_trainer_epoch on rows described by ``where`` (``_capi.epoch_rows``), their producers complete; the per-net sums.
        ``weights``: the device address of a float32 array addressed like the rows (None: the unweighted epoch).  ``errors``: the
        device address of a float32 array addressed like them that receives the trained rows' value errors (None: none)."""
        bounds = minibatch_bounds(order.shape[1], int(batch_size))
        if not bounds or max(j - i for i, j in bounds) > self.max_batch:
            raise ValueError(f"PopulationTrainer.{who}: needs minibatches of 1..{self.max_batch} rows")
        variant, w = ("errors", (weights, errors)) if errors is not None else ("weighted", (weights,)) if weights is not None else ("plain", ())
        n_steps, sums = self._call("epoch", variant, (self.flat.data_ptr(), where, *w, order, int(batch_size)))
        assert n_steps == len(bounds)
        return sums

    def train_epoch(self, rows_per_net, state_dim: int, K: int, batch_size: int = 32,
                    shuffle_seeds: Optional[Sequence[int]] = None, weights=None, errors=None) -> List[Dict[str, float]]:
        """``train_on_rows`` as one native call (``azg_trainer_epoch``): the same arguments, minibatches, arithmetic and return
        value, bit for bit, with one synchronisation for the whole epoch.  The permutations are built on the host as there; the
        minibatches are gathered from ``rows_per_net`` on the device (a [K, n, row] float32 tensor on the trainer's GPU is read in
        place).  Needs ``losses="device"``; ``grads`` (``keep_grads``) is not written.  ``weights``: a [K, n] float32 tensor, one
        weight per row, gathered with the row (azg_trainer_epoch_opt_weighted); None is the unweighted epoch.  ``errors``: a
        contiguous [K, n] float32 tensor on the trainer's GPU that receives the value error |V - z| of every row trained on, written
        by the minibatches' loss launches (azg_trainer_epoch_opt_errors); entries of rows not drawn stay as they are."""
        _need_device_losses(self.losses, "train_epoch")
        rows = rows_per_net if isinstance(rows_per_net, torch.Tensor) else torch.stack(list(rows_per_net))
        rows = rows.to(self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 3 or rows.shape[0] != len(self.agents):
            raise ValueError("PopulationTrainer.train_epoch: one block of rows per net")
        N, n = rows.shape[0], rows.shape[1]
        if rows.shape[2] != state_dim + 3 * K + 1:
            raise ValueError("PopulationTrainer.train_epoch: rows must be obs[state_dim] | actions[K] | counts[K] | Q[K] | V")
        seeds = [0] * N if shuffle_seeds is None else list(shuffle_seeds)
        order = np.stack([np.random.RandomState(int(s)).permutation(n) for s in seeds]).astype(np.int32)
        if weights is not None:
            weights = self._row_weights("train_epoch", weights, N, n)
        if errors is not None:
            _check_device_tensor("train_epoch", "errors", errors, self.device, (N, n), f"[{N}, {n}]")
        return self._epoch("train_epoch", _capi.epoch_rows(rows.data_ptr(), state_dim, K, n), order, batch_size,
                           None if weights is None else weights.data_ptr(), None if errors is None else errors.data_ptr())

    def train_epoch_ring(self, selfplay, order, batch_size: int = 32, weights=None, errors: bool = False) -> List[Dict[str, float]]:
        """One epoch straight from a ``PopulationSelfPlay`` / ``DeviceSelfPlay`` engine's replay ring, with no copy of the rows and
        no index tensors on the device.  ``order``: int array [K, n_order]; order[k] numbers net k's rows of the ring as
        ``PopulationSelfPlay._split`` orders them (row i = stored step i // T, game i % T of the net's T games) -- the caller's pick
        and shuffle composed.  The engine's stream is synchronised first (``azg_sync``); the ring is neither cleared nor changed.

        ``weights``: "priority" trains with the engine's importance-sampling weights (``PopulationSelfPlay.is_weights`` must have run
        since the last ``priorities``; the engine's refusal surfaces as it is); a [capacity_steps, n_games] float32 tensor on the
        trainer's GPU gives a weight per ring slot and game; None runs the unweighted calls.

        ``errors``: True also writes the value error |V - z| of every row trained on into the engine's kept errors
        (``PopulationSelfPlay(prioritized={..., "feedback": ...})``), from the minibatches' own loss launches; the next
        ``priorities()`` of the self-play engine reads them.  A row in several minibatches keeps the last one's error."""
        _need_device_losses(self.losses, "train_epoch_ring")
        if errors and "feedback" not in (getattr(selfplay, "prioritized", None) or {}):
            raise ValueError('PopulationTrainer.train_epoch_ring: errors=True needs a self-play engine built with '
                             'prioritized={..., "feedback": ...}')
        if isinstance(weights, str):
            if weights != "priority":
                raise ValueError('PopulationTrainer.train_epoch_ring: weights must be "priority", a tensor or None')
            if getattr(selfplay, "prioritized", None) is None:
                raise ValueError('PopulationTrainer.train_epoch_ring: weights="priority" needs a self-play engine built with '
                                 "prioritized=")
        _check_selfplay("train_epoch_ring", selfplay, self.device, len(self.agents))
        engine = selfplay.engine
        order = np.asarray(order)
        if order.ndim != 2 or order.shape[0] != len(self.agents) or order.shape[1] < 1 or order.dtype.kind not in "iu":
            raise ValueError("PopulationTrainer.train_epoch_ring: order must be an int array [K, n_order >= 1]")
        T = selfplay.games_per_net
        n = engine.selfplay_ring()[0] * T
        if int(order.min()) < 0 or int(order.max()) >= n:
            raise ValueError(f"PopulationTrainer.train_epoch_ring: order names rows outside the ring's {n} stored rows per net")
        ptr, _, row_len = engine.selfplay_rows_device()
        state_dim, A = engine.s_obs, engine.kmax
        if row_len != state_dim + 3 * A + 1:
            raise ValueError("PopulationTrainer.train_epoch_ring: unexpected replay row length")
        where = _capi.epoch_rows(ptr, state_dim, A, n, ring_trees=selfplay.n_games, games_per_net=T)
        w_ptr = None
        if isinstance(weights, str):
            w_ptr = engine.selfplay_is_weights_device()
        elif weights is not None:
            _check_device_tensor("train_epoch_ring", "weights", weights, self.device, (int(selfplay.capacity), int(selfplay.n_games)),
                                 "[capacity_steps, n_games]")
            w_ptr = weights.data_ptr()
        e_ptr = engine.selfplay_errors_device() if errors else None
        engine.sync()
        return self._epoch("train_epoch_ring", where, order.astype(np.int32), batch_size, w_ptr, e_ptr)

    def train_online_ring(self, selfplay, n_minibatches: int, batch_size: int = 32, return_drawn: bool = False):
        """Prioritised replay as published, in one native call (``azg_trainer_epoch_online``): ``n_minibatches`` minibatches of
        ``batch_size`` rows per net over the self-play engine's ring, each one drawn from priorities refreshed with the value errors
        of the minibatches before it, weighted by the importance-sampling weights of its rows, and writing its own errors back.
        Bit for bit the loop, per minibatch, of ``selfplay.priorities()``, ``selfplay.sample_order(batch_size)``,
        ``selfplay.is_weights()`` and ``train_epoch_ring(selfplay, order, batch_size, weights="priority", errors=True)`` -- with
        3 launches (5 with feedback "max") in front of each step instead of 10, and one synchronisation for the whole call.

        Needs ``losses="device"`` and a self-play object built with ``prioritized={..., "feedback": ...}``; ``alpha``, ``eps``, the
        feedback mode and ``beta`` (absent: 0) are its.  Takes ``n_minibatches`` sample indices of the self-play object's counter
        and as many optimiser (and alpha) steps.  Afterwards the engine's full weight array counts as not computed.  Returns the
        per-net loss sums like ``train_epoch``; with ``return_drawn`` also the rows drawn, int32 [n_minibatches, K, batch_size]."""
        _need_device_losses(self.losses, "train_online_ring")
        prio = getattr(selfplay, "prioritized", None) or {}
        if "feedback" not in prio:
            raise ValueError('PopulationTrainer.train_online_ring needs a self-play engine built with prioritized={..., "feedback": ...}')
        M, B = int(n_minibatches), int(batch_size)
        if M < 1 or not 1 <= B <= self.max_batch:
            raise ValueError(f"PopulationTrainer.train_online_ring: needs n_minibatches >= 1 and a batch_size of 1..{self.max_batch}")
        _check_selfplay("train_online_ring", selfplay, self.device, len(self.agents))
        head = (selfplay.engine, self.flat.data_ptr(), M, B, selfplay._sample_index, prio.get("beta", 0.0),
                _capi.trained_priority_config(prio["alpha"], prio["eps"], prio["feedback"]))
        drawn, out = self._call("epoch", "online", head, steps=M, return_drawn=return_drawn)
        selfplay._sample_index += M
        return (out, drawn) if return_drawn else out

    def export_alpha(self) -> None:
        """Write every net's learned temperature and its Adam state (step, exp_avg, exp_avg_sq) back into its agent's loss object,
        so that ``agent.update`` or a checkpoint of ``agent.loss`` continues from where the trainer stands.  ``close()`` does this;
        between ``update`` calls the agents' own ``loss.log_alpha`` / ``loss.alpha`` are stale until it is called.  With Adam under
        ``optimizers="agents"`` it also writes the trainer's step count into every ``optimizer.state[p]["step"]``."""
        if self.exp_avg is not None:
            for a in self.agents:
                for p in a.nn.parameters():
                    a.optimizer.state[p]["step"].fill_(float(self.opt_step))
        if self.log_alpha is None:
            return
        if self.alpha_optimizer is None:   # losses="device": the trainer's own tensors
            state = {"step": float(self.alpha_step), "exp_avg": self.alpha_exp_avg, "exp_avg_sq": self.alpha_exp_avg_sq} if self.alpha_step else {}
        else:
            state = self.alpha_optimizer.state.get(self.log_alpha, {})
        with torch.no_grad():
            for k, a in enumerate(self.agents):
                la = a.loss.log_alpha
                la.data.copy_(self.log_alpha[k])
                with torch.enable_grad():   # (the loss object's next _update_alpha differentiates alpha by log_alpha)
                    a.loss.alpha = la.exp()
                if state:
                    a.loss.optimizer.state[la] = {"step": torch.tensor(float(state["step"])),
                                                  "exp_avg": state["exp_avg"][k].detach().to(la.device).clone(),
                                                  "exp_avg_sq": state["exp_avg_sq"][k].detach().to(la.device).clone()}

    def close(self) -> None:
        """Hand the learned temperatures and Adam's step count back to the agents (``export_alpha``) and free the native trainer.
        The parameters and the optimiser state need no hand-back: the agents' modules and optimisers are views of ``flat`` /
        ``square_avg`` (or ``exp_avg`` / ``exp_avg_sq``)."""
        if self.trainer._h:
            self.export_alpha()
            if self.ema is not None and self.ema_decay is not None:   # (the tensor outlives the native trainer's pointer to it)
                self.trainer.set_ema(None)
                self.ema_decay = None
        self.trainer.close()
