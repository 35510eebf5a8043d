"""Importance-sampling weights of the prioritised replay ring (azg_selfplay_is_weights, include/azgym_priority.h) and the weighted
losses (include/azgym_train_weighted.h): the numpy truth of the weight rule on top of priority_util and the oracle's azg_logf /
azg_expf (oracle_lib.math_eval fn 3, then fn 0), and what the weighted-loss tests share on top of device_loss_util.  TEST
INFRASTRUCTURE ONLY.  Importing it needs neither a GPU nor the native library."""
import numpy as np
import torch

import oracle_lib as O
from alphazero_gym_amd.agent.population_trainer import population_loss
from trainer_util import DEV

BETAS = (0.0, 0.4, 1.0)


def weight_rule(q, q_min, beta):
    """w = (q_min / q)^beta by the header's rule: 1.0f where beta == 0 or q == q_min; else r = (float)((double)q_min / (double)q),
    w = azg_expf(beta * azg_logf(r)), every step rounded to float32 on its own."""
    q = np.asarray(q, np.uint64)
    w = np.ones(q.shape, np.float32)
    beta = np.float32(beta)
    if beta == 0:
        return w
    m = q != np.uint64(q_min)
    if not m.any():
        return w
    r = (np.float64(int(q_min)) / q[m].astype(np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        log = O.math_eval(3, r).astype(np.float32)
        prod = (beta * log).astype(np.float32)
        w[m] = O.math_eval(0, prod).astype(np.float32)
    return w


def is_weights(q, n_nets, beta):
    """azg_selfplay_is_weights: q [size_steps, n_trees] uint64 -> float32 [size_steps, n_trees]; q_min per net over the net's T game
    columns of the stored slots."""
    q = np.asarray(q, np.uint64)
    T = q.shape[1] // n_nets
    out = np.empty(q.shape, np.float32)
    for k in range(n_nets):
        block = q[:, k * T:(k + 1) * T]
        out[:, k * T:(k + 1) * T] = weight_rule(block, block.min(), beta)
    return out


def bits(w):
    return np.ascontiguousarray(w, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ weighted losses

def make_weights(K, B, seed):
    """[K, B] float32 on the CPU: uniform in (0, 1], with some rows exactly 0 and some exactly 1 (B >= 4: at least one of each per
    net)."""
    g = torch.Generator().manual_seed(seed)
    w = 1.0 - torch.rand((K, B), generator=g)
    kind = torch.rand((K, B), generator=g)
    w[kind < 0.15] = 0.0
    w[kind > 0.85] = 1.0
    if B >= 4:
        w[:, 1] = 0.0
        w[:, 2] = 1.0
    return w.float()


def torch_loss_weighted(policy, loss, inputs, weights, dtype, log_alpha=None, alpha_optimizer=None):
    """population_loss(weights=) on the CPU in ``dtype``: ({key: [K]}, raw.grad)."""
    raw, actions, counts, values = (x.detach().to(dtype) for x in inputs)
    raw = raw.clone().requires_grad_(True)
    w = None if weights is None else weights.detach().to(dtype)
    out = population_loss(policy, loss, raw, actions, counts, values.unsqueeze(-1), log_alpha, alpha_optimizer, weights=w)
    out["loss"].sum().backward()
    return {k: v.detach() for k, v in out.items()}, raw.grad


def kernel_loss_weighted(tr, cfg, inputs, weights, state=None, nets=False):
    """azg_trainer_loss_weighted (``nets``: _nets_weighted with ``cfg`` a list): (losses [K, 5], d_raw) on the CPU."""
    raw, actions, counts, values = (x.to(DEV).contiguous() for x in inputs)
    w = weights.to(DEV).contiguous()
    d_raw = torch.full_like(raw, float("nan"))
    losses = torch.full((raw.shape[0], 5), float("nan"), device=DEV)
    torch.cuda.synchronize()
    fn = tr.loss_nets_weighted if nets else tr.loss_weighted
    fn(raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), w.data_ptr(), raw.shape[1], actions.shape[2], cfg, state,
       d_raw.data_ptr(), losses.data_ptr())
    return losses.cpu(), d_raw.cpu()
