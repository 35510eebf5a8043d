"""CPU: the host half of the population trainer's device losses -- the ``losses=`` keyword of PopulationTrainer and
``_capi.loss_cfg``.  The kernel is tested on the GPU in test_population_device_loss.py."""
import ctypes as C
import re

import pytest
import torch

from alphazero_gym_amd import _capi
from alphazero_gym_amd.agent.losses import A0CLoss, A0CLossTuned, AlphaZeroLoss
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from alphazero_gym_amd.network.policies import make_policy
from trainer_util import make_agent, refused


@pytest.mark.parametrize("value", ["hip", "", None, "Device"])
def test_unknown_losses_value(value):
    refused([make_agent("normal") for _ in range(2)], "losses must be 'torch' or 'device'", losses=value)
    # the check comes first: agents that would be refused for another reason are not looked at
    with pytest.raises(ValueError, match=re.escape("losses must be 'torch' or 'device'")):
        PopulationTrainer([], losses=value)


@pytest.mark.parametrize("losses", ["torch", "device"])
def test_cpu_agents_still_refused(losses):
    refused([make_agent("gmm2") for _ in range(2)], "must live on one GPU", losses=losses)


def _policy(head):
    if head == "discrete":
        return make_policy(4, 1, "discrete", [16], "relu", num_actions=3)
    return make_policy(3, 1, "normal", [16], "elu", num_components={"normal": 1, "gmm": 4}[head], action_bound=2.0)


HEAD = {"discrete": _capi.HEAD_DISCRETE, "normal": _capi.HEAD_NORMAL, "gmm": _capi.HEAD_GMM}


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head", ["discrete", "normal", "gmm"])
def test_loss_cfg(head, reduction):
    policy = _policy(head)
    bound = 0.0 if head == "discrete" else 2.0
    az = AlphaZeroLoss(policy_coeff=1.5, value_coeff=0.5, reduction=reduction)
    if head == "discrete":
        c = _capi.loss_cfg(policy, az)
        assert (c.struct_size, c.kind, c.head, c.reduction) == (C.sizeof(_capi.AzgLossCfg), _capi.LOSS_ALPHAZERO, HEAD[head], _capi.REDUCE[reduction])
        assert (c.policy_coeff, c.value_coeff, c.action_bound) == (1.5, 0.5, 0.0)
    else:
        with pytest.raises(ValueError, match="AlphaZeroLoss needs a discrete policy"):
            _capi.loss_cfg(policy, az)
    c = _capi.loss_cfg(policy, A0CLoss(tau=0.25, policy_coeff=0.1, alpha=0.05, value_coeff=2.0, reduction=reduction))
    assert (c.kind, c.head, c.reduction) == (_capi.LOSS_A0C, HEAD[head], _capi.REDUCE[reduction])
    assert (c.tau, c.policy_coeff, c.alpha, c.value_coeff, c.action_bound) == (0.25, 0.1, 0.05, 2.0, bound)
    tuned = A0CLossTuned(action_dim=1, alpha_init=1.0, lr=3e-4, tau=0.5, policy_coeff=0.2, value_coeff=1.0, reduction=reduction,
                         grad_clip=0.5, device="cpu")
    c = _capi.loss_cfg(policy, tuned)
    assert (c.kind, c.head, c.reduction) == (_capi.LOSS_A0C_TUNED, HEAD[head], _capi.REDUCE[reduction])
    assert (c.tau, c.policy_coeff, c.value_coeff, c.target_entropy, c.action_bound) == (0.5, 0.2, 1.0, -1.0, bound)
    assert (c.alpha_lr, c.alpha_beta1, c.alpha_beta2, c.alpha_eps, c.alpha_weight_decay, c.alpha_clip) == (3e-4, 0.9, 0.999, 1e-8, 0.0, 0.5)
    assert _capi.LOSS_KEYS == ("loss", "policy_loss", "value_loss", "entropy_loss", "alpha_loss")


def test_loss_cfg_refuses():
    policy = _policy("normal")
    with pytest.raises(ValueError, match="reduction"):
        _capi.loss_cfg(policy, A0CLoss(tau=0.1, policy_coeff=0.1, alpha=0.05, value_coeff=1.0, reduction="none"))
    with pytest.raises(ValueError, match="not supported"):
        _capi.loss_cfg(policy, torch.nn.MSELoss())
    six = make_policy(3, 1, "normal", [16], "elu", num_components=6, action_bound=2.0)
    with pytest.raises(ValueError, match="5 mixture components"):
        _capi.loss_cfg(six, A0CLoss(tau=0.1, policy_coeff=0.1, alpha=0.05, value_coeff=1.0, reduction="mean"))
