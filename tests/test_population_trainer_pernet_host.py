"""CPU: the host half of PopulationTrainer(per_net=True) -- what it accepts (agents that differ in numeric optimiser and loss
settings) and what it still refuses, the *_nets bindings and the example's --lrs.  The kernels are tested on the GPU in
test_population_trainer_pernet.py."""
import ctypes as C
import os
import sys

import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import make_agent, refused

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ADAM = dict(run.ADAM)


def _with(agent, **attrs):
    """The agent with loss attributes changed (tau, policy_coeff, ...)."""
    for key, val in attrs.items():
        assert hasattr(agent.loss, key)
        setattr(agent.loss, key, val)
    return agent


# The agents live on the CPU, which PopulationTrainer refuses last of all: agents refused for that reason passed every other check.
MIXED = {
    "lr_rmsprop": lambda: [make_agent("normal"), make_agent("normal", optimizer=dict(run.RMSPROP, lr=0.01))],
    "lr_betas_adam": lambda: [make_agent("gmm2", optimizer=ADAM), make_agent("gmm2", optimizer=dict(ADAM, lr=3e-4, betas=(0.8, 0.99), eps=1e-6))],
    "weight_decay": lambda: [make_agent("discrete"), make_agent("discrete", optimizer=dict(run.RMSPROP, weight_decay=1e-2))],
    "grad_clip": lambda: [make_agent("normal", optimizer=ADAM, grad_clip=0.0), make_agent("normal", optimizer=ADAM, grad_clip=0.5)],
    "tau": lambda: [make_agent("normal"), _with(make_agent("normal"), tau=0.5)],
    "coefficients": lambda: [make_agent("discrete", loss="alphazero"), _with(make_agent("discrete", loss="alphazero"), policy_coeff=0.7, value_coeff=1.3)],
}


@pytest.mark.parametrize("what", list(MIXED))
def test_mixed_settings_pass_every_host_check(what):
    refused(MIXED[what](), "must live on one GPU", optimizers="agents", losses="device", per_net=True)


@pytest.mark.parametrize("what", ["lr_rmsprop", "lr_betas_adam", "weight_decay", "grad_clip"])
def test_mixed_optimiser_settings_pass_with_torch_losses(what):
    refused(MIXED[what](), "must live on one GPU", optimizers="agents", losses="torch", per_net=True)


def _one_step_ahead():
    """Two Adam agents, the first of which has taken an optimiser step."""
    agents = [make_agent("normal", optimizer=ADAM, seed=s) for s in range(2)]
    for p in agents[0].nn.parameters():
        p.grad = torch.zeros_like(p)
    agents[0].optimizer.step()
    agents[0].optimizer.zero_grad(set_to_none=True)
    return agents


def test_per_net_needs_agents_optimisers():
    refused([make_agent("normal") for _ in range(2)], 'per_net=True requires optimizers="agents"', per_net=True)
    refused([make_agent("normal") for _ in range(2)], 'per_net=True requires optimizers="agents"', optimizers="rmsprop", per_net=True)


PER_NET_REFUSALS = {
    "mixed_class": (lambda: [make_agent("normal", optimizer=ADAM), make_agent("normal")], "same optimiser class", "device"),
    "mixed_loss_class": (lambda: [make_agent("discrete", loss="alphazero"), make_agent("discrete", loss="a0c")],
                         "same loss class and hyper-parameters", "device"),
    "mixed_reduction": (lambda: [make_agent("normal"), _with(make_agent("normal"), reduction="sum")],
                        "same loss class and hyper-parameters", "device"),
    "mixed_tau_torch_losses": (lambda: [make_agent("normal"), _with(make_agent("normal"), tau=0.5)],
                               'same loss class and hyper-parameters (per-net loss settings need losses="device")', "torch"),
    "negative_clip": (lambda: [make_agent("normal", grad_clip=0.0), make_agent("normal", grad_clip=-1.0)], "grad_clip must be >= 0", "device"),
    "momentum": (lambda: [make_agent("normal"), make_agent("normal", optimizer=dict(run.RMSPROP, momentum=0.9))], "momentum", "device"),
    "shape": (lambda: [make_agent("normal"), make_agent("normal", hidden=(32, 16))], "same network shape", "device"),
}


@pytest.mark.parametrize("why", list(PER_NET_REFUSALS))
def test_per_net_refusals(why):
    build, reason, losses = PER_NET_REFUSALS[why]
    refused(build(), reason, optimizers="agents", losses=losses, per_net=True)


def test_per_net_step_counts_must_agree():
    agents = _one_step_ahead()
    with pytest.raises(ValueError, match="same number of steps"):
        PopulationTrainer(agents, optimizers="agents", losses="device", per_net=True)
    assert agents[0].optimizer.state and not agents[1].optimizer.state


DEFAULT_STILL_REFUSES = {
    "lr_rmsprop": ("same RMSprop settings", dict(optimizers="agents")),
    "lr_betas_adam": ("same Adam settings", dict(optimizers="agents")),
    "grad_clip": ("same grad_clip", dict(optimizers="agents")),
    "tau": ("same loss class and hyper-parameters", dict(optimizers="agents", losses="device")),
}


@pytest.mark.parametrize("what", list(DEFAULT_STILL_REFUSES))
def test_default_constructor_keeps_its_messages(what):
    reason, kw = DEFAULT_STILL_REFUSES[what]
    refused(MIXED[what](), reason, **kw)
    refused(MIXED[what](), reason, per_net=False, **kw)
    if what == "lr_rmsprop":
        refused(MIXED[what](), reason)


def test_nets_symbols_and_signatures():
    """The four entry points exist in the built library and are bound with the *_opt calls' prototypes."""
    from alphazero_gym_amd import _native
    lib, f = _native.lib(), _native.fns()
    vp = C.c_void_p
    want = {
        "trainer_backward_step_nets": [vp, vp, vp, C.c_int32, C.POINTER(_capi.AzgOptim), vp],
        "trainer_loss_nets": [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(_capi.AzgLossCfg), C.POINTER(_capi.AzgAlphaState), vp, vp],
        "trainer_step_nets": [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(_capi.AzgLossCfg), C.POINTER(_capi.AzgAlphaState),
                              C.POINTER(_capi.AzgOptim), vp, vp, vp],
        "trainer_epoch_nets": [vp, vp, C.POINTER(_capi.AzgEpochRows), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(_capi.AzgLossCfg),
                               C.POINTER(_capi.AzgAlphaState), C.POINTER(_capi.AzgOptim), vp, C.POINTER(C.c_int32)],
    }
    for name, argtypes in want.items():
        assert hasattr(lib, "azg_" + name), name
        assert name in f and list(f[name].argtypes) == argtypes, name
    for method in ("backward_step_nets", "loss_nets", "step_nets", "epoch_nets"):
        assert callable(getattr(_capi.Trainer, method))
    # an array of entries is what a POINTER(struct) parameter takes
    arr = (_capi.AzgOptim * 3)(*[_capi.optim("adam", 1e-3 * (k + 1), 16, 32) for k in range(3)])
    assert C.sizeof(arr) == 3 * C.sizeof(_capi.AzgOptim) and [arr[k].lr for k in range(3)] == [1e-3, 2e-3, 3e-3]
    assert C.POINTER(_capi.AzgOptim).from_param(arr) is not None


def test_example_lrs():
    import population_selfplay_train as X
    a = X.parse_args(["--seeds", "0", "1", "2", "--lrs", "1e-3", "3e-4", "1e-4"])
    assert a.lrs == [1e-3, 3e-4, 1e-4]
    assert X.parse_args(["--seeds", "0", "1"]).lrs is None
    for bad in (["--seeds", "0", "1", "2", "--lrs", "1e-3"], ["--seeds", "0", "--lrs", "1e-3", "1e-4"]):
        with pytest.raises(SystemExit):
            X.parse_args(bad)
