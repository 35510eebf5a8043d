"""CPU: the host half of PopulationTrainer(optimizers="agents") -- what it accepts (Adam, gradient clipping) and what it still
refuses, the azg_optim binding and the example's flags.  The kernels are tested on the GPU in test_population_trainer_optim.py."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
from trainer_util import make_agent, make_batch, refused

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ADAM = dict(run.ADAM)


# The agents live on the CPU, which PopulationTrainer refuses last of all: agents refused for that reason passed every other check.
ACCEPTED = {
    "adam": lambda: [make_agent("normal", optimizer=ADAM, seed=s) for s in range(2)],
    "adam_clip": lambda: [make_agent("gmm2", optimizer=ADAM, grad_clip=0.5, seed=s) for s in range(2)],
    "rmsprop_clip": lambda: [make_agent("normal", grad_clip=1.0, seed=s) for s in range(2)],
    "rmsprop": lambda: [make_agent("discrete", seed=s) for s in range(2)],
}


@pytest.mark.parametrize("what", list(ACCEPTED))
def test_agents_optimisers_pass_every_host_check(what):
    refused(ACCEPTED[what](), "must live on one GPU", optimizers="agents")


REFUSALS = {
    "amsgrad": (lambda: [make_agent("normal", optimizer=dict(ADAM, amsgrad=True)) for _ in range(2)], "amsgrad"),
    "maximize": (lambda: [make_agent("normal", optimizer=dict(ADAM, maximize=True)) for _ in range(2)], "maximize"),
    "mixed_betas": (lambda: [make_agent("normal", optimizer=ADAM), make_agent("normal", optimizer=dict(ADAM, betas=(0.9, 0.999)))],
                    "same Adam settings"),
    "mixed_grad_clip": (lambda: [make_agent("normal", optimizer=ADAM, grad_clip=1.0), make_agent("normal", optimizer=ADAM, grad_clip=2.0)],
                        "same grad_clip"),
    "mixed_class": (lambda: [make_agent("normal", optimizer=ADAM), make_agent("normal")], "same optimiser class"),
    "momentum": (lambda: [make_agent("normal", optimizer=dict(run.RMSPROP, momentum=0.9)) for _ in range(2)], "momentum"),
    "sgd": (lambda: [make_agent("normal", optimizer=dict(_target_="torch.optim.SGD", lr=1e-3)) for _ in range(2)],
            "torch.optim.RMSprop or torch.optim.Adam, not SGD"),
    "layernorm": (lambda: [make_agent("normal", optimizer=ADAM, layernorm=True) for _ in range(2)], "LayerNorm"),
    "mixed_lr": (lambda: [make_agent("normal"), make_agent("normal", optimizer=dict(run.RMSPROP, lr=0.01))], "same RMSprop settings"),
}


@pytest.mark.parametrize("why", list(REFUSALS))
def test_agents_optimisers_refusals(why):
    build, reason = REFUSALS[why]
    refused(build(), reason, optimizers="agents")


def test_bad_optimizers_value():
    refused([make_agent("normal") for _ in range(2)], "optimizers must be 'rmsprop' or 'agents'", optimizers="adam")


def test_adam_step_counts_must_agree():
    """One agent has taken an Adam step, the other has not: refused, and the optimiser state that was there stays."""
    agents = [make_agent("normal", optimizer=ADAM, seed=s) for s in range(2)]
    states, actions, counts, values = make_batch("normal", 3)
    agents[0].update((states, actions, counts, None, values))
    before = copy.deepcopy([a.nn.state_dict() for a in agents])
    with pytest.raises(ValueError, match="same number of steps"):
        PopulationTrainer(agents, optimizers="agents")
    for a, sd in zip(agents, before):
        for name, v in a.nn.state_dict().items():
            assert torch.equal(v, sd[name])
    assert len(agents[0].optimizer.state) == len(list(agents[0].nn.parameters())) and not agents[1].optimizer.state


def test_default_keeps_its_refusals():
    """optimizers="rmsprop" is the default and says what it always said."""
    refused([make_agent("normal", optimizer=dict(_target_="torch.optim.Adam", lr=1e-3)) for _ in range(2)],
             "must be torch.optim.RMSprop, not Adam", optimizers="rmsprop")
    refused([make_agent("normal", grad_clip=1.0) for _ in range(2)],
             "grad_clip != 0 is not supported (a per-net global norm needs a pass of its own)")


def test_capi_optim_fills_every_field():
    o = _capi.optim("adam", 2e-3, 0x1000, 0x2000, eps=1e-7, weight_decay=1e-4, betas=(0.8, 0.95), grad_clip=0.5, step=7, grad_norms=0x3000)
    assert o.struct_size == C.sizeof(_capi.AzgOptim) and o.kind == _capi.OPT_ADAM == 1
    assert (o.lr, o.eps, o.weight_decay, o.beta1, o.beta2, o.grad_clip, o.step) == (2e-3, 1e-7, 1e-4, 0.8, 0.95, 0.5, 7)
    assert (o.state0, o.state1, o.grad_norms) == (0x1000, 0x2000, 0x3000)
    r = _capi.optim("rmsprop", 1e-3, 0x1000, alpha=0.9, eps=1e-10)
    assert r.struct_size == C.sizeof(_capi.AzgOptim) and r.kind == _capi.OPT_RMSPROP == 0
    assert (r.lr, r.alpha, r.eps, r.weight_decay, r.grad_clip, r.step) == (1e-3, 0.9, 1e-10, 0.0, 0.0, 0)
    assert (r.state0, r.state1, r.grad_norms) == (0x1000, None, None)
    names = {n for n, _ in _capi.AzgOptim._fields_}
    assert names == {"struct_size", "kind", "lr", "eps", "weight_decay", "alpha", "beta1", "beta2", "grad_clip", "step", "state0", "state1",
                     "grad_norms"}


def test_example_flags():
    import population_selfplay_train as X
    import selfplay_train as S
    a = X.parse_args([])
    assert a.optimizer == "rmsprop" and a.grad_clip == 0.0
    a = X.parse_args(["--optimizer", "adam", "--grad-clip", "1.0"])
    assert a.optimizer == "adam" and a.grad_clip == 1.0
    with pytest.raises(SystemExit):
        X.parse_args(["--optimizer", "sgd"])
    b = S.parse_args(["--optimizer", "adam", "--grad-clip", "0.5"])
    assert b.optimizer == "adam" and b.grad_clip == 0.5
    agent, _ = S.build_agent("Pendulum-v1", [32, 32], 8, "cpu", 1e-3, "adam", 0.5)
    g = agent.optimizer.param_groups[0]
    assert type(agent.optimizer) is torch.optim.Adam and tuple(g["betas"]) == (0.9, 0.99) and g["eps"] == 1e-7 and not g["amsgrad"]
    assert agent.clip == 0.5
    agent, _ = S.build_agent("CartPole-v0", [32, 32], 8, "cpu", 1e-3)
    assert type(agent.optimizer) is torch.optim.RMSprop and agent.clip == 0
