"""CPU: the host half of training LayerNorm trunks in the population trainer -- PopulationTrainer(layernorm=True) no longer refuses
LayerNorm agents (the CPU refusal, which comes last, is what is left), what it still refuses, and the azg_trainer_create_ex binding.
The kernels are tested on the GPU in test_population_trainer_layernorm.py."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

from alphazero_gym_amd import _capi, run
from alphazero_gym_amd.agent.agents import ContinuousAgent
from alphazero_gym_amd.agent.population_trainer import PopulationTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = dict(_target_="torch.optim.Adam", lr=1e-3)


def make_agent(seed=0, hidden=(32, 32), layernorm=True, optimizer=None, grad_clip=0):
    torch.manual_seed(seed)
    cfg = run.CONTINUOUS_DEFAULTS
    policy = dict(cfg["policy"], hidden_dimensions=list(hidden), representation_dim=3, action_dim=1, action_bound=2.0, layernorm=layernorm,
                  num_components=1)
    return ContinuousAgent(policy_cfg=policy, mcts_cfg=dict(cfg["mcts"], device="cpu"), loss_cfg=run.LOSS_TUNED,
                           optimizer_cfg=optimizer or run.RMSPROP, device="cpu", **dict(cfg["agent"], grad_clip=grad_clip))


def _refused(agents, reason, **kw):
    """PopulationTrainer(agents, **kw) raises a ValueError naming ``reason`` and leaves the agents as they were: same values, same
    storage, no optimiser state."""
    before = copy.deepcopy([a.nn.state_dict() for a in agents])
    ptrs = [[p.data_ptr() for p in a.nn.parameters()] for a in agents]
    with pytest.raises(ValueError, match=re.escape(reason)):
        PopulationTrainer(agents, **kw)
    for a, sd, pp in zip(agents, before, ptrs):
        for name, v in a.nn.state_dict().items():
            assert torch.equal(v, sd[name])
        assert [p.data_ptr() for p in a.nn.parameters()] == pp and not a.optimizer.state


@pytest.mark.parametrize("form", ["rmsprop", "agents_adam_clip"])
def test_layernorm_agents_reach_the_last_refusal(form):
    """With layernorm=True the LayerNorm refusal is gone: CPU agents get as far as "must live on one GPU", which comes last."""
    if form == "rmsprop":
        agents, kw = [make_agent(s) for s in range(2)], {}
    else:
        agents, kw = [make_agent(s, optimizer=ADAM, grad_clip=0.5) for s in range(2)], dict(optimizers="agents")
    _refused(agents, "must live on one GPU", layernorm=True, **kw)
    # plain agents are taken by such a trainer as well
    plain = [make_agent(s, layernorm=False) for s in range(2)]
    _refused(plain, "must live on one GPU", layernorm=True, **kw)


def test_default_still_refuses_layernorm():
    _refused([make_agent(s) for s in range(2)], "LayerNorm")
    _refused([make_agent(s) for s in range(2)], "LayerNorm", layernorm=False)


def test_mixed_layernorm_and_plain_is_another_shape():
    _refused([make_agent(0), make_agent(1, layernorm=False)], "same network shape", layernorm=True)


@pytest.mark.parametrize("kw", [dict(eps=1e-3), dict(elementwise_affine=False)], ids=["eps", "no_affine"])
def test_other_layernorms_stay_refused(kw):
    agents = [make_agent(s) for s in range(2)]
    for a in agents:
        for i, mod in enumerate(a.nn.trunk):
            if isinstance(mod, torch.nn.LayerNorm):
                a.nn.trunk[i] = torch.nn.LayerNorm(mod.normalized_shape, **kw)
    with pytest.raises(NotImplementedError, match="LayerNorm must use eps=1e-5 and elementwise_affine=True"):
        _capi.policy_tensors(agents[0].nn)
    with pytest.raises(NotImplementedError, match="LayerNorm must use eps=1e-5 and elementwise_affine=True"):
        PopulationTrainer(agents, layernorm=True)


def test_header_and_binding():
    with open(os.path.join(ROOT, "include", "azgym_train.h")) as fh:
        header = fh.read()
    assert re.search(r"typedef struct azg_trainer_options \{\s*int32_t struct_size;\s*int32_t layernorm;\s*\} azg_trainer_options;", header)
    assert re.search(r"int azg_trainer_create_ex\(int32_t device_id, const azg_mlp_desc\* desc, int32_t n_nets, int32_t max_batch,\s*"
                     r"const azg_trainer_options\* opts,\s*azg_trainer\*\* out\);", header)
    assert "trainer_create_ex" in _capi.OPTIONAL_SYMBOLS
    assert [n for n, _ in _capi.AzgTrainerOptions._fields_] == ["struct_size", "layernorm"] and C.sizeof(_capi.AzgTrainerOptions) == 8

    # a library with the first trainer entry points only: the default path goes on, layernorm=True names what is missing
    calls = []

    def create(*a):
        calls.append(a)
        return _capi.AZG_E_UNSUPPORTED

    old = {"trainer_create": create, "trainer_last_error": lambda h: b"no"}
    desc = _capi.make_desc(4, [32], 2, "relu", layernorm=True)
    with pytest.raises(NotImplementedError, match=re.escape("this engine library has no azg_trainer_create_ex")):
        _capi.Trainer(old, desc, 1, 16, layernorm=True)
    assert not calls
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(old, desc, 1, 16)
    assert len(calls) == 1
    # ... and with it: layernorm=True calls create_ex with a filled azg_trainer_options, the default calls azg_trainer_create
    seen = []

    def create_ex(dev, d, n, b, opts, out):
        o = C.cast(opts, C.POINTER(_capi.AzgTrainerOptions)).contents
        seen.append((o.struct_size, o.layernorm))
        return _capi.AZG_E_UNSUPPORTED

    new = dict(old, trainer_create_ex=create_ex)
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, layernorm=True)
    assert seen == [(8, 1)] and len(calls) == 1
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, layernorm=False)
    assert len(seen) == 1 and len(calls) == 2


def test_native_library_exports_create_ex():
    from alphazero_gym_amd import _native
    assert "trainer_create_ex" in _native.fns()
