"""CPU: the host half of training wide nets in the population trainer -- the azg_trainer_create_wide declaration and binding,
_capi.Trainer(wide=True)'s choice of constructor, and what PopulationTrainer(wide=True) takes and still refuses (the CPU refusal,
which comes last, is what is left for the nets it takes).  The kernels are tested on the GPU in test_population_trainer_wide.py."""
import functools
import os
import re

import pytest

from alphazero_gym_amd import _capi
from trainer_util import normal_agent, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


make_agent = functools.partial(normal_agent, layernorm=False)   # [512, 272]


def test_header_declares_create_wide():
    with open(os.path.join(ROOT, "include", "azgym_train.h")) as fh:
        header = fh.read()
    assert re.search(r"int azg_trainer_create_wide\(int32_t device_id, const azg_mlp_desc\* desc, int32_t n_nets, int32_t max_batch,\s*"
                     r"azg_trainer\*\* out\);", header)


def test_binding_and_library_have_create_wide():
    assert "trainer_create_wide" in _capi.OPTIONAL_SYMBOLS
    from alphazero_gym_amd import _native
    assert "trainer_create_wide" in _native.fns()


def test_trainer_chooses_the_constructor():
    calls = {"create": 0, "create_ex": 0, "create_wide": 0}

    def counted(name):
        def fn(*a):
            calls[name] += 1
            return _capi.AZG_E_UNSUPPORTED
        return fn

    desc = _capi.make_desc(4, [512], 2, "relu")
    old = {"trainer_create": counted("create"), "trainer_create_ex": counted("create_ex"), "trainer_last_error": lambda h: b"no"}
    # a library without the symbol: wide=True names what is missing and makes no native call
    with pytest.raises(NotImplementedError, match=re.escape("this engine library has no azg_trainer_create_wide")):
        _capi.Trainer(old, desc, 1, 16, wide=True)
    assert calls == {"create": 0, "create_ex": 0, "create_wide": 0}
    new = dict(old, trainer_create_wide=counted("create_wide"))
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, wide=True)
    assert calls == {"create": 0, "create_ex": 0, "create_wide": 1}
    # wide=False goes where it goes today
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16)
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, wide=False)
    assert calls == {"create": 2, "create_ex": 0, "create_wide": 1}
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, layernorm=True)
    assert calls == {"create": 2, "create_ex": 1, "create_wide": 1}
    with pytest.raises(ValueError, match="LayerNorm"):
        _capi.Trainer(new, desc, 1, 16, layernorm=True, wide=True)
    assert calls == {"create": 2, "create_ex": 1, "create_wide": 1}


def test_default_refuses_wide_nets():
    refused([make_agent(s) for s in range(2)], "supported nets have 1-3 hidden layers of widths 16, 32, ... 256")
    refused([make_agent(s) for s in range(2)], "supported nets have 1-3 hidden layers of widths 16, 32, ... 256", wide=False)


def test_wide_agents_reach_the_last_refusal():
    refused([make_agent(s) for s in range(2)], "must live on one GPU", wide=True)
    refused([make_agent(0, hidden=[1024] * 2)], "must live on one GPU", wide=True)
    refused([make_agent(0, hidden=[16] * 8)], "must live on one GPU", wide=True)
    # narrow agents are taken by such a trainer as well
    refused([make_agent(s, hidden=(32, 32)) for s in range(2)], "must live on one GPU", wide=True)


@pytest.mark.parametrize("hidden", [[16] * 9, [1040], [40], [512, 40]], ids=["9_layers", "1040", "40", "512x40"])
def test_shapes_that_stay_refused(hidden):
    refused([make_agent(0, hidden=hidden)], "supported nets have 1-8 hidden layers of widths 16, 32, ... 1024", wide=True)


def test_wide_refuses_layernorm():
    refused([make_agent(s, hidden=(32, 32), layernorm=True) for s in range(2)], "LayerNorm", wide=True)
    refused([make_agent(s, hidden=(32, 32), layernorm=True) for s in range(2)], "LayerNorm", wide=True, layernorm=True)
    refused([make_agent(s, hidden=(32, 32)) for s in range(2)], "LayerNorm", wide=True, layernorm=True)
    refused([make_agent(s) for s in range(2)], "LayerNorm", wide=True, layernorm=True)
