"""CPU: the host half of training wide LayerNorm nets in the population trainer -- the azg_trainer_create_wide_ex declaration and
binding, _capi.Trainer(wide_layernorm=True)'s choice of constructor, and what PopulationTrainer(wide_layernorm=True) takes and still
refuses (the CPU refusal, which comes last, is what is left for the nets it takes).  The kernels are tested on the GPU in
test_population_trainer_wide_layernorm.py."""
import functools
import os
import re

import pytest

from alphazero_gym_amd import _capi
from trainer_util import normal_agent, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


make_agent = functools.partial(normal_agent, layernorm=True)   # [512, 272]


def test_header_declares_create_wide_ex():
    with open(os.path.join(ROOT, "include", "azgym_train.h")) as fh:
        header = fh.read()
    assert re.search(r"int azg_trainer_create_wide_ex\(int32_t device_id, const azg_mlp_desc\* desc, int32_t n_nets, int32_t max_batch,\s*"
                     r"const azg_trainer_options\* opts,\s*azg_trainer\*\* out\);", header)


def test_binding_and_library_have_create_wide_ex():
    assert "trainer_create_wide_ex" in _capi.OPTIONAL_SYMBOLS
    from alphazero_gym_amd import _native
    f = _native.fns()
    assert "trainer_create_wide_ex" in f
    assert len(f["trainer_create_wide_ex"].argtypes) == 6


def test_trainer_chooses_the_constructor():
    names = ("create", "create_ex", "create_wide", "create_wide_ex")
    calls = dict.fromkeys(names, 0)

    def counted(name):
        def fn(*a):
            calls[name] += 1
            return _capi.AZG_E_UNSUPPORTED
        return fn

    def seen():
        return tuple(calls[n] for n in names)

    desc = _capi.make_desc(4, [512], 2, "relu", layernorm=True)
    old = {"trainer_create": counted("create"), "trainer_create_ex": counted("create_ex"), "trainer_create_wide": counted("create_wide"),
           "trainer_last_error": lambda h: b"no"}
    # a library without the symbol: wide_layernorm=True names what is missing and makes no native call
    with pytest.raises(NotImplementedError, match=re.escape("this engine library has no azg_trainer_create_wide_ex")):
        _capi.Trainer(old, desc, 1, 16, wide_layernorm=True)
    assert seen() == (0, 0, 0, 0)
    new = dict(old, trainer_create_wide_ex=counted("create_wide_ex"))
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(new, desc, 1, 16, wide_layernorm=True)
    assert seen() == (0, 0, 0, 1)
    # two different trainers asked for: no native call
    with pytest.raises(ValueError, match="wide_layernorm"):
        _capi.Trainer(new, desc, 1, 16, wide_layernorm=True, layernorm=True)
    assert seen() == (0, 0, 0, 1)
    # the three spellings of before go where they went
    for kw, want in ((dict(), (1, 0, 0, 1)), (dict(wide_layernorm=False), (2, 0, 0, 1)), (dict(layernorm=True), (2, 1, 0, 1)),
                     (dict(wide=True), (2, 1, 1, 1))):
        with pytest.raises(_capi.EngineError):
            _capi.Trainer(new, desc, 1, 16, **kw)
        assert seen() == want
    with pytest.raises(ValueError, match="LayerNorm"):
        _capi.Trainer(new, desc, 1, 16, layernorm=True, wide=True)
    assert seen() == (2, 1, 1, 1)


def test_the_options_passed_ask_for_layernorm():
    """The one call of create_wide_ex carries an azg_trainer_options of the right size with layernorm = 1."""
    got = {}

    def create_wide_ex(device_id, desc, n_nets, max_batch, opts, out):
        o = opts._obj
        got.update(size=o.struct_size, layernorm=o.layernorm, n_nets=n_nets, max_batch=max_batch)
        return _capi.AZG_E_UNSUPPORTED

    fns = {"trainer_create": None, "trainer_create_wide_ex": create_wide_ex, "trainer_last_error": lambda h: b"no"}
    with pytest.raises(_capi.EngineError):
        _capi.Trainer(fns, _capi.make_desc(4, [512], 2, "relu", layernorm=True), 3, 16, wide_layernorm=True)
    assert got == dict(size=8, layernorm=1, n_nets=3, max_batch=16)


def test_wide_layernorm_agents_reach_the_last_refusal():
    refused([make_agent(s) for s in range(2)], "must live on one GPU", wide_layernorm=True)
    refused([make_agent(0, hidden=[1024] * 2)], "must live on one GPU", wide_layernorm=True)
    # agents without LayerNorm, and narrow ones, are taken as well
    refused([make_agent(s, layernorm=False) for s in range(2)], "must live on one GPU", wide_layernorm=True)
    refused([make_agent(s, hidden=(32, 32)) for s in range(2)], "must live on one GPU", wide_layernorm=True)


@pytest.mark.parametrize("hidden", [[16] * 9, [1040], [40], [512, 40]], ids=["9_layers", "1040", "40", "512x40"])
def test_shapes_that_stay_refused(hidden):
    refused([make_agent(0, hidden=hidden)], "supported nets have 1-8 hidden layers of widths 16, 32, ... 1024", wide_layernorm=True)


def test_two_trainers_at_once_are_refused():
    refused([make_agent(s, hidden=(32, 32)) for s in range(2)], "wide_layernorm=True and layernorm=True", wide_layernorm=True, layernorm=True)


def test_the_spellings_of_before_keep_their_refusals():
    refused([make_agent(s) for s in range(2)], "LayerNorm", wide=True)
    refused([make_agent(s) for s in range(2)], "LayerNorm", wide=True, layernorm=True)
    refused([make_agent(s) for s in range(2)], "LayerNorm")
    refused([make_agent(s) for s in range(2)], "supported nets have 1-3 hidden layers of widths 16, 32, ... 256", layernorm=True)
