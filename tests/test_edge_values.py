"""GPU (-m gpu): the HIP search against the CPU oracle at the edges of the value range, bit for bit, and the device-only
restatements (act4, tree_div) against their plain counterparts.

Every other parity test draws its networks from synthetic.make_weights: values, pre-activations and logits of a few units.  Here the
networks are built by hand (tests/edge_values.py) so that every node's V sits on a chosen float32 -- on and beside the thresholds of
backup_path's closed form (csrc/tree.cuh), on values where closed form and serial chain differ (edge_values.TEETH), at float32 max,
in the subnormals -- with paths deep enough (<= 15, == 16, >= 17, CartPole >= 33 levels) that the lanes' 16 levels, the hand-over to
backup_from and its second round all run; and so that the policy heads sit at their limits (log sigma beyond both clamps, a
saturated squash, a mixture share that rounds to 1).  What each case contains is asserted on the oracle's run alone in
tests/test_backup_closed_form.py (CPU); here the device must reproduce that run."""
import numpy as np
import pytest

import edge_values as E
import oracle_lib as O
import parity_util as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from alphazero_gym_amd import _native
    _native.lib()
    return _native


def _force(monkeypatch, variant):
    if variant != "default":
        monkeypatch.setenv(*P.VARIANT_ENV[variant])
    if variant == "no_spec":
        monkeypatch.setenv(*P.VARIANT_ENV["tile16"])            # (the specialised kernels exist for full tiles only)


@pytest.mark.parametrize("env,V,setup,variant", [pytest.param(*c[1:], id=c[0]) for c in E.discrete_device_cases()])
def test_discrete_edge_value_bit_exact_vs_oracle(native, env, V, setup, variant, monkeypatch):
    """A constant-value net with V on / beside / beyond the closed form's range, gamma 1 (setup gamma097: the control), 37 trees:
    every result and every record identical to the oracle's.  Terminal leaves (V = 0) sit beside the others, so one wave takes
    both arms of the range test in the same step."""
    opts = E.DISCRETE_SETUPS[setup]
    want = E.oracle_discrete(env, V, **opts)
    kw, desc, blob, roots, carry = E.discrete_case(env, V, **opts)
    _force(monkeypatch, variant)
    got = E.run_engine(native.HipEngine, kw, desc, blob, roots, carry)
    info = got["info"]
    E.assert_same(got, want)
    if variant == "global_tree":
        assert info["tree_storage"] == "global", info
    if setup == "sims200":
        assert info["tree_storage"] == "lds9", info              # 403 records: 9-bit ids
    if setup == "base" and env == "cartpole" and variant in ("tile16", "no_spec"):
        assert (info["tile_trees"], info["spec"]) == (16, 1 if variant == "tile16" else 0), info
    if setup == "wide512":
        assert info["kernel_form"] == "persistent" and "<" in info["kernel_name"] and " 512, 0," in info["kernel_name"], info
        assert info["tree_storage"] == ("global" if variant == "global_tree" else "lds8"), info


@pytest.mark.parametrize("env", sorted(E.ENV))
def test_population_of_edge_values_in_one_launch(native, env):
    """Three nets -- V in range, below 2^-25, at or above 2^30 -- in one launch: lanes of one workgroup take different arms for
    different nets.  Identical to three single-net oracle engines."""
    kw, desc, blobs, roots, carry = E.population_case(env)
    got = E.run_engine(native.HipEngine, kw, desc, blobs, roots, carry)
    E.assert_same(got, E.concat_runs(E.oracle_population(env)))


CONT_VARIANTS = {"pendulum256": ["default", "waves4", "global_tree", "no_spec"], "mcc64": ["default"], "gmm128": ["default"]}


@pytest.mark.parametrize("shape,setting,variant", [(s, st, v) for s in E.CONT_SHAPES for st in E.cont_settings(s) for v in CONT_VARIANTS[s]])
def test_continuous_edge_value_bit_exact_vs_oracle(native, shape, setting, variant, monkeypatch):
    """Continuous search with the value / policy heads at their limits (edge_values.continuous_case): a subnormal first-level
    product, float32 max, a -0.0 bias, log sigma beyond both clamps, mu so large that every action is +-bound, a mixture share of 1."""
    kw, desc, blob, roots = E.continuous_case(shape, setting)
    want = E.oracle_continuous(shape, setting)
    _force(monkeypatch, variant)
    got = E.run_engine(native.HipEngine, kw, desc, blob, roots, None)
    info = got["info"]
    E.assert_same(got, want)
    if shape == "pendulum256":
        assert info["waves"] == (4 if variant in ("waves4", "global_tree") else 8), info
        assert info["tree_storage"] == ("global" if variant == "global_tree" else "lds8"), info
        assert info["spec"] == (0 if variant in ("no_spec", "global_tree") else 1), info


# ------------------------------------------------------------------------------------------------ device-only restatements

def _elu_inputs():
    sub = float(np.finfo(np.float32).smallest_subnormal)
    near = np.array([-87.0], np.float32)
    for _ in range(8):
        near = np.concatenate([np.nextafter(near[:1], np.float32(-np.inf)), near, np.nextafter(near[-1:], np.float32(0))])
    x = np.concatenate([[0.0, -0.0, sub, -sub, -1e-38, -1e-30, -1e-7, -1e10, float(E.F32_MAX), -float(E.F32_MAX), -87.0, -88.0, -86.0],
                        near.astype(np.float64), np.linspace(-88, -86, 4001), np.linspace(-90, 10, 20001)])
    x = x.astype(np.float32).astype(np.float64)
    return np.repeat(x, 4)            # each input in each of the four vector components in turn (component = index & 3)


@pytest.mark.parametrize("fn_id", [13, 14], ids=["elu", "relu"])
def test_act4_is_bit_identical_to_the_scalar_activation(native, fn_id):
    """act4<false> (csrc/mlp.cuh: inline v_max_f32, an fmed3 clamp to [-87, 0], 2^k by an integer shift-add) against azg_activation /
    `x > 0 ? x : 0` on the host, in each component: +-0, +-the smallest subnormal, tiny and huge negatives, -87 with its float32
    neighbours, [-88, -86] densely, [-90, 10].  Finite inputs only: azg_expm1f is specified for finite x, so NaN is not an input."""
    x = _elu_inputs()
    assert np.isfinite(x).all() and (x == -87.0).any() and x.size % 4 == 0
    host = O.math_eval(fn_id, x)
    dev = native.math_selftest(fn_id, x)
    bad = np.nonzero(host.view(np.uint64) != dev.view(np.uint64))[0]
    assert bad.size == 0, [(float(x[i]), int(i & 3), float(host[i]), float(dev[i])) for i in bad[:8]]


def _div_pairs():
    """(numerators, divisors) for tree_div, every divisor 1..65535 (the counts a tree can hold) in each group:
      - a seeded random 53-bit numerator at a seeded exponent of 2^-150 .. 2^140, either sign;
      - exact multiples k d and half-way cases (k + 1/2) d (products below 2^53: exact), either sign: the quotient is representable
        and must come back exactly;
      - the float64 neighbours of k d on both sides, and a negative one: quotients a hair off a representable value, where a last
        correction step that is missing or misdirected rounds the wrong way."""
    rng = np.random.Generator(np.random.PCG64(11))
    d = np.arange(1, 65536, dtype=np.float64)
    sign = lambda: rng.choice([-1.0, 1.0], d.size)
    m = rng.integers(1 << 52, 1 << 53, d.size).astype(np.float64)
    rand = np.ldexp(m, rng.integers(-150 - 52, 140 - 52 + 1, d.size).astype(np.int32)) * sign()
    k = rng.integers(1, 1 << 35, d.size).astype(np.float64)
    kd = k * d                                             # < 2^51: exact
    half = (2.0 * k + 1.0) * d * 0.5                       # (2 k + 1) d < 2^52: exact, and so is its half
    assert (kd / d == k).all() and (half / d == k + 0.5).all()
    nums = [rand, kd * sign(), half * sign(), np.nextafter(kd, np.inf), np.nextafter(kd, -np.inf), -np.nextafter(kd, np.inf)]
    return np.concatenate(nums), np.tile(d, len(nums))


def test_tree_div_is_the_correctly_rounded_quotient(native):
    """tree_div (csrc/tree.cuh: v_rcp_f64, two Newton steps, quotient, one residual correction -- no operand scaling, no fix-up)
    against IEEE float64 division on the host: pairs are packed (numerator, divisor) at in[2j], in[2j + 1]."""
    n, d = _div_pairs()
    x = np.empty(2 * n.size)
    x[0::2], x[1::2] = n, d
    host = O.math_eval(15, x)
    np.testing.assert_array_equal(host[0::2].view(np.uint64), (n / d).view(np.uint64))      # the oracle's counterpart is numpy's division
    dev = native.math_selftest(15, x)
    bad = np.nonzero(host.view(np.uint64) != dev.view(np.uint64))[0]
    assert bad.size == 0, [(float(x[i & ~1]), float(x[i | 1]), float(host[i]).hex(), float(dev[i]).hex()) for i in bad[:8]]
