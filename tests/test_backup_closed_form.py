"""CPU: the claim behind backup_path's closed form (csrc/tree.cuh, the gamma == 1 arm of the discrete chain), the float32 values on
which it does NOT hold (edge_values.TEETH: what the GPU cases feed), and the conditions every case of tests/test_edge_values.py
must meet on the oracle alone before the device is compared with it.

The arm: `V == 0 or 2^-25 <= |V| < 2^30` takes V + (r_first + d r_uniform) in one float64 addition; any other V takes the serial
chain R = r + R.  Chain and closed form are restated in numpy float64 exactly as tree.cuh writes them (edge_values.chain / closed)."""
import numpy as np
import pytest

import edge_values as E


def _mantissas():
    rng = np.random.Generator(np.random.PCG64(7))
    return np.unique(np.concatenate([[0, 1, 0x7fffff, 0x7ffffe, 0x400000], rng.integers(0, 1 << 23, 300)]).astype(np.uint32))


@pytest.mark.parametrize("env", sorted(E.REWARDS))
def test_closed_form_equals_the_chain_inside_its_range(env):
    """Every float32 exponent of [2^-25, 2^30), edge and seeded random mantissas, both signs, +-0: levels 1..16 bit for bit."""
    mant = _mantissas()
    exps = np.arange(-25, 30, dtype=np.int64)
    v = (((exps[:, None] + 127).astype(np.uint32) << 23) | mant[None, :]).ravel()
    v = np.concatenate([v, v | np.uint32(0x80000000), np.array([0, 0x80000000], np.uint32)]).view(np.float32)
    assert E.in_range(v).all() and np.abs(v).max() == E.f32(0x4e7fffff) and np.abs(v[v != 0]).min() == E.LO
    for rewards in {E.REWARDS[env], E.LEAF_REWARDS[env]}:
        a, b = E.chain(v, *rewards), E.closed(v, *rewards)
        assert a.shape == (16, v.size)
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def test_range_test_is_the_kernels():
    """in_range on both sides of both thresholds (the values the GPU cases put there)."""
    for b, want in ((0x33000000, True), (0x32ffffff, False), (0x4e7fffff, True), (0x4e800000, False), (0x00000000, True),
                    (0x80000000, True), (0x00000001, False), (0x000116c2, False), (0x7f7fffff, False)):
        assert bool(E.in_range(E.f32(b))) is want and bool(E.in_range(-E.f32(b))) is want, hex(b)
    assert E.bits(np.float32(1e-40)) == 0x000116c2


@pytest.mark.parametrize("env", sorted(E.TEETH))
def test_teeth_differ_outside_the_range(env):
    """At least one value below 2^-25 and one at or above 2^30 per env; each really differs, under every reward pattern the env's
    paths carry, in a return of the first four levels and in the W of an edge visited a few times."""
    teeth = E.TEETH[env]
    assert any(0 < abs(float(t)) < 2.0 ** -25 for t in teeth) and any(abs(float(t)) >= 2.0 ** 30 for t in teeth)
    for t in teeth:
        assert t.dtype == np.float32 and np.isfinite(t) and not E.in_range(t)
        for rewards in {E.REWARDS[env], E.LEAF_REWARDS[env]}:
            a, b = E.chain(t, *rewards), E.closed(t, *rewards)
            assert (a[:4] != b[:4]).any(), (hex(E.bits(t)), rewards)
            assert E.line_W_differs(t, rewards)
    print(env, [hex(E.bits(t)) for t in teeth])


def test_known_counterexamples():
    """The two values the closed form's range was checked against when it was written: both differ at level 2."""
    for b, rewards in ((0x26d55555, (1.0, 1.0)), (0x5a7fffff, (1.0, 1.0)), (0x5a7fffff, (-1.0, -1.0))):
        a, c = E.chain(E.f32(b), *rewards), E.closed(E.f32(b), *rewards)
        assert a[0] == c[0] and a[1] != c[1], hex(b)


# ------------------------------------------------------------------------------------------------ the GPU cases, on the oracle alone

_DISCRETE = E.discrete_oracle_cases()


@pytest.mark.parametrize("env,V,setup", [pytest.param(*c[1:], id=c[0]) for c in _DISCRETE])
def test_discrete_case_conditions(env, V, setup):
    """Leaf depths <= 15, == 16 and >= 17 (CartPole: >= 33 too), the intended bits in every non-terminal node, terminal leaves
    beside them, the dump's W equal to the replayed chain, and on a TEETH value at least one edge whose W the closed form would have
    changed."""
    opts = E.DISCRETE_SETUPS[setup]
    out = E.oracle_discrete(env, V, **opts)
    n_sims = opts.get("n_sims") or E.default_sims(env)
    fig = E.check_discrete_conditions(env, V, out, n_sims, opts.get("gamma", 1.0))
    print(env, setup, hex(E.bits(V)), fig)


@pytest.mark.parametrize("env", sorted(E.ENV))
def test_population_case_conditions(env):
    """Each net of the three-net launch on its own oracle engine: the same conditions per net."""
    for V, out in zip(E.short_list(env), E.oracle_population(env)):
        fig = E.check_discrete_conditions(env, V, out, E.default_sims(env))
        print(env, hex(E.bits(V)), fig)


@pytest.mark.parametrize("shape,setting", [(s, st) for s in E.CONT_SHAPES for st in E.cont_settings(s)])
def test_continuous_case_conditions(shape, setting):
    """The intended value bits in every node, a subnormal first-level product, sigma at exp(log_param_min / max) in every evaluation,
    every sampled action exactly +-bound, the mixture's first share exactly 1."""
    E.check_continuous_conditions(shape, setting, E.oracle_continuous(shape, setting))
