"""CPU: what every case of tests/rollout_edges.py contains, shown on the CPU rollout alone (rollout_ref.cpu_rollout with a trace), at
the narrow shape.  A case whose condition fails here is a bad case, not a device bug: tests/test_rollout_edges.py (GPU) then compares
the kernels with these same rollouts bit for bit, and would compare them with something that does not hold what its name says."""
import numpy as np
import pytest

import rollout_edges as RE
import rollout_ref as R


@pytest.mark.parametrize("name", list(RE.CASES))
def test_case_contains_what_it_is_named_for(name):
    case = RE.CASES[name]
    out, trace = RE.traced(name)
    RE.check_common(case, out, trace)
    case.check(case, out, trace)
    # the trace is the rollout: replaying its rewards and flags gives the arrays
    for j, steps in RE.by_game(trace).items():
        assert [e["t"] for e in steps] == list(range(len(steps))) and len(steps) == out["lengths"][j]
        ret = 0.0
        for e in steps:
            ret = ret + e["reward"]
        assert np.float64(ret).tobytes() == out["returns"][j].tobytes()
        assert bool(steps[-1]["done"]) == bool(out["terminated"][j]) and not any(e["done"] for e in steps[:-1])
        for a, b in zip(steps, steps[1:]):
            assert a["next_state"].tobytes() == b["state"].tobytes()


def test_trace_is_optional_and_changes_nothing():
    """cpu_rollout without a trace, and the cached reference, give the traced run's arrays."""
    name = "G3_both_clamps_sample"
    out, _ = RE.traced(name)
    RE.assert_same_bits(RE.reference(name), out, name)
    a = R.reference("cartpole", (16,), "discrete", "elu", False, 500, 1.0, 5, 6, "sample", 1000, 0)
    trace = []
    b = R.cpu_rollout(R.GAMES["cartpole"], R.net_desc("cartpole", (16,), "discrete", "elu"), R.net_blob("cartpole", (16,), "discrete", False, 500),
                      5, 6, "sample", 1000, 0, trace=trace)
    RE.assert_same_bits(b, a, "make_weights net")
    assert len(trace) == int(a["lengths"].sum()) and all(0.0 < e["u"] < 1.0 for e in trace)


@pytest.mark.parametrize("name", RE.SAME_AT_EVERY_WIDTH)
def test_added_width_is_zeros(name):
    """The same arrays at the narrow, the streamed and the wide shape: the signal units move (first, middle, last of each width), the
    rest is zeros.  This licenses asserting the conditions at the narrow shape only."""
    want = RE.reference(name)
    for hidden in (RE.STREAMED, RE.WIDE):
        RE.assert_same_bits(RE.reference(name, hidden), want, f"{name} {hidden}")


def test_signal_units_sit_in_different_slices():
    for hidden in (RE.NARROW, RE.STREAMED, RE.WIDE, (512, 512), RE.WIDE_1024):
        units = RE.signal_units(hidden)
        assert len({RE.head_chunk(hidden, u) for u in units}) == 3
        if hidden[0] >= 449:
            assert len({u // 64 for u in units}) == 3 and units[-1] // 64 == (-(-hidden[0] // 64)) - 1   # the last slice holds the last unit


def test_assert_same_bits_tells_zeros_apart_and_refuses_nan():
    base = {"returns": np.zeros(2), "lengths": np.ones(2, np.int32), "terminated": np.zeros(2, bool), "first_value": np.zeros(2, np.float32)}
    RE.assert_same_bits(base, {k: v.copy() for k, v in base.items()}, "same")
    for key, bad in (("first_value", np.float32(-0.0)), ("returns", -0.0), ("first_value", np.float32(np.nan)), ("returns", np.nan)):
        a, b = {k: v.copy() for k, v in base.items()}, {k: v.copy() for k, v in base.items()}
        a[key][1] = bad
        if bad != bad:
            b[key][1] = bad                                        # NaN on both sides: still refused
        with pytest.raises(AssertionError):
            RE.assert_same_bits(a, b, "differs")
