#!/usr/bin/env python3
"""One-off soak on the GPU box: the random populations of tests/test_population_fuzz.py (per-net settings and budgets in one launch)
over many more seeds (python tests/fuzz_population.py [first_seed] [count]); prints the seeds that disagree with the oracle, if any.
Every seed runs under its own forced variant; a seed whose budgets still fit when rotated by one net searches a second time."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_util as P  # noqa: E402
import population_fuzz as F  # noqa: E402
import test_population_fuzz as T  # noqa: E402
from alphazero_gym_amd import _native  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 48
count = int(sys.argv[2]) if len(sys.argv) > 2 else 300
bad, seen, twice = [], {}, 0
t0 = time.time()
for seed in range(first, first + count):
    c = F.case(seed)
    for var in T.FORCING:
        os.environ.pop(var, None)
    if c.variant != "default":
        os.environ[P.VARIANT_ENV[c.variant][0]] = P.VARIANT_ENV[c.variant][1]
    second = c.K >= 2 and len(set(c.sims)) > 1 and F.rotated(c) is not None
    twice += second
    seen[c.variant] = seen.get(c.variant, 0) + 1
    try:
        T.run_case(_native, c, second=second)
    except AssertionError as ex:
        bad.append(seed)
        print(F.describe(c), "DIFFERS:", str(ex)[:300], flush=True)
print(f"{count} random populations from seed {first}: {len(bad)} differ {bad} ({twice} searched twice; variants {dict(sorted(seen.items()))}; "
      f"{time.time() - t0:.0f} s)")
