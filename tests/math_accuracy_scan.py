"""Interior accuracy of include/azg_math.h's float32 functions: the scans behind profiles/math_edge_accuracy.txt, part 2.

Host functions (the CPU oracle's azo_math_eval; the device computes the same bits) against numpy's float64 libm, whose own error
(about 1e-16 relative) is 1e-9 of a float32 ulp.  Error in units of the last place of the exact result.  CPU only, about a minute.

    python tests/math_accuracy_scan.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]   # (the oracle is test infrastructure: this script lives with the tests)
import oracle_lib as O  # noqa: E402


def ulps(y, ref):
    e = np.maximum(np.floor(np.log2(np.abs(ref))), -126)
    return np.abs(y - ref) / 2.0 ** (e - 23)


def scan(name, fn, lo, hi, ref_fn, n=None):
    """Every float32 of [lo, hi] (n is None) or n of them evenly spaced in bit pattern."""
    a, b = sorted(int(v) for v in np.array([lo, hi], np.float32).view(np.uint32))
    bits = np.arange(a, b + 1, dtype=np.int64) if n is None else np.linspace(a, b, n).astype(np.int64)
    x = bits.astype(np.uint32).view(np.float32).astype(np.float64)
    y, ref = O.math_eval(fn, x), ref_fn(x)
    ok = ref != 0
    u = ulps(y[ok], ref[ok])
    print(f"{name:12s} [{lo:g}, {hi:g}]  {x.size:9d} inputs  max {u.max():.3f} ulp at {float(x[ok][np.argmax(u)])!r}")


if __name__ == "__main__":
    N = 4_000_000
    scan("azg_logf", 3, 0.7072, 1.4142, np.log)                 # one whole mantissa range around 1, where the result is small
    scan("azg_tanhf", 2, 1e-30, 9.0, np.tanh, N)
    scan("azg_cos2pif", 4, 1e-30, 0.99999994, lambda u: np.cos(2 * np.pi * u), N)
    scan("azg_expm1f", 1, -87.0, -1e-30, np.expm1, N)
    scan("azg_expm1f", 1, 1e-30, 88.0, np.expm1, N)
    scan("azg_expf", 0, -87.0, -1e-30, np.exp, N)
    scan("azg_expf", 0, 1e-30, 88.0, np.exp, N)
