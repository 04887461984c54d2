#!/usr/bin/env python
"""What one ulp of the transcendentals costs the sign classifier, on the CPU.

The float32 statement of tests/_sign_ref.py is run with every exp / tanh / expm1 result moved to a
neighbouring float32 at random, DRAWS times per case, and the largest relative error against the
float64 statement is printed beside E (the unperturbed float32 statement's), the bar M and the
kernel's measured error, when one is given.  This is the computation that has to reach the kernel's
error before the factor 4 of M may rise; it prints, it decides nothing.

    python tools/sign_ulp_noise.py [--draws 40] [case[=kernel_rel_err] ...]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "isl-signlanguage-translation_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import _sign_ref as sr  # noqa: E402


class _Noisy:
    """numpy, with float32 exp / tanh / expm1 results moved by one ulp, up or down at random."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def __getattr__(self, name):
        return getattr(np, name)

    def _move(self, v):
        v = np.asarray(v)
        if v.dtype != np.float32:
            return v
        to = np.where(self.rng.rand(*v.shape) < 0.5, np.float32(np.inf), np.float32(-np.inf))
        return np.nextafter(v, to.astype(np.float32))

    def exp(self, z):
        return self._move(np.exp(z))

    def tanh(self, z):
        return self._move(np.tanh(z))

    def expm1(self, z):
        return self._move(np.expm1(z))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("cases", nargs="*", default=["odd", "workload", "shifted"])
    a = ap.parse_args()
    for spec in a.cases:
        name, _, kernel = spec.partition("=")
        c = sr.case(name)                               # the references, with numpy as it is
        sr.np = _Noisy(a.seed)
        try:
            errs = np.array([np.max(np.abs(sr.classify_batch(c["w"], c["x"], np.float32)[0].astype(np.float64)
                                           - c["p64"]) / c["p64"]) for _ in range(a.draws)])
        finally:
            sr.np = np
        line = "%-10s E %.3g  M %.3g  %d draws: median %.3g, 99 %% %.3g, max %.3g = %.2f E = %.2f M" % (
            name, c["E"], c["M"], a.draws, np.median(errs), np.quantile(errs, 0.99), errs.max(),
            errs.max() / c["E"], errs.max() / c["M"])
        if kernel:
            k = float(kernel)
            line += "; kernel %.3g = %.2f M, reached by %d draws" % (k, k / c["M"], int((errs >= k).sum()))
        print(line, flush=True)


if __name__ == "__main__":
    main()
