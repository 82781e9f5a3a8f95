"""Named node families for the direct tests of the Wavelets kernels, as integers k = 100 x (CanvasPartition reads two-decimal text); x = k / 100 bit for bit.
Non-tie families have one clear arg-max of |I+ - I-|; tie families have two (or all) indices with the same value, which the closed form must leave to the exact chain."""
import zlib

import numpy as np

KMAX = 1_999_999_999                 # the largest integer the prefix kernels accept (x < 2e7)
NON_TIE = ("poisson", "step", "headspike", "tailspike")
TIE_ANY_N = ("flat", "zero")
TIE_ODD_N = ("ramp", "one")          # symmetric about the middle: two equal maxima when n - 1 is even
FAMILIES = NON_TIE + TIE_ANY_N + TIE_ODD_N


def is_tie(name, n):
    return name in TIE_ANY_N or (name in TIE_ODD_N and n % 2 == 1)


def family(name, n, seed=0):
    """int64[n] of the family; seeded by (name, n, seed)"""
    rng = np.random.RandomState(zlib.crc32(f"{name}/{n}/{seed}".encode()) & 0x7FFFFFFF)
    if name in ("poisson", "step"):
        k = rng.poisson(100, n).astype(np.int64) * 100 + rng.randint(0, 100, n)        # mean 100.xx
        if name == "step":
            k[:max(1, n // 3)] *= 2
        return k
    k = np.zeros(n, np.int64)
    if name == "headspike":
        k[:2] = KMAX
    elif name == "tailspike":
        k[-3:] = KMAX
    elif name == "flat":
        k[:] = 10_000
    elif name == "ramp":
        k[:] = 100 * np.arange(n)
    elif name == "one":
        k[n // 2] = 100
    elif name != "zero":
        raise ValueError(name)
    return k


def decreasing_x(n):
    """x itself (not two-decimal values: the subtree walker reads the doubles): strictly decreasing and geometric, so that every node of the tree splits off its first bin
    (depth n - 1, the deepest tree a root of n bins can have)"""
    return np.array([1.0e9 * 0.25 ** i for i in range(n)], np.float64)


def to_x(k):
    x = np.asarray(k, np.int64) / 100.0
    assert (np.rint(x * 100.0).astype(np.int64) == k).all()
    return x
