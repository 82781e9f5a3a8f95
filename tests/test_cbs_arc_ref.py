"""Pins the plain restatement of the CBS arc search (cbs_arc_ref.py) on the CPU, before tests/test_cbs_arc_kernels_gpu.py holds the kernels against it: against a pure-Python
double loop, against the oracle's TMaxO, and input by input against the regime every catalogue input is named after."""
import collections

import numpy as np
import pytest

import cbs_arc_ref as R

SMALL_SIZES = (4, 5, 17, 64, 65, 129, 300)
CPU_MAX_N = 12289


def _small_inputs(kind, n):
    """the catalogue's kinds at sizes below their patterns' bins: the patterns that do not fit are moved to the front third"""
    if n >= R.min_size(kind): return np.array(R.make(kind, n))
    rng = np.random.default_rng([R.SEED, R.KINDS.index(kind), n])
    x = np.round(rng.normal(1.0, 0.3, n) * 100.0) / 100.0
    if kind == "twin": x[:] = 0.0; x[n // 4] = 1.0; x[n // 4 + 1] = -1.0; x[n // 2] = 1.0; x[n // 2 + 1] = -1.0; return x[:n]
    x[n // 3:n // 3 + 2] += 3.0
    return x - np.cumsum(x)[-1] / n


def _double_loop(sx, al0):
    n = len(sx); rn = float(n)
    dmax = [0.0] * n; first = [0] * n; M = -1.0; count = 0; arc = None
    for L in range(1, n):
        c = rn / (float(L) * (rn - float(L))); best = -1.0
        for i in range(n - L):
            d = abs(float(sx[i + L]) - float(sx[i]))
            if d > best: best = d; first[L] = i
            if max(1, al0) <= L <= min(n - 1, n - al0):
                v = c * (d * d)
                if v > M: M = v; count = 1; arc = (L, i)
                elif v == M: count += 1
        dmax[L] = best
    return M, count, arc, dmax, first


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_arc_and_per_length_against_a_double_loop(kind):
    for n in SMALL_SIZES:
        sx = R.prefix(_small_inputs(kind, n))
        dmax, first = R.per_length(sx)
        for al0 in (1, 2, 3, 70, n // 2 + 1):
            M, count, arc, dm, fi = _double_loop(sx, al0)
            assert dmax[1:].tolist() == dm[1:] and first[1:].tolist() == fi[1:], (kind, n)
            ea = R.every_arc(sx, al0, dmax)
            if al0 > n - al0 or max(1, al0) > min(n - 1, n - al0):
                assert ea == (-1.0, 0, None) and count == 0, (kind, n, al0)
            else:
                assert (R.bits(ea[0]), ea[1], ea[2]) == (R.bits(M), count, arc), (kind, n, al0, ea, (M, count, arc))
                assert R.bits(R.arc_value(sx, *ea[2])) == R.bits(M)


def _cpu_cases():
    return [(k, n, a) for k in R.KINDS for n in (R.MODE0_SIZES if k == "f2" else R.MODE0_KIND_SIZES) if R.min_size(k) <= n <= CPU_MAX_N for a in (2, 3, 70) if n >= 2 * a]


def test_incumbent_and_paths_against_the_oracle():
    """paths 1, 2 and 3 reproduce the oracle's value bit for bit through normalise; on path 2 the arc is the oracle's; path 4 only where the oracle is strictly below"""
    seen = collections.Counter()
    for kind, n, al0 in _cpu_cases():
        x, sx, inc, _, _ = R.reference(kind, n)
        (M, count, arc), _, path = R.search(kind, n, al0)
        stat, iseg = R.oracle_tmaxo(kind, n, al0)
        tss = R.tss_of(x); seen[path] += 1
        if path == 0:
            assert inc[0] == 0.0 and stat == 0.0 and iseg == inc[1], (kind, n, al0)
        elif path == 1:
            assert R.bits(stat) == R.bits(R.normalise(inc[0], tss, n)) and iseg == inc[1], (kind, n, al0, stat, inc)
        elif path == 2:
            assert R.bits(stat) == R.bits(R.normalise(M, tss, n)) and iseg == (arc[1] + 1, arc[1] + 1 + arc[0]), (kind, n, al0)
        elif path == 3:
            assert count >= 2 and R.bits(stat) == R.bits(R.normalise(M, tss, n)), (kind, n, al0, stat, M)
            assert R.bits(R.arc_value(sx, iseg[1] - iseg[0], iseg[0] - 1)) == R.bits(M), (kind, n, al0)          # the oracle's arc is one of those that tie
        else:
            assert path == 4 and count == 1 and stat < R.normalise(M, tss, n), (kind, n, al0)
    print("expected paths of the catalogue up to %d bins at al0 2, 3, 70: %s" % (CPU_MAX_N, dict(sorted(seen.items()))))
    assert all(seen[p] > 0 for p in range(5)), seen


def test_the_incumbent_starts_from_zero_at_position_n():
    """Both extremes start as the exact 0 at position n (CBSTStatistic.cs:44-110) and only a strictly smaller / larger prefix sum replaces them: where the largest prefix sum is
    the rounding residue in the last element (a step at n / 3), or no prefix sum is negative, the arc between argmax and argmin is another arc and another value"""
    differ = []
    for kind in ("step", "per4", "twin"):
        for n in R.MODE0_KIND_SIZES:
            if n > CPU_MAX_N: continue
            x, sx, inc, _, _ = R.reference(kind, n)
            if R.bits(R.naive_incumbent(sx)) == R.bits(inc[0]): continue
            differ.append((kind, n))
            if R.search(kind, n, 2)[2] == 1:          # the incumbent is what TMaxO returns: the oracle sides with incumbent()
                stat, iseg = R.oracle_tmaxo(kind, n, 2)
                assert R.bits(stat) == R.bits(R.normalise(inc[0], R.tss_of(x), n)) != R.bits(R.normalise(R.naive_incumbent(sx), R.tss_of(x), n)) and iseg == inc[1], (kind, n)
    print("inputs whose argmax / argmin arc is not the reference's incumbent:", differ)
    assert ("step", 8193) in differ and any(k == "twin" for k, _ in differ), differ
    sx = R.reference("per4", 4097)[1]
    assert sx.min() == 0.0 and R.incumbent(sx)[1] == (2, 4097)          # no prefix sum below 0: the minimum is the 0 at position n, not the first 0 of the array
    assert R.incumbent(R.prefix(np.zeros(8)))[::2] == (0.0, 0.0)


PATH_BY_KIND = {"f2": 2, "two": 2, "neg": 2, "blk": 2, "sub": 2, "last": 2, "first": 2, "twin": 3, "per4": 1, "zeros": 0}
STEP_KEPT = (4097, 5121, 8193, 20481)          # step: the incumbent (minimum to position n) is the best arc
CAUCHY_UNSCANNED = (4161, 5121)
INT_TIE = (4097,)
F2_KEPT = (4, 5)                               # too short for anything to beat the arc between the extremes


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_input_reaches_its_regime(kind):
    for n in (R.MODE0_SIZES if kind == "f2" else R.MODE0_KIND_SIZES):
        if n < R.min_size(kind): continue
        (M, count, arc), bm, path = R.search(kind, n, 2)
        _, sx, inc, _, _ = R.reference(kind, n)
        if kind == "step": assert (path == 1) == (n in STEP_KEPT) and path in (1, 2), (n, path)
        elif kind == "cauchy": assert (path == 4) == (n in CAUCHY_UNSCANNED), (n, path)
        elif kind == "int": assert (path == 3) == (n in INT_TIE) and path in (2, 3), (n, path)
        elif kind == "f2" and n in F2_KEPT: assert path == 1, (n, path)
        else: assert path == PATH_BY_KIND[kind], (kind, n, path)
        if path == 0: continue
        L, i = arc
        if kind == "blk": assert i <= 1023 and i + L >= 1024 and L == 2, (n, arc)          # across the block border
        if kind == "sub": assert i <= 63 and i + L >= 64 and L == 2, (n, arc)              # across the sub-block border
        if kind == "last": assert i + L == n - 1, (n, arc)
        if kind == "first": assert i == 0, (n, arc)
        if kind == "twin": assert count == 4 and L == 2, (n, count, arc)
        if kind == "neg":
            A, B = i // R.BK, (i + L) // R.BK
            assert sx[i] > sx[i + L], (n, arc)                                              # from a maximum down to a minimum
            if A < B: assert bm["d2"][bm["pairs"].index((A, B))], (n, arc)                  # the surviving bound of its pair is max_A - min_B
    if kind == "neg":
        assert sum(1 for n in R.MODE0_KIND_SIZES if R.search("neg", n, 2)[0][2][1] // R.BK < sum(R.search("neg", n, 2)[0][2]) // R.BK) >= 3


@pytest.mark.parametrize("kind,n", [(k, n) for k in R.KINDS for n in R.AL0_SIZES if n >= R.min_size(k)])
def test_the_length_window(kind, n):
    """the al0 values of the GPU test: past n / 2 nothing is admissible, no pair survives and the incumbent stays"""
    for al0 in R.al0_values(n):
        ea, bm, path = R.search(kind, n, al0)
        if al0 == n // 2 + 1: assert ea == (-1.0, 0, None) and bm["npairs"] == 0 and bm["word5"] == 0.0 and path in (0, 1), (kind, n, al0)
        elif path: assert al0 <= ea[2][0] <= n - al0, (kind, n, al0, ea)


@pytest.mark.parametrize("kind,n", R.OVERFLOW_INPUTS)
def test_the_overflow_cases_overflow(kind, n):
    _, bm, path = R.search(kind, n, 2)
    assert path == 2 and 5 < bm["npairs"] < R.PAIRCAP, (kind, n, bm["npairs"])
    for cap in R.overflow_caps(bm["npairs"]):
        assert 1 <= cap <= R.PAIRCAP
    assert [bm["npairs"] > cap for cap in R.overflow_caps(bm["npairs"])] == [True, True, True, False, False]
