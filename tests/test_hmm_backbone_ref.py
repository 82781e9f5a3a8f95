"""The reference and the case list of tests/test_hmm_backbone_gpu.py, checked without a GPU: numpy's accumulate restates the plain loop bit for bit, the tie cases round the way
IEEE round-half-to-even says (worked out with exact fractions), and every case called strict for a mode lies inside that mode's stated assumptions."""
from fractions import Fraction

import numpy as np
import pytest

import hmm_backbone_cases as K
import hmm_backbone_ref as R


@pytest.fixture(scope="module")
def cases():
    return K.build_cases()


def test_numpy_accumulate_restates_the_loop(cases):
    for c in cases:
        loop, fast = R.carries_loop(c.v), R.carries_numpy(c.v)
        assert len(loop) == (len(c.v) + R.CARRY_EVERY - 1) // R.CARRY_EVERY
        assert R.same_bits(loop, fast), c.name
        if len(c.v):
            assert loop.view(np.uint64)[0] == 0          # +0.0 in front of the first step


def _is_exact_tie(acc, v, result):
    """acc + v lies exactly half-way between two neighbouring doubles, and `result` is the one of them with the even mantissa"""
    exact = Fraction(acc) + Fraction(v)
    other = np.nextafter(result, -np.inf if exact < Fraction(result) else np.inf)
    half_way = Fraction(result) + Fraction(float(other)) == 2 * exact
    even = (np.float64(result).view(np.uint64) & np.uint64(1)) == 0
    return half_way and bool(even)


def test_tie_cases_by_hand():
    u = K.U
    # k = |D| / u even, half an ulp: stays
    assert -1.25 + -0.5 * u == -1.25 and _is_exact_tie(-1.25, -0.5 * u, -1.25)
    # k odd, half an ulp: up to the even neighbour
    assert -(1.25 + u) + -0.5 * u == -(1.25 + 2 * u) and _is_exact_tie(-(1.25 + u), -0.5 * u, -(1.25 + 2 * u))
    # three halves: k even -> k + 2, k odd -> k + 1
    assert -1.25 + -1.5 * u == -(1.25 + 2 * u) and _is_exact_tie(-1.25, -1.5 * u, -(1.25 + 2 * u))
    assert -(1.25 + u) + -1.5 * u == -(1.25 + 2 * u) and _is_exact_tie(-(1.25 + u), -1.5 * u, -(1.25 + 2 * u))
    # the last odd k of a binade, half an ulp: up to the power of two (the step that leaves the binade)
    assert -(2.0 - u) + -0.5 * u == -2.0 and _is_exact_tie(-(2.0 - u), -0.5 * u, -2.0)
    # and the reference follows, seen at the carry in front of step 64: a run of three-halves steps from an even k adds 2 at every step (k stays even)
    v = np.array([-1.25] + [-1.5 * u] * 128)
    assert R.carries_numpy(v)[1] == -(1.25 + 2 * 63 * u)
    v = np.array([-1.25, -u] + [-1.5 * u] * 127)
    assert R.carries_numpy(v)[1] == -(1.25 + u + (1 + 2 * 61) * u)          # k odd: +1 (to even), then +2 per step (62 steps of the run lie in front of t = 64)


def test_ties_really_occur(cases):
    """the tie cases are ties at the step where they arrive (not merely multiples of half an ulp of 1.25)"""
    c = next(x for x in cases if x.name == "ties")
    d = R.running_sums(c.v)
    n = 0
    for t in range(1, len(c.v)):
        if c.v[t] != 0 and _is_exact_tie(float(d[t]), float(c.v[t]), float(d[t + 1])):
            n += 1
    assert n >= 2000, n


def test_strict_cases_are_inside_the_assumptions(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        bad = bool(R.bad_increment(c.v).any())
        if len(c.v) < R.MIN_T:
            continue
        per_chunk = R.crossings_per_chunk(c.v)
        # the chain: finite or -inf increments only
        if K.CHAIN in c.modes:
            assert not np.isnan(c.v).any() and not (c.v == np.inf).any(), c.name
        # the scan assumes no bad increment, nothing else
        if K.SCAN in c.modes and c.strict(K.SCAN):
            assert not bad, c.name
        # the pieces: no bad increment, at most BB_MAXC crossings in a chunk, and running sums far enough from the powers of two for the predicted binades to be right
        if K.PIECES in c.modes and c.strict(K.PIECES):
            assert not bad, c.name
            assert per_chunk.max() <= R.BB_MAXC, (c.name, per_chunk.tolist())
            assert R.binade_margin(c.v) >= 1e-9, (c.name, R.binade_margin(c.v))
    by = {c.name: c for c in cases}
    # the cases built for the edges are at them
    assert R.crossings_per_chunk(by["crossings_16_in_a_chunk"].v)[1] == R.BB_MAXC
    assert R.crossings_per_chunk(by["crossings_16_spread"].v)[1] == R.BB_MAXC
    assert R.crossings_per_chunk(by["crossings_17_in_a_chunk"].v)[1] == R.BB_MAXC + 1
    assert R.crossings_per_chunk(by["crossings_30"].v).sum() > 21
    assert R.binade_margin(by["rounds_up_to_the_binade_edge"].v) == 0.0
    assert R.binade_margin(by["vanishing_below_the_binade_edge"].v) < 1e-15
    d = R.running_sums(by["crossing_placement"].v)
    e = np.frexp(np.abs(d))[1]
    for t in (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 8191, 8192, 8193):
        assert e[t + 1] > e[t], t                                       # the step t leaves its binade
    z = R.running_sums(by["negative_zero_run"].v)[:71]
    assert (z.view(np.uint64) == 0).all()                               # +0.0 all along the run of -0.0


def test_genome_keeps_every_case_of_the_mode(cases):
    for mode in K.MODES:
        mine, v, off = K.genome(cases, mode)
        assert sorted(c.name for c in mine) == sorted(c.name for c in cases if mode in c.modes)
        assert off[-1] == len(v) and (np.diff(off) == [len(c.v) for c in mine]).all()
        assert any(len(c.v) <= 10 for c in mine)
