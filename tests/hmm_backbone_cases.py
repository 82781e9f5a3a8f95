"""The increments tests/test_hmm_backbone_gpu.py feeds to canvas_hmm_backbone_probe: one chromosome per case.  A case names the modes that may give it up (a fail word instead
of carries): only cases built to lie outside a mode's stated assumptions.  Every other (case, mode) is strict: fail == 0 and bit-equal carries.  tests/test_hmm_backbone_ref.py
checks the classification on the host (no bad increment, crossings per chunk, distance of the running sums from a power of two)."""
import math

import numpy as np

from hmm_backbone_ref import BB_CHUNK, BB_MAXC

CHAIN, SCAN, PIECES = 0, 1, 2
MODES = (CHAIN, SCAN, PIECES)
MODE_NAMES = {CHAIN: "chain", SCAN: "scan", PIECES: "pieces"}
LOG_STAY, LOG_MOVE = math.log(0.99), math.log(0.0025)
U = 2.0 ** -52          # ulp of a running sum in [1, 2)


class Case:
    def __init__(self, name, v, may_fail=(), modes=MODES):
        self.name = name
        self.v = np.ascontiguousarray(v, np.float64)
        self.may_fail = frozenset(may_fail)      # modes whose fail word is accepted (built to lie outside their assumptions)
        self.modes = tuple(modes)                # modes the case is given to (the chain takes no NaN)

    def strict(self, mode):
        return mode not in self.may_fail


def realistic(rng, n, first=None):
    """negative logs like the HMM's: an emission term plus log 0.99, now and then log 0.0025; the first step carries log pi instead"""
    v = -rng.gamma(2.0, 1.7, n) + np.where(rng.random_sample(n) < 0.01, LOG_MOVE, LOG_STAY)
    if n:
        v[0] = first if first is not None else -rng.gamma(2.0, 1.7) + math.log(0.2)
    return v


def _grow(acc_abs):
    """an increment that takes the running sum |D| = acc_abs into a higher binade, well away from the powers of two on both sides"""
    return -1.1 * acc_abs


def _with_crossings(rng, n, at):
    """|D| = 1.25 after step 0, then increments near 1e-9 (the sum stays in its binade for the lengths used here) and a crossing at every position of `at`"""
    v = -rng.uniform(0.5e-9, 1.5e-9, n)
    v[0] = -1.25
    acc = 0.0
    at = set(at)
    for t in range(n):
        if t in at:
            v[t] = _grow(-acc)
        acc = acc + v[t]
    return v


def build_cases():
    rng = np.random.RandomState(20260927)
    cases = []
    # ---- lengths: block, chunk and scan-iteration edges (one scan iteration is 8192 steps)
    for n in (11, 63, 64, 65, 1023, 1024, 1025, 2048, 8191, 8192, 8193, 3 * 8192 + 1):
        cases.append(Case(f"len{n}", realistic(rng, n)))
    # ---- realistic increments whose first one is the only large one
    cases.append(Case("first_large", np.concatenate([[-745.0], -rng.uniform(1e-3, 2e-2, 2999)])))
    # ---- exact ties: odd multiples of half an ulp of the running sum, k even and k odd, alone and in runs.  |D| stays in [1.25, 1.26): u = 2^-52, k = |D| / u
    t = [-1.25]                                                # k even
    t += [-0.5 * U] * 70                                       # tie, k even: stays (a run across a carry)
    t += [-U]                                                  # k odd
    t += [-0.5 * U]                                            # tie, k odd: up to even
    t += [-U] + [-0.5 * U] * 70                                # k odd, then a run: the first rounds up, the others stay
    t += [-1.5 * U] * 131                                      # k even: +2, k odd: +1 — the parity decides at every step
    t += [-U] + [-2.5 * U] * 67 + [-U] + [-3.5 * U] * 64
    t += list(-(2 * rng.randint(0, 512, 3000) + 1) * 0.5 * U)  # random odd multiples of half an ulp
    t += list(-rng.randint(0, 2048, 3000) * 0.25 * U)          # quarters: below, at and above one half
    cases.append(Case("ties", t))
    # the same in a binade the predicted pieces reach through crossings, with ties right behind a crossing and in front of the next
    t = [-0.3, -0.3, -0.3, -0.3]                               # |D| = 1.2 (inexact steps), then exact ties in [1, 2)
    t += [-0.5 * U, -U, -0.5 * U, -1.5 * U, -1.5 * U] * 40
    t += [-1.7]                                                # into [2, 4): u doubles
    t += [-U, -2 * U, -U, -3 * U, -3 * U] * 40                 # odd multiples of half the new ulp
    cases.append(Case("ties_across_binades", t))
    # ---- tiny increments: vanishing (shift >= 64), subnormal, zeros of both signs — in front of the first real increment and inside the sum
    t = [-1e-310, -5e-324, 0.0, -0.0]                          # |D| subnormal for four steps (each is a "crossing" for the pieces: four of the sixteen a chunk keeps)
    t += list(realistic(rng, 300, first=-40.0))
    t += [-1e-300, -5e-324, -0.0, 0.0, -2.2250738585072014e-308, -1e-30] * 150
    t += list(realistic(rng, 200))
    cases.append(Case("tiny", t))
    cases.append(Case("leading_zeros", [0.0, -0.0, -0.0] + list(realistic(rng, 500, first=-40.0))))
    # 70 leading -0.0: the sum must stay +0.0 (0.0 + -0.0), which carry[64] shows.  The pieces count every step on a zero sum as a crossing: more than they keep
    cases.append(Case("negative_zero_run", [-0.0] * 70 + list(realistic(rng, 200)), may_fail=(PIECES,)))
    # ---- large increments: larger than the running sum (shift <= 0), several binades at once
    t = [-0.7] + list(-rng.uniform(1e-4, 1e-3, 100)) + [-1e5] + list(-rng.uniform(1e-4, 1e-3, 100)) + [-3e12] + list(realistic(rng, 100)) + [-7e200, -1e-3, -6e250, -5e250]
    t += list(realistic(rng, 100))
    cases.append(Case("large", t))
    # ---- crossing placement: chunk step 0 and 1023, multiples of 64 and one step either side, the scan's iteration edge
    at = [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 8191, 8192, 8193]
    cases.append(Case("crossing_placement", _with_crossings(rng, 9000, at)))
    # ---- crossing count: exactly BB_MAXC and BB_MAXC + 1 inside one chunk, and more than 21 in a chromosome
    cases.append(Case("crossings_16_in_a_chunk", _with_crossings(rng, 3000, range(1100, 1100 + BB_MAXC))))
    cases.append(Case("crossings_16_spread", _with_crossings(rng, 3000, range(BB_CHUNK, 2 * BB_CHUNK, BB_CHUNK // BB_MAXC))))
    cases.append(Case("crossings_17_in_a_chunk", _with_crossings(rng, 3000, range(1100, 1100 + BB_MAXC + 1)), may_fail=(PIECES,)))
    cases.append(Case("crossings_30", _with_crossings(rng, 4000, list(range(200, 2200, 200)) + list(range(2300, 2310)) + list(range(3500, 3510)))))
    # ---- a piece reaching 2^53 / a predicted crossing that is none: the running sum sits next to a power of two and the re-associated prediction gets the step wrong
    #      (the scan and the chain must still be exact).  In the second case the prediction drifts into [2, 4) while the sum stays at 2 - u; the small increments behind the
    #      run are then placed in the wrong binade (a large one would be predicted as a crossing and done with a real add: measured, exact)
    cases.append(Case("rounds_up_to_the_binade_edge", [-(2.0 - 600 * U)] + [-(0.5 + 2.0 ** -10) * U] * 1500 + list(realistic(rng, 300)), may_fail=(PIECES,)))
    cases.append(Case("vanishing_below_the_binade_edge", [-(2.0 - U)] + [-0.25 * U] * 1500 + [-0.01] * 50 + list(realistic(rng, 300)), may_fail=(PIECES,)))
    # ---- outside the assumptions of the parallel forms
    t = realistic(rng, 700); t[333] = 1e-3
    cases.append(Case("positive_increment", t, may_fail=(SCAN, PIECES)))
    t = realistic(rng, 700); t[129] = -math.inf
    cases.append(Case("minus_infinity", t, may_fail=(SCAN, PIECES)))
    t = realistic(rng, 700); t[640] = math.nan
    cases.append(Case("nan", t, may_fail=(SCAN, PIECES), modes=(SCAN, PIECES)))
    # ---- skipped chromosomes (at most ten steps): nothing is written for them
    cases.append(Case("skipped10", realistic(rng, 10)))
    cases.append(Case("skipped1", realistic(rng, 1)))
    cases.append(Case("skipped0", realistic(rng, 0)))
    return cases


def genome(cases, mode):
    """the cases given to `mode` as one call: (cases, increments, offsets); skipped and empty chromosomes sit between the others"""
    mine = [c for c in cases if mode in c.modes]
    order = sorted(range(len(mine)), key=lambda i: (i * 7) % len(mine))      # a fixed shuffle: long and short chromosomes mixed
    mine = [mine[i] for i in order]
    off = np.concatenate([[0], np.cumsum([len(c.v) for c in mine])]).astype(np.int64)
    v = np.concatenate([c.v for c in mine]) if mine else np.zeros(0)
    return mine, v, off
