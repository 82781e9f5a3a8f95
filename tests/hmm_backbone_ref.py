"""Reference of the exact backbone of the speculative Viterbi pass (canvas_amd/csrc/hmm.hip, stage B1): the plain sequential IEEE double sum D_t = D_{t-1} + v_t from
D_{-1} = +0.0, recorded in front of every step t that is a multiple of 64 — what k_vit_verify starts its blocks from.  Also the host restatements of what the parallel forms
of the backbone assume about their increments (bb_bad_increment, the binade crossings per 1024-step chunk), used to classify the cases of tests/hmm_backbone_cases.py."""
import math

import numpy as np

CARRY_EVERY = 64     # carry[] holds D at the multiples of 64
BB_CHUNK = 1024      # steps per chunk of the predicted pieces
BB_MAXC = 16         # binade crossings a chunk of the predicted pieces keeps
MIN_T = 11           # chromosomes of at most ten steps are skipped


def carries_loop(v):
    """the definition: a plain Python loop over IEEE doubles"""
    acc = 0.0
    out = []
    for t in range(len(v)):
        if t % CARRY_EVERY == 0:
            out.append(acc)
        acc = acc + float(v[t])
    return np.array(out, np.float64)


def running_sums(v):
    """D_{-1}, D_0, ..., D_{T-1} (T + 1 values) by numpy's sequential accumulate; the leading +0.0 makes the first step the addition 0.0 + v_0 of the loop"""
    return np.add.accumulate(np.concatenate([[0.0], np.asarray(v, np.float64)]))


def carries_numpy(v):
    return np.ascontiguousarray(running_sums(v)[:len(v)][::CARRY_EVERY])


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload of a propagated NaN is the host's business)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


def bad_increment(v):
    """bb_bad_increment: NaN, an infinity, or a positive value (+0.0 is fine)"""
    b = np.asarray(v, np.float64).view(np.uint64)
    return (((b >> np.uint64(52)) & np.uint64(0x7FF)) == np.uint64(0x7FF)) | (((b >> np.uint64(63)) == 0) & ((b << np.uint64(1)) != 0))


def _exponent(x):
    return ((np.abs(x).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def crossings_per_chunk(v):
    """steps that leave their binade, per BB_CHUNK steps, by the exact sums: the biased exponent of |D| changes over the step, or |D| in front of it is zero / subnormal
    (k_bb_pieces: ep == 0 || ec != ep, there on predicted sums)"""
    d = running_sums(v)
    e = _exponent(d)
    cross = (e[:-1] == 0) | (e[1:] != e[:-1])
    n = len(v)
    pad = (-n) % BB_CHUNK
    return np.concatenate([cross, np.zeros(pad, bool)]).reshape(-1, BB_CHUNK).sum(axis=1)


def binade_margin(v):
    """smallest relative distance of a running sum |D_t| (normal numbers only) from a power of two: the predicted pieces place their crossings with a re-associated sum that
    is good to about 1e-12 for the lengths used here, so a case is inside their assumptions only when this is far larger"""
    m = np.abs(running_sums(v))
    m = m[(m >= 2.2250738585072014e-308) & np.isfinite(m)]
    if len(m) == 0:
        return math.inf
    frac, _ = np.frexp(m)              # m = frac * 2^e, frac in [0.5, 1)
    return float(np.minimum(frac * 2 - 1, 1 - frac).min() if len(frac) else math.inf)
