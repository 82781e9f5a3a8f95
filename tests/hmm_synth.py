"""Low-noise synthetic coverage with chosen chromosome lengths for the HMM tests: what CanvasPartition reads (F2 text parsed as double) around a diploid level, with planted
copy-number segments.  IQR / median stays below 0.2 (asserted by the callers): the dispersion at which the first speculative attempt verifies in the project's soak runs."""
import numpy as np


def coverage(seed, lengths, median=100.0, sd=4.0, alts=(1, 3, 4, 0)):
    """(bins, cov, off): bins has the start / stop arrays segment_ids wants (100-base bins, 50-base gaps every 97 bins)"""
    rng = np.random.RandomState(seed)
    lengths = [int(n) for n in lengths]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N = int(off[-1])
    cn = np.full(N, 2.0)
    k = 0
    for c, n in enumerate(lengths):            # a diploid stretch of 50-110 bins, then 15-40 bins of another copy number (about a fifth of the bins: both quartiles stay diploid)
        t = int(rng.randint(50, 110))
        while t < n:
            w = int(rng.randint(15, 40))
            cn[off[c] + t:off[c] + min(n, t + w)] = alts[k % len(alts)]
            k += 1
            t += w + int(rng.randint(50, 110))
    cov = np.round((median / 2.0 * cn + rng.normal(0.0, sd, N)).clip(0.0), 2)
    start = np.concatenate([np.arange(n, dtype=np.int64) * 100 + (np.arange(n) // 97) * 50 for n in lengths] or [np.zeros(0, np.int64)]).astype(np.int32)
    bins = {"start": start, "stop": (start + 100).astype(np.int32)}
    return bins, np.ascontiguousarray(cov, np.float64), off


def dispersion(cov):
    """IQR / median as the driver sees it (float quartiles)"""
    q1, q2, q3 = np.percentile(cov.astype(np.float32), [25, 50, 75])
    return float((q3 - q1) / q2)
