"""Inputs and settings of the parameter-axis tests (test_parameters_gpu.py, test_parameters_oracle.py): everything the product reads from CanvasPartitionParameters.json or the
command line and the suite otherwise holds at its default — CBS (nperm, alpha, undo_sd), the Wavelets thresholds and MinSize, MaxInterBinDistInSegment, CanvasBin -d.
The CPU companion asserts on the oracle alone that each setting reaches the regime it is meant for, so that an edit here cannot quietly empty the GPU tests."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------------------------- CBS
# floor(nperm alpha) = 500, 10, 2000, 200, 1 (one rejection allowed), 0 (a table of one entry); CanvasPartition's default last
CBS_PAIRS = [(10000, 0.05), (10000, 0.001), (10000, 0.2), (2000, 0.1), (500, 0.002), (1000, 0.0005), (10000, 0.01)]
CBS_DEGENERATE = (1000, 0.0005)
CBS_UNDO_PAIRS = [(2000, 0.1), (10000, 0.001)]            # the two pairs that also run with Prune and SDUndo
CBS_UNDO_SDS = [1.0, 3.0, 6.0]
CBS_LENGTHS = (24_000, 1_500, 150, 6_000)                  # above 20 000 bins; 201-2 000 (device loops, no stream); below 201 (non-hybrid test); one more long one
CBS_SEED = 2


def cbs_genome(seed=CBS_SEED, lengths=CBS_LENGTHS):
    """normal noise in two-decimal values with planted shifts of 4-500 bins whose t statistic (shift sqrt(width) / sd) lies between 3.5 and 6.5: above where TailP alone
    decides, below the t > 7 shortcut, so most candidate splits go through the permutation loop"""
    rng = np.random.RandomState(seed)
    parts = []
    for n in lengths:
        x = rng.normal(100, 10, n)
        for _ in range(max(1, n // 1200)):
            w = min(int(rng.choice([4, 8, 16, 40, 120, 500])), n // 3)
            a = int(rng.randint(0, n - w))
            t = rng.uniform(3.5, 6.5)
            x[a:a + w] += rng.choice([-1, 1]) * t * 10 / np.sqrt(w)
        parts.append(np.round(x, 2))
    return parts


def cbs_undo_genome():
    """the inputs of the undo runs: the three shorter chromosomes (Prune searches every subset of a chromosome's change points: a dozen at most here) plus two strong steps,
    of 4.5 and 8 standard deviations, so that undo_sd 1, 3 and 6 keep different sets"""
    per = cbs_genome()
    x = per[3].copy()
    x[1000:1400] += 45.0; x[3000:3300] += 80.0
    return [np.round(x, 2), per[1], per[2]]


def offsets(per):
    return np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------------------------ Wavelets
WV_LENGTHS = [40_000, 9_001, 300, 11, 10]
WV_WINDOW = 1000
WV_SEED = 31
# falling threshold: MadFactor 50 > 5 (default) > 0.5 > 0.05 > 0 — the breakpoint counts must grow along this list
WV_FALLING = [dict(mad_factor=50.0), dict(), dict(mad_factor=0.5), dict(mad_factor=0.05), dict(mad_factor=0.0)]
WV_CLAMPS = [dict(thr_upper=1.0),                           # the clamp from above takes effect (the unclamped threshold is far above 1)
             dict(thr_lower=0.0, thr_upper=0.0),            # threshold 0: every coefficient survives
             dict(thr_lower=500.0, thr_upper=1000.0)]       # the clamp from below: nothing survives
WV_MIN_SIZES = [4, 299, 300, 9_001]                         # the reference segments a chromosome when length > MinSize: 300 and 9 001 sit exactly on the bound, 299 one below
WV_SETTINGS = WV_FALLING + WV_CLAMPS + [dict(min_size=m) for m in WV_MIN_SIZES]
WV_SHARDED = [dict(mad_factor=0.05), dict(thr_upper=1.0), dict(min_size=300)]
WV_BIG_N, WV_BIG_SEED = 1_200_000, 32


def wv_genome():
    from test_wavelets_gpu import _coverage
    rng = np.random.RandomState(WV_SEED)
    return [_coverage(rng, n, mean=100.0, wave=0.05) for n in WV_LENGTHS]


def wv_big():
    from test_wavelets_gpu import _coverage
    rng = np.random.RandomState(WV_BIG_SEED)
    return [_coverage(rng, WV_BIG_N, mean=100.0, events=40, wave=0.05)]


def wv_device_kw(s):
    """oracle keyword names -> Canvas.wavelets keyword names"""
    names = dict(thr_lower="threshold_lower", thr_upper="threshold_upper")
    return {names.get(k, k): v for k, v in s.items()}


# ------------------------------------------------------------------------------------------------------------------------------------ segment ids at the gap bound
GAP_DISTS = [1, 1000, 1_000_000]
BIN_W = 100


def gap_case(D):
    """Five chromosomes of hand-placed bins of 100 bases for MaxInterBinDistInSegment = D.  The gap between a bin and its predecessor (start - previous end) is D - 1, D or
    D + 1 where listed below and 0 elsewhere; the reference splits when previousBinEnd + D < start, i.e. at D + 1 only.
      chr0  inside state runs, at a state change, two in a row, at the last two bins; its first bin starts D + 1 after position 0 (no previous bin: no split by the rule)
      chr1  excluded intervals [p + 1, p + 51] right behind the previous bin's end p, in a gap of D + 1 (both rules), of D and of D - 1 (the interval rule alone)
      chr2  a ploidy record that starts inside a gap of D and ends inside a gap of D + 1, then plain gaps of D + 1 and D
      chr3  five bins (no HMM state: -1 everywhere) with gaps D + 1, D, D - 1, D + 1
      chr4  an excluded interval and a ploidy boundary in the same gap of D, then a gap of D + 1
    Returns dict(chr, start, stop, off, state, gaps, excl, ploidy); excl / ploidy per chromosome in the form Canvas.segment_ids and the oracle take."""
    def place(gaps):
        st = np.zeros(len(gaps), np.int64); p = 0
        for i, g in enumerate(gaps):
            st[i] = p + g; p = st[i] + BIN_W
        return st
    G = []; S = []
    g = np.zeros(40, np.int64); g[0] = D + 1; g[5] = D - 1; g[6] = D; g[7] = D + 1; g[12] = D + 1; g[13] = D; g[20] = D + 1; g[21] = D + 1; g[38] = D; g[39] = D + 1
    s = np.full(40, 2, np.int32); s[12:26] = 3
    G.append(g); S.append(s)
    g = np.zeros(30, np.int64); g[8] = D + 1; g[15] = D; g[22] = D - 1; g[29] = D
    G.append(g); S.append(np.full(30, 2, np.int32))
    g = np.zeros(30, np.int64); g[0] = 7; g[8] = D; g[17] = D + 1; g[24] = D + 1; g[25] = D
    s = np.full(30, 1, np.int32); s[20:] = 2
    G.append(g); S.append(s)
    G.append(np.array([7, D + 1, D, D - 1, D + 1], np.int64)); S.append(np.full(5, -1, np.int32))
    g = np.zeros(12, np.int64); g[0] = 1; g[5] = D; g[9] = D + 1
    G.append(g); S.append(np.full(12, 3, np.int32))
    starts = [place(g) for g in G]
    z = np.zeros(0, np.int32)
    excl = [(z, z)] * 5; ploidy = [(z, z, z)] * 5
    prev_end = lambda c, i: int(starts[c][i - 1]) + BIN_W
    e = [prev_end(1, i) + 1 for i in (8, 15, 22)]
    excl[1] = (np.array(e, np.int32), np.array(e, np.int32) + 50)
    ploidy[2] = (np.array([prev_end(2, 8) + 1], np.int32), np.array([prev_end(2, 17) + 1], np.int32), np.array([1], np.int32))
    excl[4] = (np.array([prev_end(4, 5) + 1], np.int32), np.array([prev_end(4, 5) + 51], np.int32))
    ploidy[4] = (np.array([1], np.int32), np.array([prev_end(4, 5)], np.int32), np.array([3], np.int32))
    nb = [len(g) for g in G]
    start = np.concatenate(starts); assert start.max() + BIN_W < 2 ** 31
    return dict(chr=np.repeat(np.arange(5, dtype=np.int32), nb), start=start.astype(np.int32), stop=(start + BIN_W).astype(np.int32), off=offsets(G), state=np.concatenate(S),
                gaps=G, excl=excl, ploidy=ploidy)


def gap_expected(case, D, with_excl, with_ploidy):
    """the oracle's segment ids of a gap_case: segment starts from the state runs (DeriveSegments), then PostProcessSegments"""
    import oracle_lib as O
    off = case["off"]; nchr = len(off) - 1
    bs = [case["start"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]; be = [case["stop"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    segstarts = []
    for c in range(nchr):
        s = case["state"][off[c]:off[c + 1]]
        first = np.nonzero((s >= 0) & np.concatenate([[True], s[1:] != s[:-1]]))[0]
        segstarts.append(bs[c][first].astype(np.uint32))
    excl = case["excl"] if with_excl else None
    if with_ploidy:
        ids, last = O.postprocess_ploidy(bs, be, segstarts, excl, case["ploidy"], D)
    else:
        ids, last = O.postprocess(bs, be, segstarts, excl, D)
    return ids, last


# ---------------------------------------------------------------------------------------------------------------------------------------------- CanvasBin -d
BIN_NCHR = 70
BIN_DEPTHS = [1, 7, 100, 1000, 50_000]     # 50 000 counts per bin: a bin longer than the shortest primary chromosome's unique positions (and than every contig's)
