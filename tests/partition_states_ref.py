"""Partition states restated in plain numpy, for the tests of canvas_partition_states_cbs / canvas_partition_states_breakpoints, and the reference's segment START
COORDINATES per chromosome built by two routes:

    literally          CBSRunner.cs:127-137 (the cs1 / cs2 loop over lengthSeg) and SegmentationInput.DeriveSegments (Segmentation.cs:83-125), which is what the
                       CanvasPartition executable runs on the host
    from the states    the starts of the bins where the state changes, or where the chromosome opens with a state >= 0: what canvas_segment_ids* makes of a state array

Only the SET of starts reaches SegmentationResultsProcessor.PostProcessSegments, so two routes agree when their sets do.  Also the directed and random configurations the CPU
and the GPU tests share."""
import numpy as np


class Invalid(Exception):
    """what the CBS entry refuses: (chromosome, kind), kind one of "nseg", "length", "sum" """
    def __init__(self, chromosome, kind):
        super().__init__(chromosome, kind)
        self.chromosome, self.kind = chromosome, kind


def states_cbs(chr_offset, seg_len, nseg):
    """seg_len in the layout canvas_cbs documents: chromosome c has its nseg[c] lengths at seg_len[chr_offset[c]:]"""
    off = np.asarray(chr_offset, np.int64)
    state = np.full(int(off[-1]), -1, np.int32)
    first_bad = None
    for c in range(len(off) - 1):
        T, k = int(off[c + 1] - off[c]), int(nseg[c])
        bad = None
        if k < 0 or k > T:
            bad = "nseg"
        elif k > 0:
            lens = np.asarray(seg_len[off[c]:off[c] + k], np.int64)
            if (lens < 1).any():
                bad = "length"
            elif int(lens.sum()) != T:
                bad = "sum"
            else:
                state[off[c]:off[c + 1]] = np.repeat(np.arange(k, dtype=np.int32), lens)
        if bad and first_bad is None:
            first_bad = Invalid(c, bad)
    if first_bad:
        raise first_bad
    return state


def states_breakpoints(chr_offset, breakpoints):
    off = np.asarray(chr_offset, np.int64)
    state = np.full(int(off[-1]), -1, np.int32)
    for c in range(len(off) - 1):
        T = int(off[c + 1] - off[c])
        bp = np.asarray(breakpoints[c], np.int64)
        assert ((bp >= 0) & (bp < T)).all()                  # refused on the host
        if T == 0:
            continue
        flag = np.zeros(T, np.int32)
        flag[0] = 1
        if len(bp) >= 2 and T > 10:
            flag[bp] = 1
        state[off[c]:off[c + 1]] = np.cumsum(flag) - 1
    return state


def starts_from_states(chr_offset, state, bin_start):
    """per chromosome: the start coordinates of the bins k_seg_flags opens a segment at for the state alone, state >= 0 && (first || state != previous)"""
    off = np.asarray(chr_offset, np.int64)
    out = []
    for c in range(len(off) - 1):
        s = np.asarray(state[off[c]:off[c + 1]]); b = np.asarray(bin_start[off[c]:off[c + 1]])
        opens = np.zeros(len(s), bool)
        if len(s):
            opens[0] = True
            opens[1:] = s[1:] != s[:-1]
            opens &= s >= 0
        out.append(b[opens].astype(np.uint32))
    return out


def literal_starts_cbs(chr_offset, seg_len, nseg, bin_start):
    """CBSRunner.cs:127-137, the loop as it stands"""
    off = np.asarray(chr_offset, np.int64)
    out = []
    for c in range(len(off) - 1):
        start_by_chr = bin_start[off[c]:off[c + 1]]
        length_seg = [int(v) for v in seg_len[off[c]:off[c] + int(nseg[c])]]
        starts = []
        cs1, cs2 = 0, -1
        for i in range(len(length_seg)):
            cs2 += length_seg[i]
            starts.append(start_by_chr[cs1])
            cs1 += length_seg[i]
        out.append(np.array(starts, np.uint32))
    return out


def literal_starts_breakpoints(chr_offset, breakpoints, bin_start):
    """DeriveSegments (Segmentation.cs:83-125) as the executable applies it to every chromosome that has bins"""
    off = np.asarray(chr_offset, np.int64)
    out = []
    for c in range(len(off) - 1):
        start_by_chr = bin_start[off[c]:off[c + 1]]
        segments_length = len(start_by_chr)
        if segments_length == 0:
            out.append(np.zeros(0, np.uint32))
            continue
        bp = [int(v) for v in breakpoints[c]]
        start_pos = []
        if len(bp) >= 2 and segments_length > 10:
            if bp[0] != 0:
                bp.insert(0, 0)
            start_pos.append(bp[0])
            for i in range(1, len(bp) - 1):
                start_pos.append(bp[i])
            start_pos.append(bp[len(bp) - 1])
        else:
            start_pos.append(0)
        out.append(np.array([start_by_chr[p] for p in start_pos], np.uint32))
    return out


def same_start_sets(a, b):
    return len(a) == len(b) and all(set(x.tolist()) == set(y.tolist()) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- configurations
LENGTHS = (0, 1, 10, 11, 255, 0, 256, 257, 2047, 2048, 2049, 4097, 0)      # the 256-thread workgroup, the 2 048-bin block of the segment-id scan; empty first, midway, last


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def bins(lengths, seed, far=0.01):
    """start / stop (int32, concatenated) with strictly increasing starts: abutting bins of 50 .. 149 bases, now and then a gap of 5 000 .. 50 000 bases"""
    rng = np.random.RandomState(seed)
    start, stop = [], []
    for T in lengths:
        size = rng.randint(50, 150, T); gap = np.where(rng.rand(T) < far, rng.randint(5000, 50000, T), rng.choice([0, 0, 0, 1, 7], T))
        s = 1000 + np.cumsum(size + gap) - size
        start.append(s); stop.append(s + size)
    return np.concatenate(start + [np.zeros(0, np.int64)]).astype(np.int32), np.concatenate(stop + [np.zeros(0, np.int64)]).astype(np.int32)


def cbs_layout(lengths, cuts):
    """cuts[c]: sorted segment starts within chromosome c (bin indices; empty: no segment) -> (seg_len with one spare entry as Canvas.cbs returns it, nseg)"""
    off = offsets(lengths)
    seg_len = np.zeros(int(off[-1]) + 1, np.int32); nseg = np.zeros(len(lengths), np.int32)
    for c, T in enumerate(lengths):
        k = np.asarray(cuts[c], np.int64)
        if len(k):
            assert k[0] == 0 and (np.diff(k) > 0).all() and k[-1] < T
            seg_len[off[c]:off[c] + len(k)] = np.diff(np.concatenate([k, [T]]))
            nseg[c] = len(k)
    return seg_len, nseg


def directed_cbs(lengths=LENGTHS):
    """[(name, seg_len, nseg)]: nseg of 0, 1 and T_c (every length 1: the tiled length scan beyond one tile); boundaries on a workgroup edge (a multiple of 256 bins from
    the first bin of the call), on a block edge (a multiple of 2 048) and on the chromosome's last bin"""
    off = offsets(lengths)
    out = [("no segment anywhere", ) + cbs_layout(lengths, [[] for _ in lengths]),
           ("one segment each", ) + cbs_layout(lengths, [[0] if T else [] for T in lengths]),
           ("every length 1", ) + cbs_layout(lengths, [np.arange(T) for T in lengths]),
           ("every length 1, every other chromosome without segments", ) + cbs_layout(lengths, [np.arange(T) if c & 1 else [] for c, T in enumerate(lengths)])]
    edges = []
    for c, T in enumerate(lengths):
        g = np.arange(off[c], off[c + 1])
        k = set(g[(g % 256 == 0)].tolist()) | set(g[(g % 2048 == 0)].tolist()) | ({int(off[c + 1]) - 1} if T else set()) | ({int(off[c])} if T else set())
        k |= set((g[(g - off[c]) % 256 == 0]).tolist())                         # ... and a multiple of 256 bins from the first bin of the chromosome
        edges.append(np.array(sorted(k), np.int64) - off[c])
    out.append(("boundaries on workgroup edges, block edges and last bins", ) + cbs_layout(lengths, edges))
    return out


BP_PATTERNS = ("none", "one", "two from 0", "two not from 0", "repeated", "descending", "last bin", "many")


def breakpoints_of(pattern, T):
    """the pattern cut to a chromosome of T bins (every breakpoint inside [0, T))"""
    if T == 0 or pattern == "none":
        return []
    last, mid = T - 1, T // 2
    bp = {"one": [mid], "two from 0": [0, mid], "two not from 0": [min(1, last), last], "repeated": [mid, mid, 0, mid], "descending": [last, mid, min(2, last)],
          "last bin": [0, last], "many": list(range(0, T, 3))}[pattern]
    return bp


def directed_breakpoints(lengths=LENGTHS):
    """[(name, breakpoints per chromosome)]: configuration k gives chromosome c pattern (c + k) % 8, so every chromosome length meets every pattern — among them two and
    more breakpoints on the chromosomes of 10 and of 11 bins"""
    return [("patterns rotated by %d" % k, [np.array(breakpoints_of(BP_PATTERNS[(c + k) % len(BP_PATTERNS)], T), np.int32) for c, T in enumerate(lengths)])
            for k in range(len(BP_PATTERNS))]


def random_config(seed, total=3000):
    """(lengths, "cbs", seg_len, nseg) or (lengths, "breakpoints", breakpoints): 1 .. 9 chromosomes of together a few thousand bins, some empty or short"""
    rng = np.random.RandomState(seed)
    nchr = int(rng.randint(1, 10))
    lengths = [int(v) for v in rng.choice([0, 1, 5, 10, 11, 12, 64, 255, 256, 257, 600, 2048, 2049], nchr)]
    lengths[int(rng.randint(nchr))] += int(rng.randint(total // 2, total))
    if seed & 1:
        cuts = []
        for T in lengths:
            style = rng.randint(4)
            if T == 0 or style == 0:
                cuts.append([])
            elif style == 1:
                cuts.append(np.arange(T))
            else:
                inner = np.nonzero(rng.rand(T) < rng.choice([0.002, 0.05, 0.5]))[0]
                cuts.append(np.unique(np.concatenate([[0], inner])))
        return (lengths, "cbs") + cbs_layout(lengths, cuts)
    bps = []
    for T in lengths:
        n = int(rng.choice([0, 1, 2, 3, 40])) if T else 0
        bp = rng.randint(0, T, n) if T else np.zeros(0, np.int64)
        if n and rng.rand() < 0.3:
            bp[0] = 0
        bps.append(bp.astype(np.int32))
    return lengths, "breakpoints", bps


def intervals(lengths, start, stop, seed):
    """excluded intervals (sorted by end) and ploidy records for the chain through segment_ids: every chromosome with at least 20 bins gets a few of each, so that they also
    fall on chromosomes whose states are -1.  Returns (excluded, ploidy): per chromosome (starts, stops) and (one-based starts, ends, copy numbers) or None"""
    rng = np.random.RandomState(seed)
    off = offsets(lengths)
    z = np.zeros(0, np.int32)
    excluded, ploidy = [], []
    for c, T in enumerate(lengths):
        if T < 20:
            excluded.append((z, z)); ploidy.append(None)
            continue
        s, e = start[off[c]:off[c + 1]].astype(np.int64), stop[off[c]:off[c + 1]].astype(np.int64)
        pick = np.sort(rng.choice(T - 2, min(4, T // 5), replace=False))
        a = e[pick] - rng.randint(0, 40, len(pick)); b = a + rng.randint(10, 90, len(pick))
        order = np.argsort(b, kind="stable")
        excluded.append((a[order].astype(np.int32), b[order].astype(np.int32)))
        k1, k2 = T // 3, 2 * T // 3
        ploidy.append((np.array([int((s[k1] + e[k1]) // 2) + 1, int(e[k2]) + 1], np.int32), np.array([int(e[k2]), int(e[-1]) + 100], np.int32), np.array([1, int(rng.choice([0, 2, 3]))], np.int32)))
    return excluded, ploidy
