"""Segments.ReadSegments (CanvasCommon/Segments.cs:52-144) restated in Python from the C#, for the tests of canvas_segment_tables: one entry from the rows of a
*.partitioned file (from_text, the reference's own input) and one from per-bin arrays (from_arrays, what the device entry is given).  Both go through the same grouping.

    rows      -> GroupByAdjacent(chromosome)            (:55)   a chromosome is a run of rows with the same name
    per chr   -> GroupByAdjacent(segment id)            (:63)   a segment is a run of rows with the same id: an id that returns later is a new segment
    segment   -> Begin = first bin's start, End = last bin's stop, its bins' counts = float.Parse(column 4)                       (:106-124)
                 StartConfidenceInterval / EndConfidenceInterval from the segment's outer bins and their neighbours IN THE CHROMOSOME (:67-104)
"""
import fractions

import numpy as np


def half_length(start, stop):
    """(int)Math.Round(Length / 2.0, MidpointRounding.AwayFromZero), Length = stop - start >= 0 (:95-98): halves go up"""
    length = int(stop) - int(start)
    assert length >= 0
    return (length + 1) // 2


def start_ci(this, prev):
    """GetStartConfidenceInterval (:81-86); a bin is (start, stop), prev is None at the first segment of a chromosome"""
    if prev is None or prev[1] != this[0]:
        return (-half_length(*this), half_length(*this))
    return (-half_length(*prev), half_length(*this))


def end_ci(this, nxt):
    """GetEndConfidenceInterval (:88-93)"""
    if nxt is None or this[1] != nxt[0]:
        return (-half_length(*this), half_length(*this))
    return (-half_length(*this), half_length(*nxt))


def parse_float32(text):
    """float.Parse: the float32 NEAREST to the decimal the text denotes (ties to even), decided in exact rational arithmetic — not the text rounded to double and then to
    float, which is the double rounding the library's cast has to be shown equal to"""
    exact = fractions.Fraction(text)
    guess = np.float32(float(text))                            # at most one float away
    cands = {float(guess), float(np.nextafter(guess, np.float32(np.inf))), float(np.nextafter(guess, np.float32(-np.inf)))}
    best = None
    for c in sorted(cands):
        if not np.isfinite(c):
            continue
        d = abs(fractions.Fraction(c) - exact)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[1]):
            best = (d, even, c)
    return np.float32(best[2])


def format_g15(v):
    """the text CanvasPartition writes for a coverage (Segmentation.cs:247: the double's default ToString, 15 significant digits) in the range the counts live in"""
    s = "%.15g" % float(v)
    assert "e" not in s, s
    return s


def _group_adjacent(keys):
    """[(key, first, last + 1)] of the runs of equal keys"""
    runs = []
    for i, k in enumerate(keys):
        if runs and runs[-1][0] == k:
            runs[-1][2] = i + 1
        else:
            runs.append([k, i, i + 1])
    return runs


def _tables(chr_runs, start, stop, ids, counts):
    """chr_runs: [(first bin, last bin + 1)] per chromosome, empty chromosomes included"""
    begin, end, bin_off, ci4, chr_seg = [], [], [], [], [0]
    for b0, b1 in chr_runs:
        groups = [(b0 + f, b0 + l) for _, f, l in _group_adjacent(list(ids[b0:b1]))]
        for g, (f, l) in enumerate(groups):
            first, last = (start[f], stop[f]), (start[l - 1], stop[l - 1])
            prev = None if g == 0 else (start[f - 1], stop[f - 1])
            nxt = None if g == len(groups) - 1 else (start[l], stop[l])
            begin.append(first[0]); end.append(last[1]); bin_off.append(f)
            ci4.append(start_ci(first, prev) + end_ci(last, nxt))
        chr_seg.append(len(begin))
    n = chr_runs[-1][1] if chr_runs else 0
    return dict(nseg=len(begin), chr_seg_offset=np.array(chr_seg, np.int64), seg_begin=np.array(begin, np.int32), seg_end=np.array(end, np.int32),
                seg_bin_offset=np.array(bin_off + [n], np.int64), seg_ci4=np.array(ci4, np.int32).reshape(-1, 4), counts=counts)


def from_arrays(chr_offset, start, stop, segment_id, cov=None):
    """what canvas_segment_tables is defined to return: the chromosomes are chr_offset's (empty ones allowed), counts = (float)cov"""
    off = [int(v) for v in chr_offset]
    start = [int(v) for v in start]; stop = [int(v) for v in stop]; ids = [int(v) for v in segment_id]
    assert off[0] == 0 and off[-1] == len(start) == len(stop) == len(ids)
    counts = None if cov is None else np.asarray(cov, np.float64).astype(np.float32)
    return _tables([(off[c], off[c + 1]) for c in range(len(off) - 1)], start, stop, ids, counts)


def from_text(text):
    """the reference's entry: (chromosome names in file order, tables); the chromosomes are the runs of equal names, the ids are compared as the strings they are"""
    rows = [line.split("\t") for line in text.splitlines()]
    names = [r[0] for r in rows]
    runs = _group_adjacent(names)
    assert len({k for k, _, _ in runs}) == len(runs), "a chromosome that returns: ToOrderedDictionary throws"
    counts = np.array([parse_float32(r[3]) for r in rows], np.float32)
    t = _tables([(f, l) for _, f, l in runs], [int(r[1]) for r in rows], [int(r[2]) for r in rows], [r[4] for r in rows], counts)
    return [k for k, _, _ in runs], t


def same_tables(got, want, counts=True):
    """every table (and every float, by its bits) equal"""
    assert int(got["nseg"]) == int(want["nseg"]), (got["nseg"], want["nseg"])
    for k in ("chr_seg_offset", "seg_begin", "seg_end", "seg_bin_offset", "seg_ci4"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (k, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    if counts and want["counts"] is not None:
        g, w = np.asarray(got["counts"], np.float32), np.asarray(want["counts"], np.float32)
        assert g.shape == w.shape
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert len(bad) == 0, ("counts", bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())
