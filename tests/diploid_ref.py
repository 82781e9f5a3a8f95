"""Two CPU restatements of CanvasDiploidCaller.CallVariants between the parsed files and the written ones (CanvasDiploidCaller.cs:295-343 with IO.cs:134-179,
CanvasSegment.cs MergeIn / MergeSegments / SetFilterForSegments, SegmentScoringModel.cs:26-41,114-171, Utilities.cs:188-196,470-474,948-955), written independently of
each other and of call.hip — each from the C#:

  direct(...)      one object per segment and per site, the reference's loops as they stand (the forward-only pointer of ReadFrequencies, sorted lists, the scans)
  vectorised(...)  numpy over offsets (searchsorted, cumsum, reduceat-style gathers), no per-segment objects

Both take the arguments of Canvas.call_diploid as numpy arrays and return its dict.  float32 / float64 are used exactly where the reference uses float / double.  exp, log10
and pow go through Python's math module, i.e. the C library the product's host code calls as well (numpy's vector forms of them may differ in the last bit)."""
import math

import numpy as np

F32 = np.float32
LOGISTIC_GERMLINE = (-5.0123, 4.9801, -5.5472, -1.7914)
INT_MIN = -2**31


# ---------------------------------------------------------------------------------------------------------------- shared by neither: each restatement has its own helpers
class _Seg:
    def __init__(self, chrom, begin, end, counts):
        self.chr, self.begin, self.end, self.counts = chrom, begin, end, list(counts)
        self.freqs, self.cover = [], []
        self.cn, self.mcc, self.dist, self.dist2, self.q = -1, None, 0.0, 0.0, 0
        self.first = self.last = None
        self.start_ci = self.end_ci = None


def _median_sorted_list(values, as_double):
    """SortedList<T>.Median(): a[n/2] for odd n, (a[n/2-1] + a[n/2]) / 2 in T for even n"""
    a = sorted(values); n = len(a)
    if n % 2 == 1:
        return float(a[n // 2])
    if as_double:
        return (float(a[n // 2 - 1]) + float(a[n // 2])) / 2
    return float(F32(F32(a[n // 2 - 1]) + F32(a[n // 2])) / F32(2))


def _round_to_int(v):
    """(int)Math.Round(v): half to even; what does not fit an int becomes int.MinValue (the x86 conversion)"""
    if v != v or v in (math.inf, -math.inf):
        return INT_MIN
    r = round(v)
    return r if -2**31 <= r <= 2**31 - 1 else INT_MIN


def _log10(x):
    return math.log10(x) if x > 0 else (-math.inf if x == 0 else math.nan)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def qscore_direct(b, bin_count, cn, dist, dist2):
    score = b[0]
    score += math.log10(1 + bin_count) * b[1]
    score += (dist / max(1.0, cn - 4.0)) * b[2]
    score += (0.0 if dist2 == 0 else dist / dist2) * b[3]
    score = _exp(score)
    score = score / (score + 1) if score != math.inf else math.nan
    q = _round_to_int(-10 * _log10(1 - score)) if score == score else INT_MIN
    return max(2, min(40, q))


def estimate_diploid_maf(cn, mean_coverage):
    c1 = mean_coverage / 2.0
    return 0.5 - 1 / (3.352 * math.pow(cn * c1, 0.4747))


def ploidy_table(mean_coverage):
    """InitializePloidies: (copy number, major chromosome count, minor allele frequency) in the reference's order"""
    out = []
    for cn in range(0, 11):
        major = cn
        while major * 2 >= cn:
            if cn == 0:
                maf = 0.01
            else:
                vf = F32(major) / F32(cn)
                maf = float(vf) if vf < 0.5 else float(F32(1) - vf)
                if major * 2 == cn:
                    maf = estimate_diploid_maf(cn, mean_coverage)
            out.append((cn, major, maf))
            major -= 1
    return out


def merge_segments(segs, minimum_call_size=0, maximum_merge_span=10000):
    """CanvasSegment.MergeSegments(segments, minimumCallSize, maximumMergeSpan) on _Seg objects (copyNumbers == null); returns the merged list"""
    def merge_in(a, s):                                                          # CanvasSegment.MergeIn (also exported below as merge_in)
        if s.begin < a.begin:
            a.start_ci = s.start_ci; a.begin = s.begin; a.counts = s.counts + a.counts; a.freqs = s.freqs + a.freqs; a.cover = s.cover + a.cover; a.first = s.first
        if s.end > a.end:
            a.end_ci = s.end_ci; a.end = s.end; a.counts = a.counts + s.counts; a.freqs = a.freqs + s.freqs; a.cover = a.cover + s.cover; a.last = s.last

    merged = []
    if not segs:
        return merged
    i = 0
    while i < len(segs):
        if segs[i].end - segs[i].begin >= minimum_call_size:
            merged.append(segs[i]); i += 1; continue
        prev, prev_q = -1, -1
        for k in range(i - 1, -1, -1):
            if segs[k].chr != segs[i].chr:
                break
            if segs[k].end - segs[k].begin < minimum_call_size:
                continue
            if segs[i].begin - segs[k].end > maximum_merge_span:
                break
            prev, prev_q = k, segs[k].q
            break
        nxt, next_q = -1, -1
        for k in range(i + 1, len(segs)):
            if segs[k].chr != segs[i].chr:
                break
            if segs[k].end - segs[k].begin < minimum_call_size:
                continue
            if segs[k].begin - segs[i].end > maximum_merge_span:
                break
            nxt, next_q = k, segs[k].q
            break
        if prev_q >= 0 and prev_q >= next_q:
            merge_in(segs[prev], segs[i]); i += 1; continue
        if next_q >= 0:
            for t in range(nxt - 1, i - 1, -1):
                merge_in(segs[nxt], segs[t])
            i = nxt; continue
        merged.append(segs[i]); i += 1
    segs = merged
    merged = [segs[0]]
    last = segs[0]
    for s in segs[1:]:
        if last.cn == s.cn and last.chr == s.chr and s.begin - last.end < maximum_merge_span:
            merge_in(last, s)
            continue
        last = s
        merged.append(s)
    return merged


def direct(counts, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt, logistic=LOGISTIC_GERMLINE):
    nchr = len(chr_seg_offset) - 1
    segs = []
    for c in range(nchr):
        for s in range(chr_seg_offset[c], chr_seg_offset[c + 1]):
            sg = _Seg(c, int(seg_begin[s]), int(seg_end[s]), counts[seg_bin_offset[s]:seg_bin_offset[s + 1]])
            sg.first = sg.last = s
            segs.append(sg)
    # ReadFrequencies: the forward-only pointer per chromosome
    for c in range(nchr):
        mine = segs[chr_seg_offset[c]:chr_seg_offset[c + 1]]
        if not mine:
            continue
        index = 0
        for i in range(chr_site_offset[c], chr_site_offset[c + 1]):
            position, ref, alt = int(site_pos[i]), int(site_ref[i]), int(site_alt[i])
            if ref + alt < 10:
                continue
            while index < len(mine):
                if mine[index].end > position:
                    break
                index += 1
            if index >= len(mine):
                continue
            if mine[index].begin > position:
                continue
            mine[index].freqs.append(F32(alt) / F32(ref + alt))
            mine[index].cover.append(ref + alt)
    cover = [t for sg in segs for t in sg.cover]
    mean_coverage = sum(cover) / len(cover)
    table = ploidy_table(mean_coverage)
    total = 0.0
    for sg in segs:
        for v in sg.counts:
            total += float(v)
    diploid = total / sum(len(sg.counts) for sg in segs)
    factor = 0.6 / diploid
    points = [(diploid * cn / 2.0, 0.0 if maf != maf else maf, cn, major) for cn, major, maf in table]
    res = dict((k, []) for k in ("bin_count", "median_count", "site_count", "informative", "median_maf", "cn", "mcc", "dist", "dist2", "qscore"))
    for sg in segs:
        mafs = [float(F32(1) - f) if f > 0.5 else float(f) for f in sg.freqs]
        cutoff = (sg.end - sg.begin) // 463 // 2                                  # (lengths are not negative: // is the integer division of C#)
        median_coverage = _median_sorted_list(sg.counts, False)
        informative = len(mafs) >= max(10, cutoff)
        median_maf = _median_sorted_list(mafs, True) if informative else -1.0
        best = second = 1.7976931348623157e308
        best_point = None
        for cov, maf, cn, major in points:
            diff = (cov - median_coverage) * factor
            distance = diff * diff
            if informative:
                diff = maf - median_maf
                distance += diff * diff
            if distance < best:
                second = best; best = distance; best_point = (cn, major)
            elif distance < second:
                second = distance
        sg.cn, sg.mcc = best_point
        sg.dist, sg.dist2 = best, second
        if len(mafs) < 10:
            sg.mcc = None
        sg.q = qscore_direct(logistic, len(sg.counts), sg.cn, sg.dist, sg.dist2)
        for k, v in (("bin_count", len(sg.counts)), ("median_count", median_coverage), ("site_count", len(mafs)), ("informative", int(informative)), ("median_maf", median_maf),
                     ("cn", sg.cn), ("mcc", -1 if sg.mcc is None else sg.mcc), ("dist", best), ("dist2", second), ("qscore", sg.q)):
            res[k].append(v)
    runs = merge_segments(segs)
    rr = dict((k, []) for k in ("run_first", "run_last", "run_begin", "run_end", "run_cn", "run_mcc", "run_qscore", "run_filter", "run_bin_count", "run_median_count"))
    for r in runs:
        q = qscore_direct(logistic, len(r.counts), r.cn, r.dist, r.dist2)
        flt = (1 if q < 10 else 0) | (2 if r.end - r.begin < 10000 else 0)
        for k, v in (("run_first", r.first), ("run_last", r.last), ("run_begin", r.begin), ("run_end", r.end), ("run_cn", r.cn), ("run_mcc", -1 if r.mcc is None else r.mcc),
                     ("run_qscore", q), ("run_filter", flt), ("run_bin_count", len(r.counts)), ("run_median_count", _median_sorted_list([float(v) for v in r.counts], True))):
            rr[k].append(v)
    res.update(rr)
    return _as_arrays(res, diploid, mean_coverage, len(cover))


_DTYPES = dict(bin_count=np.int64, median_count=np.float64, site_count=np.int64, informative=np.int32, median_maf=np.float64, cn=np.int32, mcc=np.int32, dist=np.float64,
               dist2=np.float64, qscore=np.int32, run_first=np.int64, run_last=np.int64, run_begin=np.int32, run_end=np.int32, run_cn=np.int32, run_mcc=np.int32,
               run_qscore=np.int32, run_filter=np.int32, run_bin_count=np.int64, run_median_count=np.float64)


def _as_arrays(res, diploid, mean_coverage, kept):
    out = {k: np.asarray(res[k], _DTYPES[k]) for k in _DTYPES}
    out.update(diploid_coverage=float(diploid), mean_coverage=float(mean_coverage), kept_sites=int(kept))
    return out


# ---------------------------------------------------------------------------------------------------------------- the vectorised restatement
def _seg_medians(values, off, double_average):
    """median of values[off[s]:off[s+1]] for every s with a sort of (segment, value) pairs; empty segments give nan"""
    n = np.diff(off)
    ids = np.repeat(np.arange(len(n)), n)
    v = np.asarray(values[off[0]:off[-1]])
    order = np.lexsort((v, ids))
    sv = v[order]
    base = off[:-1] - off[0]
    out = np.full(len(n), np.nan, np.float64)
    ok = n > 0
    hi = sv[(base + n // 2)[ok]]
    lo = sv[(base + np.maximum(n // 2 - 1, 0))[ok]]
    even = (n % 2 == 0)[ok]
    if double_average:
        avg = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    else:
        avg = ((lo.astype(F32) + hi.astype(F32)) / F32(2)).astype(np.float64)
    out[ok] = np.where(even, avg, hi.astype(np.float64))
    return out


def _qscores(b, bins, cn, dist, dist2):
    out = np.zeros(len(bins), np.int32)
    ratio = np.divide(dist, dist2, out=np.zeros_like(dist), where=dist2 != 0)
    md = dist / np.maximum(1.0, cn - 4.0)
    for i in range(len(bins)):
        x = b[0]
        x = x + math.log10(1 + int(bins[i])) * b[1]
        x = x + md[i] * b[2]
        x = x + ratio[i] * b[3]
        e = _exp(x)
        p = e / (e + 1) if e != math.inf else math.nan
        t = -10 * _log10(1 - p) if p == p else math.nan
        if t != t or abs(t) == math.inf:
            q = INT_MIN
        else:
            q = int(np.rint(t))
            q = q if -2**31 <= q < 2**31 else INT_MIN
        out[i] = max(2, min(40, q))
    return out


def vectorised(counts, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt, logistic=LOGISTIC_GERMLINE):
    cso = np.asarray(chr_seg_offset, np.int64); csi = np.asarray(chr_site_offset, np.int64); sbo = np.asarray(seg_bin_offset, np.int64)
    beg = np.asarray(seg_begin, np.int64); end = np.asarray(seg_end, np.int64)
    pos = np.asarray(site_pos, np.int64); ref = np.asarray(site_ref, np.int64); alt = np.asarray(site_alt, np.int64)
    nseg, nchr = len(beg), len(cso) - 1
    seg_chr = np.repeat(np.arange(nchr), np.diff(cso))
    # sites to segments: first segment of the chromosome whose End > position (ends increase, positions do not decrease: that is where the forward pointer stands)
    site_seg = np.full(len(pos), -1, np.int64)
    for c in range(nchr):
        a, b = csi[c], csi[c + 1]
        if cso[c + 1] == cso[c] or a == b:
            continue
        k = cso[c] + np.searchsorted(end[cso[c]:cso[c + 1]], pos[a:b], side="right")
        inside = k < cso[c + 1]
        kk = np.where(inside, k, cso[c])
        good = inside & (beg[kk] <= pos[a:b]) & (ref[a:b] + alt[a:b] >= 10)
        site_seg[a:b] = np.where(good, kk, -1)
    kept = site_seg >= 0
    tot = (ref + alt)[kept]
    mean_coverage = float(int(tot.sum()) / int(kept.sum()))
    f = alt[kept].astype(F32) / tot.astype(F32)
    folded = np.where(f > 0.5, F32(1) - f, f).astype(F32)
    site_off = np.searchsorted(site_seg[kept], np.arange(nseg + 1), side="left").astype(np.int64)
    n_maf = np.diff(site_off)
    x = np.asarray(counts, F32)
    diploid = float(np.cumsum(x.astype(np.float64))[-1] / len(x))                 # cumsum adds in order: the serial loop of Utilities.Mean
    factor = 0.6 / diploid
    # model points
    cn_l, mj_l = [], []
    for cn in range(11):
        for mj in range(cn, -1, -1):
            if 2 * mj >= cn:
                cn_l.append(cn); mj_l.append(mj)
    pcn = np.array(cn_l); pmj = np.array(mj_l)
    with np.errstate(invalid="ignore", divide="ignore"):
        vf = pmj.astype(F32) / pcn.astype(F32)
    pmaf = np.where(vf < 0.5, vf, F32(1) - vf).astype(np.float64)
    for i in range(len(pcn)):
        if pcn[i] == 0:
            pmaf[i] = 0.01
        elif 2 * pmj[i] == pcn[i]:
            pmaf[i] = 0.5 - 1 / (3.352 * math.pow(int(pcn[i]) * (mean_coverage / 2.0), 0.4747))
    pmaf = np.where(np.isnan(pmaf), 0.0, pmaf)
    pcov = diploid * pcn / 2.0
    assert len(pcn) == 36
    med_cov = _seg_medians(x, sbo, False)
    cutoff = (end - beg) // 463 // 2
    informative = n_maf >= np.maximum(10, cutoff)
    med_maf = np.where(informative, np.nan_to_num(_seg_medians(folded, site_off, True), nan=-1.0), -1.0)
    d = (pcov[None, :] - med_cov[:, None]) * factor
    dist = d * d
    dm = pmaf[None, :] - med_maf[:, None]
    dist = np.where(informative[:, None], dist + dm * dm, dist)
    # the strict scan: best = first minimum; runner-up = the smallest of the others, where an earlier point that was best and then displaced counts with its distance
    bi = np.argmin(dist, axis=1)                                                   # argmin returns the first of equal minima
    rows = np.arange(nseg)
    best = dist[rows, bi]
    rest = dist.copy(); rest[rows, bi] = np.inf
    second = np.minimum(rest.min(axis=1), 1.7976931348623157e308)
    cn = pcn[bi].astype(np.int32)
    mcc = np.where(n_maf < 10, -1, pmj[bi]).astype(np.int32)
    bins = np.diff(sbo)
    q = _qscores(logistic, bins, cn, best, second)
    # runs: a segment starts a run unless it joins the run in front of it; the run's end is the end of the segment in front (ends increase within a chromosome)
    starts = np.ones(nseg, bool)
    if nseg > 1:
        same = (seg_chr[1:] == seg_chr[:-1]) & (beg[1:] - end[:-1] < 10000)
        # same CN as the RUN's first segment: a run is a stretch of equal CN, so equal to the neighbour is the same thing
        starts[1:] = ~(same & (cn[1:] == cn[:-1]))
    first = np.nonzero(starts)[0]
    last = np.append(first[1:] - 1, nseg - 1)
    rbins = sbo[last + 1] - sbo[first]
    rq = _qscores(logistic, rbins, cn[first], best[first], second[first])
    rf = (rq < 10).astype(np.int32) | ((end[last] - beg[first] < 10000).astype(np.int32) << 1)
    rmed = _seg_medians(x, np.append(sbo[first], sbo[-1]), True)
    res = dict(bin_count=bins, median_count=med_cov, site_count=n_maf, informative=informative, median_maf=med_maf, cn=cn, mcc=mcc, dist=best, dist2=second, qscore=q,
               run_first=first, run_last=last, run_begin=beg[first], run_end=end[last], run_cn=cn[first], run_mcc=mcc[first], run_qscore=rq, run_filter=rf,
               run_bin_count=rbins, run_median_count=rmed)
    return _as_arrays(res, diploid, mean_coverage, int(kept.sum()))


# ---------------------------------------------------------------------------------------------------------------- the file side of the caller (readers, CNV type, genotypes)
INT_MAX = 2**31 - 1


def merge_in(a, s):
    """CanvasSegment.MergeIn (CanvasSegment.cs:318-334) on _Seg objects, confidence intervals included"""
    if s.begin < a.begin:
        a.start_ci = s.start_ci; a.begin = s.begin; a.counts = s.counts + a.counts; a.freqs = s.freqs + a.freqs; a.cover = s.cover + a.cover
    if s.end > a.end:
        a.end_ci = s.end_ci; a.end = s.end; a.counts = a.counts + s.counts; a.freqs = a.freqs + s.freqs; a.cover = a.cover + s.cover


def _half_length(begin, end):
    """(int)Math.Round(Length / 2.0, MidpointRounding.AwayFromZero) of a bin (Segments.cs:95-98)"""
    return (end - begin + 1) // 2


def read_segments(lines):
    """Segments.ReadSegments (Segments.cs:52-144): rows chr, start, end, count, segment id; bins grouped by adjacent chromosome, then by adjacent segment id; the start
    (end) interval reaches half the previous (next) bin of the chromosome back (forward) when that bin touches this one.  Returns _Seg objects with start_ci / end_ci."""
    rows = [l.rstrip("\n").split("\t") for l in lines if l.strip()]
    by_chr, seen = [], set()
    for r in rows:
        if not by_chr or by_chr[-1][0] != r[0]:
            if r[0] in seen:
                raise ValueError("chromosome %s comes back" % r[0])
            seen.add(r[0]); by_chr.append((r[0], []))
        by_chr[-1][1].append((int(r[1]), int(r[2]), F32(r[3]), r[4]))
    out = []
    for chrom, bins in by_chr:
        groups = []
        for b in bins:
            if not groups or groups[-1][-1][3] != b[3]:
                groups.append([])
            groups[-1].append(b)
        for g, grp in enumerate(groups):
            first, last = grp[0], grp[-1]
            prev = groups[g - 1][-1] if g > 0 else None
            nxt = groups[g + 1][0] if g + 1 < len(groups) else None
            h = _half_length(first[0], first[1])
            start_ci = (-h, h) if prev is None or prev[1] != first[0] else (-_half_length(prev[0], prev[1]), h)
            h = _half_length(last[0], last[1])
            end_ci = (-h, h) if nxt is None or last[1] != nxt[0] else (-h, _half_length(nxt[0], nxt[1]))
            sg = _Seg(chrom, first[0], last[1], [b[2] for b in grp])
            sg.start_ci, sg.end_ci = start_ci, end_ci
            out.append(sg)
    return out


def read_frequencies(lines, intervals_by_chromosome):
    """CanvasIO.ReadFrequencies (IO.cs:134-179) on text lines: {chromosome: [(begin, end)]} -> {chromosome: [[(position, ref, alt)] per interval]}"""
    out = {c: [[] for _ in iv] for c, iv in intervals_by_chromosome.items()}
    index, prev = 0, ""
    for line in lines:
        line = line.rstrip("\n")
        if len(line) == 0 or line[0] == "#":
            continue
        col = line.split("\t")
        if col[0] != prev:
            prev, index = col[0], 0
        position, ref, alt = int(col[1]), int(col[4]), int(col[5])
        if col[0] not in intervals_by_chromosome or ref + alt < 10:
            continue
        iv = intervals_by_chromosome[col[0]]
        while index < len(iv) and not iv[index][1] > position:
            index += 1
        if index >= len(iv) or iv[index][0] > position:
            continue
        out[col[0]][index].append((position, ref, alt))
    return out


def cnv_type_and_allele_copy_numbers(cn, mcc, reference_cn):
    """CanvasSegment.GetCnvTypeAndAlleleCopyNumbers (CanvasSegment.cs:280-312); mcc None = null; INT_MAX stands for <DUP>"""
    if reference_cn > 2:
        raise ValueError("Reference copy number > 2 is not supported")
    if cn == reference_cn:
        if reference_cn == 1:
            return "REF", [1]
        if reference_cn == 2 and mcc is not None:
            return ("LOH", [0, 2]) if mcc == 2 else ("REF", [1, 1])
        return "REF", [-1] * max(1, reference_cn)
    if cn > reference_cn:
        if reference_cn == 1:
            return "GAIN", [cn]
        if reference_cn == 2:
            return ("GAIN", [cn - mcc, mcc]) if mcc is not None else ("GAIN", [-1, INT_MAX])
        return "GAIN", [-1] * max(1, reference_cn)
    return ("LOSS", [0] * reference_cn) if cn == 0 else ("LOSS", [0, 1])


def alt_cn_header_lines(max_copy_number=5):
    """CanvasSegmentWriter.WriteHeaderAllAltCnTags"""
    return ['##ALT=<ID=CN%d,Description="Copy number allele: %d copies">' % (k, k) for k in range(max_copy_number + 1) if k != 1]


def alt_alleles_and_genotypes(sample_allele_copy_numbers):
    """CanvasSegmentWriter.GetAltAllelesAndGenotypes: (ALT column, one genotype per sample)"""
    uniq = sorted({x for a in sample_allele_copy_numbers for x in a if x not in (1, -1)})
    names = ["<DUP>" if x == INT_MAX else "<CN%d>" % x for x in uniq]
    genotypes = []
    for a in sample_allele_copy_numbers:
        g = ["0" if x == 1 else "." if x == -1 else str(uniq.index(x) + 1) for x in a]
        genotypes.append("/".join(sorted(g, key=lambda t: -1 if t == "." else int(t))))
    return (",".join(names) if names else "."), genotypes


def cnv_size_filter(size):
    """CanvasFilter.GetCnvSizeFilter"""
    if size % 1000000 == 0:
        return "L%dMb" % (size // 1000000)
    if size % 1000 == 0:
        return "L%dkb" % (size // 1000)
    return "L%dbp" % size


def reference_copy_number(ploidy_by_chromosome, chrom, begin, end):
    """PloidyInfo.GetReferenceCopyNumber (PloidyInfo.cs:56-109): ploidy intervals are (one-based start, end, ploidy); the query is the segment's bases Begin + 1 .. End"""
    if chrom not in ploidy_by_chromosome:
        return 2
    counts = [0] * 5
    counts[2] = end - begin
    for start, stop, ploidy in ploidy_by_chromosome[chrom]:
        if ploidy == 2:
            continue
        overlap_start = max(begin, start - 1)
        if overlap_start > stop:
            continue
        bases = min(end, stop) - overlap_start
        if bases <= 0:
            continue
        counts[2] -= bases
        counts[ploidy] += bases
    best, ref = 0, 2
    for k, c in enumerate(counts):
        if c > best:
            best, ref = c, k
    return ref


# ---------------------------------------------------------------------------------------------------------------- the written files (CanvasSegmentWriter.cs, CanvasSegment.cs:557-747)
from decimal import Decimal, ROUND_HALF_UP


def f2(v, digits=15):
    """.NET Core 2.x "F2": the value to `digits` significant digits (15 for a double, 7 for a float), then half-up at two decimals"""
    d = Decimal("%.*e" % (digits - 1, float(v)))
    s = str(d.quantize(Decimal("0.01"), rounding=ROUND_HALF_UP))
    return "0.00" if s in ("-0.00", "0.00") else s


def g15(v):
    s = "%.15g" % v
    assert "e" not in s, s
    return s


VCF_FIXED_HEADER = [
    '##ALT=<ID=DUP,Description="Region of elevated copy number relative to the reference">'] + alt_cn_header_lines() + [
    '##FILTER=<ID=q10,Description="Quality below 10">',
    '##FILTER=<ID=FailedFT,Description="Sample-level filter failed in all the samples">',
    '##INFO=<ID=CIEND,Number=2,Type=Integer,Description="Confidence interval around END for imprecise variants">',
    '##INFO=<ID=CIPOS,Number=2,Type=Integer,Description="Confidence interval around POS for imprecise variants">',
    '##INFO=<ID=CNVLEN,Number=1,Type=Integer,Description="Number of reference positions spanned by this CNV">',
    '##INFO=<ID=END,Number=1,Type=Integer,Description="End position of the variant described in this record">',
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
    '##INFO=<ID=SUBCLONAL,Number=0,Type=Flag,Description="Subclonal variant">',
    '##INFO=<ID=COMMONCNV,Number=0,Type=Flag,Description="Common CNV variant identified from pre-specified bed intervals">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##FORMAT=<ID=RC,Number=1,Type=Float,Description="Mean counts per bin in the region">',
    '##FORMAT=<ID=BC,Number=1,Type=Float,Description="Number of bins in the region">',
    '##FORMAT=<ID=CN,Number=1,Type=Integer,Description="Copy number genotype for imprecise events">',
    '##FORMAT=<ID=MCC,Number=1,Type=Integer,Description="Major chromosome count (equal to copy number for LOH regions)">',
    '##FORMAT=<ID=MCCQ,Number=1,Type=Float,Description="Major chromosome count quality score">',
    '##FORMAT=<ID=QS,Number=1,Type=Float,Description="Phred-scaled quality score. If CN is reference then this is -10log10(prob(variant)) otherwise this is -10log10(prob(no variant).">',
    "##FORMAT=<ID=FT,Number=1,Type=String,Description=\"Sample filter, 'PASS' indicates that all filters have passed for this sample\">"]


def vcf_header(version, ref_folder, contigs, sample, ploidy_and_coverage=None):
    out = ["##fileformat=VCFv4.1", "##source=Canvas " + version, "##reference=%s/genome.fa" % ref_folder]
    if ploidy_and_coverage is not None:
        out += ["##OverallPloidy=" + f2(ploidy_and_coverage[0]), "##DiploidCoverage=" + f2(ploidy_and_coverage[1])]
    out += ["##contig=<ID=%s,length=%d>" % c for c in contigs] + VCF_FIXED_HEADER
    return out + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]


class _Run:
    pass


def files_from_text(partitioned, vaf, contigs, version, ref_folder, sample="SAMPLE", ploidy=None, logistic=LOGISTIC_GERMLINE):
    """what CallVariants writes for these inputs: (VCF text, CoverageAndVariantFrequency text).  partitioned / vaf: lists of lines; contigs: [(name, length)] of GenomeSize.xml;
    ploidy: {chromosome: [(one-based start, end, ploidy)]} or None"""
    segs = read_segments(partitioned)
    if not segs:
        return "\n".join(vcf_header(version, ref_folder, contigs, sample)) + "\n", None
    chroms = []
    for s in segs:
        if s.chr not in chroms:
            chroms.append(s.chr)
    cso = [0] + [sum(1 for s in segs if chroms.index(s.chr) <= c) for c in range(len(chroms))]
    sites = read_frequencies(vaf, {c: [(s.begin, s.end) for s in segs if s.chr == c] for c in chroms})
    per_seg = [x for c in chroms for x in sites[c]]
    raw = {c: [] for c in chroms}
    for line in vaf:
        t = line.rstrip("\n").split("\t")
        if line.strip() and line[0] != "#" and t[0] in raw:
            raw[t[0]].append((int(t[1]), int(t[4]), int(t[5])))
    flat = [x for c in chroms for x in raw[c]]
    csi = [0] + list(np.cumsum([len(raw[c]) for c in chroms]))
    counts = np.array([v for s in segs for v in s.counts], F32)
    sbo = np.concatenate([[0], np.cumsum([len(s.counts) for s in segs])])
    d = direct(counts, cso, [s.begin for s in segs], [s.end for s in segs], sbo, csi, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat], logistic)
    runs = []
    for k in range(len(d["run_first"])):
        f, l = int(d["run_first"][k]), int(d["run_last"][k])
        r = _Run()
        r.chr, r.begin, r.end, r.cn, r.mcc, r.q, r.filter = segs[f].chr, segs[f].begin, segs[l].end, int(d["run_cn"][k]), int(d["run_mcc"][k]), int(d["run_qscore"][k]), int(d["run_filter"][k])
        r.counts = [v for s in segs[f:l + 1] for v in s.counts]
        r.sites = [x for ps in per_seg[f:l + 1] for x in ps]
        r.med, r.start_ci, r.end_ci = float(d["run_median_count"][k]), segs[f].start_ci, segs[l].end_ci
        runs.append(r)
    dip = d["diploid_coverage"]
    # ---- VCF
    w = sum(r.end - r.begin for r in runs if r.filter == 0)
    pc = (sum(float(r.cn * (r.end - r.begin)) for r in runs if r.filter == 0) / w, dip) if w > 0 else None
    lines = vcf_header(version, ref_folder, contigs, sample, pc)
    for name, _ in contigs:
        for r in runs:
            if r.chr.lower() != name.lower():
                continue
            ref_cn = reference_copy_number(ploidy, r.chr, r.begin, r.end) if ploidy is not None else 2
            kind, alleles = cnv_type_and_allele_copy_numbers(r.cn, None if r.mcc < 0 else r.mcc, ref_cn)
            alt, gts = alt_alleles_and_genotypes([alleles])
            pos = r.begin if alt.startswith("<") and alt.endswith(">") else r.begin + 1
            ft = ";".join(n for bit, n in ((1, "q10"), (2, cnv_size_filter(10000))) if r.filter & bit) or "PASS"
            info = ("" if kind == "REF" else "SVTYPE=%s;" % ("LOH" if kind == "LOH" else "CNV")) + "END=%d" % r.end + ("" if kind == "REF" else ";CNVLEN=%d" % (r.end - r.begin))
            info += ";CIPOS=%d,%d;CIEND=%d,%d" % (r.start_ci + r.end_ci)
            lines.append("\t".join([r.chr, str(pos), "Canvas:%s:%s:%d-%d" % (kind, r.chr, r.begin + 1, r.end), "N", alt, f2(r.q), "PASS" if r.filter == 0 else "FailedFT", info,
                                    "GT:RC:BC:CN:MCC:MCCQ:QS:FT", ":".join([gts[0], f2(r.med), str(len(r.counts)), str(r.cn), "." if r.mcc < 0 else str(r.mcc), ".", f2(r.q), ft])]))
    # ---- coverage file
    total_bins = sum(len(r.counts) for r in runs); total_len = sum(r.end - r.begin for r in runs)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = F32(0.25) * F32(total_bins) / F32(total_len // 100000)
    min_bins = max(1, int(v) if np.isfinite(v) else INT_MIN)
    out = ["#Chromosome\tStart\tEnd\tCopyNumber\tMajorChromosomeCount\tMedianHits\tNormalizedCoverage\tMedianMinorAlleleFrequency\tReferencePloidy\t" + "".join("VariantFrequencyBin%d\t" % i for i in range(100))]
    for name, length in contigs:
        mine = [r for r in runs if r.chr == name]
        if not mine:
            continue
        for start in range(0, length, 100000):
            end = min(length, start + 100000)
            by_pair, by_cn, overlap = {}, {}, []
            for r in mine:
                if r.begin > end or r.end < start:
                    continue
                wgt = min(r.end, end) - max(r.begin, start)
                by_pair[(r.cn, r.mcc)] = by_pair.get((r.cn, r.mcc), 0) + wgt
                by_cn[r.cn] = by_cn.get(r.cn, 0) + wgt
                overlap.append(r)
            best, major = 0, 0
            for k, wv in by_cn.items():
                if wv > best:
                    best, major = wv, k
            cand = sorted([(k, wv) for k, wv in by_pair.items() if k[0] == major], key=lambda t: -t[1])
            major_mcc = cand[0][0][1] if cand else -1
            cnts, maf, vf = [], [], []
            for r in overlap:
                if (major == 2 and r.cn != 2) or (major < 2 and r.cn >= 2) or (major > 2 and r.cn <= 2):
                    continue
                ln = r.end - r.begin

                def cut(n):
                    i0 = int(F32(n) * F32(start - r.begin) / F32(ln)) if start > r.begin else 0
                    i1 = int(F32(n) * F32(end - r.begin) / F32(ln)) if end < r.end else n
                    return i0, i1
                i0, i1 = cut(len(r.counts)); cnts += r.counts[i0:max(i0, i1)]
                i0, i1 = cut(len(r.sites))
                for p, rf, al in r.sites[i0:max(i0, i1)]:
                    vf.append(F32(al) / F32(rf + al)); maf.append(F32(1) - F32(max(rf, al) / (rf + al)))
            line = "%s\t%d\t%d\t" % (name, start, end)
            if len(cnts) >= min_bins:
                hits = float(sorted(cnts)[len(cnts) // 2])
                line += "%d\t%s\t%s\t%s\t" % (major, "" if major_mcc < 0 else str(major_mcc), f2(hits), f2(2 * hits / dip))
                line += (g15(_median_sorted_list(maf, False)) if len(maf) >= 10 else "") + "\t"
                ref_ploidy = 2
                for st, en, pl in (ploidy or {}).get(name, []):
                    if st - 1 <= end and en >= start:
                        ref_ploidy = pl
                line += "%d\t" % ref_ploidy
                if len(vf) >= 10:
                    hist = np.zeros(100, F32)
                    for x in vf:
                        hist[min(99, int(math.floor(float(x) / 0.01)))] += F32(1)
                    line += "".join(f2(h / F32(len(vf)) * F32(100), 7) + "\t" for h in hist)
                else:
                    line += "\t" * 100
            out.append(line)
    return "\n".join(lines) + "\n", "\n".join(out) + "\n"
