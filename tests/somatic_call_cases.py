"""Cases for canvas_call_somatic (tests/test_somatic_call_ref.py, tests/test_somatic_call_gpu.py).  Every case is small: tens of segments, 10^2 - 10^4 bins, a few thousand
sites, a median level near 20 (diploid coverage 20, purity 100 %: copy number c sits at a count of 10 c).  Most cases narrow the purity range (minimum_purity_hard_limit 95)
so that the restatements' fit stays short; `whole grid` keeps the reference's 20 (coverages 10 .. 47, about 3 000 models).  Each case names the edge it is there for; the
CPU test asserts that the restatements really take it."""
import functools

import numpy as np

import somatic_call_ref as CR

GENOME = 3_000_000_000
BIG = 60000                                                   # a segment the merges leave alone (MinimumCallSize 50 000)
MAF_OF_CN = {0: 0.02, 1: 0.03, 2: 0.41, 3: 0.32, 4: 0.25}      # what AdjustedMAF expects near coverage 20 at purity 100 %
FAST = dict(minimum_purity_hard_limit=95)


def seg(length=BIG, bins=100, cn=2, sites=60, gap=0, ref_cn=2, counts=None, maf=None, depth=40):
    return dict(length=length, bins=bins, cn=cn, sites=sites, gap=gap, ref_cn=ref_cn, counts=counts, maf=maf, depth=depth)


def alternating(v, bins):
    """v, v + 1, v, v + 1 ...: the two middle values of an even number of bins are v and v + 1"""
    return np.array([v + (i & 1) for i in range(bins)], np.float32)


def build(chroms, params=None, excluded=None, genome_length=GENOME):
    counts, beg, end, bins, ref_cn, pos, ref, alt = [], [], [], [], [], [], [], []
    cso, csi = [0], [0]
    k = 0
    for chrom in chroms:
        at = 1000
        for sp in chrom:
            b = at + sp["gap"]
            e = b + sp["length"]
            at = e
            v = 10 * sp["cn"]
            c = sp["counts"]
            if c is None:
                c = np.array([(v + ((i * 7 + k * 3) % 5 - 2)) if v >= 10 else (i & 1) for i in range(sp["bins"])], np.float32)
            c = np.asarray(c, np.float32)
            assert len(c) == sp["bins"]
            counts.append(c); beg.append(b); end.append(e); bins.append(len(c)); ref_cn.append(sp["ref_cn"])
            n = sp["sites"]
            if n:
                maf = MAF_OF_CN.get(sp["cn"], 0.3) if sp["maf"] is None else sp["maf"]
                step = max(1, (sp["length"] - 2) // n)
                for j in range(n):
                    a = int(round(sp["depth"] * maf)) + ((j * 5 + k) % 3 - 1)
                    a = min(max(a, 0), sp["depth"])
                    if j & 1:
                        a = sp["depth"] - a                          # the other allele: folded back by the caller
                    pos.append(b + 1 + j * step); alt.append(a); ref.append(sp["depth"] - a)
            k += 1
        cso.append(k); csi.append(len(pos))
    case = dict(counts=np.concatenate(counts), chr_seg_offset=np.array(cso, np.int64), seg_begin=np.array(beg, np.int32), seg_end=np.array(end, np.int32),
                seg_bin_offset=np.concatenate([[0], np.cumsum(bins)]).astype(np.int64), chr_site_offset=np.array(csi, np.int64), site_pos=np.array(pos, np.int32),
                site_ref=np.array(ref, np.int32), site_alt=np.array(alt, np.int32), seg_ref_cn=np.array(ref_cn, np.int32), genome_length=genome_length,
                params=dict(FAST, **(params or {})))
    if excluded is not None:
        case["excluded"] = [(np.asarray(e[0], np.int32), np.asarray(e[1], np.int32)) for e in excluded]
    return case


PATTERN = (2, 2, 1, 2, 3, 2, 2, 4, 2, 1, 2, 3)


def autosomes(sites=60, n=2, **kw):
    return [[seg(cn=c, sites=sites, **kw) for c in PATTERN] for _ in range(n)]


def base_case(params=None, sites=60):
    return build(autosomes(sites), params)


def whole_grid_case():
    """the reference's minimum_purity_hard_limit 20 and a minor allele coverage that lets every coverage reach it: coverages 10 .. 47 times purities 20 .. 100, 3 078 models"""
    return build(autosomes(), dict(minimum_purity_hard_limit=20, min_minor_allele_coverage=17.0))


def site_count_case():
    """segments of 4 999 and 5 000 bases; 0, 9, 10, 49 and 50 frequencies"""
    extra = [seg(length=4999, bins=9, sites=60), seg(length=5000, bins=10, sites=60), seg(sites=0), seg(sites=9), seg(sites=10), seg(sites=49), seg(sites=50), seg(cn=3, sites=9)]
    return build(autosomes() + [extra])


def coverage_cut_case():
    """a coverage exactly 2 q2 is kept, the next float above it is dropped (coverages are floats widened, so that is the next value a coverage can take)"""
    plain = build(autosomes())
    q2 = float(CR._quartiles_item2(plain["counts"]))
    keep, drop = np.float32(2 * q2), np.nextafter(np.float32(2 * q2), np.float32(np.inf))
    assert float(keep) == 2 * q2
    extra = [seg(cn=4, counts=np.full(100, keep, np.float32)), seg(cn=4, counts=np.full(100, drop, np.float32)), seg(cn=1, bins=200)]      # (200 bins below the median balance them)
    case = build(autosomes() + [extra])
    assert float(CR._quartiles_item2(case["counts"])) == q2                               # both sit above the median: it has not moved
    return case


def threshold_case(sites):
    """40 frequencies everywhere: the loop ends at 35; 25: at 20"""
    return build(autosomes(sites))


def threshold_gives_up_case():
    """only 10 segments have frequencies at all: 50, 35, 20, 5 and the loop gives up"""
    chroms = autosomes(0)
    for sp in chroms[0][:10]:
        sp["sites"] = 60
    return build(chroms)


def usable_count_case(n):
    """exactly n usable segments (the others are shorter than 5 000 bases)"""
    chrom = [seg(cn=c, length=BIG if i < n else 4000, bins=100 if i < n else 8) for i, c in enumerate((2, 1, 3, 2, 2, 2))]
    return build([chrom])


def half_case(v, odd_overall):
    """the bins of the usable segments at reference copy number 2 are v c / 2 and v c / 2 + 1 alternating, copy numbers 1 and 3 balanced: the median level is v + 0.5.
    An unusable short segment makes the subset non-contiguous, and (odd_overall) one more bin makes the total of the first Quartiles call odd"""
    chrom = []
    for i, c in enumerate((2, 1, 2, 3, 2, 2, 1, 3, 2, 2)):
        chrom.append(seg(cn=c, counts=alternating(v * c // 2, 100)))
        if i == 4:
            chrom.append(seg(length=4000, bins=7 if odd_overall else 8, cn=2, sites=5))
    return build([chrom, [seg(cn=c, counts=alternating(v * c // 2, 100)) for c in (2, 1, 3, 2, 2, 2, 1, 3, 2, 2, 2, 2, 2, 2)]])


def odd_level_case():
    """an odd number of bins in the second Quartiles call"""
    chroms = autosomes()
    chroms[0][0]["bins"] = 101
    return build(chroms)


def reference_cn_case():
    """a chromosome at reference copy number 1 (the haploid columns) and a segment at 0, which stays out of stage 3 and is still called"""
    x = [seg(cn=1, ref_cn=1, sites=4), seg(cn=2, ref_cn=1, sites=12, maf=0.02), seg(cn=1, ref_cn=1, sites=0)]
    y = [seg(cn=0, ref_cn=0, sites=0), seg(cn=1, ref_cn=0, sites=3)]
    return build(autosomes() + [x, y])


def tie_case():
    """a segment without a MAF (two ploidies of its copy number share their coverage: best and runner-up distances are equal) and an unusable one midway between two points"""
    extra = [seg(cn=2, sites=3), seg(length=4000, bins=8, sites=0, counts=np.full(8, 15, np.float32)), seg(cn=4, sites=0)]
    return build(autosomes() + [extra], dict(user_purity=1.0))           # purity exactly 1: copy numbers 1 and 2 sit at 10 and 20, and 15 is midway


def spread_counts(n=5000):
    """counts whose serial double sum in bin order rounds to another float than their sum in any other order.  Bin 0 holds 2^38, so every later addition of the serial
    loop rounds to a multiple of 2^-14 and drops the 2^-17 of a count of 80 + 2^-17: the serial total is 2^38 + 25 * 2^14 - 2^-6 exactly, just BELOW the midpoint of the
    two floats 2^38 + 24 * 2^14 and 2^38 + 26 * 2^14 (bin 1 is chosen for that).  The exact total is 4 998 * 2^-17 = 0.038 larger, just ABOVE the midpoint, and so is
    every sum that adds most of the small counts to each other before it meets 2^38.  55 bits lie between the largest and the smallest set bit"""
    small = np.float32(80) + np.float32(2.0 ** -17)
    c = np.full(n, small, np.float32)
    c[0] = np.float32(2.0 ** 38)
    adjust = 25 * 2 ** 14 - 2.0 ** -6 - (n - 2) * 80.0
    c[1] = np.float32(adjust)
    assert float(c[1]) == adjust and float(small) == 80 + 2.0 ** -17 and 0 < adjust
    return c


def high_cn_case():
    """segments whose best ploidy is MaximumCopyNumber (8): a mean of 80 (estimate 8, kept), 90 (9), 85 (8.5 -> 8), 95 (9.5 -> 10), one of 5 000 bins whose serial sum is
    not the sum in any other order, one of 150 for a copy number >= 15 (the amplification term of the q-score)"""
    flat = lambda v, n=100: np.full(n, v, np.float32)
    extra = [seg(cn=8, counts=flat(80), sites=0), seg(cn=8, counts=flat(90), sites=0), seg(cn=8, counts=flat(85), sites=20, maf=0.2), seg(cn=8, counts=flat(95), sites=0),
             seg(cn=8, bins=5000, counts=spread_counts(), sites=0), seg(cn=8, counts=flat(150), sites=0)]
    low = [seg(cn=1, length=4000, bins=5400, sites=0)]          # keeps overallMedianCoverage at copy number 2; too short to be usable
    return build(autosomes() + [extra, low], dict(user_purity=1.0))      # purity 100 / 100f = 1 exactly: the estimate is 2 MeanCount / DiploidCoverage


def big_segment_case():
    """one segment of more than 8 192 bins: the tiled select class runs inside the call"""
    chroms = autosomes()
    chroms[1][3] = seg(cn=2, bins=9001, length=4 * BIG)
    return build(chroms)


def merge_layout(enrichment, lead=False, span=1):
    """short segments (below MinimumCallSize) in every position the merges treat differently.  Not enrichment: neighbours are cut off by excluded intervals; enrichment: by a
    gap of more than merge_span.  At span 1 a short segment never sees past a short neighbour (that neighbour is the gap), so the chain of short segments assimilated
    forwards needs a span above their 20 000 bases: 30 000"""
    S = lambda cn=2, gap=0, **kw: seg(length=20000, bins=30, cn=cn, gap=gap, **kw)
    L = lambda cn=2, gap=0, **kw: seg(cn=cn, gap=gap, **kw)
    far = 5000
    a = [S(3), L(2), S(1), L(2), L(2), S(3), S(1), S(4), L(3), L(3, gap=far), S(1, gap=far), L(2), S(2), L(1, gap=far), L(1), S(3), S(3)]
    b = [S(1), S(3), L(2), L(2, gap=1), L(2, gap=2), S(2), L(4), S(1, gap=far), S(2, gap=far)]
    if lead:
        a = [L(4)] + a                                          # the short segment behind it has segment 0 as its only large predecessor
    c = [seg(length=8000, bins=12, cn=3)]
    chroms = [a, b, c] + autosomes(n=1)
    case = build(chroms, dict(is_enrichment=int(enrichment), merge_span=span))
    if not enrichment:
        beg, end = case["seg_begin"], case["seg_end"]
        gaps = [(int(end[i - 1]), int(beg[i])) for i in range(1, len(a)) if beg[i] - end[i - 1] == far]
        # one interval inside the gap between two large segments of one call, one that only touches the gap behind a short segment with its stop, one inside the gap ahead of a short segment
        ex_a = ([gaps[0][0] + 10, gaps[1][0] - 500, gaps[2][0] + 7], [gaps[0][0] + 20, gaps[1][0], gaps[2][0] + 9])
        nb0 = len(a)
        gb = [(int(end[nb0 + i - 1]), int(beg[nb0 + i])) for i in range(1, len(b)) if beg[nb0 + i] - end[nb0 + i - 1] == far]
        ex_b = ([gb[0][0] + 100], [gb[0][0] + 200])
        case["excluded"] = [(np.array(ex_a[0], np.int32), np.array(ex_a[1], np.int32)), (np.array(ex_b[0], np.int32), np.array(ex_b[1], np.int32)),
                            (np.zeros(0, np.int32), np.zeros(0, np.int32)), (np.zeros(0, np.int32), np.zeros(0, np.int32))]
    return case


def filter_case():
    """both filter bits, alone and together: a lone run shorter than 10 kb with few bins (3), one with so many bins that its q-score passes (2), runs with q below the
    threshold (1), and runs that pass"""
    return build(autosomes() + [[seg(length=8000, bins=3, cn=3, sites=0)], [seg(length=9000, bins=2, cn=1, sites=0), seg(cn=2, gap=70000)], [seg(length=9500, bins=4000, cn=2, sites=0)]],
                 dict(quality_filter_threshold=7))


def snv_case(purity, snv=0.77):
    """an all-diploid sample at a user purity: 0.4 lets the SNV estimate override, 0.6 does not"""
    chroms = [[seg(cn=2) for _ in range(12)] for _ in range(2)]
    chroms[0][5] = seg(cn=3, length=BIG // 2, bins=50)
    return build(chroms, dict(user_purity=purity, snv_purity_estimate=snv))


def few_segments_case():
    return usable_count_case(2)


def no_reference_two_case():
    """no usable segment at reference copy number 2: CANVAS_ERR_INVALID after stage 2"""
    return build([[seg(cn=1, ref_cn=1) for _ in range(5)]])


def low_level_case():
    """a median level of 0: the reference divides the coverage weighting by it"""
    return build([[seg(cn=2, counts=np.full(100, 0.25, np.float32)) for _ in range(5)]])


def no_model_case():
    """MaxAllowedPloidy below every model's ploidy: the fit's own code passes through with stages 1 - 3 filled"""
    return base_case(dict(max_allowed_ploidy=0.6))


CASES = {
    "base": base_case,
    "whole grid": whole_grid_case,
    "site counts": site_count_case,
    "coverage cut": coverage_cut_case,
    "threshold 35": lambda: threshold_case(40),
    "threshold 20": lambda: threshold_case(25),
    "threshold gives up": threshold_gives_up_case,
    "3 usable": lambda: usable_count_case(3),
    "level 20.5": lambda: half_case(20, False),
    "level 21.5 odd overall": lambda: half_case(21, True),
    "odd level total": odd_level_case,
    "reference copy number": reference_cn_case,
    "ties": tie_case,
    "high copy number": high_cn_case,
    "big segment": big_segment_case,
    "evenness above": lambda: base_case(dict(evenness_score=95.0)),
    "evenness between": lambda: base_case(dict(evenness_score=91.0)),
    "evenness below": lambda: base_case(dict(evenness_score=80.0)),
    "user purity": lambda: base_case(dict(user_purity=0.97)),
    "user ploidy": lambda: base_case(dict(user_ploidy=2.1)),
    "merges": lambda: merge_layout(False),
    "merges enrichment": lambda: merge_layout(True),
    "merges behind segment 0": lambda: merge_layout(False, True),
    "merges enrichment behind segment 0": lambda: merge_layout(True, True),
    "merges enrichment span 30000": lambda: merge_layout(True, False, 30000),
    "filters": filter_case,
    "snv overrides": lambda: snv_case(0.4),
    "snv does not override": lambda: snv_case(0.6),
}
ERROR_CASES = {"2 usable": few_segments_case, "no reference 2": no_reference_two_case, "level 0": low_level_case, "no model": no_model_case}


@functools.lru_cache(maxsize=None)
def built(name):
    return (CASES.get(name) or ERROR_CASES[name])()


_FITS = {}


def shared_fit(fc):
    """somatic_ref.fit_vectorised, computed once per distinct input: both restatements hand it the arrays of their own stage 2, and equal arrays share one fit"""
    import somatic_ref as R
    key = (fc["coverage"].tobytes(), fc["maf"].tobytes(), fc["weight"].tobytes(), fc["length"].tobytes(), repr(sorted((k, v) for k, v in fc.items() if not isinstance(v, np.ndarray) and k != "params")),
           repr(sorted(fc["params"].items())))
    if key not in _FITS:
        try:
            _FITS[key] = (R.fit_vectorised(fc), None)
        except (R.NoModel, R.NoScore) as e:
            _FITS[key] = (None, e)
    res, err = _FITS[key]
    if err is not None:
        raise type(err)(*err.args)
    return res


def _catch(fn, case):
    import somatic_ref as R
    try:
        return fn(case, fit=shared_fit)
    except (CR.FewSegments, CR.Invalid, R.NoModel, R.NoScore) as e:
        return e


@functools.lru_cache(maxsize=None)
def literal(name):
    return _catch(CR.literal, built(name))


@functools.lru_cache(maxsize=None)
def arrays(name):
    return _catch(CR.arrays, built(name))
