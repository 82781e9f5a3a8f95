"""Two independent restatements of what canvas_call_somatic computes around the model fit (CanvasSomaticCaller/SomaticCaller.cs CallVariants, :366-476): the usable segments
and the threshold loop (stage 2), the median level, weighting factor and grid bounds (stage 3), AssignPloidyCalls with the MaximumCopyNumber rule (stage 5), and the host
tail: Logistic q-scores, the two merges, filters, EstimateChromosomeCount, SelectPurityEstimate (stage 6).  The fit itself (stage 4) and the model points come from
tests/somatic_ref.py.

  literal  (a) follows the C# statement by statement: lists, the reference's loops, segment objects that MergeIn mutates.
  arrays   (b) written separately: numpy for the per-segment stages (searchsorted, sorts of slices, a distance matrix whose rows give best and runner-up from the
           minimum and the rule for equals), index arrays and a parent table for the merges, np.add.accumulate for the ordered sums.

A case is a dict: counts (float32), chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt, genome_length, and optionally
seg_ref_cn, excluded (per chromosome (starts, stops)), params (overrides of CALL_DEFAULTS and somatic_ref.DEFAULTS).  Both return the dict Canvas.call_somatic returns (without
seg_mean_route, which is the device's choice; `mean_needed` says where MeanCount was read).  FewSegments / Invalid / somatic_ref.NoModel / NoScore carry .partial."""
import math

import numpy as np

import somatic_ref as R

F32 = np.float32
INT_MIN = -2**31
DBL_MAX = 1.7976931348623157e308
CALL_DEFAULTS = dict(minimum_variant_frequencies=50, minimum_call_size=50000, quality_filter_threshold=10, merge_span=1, is_enrichment=0, minimum_purity_hard_limit=20,
                     lower_coverage_level_weighting_factor=4.0, upper_coverage_level_weighting_factor=2.355, user_purity=-1.0, user_ploidy=-1.0,
                     coverage_weighting=0.333, coverage_weighting_with_maf_segmentation=0.20, evenness_score_threshold=94.5, min_evenness_score=88.0,
                     logistic_intercept=-0.5143, logistic_log_bin_count=0.8596, logistic_model_distance=-50.4366, logistic_distance_ratio=-0.6511,
                     evenness_score=float("nan"), snv_purity_estimate=float("nan"), min_minor_allele_coverage=0.0, genome_length=0)
SEG_FLOATS = ("seg_median_count", "seg_maf_upper", "seg_coverage", "seg_maf", "seg_weight", "seg_dist", "seg_dist2", "seg_mean_count")
SCALAR_FLOATS = ("mean_coverage", "coverage_weighting_factor", "reported_purity", "purity_model_fit", "inter_model_distance", "estimated_chromosome_count",
                 "heterogeneity_proportion", "overall_median_coverage", "deviation_factor")
FIT_FIELDS = ("best_model", "best_coverage", "best_percent_purity", "info", "nmodels", "nvalid", "nscored", "diploid_coverage", "purity", "deviation", "precision_deviation",
              "accuracy_deviation", "ploidy", "percent_normal", "diploid_distance", "percent_cn", "score", "inter_model_distance", "best_deviation", "worst_allowed_deviation")


class FewSegments(Exception):
    """fewer than 3 usable segments (NotEnoughUsableSegementsException, :1636)"""


class Invalid(Exception):
    """what the reference would divide by zero or index out of range on"""


def call_params(case):
    p = dict(CALL_DEFAULTS, **{k: v for k, v in case.get("params", {}).items() if k in CALL_DEFAULTS})
    p["genome_length"] = case["genome_length"]
    for k in ("lower_coverage_level_weighting_factor", "upper_coverage_level_weighting_factor", "user_purity", "user_ploidy"):     # floats in the reference
        p[k] = F32(p[k])
    return p


def fit_params(case):
    return {k: v for k, v in case.get("params", {}).items() if k in R.DEFAULTS}


def _fit_case(case, p, cov, maf, w, length, scal, nseg):
    fp = fit_params(case)
    if nseg < 500:
        fp["deviation_factor"] = 2.0
    return dict(coverage=np.array(cov, np.float64), maf=np.array(maf, np.float64), weight=np.array(w, np.float64), length=np.array(length, np.int32),
                cwf=scal["coverage_weighting_factor"], genome_length=case["genome_length"], min_coverage=scal["min_coverage"], max_coverage=scal["max_coverage"],
                hard_limit=p["minimum_purity_hard_limit"], mmac=p["min_minor_allele_coverage"], is_enrichment=bool(p["is_enrichment"]),
                fixed_percent_purity=scal["fixed_percent_purity"], fixed_coverage=scal["min_coverage"] if p["user_ploidy"] >= 0 else -1, params=fp)


def _fit_fields(res):
    """the fields of canvas_somatic_result out of a result of somatic_ref"""
    g = lambda k, d=0.0: res.get(k, d)
    return dict(best_model=res["model"], best_coverage=g("coverage", 0), best_percent_purity=g("percent_purity", 0), info=res["info"], nmodels=res["nmodels"], nvalid=res["nvalid"],
                nscored=res["nscored"], diploid_coverage=float(g("coverage", 0)), purity=g("purity"), deviation=g("deviation"), precision_deviation=g("precision_deviation"),
                accuracy_deviation=g("accuracy_deviation"), ploidy=g("ploidy"), percent_normal=g("percent_normal"), diploid_distance=g("diploid_distance"),
                percent_cn=np.asarray(g("percent_cn", np.zeros(0)), np.float64), score=g("score"), inter_model_distance=g("inter_model_distance"),
                best_deviation=g("best_deviation"), worst_allowed_deviation=g("worst_allowed_deviation"))


def _wrap32(v):
    return (int(v) + 2**31) % 2**32 - 2**31


def _round_to_int(v):
    """(int)Math.Round(v): half to even; what does not fit an int becomes int.MinValue"""
    if v != v or v in (math.inf, -math.inf):
        return INT_MIN
    r = round(v)
    return r if -2**31 <= r <= 2**31 - 1 else INT_MIN


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _log10(x):
    return math.log10(x) if x > 0 else (-math.inf if x == 0 else math.nan)


# ================================================================================================================ (a) literal
class _Segment:
    def __init__(self, index, chrom, begin, end, counts, ref_cn):
        self.index, self.chr, self.begin, self.end, self.counts, self.ref_cn = index, chrom, begin, end, [F32(v) for v in counts], ref_cn
        self.bins = len(self.counts)                          # GenomicBins.Count: MergeIn concatenates
        self.frequencies, self.total_coverage = [], []
        self.cn = self.cn2 = -1
        self.mcc = None
        self.dist = self.dist2 = 0.0
        self.q = 0
        self.filter = 0                                         # PASS until SetFilterForSegments says otherwise
        self.absorbed_by = None

    @property
    def length(self):
        return self.end - self.begin

    def merge_in(self, s):
        if s.begin < self.begin:
            self.begin = s.begin
            self.bins = s.bins + self.bins
        if s.end > self.end:
            self.end = s.end
            self.bins = self.bins + s.bins
        s.absorbed_by = self


def _median_float_list(values):
    """SortedList<float>.Median(): the average of an even length in float, widened"""
    a = sorted(values)
    n = len(a)
    if n % 2 == 1:
        return float(a[n // 2])
    return float((F32(a[n // 2 - 1]) + F32(a[n // 2])) / F32(2))


def _quartiles_item2(x):
    a = sorted(F32(v) for v in x)
    n = len(a)
    mid = n // 2
    if n % 2 == 0:
        return F32((a[mid - 1] + a[mid]) / F32(2))
    return a[mid]


def _is_forbidden(chrom, start, end, excluded):
    if excluded is None:
        return False
    starts, stops = excluded[chrom]
    for st, sp in zip(starts, stops):
        if st >= start and st <= end:
            return True
        if sp >= start and sp <= end:
            return True
        if st > end:
            break
    return False


def _qscore_literal(p, seg):
    log_bins = math.log10(1 + seg.bins)
    score = p["logistic_intercept"]
    score += log_bins * p["logistic_log_bin_count"]
    score += (seg.dist / max(1.0, seg.cn - 4.0)) * p["logistic_model_distance"]
    score += (0.0 if seg.dist2 == 0 else seg.dist / seg.dist2) * p["logistic_distance_ratio"]
    score += log_bins if seg.cn >= 15 else 0.0
    score = _exp(score)
    score = score / (score + 1) if score != math.inf else math.nan
    q = _round_to_int(-10 * _log10(1 - score)) if score == score else INT_MIN
    q = min(60, q)
    return max(2, q)


def _merge_excluded(segments, minimum_call_size, excluded, events=None):
    """MergeSegmentsUsingExcludedIntervals, CanvasSegment.cs:863-951.  `events` (a set, or None) collects the names of the branches taken: it changes nothing"""
    events = set() if events is None else events
    merged = []
    i = 0
    while i < len(segments):
        if segments[i].end - segments[i].begin >= minimum_call_size:
            merged.append(segments[i])
            i += 1
            continue
        if i == 0:
            events.add("short first segment")
        prev_index, prev_q = -1, 0
        check = i - 1
        while check > 0:
            if segments[check].chr != segments[i].chr:
                events.add("chromosome change behind")
                break
            if segments[check].end - segments[check].begin < minimum_call_size:
                check -= 1
                continue
            if _is_forbidden(segments[check].chr, segments[check].end, segments[i].begin, excluded):
                events.add("excluded interval behind")
                break
            prev_index, prev_q = check, segments[check].q
            break
        if check == 0 and i > 0 and segments[0].chr == segments[i].chr and segments[0].end - segments[0].begin >= minimum_call_size and \
                not _is_forbidden(segments[0].chr, segments[0].end, segments[i].begin, excluded):
            events.add("segment 0 not looked at")
        next_index, next_q = -1, 0
        check = i + 1
        while check < len(segments):
            if segments[check].chr != segments[i].chr:
                events.add("chromosome change ahead")
                break
            if segments[check].end - segments[check].begin < minimum_call_size:
                check += 1
                continue
            if _is_forbidden(segments[check].chr, segments[i].end, segments[check].begin, excluded):
                events.add("excluded interval ahead")
                break
            next_index, next_q = check, segments[check].q
            break
        if prev_q > 0 and prev_q == next_q:
            events.add("equal q-scores")
        if prev_q > 0 and prev_q >= next_q:
            events.add("merged backwards")
            segments[prev_index].merge_in(segments[i])
            i += 1
            continue
        if next_q > 0:
            events.add("merged forwards")
            if next_index - i >= 2:
                events.add("chain merged forwards")
            for t in range(i, next_index):
                segments[next_index].merge_in(segments[t])
            i = next_index
            continue
        events.add("short segment kept")
        merged.append(segments[i])
        i += 1
    segments = merged
    merged = []
    last = segments[0]
    merged.append(last)
    i = 1
    while i < len(segments):
        if last.cn == segments[i].cn and last.chr == segments[i].chr and _is_forbidden(last.chr, last.end, segments[i].begin, excluded):
            events.add("equal calls across an excluded interval")
        if last.cn == segments[i].cn and last.chr == segments[i].chr and not _is_forbidden(last.chr, last.end, segments[i].begin, excluded):
            events.add("equal calls merged")
            last.merge_in(segments[i])
            i += 1
            continue
        last = segments[i]
        merged.append(segments[i])
        i += 1
    return merged


def merge_segments(segments, minimum_call_size=0, maximum_merge_span=10000, events=None):
    """MergeSegments without copyNumbers / qscores, CanvasSegment.cs:961-1075"""
    events = set() if events is None else events
    merged = []
    if not segments:
        return merged
    i = 0
    while i < len(segments):
        if segments[i].end - segments[i].begin >= minimum_call_size:
            merged.append(segments[i])
            i += 1
            continue
        if i == 0:
            events.add("short first segment")
        prev_index, prev_q = -1, -1
        check = i - 1
        while check >= 0:
            if segments[check].chr != segments[i].chr:
                events.add("chromosome change behind")
                break
            if segments[check].end - segments[check].begin < minimum_call_size:
                check -= 1
                continue
            if segments[i].begin - segments[check].end > maximum_merge_span:
                events.add("gap behind")
                break
            prev_index, prev_q = check, segments[check].q
            if check == 0:
                events.add("segment 0 looked at")
            break
        next_index, next_q = -1, -1
        check = i + 1
        while check < len(segments):
            if segments[check].chr != segments[i].chr:
                events.add("chromosome change ahead")
                break
            if segments[check].end - segments[check].begin < minimum_call_size:
                check += 1
                continue
            if segments[check].begin - segments[i].end > maximum_merge_span:
                events.add("gap ahead")
                break
            next_index, next_q = check, segments[check].q
            break
        if prev_q >= 0 and prev_q == next_q:
            events.add("equal q-scores")
        if prev_q >= 0 and prev_q >= next_q:
            events.add("merged backwards")
            segments[prev_index].merge_in(segments[i])
            i += 1
            continue
        if next_q >= 0:
            events.add("merged forwards")
            if next_index - i >= 2:
                events.add("chain merged forwards")
            t = next_index - 1
            while i <= t:
                segments[next_index].merge_in(segments[t])
                t -= 1
            i = next_index
            continue
        events.add("short segment kept")
        merged.append(segments[i])
        i += 1
    segments = merged
    merged = []
    last = segments[0]
    merged.append(last)
    i = 1
    while i < len(segments):
        if last.cn == segments[i].cn and last.chr == segments[i].chr and not segments[i].begin - last.end < maximum_merge_span:
            events.add("equal calls across a gap")
        if last.cn == segments[i].cn and last.chr == segments[i].chr and segments[i].begin - last.end < maximum_merge_span:
            events.add("equal calls merged")
            last.merge_in(segments[i])
            i += 1
            continue
        last = segments[i]
        merged.append(segments[i])
        i += 1
    return merged


def usable_segments_literal(segments, is_enrichment, minimum_variant_frequencies, out=None):
    """GetUsableSegmentsAndSourcesForModeling (:1432-1493) with overallMedianCoverage = null; returns [(segment, coverage, maf, weight)] and the median"""
    temp = []
    for segment in segments:
        if is_enrichment:
            temp.append(F32(_median_float_list(segment.counts)))
        else:
            for value in segment.counts:
                temp.append(value)
    overall = float(_quartiles_item2(temp))
    usable = []
    for segment in segments:
        if segment.length < 5000:
            continue
        if len(segment.frequencies) < minimum_variant_frequencies:
            maf = -1.0
        else:
            mafs = [float(F32(1) - value) if value > 0.5 else float(value) for value in segment.frequencies]
            mafs.sort()
            maf = mafs[len(mafs) // 2]
        coverage = _median_float_list(segment.counts)
        if coverage > overall * 2:
            continue
        weight = float(segment.length)
        if len(segment.frequencies) < 10:
            weight *= len(segment.frequencies) / 10
        usable.append((segment, coverage, maf, weight))
    return usable, F32(overall)


def literal(case, fit=None):
    fit = fit or R.fit_vectorised
    p = call_params(case)
    max_cn = dict(R.DEFAULTS, **fit_params(case))["maximum_copy_number"]
    cso, csi, sbo = case["chr_seg_offset"], case["chr_site_offset"], case["seg_bin_offset"]
    nchr = len(cso) - 1
    ref_cn = case.get("seg_ref_cn")
    excluded = case.get("excluded")
    segments = []
    for c in range(nchr):
        for s in range(cso[c], cso[c + 1]):
            segments.append(_Segment(s, c, int(case["seg_begin"][s]), int(case["seg_end"][s]), case["counts"][sbo[s]:sbo[s + 1]], 2 if ref_cn is None else int(ref_cn[s])))
    nseg = len(segments)
    # ---- stage 1: ReadFrequenciesWrapper (the forward-only pointer per chromosome), MeanCoverage
    for c in range(nchr):
        mine = segments[cso[c]:cso[c + 1]]
        index = 0
        for i in range(csi[c], csi[c + 1]):
            position, ref, alt = int(case["site_pos"][i]), int(case["site_ref"][i]), int(case["site_alt"][i])
            if ref + alt < 10 or not mine:
                continue
            while index < len(mine) and not mine[index].end > position:
                index += 1
            if index >= len(mine) or mine[index].begin > position:
                continue
            mine[index].frequencies.append(F32(alt) / F32(ref + alt))
            mine[index].total_coverage.append(ref + alt)
    cover = [t for sg in segments for t in sg.total_coverage]
    if not cover:
        raise Invalid("no site")
    out = dict(kept_sites=len(cover), mean_coverage=sum(cover) / len(cover), stages=0)
    out["seg_median_count"] = np.array([_median_float_list(sg.counts) for sg in segments], np.float64)
    out["site_count"] = np.array([len(sg.frequencies) for sg in segments], np.int64)
    upper = []
    for sg in segments:
        mafs = sorted(float(F32(1) - f) if f > 0.5 else float(f) for f in sg.frequencies)
        upper.append(mafs[len(mafs) // 2] if mafs else 0.0)
    out["seg_maf_upper"] = np.array(upper, np.float64)
    # ---- stage 2: the loop of :1626-1634
    threshold = p["minimum_variant_frequencies"]
    while True:
        usable, overall = usable_segments_literal(segments, p["is_enrichment"], threshold)
        valid_maf_count = sum(1 for u in usable if u[2] >= 0)
        if valid_maf_count > min(20, nseg):
            break
        if threshold <= 5:
            break
        threshold -= 15
        threshold = max(5, threshold)
    usable_of = {u[0].index: u for u in usable}
    out.update(threshold_used=threshold, nusable=len(usable), overall_median_coverage=float(overall), stages=2,
               seg_usable=np.array([1 if sg.index in usable_of else 0 for sg in segments], np.int32), seg_coverage=out["seg_median_count"].copy(),
               seg_maf=np.array([-1.0 if len(sg.frequencies) < threshold else upper[sg.index] for sg in segments], np.float64),
               seg_weight=np.array([float(sg.length) * (len(sg.frequencies) / 10) if len(sg.frequencies) < 10 else float(sg.length) for sg in segments], np.float64))
    for sg, coverage, maf, weight in usable:                     # the per-segment outputs are those the reference holds for its usable segments
        assert (out["seg_coverage"][sg.index], out["seg_maf"][sg.index], out["seg_weight"][sg.index]) == (coverage, maf, weight)
    if len(usable) < 3:
        e = FewSegments("fewer than 3 usable segments"); e.partial = out
        raise e
    # ---- stage 3
    temp_coverage = []
    for sg, _, _, _ in usable:
        if sg.ref_cn != 2:
            continue
        temp_coverage.extend(sg.counts)
    if not temp_coverage:
        e = Invalid("no usable segment at reference copy number 2"); e.partial = out
        raise e
    median_coverage_level = round(float(_quartiles_item2(temp_coverage)))      # Convert.ToInt32(float): half to even
    out["median_coverage_level"] = median_coverage_level
    if median_coverage_level < 1:
        e = Invalid("median coverage level"); e.partial = out
        raise e
    ev = p["evenness_score"]
    if ev == ev and ev < p["evenness_score_threshold"]:
        scaler = max(ev - p["min_evenness_score"], 0.0) / (p["evenness_score_threshold"] - p["min_evenness_score"])
        cwf = p["coverage_weighting_with_maf_segmentation"] + (p["coverage_weighting"] - p["coverage_weighting_with_maf_segmentation"]) * scaler
        cwf /= median_coverage_level
    else:
        cwf = p["coverage_weighting"] / median_coverage_level
    min_coverage = int(max(F32(10), F32(median_coverage_level) / p["lower_coverage_level_weighting_factor"]))
    max_coverage = int(max(F32(10), F32(median_coverage_level) * p["upper_coverage_level_weighting_factor"]))
    if p["user_ploidy"] >= 0:
        min_coverage = max_coverage = int(float(F32(median_coverage_level) / p["user_ploidy"]) * 2.0)
    out.update(coverage_weighting_factor=cwf, min_coverage=min_coverage, max_coverage=max_coverage, deviation_factor=2.0 if nseg < 500 else float(F32(dict(R.DEFAULTS, **fit_params(case))["deviation_factor"])),
               fixed_percent_purity=int(p["user_purity"] * F32(100)) if p["user_purity"] >= 0 else -1, stages=3)
    # ---- stage 4
    fc = _fit_case(case, p, [u[1] for u in usable], [u[2] for u in usable], [u[3] for u in usable], [u[0].length for u in usable], out, nseg)
    try:
        res = fit(fc)
    except (R.NoModel, R.NoScore) as e:
        out["fit"] = _fit_fields(e.args[0]); e.partial = out
        raise
    out["fit"] = _fit_fields(res)
    diploid_coverage, purity = float(res["coverage"]), res["purity"]
    # ---- stage 5: AssignPloidyCalls against the unrefined table
    points = R._Scalar().model_points(res["coverage"], res["percent_purity"], max_cn)
    tumor_haploid, normal_haploid = diploid_coverage * purity / 2.0, diploid_coverage * (1.0 - purity) / 2.0
    mean_count = np.zeros(nseg)
    needed = np.zeros(nseg, bool)
    for sg in segments:
        mafs = sorted(float(F32(1) - f) if f > 0.5 else float(f) for f in sg.frequencies)
        median_coverage = _median_float_list(sg.counts)
        median_maf = mafs[len(mafs) // 2] if len(mafs) >= 10 else None
        best_distance = second_distance = DBL_MAX
        best = second = None
        for pt in points:
            target_coverage = pt["cn"] * tumor_haploid + normal_haploid if sg.ref_cn == 1 else pt["coverage"]
            target_maf = 0.0 if sg.ref_cn == 1 else pt["maf"]
            diff = (median_coverage - target_coverage) * cwf
            distance = diff * diff
            if median_maf is None or median_maf < 0:
                distance = 2 * distance
            else:
                diff = median_maf - target_maf
                distance += diff * diff
            if distance < best_distance:
                second_distance, second = best_distance, best
                best_distance, best = distance, pt
            elif distance < second_distance:
                second_distance, second = distance, pt
        sg.cn, sg.cn2 = best["cn"], (second["cn"] if second is not None else -1)
        sg.mcc = best["major"] if median_maf is not None else None
        sg.dist, sg.dist2 = best_distance, second_distance
        if sg.cn == max_cn:
            total = 0.0
            for v in sg.counts:
                total += float(v)
            with np.errstate(over="ignore"):
                mean = float(F32(total)) / sg.bins
            mean_count[sg.index], needed[sg.index] = mean, True
            coverage_ratio = mean / diploid_coverage
            estimate = (2 * coverage_ratio - sg.ref_cn * (1 - purity)) / purity if purity != 0 else math.nan
            estimate_cn = _round_to_int(estimate)
            if estimate_cn > max_cn:
                sg.cn, sg.mcc = estimate_cn, None
                coverage = diploid_coverage * ((1 - purity) + purity * estimate_cn / 2.0)
                sg.dist = abs(mean - coverage) * cwf
    out.update(seg_cn=np.array([sg.cn for sg in segments], np.int32), seg_cn2=np.array([sg.cn2 for sg in segments], np.int32),
               seg_mcc=np.array([-1 if sg.mcc is None else sg.mcc for sg in segments], np.int32), seg_dist=np.array([sg.dist for sg in segments]),
               seg_dist2=np.array([sg.dist2 for sg in segments]), seg_mean_count=mean_count, mean_needed=needed)
    # ---- stage 6
    reported_purity = purity
    snv = p["snv_purity_estimate"]
    if snv == snv:
        fraction_abnormal = total_weight = 0.0
        for sg in segments:
            total_weight += sg.length
            if sg.cn != 2 or sg.mcc != 1:
                fraction_abnormal += sg.length
        fraction_abnormal /= total_weight
        if fraction_abnormal < 0.07 and purity < 0.5:
            reported_purity = snv
    for sg in segments:
        sg.q = _qscore_literal(p, sg)
    out["seg_qscore"] = np.array([sg.q for sg in segments], np.int32)
    events = set()
    if p["is_enrichment"]:
        merged = merge_segments(segments, p["minimum_call_size"], p["merge_span"], events)
    else:
        merged = _merge_excluded(segments, p["minimum_call_size"], excluded, events)
    out["merge_events"] = events
    for sg in merged:
        sg.q = _qscore_literal(p, sg)
    for sg in merged:
        sg.filter = (1 if sg.q < p["quality_filter_threshold"] else 0) | (2 if sg.end - sg.begin < 10000 else 0)
    run_of = {sg.index: r for r, sg in enumerate(merged)}
    seg_run = []
    for sg in segments:
        t = sg
        while t.index not in run_of:
            t = t.absorbed_by
        seg_run.append(run_of[t.index])
    # EstimateChromosomeCount
    base = [0] * (max_cn + 1)
    current, overall_count = None, 0.0

    def weighted(base):
        weighted_mean = weight = 0.0
        for cn in range(len(base)):
            weight += base[cn]
            weighted_mean += _wrap32(base[cn] * cn)
        return 0.0 if weight == 0 else weighted_mean / weight
    for sg in segments:
        if sg.chr != current:
            if current is not None:
                overall_count += weighted(base)
            base = [0] * (max_cn + 1)
            current = sg.chr
        if sg.filter != 0:
            continue
        if sg.cn == -1:
            continue
        base[min(sg.cn, max_cn)] = _wrap32(base[min(sg.cn, max_cn)] + sg.length)
    overall_count += weighted(base)
    out.update(seg_run=np.array(seg_run, np.int64), nruns=len(merged), run_owner=np.array([sg.index for sg in merged], np.int64), run_begin=np.array([sg.begin for sg in merged], np.int32),
               run_end=np.array([sg.end for sg in merged], np.int32), run_bin_count=np.array([sg.bins for sg in merged], np.int64), run_qscore=np.array([sg.q for sg in merged], np.int32),
               run_filter=np.array([sg.filter for sg in merged], np.int32), reported_purity=reported_purity, purity_model_fit=res["deviation"],
               inter_model_distance=res["inter_model_distance"], estimated_chromosome_count=overall_count, heterogeneity_proportion=0.0, stages=6)
    return out


# ================================================================================================================ (b) arrays
def _slice_stat(values, off, upper):
    """per slice: the float median (average in float) or the upper median a[n/2]; 0 for an empty slice"""
    res = np.zeros(len(off) - 1, np.float64)
    for s in range(len(off) - 1):
        a = np.sort(values[off[s]:off[s + 1]])
        n = len(a)
        if n == 0:
            continue
        res[s] = a[n // 2] if (upper or n % 2) else (a[n // 2 - 1] + a[n // 2]) / F32(2)
    return res


def _q2(values):
    a = np.sort(np.asarray(values, F32))
    n = len(a)
    return a[n // 2] if n % 2 else F32((a[n // 2 - 1] + a[n // 2]) / F32(2))


def _qscores_arrays(p, bins, cn, dist, dist2):
    res = np.zeros(len(bins), np.int32)
    for i in range(len(bins)):
        lb = math.log10(1 + int(bins[i]))
        ratio = 0.0 if dist2[i] == 0 else dist[i] / dist2[i]
        x = p["logistic_intercept"] + lb * p["logistic_log_bin_count"]
        x = x + (dist[i] / max(1.0, int(cn[i]) - 4.0)) * p["logistic_model_distance"]
        x = x + ratio * p["logistic_distance_ratio"]
        x = x + (lb if cn[i] >= 15 else 0.0)
        e = _exp(x)
        pr = e / (e + 1) if e != math.inf else math.nan
        q = _round_to_int(-10 * _log10(1 - pr)) if pr == pr else INT_MIN
        res[i] = max(2, min(60, q))
    return res


def arrays(case, fit=None):
    fit = fit or R.fit_vectorised
    p = call_params(case)
    max_cn = dict(R.DEFAULTS, **fit_params(case))["maximum_copy_number"]
    cso, csi = np.asarray(case["chr_seg_offset"], np.int64), np.asarray(case["chr_site_offset"], np.int64)
    sbo = np.asarray(case["seg_bin_offset"], np.int64)
    begin, end = np.asarray(case["seg_begin"], np.int64), np.asarray(case["seg_end"], np.int64)
    counts = np.asarray(case["counts"], F32)
    nchr, nseg = len(cso) - 1, len(begin)
    chrom = np.repeat(np.arange(nchr), np.diff(cso))
    ref_cn = np.full(nseg, 2, np.int64) if case.get("seg_ref_cn") is None else np.asarray(case["seg_ref_cn"], np.int64)
    excluded = case.get("excluded")
    length = end - begin
    bins = np.diff(sbo)
    # ---- stage 1: the first segment of the chromosome with End > position, if it begins at or before it
    pos, ref, alt = (np.asarray(case[k], np.int64) for k in ("site_pos", "site_ref", "site_alt"))
    site_seg = np.full(len(pos), -1, np.int64)
    for c in range(nchr):
        s0, s1 = cso[c], cso[c + 1]
        if s1 == s0:
            continue
        sl = slice(csi[c], csi[c + 1])
        k = s0 + np.searchsorted(end[s0:s1], pos[sl], side="right")
        ok = (k < s1) & (ref[sl] + alt[sl] >= 10)
        ok &= begin[np.minimum(k, s1 - 1)] <= pos[sl]
        site_seg[sl] = np.where(ok, k, -1)
    kept = site_seg >= 0
    if not kept.any():
        raise Invalid("no site")
    freq = alt[kept].astype(F32) / (ref[kept] + alt[kept]).astype(F32)
    folded = np.where(freq > F32(0.5), F32(1) - freq, freq).astype(F32)
    site_off = np.searchsorted(site_seg[kept], np.arange(nseg + 1), side="left")
    nf = np.diff(site_off)
    med = _slice_stat(counts, sbo, False)
    upper = _slice_stat(folded, site_off, True)
    out = dict(kept_sites=int(kept.sum()), mean_coverage=int((ref[kept] + alt[kept]).sum()) / int(kept.sum()), seg_median_count=med, site_count=nf.astype(np.int64), seg_maf_upper=upper)
    # ---- stage 2
    overall = _q2(med.astype(F32)) if p["is_enrichment"] else _q2(counts)
    usable = (length >= 5000) & ~(med > float(overall) * 2)
    threshold = p["minimum_variant_frequencies"]
    while not (np.count_nonzero(usable & (nf >= threshold)) > min(20, nseg)) and threshold > 5:
        threshold = max(5, threshold - 15)
    maf = np.where(nf < threshold, -1.0, upper)
    weight = np.where(nf < 10, length.astype(np.float64) * (nf / 10), length.astype(np.float64))
    out.update(threshold_used=int(threshold), nusable=int(usable.sum()), overall_median_coverage=float(overall), seg_usable=usable.astype(np.int32), seg_coverage=med.copy(),
               seg_maf=maf, seg_weight=weight, stages=2)
    if usable.sum() < 3:
        e = FewSegments("fewer than 3 usable segments"); e.partial = out
        raise e
    # ---- stage 3
    take = usable & (ref_cn == 2)
    mask = np.repeat(take, bins)
    if not mask.any():
        e = Invalid("no usable segment at reference copy number 2"); e.partial = out
        raise e
    level = int(np.rint(np.float64(_q2(counts[mask]))))          # rint: half to even
    out["median_coverage_level"] = level
    if level < 1:
        e = Invalid("median coverage level"); e.partial = out
        raise e
    ev, cw, cwm = p["evenness_score"], p["coverage_weighting"], p["coverage_weighting_with_maf_segmentation"]
    if not math.isnan(ev) and ev < p["evenness_score_threshold"]:
        cwf = (cwm + (cw - cwm) * (max(ev - p["min_evenness_score"], 0.0) / (p["evenness_score_threshold"] - p["min_evenness_score"]))) / level
    else:
        cwf = cw / level
    lo = int(np.maximum(F32(10), np.divide(F32(level), p["lower_coverage_level_weighting_factor"], dtype=F32)))
    hi = int(np.maximum(F32(10), np.multiply(F32(level), p["upper_coverage_level_weighting_factor"], dtype=F32)))
    if p["user_ploidy"] >= 0:
        lo = hi = int(np.float64(np.divide(F32(level), p["user_ploidy"], dtype=F32)) * 2.0)
    fixed_purity = int(np.multiply(p["user_purity"], F32(100), dtype=F32)) if p["user_purity"] >= 0 else -1
    dev_factor = 2.0 if nseg < 500 else float(F32(dict(R.DEFAULTS, **fit_params(case))["deviation_factor"]))
    out.update(coverage_weighting_factor=cwf, min_coverage=lo, max_coverage=hi, deviation_factor=dev_factor, fixed_percent_purity=fixed_purity, stages=3)
    # ---- stage 4
    fc = _fit_case(case, p, med[usable], maf[usable], weight[usable], length[usable], out, nseg)
    try:
        res = fit(fc)
    except (R.NoModel, R.NoScore) as e:
        out["fit"] = _fit_fields(e.args[0]); e.partial = out
        raise
    out["fit"] = _fit_fields(res)
    dc, purity = float(res["coverage"]), res["purity"]
    # ---- stage 5: the distance matrix (segments x points), best and runner-up by a stable order of each row
    pc, pm = R.table_vectorised([(res["coverage"], res["percent_purity"])], max_cn)
    pl = np.array(R.ploidies(max_cn), np.int64)
    th, nh = dc * purity / 2.0, dc * (1.0 - purity) / 2.0
    haploid = (ref_cn == 1)[:, None]
    tcov = np.where(haploid, (pl[:, 0] * th + nh)[None, :], pc[0][None, :])
    tmaf = np.where(haploid, 0.0, pm[0][None, :])
    has = nf >= 10
    dcov = (med[:, None] - tcov) * cwf
    d2 = dcov * dcov
    dm = np.where(has, upper, 0.0)[:, None] - tmaf
    dist_all = np.where(has[:, None], d2 + dm * dm, 2 * d2)
    cn = np.zeros(nseg, np.int64); cn2 = np.zeros(nseg, np.int64); mcc = np.zeros(nseg, np.int64); dist = np.zeros(nseg); dist2 = np.zeros(nseg)
    for s in range(nseg):
        row = dist_all[s]
        b = int(np.argmin(row))                                  # the first minimum: strict <
        # the runner-up of the scan is the smallest of the others; among equals it is the best displaced last (the first minimum in front of b) if that one has the
        # value, since a displaced best replaces the runner-up unconditionally, and otherwise the first index with the value (later equals fail the strict <)
        others = np.delete(row, b)
        v = others.min()
        m = int(np.argmin(row[:b])) if b > 0 else -1
        r = m if (m >= 0 and row[m] == v) else [i for i in range(len(row)) if i != b and row[i] == v][0]
        cn[s], cn2[s], mcc[s], dist[s], dist2[s] = pl[b, 0], pl[r, 0], (pl[b, 1] if has[s] else -1), row[b], row[r]
    mean_count = np.zeros(nseg)
    needed = cn == max_cn
    for s in np.nonzero(needed)[0]:
        total = np.add.accumulate(counts[sbo[s]:sbo[s + 1]].astype(np.float64))[-1]
        with np.errstate(over="ignore"):
            mean_count[s] = float(F32(total)) / int(bins[s])
        est = (2 * (mean_count[s] / dc) - int(ref_cn[s]) * (1 - purity)) / purity if purity != 0 else math.nan
        k = _round_to_int(est)
        if k > max_cn:
            cn[s], mcc[s] = k, -1
            dist[s] = abs(mean_count[s] - dc * ((1 - purity) + purity * k / 2.0)) * cwf
    out.update(seg_cn=cn.astype(np.int32), seg_cn2=cn2.astype(np.int32), seg_mcc=mcc.astype(np.int32), seg_dist=dist, seg_dist2=dist2, seg_mean_count=mean_count, mean_needed=needed)
    # ---- stage 6
    reported = purity
    if not math.isnan(p["snv_purity_estimate"]):
        abnormal = float(np.add.accumulate(np.where((cn != 2) | (mcc != 1), length, 0).astype(np.float64))[-1]) / float(np.add.accumulate(length.astype(np.float64))[-1])
        if abnormal < 0.07 and purity < 0.5:
            reported = p["snv_purity_estimate"]
    q = _qscores_arrays(p, bins, cn, dist, dist2)
    out["seg_qscore"] = q
    B, E, N = begin.copy(), end.copy(), bins.copy()              # the segments as the merges leave them
    parent = np.arange(nseg)
    enrich, mcs, span = bool(p["is_enrichment"]), p["minimum_call_size"], p["merge_span"]

    def blocked(c, a, b):
        if excluded is None:
            return False
        st, sp = np.asarray(excluded[c][0], np.int64), np.asarray(excluded[c][1], np.int64)
        seen = np.concatenate([[True], np.logical_not(np.cumsum(st > b)[:-1] > 0)]) if len(st) else np.zeros(0, bool)      # intervals the reference's loop reaches
        return bool((seen & (((st >= a) & (st <= b)) | ((sp >= a) & (sp <= b)))).any())

    def absorb(a, b):
        grow_left, grow_right = B[b] < B[a], E[b] > E[a]
        if grow_left:
            B[a] = B[b]; N[a] += N[b]
        if grow_right:
            E[a] = E[b]; N[a] += N[b]
        parent[b] = a

    def neighbour(i, step):
        j = i + step
        stop = (-1 if enrich else 0) if step < 0 else nseg
        while j != stop and chrom[j] == chrom[i]:
            if E[j] - B[j] >= mcs:
                gap_blocked = ((B[i] - E[j] if step < 0 else B[j] - E[i]) > span) if enrich else (blocked(chrom[j], E[j], B[i]) if step < 0 else blocked(chrom[j], E[i], B[j]))
                return None if gap_blocked else j
            j += step
        return None
    none_q = -1 if enrich else 0
    found = (lambda x: x >= 0) if enrich else (lambda x: x > 0)
    keep, i = [], 0
    while i < nseg:
        if E[i] - B[i] >= mcs:
            keep.append(i); i += 1
            continue
        pv, nx = neighbour(i, -1), neighbour(i, +1)
        pq = none_q if pv is None else q[pv]
        nq = none_q if nx is None else q[nx]
        if found(pq) and pq >= nq:
            absorb(pv, i); i += 1
        elif found(nq):
            for t in (range(nx - 1, i - 1, -1) if enrich else range(i, nx)):
                absorb(nx, t)
            i = nx
        else:
            keep.append(i); i += 1
    runs = [keep[0]]
    for s in keep[1:]:
        a = runs[-1]
        close = (B[s] - E[a] < span) if enrich else not blocked(chrom[a], E[a], B[s])
        if cn[a] == cn[s] and chrom[a] == chrom[s] and close:
            absorb(a, s)
        else:
            runs.append(s)
    runs = np.array(runs, np.int64)
    rq = _qscores_arrays(p, N[runs], cn[runs], dist[runs], dist2[runs])
    rf = np.where(rq < p["quality_filter_threshold"], 1, 0) | np.where(E[runs] - B[runs] < 10000, 2, 0)
    root = parent.copy()
    while (root != root[root]).any():
        root = root[root]
    seg_run = np.searchsorted(runs, root)
    assert (runs[seg_run] == root).all()
    passes = np.ones(nseg, bool); passes[runs] = rf == 0
    count = 0.0
    for c in range(nchr):
        sl = slice(cso[c], cso[c + 1])
        if cso[c] == cso[c + 1]:
            continue
        base = np.zeros(max_cn + 1, np.int64)
        for s in np.nonzero(passes[sl])[0] + cso[c]:
            k = min(int(cn[s]), max_cn)
            base[k] = _wrap32(base[k] + (E[s] - B[s]))
        weight_sum = float(np.add.accumulate(base.astype(np.float64))[-1])
        prod = np.array([_wrap32(int(base[k]) * k) for k in range(max_cn + 1)], np.float64)
        count += 0.0 if weight_sum == 0 else float(np.add.accumulate(prod)[-1]) / weight_sum
    out.update(seg_run=seg_run.astype(np.int64), nruns=len(runs), run_owner=runs, run_begin=B[runs].astype(np.int32), run_end=E[runs].astype(np.int32), run_bin_count=N[runs].astype(np.int64),
               run_qscore=rq, run_filter=rf.astype(np.int32), reported_purity=reported, purity_model_fit=res["deviation"], inter_model_distance=res["inter_model_distance"],
               estimated_chromosome_count=count, heterogeneity_proportion=0.0, stages=6)
    return out


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def differences(got, want, skip=()):
    """names of the outputs of `want` that `got` does not reproduce bit for bit"""
    bad = []
    for k, w in want.items():
        if k in skip or k in ("mean_needed", "merge_events"):
            continue
        if k not in got:
            bad.append(k + " (missing)")
            continue
        g = got[k]
        if k == "fit":
            for f in FIT_FIELDS:
                if f == "percent_cn" and len(w[f]) == 0:             # a fit that ended without a best model: the row stays cleared
                    ok = not np.any(g[f])
                elif f == "percent_cn":
                    ok = len(g[f]) == len(w[f]) and (bits(g[f]) == bits(w[f])).all()
                elif isinstance(w[f], float):
                    ok = bits(g[f]) == bits(w[f])
                else:
                    ok = int(g[f]) == int(w[f])
                if not ok:
                    bad.append("fit." + f)
        elif isinstance(w, np.ndarray):
            g = np.asarray(g)
            if g.shape != w.shape:
                bad.append(k + " (shape)")
            elif k in SEG_FLOATS:
                if not (bits(g) == bits(w)).all():
                    bad.append(k)
            elif not (g.astype(np.int64) == w.astype(np.int64)).all():
                bad.append(k)
        elif k in SCALAR_FLOATS:
            if bits(float(g)) != bits(float(w)):
                bad.append(k)
        elif int(g) != int(w):
            bad.append(k)
    return bad
