"""The two restatements of tests/somatic_call_ref.py agree on every output of every case of tests/somatic_call_cases.py (doubles as bit patterns), the cases really take the
edges they are named for, and the literal restatement reproduces two of the reference's own unit tests (fixtures under tests/golden/somatic_call: data only)."""
import json
import math
import os

import numpy as np
import pytest

import somatic_call_cases as C
import somatic_call_ref as CR
import somatic_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "somatic_call")
F32 = np.float32


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatements_agree_on_every_output(name):
    a, b = C.literal(name), C.arrays(name)
    assert not isinstance(a, Exception) and not isinstance(b, Exception), (a, b)
    assert CR.differences(a, b) == [] and CR.differences(b, a) == []
    assert (a["mean_needed"] == b["mean_needed"]).all()
    assert a["stages"] == 6 and set(a) - {"merge_events"} == set(b)


@pytest.mark.parametrize("name,kind,stages", [("2 usable", CR.FewSegments, 2), ("no reference 2", CR.Invalid, 2), ("level 0", CR.Invalid, 2), ("no model", R.NoModel, 3)])
def test_restatements_agree_on_what_an_error_leaves(name, kind, stages):
    a, b = C.literal(name), C.arrays(name)
    assert type(a) is kind and type(b) is kind
    assert a.partial["stages"] == stages and CR.differences(a.partial, b.partial) == [] and CR.differences(b.partial, a.partial) == []


def test_literal_restatement_with_the_scalar_fit():
    """the statement-by-statement fit of tests/somatic_ref.py under the statement-by-statement caller, on the smallest case"""
    case = C.built("3 usable")
    assert CR.differences(CR.literal(case, fit=R.fit_scalar), C.literal("3 usable")) == []


def _extra(name, k):
    """index of the k-th segment of the chromosome a case appends behind the two autosomes"""
    return int(C.built(name)["chr_seg_offset"][2]) + k


def test_site_count_and_length_edges():
    r, case = C.literal("site counts"), C.built("site counts")
    e = lambda k: _extra("site counts", k)
    length = case["seg_end"] - case["seg_begin"]
    assert (length[e(0)], length[e(1)]) == (4999, 5000) and (r["seg_usable"][e(0)], r["seg_usable"][e(1)]) == (0, 1)
    assert r["site_count"][e(2):e(7)].tolist() == [0, 9, 10, 49, 50] and r["threshold_used"] == 50
    assert r["seg_maf"][e(5)] == -1.0 and r["seg_maf"][e(6)] == r["seg_maf_upper"][e(6)] > 0                    # 49 / 50 against the threshold
    assert r["seg_weight"][e(2):e(5)].tolist() == [0.0, 60000 * 0.9, 60000.0]                                    # 0 / 9 / 10 against the weight's 10
    assert r["seg_mcc"][e(3)] == -1 and r["seg_mcc"][e(4)] >= 0                                                 # ... and against AssignPloidyCalls' 10
    assert r["seg_mcc"][e(7)] == -1 and r["seg_cn"][e(7)] == 3


def test_coverage_cut_edge():
    r, case = C.literal("coverage cut"), C.built("coverage cut")
    a, b = _extra("coverage cut", 0), _extra("coverage cut", 1)
    q2 = r["overall_median_coverage"]
    assert r["seg_coverage"][a] == 2 * q2 and r["seg_usable"][a] == 1
    assert r["seg_coverage"][b] == float(np.nextafter(F32(2 * q2), F32(np.inf))) and r["seg_usable"][b] == 0
    assert r["seg_cn"][b] == 4                                                                                   # dropped from the model, still called


def test_threshold_loop_edges():
    assert [C.literal(n)["threshold_used"] for n in ("base", "threshold 35", "threshold 20", "threshold gives up")] == [50, 35, 20, 5]
    r = C.literal("threshold gives up")
    assert np.count_nonzero(r["seg_maf"] >= 0) == 10 and r["nusable"] == 24
    assert C.literal("3 usable")["nusable"] == 3 and C.literal("2 usable").partial["nusable"] == 2


def test_quartile_edges():
    lo, hi = C.literal("level 20.5"), C.literal("level 21.5 odd overall")
    assert (lo["median_coverage_level"], hi["median_coverage_level"]) == (20, 22)                                # 20.5 and 21.5, half to even both ways
    for name, r in (("level 20.5", lo), ("level 21.5 odd overall", hi)):
        case = C.built(name)
        take = np.repeat(r["seg_usable"].astype(bool) & (case["seg_ref_cn"] == 2), np.diff(case["seg_bin_offset"]))
        assert float(CR._quartiles_item2(case["counts"][take])) == (20.5 if r is lo else 21.5)
        u = r["seg_usable"]
        assert u[0] == 1 and u[-1] == 1 and (u == 0).any()                                                       # the subset is not contiguous
    parity = lambda name: (len(C.built(name)["counts"]) % 2, int(np.diff(C.built(name)["seg_bin_offset"])[C.literal(name)["seg_usable"].astype(bool)].sum()) % 2)
    assert parity("level 20.5") == (0, 0) and parity("level 21.5 odd overall") == (1, 0) and parity("odd level total") == (1, 1)
    assert C.literal("merges enrichment")["overall_median_coverage"] == float(CR._quartiles_item2(C.literal("merges enrichment")["seg_median_count"].astype(F32)))
    assert len(C.built("merges enrichment")["seg_begin"]) % 2 == 1 and len(C.built("merges enrichment behind segment 0")["seg_begin"]) % 2 == 0


def test_reference_copy_number_edges():
    r, case = C.literal("reference copy number"), C.built("reference copy number")
    x, y = int(case["chr_seg_offset"][2]), int(case["chr_seg_offset"][3])
    assert case["seg_ref_cn"][x:x + 3].tolist() == [1, 1, 1] and r["seg_cn"][x:x + 3].tolist() == [1, 2, 1]         # the haploid columns: copy number c sits at 10 c here too
    assert case["seg_ref_cn"][y] == 0 and r["seg_usable"][y] == 1 and r["seg_cn"][y] == 0
    assert r["median_coverage_level"] == C.literal("base")["median_coverage_level"] == 20


def test_tie_edges():
    r = C.literal("ties")
    a, b = _extra("ties", 0), _extra("ties", 1)
    assert r["site_count"][a] < 10 and r["seg_dist"][a] == r["seg_dist2"][a] and r["seg_cn"][a] == r["seg_cn2"][a] == 2 and r["seg_mcc"][a] == -1
    assert r["seg_usable"][b] == 0 and (r["seg_cn"][b], r["seg_cn2"][b]) == (1, 2) and r["seg_dist"][b] == r["seg_dist2"][b] > 0      # midway: the first of the two wins


def test_high_copy_number_edges():
    r, case = C.literal("high copy number"), C.built("high copy number")
    e = lambda k: _extra("high copy number", k)
    assert r["fit"]["purity"] == 1.0 and r["fit"]["diploid_coverage"] == 20.0
    assert r["seg_mean_count"][e(0):e(4)].tolist() == [80.0, 90.0, 85.0, 95.0] and r["seg_cn"][e(0):e(4)].tolist() == [8, 9, 8, 10]      # 8, 9, 8.5 -> 8, 9.5 -> 10
    assert r["mean_needed"][e(0):e(6)].all() and r["mean_needed"].sum() == 6
    assert r["seg_mcc"][e(2)] >= 4 and r["seg_mcc"][e(1)] == -1                                                  # 20 frequencies; the adjusted call loses its count
    assert r["seg_cn"][e(5)] == 15 and r["seg_cn"][e(4)] > 10 ** 6
    sl = slice(case["seg_bin_offset"][e(4)], case["seg_bin_offset"][e(4) + 1])
    x = case["counts"][sl].astype(np.float64)
    assert len(x) == 5000
    serial = 0.0
    for v in x.tolist():
        serial += v
    # the order of the additions decides the FLOAT the total rounds to, hence MeanCount and the copy number: every other order lands one float higher
    others = dict(pairwise=float(np.sum(x)), reversed=float(np.add.accumulate(x[::-1])[-1]), ascending=float(np.add.accumulate(np.sort(x))[-1]),
                  strided=float(np.add.accumulate(np.array([np.add.accumulate(x[k::256])[-1] for k in range(256)]))[-1]), exact=math.fsum(x))
    for name, total in others.items():
        assert float(F32(total)) == 2.0 ** 38 + 26 * 2.0 ** 14 != float(F32(serial)), name
    assert float(F32(serial)) == 2.0 ** 38 + 24 * 2.0 ** 14 and r["seg_mean_count"][e(4)] == float(F32(serial)) / 5000
    assert r["seg_cn"][e(4)] == round(2 * r["seg_mean_count"][e(4)] / 20.0) != round(2 * (float(F32(others["exact"])) / 5000) / 20.0)
    positive = x[x > 0]
    assert np.log2(positive.max()) - np.log2(2.0 ** -17) > 53                                                      # no integer unit holds these counts in 53 bits
    y = case["counts"][case["seg_bin_offset"][e(0)]:case["seg_bin_offset"][e(0) + 1]].astype(np.float64)
    assert float(np.sum(y)) == float(np.sum(y[::-1])) == 8000.0
    # the amplification term: the q-score of the copy number 15 segment is the formula's with log10(1 + BinCount) added, and another number without it
    p = CR.call_params(case)
    k = e(5)
    log_bins = math.log10(1 + 100)
    core = p["logistic_intercept"] + log_bins * p["logistic_log_bin_count"] + (r["seg_dist"][k] / max(1.0, 15 - 4.0)) * p["logistic_model_distance"] + \
        (r["seg_dist"][k] / r["seg_dist2"][k]) * p["logistic_distance_ratio"]
    q_of = lambda score: max(2, min(60, round(-10 * math.log10(1 - math.exp(score) / (math.exp(score) + 1)))))
    assert r["seg_cn"][k] == 15 and r["seg_qscore"][k] == q_of(core + log_bins) != q_of(core)


def test_evenness_and_user_edges():
    base = C.literal("base")
    assert base["coverage_weighting_factor"] == 0.333 / 20
    assert C.literal("evenness above")["coverage_weighting_factor"] == 0.333 / 20
    assert C.literal("evenness between")["coverage_weighting_factor"] == (0.20 + (0.333 - 0.20) * ((91.0 - 88.0) / (94.5 - 88.0))) / 20
    assert C.literal("evenness below")["coverage_weighting_factor"] == (0.20 + (0.333 - 0.20) * 0.0) / 20
    assert (base["min_coverage"], base["max_coverage"], base["fixed_percent_purity"], base["deviation_factor"]) == (10, 47, -1, 2.0)
    r = C.literal("user purity")
    assert r["fixed_percent_purity"] == int(F32(0.97) * F32(100)) == 97 and r["fit"]["best_percent_purity"] == 97 and r["fit"]["nmodels"] == 38
    r = C.literal("user ploidy")
    assert r["min_coverage"] == r["max_coverage"] == int(float(F32(20) / F32(2.1)) * 2.0) == 19 and r["fit"]["best_coverage"] == 19
    assert C.literal("whole grid")["fit"]["nmodels"] == sum(101 - 20 for _ in range(10, 48))


def test_merge_edges():
    plain = {"short first segment", "equal q-scores", "chain merged forwards", "merged backwards", "chromosome change behind", "chromosome change ahead", "short segment kept", "equal calls merged"}
    ev = C.literal("merges")["merge_events"]
    assert plain | {"excluded interval behind", "excluded interval ahead", "equal calls across an excluded interval"} <= ev
    assert "segment 0 not looked at" in C.literal("merges behind segment 0")["merge_events"]
    ev = C.literal("merges enrichment")["merge_events"]
    assert (plain - {"chain merged forwards"}) | {"gap behind", "gap ahead", "equal calls across a gap"} <= ev
    assert "segment 0 looked at" in C.literal("merges enrichment behind segment 0")["merge_events"]
    # the look-back that stops in front of segment 0: the short segment goes forwards, not to segment 0; under the enrichment rules it goes to segment 0
    r, e = C.literal("merges behind segment 0"), C.literal("merges enrichment behind segment 0")
    assert r["seg_run"][1] == r["seg_run"][2] != r["seg_run"][0] and e["seg_run"][1] == e["seg_run"][0]
    # MergeIn as it is: a chain merged forwards in ascending order moves Begin once, so only its first segment's bins arrive
    r, case = C.literal("merges"), C.built("merges")
    bins = np.diff(case["seg_bin_offset"])
    members = np.array([bins[r["seg_run"] == k].sum() for k in range(r["nruns"])])
    assert (r["run_bin_count"] <= members).all() and (r["run_bin_count"] < members).any()
    # MergeSegments assimilates a chain in DESCENDING order, so every segment moves Begin and brings its bins: the same chain of two short segments in front of a
    # large one (the first three segments of the second chromosome) under both merges
    first = int(case["chr_seg_offset"][1])
    assert r["seg_run"][first] == r["seg_run"][first + 1] == r["seg_run"][first + 2] and r["run_owner"][r["seg_run"][first]] == first + 2
    e, ecase = C.literal("merges enrichment span 30000"), C.built("merges enrichment span 30000")
    assert "chain merged forwards" in e["merge_events"] and ecase["params"]["merge_span"] == 30000 and (ecase["seg_begin"] == case["seg_begin"]).all()
    assert e["seg_run"][first] == e["seg_run"][first + 1] == e["seg_run"][first + 2] and e["run_owner"][e["seg_run"][first]] == first + 2
    members = np.array([bins[e["seg_run"] == k].sum() for k in range(e["nruns"])])
    assert (e["run_bin_count"] == members).all()
    assert bins[first:first + 3].tolist() == [30, 30, 100]
    same_run = lambda res: bins[res["seg_run"] == res["seg_run"][first]].sum()
    assert e["run_bin_count"][e["seg_run"][first]] == same_run(e) and r["run_bin_count"][r["seg_run"][first]] == same_run(r) - 30      # ascending: the second short segment's 30 bins are lost
    e1 = C.literal("merges enrichment")
    members = np.array([np.diff(C.built("merges enrichment")["seg_bin_offset"])[e1["seg_run"] == k].sum() for k in range(e1["nruns"])])
    assert (e1["run_bin_count"] == members).all() and "chain merged forwards" not in e1["merge_events"]          # at span 1 a short neighbour is itself the gap


def test_filter_snv_and_chromosome_count_edges():
    r = C.literal("filters")
    assert set(r["run_filter"].tolist()) == {0, 1, 2, 3}                                                          # pass, q alone, size alone, both
    assert C.literal("snv overrides")["reported_purity"] == 0.77 and C.literal("snv overrides")["fit"]["purity"] == float(F32(40) / F32(100))
    assert C.literal("snv does not override")["reported_purity"] == C.literal("snv does not override")["fit"]["purity"] == float(F32(60) / F32(100))
    assert C.literal("base")["reported_purity"] == C.literal("base")["fit"]["purity"]
    # EstimateChromosomeCount walks the original list: with every run filtered (q below 10) only the absorbed segments count, each with its PASS default
    b = C.literal("base")
    assert (b["run_filter"] != 0).all() and b["estimated_chromosome_count"] == 2.0 + 2.0
    assert len(C.built("big segment")["counts"]) > 8192 + 2300 and np.diff(C.built("big segment")["seg_bin_offset"]).max() == 9001


def test_reference_unit_test_usable_segments():
    """TestCanvasSomatic.TestUsableSegments: 50 of 100"""
    g = json.load(open(os.path.join(GOLDEN, "usable_segments.json")))
    rng = np.random.RandomState(1)
    segments, at = [], g["first_position"]
    for i in range(g["nsegments"]):
        length = g["length_odd_index"] if i % 2 == 1 else g["length_even_index"]
        variants = g["variant_count_index_mod_4_above_1"] if i % 4 > 1 else g["variant_count"]
        sg = CR._Segment(i, 0, at, at + length, rng.randint(0, g["count_below"], length // g["bases_per_bin"]).astype(F32), 2)      # (the reference does not advance the position either)
        sg.frequencies = [F32(0.5)] * variants
        segments.append(sg)
    usable, _ = CR.usable_segments_literal(segments, g["is_enrichment"], g["minimum_variant_frequencies"])
    assert len(usable) == g["expected_usable"]
    assert sum(1 for u in usable if u[2] >= 0) == 25


def test_reference_unit_test_merge_segments():
    """TestSegments.TestMergeSegments: 3 / 3 / 1 runs at (50000, 10000)"""
    g = json.load(open(os.path.join(GOLDEN, "merge_segments.json")))
    segments = []
    for i, (chrom, begin, end, cn) in enumerate(g["segments"]):
        sg = CR._Segment(i, chrom, begin, end, [], 2)
        sg.cn = cn
        segments.append(sg)
    merged = CR.merge_segments(segments, g["minimum_call_size"], g["maximum_merge_span"])
    runs = {}
    for sg in merged:
        runs[sg.chr] = runs.get(sg.chr, 0) + 1
    assert runs == g["expected_runs"]
