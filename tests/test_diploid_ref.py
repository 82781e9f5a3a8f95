"""The two CPU restatements of CanvasDiploidCaller's calling step (tests/diploid_ref.py) against each other on the hand-built and the randomised cases, and against what the
reference's own sources pin down (tests/golden/diploid_caller_cases.json: TestMergeSegments, the order of InitializePloidies, the default coefficients), plus the properties
the hand-built case was built for — so that the GPU tests compare with restatements that are known to take the branches in question."""
import json
import math
import os

import numpy as np
import pytest

import diploid_cases as DC
import diploid_ref as R

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diploid_caller_cases.json")))
FLOATS = ("median_count", "median_maf", "dist", "dist2", "run_median_count")


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            x, y = (a[k].view(np.int64), b[k].view(np.int64)) if k in FLOATS else (a[k], b[k])
            assert x.shape == y.shape and (x == y).all(), (k, np.nonzero(x != y)[0][:8], a[k][x != y][:8], b[k][x != y][:8])
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def edge():
    case, names = DC.edge_case()
    return case, names, R.direct(*DC.args(case))


def test_the_restatements_agree_on_the_hand_built_case(edge):
    case, _, d = edge
    same(d, R.vectorised(*DC.args(case)))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_restatements_agree_on_randomised_cases(seed):
    case = DC.random_case(seed)
    d = R.direct(*DC.args(case))
    same(d, R.vectorised(*DC.args(case)))
    assert len(set(d["cn"].tolist())) >= 4 and (d["mcc"] == -1).any() and (d["informative"] == 1).any() and len(d["run_first"]) < len(d["cn"])


def test_merge_segments_reference_case():
    g = GOLDEN["merge_segments"]
    segs = []
    for chrom, begin, end, cn in g["segments"]:
        s = R._Seg(chrom, begin, end, []); s.cn = cn
        segs.append(s)
    merged = R.merge_segments(segs, g["minimum_call_size"], g["maximum_merge_span"])
    got = {}
    for s in merged:
        got[s.chr] = got.get(s.chr, 0) + 1
    assert got == g["expected_counts"]


def test_ploidy_table_order_and_values():
    t = R.ploidy_table(30.0)
    assert [[cn, mj] for cn, mj, _ in t] == GOLDEN["ploidy_order"]["points"] and len(t) == 36
    maf = {(cn, mj): m for cn, mj, m in t}
    assert maf[(0, 0)] == 0.01 and maf[(1, 1)] == 0.0 and maf[(3, 2)] == float(np.float32(1) - np.float32(2) / np.float32(3))
    for cn in (2, 4, 6, 8, 10):
        assert maf[(cn, cn // 2)] == 0.5 - 1 / (3.352 * math.pow(cn * 15.0, 0.4747))
    assert list(R.LOGISTIC_GERMLINE) == GOLDEN["logistic_germline"]["coefficients"]


def test_the_hand_built_case_takes_the_branches_it_was_built_for(edge):
    case, n, d = edge
    assert d["diploid_coverage"] == 100.0
    # sites: at Begin and at End - 1 kept, at End it belongs to the next segment, in the gap and at depth 9 dropped
    assert d["site_count"][n["begin_end"]] == 252 and d["informative"][n["begin_end"]] == 1 and d["site_count"][n["takes_site_at_end"]] == 1
    assert d["site_count"][n["nine_sites"]] == 9 and d["mcc"][n["nine_sites"]] == -1 and d["informative"][n["nine_sites"]] == 0
    assert d["site_count"][n["ten_sites"]] == 10 and d["mcc"][n["ten_sites"]] >= 0
    # the density bound
    assert d["site_count"][n["density_10"]] == 10 and d["informative"][n["density_10"]] == 1
    assert d["site_count"][n["density_11"]] == 10 and d["informative"][n["density_11"]] == 0 and d["mcc"][n["density_11"]] >= 0 and d["median_maf"][n["density_11"]] == -1
    # ties keep the earlier point, the other becomes the runner-up
    for k, cn in (("tie_125", 2), ("tie_75", 1)):
        assert d["cn"][n[k]] == cn and d["dist"][n[k]] == d["dist2"][n[k]] > 0
    assert d["informative"][n["tie_125_maf"]] == 1 and d["informative"][n["tie_75_maf"]] == 1 and d["dist"][n["tie_125_maf"]] < d["dist2"][n["tie_125_maf"]]
    # a runner-up distance of 0 (both CN 2 points at distance 0 without MAF), CN above 4
    assert d["dist2"][n["gap_10000"]] == 0 and d["dist"][n["gap_10000"]] == 0 and d["cn"][n["gap_10000"]] == 2
    assert d["informative"][n["cn6"]] == 1 and d["informative"][n["cn3"]] == 1 and d["cn"][n["cn6"]] == 6 and d["cn"][n["cn0"]] == 0 and d["cn"][n["cn3"]] == 3 and d["cn"][n["cn1"]] == 1
    # merges
    runs = list(zip(d["run_first"].tolist(), d["run_last"].tolist()))
    assert (n["begin_end"], n["gap_9999"]) in runs                                # across a gap of 9 999
    assert any(f == n["gap_10000"] for f, _ in runs)                              # not across 10 000
    assert (n["moved_end_a"], n["moved_end_c"]) in runs                           # the gap closes against the run's moved end
    assert any(f == n["next_chromosome"] for f, _ in runs)                        # not across a chromosome boundary
    r = [f for f, _ in runs].index(n["three_bins"])
    assert runs[r] == (n["three_bins"], n["thousand_bins"]) and d["qscore"][n["three_bins"]] < 10 <= d["run_qscore"][r] and d["run_filter"][r] == 0
    assert d["run_filter"][[f for f, _ in runs].index(n["short"])] & 2


# ---------------------------------------------------------------------------------------------------------------- the file side: what the reference's unit tests pin
def test_read_segments_confidence_intervals():
    g = GOLDEN["read_segments"]
    segs = R.read_segments(g["partitioned"])
    assert [(s.chr, s.begin, s.end) for s in segs] == [("chr22", 1, 10), ("chr22", 10, 30), ("chr22", 30, 40)]
    assert [[list(s.start_ci), list(s.end_ci)] for s in segs] == g["confidence_intervals"]
    assert [len(s.counts) for s in segs] == [1, 1, 1] and segs[1].counts[0] == np.float32(31)


def test_read_segments_groups_by_adjacent_id_and_refuses_a_chromosome_that_comes_back():
    rows = ["chr1\t0\t100\t5\t0", "chr1\t100\t201\t6\t0", "chr1\t300\t401\t7\t0", "chr1\t401\t500\t8\t1", "chr2\t0\t51\t9\t1"]
    segs = R.read_segments(rows)
    assert [(s.chr, s.begin, s.end, len(s.counts)) for s in segs] == [("chr1", 0, 401, 3), ("chr1", 401, 500, 1), ("chr2", 0, 51, 1)]
    # half lengths round half away from zero: 101 -> 51, 99 -> 50, 51 -> 26; the first segment's end touches the second's first bin
    assert (segs[0].start_ci, segs[0].end_ci) == ((-50, 50), (-51, 50)) and (segs[1].start_ci, segs[1].end_ci) == ((-51, 50), (-50, 50)) and segs[2].start_ci == (-26, 26)
    with pytest.raises(ValueError):
        R.read_segments(rows + ["chr1\t600\t700\t1\t2"])


def test_read_frequencies_reference_case():
    g = GOLDEN["read_frequencies"]
    got = R.read_frequencies(g["vaf"], {c: [tuple(i) for i in iv] for c, iv in g["intervals"].items()})
    assert {c: [len(x) for x in v] for c, v in got.items()} == g["sizes"]
    more = R.read_frequencies(["#header", "", "chr22\t50\tC\tT\t5\t5", "chr22\t51\tC\tT\t5\t5", "chr22\t52\tC\tT\t5\t4", "chr9\t1\tC\tT\t50\t50", "chr22\t150\tC\tT\t9\t9"], {"chr22": [(1, 50), (51, 150)]})
    # position 50: End 50 is not > 50 and the next interval starts at 51, dropped; 52 has depth 9; chr9 has no intervals; 150 is not below End 150
    assert [[p for p, _, _ in x] for x in more["chr22"]] == [[], [51]]


def test_cipos_reference_case():
    g = GOLDEN["cipos"]
    a = R._Seg(*g["first"][:3], [100, 90, 110, 100, 95, 105]); a.start_ci, a.end_ci = tuple(g["first"][3]), tuple(g["first"][4])
    b = R._Seg(*g["second"][:3], [100, 90, 110, 100, 95, 105]); b.start_ci, b.end_ci = tuple(g["second"][3]), tuple(g["second"][4])
    R.merge_in(a, b)
    assert a.end == g["merged_end"] and a.end_ci[0] == g["merged_end_ci_lower"] and a.start_ci[1] == g["merged_start_ci_upper"] and len(a.counts) == 12


def test_cnv_type_and_allele_copy_numbers_reference_cases():
    for cn, mcc, ref, kind, alleles in GOLDEN["cnv_type_and_allele_copy_numbers"]["cases"]:
        assert R.cnv_type_and_allele_copy_numbers(cn, mcc, ref) == (kind, alleles), (cn, mcc, ref)
    with pytest.raises(ValueError):
        R.cnv_type_and_allele_copy_numbers(2, None, 3)


def test_alt_header_lines_genotypes_and_size_filter_names():
    g = GOLDEN["alt_cn_header"]
    assert R.alt_cn_header_lines(g["max_copy_number"]) == g["lines"] and len(R.alt_cn_header_lines()) == 5
    for c in GOLDEN["alt_alleles_and_genotypes"]["cases"]:
        assert R.alt_alleles_and_genotypes(c["alleles"]) == (c["alt"], c["genotypes"])
    for size, name in GOLDEN["cnv_size_filter"]["cases"]:
        assert R.cnv_size_filter(size) == name


def test_reference_copy_number_on_hand_checked_intervals():
    g = GOLDEN["reference_copy_number"]
    ploidy = {c: [tuple(i) for i in iv] for c, iv in g["ploidy"].items()}
    for chrom, begin, end, want in g["cases"]:
        assert R.reference_copy_number(ploidy, chrom, begin, end) == want, (chrom, begin, end)
