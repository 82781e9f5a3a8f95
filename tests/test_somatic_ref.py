"""The two restatements of the somatic model fit (tests/somatic_ref.py) agree bit for bit on every small case, a few facts checked by hand hold, and every case of
tests/somatic_cases.py really reaches the branch it is named after.  No GPU, no library."""
import numpy as np
import pytest

import somatic_cases as Cs
import somatic_ref as R


@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_scalar_equals_vectorised(name):
    a, b = Cs.scalar(name), Cs.vectorised(name)
    assert not isinstance(a, Exception) and not isinstance(b, Exception)
    assert Cs.differences(a, b) == []
    grid, max_cn = R.grid_of(Cs.built(name)), R.params_of(Cs.built(name))["maximum_copy_number"]
    pc, pm = R.table_vectorised(grid, max_cn)
    initial = R._Scalar()
    for m, (cov, percent) in enumerate(grid):                  # the tables before RefineDiploidMAF
        pts = initial.model_points(cov, percent, max_cn)
        assert np.array_equal(Cs.bits([p["coverage"] for p in pts]), Cs.bits(pc[m])) and np.array_equal(Cs.bits([p["maf"] for p in pts]), Cs.bits(pm[m]))


def test_error_cases_agree():
    for name, kind in (("no_model", R.NoModel), ("no_score", R.NoScore)):
        a, b = Cs.scalar(name), Cs.vectorised(name)
        assert isinstance(a, kind) and isinstance(b, kind)
        assert Cs.differences(a.args[0], b.args[0], fields=("nmodels", "nvalid", "nscored", "info", "model")) == []
    assert Cs.scalar("no_model").args[0]["nvalid"] == 0 and Cs.scalar("no_score").args[0]["nscored"] > 0


def test_point_counts_and_order():
    assert len(R.ploidies(8)) == 25 and len(R.ploidies(10)) == 36 and len(R.ploidies(2)) == 4 and len(R.ploidies(3)) == 6
    assert R.ploidies(4) == [(0, 0), (1, 1), (2, 2), (2, 1), (3, 3), (3, 2), (4, 4), (4, 3), (4, 2)]


def test_float_purity_differs_from_the_double_quotient():
    for percent in Cs.FLOAT_PURITIES:
        assert R.purity_of(percent) != percent / 100.0
        c = Cs.built("float purity %d" % percent)
        f, d = R.table_vectorised(R.grid_of(c), 8), R.table_vectorised(R.grid_of(c), 8, double_division=True)
        assert np.count_nonzero(Cs.bits(f[0]) != Cs.bits(d[0])) > 0 and np.count_nonzero(Cs.bits(f[1]) != Cs.bits(d[1])) > 0        # a point's coverage and a point's MAF change
        assert Cs.differences(Cs.scalar("float purity %d" % percent), R.fit_scalar(c, double_division=True)) != []


def _model(case, coverage, percent):
    p = R.params_of(case)["maximum_copy_number"]
    return R.model_deviation_scalar(case, R._Scalar().model_points(coverage, percent, p), p)


def test_tie_rules():
    c = Cs.built("tie")
    pts = R._Scalar().model_points(14, 100, 8)
    assert (pts[1]["cn"], pts[1]["coverage"]) == (1, 7.0) and (pts[2]["cn"], pts[2]["major"], pts[2]["coverage"]) == (2, 2, 14.0) and pts[3]["coverage"] == 14.0
    d = [R.distance(10.5, p["coverage"], -1.0, p["maf"], c["cwf"]) for p in pts]
    assert d[1] == d[2] == d[3] == min(d)                                    # a tie between copy number 1 and both points of copy number 2
    m = _model(c, 14, 100)
    assert m["seg_point"][0] == 1 and m["cns"][0] == 1                       # the first point of the tie
    assert m["seg_point"][1] == 2 and m["cns"][1] == 1                       # no MAF on copy number 2: the LOH point (major == copy number), profile entry 1 ...
    # ... and nothing towards PercentNormal: without the segment the normal bases are the same, only the total weight changes
    w = np.asarray(c["weight"], np.float64)
    normal = [s for s in range(len(w)) if m["seg_point"][s] == 3]
    assert 1 not in normal and len(normal) > 0
    total = tw = 0.0
    for s in range(len(w)):
        tw += w[s]
        if s in normal:
            total += w[s]
    assert m["percent_normal"] == total / tw
    assert (Cs.scalar("tie")["coverage"], 100) in [tuple(g) for g in R.grid_of(c)]            # the model of the tie is in the grid the GPU test runs


def test_refinement_takes_0_4_and_leaves_0_399():
    base = Cs.built("maf exact")
    def refined(maf0):
        c = dict(base, coverage=base["coverage"].copy(), maf=base["maf"].copy())
        c["coverage"][:] = 21.0; c["maf"][:] = 0.33                         # everything else on copy number 3: no other segment enters the refinement
        c["coverage"][0] = 14.0; c["maf"][0] = maf0
        pts = R._Scalar().model_points(14, 100, 8)
        before = pts[3]["maf"]
        R._refine_diploid_maf(c, pts, 8)
        return before, pts[3]["maf"]
    before, after = refined(0.4)
    assert after == (10000000.0 * before + base["weight"][0] * 0.4) / (10000000.0 + base["weight"][0]) and after != before
    before, after = refined(0.399)
    assert after == (10000000.0 * before) / 10000000.0
    assert set(base["maf"][:6]) == {0.4, 0.5, 0.399}


def test_a_point_of_weight_0_is_skipped():
    c = Cs.built("maf all")
    m = _model(c, 14, 98)
    empty = [p for p in m["points"] if p["weight"] == 0]
    assert len(empty) > 0 and all(p["emp_cov"] == 0 and p["emp_maf"] == 0 for p in empty)
    acc = 0.0
    for p in m["points"]:
        if p["weight"] != 0:
            acc += np.sqrt(R.distance(p["coverage"], p["emp_cov"], p["maf"], p["emp_maf"], c["cwf"])) * p["weight"]
    tw = 0.0
    for w in c["weight"]:
        tw += w
    assert m["accuracy_deviation"] == acc / tw and np.isfinite(m["accuracy_deviation"])


def test_cases_reach_their_branches():
    S = Cs.scalar
    # the DeviationIndexCutoff fallback fires with fewer than 11 models within DeviationFactor, and not otherwise
    f = S("fallback")
    assert f["counter"] < 11 and f["info"] & R.INFO_INDEX_CUTOFF
    dev = np.sort(np.asarray(f["models"]["deviation"])[np.asarray(f["models"]["flags"]) != 0])
    assert f["worst_allowed_deviation"] == dev[min(11, len(dev) - 1)] and f["worst_allowed_deviation"] != f["best_deviation"] * 1.75
    n = S("few candidates")
    assert n["counter"] >= 11 and not n["info"] & R.INFO_INDEX_CUTOFF and n["worst_allowed_deviation"] == n["best_deviation"] * 1.75
    assert 1 < n["ncandidates"] < 64 and n["inter_model_distance"] > 0
    # the ploidy filter removes models on both sides
    p = S("ploidy filter")
    pl, fl = np.asarray(p["models"]["ploidy"]), np.asarray(p["models"]["flags"])
    assert (pl[fl == 0] >= np.float32(2.6)).any() and (pl[fl == 0] <= np.float32(1.9)).any() and 0 < p["nvalid"] < p["nmodels"]
    # two models of equal best score: the earlier one wins
    e = S("equal score")
    sc = np.asarray(e["models"]["score"])
    same = np.nonzero(Cs.bits(sc) == Cs.bits(e["score"]))[0]
    assert len(same) >= 2 and e["model"] == same[0] and e["score"] == sc.max()
    # purity and coverage edges
    assert S("purity 5")["models"]["percent_purity"][0] == 5 and S("purity 5")["nmodels"] == 96
    assert set(S("coverage 10")["models"]["coverage"]) == {10} and S("fixed")["nmodels"] == 1
    mm = S("mmac")["models"]
    lows = {c: int(np.asarray(mm["percent_purity"])[np.asarray(mm["coverage"]) == c].min()) for c in range(10, 17)}
    assert lows[10] == lows[11] == lows[12] == 81 and lows[13] == 82 and lows[16] == 83
    pts = R._Scalar().model_points(14, 100, 8)                               # purity 100: no normal contribution, copy number 0 at coverage 0, the early returns
    assert pts[0]["coverage"] == 0 and pts[0]["maf"] == 0 and all(q["maf"] == 0 for q in pts if q["major"] == q["cn"]) and pts[3]["maf"] > 0.3
    assert 100 in S("size 64")["models"]["percent_purity"]
    # MAF edges
    assert (Cs.built("maf none")["maf"] < 0).all() and (Cs.built("maf all")["maf"] >= 0).all() and 0 < (Cs.built("maf mixed")["maf"] < 0).sum() < 60
    # the full-width case: coverages 10 .. 25, purities 20 .. 100, about a quarter of the 300 segments without MAF
    fw = Cs.built("full_width")
    g = R.grid_of(fw)
    assert len(g) == 16 * 81 and g[0] == (10, 20) and g[-1] == (25, 100) and len(fw["maf"]) == 300 and 50 < (fw["maf"] < 0).sum() < 100


def test_cluster_term_bit():
    assert R.info_of(Cs.cluster_bit_case(101, False)) == R.INFO_CLUSTER_TERM
    assert R.info_of(Cs.cluster_bit_case(101, True)) == 0 and R.info_of(Cs.cluster_bit_case(100, False)) == 0
    assert (Cs.cluster_bit_case(101, False)["maf"] >= 0).sum() == 101
