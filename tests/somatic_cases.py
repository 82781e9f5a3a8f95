"""Inputs of the canvas_somatic_model_fit tests, from fixed seeds.  A case is the dict tests/somatic_ref.py describes.  The synthetic tumour: segments drawn from the
model points of a true (coverage, purity) model with a little noise, weight = length (as GetUsableSegmentsAndSourcesForModeling sets it for whole-genome data)."""
import numpy as np

import somatic_ref as R

TILE = 256           # canvas_amd.lib.SOMATIC_TILE (tests/test_somatic_abi.py checks that they agree)
GENOME = 3_000_000_000


def segments(seed, n, true_coverage=14, true_percent=98, max_cn=8, no_maf=0.25, cns=(1, 2, 2, 2, 3, 4), noise=1.0):
    rng = np.random.default_rng(seed)
    pts = R._Scalar().model_points(true_coverage, true_percent, max_cn)
    usable = [p for p in pts if p["cn"] in cns and p["cn"] <= max_cn]
    pick = rng.integers(0, len(usable), n)
    cov = np.array([usable[k]["coverage"] for k in pick]) + rng.normal(0, 0.25 * noise, n)
    maf = np.clip(np.array([usable[k]["maf"] for k in pick]) + rng.normal(0, 0.015 * noise, n), 0.0, 0.5)
    maf[rng.random(n) < no_maf] = -1.0
    length = rng.integers(5_000, 5_000_000, n).astype(np.int32)
    return np.abs(cov), maf, length.astype(np.float64), length


def case(seed=1, n=40, coverages=(13, 15), hard_limit=96, mmac=0.0, fixed_percent_purity=-1, fixed_coverage=-1, is_enrichment=False, params=None, **seg):
    cov, maf, w, length = segments(seed, n, **seg)
    return dict(coverage=cov, maf=maf, weight=w, length=length, cwf=0.6 / float(np.median(cov)), genome_length=GENOME, min_coverage=coverages[0], max_coverage=coverages[1],
                hard_limit=hard_limit, mmac=mmac, is_enrichment=is_enrichment, fixed_percent_purity=fixed_percent_purity, fixed_coverage=fixed_coverage, params=dict(params or {}))


SIZES = (3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def size_case(n):
    """3 coverages x 5 purities (96 .. 100)"""
    return case(seed=100 + n, n=n)


def max_cn_case(k):
    return case(seed=200 + k, n=70, max_cn=k, cns=tuple(c for c in (1, 2, 2, 3, 4) if c <= k), params=dict(maximum_copy_number=k))


def maf_none_case():
    return case(seed=301, n=60, no_maf=1.0)


def maf_all_case():
    return case(seed=302, n=60, no_maf=0.0)


def maf_mixed_case():
    return case(seed=303, n=60, no_maf=0.5)


def maf_exact_case():
    """MAFs of exactly 0.4 and 0.5 on copy number 2 / 4 coverage, and 0.399 beside them"""
    c = case(seed=304, n=60, no_maf=0.0)
    c["coverage"][:6] = [14.0, 14.0, 14.0, 28.0, 28.0, 14.1]
    c["maf"][:6] = [0.4, 0.5, 0.399, 0.4, 0.5, 0.4]
    return c


def tie_case():
    """segment 0 has no MAF and lies exactly midway between the coverages of copy number 1 (7) and 2 (14) of the model (14, 100 %): both are at the same distance, and
    segment 1 (no MAF, on the coverage of copy number 2) is at the same distance from both points of copy number 2"""
    c = case(seed=305, n=40)
    c["coverage"][:2] = [10.5, 14.0]
    c["maf"][:2] = [-1.0, -1.0]
    return c


def purity_5_case():
    return case(seed=401, n=40, true_percent=60, hard_limit=5, mmac=6.3, fixed_coverage=14)       # 100 * (1 - 2 * 6.3 / 14) - 10 = 0: the hard limit decides


def coverage_10_case():
    return case(seed=402, n=40, true_coverage=10, coverages=(10, 10))


def fixed_case():
    return case(seed=403, n=40, true_percent=70, hard_limit=20, fixed_percent_purity=70, fixed_coverage=14)


def mmac_case():
    """hard limit 81: the lower purity is 81 for coverages 10 .. 12 and 82 or 83 above"""
    return case(seed=404, n=30, true_percent=90, coverages=(10, 16), hard_limit=81, mmac=0.5)


FLOAT_PURITIES = (29, 57, 58)


def float_purity_case(percent):
    return case(seed=500 + percent, n=40, true_percent=percent, hard_limit=20, fixed_percent_purity=percent)


def ploidy_filter_case():
    """purity 100 %, coverages 8 .. 24 around a true 14: the model ploidy falls as the diploid coverage grows, and the window 1.9 .. 2.6 cuts on both sides"""
    return case(seed=601, n=40, true_percent=100, coverages=(8, 24), fixed_percent_purity=100, params=dict(min_allowed_ploidy=1.9, max_allowed_ploidy=2.6))


def fallback_case():
    """15 models, one of them far better than the rest: fewer than DeviationIndexCutoff = 11 lie within DeviationFactor"""
    return case(seed=602, n=50)


def equal_score_case():
    """only the diploid distance scores: every model with the best copy-number profile has the same score, and the first of them wins"""
    return case(seed=603, n=40, params=dict(cn2_weighting_factor=0.0, deviation_score_weighting_factor=0.0))


def few_candidates_case():
    return case(seed=604, n=40, noise=6.0, params=dict(maximum_related_models=64))


def full_width_case():
    return case(seed=701, n=300, true_coverage=17, true_percent=64, coverages=(10, 25), hard_limit=20, mmac=9.0, noise=5.0)       # 90 - 200 * 9 / 25 = 18 < 20: purities 20 .. 100 everywhere


def no_model_case():
    return case(seed=801, n=20, params=dict(min_allowed_ploidy=0.5, max_allowed_ploidy=0.6))


def no_score_case():
    """score = lowPurityWeightingFactor * (PercentCN[2] / bestCN2 - 1) <= 0 for every model"""
    return case(seed=802, n=20, params=dict(cn2_weighting_factor=1.0, deviation_score_weighting_factor=0.0, diploid_distance_score_weighting_factor=0.0))


def cluster_bit_case(n, is_enrichment):
    return case(seed=900 + n, n=n, no_maf=0.0, fixed_percent_purity=98, fixed_coverage=14, is_enrichment=is_enrichment)


def invalid_cases():
    """name -> case the entry must refuse with CANVAS_ERR_INVALID"""
    out = {}
    out["two segments"] = case(seed=1001, n=2)
    c = case(seed=1002, n=10); c["weight"][:] = 0.0; out["total weight 0"] = c
    c = case(seed=1003, n=10); c["length"][4] = 2 ** 31 // 8 + 1; out["length times MaximumCopyNumber leaves int32"] = c
    out["empty grid"] = case(seed=1004, n=10, coverages=(15, 13))
    out["MaximumCopyNumber 1"] = case(seed=1005, n=10, params=dict(maximum_copy_number=1))
    out["MaximumCopyNumber 11"] = case(seed=1006, n=10, params=dict(maximum_copy_number=11))
    return out


SMALL = dict([("size %d" % n, lambda n=n: size_case(n)) for n in SIZES] + [("max_cn %d" % k, lambda k=k: max_cn_case(k)) for k in (2, 3, 8, 10)] +
             [("maf none", maf_none_case), ("maf all", maf_all_case), ("maf mixed", maf_mixed_case), ("maf exact", maf_exact_case), ("tie", tie_case),
              ("purity 5", purity_5_case), ("coverage 10", coverage_10_case), ("fixed", fixed_case), ("mmac", mmac_case)] +
             [("float purity %d" % p, lambda p=p: float_purity_case(p)) for p in FLOAT_PURITIES] +
             [("ploidy filter", ploidy_filter_case), ("fallback", fallback_case), ("equal score", equal_score_case), ("few candidates", few_candidates_case)])


# ---- the references, computed once per process and shared by the tests (never modified by them)
import functools


def _catch(fn, c):
    try:
        return fn(c)
    except (R.NoModel, R.NoScore) as e:
        return e


@functools.lru_cache(maxsize=None)
def built(name):
    return SMALL[name]() if name in SMALL else dict(full_width=full_width_case, no_model=no_model_case, no_score=no_score_case)[name]()


@functools.lru_cache(maxsize=None)
def scalar(name):
    return _catch(R.fit_scalar, built(name))


@functools.lru_cache(maxsize=None)
def vectorised(name):
    return _catch(R.fit_vectorised, built(name))


def bits(x):
    a = np.ascontiguousarray(x)
    return a.astype(np.float64).view(np.uint64) if a.dtype.kind == "f" else a.astype(np.int64)


RESULT_FIELDS = ("model", "coverage", "percent_purity", "info", "nmodels", "nvalid", "nscored", "purity", "deviation", "precision_deviation", "accuracy_deviation", "ploidy",
                 "percent_normal", "diploid_distance", "percent_cn", "score", "inter_model_distance", "best_deviation", "worst_allowed_deviation", "seg_point", "seg_distance")
MODEL_FIELDS = ("coverage", "percent_purity", "deviation", "precision_deviation", "accuracy_deviation", "ploidy", "percent_normal", "percent_cn", "diploid_distance", "flags", "score")


def differences(x, y, fields=RESULT_FIELDS, models=True):
    """names of the fields of two results whose bit patterns differ"""
    bad = [k for k in fields if k in x or k in y if k not in x or k not in y or bits(x[k]).shape != bits(y[k]).shape or not np.array_equal(bits(x[k]), bits(y[k]))]
    if models:
        bad += ["models." + k for k in MODEL_FIELDS if bits(x["models"][k]).shape != bits(y["models"][k]).shape or not np.array_equal(bits(x["models"][k]), bits(y["models"][k]))]
    return bad
