"""canvas_somatic_model_fit on the GPU against the restatements of tests/somatic_ref.py: equal bit patterns of every double of the result, of the best model's per-segment
assignment and of every model's columns.  The cases (tests/somatic_cases.py) are checked on the CPU to reach the branches they are named after (tests/test_somatic_ref.py);
the references are computed once per process and shared."""
import numpy as np
import pytest

import somatic_cases as Cs
import somatic_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def fit(cv, c, device=False, **kw):
    arrs = [np.ascontiguousarray(c[k], dt) for k, dt in (("coverage", np.float64), ("maf", np.float64), ("weight", np.float64), ("length", np.int32))]
    if device:
        arrs = [to_dev(a, cv.device) for a in arrs]
    return cv.somatic_model_fit(*arrs, c["cwf"], c["genome_length"], c["min_coverage"], c["max_coverage"], minimum_purity_hard_limit=c["hard_limit"],
                                min_minor_allele_coverage=c["mmac"], is_enrichment=c["is_enrichment"], fixed_percent_purity=c["fixed_percent_purity"],
                                fixed_coverage=c["fixed_coverage"], **dict(c["params"], **kw))


def check(cv, name, scalar=True):
    got = fit(cv, Cs.built(name))
    assert Cs.differences(got, Cs.vectorised(name)) == []
    if scalar:
        assert Cs.differences(got, Cs.scalar(name)) == []
    return got


@pytest.mark.parametrize("n", Cs.SIZES)
def test_segment_count_edges(cv, n):
    got = check(cv, "size %d" % n)
    assert got["nmodels"] == 15 and len(got["seg_point"]) == n


@pytest.mark.parametrize("k", (2, 3, 8, 10))
def test_point_count_edges(cv, k):
    got = check(cv, "max_cn %d" % k)
    assert got["percent_cn"].shape == (k + 1,) and got["seg_point"].max() < len(R.ploidies(k))


@pytest.mark.parametrize("name", ("maf none", "maf all", "maf mixed", "maf exact", "tie"))
def test_maf_edges(cv, name):
    check(cv, name)


def test_tie_takes_the_first_point_and_the_loh_point(cv):
    """the one model in which segment 0 is tied between copy numbers 1 and 2: its assignment is in the result"""
    c = dict(Cs.built("tie"), min_coverage=14, max_coverage=14, fixed_percent_purity=100)
    got = fit(cv, c)
    assert Cs.differences(got, R.fit_scalar(c)) == [] and (got["seg_point"][0], got["seg_point"][1]) == (1, 2)


@pytest.mark.parametrize("name", ("purity 5", "coverage 10", "fixed", "mmac"))
def test_purity_and_coverage_edges(cv, name):
    check(cv, name)


@pytest.mark.parametrize("percent", Cs.FLOAT_PURITIES)
def test_purity_is_a_float_quotient(cv, percent):
    got = check(cv, "float purity %d" % percent)
    assert Cs.differences(got, R.fit_vectorised(Cs.built("float purity %d" % percent), double_division=True)) != []


@pytest.mark.parametrize("name", ("ploidy filter", "fallback", "equal score", "few candidates"))
def test_selection(cv, name):
    got = check(cv, name)
    if name == "fallback":
        assert got["info"] & R.INFO_INDEX_CUTOFF
    if name == "few candidates":
        assert not got["info"] & R.INFO_INDEX_CUTOFF and got["nscored"] < 64


def test_full_width(cv):
    got = check(cv, "full_width", scalar=False)
    assert got["nmodels"] == 16 * 81 and got["info"] == R.INFO_CLUSTER_TERM


def test_the_two_exception_codes(cv):
    from canvas_amd import CanvasError
    from canvas_amd.lib import ERR_SOMATIC_NO_MODEL, ERR_SOMATIC_NO_SCORE
    for name, code in (("no_model", ERR_SOMATIC_NO_MODEL), ("no_score", ERR_SOMATIC_NO_SCORE)):
        with pytest.raises(CanvasError) as e:
            fit(cv, Cs.built(name))
        want = Cs.vectorised(name).args[0]
        assert e.value.code == code and e.value.partial["model"] == -1
        assert Cs.differences(e.value.partial, want, fields=("nmodels", "nvalid", "nscored", "info", "model")) == []
        assert Cs.differences(e.value.partial, Cs.scalar(name).args[0], fields=()) == []


def test_every_invalid_condition(cv):
    from canvas_amd import CanvasError
    for device in (False, True):
        for name, c in Cs.invalid_cases().items():
            with pytest.raises(CanvasError) as e:
                fit(cv, c, device=device)
            assert e.value.code == -1, name
    fit(cv, Cs.built("fixed"))                       # the context is fine afterwards


def test_cluster_term_bit(cv):
    assert fit(cv, Cs.cluster_bit_case(101, False))["info"] & R.INFO_CLUSTER_TERM
    assert not fit(cv, Cs.cluster_bit_case(101, True))["info"] & R.INFO_CLUSTER_TERM
    assert not fit(cv, Cs.cluster_bit_case(100, False))["info"] & R.INFO_CLUSTER_TERM
    for n, enrichment in ((101, False), (101, True), (100, False)):         # and the two-term deviation is computed either way
        c = Cs.cluster_bit_case(n, enrichment)
        assert Cs.differences(fit(cv, c), R.fit_vectorised(c)) == []


@pytest.mark.parametrize("name", ("size 257", "mmac"))
def test_device_and_host_inputs_agree(cv, name):
    host, dev = fit(cv, Cs.built(name)), fit(cv, Cs.built(name), device=True)
    assert Cs.differences(host, dev) == [] and Cs.differences(dev, Cs.vectorised(name)) == []
