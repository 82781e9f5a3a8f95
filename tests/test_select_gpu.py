"""The order-statistics engine of canvas_amd/csrc/select.hpp on its own, through canvas_select_probe: radix_select with 32- and 64-bit keys (results through the host and
left on the device) and wg_select2, at the key, tile, query and call-sequence edges the stages above it never feed it.  Every key returned must EQUAL the k-th smallest
key of a plain sort (tests/select_ref.py, pinned on the CPU by tests/test_select_ref.py): no tolerance anywhere."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import select_ref as R
from canvas_amd import synth, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
from canvas_amd.lib import CanvasError
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu

WIDTHS = (4, 8)
INVALID = "libcanvas_hip error -1:"          # CANVAS_ERR_INVALID


@functools.lru_cache(maxsize=None)
def _canvas():
    return get_canvas()


def _probe(cv, case, variant):
    lo, hi, k = (np.array([q[i] for q in case.queries], np.int64) for i in range(3))
    return cv.select_probe(variant, R.dtype_code(case.data), case.data, case.seg_off, lo, hi, k)


def _check(case, cv=None, variants=(0, 1)):
    """every query of the case through radix_select, results through the host (0) and left on the device (1)"""
    cv = cv or _canvas()
    want = R.expected(case)
    for variant in variants:
        got = _probe(cv, case, variant)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (case.name, variant, [(case.queries[i], hex(int(got[i])), hex(int(want[i]))) for i in bad[:4]])


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", R.SIZES)
def test_one_segment_of_every_size(n, width):
    for call in R.calls_of(R.size_case(n, width)):
        _check(call)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", R.CONTENT_SIZES)
@pytest.mark.parametrize("kind", R.CONTENT_KINDS)
def test_key_content(kind, n, width):
    for call in R.calls_of(R.content_case(kind, n, width)):
        _check(call)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", R.AGG_NAMES)
def test_ballot_aggregation_paths(name, width):
    _check(R.aggregation_case(name, width))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", R.QUERY_NAMES)
def test_query_sharing(name, width):
    _check(R.query_case(name, width))


@pytest.mark.parametrize("width", WIDTHS)
def test_seventeen_queries_on_one_segment_are_refused_and_the_context_goes_on(width):
    cv = get_canvas()
    _check(R.query_case("sixteen_identical", width), cv)
    for variant in (0, 1):
        with pytest.raises(CanvasError, match=INVALID + ".*too many queries per segment"):
            _probe(cv, R.too_many_queries_case(width), variant)
        _check(R.query_case("sixteen_distinct", width), cv)
    cv.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_segments_like_gc_buckets(width):
    _check(R.segments_case(width))


@pytest.mark.parametrize("width", WIDTHS)
def test_sixteen_queries_on_a_segment_that_union_queries_cover_too(width):
    cv = get_canvas()
    _check(R.segments_case(width, crowded=True), cv)
    for variant in (0, 1):
        with pytest.raises(CanvasError, match=INVALID + ".*too many queries per segment"):
            _probe(cv, R.segments_case(width, crowded=True, one_more=True), variant)
    _check(R.segments_case(width, crowded=True), cv)
    cv.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_call_sequence_on_one_context(width):
    """1, 16, 3, 40 and 2 queries in turn on a fresh context, each on data of its own: prefixes an earlier call left behind, scratch that grows, histograms that must be zero again"""
    cv = get_canvas()
    for variant in (0, 1):
        for case in R.sequence_cases(width):
            _check(case, cv, (variant,))
    cv.close()


def test_device_driven_clean_between_two_selects(monkeypatch):
    """CanvasClean's device-driven chain with its radix selects keeps its histograms in the same buffer of the context: a select before it, the Clean against the oracle
    as tests/test_clean_gpu.py compares it, a select after it"""
    monkeypatch.setenv("CANVAS_CLEAN_RADIX_SELECT", "1")
    flags = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD
    cv = get_canvas()
    _check(R.segments_case(4), cv)
    bins = synth.generate_bins(20261018, 60_000)
    is_auto = synth.IS_AUTOSOME[:24]
    is_y = np.zeros(24, np.uint8); is_y[-1] = 1
    exp = O.clean(bins["chr"], bins["start"], bins["stop"], bins["count"], bins["gc"], is_auto, is_y, flags, min_bins_weighted=100)
    dev = {k: to_dev(v, cv.device) for k, v in bins.items()}
    n_out, lsd, info = cv.clean(dev, len(bins["chr"]), is_auto, flags, min_bins_per_gc=100)
    assert info[6] == 0 and info[7] == 1 and info[5] == 0, info            # the device-driven chain, order statistics by radix select
    assert n_out == len(exp["chr"]), (n_out, len(exp["chr"]), info)
    for k in ("chr", "start", "stop", "gc"):
        assert (dev[k][:n_out].cpu().numpy() == exp[k]).all(), k
    got = dev["count"][:n_out].cpu().numpy()
    assert (got.view(np.uint32) == exp["count"].view(np.uint32)).all()
    assert lsd == exp["local_sd"]
    _check(R.segments_case(8, crowded=True), cv)
    _check(R.query_case("sixteen_distinct", 4), cv)
    cv.close()


def test_argument_checks_leave_the_context_usable():
    cv = get_canvas()
    case = R.query_case("sixteen_distinct", 8)
    n = len(case.data)
    for variant in (0, 1):
        for bad in ([(0, 0, n)], [(0, 0, -1)], [(0, 0, 5), (0, 0, n)]):
            with pytest.raises(CanvasError, match=INVALID):
                _probe(cv, case._replace(queries=bad), variant)
            _check(case, cv, (variant,))
    two = R.Case("two-segments", case.data, np.array([0, 1000, n], np.int64), [(1, 0, 0)])
    for bad_case in (two, two._replace(queries=[(0, 2, 0)]), two._replace(queries=[(-1, 0, 0)]), two._replace(queries=[(0, 0, 1000)]),
                     two._replace(seg_off=np.array([0, n, 1000], np.int64), queries=[(0, 0, 0)])):
        with pytest.raises(CanvasError, match=INVALID):
            _probe(cv, bad_case, 0)
    with pytest.raises(CanvasError, match=INVALID):                          # wg_select2 takes 64-bit keys only
        cv.select_probe(2, 2, R.query_case("sixteen_distinct", 4).data, [0, n], [0], [0], [[0, 0]])
    with pytest.raises(CanvasError, match=INVALID):
        cv.select_probe(2, 3, case.data, [0, n], [0], [0], [[0, n]])
    _check(two._replace(queries=[(0, 0, 999), (1, 1, 0), (0, 1, n - 1)]), cv)
    cv.close()


@pytest.mark.parametrize("kind", R.WG_KINDS)
def test_wg_select2(kind):
    """one launch, one workgroup of 1024 threads per rank pair, over segments of 1 to 5000 keys that start at non-zero offsets"""
    cv = _canvas()
    case = R.wg_case(kind)
    seg = np.array([q[0] for q in case.queries], np.int32)
    pairs = np.array([q[2] for q in case.queries], np.int64)
    want = R.expected_pairs(case)
    got = cv.select_probe(2, R.dtype_code(case.data), case.data, case.seg_off, seg, seg, pairs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (kind, [(case.queries[i], [hex(int(x)) for x in got[i]], [hex(int(x)) for x in want[i]]) for i in bad[:4]])
