"""Canvas.call_diploid (canvas_call_diploid) on the GPU against BOTH CPU restatements of tests/diploid_ref.py, every output array bit for bit: the hand-built case with
every boundary of the caller (tests/diploid_cases.py; tests/test_diploid_ref.py checks that the restatements take those branches), randomised cases, the serial-sum case
(three million counts, the one large array: compared with the vectorised restatement and a plain serial loop), and what the call refuses."""
import numpy as np
import pytest

import diploid_cases as DC
import diploid_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
FLOATS = ("median_count", "median_maf", "dist", "dist2", "run_median_count")


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def run(cv, case, **kw):
    a = dict(case)
    dev = {k: to_dev(a[k], cv.device) for k in ("counts", "site_pos", "site_ref", "site_alt")}
    return cv.call_diploid(dev["counts"], a["chr_seg_offset"], a["seg_begin"], a["seg_end"], a["seg_bin_offset"], a["chr_site_offset"], dev["site_pos"], dev["site_ref"], dev["site_alt"], **kw)


def same(got, want):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            x, y = (g.view(np.int64), w.view(np.int64)) if k in FLOATS else (g.astype(np.int64), w.astype(np.int64))
            assert x.shape == y.shape, (k, x.shape, y.shape)
            bad = np.nonzero(x != y)[0]
            assert len(bad) == 0, (k, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
        elif isinstance(w, float):
            assert np.float64(g).view(np.int64) == np.float64(w).view(np.int64), (k, g, w)
        else:
            assert g == w, (k, g, w)


def test_hand_built_case_equals_both_restatements(cv):
    case, names = DC.edge_case()
    got = run(cv, case)
    same(got, R.direct(*DC.args(case)))
    same(got, R.vectorised(*DC.args(case)))
    assert got["integer_sum"] and got["diploid_coverage"] == 100.0


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_randomised_cases_equal_both_restatements(cv, seed):
    case = DC.random_case(seed)
    got = run(cv, case)
    same(got, R.direct(*DC.args(case)))
    same(got, R.vectorised(*DC.args(case)))


def test_other_coefficients_and_confidence_intervals(cv):
    case = DC.random_case(4, nchr=2, nseg=40)
    b = (-1.5, 2.25, -30.0, -0.75)
    nseg = len(case["seg_begin"])
    ci0 = np.stack([-np.arange(nseg), np.arange(nseg)], 1); ci1 = ci0 * 2
    got = run(cv, case, logistic=b, seg_start_ci=ci0, seg_end_ci=ci1)
    same(got, R.direct(*DC.args(case), logistic=b))
    same(got, R.vectorised(*DC.args(case), logistic=b))
    assert (got["run_start_ci"] == ci0[got["run_first"]]).all() and (got["run_end_ci"] == ci1[got["run_last"]]).all()


def test_serial_sum_of_three_million_counts(cv):
    """counts below 0.5 that are no multiples of 2^-24: the integer sum on the device is refused by its own check and the mean is the serial sum in bin order"""
    case = DC.big_case()
    x = case["counts"].astype(np.float64)
    serial = 0.0
    for v in x.tolist():
        serial += v
    serial /= len(x)
    assert serial != float(np.sum(x) / len(x)), "the case must tell a serial sum from a pairwise one"
    got = run(cv, case)
    assert not got["integer_sum"]
    assert np.float64(got["diploid_coverage"]).view(np.int64) == np.float64(serial).view(np.int64)
    same(got, R.vectorised(*DC.args(case)))


def test_refused_calls(cv):
    from canvas_amd import CanvasError
    case, _ = DC.edge_case()
    want = R.vectorised(*DC.args(case))

    def refused(change, text):
        bad = {k: v.copy() for k, v in case.items()}
        change(bad)
        with pytest.raises(CanvasError) as e:
            run(cv, bad)
        assert "error -1" in str(e.value) and text in str(e.value), str(e.value)
        same(run(cv, case), want)                              # the context is still usable

    def unsorted_sites(c):
        c["site_pos"][5], c["site_pos"][6] = c["site_pos"][6] + 1, c["site_pos"][5]
    refused(unsorted_sites, "site 6")
    refused(lambda c: (c["seg_begin"].__setitem__(3, c["seg_begin"][2]), c["seg_end"].__setitem__(3, c["seg_end"][2])), "ends must increase")
    refused(lambda c: c["seg_begin"].__setitem__(3, c["seg_begin"][2] - 1), "begins must not decrease")
    refused(lambda c: c["seg_bin_offset"].__setitem__(4, c["seg_bin_offset"][3]), "has no bins")
    refused(lambda c: c["counts"].__setitem__(777, np.nan), "index 777")
    refused(lambda c: c["site_ref"].__setitem__(slice(None), 0) or c["site_alt"].__setitem__(slice(None), 4), "no site")
    refused(lambda c: c["site_alt"].__setitem__(9, -1), "site 9")
