"""Canvas.call_somatic (canvas_call_somatic) on the GPU against BOTH restatements of tests/somatic_call_ref.py on every case of tests/somatic_call_cases.py: every output of
every stage, doubles and floats as bit patterns; the error codes with the stages they leave filled; the two routes of MeanCount against each other."""
import os

import numpy as np
import pytest

import somatic_call_cases as C
import somatic_call_ref as CR
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def run(cv, case):
    dev = {k: to_dev(case[k], cv.device) for k in ("counts", "site_pos", "site_ref", "site_alt")}
    return cv.call_somatic(dev["counts"], case["chr_seg_offset"], case["seg_begin"], case["seg_end"], case["seg_bin_offset"], case["chr_site_offset"], dev["site_pos"], dev["site_ref"],
                           dev["site_alt"], case["genome_length"], seg_ref_cn=case.get("seg_ref_cn"), excluded=case.get("excluded"), **case["params"])


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_output_of_every_stage_equals_both_restatements(cv, name):
    got = run(cv, C.built(name))
    for want in (C.literal(name), C.arrays(name)):
        assert not isinstance(want, Exception), want
        assert CR.differences(got, want) == []
        assert ((got["seg_mean_route"] != -1) == want["mean_needed"]).all()              # MeanCount is read exactly where the best ploidy is MaximumCopyNumber
    assert got["stages"] == 6 and got["heterogeneity_proportion"] == 0.0


def test_reference_copy_number_may_be_left_out(cv):
    """NULL means 2 everywhere"""
    case = dict(C.built("base"))
    assert (case["seg_ref_cn"] == 2).all()
    want = C.literal("base")
    del case["seg_ref_cn"]
    assert CR.differences(run(cv, case), want) == []


@pytest.mark.parametrize("name,code,stages", [("2 usable", -8, 2), ("no reference 2", -1, 2), ("level 0", -1, 2), ("no model", -6, 3)])
def test_error_codes_leave_the_earlier_stages_filled(cv, name, code, stages):
    from canvas_amd import CanvasError, lib as L
    assert (L.ERR_SOMATIC_FEW_SEGMENTS, L.ERR_SOMATIC_NO_MODEL) == (-8, -6)
    with pytest.raises(CanvasError) as e:
        run(cv, C.built(name))
    assert e.value.code == code, str(e.value)
    for want in (C.literal(name), C.arrays(name)):
        assert isinstance(want, Exception) and want.partial["stages"] == stages
        assert e.value.partial["stages"] == stages
        assert CR.differences(e.value.partial, want.partial) == []
    text = str(e.value)
    assert {"2 usable": "less than 3 usable segments", "no reference 2": "reference copy number 2", "level 0": "median coverage level is 0", "no model": "ploidy filter"}[name] in text, text
    assert CR.differences(run(cv, C.built("base")), C.literal("base")) == []             # the context is still usable


def test_no_score_passes_through(cv):
    """a fit in which no model scores above 0: the weighting factors of the sub-scores are all negative"""
    from canvas_amd import CanvasError
    case = dict(C.built("base"), params=dict(C.built("base")["params"], cn2_weighting_factor=0.0, deviation_score_weighting_factor=-1.0, diploid_distance_score_weighting_factor=-1.0))
    with pytest.raises(CanvasError) as e:
        run(cv, case)
    assert e.value.code == -7 and e.value.partial["stages"] == 3 and e.value.partial["fit"]["nscored"] > 0


def test_mean_count_routes_agree(cv):
    """the workgroup's integer sum is taken exactly where its proof holds, the ordered walk elsewhere, and the walk gives the same bits where both apply"""
    from canvas_amd import lib as L
    case = C.built("high copy number")
    want = C.literal("high copy number")
    nseg = len(case["seg_begin"])
    high = np.nonzero(want["mean_needed"])[0]
    spread = int(np.argmax(np.diff(case["seg_bin_offset"]) == 5000))
    assert os.environ.get("CANVAS_TEST_HOOKS") and "CANVAS_SOMATIC_MEAN" not in os.environ
    got = run(cv, case)
    expect = np.full(nseg, L.SOMATIC_MEAN_NONE); expect[high] = L.SOMATIC_MEAN_EXACT; expect[spread] = L.SOMATIC_MEAN_WALK
    assert (got["seg_mean_route"] == expect).all()
    os.environ["CANVAS_SOMATIC_MEAN"] = "walk"
    try:
        walked = run(cv, case)
    finally:
        del os.environ["CANVAS_SOMATIC_MEAN"]
    expect[high] = L.SOMATIC_MEAN_WALK
    assert (walked["seg_mean_route"] == expect).all()
    assert CR.differences(walked, want) == [] and CR.differences(got, want) == []
    assert (CR.bits(walked["seg_mean_count"]) == CR.bits(got["seg_mean_count"])).all()
    # the walk is in bin order: on the 5 000-bin segment any other order of the additions rounds to the next float (tests/test_somatic_call_ref.py shows it on the CPU)
    x = case["counts"][case["seg_bin_offset"][spread]:case["seg_bin_offset"][spread + 1]].astype(np.float64)
    elsewise = float(np.float32(np.sum(x))) / 5000
    assert got["seg_mean_count"][spread] == want["seg_mean_count"][spread] != elsewise and got["seg_cn"][spread] != round(2 * elsewise / 20.0)
