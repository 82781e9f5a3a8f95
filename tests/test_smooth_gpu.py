"""Canvas.smooth (canvas_smooth) on the GPU against the CPU restatement of CanvasSmooth (tests/smooth_ref.py), bit for bit: the fused LDS path, the per-pass path
forced through CANVAS_SMOOTH_PER_PASS in a fresh child process and taken naturally just above the fused limit, the truncation of short chromosomes, the copy of
W = 0, what the call refuses, and that nothing beyond out_n[c] is written.  The cases are in tests/smooth_cases.py; the reference and both device runs are
computed once per session and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import smooth_cases as SC
import smooth_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
GROUPS = ("small", "small-concat", "tile", "many")


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


@pytest.fixture(scope="module")
def cases():
    return SC.cases()


@pytest.fixture(scope="module")
def want(cases):
    return [SC.expected(c) for c in cases]


@pytest.fixture(scope="module")
def fused(cv, cases):
    assert SC.plan(1)["fused"]
    return [SC.run_case(cv, c) for c in cases]


@pytest.fixture(scope="module")
def per_pass(cases, tmp_path_factory):
    """every case again under CANVAS_SMOOTH_PER_PASS, in a process of its own"""
    out = str(tmp_path_factory.mktemp("smooth") / "per_pass.npz")
    env = dict(os.environ, CANVAS_TEST_HOOKS="1")
    env.pop("CANVAS_SMOOTH_PER_PASS", None)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "smooth_cases.py"), out, "--per-pass"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["fused_w1"][0]) == 0, "the hook did not reach the library"
    return [(z["n%d" % i], z["o%d" % i]) for i in range(len(cases))]


def _same(cases, got, want, group):
    k = 0
    for case, (gn, gb), (wn, wb) in zip(cases, got, want):
        if case["group"] != group:
            continue
        k += 1
        assert gn.tolist() == wn.tolist(), case["name"]
        bad = np.nonzero(gb != wb)[0]
        assert len(bad) == 0, (case["name"], case["W"], bad[:8].tolist(), gb[bad[:8]].view(np.float32).tolist(), wb[bad[:8]].view(np.float32).tolist())
    assert k > 0


@pytest.mark.parametrize("group", GROUPS)
def test_fused_path_equals_the_restatement(cases, fused, want, group):
    """counts and lengths bit for bit; whatever lies beyond out_n[c] still holds the sentinel d_out was filled with"""
    _same(cases, fused, want, group)


@pytest.mark.parametrize("group", GROUPS)
def test_per_pass_path_equals_the_fused_path_and_the_restatement(cases, per_pass, fused, want, group):
    _same(cases, per_pass, fused, group)
    _same(cases, per_pass, want, group)


def test_pinned_vector(cv):
    got, n = cv.smooth(to_dev(np.array([2, 1, 3, 5, 4, 6, 7, 8], np.float32), cv.device), [0, 8], 1)
    assert n.tolist() == [8] and got.cpu().numpy().tolist() == [1.5, 2, 3, 4, 5, 6, 7, 7.5]


def test_just_above_the_fused_limit_the_per_pass_path_runs(cv):
    W = SC.largest_fused_w() + 1
    assert not SC.plan(W)["fused"] and SC.plan(W)["launches"] == W
    case = dict(W=W, off=np.array([0, 5000, 5000, 5007], np.int64), counts=np.concatenate([SC.data("ties", 5000, 1), SC.data("big", 7, 2)]))
    wn, wb = SC.expected(case)
    gn, gb = SC.run_case(cv, case)
    assert gn.tolist() == wn.tolist() == [5000, 0, 0] and (gb == wb).all()


def test_w0_is_a_copy(cv):
    case = dict(W=0, off=np.array([2, 10, 10, 4000], np.int64), counts=SC.data("ties", 4003, 5))
    gn, gb = SC.run_case(cv, case)
    assert gn.tolist() == [8, 0, 3990]
    assert (gb[2:4000] == case["counts"][2:4000].view(np.uint32)).all() and (gb[:2] == SC.SENTINEL).all() and (gb[4000:] == SC.SENTINEL).all()


def test_w_larger_than_every_chromosome_writes_nothing(cv):
    rng = np.random.RandomState(8)
    lens = rng.randint(0, 41, 200)
    for W in (41, SC.largest_fused_w() + 30):                                   # the per-pass path either way: W = 41 is past the fused limit as well
        case = SC._one("x", "x", W, [SC.data("ties", int(n), i) for i, n in enumerate(lens)])
        gn, gb = SC.run_case(cv, case)
        assert gn.tolist() == [0] * 200 and (gb == SC.SENTINEL).all()
    W = SC.largest_fused_w()                                                    # and on the fused path: chromosomes shorter than W
    case = SC._one("x", "x", W, [SC.data("ties", int(n) % W, i) for i, n in enumerate(lens)])
    gn, gb = SC.run_case(cv, case)
    assert gn.tolist() == [0] * 200 and (gb == SC.SENTINEL).all()


def test_refused_calls_leave_the_context_usable(cv):
    import torch
    from canvas_amd import CanvasError
    x = SC.data("ties", 9000, 3)
    ok_case = dict(W=2, off=np.array([0, 9000], np.int64), counts=x)
    want = SC.expected(ok_case)

    def refused(fn, text):
        with pytest.raises(CanvasError) as e:
            fn()
        assert "error -1" in str(e.value) and text in str(e.value), str(e.value)
        gn, gb = SC.run_case(cv, ok_case)
        assert gn.tolist() == want[0].tolist() and (gb == want[1]).all()

    for W in (0, 2, SC.largest_fused_w() + 1):                                  # the copy, the fused path, the per-pass path
        for bad in (np.nan, np.inf, -np.inf):
            y = x.copy(); y[4321] = bad; y[8000] = bad
            refused(lambda: cv.smooth(to_dev(y, cv.device), [0, 9000], W), "index 4321")
    d = to_dev(x, cv.device)
    refused(lambda: cv.smooth(d, [0, 9000], 2, out=d), "overlap")
    both = torch.zeros(12000, dtype=torch.float32, device=cv.device)
    refused(lambda: cv.smooth(both[:9000], [0, 9000], 2, out=both[3000:]), "overlap")
    refused(lambda: cv.smooth(d, [0, 9000], -1), "negative")
    refused(lambda: cv.smooth(d, [0, 5000, 4000, 9000], 1), "non-decreasing")
