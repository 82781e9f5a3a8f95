"""Canvas.segment_select (canvas_segment_select) on the GPU against numpy sorting, bit for bit, in its three modes (median with the even-length average in float, in
double, upper median), with the default dispatch over the size classes and with each class forced through CANVAS_CALL_CLASS on every segment it can hold.  The segment
lengths sit at the edges of the classes (the bounds are read from segment_select_plan, not copied), the key patterns are the ones a selection can get wrong (ties, a split
exactly at the middle, descending order, a zero, a middle pair whose float and double averages differ).  The reference is computed once per session."""
import os

import numpy as np
import pytest

from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
MODES = (0, 1, 2)                                            # SELECT_MEDIAN_F32, SELECT_MEDIAN_F64, SELECT_UPPER
PATTERNS = ("equal", "split", "descending", "zero", "avgdiff", "random")
LEAD = 3                                                     # values in front of the first segment: the offsets need not start at 0


def plan():
    from canvas_amd.lib import segment_select_plan
    return segment_select_plan()


def lengths():
    p = plan()
    assert p["wave_max"] == 64 and p["lds_max"] > 65 and 70000 > p["lds_max"] + 1 and 70000 > 2 * p["tile"]
    return [0, 1, 2, 3, 4, 63, 64, 65, p["lds_max"] - 1, p["lds_max"], p["lds_max"] + 1, 70000]


def pattern(name, n, rng):
    if name == "equal":
        return np.full(n, 97.25, np.float32)
    if name == "split":                                      # two distinct values, the lower one n // 2 times: an even length has one of each at its middle
        x = np.full(n, 103.5, np.float32); x[:n // 2] = 51.75
        return x[rng.permutation(n)]
    if name == "descending":
        return (np.arange(n, 0, -1) * 0.25 + 7).astype(np.float32)
    if name == "zero":
        x = (rng.poisson(100, n) + 1).astype(np.float32)
        if n:
            x[rng.randint(n)] = 0.0
        if n > 70:
            x[rng.randint(0, n, n // 3)] = 0.0               # and a zero as the median's neighbour now and then
        return x
    if name == "avgdiff":                                    # the middle pair is (x, the float after x): their mean is no float, so (a + b) / 2f and the double mean differ
        lo = (1.0 + 0.4 * rng.rand(n)).astype(np.float32); hi = (1.6 + 0.4 * rng.rand(n)).astype(np.float32)
        x = np.where(np.arange(n) < n // 2, lo, hi).astype(np.float32)
        if n >= 2 and n % 2 == 0:
            x[n // 2 - 1] = np.float32(1.5); x[n // 2] = np.nextafter(np.float32(1.5), np.float32(2))
        return x[rng.permutation(n)]
    return (rng.rand(n) * 200).astype(np.float32) * np.float32(rng.choice([1.0, 1e-3, 1e6]))


def expected(values, off, mode):
    """numpy: sort every segment, pick, average where the mode says so; float64 bits"""
    out = np.zeros(len(off) - 1, np.float64)
    for s in range(len(off) - 1):
        a = np.sort(values[off[s]:off[s + 1]]); n = len(a)
        if n == 0:
            continue
        if mode == 2 or n % 2 == 1:
            out[s] = np.float64(a[n // 2])
        elif mode == 0:
            out[s] = np.float64(np.float32(np.float32(a[n // 2 - 1] + a[n // 2]) / np.float32(2)))
        else:
            out[s] = (np.float64(a[n // 2 - 1]) + np.float64(a[n // 2])) / 2
    return out.view(np.int64)


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


@pytest.fixture(scope="module")
def edge():
    """every length x every pattern as one call's segments"""
    rng = np.random.RandomState(11)
    parts, names = [], []
    for n in lengths():
        for p in PATTERNS:
            parts.append(pattern(p, n, rng)); names.append("%s/%d" % (p, n))
    values = np.concatenate([np.full(LEAD, 1e9, np.float32)] + parts)
    off = LEAD + np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    assert not np.signbit(values[values == 0]).any()         # (-0.0 sorts in front of 0.0 on the device and nowhere in particular in numpy)
    return dict(values=values, off=off, names=names, want=[expected(values, off, m) for m in MODES], nempty=len(PATTERNS))


@pytest.fixture(scope="module")
def tiny():
    """20 000 segments of 1 .. 5 values"""
    rng = np.random.RandomState(12)
    lens = rng.randint(1, 6, 20000)
    values = np.round(rng.poisson(60, int(lens.sum())) * rng.choice([1.0, 0.5, 0.01], int(lens.sum())), 2).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(values=values, off=off, names=["tiny/%d" % i for i in range(len(lens))], want=[expected(values, off, m) for m in MODES], nempty=0)


def run(cv, case, mode, forced=None):
    old = os.environ.pop("CANVAS_CALL_CLASS", None)
    try:
        if forced:
            os.environ["CANVAS_CALL_CLASS"] = forced
        assert plan()["forced"] == forced, "the hook did not reach the library"
        out, nempty = cv.segment_select(to_dev(case["values"], cv.device), case["off"], mode)
    finally:
        os.environ.pop("CANVAS_CALL_CLASS", None)
        if old is not None:
            os.environ["CANVAS_CALL_CLASS"] = old
    assert nempty == case["nempty"]
    return out.cpu().numpy().view(np.int64)


def same(case, got, want):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(case["names"][i], got[i:i + 1].view(np.float64)[0], want[i:i + 1].view(np.float64)[0]) for i in bad[:8]]


def test_the_double_average_flag_is_really_tested(edge):
    """some even-length segment has a middle pair whose float average and double average differ in bits"""
    differ = np.nonzero(edge["want"][0] != edge["want"][1])[0]
    assert any(edge["names"][i].startswith("avgdiff") for i in differ)
    n = np.diff(edge["off"])
    assert (n[differ] % 2 == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_default_dispatch_equals_numpy(cv, edge, mode):
    same(edge, run(cv, edge, mode), edge["want"][mode])


@pytest.mark.parametrize("forced", ("wave", "lds", "tiled"))
@pytest.mark.parametrize("mode", MODES)
def test_each_forced_class_equals_the_default_dispatch_and_numpy(cv, edge, mode, forced):
    got = run(cv, edge, mode, forced)
    same(edge, got, run(cv, edge, mode))
    same(edge, got, edge["want"][mode])


@pytest.mark.parametrize("forced", (None, "lds", "tiled"))
@pytest.mark.parametrize("mode", MODES)
def test_many_tiny_segments(cv, tiny, mode, forced):
    if forced == "tiled":                                     # 16 KiB of histograms per rank: the tiled class is not for thousands of segments, 300 of them say as much
        k = 300
        tiny = dict(values=tiny["values"], off=tiny["off"][:k + 1], names=tiny["names"][:k], want=[w[:k] for w in tiny["want"]], nempty=0)
    same(tiny, run(cv, tiny, mode, forced), tiny["want"][mode])


def test_pinned_vector(cv):
    x = np.array([5, 1, 4, 2, 9, 7, 3], np.float32)          # segments [5 1 4 2], [], [9 7 3]
    for mode, want in ((0, [3.0, 0.0, 7.0]), (1, [3.0, 0.0, 7.0]), (2, [4.0, 0.0, 7.0])):
        out, nempty = cv.segment_select(to_dev(x, cv.device), [0, 4, 4, 7], mode)
        assert nempty == 1 and out.cpu().numpy().tolist() == want


def test_non_finite_values_are_refused_in_every_class(cv):
    from canvas_amd import CanvasError
    p = plan()
    ok = np.arange(1, 8, dtype=np.float32)
    for n in (5, 64, 65, p["lds_max"], p["lds_max"] + 1, 70000):
        for bad in (np.nan, np.inf, -np.inf):
            x = (np.arange(n + 2) % 50 + 1).astype(np.float32); x[1 + n // 2] = bad; x[n] = bad
            with pytest.raises(CanvasError) as e:
                cv.segment_select(to_dev(x, cv.device), [1, n + 1], 0)
            assert "error -1" in str(e.value) and "index %d" % (1 + n // 2) in str(e.value), str(e.value)
            out, _ = cv.segment_select(to_dev(ok, cv.device), [0, 7], 0)         # the context is still usable
            assert out.cpu().numpy().tolist() == [4.0]
