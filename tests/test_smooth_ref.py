"""The two CPU restatements of CanvasSmooth (tests/smooth_ref.py) against each other, against the vector the reference's own unit test pins, and against the
length recurrence.  No GPU, no library."""
import numpy as np
import pytest

import smooth_ref as R


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_pinned_vector_of_the_reference_unit_test():
    """CanvasTest/TestUtilities.cs:195-206"""
    want = np.array([1.5, 2, 3, 4, 5, 6, 7, 7.5], np.float32)
    x = [2, 1, 3, 5, 4, 6, 7, 8]
    assert (_bits(R.median_filter_literal(x, 1)) == _bits(want)).all()
    assert (_bits(R.median_filter_windows(x, 1)) == _bits(want)).all()
    assert (_bits(R.smooth_literal(x, 1)) == _bits(want)).all() and (_bits(R.smooth_windows(x, 1)) == _bits(want)).all()


def test_length_recurrence():
    """both restatements emit f(n, h) values per pass, and out_len(n, W) of them at the end"""
    rng = np.random.RandomState(3)
    for n in range(0, 41):
        x = rng.randint(0, 50, n).astype(np.float32)
        for h in range(0, 7):
            assert len(R.median_filter_literal(x, h)) == len(R.pass_windows(n, h)) == R.next_len(n, h)
        for W in range(0, 7):
            assert len(R.smooth_literal(x, W)) == len(R.smooth_windows(x, W)) == R.out_len(n, W)
    assert [R.out_len(n, 1) for n in (1, 2, 3)] == [0, 1, 3]               # the issue's examples
    assert [R.out_len(n, 3) for n in (5, 6, 7)] == [3, 5, 7]


def test_the_window_list_is_what_the_queue_does():
    """medians of the listed windows, formed directly, equal the streaming filter's output for h = 0..5, n = 0..15"""
    rng = np.random.RandomState(11)
    for n in range(0, 16):
        x = (rng.randint(0, 6, n) / 4.0).astype(np.float32)
        for h in range(0, 6):
            direct = [R._window_median(x.tolist()[lo:hi + 1]) for lo, hi in R.pass_windows(n, h)]
            assert (_bits(direct) == _bits(R.median_filter_literal(x, h))).all(), (n, h)


@pytest.fixture(scope="module")
def all_cases():
    import smooth_cases as SC
    return SC.cases()


def test_restatements_agree_on_every_case(all_cases):
    for case in all_cases:
        off, x, W = case["off"], case["counts"], case["W"]
        a = R.smooth_genome(x, off, W, R.smooth_literal)
        b = R.smooth_genome(x, off, W, R.smooth_windows)
        assert len(a) == len(b)
        for c, (u, v) in enumerate(zip(a, b)):
            assert len(u) == len(v) == R.out_len(int(off[c + 1] - off[c]), W), (case["name"], c)
            assert (_bits(u) == _bits(v)).all(), (case["name"], c)


def test_the_even_mean_rounds_in_the_big_kind():
    """the 'big' data are there for this: a mean of two floats that is not a float"""
    import smooth_cases as SC
    x = SC.data("big", 64, 1)
    pairs = [(a, b) for a, b in zip(x[:-1], x[1:]) if (float(a) + float(b)) / 2 != float(np.float32((float(a) + float(b)) / 2))]
    assert pairs
