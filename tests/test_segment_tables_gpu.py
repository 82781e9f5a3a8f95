"""Canvas.segment_tables (canvas_segment_tables) on the GPU against the restatement of Segments.ReadSegments (tests/segment_tables_ref.py): every table and every float
exactly, at the smallest sizes at which each part of the three launches can go wrong, and every refusal the device decides with the bin it names."""
import numpy as np
import pytest

import segment_tables_ref as S
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
BLOCK = 256                                                  # ST_BLOCK (segtab.hip): bins per workgroup of the flag and scatter kernels
SCAN_WIDTH = 1024                                            # threads of the one workgroup that scans the workgroup counts


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def make(per_chr, seed, ids="random", p_change=0.2, p_abut=0.7):
    """bins of 1 .. 200 bases (odd and even lengths, some of length 0) that abut their predecessor with probability p_abut; every chromosome starts over near 0, so a start may
    go down across a chromosome boundary; ids from a small set that includes negative values, so ids return and run across boundaries.  cov = k / 100"""
    rng = np.random.RandomState(seed)
    n = int(sum(per_chr))
    length = rng.choice([0, 1, 2, 9, 10, 11, 49, 100, 101, 200], n)
    gap = np.where(rng.rand(n) < p_abut, 0, rng.choice([1, 7, 300], n))
    start = np.zeros(n, np.int64); off = np.concatenate([[0], np.cumsum(per_chr)]).astype(np.int64)
    for c in range(len(per_chr)):
        a, b = off[c], off[c + 1]
        if b > a:
            step = (length + gap)[a:b]
            start[a:b] = 5 + np.concatenate([[0], np.cumsum(step[:-1])])
    stop = start + length
    if ids == "random":
        seg = np.cumsum(rng.rand(n) < p_change) % 5 - 2        # -2 .. 2, the change points random: values return after five changes
    elif ids == "each":
        seg = np.arange(n) % 2 - 1                              # one bin per segment
    else:
        seg = np.full(n, 7)                                     # one segment per chromosome
    k = rng.randint(0, 40000, n).astype(np.int64)
    special = rng.rand(n) < 0.05
    k[special] = rng.choice([0, 12800, 3276800, 1677721650], int(special.sum()))      # zero, powers of two, and 16777216.5: a float tie
    return dict(off=off, start=start.astype(np.int32), stop=stop.astype(np.int32), seg=seg.astype(np.int32), cov=k / 100.0)


def run(cv, c, cov=True, **kw):
    return cv.segment_tables(c["off"], to_dev(c["start"], cv.device), to_dev(c["stop"], cv.device), to_dev(c["seg"], cv.device), to_dev(c["cov"], cv.device) if cov else None, **kw)


def check(cv, c, **kw):
    got = run(cv, c, **kw)
    want = S.from_arrays(c["off"], c["start"], c["stop"], c["seg"], c["cov"])
    S.same_tables(dict(got, counts=got["counts"].cpu().numpy()), want)
    assert (got["seg_start_ci"] == want["seg_ci4"][:, :2]).all() and (got["seg_end_ci"] == want["seg_ci4"][:, 2:]).all()
    return got


def test_one_bin(cv):
    c = dict(off=np.array([0, 1]), start=np.array([7], np.int32), stop=np.array([18], np.int32), seg=np.array([-4], np.int32), cov=np.array([12.34]))
    got = check(cv, c)
    assert got["nseg"] == 1 and got["seg_ci4"].tolist() == [[-6, 6, -6, 6]] and got["seg_bin_offset"].tolist() == [0, 1]
    c["off"] = np.array([0, 0, 1, 1])                         # the same bin between two empty chromosomes
    assert check(cv, c)["chr_seg_offset"].tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("ids", ("each", "one"))
def test_one_bin_per_segment_and_one_segment_per_chromosome(cv, ids):
    # empty chromosomes first, in the middle (two in a row) and last (two in a row); a chromosome of one bin; chromosomes that end inside a workgroup and on its edge
    per = [0, 300, 0, 0, 1, BLOCK - 301 + BLOCK, 211, 0, 0]
    got = check(cv, make(per, 3, ids=ids))
    assert got["nseg"] == (sum(per) if ids == "each" else 4)
    assert run(cv, make(per, 3, ids=ids), cov=False)["counts"] is None


def test_segment_starts_on_the_first_and_last_thread_of_a_workgroup(cv):
    c = make([3 * BLOCK], 5, ids="one")
    c["seg"][BLOCK:2 * BLOCK - 1] = 1                         # starts at BLOCK (first thread of the second workgroup) and at 2 * BLOCK - 1 (its last thread)
    got = check(cv, c)
    assert got["seg_bin_offset"].tolist() == [0, BLOCK, 2 * BLOCK - 1, 3 * BLOCK]
    c = make([BLOCK - 1, 1, BLOCK], 5, ids="one")              # chromosomes that start on a last and on a first thread
    assert check(cv, c)["seg_bin_offset"].tolist() == [0, BLOCK - 1, BLOCK, 2 * BLOCK]


@pytest.mark.parametrize("n", (2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1))
def test_bins_around_a_multiple_of_the_workgroup(cv, n):
    check(cv, make([n // 3, n - n // 3], 7 + n))
    c = make([n], 11 + n); c["seg"][-1] = c["seg"][-2] + 1       # the last bin is a segment of its own
    assert check(cv, c)["seg_bin_offset"][-2] == n - 1


def test_one_workgroup_count_more_than_the_scan_is_wide(cv):
    n = SCAN_WIDTH * BLOCK + 1                                 # 1025 workgroup counts: the scan's threads take two counts each, the last of them none
    c = make([100_000, 0, n - 100_000], 13, p_change=0.02)
    got = check(cv, c)
    assert got["nseg"] > 4000 and got["seg_bin_offset"][-1] == n


def test_more_segments_than_the_first_offer_and_than_cap_seg(cv):
    from canvas_amd import CanvasError
    c = make([700, 45], 17)
    want = S.from_arrays(c["off"], c["start"], c["stop"], c["seg"], c["cov"])
    cv.SEGMENT_TABLES_CAP = 4                                   # (an attribute of this instance: the class keeps its value)
    try:
        check(cv, c)                                           # refused once, repeated with the count the refusal reported
    finally:
        del cv.SEGMENT_TABLES_CAP
    check(cv, c, cap_seg=want["nseg"])
    with pytest.raises(CanvasError) as e:
        run(cv, c, cap_seg=want["nseg"] - 1)
    assert "error -1" in str(e.value) and "%d segments, room for %d" % (want["nseg"], want["nseg"] - 1) in str(e.value), str(e.value)
    with pytest.raises(CanvasError) as e:
        run(cv, c, cap_seg=0)
    assert "%d segments, room for 0" % want["nseg"] in str(e.value)
    check(cv, c)


def test_refusals_the_device_decides_name_their_bin(cv):
    from canvas_amd import CanvasError
    base = make([BLOCK + 40, 0, 300], 19)

    def refused(change, text):
        bad = {k: v.copy() for k, v in base.items()}
        change(bad)
        with pytest.raises(CanvasError) as e:
            run(cv, bad)
        assert "error -1" in str(e.value) and text in str(e.value), str(e.value)
        check(cv, base)                                        # the context is still usable

    first = BLOCK + 40                                         # first bin of the last chromosome: its start lies below its predecessor's, which is no refusal
    assert base["start"][first] < base["start"][first - 1]

    def backwards(i):
        def f(c):
            c["start"][i] = c["start"][i - 1] - 1; c["stop"][i] = max(c["stop"][i], c["start"][i])
        return f
    refused(backwards(BLOCK + 2), "starts must not decrease (bin %d)" % (BLOCK + 2))
    refused(lambda c: (backwards(first + 200)(c), backwards(9)(c)), "starts must not decrease (bin 9)")
    refused(lambda c: c["stop"].__setitem__(BLOCK - 1, c["start"][BLOCK - 1] - 1), "stop before it starts (bin %d)" % (BLOCK - 1))
    refused(lambda c: c["cov"].__setitem__(first + 5, np.nan), "non-finite value at bin %d" % (first + 5))
    refused(lambda c: (c["cov"].__setitem__(300, -np.inf), c["cov"].__setitem__(17, np.inf)), "non-finite value at bin 17")
    refused(lambda c: c.__setitem__("off", np.array([0, 5, 4, len(c["start"])])), "non-decreasing")
