"""The two restatements of CanvasBin -m Fragment in tests/fragment_ref.py agree with each other — the sequential loop of FragmentBinner.cs with its dictionary, set and
forward pointer, and the decomposition into per-name state machines with the pointer found by binary search in the running maximum of Stop, which is what frag.hip
computes — and the sequential one gives the reference's own unit cases (CanvasBinTest/TestCanvasBin.cs:14-78)."""
import numpy as np
import pytest

import fragment_ref as F


def run_chunks(chunks, bins, q=3):
    counts = st = None
    for reads in chunks:
        counts, st = F.sequential(reads, 0, bins, q, counts, st)
    if st is None:
        counts, st = F.sequential([], 0, bins, q)
    return counts, st


@pytest.mark.parametrize("seed", range(60))
def test_sequential_equals_decomposed(seed):
    rng = np.random.RandomState(seed)
    nbins = [0, 1, 2, 7, 40, 150][seed % 6]
    bins = F.random_bins(rng, nbins)
    reads = F.random_reads(rng, int(rng.randint(1, 60)), max_group=40, other_ref_tail=seed % 3)
    cut = sorted(int(x) for x in rng.randint(0, len(reads) + 1, size=seed % 4))
    chunks = [reads[a:b] for a, b in zip([0] + cut, cut + [len(reads)])]
    counts, st = run_chunks(chunks, bins)
    c2, usable, left_binned, left_same = F.decomposed(chunks, 0, bins)
    assert st["unsorted"] == 0
    assert (counts == c2).all() and st["usable"] == usable and st["binned"] == left_binned and st["same_pos"] == left_same
    assert st["stopped"] == (1 if seed % 3 else 0)


def test_something_is_binned_in_the_random_cases():
    total = 0
    for seed in range(60):
        rng = np.random.RandomState(seed)
        bins = F.random_bins(rng, [0, 1, 2, 7, 40, 150][seed % 6])
        reads = F.random_reads(rng, int(rng.randint(1, 60)), max_group=40)
        total += int(np.abs(F.sequential(reads, 0, bins)[0]).sum())
    assert total > 200


UNIT_CASES = [((10, 10), 1), ((10, 2), 0), ((2, 10), 0), ((2, 2), 0)]


def unit_pair(positions, mapqs):
    """alignment1 / alignment2 of TestBinOneAlignment: flags 0x1 | 0x2, fragment lengths 100 and -100 at either pair of positions"""
    p1, p2 = positions
    return [F.rd(p1, "ReadName", 0x3, mapqs[0], p2, 100), F.rd(p2, "ReadName", 0x3, mapqs[1], p1, -100)]


@pytest.mark.parametrize("positions", [(100, 120), (100, 100)])
@pytest.mark.parametrize("mapqs, expected", UNIT_CASES)
def test_reference_unit_cases(positions, mapqs, expected):
    """TestCanvasBin.cs:14-78: one bin, one pair; only a pair whose reads both reach the quality threshold stays counted"""
    bins = [(100, 200)]
    reads = unit_pair(positions, mapqs)
    counts, st = F.sequential(reads, 0, bins, 3)
    assert counts[0] == expected and st["usable"] == expected
    c2, usable, _, _ = F.decomposed([reads], 0, bins, 3)
    assert c2[0] == expected and usable == expected


@pytest.mark.parametrize("positions", [(100, 120), (100, 100)])
def test_reference_unit_cases_as_one_sequence(positions):
    """the same four steps the way the reference's test runs them: dictionary, set and pointer live on from step to step, the bin count is reset"""
    bins, st = [(100, 200)], None
    for mapqs, expected in UNIT_CASES:
        if st is not None:
            st["prev"] = -1                      # (BinOneAlignment is called directly: no sortedness check between the steps)
        counts, st = F.sequential(unit_pair(positions, mapqs), 0, bins, 3, None, st)
        assert counts[0] == expected, (positions, mapqs)


def test_every_two_chunk_split_gives_the_unsplit_result():
    rng = np.random.RandomState(11)
    bins = F.random_bins(rng, 30)
    reads = F.random_reads(rng, 30, max_group=6)[:40]
    assert len(reads) == 40
    whole, wst = run_chunks([reads], bins)
    assert np.abs(whole).sum() > 0
    for cut in range(41):
        counts, st = run_chunks([reads[:cut], reads[cut:]], bins)
        assert (counts == whole).all() and F.state_words(st) == F.state_words(wst) and st["binned"] == wst["binned"] and st["same_pos"] == wst["same_pos"]


def test_fragment_stop_past_2_31_wraps():
    """pos + tlen wraps to a negative stop, and min(Stop, stop) - max(Start, start) wraps back: unchecked C# counts an overlap of 1000"""
    bins = [(2 ** 31 - 500, 2 ** 31 - 1)]
    reads = F.pair("w", 2 ** 31 - 300, 2 ** 31 - 200, tlen=1000)
    counts, st = F.sequential(reads, 0, bins)
    assert F.wrap32(2 ** 31 - 300 + 1000) < 0 and counts[0] == 1 and st["usable"] == 1
    assert (F.decomposed([reads], 0, bins)[0] == counts).all()
