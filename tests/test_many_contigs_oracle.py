"""The oracle's genome-level entry points on references with hundreds to thousands of contigs (tests/many_contigs.py) against the independent restatements of
test_oracle_independent.py: the bin size (median of the autosomes' rates) and CanvasClean's autosome-dependent steps.  The GPU tests of test_many_contigs_gpu.py
take the oracle as the truth at these chromosome counts; this checks that it holds there.  CPU only."""
import numpy as np
import pytest

import many_contigs as M
import oracle_lib as O
from test_oracle_independent import np_clean_whole_genome

ALL = O.CLEAN_GCNORM | O.CLEAN_FILTSIZE | O.CLEAN_OUTLIERS | O.CLEAN_LOCALSD


def np_bin_size(masks, hits, is_auto, counts_per_bin):
    """SampleHitArrays.GetRates + GetBinSize (CanvasBin.cs:30-83): observed / possible per autosome, median of the sorted rates"""
    rates = []
    for m, h, a in zip(masks, hits, is_auto):
        if not a:
            continue
        possible = np.unpackbits(m, bitorder="little")[:len(h)].astype(bool)
        rates.append(np.count_nonzero(h[possible] > 0) / float(np.count_nonzero(possible)))
    s = sorted(rates)
    n = len(s)
    median = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    return int(counts_per_bin / median)


@pytest.mark.parametrize("nchr", [65, 257, 1025, 3000])
def test_bin_size_many_contigs_two_restatements(nchr):
    data, is_auto = M.genome(nchr)
    masks = [d[2] for d in data]; hits = [d[1] for d in data]
    rates = O.bin_rates_genome(masks, hits, threads=4)
    for flags in (is_auto, M.flipped(is_auto)):
        assert O.bin_size(rates[flags == 1], 100) == np_bin_size(masks, hits, flags, 100)
    if nchr > 1024:
        assert np_bin_size(masks, hits, is_auto, 100) != np_bin_size(masks, hits, M.flipped(is_auto), 100)


@pytest.mark.parametrize("nchr", [257, 1025, 3000])
def test_clean_many_contigs_two_restatements(nchr):
    per = M.bin_counts_per_contig(nchr)
    per[:len(M.PRIMARY)] = [270_000, 240_000, 160_000]          # (the restatement's variance normalisation is written for whole genomes)
    b, is_auto = M.bins(nchr, per=per)
    b["count"] = np.round(b["count"]).astype(np.float32)
    results = []
    for flags in (is_auto, M.flipped(is_auto)):
        want = np_clean_whole_genome(b["chr"], b["start"], b["stop"], b["count"], b["gc"], flags)
        got = O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], flags, np.zeros(nchr, np.uint8), ALL)
        assert got["local_sd"] == want[3]
        assert len(got["chr"]) == len(want[0]) and (got["chr"] == want[0]).all() and (got["start"] == want[1]).all()
        assert (got["count"].view(np.uint32) == want[2].view(np.uint32)).all()
        results.append(got["count"])
    if nchr > 1024:
        assert len(results[0]) != len(results[1]) or not (results[0].view(np.uint32) == results[1].view(np.uint32)).all()
