"""CPU companion of test_parameters_gpu.py: on the oracle alone, the inputs of tests/parameter_cases.py must reach the regimes the GPU tests are there for — every CBS
(nperm, alpha) pair but the degenerate one runs permutations and finds change points (and the pairs do not all give the same answer), the Wavelets breakpoint counts grow as the
threshold falls, the MinSize and gap cases sit exactly on their bounds, and the CanvasBin depths give the bin sizes the test names.  Runs without a GPU."""
import numpy as np
import pytest

import many_contigs as M
import oracle_lib as O
import parameter_cases as P


@pytest.fixture(scope="module")
def cbs_results():
    per = P.cbs_genome()
    return per, {p: O.cbs_genome(per, p[1], p[0], threads=8) for p in P.CBS_PAIRS}


def test_cbs_inputs_have_the_three_length_classes():
    n = sorted(P.CBS_LENGTHS)
    assert n[0] < 201 and 201 <= n[1] <= 2000 and n[-1] > 20_000
    assert (P.CBS_DEGENERATE in P.CBS_PAIRS) and P.CBS_PAIRS[-1] == (10000, 0.01)
    assert [int(np.floor(n_ * a)) for n_, a in P.CBS_PAIRS] == [500, 10, 2000, 200, 1, 0, 100]
    assert len(O.cbs_boundary(*P.CBS_DEGENERATE)) == 1 and len(O.cbs_boundary(10000, 0.05)) == 125_751 and len(O.cbs_boundary(10000, 0.001)) == 66


def test_every_cbs_pair_runs_permutations_and_finds_change_points(cbs_results):
    per, res = cbs_results
    for p in P.CBS_PAIRS:
        seg, st = res[p]
        assert [int(s.sum()) for s in seg] == [len(x) for x in per], p
        if p == P.CBS_DEGENERATE:
            continue
        assert sum(len(s) for s in seg) > len(per), (p, [len(s) for s in seg])       # change points beyond the chromosome starts
        assert st[2] > 0 and st[4] > 0, (p, st)                                          # permutations ran, edge tests drew
    # the pairs discriminate: a library that ignored alpha (or nperm) could not match all of them
    key = lambda p: [s.tolist() for s in res[p][0]]
    assert key((10000, 0.05)) != key((10000, 0.01)) and key((10000, 0.001)) != key((10000, 0.01)) and key((10000, 0.2)) != key((10000, 0.05))
    assert len({int(res[p][1][2]) for p in P.CBS_PAIRS}) == len(P.CBS_PAIRS)           # no two pairs consume the same number of permutations


def test_cbs_undo_settings_change_the_answer():
    per = P.cbs_undo_genome()
    for nperm, alpha in P.CBS_UNDO_PAIRS:
        base = O.cbs_genome(per, alpha, nperm, threads=8, undo=0)[0]
        n0 = sum(len(s) for s in base)
        got = {sd: sum(len(s) for s in O.cbs_genome(per, alpha, nperm, threads=8, undo=2, undo_sd=sd)[0]) for sd in P.CBS_UNDO_SDS}
        assert n0 >= got[1.0] > got[3.0] > got[6.0] > len(per), (nperm, alpha, n0, got)     # a larger undo_sd merges more
        prune = sum(len(s) for s in O.cbs_genome(per, alpha, nperm, threads=8, undo=1)[0])
        assert len(per) < prune <= n0, (nperm, alpha, prune, n0)


def test_wavelets_breakpoints_grow_as_the_threshold_falls():
    per = P.wv_genome()
    for germline in (False, True):
        counts = [sum(len(b) for b in O.wavelets_genome(per, is_germline=germline, window=P.WV_WINDOW, **s)) for s in P.WV_FALLING]
        assert all(a < b for a, b in zip(counts, counts[1:])), (germline, counts)
        assert counts[-1] > 0.9 * sum(n for n in P.WV_LENGTHS if n > 10), counts          # MadFactor 0: nearly every bin is a breakpoint (the lists fill up)
        assert counts[2] > 50 * counts[1]                                                     # MadFactor 0.5 is already far from the default regime
        up, zero, none = [[len(b) for b in O.wavelets_genome(per, is_germline=germline, window=P.WV_WINDOW, **s)] for s in P.WV_CLAMPS]
        assert counts[1] < sum(up) < counts[-1]                                               # the clamp at threshold_upper 1.0 lowers the threshold
        assert sum(zero) >= counts[-1]
        assert sum(none) < counts[0] and none[4] == 0                                         # clamped from below at 500: only the root splits are left


def test_wavelets_big_run_reaches_the_low_threshold_regime():
    big = P.wv_big()
    d = sum(len(b) for b in O.wavelets_genome(big, mad_factor=5.0))
    low = sum(len(b) for b in O.wavelets_genome(big, mad_factor=0.5))
    assert len(big[0]) == 1_200_000 and low > 100 * d and low > 10_000, (d, low)


def test_min_size_cases_sit_on_the_bound():
    """length > MinSize (WaveletsRunner.cs): MinSize 300 drops the 300-bin chromosome, 299 keeps it; 9 001 drops the 9 001-bin one; 4 segments the 10-bin one"""
    per = P.wv_genome()
    n = {m: [len(b) for b in O.wavelets_genome(per, window=P.WV_WINDOW, min_size=m)] for m in P.WV_MIN_SIZES + [10, 9_000]}
    assert P.WV_LENGTHS == [40_000, 9_001, 300, 11, 10]
    assert n[10][3] > 0 and n[10][4] == 0 and n[4][4] > 0
    assert n[299][2] > 0 and n[299][3] == 0 and n[300][2] == 0
    assert n[9_000][1] > 0 and n[9_001][1] == 0 and n[9_001][0] > 0


@pytest.mark.parametrize("D", P.GAP_DISTS)
def test_gap_cases_sit_on_the_bound(D):
    case = P.gap_case(D)
    off = case["off"]
    gaps = np.concatenate(case["gaps"])
    assert (case["start"][1:] - case["stop"][:-1])[np.diff(case["chr"]) == 0].tolist() == np.delete(gaps, off[:-1]).tolist()
    assert {int(g) for g in gaps} >= {D - 1, D, D + 1}
    ids, last = P.gap_expected(case, D, False, False)
    a = ids[0]
    assert a[5] == a[4] and a[6] == a[5] and a[7] == a[6] + 1                 # D - 1 and D stay, D + 1 splits
    assert a[12] == a[11] + 1 and a[13] == a[12]                             # a state change in a gap of D + 1 is one split, not two
    assert a[21] == a[19] + 2 and a[38] == a[37] and a[39] == a[38] + 1
    assert ids[3].tolist() == [ids[3][0] + k for k in (0, 1, 1, 1, 2)]       # no state: only the gaps split
    flat = lambda r: np.concatenate(r[0]).tolist()
    assert flat(P.gap_expected(case, D + 1, False, False)) != flat((ids, last)) != flat(P.gap_expected(case, D - 1, False, False))
    ex = P.gap_expected(case, D, True, False); pl = P.gap_expected(case, D, False, True); both = P.gap_expected(case, D, True, True)
    assert ex[0][1][15] == ex[0][1][14] + 1 and ids[1][15] == ids[1][14]     # the excluded interval splits in a gap of D, the gap alone does not
    assert ex[0][1][8] == ex[0][1][7] + 1                                    # both rules in one gap: one split
    assert pl[0][2][8] == pl[0][2][7] + 1 and ids[2][8] == ids[2][7] and pl[0][2][17] == pl[0][2][16] + 1
    assert len({tuple(flat(r)) for r in ((ids, last), ex, pl, both)}) == 4


def test_bin_depths_give_the_bin_sizes_the_test_is_for():
    data, is_auto = M.genome(P.BIN_NCHR)
    rates = O.bin_rates_genome([d[2] for d in data], [d[1] for d in data], threads=8)
    sizes = [O.bin_size(rates[is_auto == 1], d) for d in P.BIN_DEPTHS]
    assert sizes == sorted(sizes) and sizes[0] >= 1 and len(set(sizes)) == len(sizes), sizes
    shortest_primary = min(int(np.unpackbits(d[2], bitorder="little")[:len(d[0])].sum()) for d in data[:len(M.PRIMARY)])
    assert sizes[-1] > shortest_primary > sizes[-2], (sizes, shortest_primary)
