"""Pins tests/select_ref.py, the reference and the inputs of tests/test_select_gpu.py, on the CPU: the key image against an independent total order, its inverse,
kth against np.partition, and for every input that is named after a path of the kernel that the keys really lead there."""
import functools
import math
import struct

import numpy as np
import pytest

import select_ref as R

WIDTHS = (4, 8)
_FMT = {4: ("<I", "<f"), 8: ("<Q", "<d")}


def _bits(x):
    """the bit pattern of a numpy float scalar, through its bytes"""
    return struct.unpack(_FMT[x.itemsize][0], x.tobytes())[0]


def _compare(a, b):
    """total order on floats of one width from sign and magnitude alone: a negative before a non-negative, two negatives by falling magnitude, two non-negatives by rising"""
    w = 8 * a.itemsize
    ba, bb = _bits(a), _bits(b)
    sa, sb = ba >> (w - 1), bb >> (w - 1)
    ma, mb = ba & ((1 << (w - 1)) - 1), bb & ((1 << (w - 1)) - 1)
    if sa != sb:
        return -1 if sa else 1
    if ma == mb:
        return 0
    return (-1 if ma > mb else 1) if sa else (-1 if ma < mb else 1)


def _class(x):
    """0 -NaN, 1 -inf, 2 negative, 3 -0, 4 +0, 5 positive, 6 +inf, 7 +NaN"""
    neg = _bits(x) >> (8 * x.itemsize - 1)
    v = float(x)
    if math.isnan(v):
        return 0 if neg else 7
    if math.isinf(v):
        return 1 if neg else 6
    if v == 0.0:
        return 3 if neg else 4
    return 2 if neg else 5


@pytest.mark.parametrize("width", WIDTHS)
def test_key_order_is_the_total_order_on_sign_and_magnitude(width):
    v, _ = R.special_values(width, 640)
    by_key = [v[i] for i in np.argsort(R.key_of(v), kind="stable")]
    by_cmp = sorted(v, key=functools.cmp_to_key(_compare))
    assert [_bits(x) for x in by_key] == [_bits(x) for x in by_cmp]
    classes = [_class(x) for x in by_key]
    assert classes == sorted(classes) and set(classes) == set(range(8))
    nans = [_bits(x) for x in by_key if _class(x) == 7]
    assert nans == sorted(nans) and len(set(nans)) >= 4          # payloads ordered by their bits
    nneg = [_bits(x) for x in by_key if _class(x) == 0]
    assert nneg == sorted(nneg, reverse=True) and len(set(nneg)) >= 4


@pytest.mark.parametrize("width", WIDTHS)
def test_inverse_of_the_key_is_bit_identical(width):
    v, _ = R.special_values(width, 640)
    U = R._UINT[width]
    assert (R.value_of(R.key_of(v)).view(U) == v.view(U)).all()
    k = np.random.default_rng(5).integers(0, 1 << (8 * width), 1000, dtype=U)
    assert (R.key_of(R.value_of(k)) == k).all()


@pytest.mark.parametrize("width", WIDTHS)
def test_special_value_boundaries_separate_the_classes(width):
    for n in R.CONTENT_SIZES:
        v, bounds = R.special_values(width, n)
        s = R.value_of(np.sort(R.key_of(v)))
        assert len(bounds) == 9
        denormal = lambda x: x != 0 and abs(float(x)) < float(np.finfo(v.dtype).tiny)
        for b in bounds:
            lo, hi = s[b - 1], s[b]
            assert (_class(lo), denormal(lo)) != (_class(hi), denormal(hi)), (b, lo, hi)


@pytest.mark.parametrize("width", WIDTHS)
def test_kth_equals_partition_on_plain_values(width):
    for case in [R.size_case(n, width) for n in (1, 65, 4097, 17 * 4096 + 1)] + [R.content_case(k, 4097, width) for k in ("whole_near_100", "two_decimal_near_37", "descending")]:
        assert not np.isnan(case.data).any() and not (case.data == 0).any()
        keys = R.keys_of(case.data)
        got = R.value_of(R.expected(case).astype(keys.dtype))
        for (lo, hi, k), g in zip(case.queries, got):
            assert g == np.partition(case.data, k)[k]
            assert R.kth(keys, case.seg_off, lo, hi, k) == int(R.key_of(np.array([g]))[0])


def test_sizes_and_ranks_are_those_of_the_plan():
    assert R.SIZES == (1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 69633)
    for n in R.SIZES:
        ranks = R.standard_ranks(n, 1)
        if n <= 257:
            assert ranks == list(range(n))
        else:
            assert len(ranks) == 16 and ranks[:6] == [0, 1, n // 2 - 1, n // 2, n - 2, n - 1] and all(0 <= k < n for k in ranks)
    assert len(R.size_case(69633, 4).data) > R.REP * R.TILE             # more tiles than replicas


@pytest.mark.parametrize("width", WIDTHS)
def test_content_cases_hold_what_their_names_say(width):
    bits = 8 * width
    for n in R.CONTENT_SIZES:
        c = {k: R.content_case(k, n, width) for k in R.CONTENT_KINDS}
        assert all(len(x.data) == n and all(0 <= q[2] < n for q in x.queries) for x in c.values())
        assert c["random_bits"].data.dtype.kind == "u" and len(np.unique(c["random_bits"].data >> (bits - 8))) == 256
        assert (c["whole_near_100"].data == np.round(c["whole_near_100"].data)).all() and 95 < c["whole_near_100"].data.mean() < 105
        assert len(np.unique(c["all_equal"].data)) == 1
        tv = c["two_values"]
        assert len(np.unique(tv.data)) == 2
        e = R.expected(tv)
        assert len(set(e.tolist())) == 2 and e[2] != e[3]                # ranks na - 1 and na straddle the boundary
        top, bot = c["top_byte_only"].data, c["bottom_byte_only"].data
        assert len(np.unique(top & ((1 << (bits - 8)) - 1))) == 1 and len(np.unique(top >> (bits - 8))) > 200
        assert len(np.unique(bot >> 8)) == 1 and len(np.unique(bot & 255)) > 200
        assert (np.diff(c["ascending"].data) >= 0).all() and (np.diff(c["descending"].data) <= 0).all() and (c["ascending"].data < 0).any()
        sp = c["special"]
        assert np.isnan(sp.data).any() and np.isinf(sp.data).any() and len(sp.queries) == 20


def _profiles(case, p, tile=0):
    """the wave profile of pass p over tile `tile` of a one-segment case, for the prefixes its queries have reached by then"""
    keys = R.keys_of(case.data)
    bits = 8 * keys.itemsize
    prefixes = [R.prefix_of(a, bits, p) for a in R.expected(case)]
    return R.wave_profile(keys, tile * R.TILE, min(len(keys), (tile + 1) * R.TILE), prefixes, p)


@pytest.mark.parametrize("width", WIDTHS)
def test_aggregation_cases_reach_the_path_they_are_named_after(width):
    last = width - 1
    c = R.aggregation_case("const_then_random", width)
    prof = _profiles(c, 0)
    assert len(prof) == 64 and all(d == 1 and left == 0 for _, d, left, _ in prof[:32]) and all(d > 28 for _, d, _, _ in prof[32:])
    assert R.switch_rounds(prof) == [8, 8, 8, 8]                           # in the middle of the tile: rounds 9..15 of every wave count with plain atomics

    c = R.aggregation_case("random_then_const", width)
    prof = _profiles(c, 0)
    assert R.switch_rounds(prof) == [0, 0, 0, 0] and all(d == 1 for _, d, _, _ in prof[32:])

    for d in R.AGG_DISTINCT:
        for where, p in (("top", 0), ("bottom", last)):
            c = R.aggregation_case(f"distinct_{d}_{where}", width)
            prof = _profiles(c, p)
            assert len(prof) == 64 and all(m == 64 and dd == d and left == d - 4 for m, dd, left, _ in prof), (d, where)
            # at most 4: fully aggregated; 5..28: lanes are left over, the switch stays on; more than 28: the switch goes off (in the first round here)
            assert R.switch_rounds(prof) == ([None] * 4 if d <= 28 else [0] * 4)
            assert all(left > 0 for _, _, left, _ in prof)
            for q in range(width):                                       # every other pass sees one digit per row (the queries part in pass p: several rows after it)
                if q != p:
                    assert all(dd == rows and left == 0 for m, dd, left, rows in _profiles(c, q) if m), (d, where, q)

    c = R.aggregation_case("partial_random", width)
    assert len(c.data) == R.TILE + 37
    prof = _profiles(c, 0, tile=1)
    assert [m for m, _, _, _ in prof] == [37]                              # one group, 37 lanes in range
    c = R.aggregation_case("partial_5", width)
    prof = _profiles(c, 0)
    assert [(m, d, left) for m, d, left, _ in prof] == [(64, 5, 1), (64, 5, 1), (37, 5, 1)]

    for name, off in (("two_rows_on", False), ("two_rows_off", True)):
        c = R.aggregation_case(name, width)
        assert all(rows == 1 for _, _, _, rows in _profiles(c, 0))
        for p in range(1, last):
            assert all(rows == 2 and d == 2 for _, d, _, rows in _profiles(c, p))      # the queries have parted: two rows, one digit each
        prof = _profiles(c, last)
        assert all(m == 64 and rows == 2 for m, _, _, rows in prof)
        if off:
            assert all(d == 32 and left == 28 for _, d, left, _ in prof) and R.switch_rounds(prof) == [0] * 4
        else:
            assert all(d == 8 and left == 4 for _, d, left, _ in prof) and R.switch_rounds(prof) == [None] * 4


@pytest.mark.parametrize("width", WIDTHS)
def test_query_cases_part_where_their_names_say(width):
    bits = 8 * width
    c = R.query_case("sixteen_distinct", width)
    assert len({q[2] for q in c.queries}) == 16
    c = R.query_case("sixteen_identical", width)
    assert len(c.queries) == 16 and len(set(c.queries)) == 1
    a, b = (int(x) for x in R.expected(R.query_case("pair_last_pass", width)))
    assert b == a + 1 and a >> 8 == b >> 8
    a, b = (int(x) for x in R.expected(R.query_case("pair_first_pass", width)))
    assert a >> (bits - 8) == 0x10 and b >> (bits - 8) == 0x90
    assert len(R.too_many_queries_case(width).queries) == 17


def _queries_per_segment(case):
    per = np.zeros(len(case.seg_off) - 1, int)
    for lo, hi, _ in case.queries:
        per[lo:hi + 1] += 1
    return per


@pytest.mark.parametrize("width", WIDTHS)
def test_segment_cases(width):
    c = R.segments_case(width)
    lens = np.diff(c.seg_off)
    assert len(lens) == 101 and set(lens.tolist()) == set(R.SEG_LENGTHS) and c.seg_off[-1] <= 1 << 20
    assert lens[0] == lens[50] == lens[100] == 0 and lens[49] > 0 and lens[52] > 0
    assert (0, 100, int(c.seg_off[-1]) // 2) in c.queries and any(q[:2] == (40, 60) for q in c.queries)
    assert _queries_per_segment(c).max() <= R.MAXQ
    for lo, hi, k in c.queries:
        assert 0 <= k < c.seg_off[hi + 1] - c.seg_off[lo]
    crowded = R.segments_case(width, crowded=True)
    per = _queries_per_segment(crowded)
    assert per.max() == R.MAXQ and per[45] == R.MAXQ
    assert _queries_per_segment(R.segments_case(width, crowded=True, one_more=True))[45] == R.MAXQ + 1


def test_sequence_and_workgroup_cases():
    seq = R.sequence_cases(8)
    assert [len(c.queries) for c in seq] == [1, 16, 3, 40, 2] and all(_queries_per_segment(c).max() <= R.MAXQ for c in seq)
    for kind in R.WG_KINDS:
        c = R.wg_case(kind)
        assert tuple(np.diff(c.seg_off)) == R.WG_COUNTS and c.data.itemsize == 8
        for s, _, (r0, r1) in c.queries:
            n = R.WG_COUNTS[s]
            assert 0 <= r0 < n and 0 <= r1 < n
        pairs = {(s, p) for s, _, p in c.queries}
        assert (9, (0, 4999)) in pairs and (9, (2500, 2500)) in pairs and (9, (2499, 2500)) in pairs and (0, (0, 0)) in pairs
        e = R.expected_pairs(c)
        assert e.shape == (len(c.queries), 2)
    e = R.expected_pairs(R.wg_case("special"))
    assert any((int(a) >> 56) != (int(b) >> 56) for a, b in e)           # a pair that parts in the first pass
    e = R.expected_pairs(R.wg_case("neighbours"))
    assert any(int(a) != int(b) and (int(a) >> 8) == (int(b) >> 8) for a, b in e)      # and one that parts only in the last
