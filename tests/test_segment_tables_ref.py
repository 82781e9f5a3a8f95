"""The Python restatement of Segments.ReadSegments (tests/segment_tables_ref.py) against the reference's own TestReadSegments (a fixture under tests/golden) and hand-computed
cases, and the claim canvas_segment_tables' float counts rest on: for a coverage k/100, rounding the double to float gives what float.Parse gives for the text."""
import fractions
import json
import os

import numpy as np

import segment_tables_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_s_own_read_segments_case():
    case = json.load(open(os.path.join(ROOT, "tests", "golden", "read_segments_case.json")))
    names, t = S.from_text(case["partitioned"])
    assert names == ["chr22"] and t["nseg"] == 3 and t["chr_seg_offset"].tolist() == [0, 3]
    for s, want in enumerate(case["expected_confidence_intervals"]):
        assert t["seg_ci4"][s].tolist() == want["start"] + want["end"], s
    assert [t["seg_ci4"][s].tolist() for s in range(3)] == [[-5, 5, -5, 10], [-5, 10, -10, 5], [-10, 5, -5, 5]]      # the figures of TestSegments.cs:188-204, spelled out
    assert t["seg_begin"].tolist() == [1, 10, 30] and t["seg_end"].tolist() == [10, 30, 40] and t["seg_bin_offset"].tolist() == [0, 1, 2, 3]
    assert t["counts"].tolist() == [14.0, 31.0, 6.0]


# chromosome, start, stop, count text, id
HAND = [("chrA", 0, 100, "10.5", 0), ("chrA", 100, 200, "11", 0), ("chrA", 250, 351, "12.25", 1), ("chrA", 351, 400, "0", 1),          # a gap between two segments; lengths 101 and 49
        ("chrB", 0, 10, "7", 5), ("chrC", 10, 20, "8", 5),                                                                       # the same id across a chromosome change
        ("chrD", 0, 10, "1", 0), ("chrD", 10, 21, "2", 1), ("chrD", 21, 30, "3", 0), ("chrD", 30, 31, "4", -3), ("chrD", 31, 31, "5", -3)]     # an id that returns; lengths 11, 9, 1, 0
HAND_WANT = dict(nseg=8, chr_seg_offset=[0, 2, 3, 4, 8], seg_begin=[0, 250, 0, 10, 0, 10, 21, 30], seg_end=[200, 400, 10, 20, 10, 21, 30, 31], seg_bin_offset=[0, 2, 4, 5, 6, 7, 8, 9, 11],
                 seg_ci4=[[-50, 50, -50, 50],          # first of its chromosome; 200 != 250
                          [-51, 51, -25, 25],          # no abutting neighbour: its own halves, 50.5 -> 51 and 24.5 -> 25 (away from zero)
                          [-5, 5, -5, 5], [-5, 5, -5, 5],      # chrB ends at 10 and chrC starts at 10: another chromosome, not a neighbour
                          [-5, 5, -5, 6], [-5, 6, -6, 5], [-6, 5, -5, 1], [-5, 1, 0, 0]])      # 5.5 -> 6, 4.5 -> 5, 0.5 -> 1; the last bin has length 0


def test_hand_computed_cases_from_text_and_from_arrays():
    text = "".join("%s\t%d\t%d\t%s\t%d\n" % r for r in HAND)
    names, t = S.from_text(text)
    assert names == ["chrA", "chrB", "chrC", "chrD"]
    want = {k: (v if k == "nseg" else np.array(v)) for k, v in HAND_WANT.items()}
    want["counts"] = np.array([float(r[3]) for r in HAND], np.float32)
    S.same_tables(t, want)
    # the arrays entry, with empty chromosomes first, in the middle and last: they only repeat an offset
    a = S.from_arrays([0, 0, 4, 5, 5, 6, 11, 11], [r[1] for r in HAND], [r[2] for r in HAND], [r[4] for r in HAND], [float(r[3]) for r in HAND])
    want["chr_seg_offset"] = np.array([0, 0, 2, 3, 3, 4, 8, 8])
    S.same_tables(a, want)
    assert [S.half_length(0, n) for n in (0, 1, 2, 3, 9, 11, 49, 101)] == [0, 1, 1, 2, 5, 6, 25, 51]


def test_parse_float32_rounds_the_decimal_once():
    """16777217 = 2^24 + 1 is a float midpoint: the text just above it goes up, the tie goes to even, and a double-rounded parse of the first would not"""
    assert S.parse_float32("16777217") == np.float32(16777216.0)
    assert S.parse_float32("16777217.0000000001") == np.float32(16777218.0)
    assert np.float32(float("16777217.0000000001")) == np.float32(16777216.0)             # the double rounding this parser avoids
    assert S.parse_float32("16777219") == np.float32(16777220.0)
    assert S.parse_float32("0") == 0.0 and S.parse_float32("0.1").view(np.uint32) == np.float32(0.1).view(np.uint32)


def _directed_k():
    ks = {0, 1, 25, 50, 75, 100, 12800, 12825, 3276800, 3276850, 838860800, 838860875}      # 0, exact dyadic values (multiples of 1/4) up to 2^23
    for p in (7, 15, 23):
        f = np.float32(2.0 ** p)
        for _ in range(6):
            f = np.nextafter(f, np.float32(0))
        for _ in range(12):                                  # the floats on both sides of the power of two (the spacing halves below it)
            g = np.nextafter(f, np.float32(np.inf))
            m = (float(f) + float(g)) / 2                    # a float midpoint, exact in double
            k0 = int(np.floor(m * 100))
            ks.update(k0 + d for d in (-1, 0, 1, 2))
            f = g
    from canvas_amd import synth
    ks.add(int(round(float(synth.generate_bins(20260927, 20000)["count"].max()) * 100)))      # the largest count of the synthetic bins
    return sorted(ks)


def test_float_of_the_double_is_float_parse_of_the_text():
    ks = _directed_k()
    assert len(ks) > 60 and ks[0] == 0                   # (around 2^7 neighbouring midpoints share their k: the floats are 7.6e-6 apart there)
    for k in ks:
        x = k / 100.0                                        # what canvas_quantize_f2 leaves
        text = S.format_g15(x)
        assert fractions.Fraction(text) == fractions.Fraction(k, 100), (k, text)         # the double and the text denote the same decimal
        got, want = np.float32(x), S.parse_float32(text)
        assert got.view(np.uint32) == want.view(np.uint32), (k, text, got, want)
        # the argument: the decimal is a float midpoint exactly (then the double is exact too) or lies at least x * 2^-24 / 100 from one — far more than the double's 2^-53 x
        lo = np.nextafter(want, np.float32(-np.inf)); hi = np.nextafter(want, np.float32(np.inf))
        d = min(abs(fractions.Fraction(k, 100) - (fractions.Fraction(float(want)) + fractions.Fraction(float(n))) / 2) for n in (lo, hi))
        if d == 0:
            assert fractions.Fraction(x) == fractions.Fraction(k, 100)
        else:
            assert d >= fractions.Fraction(k, 100) / (100 * 2 ** 24), (k, float(d))
