"""CanvasClean -m LOESS on the CPU, before anything runs on a GPU: the two layers of the extended-precision restatement (tests/loess_ref.py) against each other, and
the oracle (oracle_bin_clean.cpp, the reference's loops in double) against that restatement, on the inputs of tests/loess_cases.py.

The rule for the oracle (and, in test_clean_loess_gpu.py, for the product) is derived from the arithmetic, not measured: two double evaluations of these sums differ
by about n * 2^-53 relative at worst (2e-10 at 2.1 M bins), far below half a float32 ulp (3e-8), so after rounding to float32 they can disagree only where the value
sits on a rounding boundary, and then by 1 ulp.  The premise is asserted here: the oracle's double result, before its cast to float, is within 2^-26 relative of the
longdouble one."""
import math

import numpy as np
import pytest

import loess_cases as LC
import loess_ref as R
import oracle_lib as O

FLAGS = O.CLEAN_GCNORM | O.CLEAN_LOESS          # nothing else: no later stage mixes in


def _same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", [k for k in LC.SMALL if k != "gc0_autosome"])
def test_loess_two_restatements(name):
    """grouped == literal: same NaN mask, same golden-section decisions, float32 results bit-equal"""
    g = LC.reference(name); l = LC.reference(name, "literal")
    assert (g["nan"] == l["nan"]).all()
    assert len(g["probes"]) == len(l["probes"])
    for pg, pl in zip(g["probes"], l["probes"]):
        assert pg[:2] == pl[:2] and bool(pg[2] < pg[3]) == bool(pl[2] < pl[3]), (pg, pl)
    assert g["bandwidth"] == l["bandwidth"]
    assert _same_bits(g["f32"], l["f32"]).all(), int((~_same_bits(g["f32"], l["f32"])).sum())


def test_loess_restatements_refuse_gc0_on_an_autosome():
    c = LC.get("gc0_autosome")
    for layer in ("literal", "grouped"):
        with pytest.raises(R.LoessIndexError):
            R.normalize(c["count"], c["gc"], c["chr"], c["is_y"], layer=layer)


@pytest.mark.parametrize("name", LC.OK_NAMES)
def test_cases_are_decidable(name):
    """No committed case leaves a decision to rounding.  At every comparison the golden section makes, one side is NaN (`fc < fd` is then false for every reader), or the
    two objectives differ by more than 1e-9 relative, or they are EQUAL bit for bit.  The last happens at every case once the search has narrowed to bandwidths whose
    ceil(bandwidth * n) windows differ only by points at the window's edge: those have tricube weight exactly 0 and add exact zeros to every sum, in the reference's
    loop and in any reader that sums left to right or run by run, so the tie is exact there too and `fc < fd` is false.  (The search stops at |d - c| <= 1e-5, less
    than one point below 100 000 bins, so no case can avoid such ties.)  And no bin reads a fit whose value is rounding noise (loess_ref.Diag)."""
    r = LC.reference(name)
    for c, d, fc, fd in r["probes"]:
        if np.isnan(fc) or np.isnan(fd) or fc == fd:
            continue
        assert abs(fc - fd) > 1e-9 * max(abs(fc), abs(fd)), (c, d, fc, fd)
    assert r["degenerate"] == 0, (r["degenerate"], r["fits"])


def test_case_shapes():
    """the cases are what they claim: tile counts, parities, signs, NaN regimes"""
    tiles = lambda k: -(-k // LC.TILE)
    z = LC.get("zeros4097"); m = int((z["count"] > 0).sum())
    assert len(z["count"]) == 4097 and 4097 - m == 60 and tiles(m) == tiles(4097) - 1
    assert LC.LARGE_N == 2_097_153 and tiles(LC.LARGE_N) == 1025 and LC.LARGE_N % LC.TILE == 1
    for name, par in (("neg_even", 0), ("neg_odd", 1)):
        c = LC.get(name)
        assert (c["count"] > 0).all() and len(c["count"]) % 2 == par and (c["count"] < 1).mean() > 0.95
    g = LC.get("gaps")["gc"]
    assert not np.isin(g, [40, 41, 42, 43, 44, 45, 46, 47]).any() and not (g % 5 == 0).any() and g.min() < 40 and g.max() > 47
    l = LC.get("lone95")["gc"]; assert (l == 95).sum() == 1 and np.sort(l)[-2] <= 60
    assert len(np.unique(LC.get("two_gc")["gc"])) == 2 and len(np.unique(LC.get("one_gc")["gc"])) == 1
    assert LC.reference("one_gc")["nan"].all()
    h = LC.reference("heavy80")["nan"]; assert 0 < h.sum() < len(h)
    for name, lo in (("y_10_90", 10), ("y_0_90", 0)):
        c = LC.get(name); y = c["is_y"][c["chr"]] == 1
        assert set(np.unique(c["gc"][y])) == {lo, 90} and c["gc"][~y].min() > lo and c["gc"][~y].max() < 90
    c = LC.get("gc0_autosome"); assert c["gc"][0] == 0 and c["is_y"][c["chr"][0]] == 0 and c["error"]
    assert LC.get("no_is_y")["is_y"] is None


@pytest.mark.parametrize("name", LC.OK_NAMES)
def test_oracle_matches_reference(name):
    """O.clean with CLEAN_GCNORM | CLEAN_LOESS: zero mask and NaN mask identical to the reference's, every finite count within 1 float32 ulp of the reference rounded
    to float32, and (the premise of that rule) the oracle's double within 2^-26 relative of the longdouble before rounding.  The share of bins not bit-equal is what
    loess_cases.ORACLE_SHARES records: it may not exceed the committed figure."""
    c = LC.get(name); r = LC.reference(name)
    n = len(c["count"])
    is_y = c["is_y"] if c["is_y"] is not None else np.zeros(c["nchr"], np.uint8)
    ex = O.clean(c["chr"], c["start"], c["stop"], c["count"], c["gc"], c["is_auto"], is_y, FLAGS)
    dbl = O.last_loess_double()
    assert len(ex["count"]) == n and len(dbl) == n
    got = ex["count"]
    assert (np.isnan(got) == r["nan"]).all()
    assert ((got == 0) == (r["f32"] == 0)).all()
    if name == "zeros4097":
        assert (got[c["count"] == 0] == 0).all()
    fin = ~r["nan"]
    ulp = R.ulp_distance(got[fin], r["f32"][fin])
    hist = np.bincount(np.minimum(ulp, 3), minlength=4)
    nz = fin & (r["ld"] != 0)
    rel = np.abs((dbl[nz].astype(R.LD) - r["ld"][nz]) / r["ld"][nz])
    worst_rel = float(rel.max()) if nz.any() else 0.0
    share = float((ulp != 0).sum()) / n
    print(f"{name}: n={n} ulp histogram [0,1,2,3+]={hist.tolist()} share={share:.3e} worst relative error of the double result={worst_rel:.3e}")
    assert worst_rel < 2.0 ** -26, worst_rel
    assert (ulp <= 1).all(), hist.tolist()
    assert share <= LC.ORACLE_SHARES.get(name, 0.0) + 1e-12, (share, "loess_cases.ORACLE_SHARES is out of date")
