"""Canvas.clean with CLEAN_GCNORM | CLEAN_LOESS (canvas_amd/csrc/loess.hpp, normalize_by_gc_loess in clean.hip) against the extended-precision restatement of
LoessGCNormalizer (tests/loess_ref.py) on the inputs of tests/loess_cases.py.  The rule, derived in test_loess_ref.py where the oracle is held to it on the CPU:
same zero mask, same NaN mask, every finite count within 1 float32 ulp of the reference rounded to float32, and no more bins off by that ulp than
loess_cases.cap_bins allows."""
import gzip
import os
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import loess_cases as LC
import loess_ref as R
import oracle_lib as O
from canvas_amd import CLEAN_GCNORM, CLEAN_LOESS, CanvasError
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
FLAGS = CLEAN_GCNORM | CLEAN_LOESS
KEYS = ("chr", "start", "stop", "gc", "count")
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canvas_amd", "bin")


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def _upload(cv, c):
    return {k: to_dev(c[k].copy(), cv.device) for k in KEYS}


def _clean(cv, c):
    dev = _upload(cv, c)
    n = len(c["count"])
    n_out, lsd, info = cv.clean(dev, n, c["is_auto"], FLAGS, is_y=c["is_y"])
    assert n_out == n
    out = {k: dev[k].cpu().numpy() for k in KEYS}
    for k in ("chr", "start", "stop", "gc"):
        assert (out[k] == c[k]).all(), k
    return out["count"], info


def check_against_reference(got, ref, what):
    """the rule; the message carries the ulp histogram (one fit moved, or all of them?) and the first tile that differs"""
    n = len(got)
    nan_same = np.isnan(got) == ref["nan"]
    zero_same = (got == 0) == (ref["f32"] == 0)
    fin = ~ref["nan"] & ~np.isnan(got)
    ulp = np.zeros(n, np.int64); ulp[fin] = R.ulp_distance(got[fin], ref["f32"][fin])
    hist = np.bincount(np.minimum(ulp[fin], 4), minlength=5).tolist()
    bad = np.flatnonzero(~nan_same | ~zero_same | (ulp > 0))
    first = None if len(bad) == 0 else "bin %d (tile %d of %d)" % (bad[0], bad[0] // LC.TILE, -(-n // LC.TILE))
    ndiff = int((ulp > 0).sum()); cap = LC.cap_bins(n)
    msg = f"{what}: n={n} ulp histogram [0,1,2,3,4+]={hist} not bit-equal={ndiff} (cap {cap}) NaN mask differs at {int((~nan_same).sum())} zero mask differs at {int((~zero_same).sum())} first difference: {first}"
    print(msg)
    assert nan_same.all(), msg
    assert zero_same.all(), msg
    assert (ulp <= 1).all(), msg
    assert ndiff <= cap, msg
    return ndiff


@pytest.mark.parametrize("name", [k for k in LC.OK_NAMES if k != "large"])
def test_loess_matches_reference(cv, name):
    c = LC.get(name)
    got, info = _clean(cv, c)
    assert info[6] == 0 and info[7] == 0            # the host-driven path
    check_against_reference(got, LC.reference(name), name)
    if name == "zeros4097":
        assert (got[c["count"] == 0] == 0).all()


def test_loess_large_takes_the_second_chunk_of_the_column_scan(cv):
    """2 097 153 bins = 1 025 tiles of 2 048: k_loess_col_scan runs its loop a second time, with the carry, and the last tile holds one element.  Compared with the
    grouped layer (the oracle was compared with it on the CPU, test_loess_ref.py)."""
    c = LC.get("large")
    got, info = _clean(cv, c)
    check_against_reference(got, LC.reference("large"), "large")


def test_loess_gc0_on_an_autosome_is_refused(cv):
    c = LC.get("gc0_autosome")
    dev = _upload(cv, c)
    with pytest.raises(CanvasError, match="GC = 0"):
        cv.clean(dev, len(c["count"]), c["is_auto"], FLAGS, is_y=c["is_y"])


@pytest.mark.parametrize("name", ["plain30k_s0", "heavy80", "zeros4097"])
def test_loess_is_repeatable(cv, name):
    c = LC.get(name)
    a, _ = _clean(cv, c); b, _ = _clean(cv, c)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_loess_batch_equals_single_calls(cv):
    """canvas_clean_batch hands LOESS samples to the host-driven path one by one: bit for bit what two clean calls give"""
    cs = [LC.get("m2049"), LC.get("zeros4097")]
    single = [_clean(cv, c)[0] for c in cs]
    devs = [_upload(cv, c) for c in cs]
    ns = [len(c["count"]) for c in cs]
    nout, lsd, info = cv.clean_batch(devs, ns, cs[0]["is_auto"], FLAGS, is_y=cs[0]["is_y"])
    assert list(nout) == ns
    for s in range(2):
        assert info[s][6] == 0 and info[s][7] == 0 and info[s][0] == ns[s]
        assert (devs[s]["count"].cpu().numpy().view(np.uint32) == single[s].view(np.uint32)).all()
        for k in ("chr", "start", "stop", "gc"):
            assert (devs[s][k].cpu().numpy() == cs[s][k]).all()


def _rows(c, count):
    return ["%s\t%d\t%d\t%s\t%d" % (LC.EXE_NAMES[ch], s, e, O.format_f2(float(v)), g) for ch, s, e, v, g in zip(c["chr"], c["start"], c["stop"], count, c["gc"])]


def test_canvas_clean_executable_loess(cv, tmp_path):
    """CanvasClean -g -m LOESS on a .binned file whose chrY runs are named chrY, Y and chry: rows identical to the oracle's, except that a count may differ by one unit of its
    last printed digit, in no more rows than the cap allows"""
    c = LC.get("exe_names")
    n = len(c["count"])
    binned = str(tmp_path / "S.binned"); cleaned = str(tmp_path / "S.cleaned")
    with gzip.open(binned, "wt") as f:
        f.write("\n".join(_rows(c, c["count"])) + "\n")
    r = subprocess.run([os.path.join(BIN, "CanvasClean"), "-i", binned, "-o", cleaned, "-g", "-m", "LOESS"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ex = O.clean(c["chr"], c["start"], c["stop"], c["count"], c["gc"], c["is_auto"], c["is_y"], O.CLEAN_GCNORM | O.CLEAN_LOESS)
    exp = _rows(c, ex["count"])
    with gzip.open(cleaned, "rt") as f:
        got = f.read().splitlines()
    assert len(got) == len(exp) == n
    off = 0
    for g, e in zip(got, exp):
        if g == e:
            continue
        gf, ef = g.split("\t"), e.split("\t")
        assert gf[:3] + gf[4:] == ef[:3] + ef[4:], (g, e)
        assert abs(Decimal(gf[3]) - Decimal(ef[3])) == Decimal("0.01"), (g, e)
        off += 1
    print(f"CanvasClean -m LOESS: {off} of {n} rows differ in the last printed digit (cap {LC.cap_bins(n)})")
    assert off <= LC.cap_bins(n)
