"""The device arc search of CBS on its own, through canvas_cbs_arc_probe: the pruned search k_arcp_blocks -> k_arcp_bounds -> k_arcp_eval -> k_arcp_mail (mode 0) and the exhaustive
k_arc_search (mode 1, and mode 0 when the pair list overflows), against the every-arc search in numpy (cbs_arc_ref.py, pinned on the CPU by test_cbs_arc_ref.py) and the oracle's
TMaxO.  Every comparison is exact: bit patterns for doubles, equality for integers.

canvas_cbs replays the search on the host whenever the device does not report one unique maximiser, so a kernel that miscounts ties or misses the maximum still yields the right
segments there.  Here h_path must be the path the reference predicts and the result words must be the reference's: hiding behind the replay fails.

Cases left out: none."""
import functools

import numpy as np
import pytest

import cbs_arc_ref as R
import oracle_lib as O
from canvas_amd import synth
from canvas_amd.lib import CanvasError
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _canvas():
    return get_canvas()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _segment(out, s):
    """the outputs of segment s of a probe call"""
    a, b = int(out["off"][s]), int(out["off"][s + 1])
    return dict(sx=out["sx"][a:b], tau=float(out["tau"][s]), stat=float(out["stat"][s]), iseg=(int(out["iseg"][s, 0]), int(out["iseg"][s, 1])), path=int(out["path"][s]),
                words=[int(w) for w in out["words"][s]], dmax=out["dmax"][a:b], first=out["first"][a:b])


@functools.lru_cache(maxsize=None)
def _alone(kind, n, al0, mode, cap=0):
    """one catalogue input probed on its own (run once, shared by the cases that compare with it)"""
    return _segment(_canvas().cbs_arc_probe([R.make(kind, n)], al0, mode, cap), 0)


def _same(a, b, what):
    assert (_u64(a["sx"]) == _u64(b["sx"])).all() and R.bits(a["tau"]) == R.bits(b["tau"]) and R.bits(a["stat"]) == R.bits(b["stat"]) and a["iseg"] == b["iseg"], what
    assert a["path"] == b["path"] and a["words"] == b["words"] and (_u64(a["dmax"]) == _u64(b["dmax"])).all() and (a["first"] == b["first"]).all(), what


def _check(g, kind, n, al0, mode, cap=0):
    """one segment's outputs g against the reference"""
    what = (kind, n, al0, mode, cap)
    x, sx, inc, dmax, first = R.reference(kind, n)
    (M, count, arc), bm, path = R.search(kind, n, al0)
    stat, iseg = R.oracle_tmaxo(kind, n, al0)
    overflow = mode == 0 and path != 0 and bm["npairs"] > (cap or R.PAIRCAP)
    print(f"{kind} n {n} al0 {al0} mode {mode} cap {cap}: path {g['path']} (expected {path}{' + 8' if overflow else ''}), words {g['words']}, model: pairs {bm['npairs']}, count {count}, arc {arc}")
    assert (_u64(g["sx"]) == _u64(sx)).all(), what
    assert R.bits(g["tau"]) == R.bits(inc[0]), (what, g["tau"], inc)
    assert R.bits(g["stat"]) == R.bits(stat) and g["iseg"] == iseg, (what, g["stat"], g["iseg"], stat, iseg)
    assert g["path"] == path + (8 if overflow else 0), (what, g["path"], path, overflow)
    if mode == 0 and path != 0:
        w = g["words"]
        assert w[3] == bm["npairs"] and w[5] == R.bits(bm["word5"]) and w[4] == (1 if overflow else 0), (what, w, bm["npairs"], R.bits(bm["word5"]))
        if not overflow:
            if count and M >= inc[0]:
                assert w[0] == R.bits(M) and w[1] == count and w[2] == (arc[0] << 32 | arc[1]), (what, w, R.bits(M), count, arc)
            else:
                assert w[3] == 0 or float(np.uint64(w[0]).view(np.float64)) < inc[0], (what, w, inc)
    else:
        assert g["words"] == [0] * 6, (what, g["words"])
    if (mode == 1 and path != 0) or overflow:
        assert (_u64(g["dmax"][1:]) == _u64(dmax[1:])).all() and (g["first"][1:] == first[1:]).all(), (what, np.nonzero(_u64(g["dmax"][1:]) != _u64(dmax[1:]))[0][:4] + 1, np.nonzero(g["first"][1:] != first[1:])[0][:4] + 1)
    else:
        assert not g["dmax"].any() and not g["first"].any(), what


_MODE0 = R.mode0_cases()


@pytest.mark.parametrize("kind,n,al0", _MODE0, ids=[f"{k}-{n}-al0_{a}" for k, n, a in _MODE0])
def test_pruned_search(kind, n, al0):
    _check(_alone(kind, n, al0, 0), kind, n, al0, 0)


_MODE1 = [(k, n) for n in R.MODE1_SIZES for k in ("f2", "int", "twin") if n >= R.min_size(k)]


@pytest.mark.parametrize("kind,n", _MODE1, ids=[f"{k}-{n}" for k, n in _MODE1])
def test_exhaustive_search(kind, n):
    g = _alone(kind, n, 2, 1)
    _check(g, kind, n, 2, 1)
    g0 = _alone(kind, n, 2, 0)
    assert R.bits(g["stat"]) == R.bits(g0["stat"]) and g["iseg"] == g0["iseg"] and g["path"] & 7 == g0["path"] & 7, (kind, n, g["stat"], g["iseg"], g["path"], g0["stat"], g0["iseg"], g0["path"])


MIXED = (("step", 4097), ("f2", 5), ("two", 20481), ("f2", 1024), ("zeros", 4096), ("twin", 8193), ("cauchy", 4161))
MANY_KINDS = ("f2", "int", "twin", "step", "neg", "zeros", "cauchy", "per4")
MANY = tuple((MANY_KINDS[k % len(MANY_KINDS)], 4096 + k) for k in range(65))


@pytest.mark.parametrize("mode", (0, 1))
def test_requests_of_different_lengths_share_a_launch(mode):
    """grid.y = request: workgroups past a request's own block count return early, every request keeps its own result words"""
    out = _canvas().cbs_arc_probe([R.make(k, n) for k, n in MIXED], 2, mode)
    for s, (kind, n) in enumerate(MIXED):
        g = _segment(out, s)
        _check(g, kind, n, 2, mode)
        _same(g, _alone(kind, n, 2, mode), (kind, n, mode))


@pytest.mark.parametrize("mode", (0, 1))
def test_sixty_five_requests_take_two_launches(mode):
    out = _canvas().cbs_arc_probe([R.make(k, n) for k, n in MANY], 2, mode)
    for s, (kind, n) in enumerate(MANY):
        _check(_segment(out, s), kind, n, 2, mode)


_OVERFLOW = [(k, n, c) for k, n in R.OVERFLOW_INPUTS for c in range(5)]


@pytest.mark.parametrize("kind,n,which", _OVERFLOW, ids=[f"{k}-{n}-{('cap_1', 'cap_4', 'pairs_minus_1', 'pairs', 'pairs_plus_1')[c]}" for k, n, c in _OVERFLOW])
def test_pair_list_overflow(kind, n, which):
    """a pair list shorter than the surviving pairs: the overflow word is set, the exhaustive kernel supplies the same answer"""
    npairs = R.search(kind, n, 2)[1]["npairs"]
    cap = R.overflow_caps(npairs)[which]
    g = _alone(kind, n, 2, 0, cap)
    _check(g, kind, n, 2, 0, cap)
    g0 = _alone(kind, n, 2, 0)
    assert g["words"][4] == (1 if npairs > cap else 0) and (g["path"] & 8 != 0) == (npairs > cap), (kind, n, cap, g["words"], g["path"])
    assert R.bits(g["stat"]) == R.bits(g0["stat"]) and g["iseg"] == g0["iseg"] and g["path"] & 7 == g0["path"] & 7 == 2, (kind, n, cap)
    if npairs <= cap: _same(g, g0, (kind, n, cap))


@pytest.mark.parametrize("n", R.LARGE_SIZES)
def test_large_segment(n):
    """without the every-arc search; at 1 048 577 bins nb = 1025, and nb * nb pairs go through the 64-bit index of k_arcp_bounds"""
    x = R.make("two", n, R.LARGE_STEP); sx = R.prefix(x); inc = R.incumbent(sx); bm = R.block_model(sx, 2, inc[0])
    stat, iseg = R.oracle_tmaxo("two", n, 2, R.LARGE_STEP)
    g = _segment(_canvas().cbs_arc_probe([x], 2, 0), 0)
    w = g["words"]
    print(f"two (step {R.LARGE_STEP}) n {n}: path {g['path']}, words {w}, model: pairs {bm['npairs']}, word 5 {R.bits(bm['word5'])}")
    assert (_u64(g["sx"]) == _u64(sx)).all() and R.bits(g["tau"]) == R.bits(inc[0]), n
    assert R.bits(g["stat"]) == R.bits(stat) and g["iseg"] == iseg, (n, g["stat"], g["iseg"], stat, iseg)
    assert w[3] == bm["npairs"] and w[5] == R.bits(bm["word5"]) and w[4] == 0, (n, w, bm["npairs"])
    assert g["path"] == 2 and w[1] == 1, (n, g["path"], w)
    assert R.bits(R.arc_value(sx, w[2] >> 32, w[2] & 0xFFFFFFFF)) == w[0], (n, w)


def test_the_context_afterwards():
    """a capped probe call leaves nothing behind: canvas_cbs on the same context returns the oracle's segments"""
    cv = _canvas()
    g = _alone("two", 5121, 2, 0, 1)
    assert g["path"] & 8
    bins = synth.generate_bins(20260927 + 31, 30_000, nchr=3)
    cov = np.round(bins["count"].astype(np.float64), 2)
    off = np.concatenate([[0], np.cumsum(np.bincount(bins["chr"], minlength=3))]).astype(np.int64)
    per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(3)]
    exp, est = O.cbs_genome(per, 0.01, 2000, threads=8)
    seg_len, nseg, stats = cv.cbs(to_dev(cov, cv.device), off, 0.01, 2000)
    got = seg_len.cpu().numpy()
    for c in range(3):
        assert nseg[c] == len(exp[c]) and (got[off[c]:off[c] + nseg[c]] == exp[c]).all(), c
    assert stats[0] == est[0] and stats[6] > 0


def _raw(cv, mode=0, nseg=1, off=(0, 8), x=None, al0=2, cap=0, null=None):
    """canvas_cbs_arc_probe with arguments the wrapper would not pass"""
    import ctypes as C
    off = np.asarray(off, np.int64); x = np.ascontiguousarray(np.arange(8, dtype=np.float64) - 3.5 if x is None else x)
    tot = max(8, len(x)); ns = max(1, nseg)
    arrs = dict(off=off, x=x, sx=np.zeros(tot), tau=np.zeros(ns), stat=np.zeros(ns), iseg=np.zeros(2 * ns, np.int32), path=np.zeros(ns, np.int32), words=np.zeros(6 * ns, np.uint64),
                dmax=np.zeros(tot), first=np.zeros(tot, np.int32))
    p = {k: (None if k == null else v.ctypes.data_as(C.c_void_p)) for k, v in arrs.items()}
    cv._check(cv.lib.canvas_cbs_arc_probe(cv.ctx, C.c_int32(mode), C.c_int32(nseg), p["off"], p["x"], C.c_int32(al0), C.c_int32(cap), p["sx"], p["tau"], p["stat"], p["iseg"], p["path"],
                                          p["words"], p["dmax"], p["first"]))


_REFUSALS = [(f"null_{k}", dict(null=k)) for k in ("off", "x", "sx", "tau", "stat", "iseg", "path", "words", "dmax", "first")] + [
    ("nseg_0", dict(nseg=0)), ("offsets_start_at_1", dict(off=(1, 8))), ("offsets_decrease", dict(nseg=2, off=(0, 8, 4))), ("segment_of_3", dict(nseg=2, off=(0, 5, 8))),
    ("al0_0", dict(al0=0)), ("mode_2", dict(mode=2)), ("mode_minus_1", dict(mode=-1)), ("pair_cap_minus_1", dict(cap=-1)), ("pair_cap_8193", dict(cap=R.PAIRCAP + 1)),
    ("nan", dict(x=np.array([0.0, 1.0, np.nan, 0.0, 0.0, 0.0, 0.0, -1.0]))), ("inf", dict(x=np.array([0.0, 1.0, np.inf, 0.0, 0.0, 0.0, 0.0, -1.0])))]


@pytest.mark.parametrize("name,kw", _REFUSALS, ids=[n for n, _ in _REFUSALS])
def test_bad_arguments_are_refused(name, kw):
    cv = _canvas()
    with pytest.raises(CanvasError, match="libcanvas_hip error -1:.*canvas_cbs_arc_probe"):          # CANVAS_ERR_INVALID
        _raw(cv, **kw)
    _raw(cv)
    _check(_segment(cv.cbs_arc_probe([R.make("f2", 65)], 2, 0), 0), "f2", 65, 2, 0)          # the context goes on working
