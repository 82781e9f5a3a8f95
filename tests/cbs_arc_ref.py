"""Plain numpy float64 restatement of what the CBS arc-search kernels compute (k_arcp_blocks, k_arcp_bounds, k_arcp_eval, k_arc_search), written from the definitions, and the
seeded input catalogue of tests/test_cbs_arc_ref.py (CPU) and tests/test_cbs_arc_kernels_gpu.py.

The statistic of the arc between the 0-based prefix-sum indices i < j = i + L of a segment of n bins is c(L) * (d * d), c(L) = n / (L * (n - L)) (an exact integer product and one
IEEE division), d = |sx[j] - sx[i]| (one IEEE subtraction).  The library is built without contraction, so every value here is the device's value bit for bit: no tolerance anywhere."""
import functools

import numpy as np

BK = 1024          # block length of the pruned search
PAIRCAP = 8192     # its pair list


def prefix(x):
    """the sequential chain sx[i] = sx[i - 1] + x[i]"""
    return np.cumsum(np.asarray(x, np.float64))


def tss_of(x):
    """sum of squares in the order FindChangePoint adds them"""
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x * x)[-1])


def c_of(n, L):
    rn = np.float64(n); rj = np.asarray(L, np.float64)
    return rn / (rj * (rn - rj))


def incumbent(sx):
    """The reference's starting arc (CBSTStatistic.cs:44-137): the global extremes of the prefix sums, where both start as the exact value 0 at position n and only a strictly
    smaller / larger prefix sum replaces them, the first one met.  Returns (value, (lo, hi) 1-based, psdiff); the value is 0 when psdiff <= 0."""
    n = len(sx)
    mn, imn, mx, imx = 0.0, n, 0.0, n
    if sx.min() < 0.0: imn = int(np.argmin(sx)) + 1; mn = float(sx[imn - 1])
    if sx.max() > 0.0: imx = int(np.argmax(sx)) + 1; mx = float(sx[imx - 1])
    psdiff = mx - mn
    pair = (min(imn, imx), max(imn, imx))
    if psdiff <= 0: return 0.0, pair, psdiff
    rj = float(abs(imx - imn))
    return float(c_of(n, rj) * (psdiff * psdiff)), pair, psdiff


def per_length(sx):
    """for every L in 1 .. n - 1: max_i |sx[i + L] - sx[i]| and the smallest i attaining it (index 0 of both arrays is unused)"""
    n = len(sx); dmax = np.zeros(n, np.float64); first = np.zeros(n, np.int32)
    for L in range(1, n):
        d = np.abs(sx[L:] - sx[:-L]); k = int(np.argmax(d)); dmax[L] = d[k]; first[L] = k
    return dmax, first


def every_arc(sx, al0, dmax=None):
    """Every admissible arc: L in max(1, al0) .. min(n - 1, n - al0), every i.  Returns (maximum, number of arcs attaining it, (L, i) smallest among them); (-1.0, 0, None) when no
    length is admissible.  (Rounding is monotone, so the largest statistic of a length is the statistic of its largest |d|; the arcs attaining the maximum are counted by value.)"""
    n = len(sx)
    if dmax is None: dmax = per_length(sx)[0]
    lo, hi = max(1, al0), min(n - 1, n - al0)
    if lo > hi: return -1.0, 0, None
    Ls = np.arange(lo, hi + 1)
    vmax = c_of(n, Ls) * (dmax[lo:hi + 1] * dmax[lo:hi + 1])
    M = float(vmax.max()); count = 0; arc = None
    for L in Ls[vmax == M]:
        L = int(L); d = np.abs(sx[L:] - sx[:-L]); hit = np.nonzero(c_of(n, L) * (d * d) == M)[0]
        count += len(hit)
        if arc is None: arc = (L, int(hit[0]))
    return M, count, arc


def arc_value(sx, L, i):
    d = abs(float(sx[i + L]) - float(sx[i]))
    return float(c_of(len(sx), L) * np.float64(d * d))


def block_model(sx, al0, tau):
    """The pruned search's block level.  Blocks of 1024 prefix sums: first minimum / first maximum (value, position).  word5: the best admissible arc between the extremes of two
    blocks A <= B (min_A to max_B, max_A to min_B), 0 when there is none.  Pairs A <= B survive when max(c(llo), c(lhi)) * D * D >= max(tau, word5), D = max(max_B - min_A,
    max_A - min_B) > 0, [llo, hi] = the pair's arc lengths cut to al0 .. n - al0, not empty.  Returns dict(bmin, bmax, pmin, pmax, word5, npairs, pairs (A, B), d2 (per surviving
    pair: the bound came from max_A - min_B))."""
    n = len(sx); nb = (n + BK - 1) // BK
    bmin = np.zeros(nb); bmax = np.zeros(nb); pmin = np.zeros(nb, np.int64); pmax = np.zeros(nb, np.int64)
    for b in range(nb):
        blk = sx[b * BK:(b + 1) * BK]
        pmin[b] = b * BK + int(np.argmin(blk)); pmax[b] = b * BK + int(np.argmax(blk)); bmin[b] = sx[pmin[b]]; bmax[b] = sx[pmax[b]]
    A, B = np.meshgrid(np.arange(nb), np.arange(nb), indexing="ij")
    upper = B >= A
    rn = np.float64(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        best = 0.0
        for p, q, vp, vq in ((pmin[A], pmax[B], bmin[A], bmax[B]), (pmax[A], pmin[B], bmax[A], bmin[B])):
            L = np.abs(q - p); ok = upper & (L >= al0) & (L <= n - al0)
            d = np.abs(vq - vp); v = (rn / (L.astype(np.float64) * (rn - L))) * (d * d)
            if ok.any(): best = max(best, float(v[ok].max()))
        thr = max(float(tau), best)
        D1 = bmax[B] - bmin[A]; D2 = bmax[A] - bmin[B]; D = np.where(D2 > D1, D2, D1)
        lmin = np.where(B == A, 1, (B - A - 1) * BK + 1); lmax = np.minimum((B - A + 1) * BK - 1, n - 1)
        llo = np.maximum(lmin, al0); lhi = np.minimum(lmax, n - al0)
        live = upper & (D > 0.0) & (llo <= lhi)
        c1 = rn / (llo.astype(np.float64) * (rn - llo)); c2 = rn / (lhi.astype(np.float64) * (rn - lhi)); c = np.where(c1 > c2, c1, c2)
        surv = live & (c * (D * D) >= thr)
    ia, ib = np.nonzero(surv)
    return dict(bmin=bmin, bmax=bmax, pmin=pmin, pmax=pmax, word5=best, npairs=int(surv.sum()), pairs=list(zip(ia.tolist(), ib.tolist())), d2=(D2 > D1)[surv].tolist())


def normalise(b, tss, n):
    """CBSTStatistic.cs:334-337"""
    if tss <= b + 0.0001: tss = b + 1.0
    return b / ((tss - b) / (float(n) - 2.0))


def bits(v):
    return int(np.float64(v).view(np.uint64))


def expected_path(x, sx, al0, inc, ea, oracle):
    """Which way TMaxO of this input is decided (canvas_cbs_arc_probe's h_path & 7).  inc = incumbent(sx), ea = every_arc(sx, al0), oracle() = (statistic, (lo, hi)) of the
    reference's TMaxO (asked only where it decides).  0: the extremes coincide; 1: no admissible arc beats the incumbent; 3: several arcs attain the maximum; otherwise the unique maximiser is the reference's
    answer (2) or an arc its scan leaves out, so that the reference returns less (4)."""
    bss0, _, psdiff = inc
    M, count, arc = ea
    if psdiff <= 0: return 0
    if not (M > bss0): return 1
    if count >= 2: return 3
    n = len(sx); L, i = arc
    stat, iseg = oracle()
    if bits(stat) == bits(normalise(M, tss_of(x), n)) and (int(iseg[0]), int(iseg[1])) == (i + 1, i + 1 + L): return 2
    assert stat < normalise(M, tss_of(x), n), "the reference returned the maximum on another arc, or more than the maximum"
    return 4


# ---------------------------------------------------------------------------------------------------------------- the input catalogue
KINDS = ("f2", "step", "two", "neg", "blk", "sub", "last", "first", "int", "per4", "twin", "cauchy", "zeros")
SEED = 20240611
# (kind, n) -> seed where the catalogue's default does not put the input into the regime it is named after (tests/test_cbs_arc_ref.py checks every one of them)
SEEDS = {("last", 4096): SEED + 3, ("last", 4097): SEED + 3, ("last", 4160): SEED + 1, ("last", 4161): SEED + 2, ("last", 5121): SEED + 1, ("last", 8193): SEED + 2, ("last", 20481): SEED + 1,
         ("first", 4097): SEED + 2, ("first", 4160): SEED + 1, ("first", 5121): SEED + 3, ("first", 8193): SEED + 1, ("first", 12289): SEED + 2, ("first", 20481): SEED + 1,
         ("cauchy", 5121): SEED + 1, ("int", 4097): SEED + 198}


def _centre(x):
    return x - np.cumsum(x)[-1] / len(x)


def _f2(rng, n):
    return np.round(rng.normal(1.0, 0.3, n) * 100.0) / 100.0


@functools.lru_cache(maxsize=None)
def make(kind, n, step=None):
    """the centred segment of a catalogue input (read-only); step: the height of `two`'s step where it is not 0.3"""
    rng = np.random.default_rng([SEEDS.get((kind, n), SEED), KINDS.index(kind), n])
    if kind == "zeros": x = np.zeros(n)
    elif kind == "int":
        x = rng.integers(-1, 2, n).astype(np.float64); s = int(x.sum())
        idx = np.nonzero(x > -1 if s > 0 else x < 1)[0][:abs(s)]; x[idx] -= np.sign(s)
        assert x.sum() == 0
    elif kind == "per4":
        x = np.tile([1.0, 1.0, -1.0, -1.0], n // 4 + 1)[:n]; x[n - n % 4:] = 0.0
    elif kind == "twin":
        x = np.zeros(n); x[100] = 1.0; x[101] = -1.0; x[3000] = 1.0; x[3001] = -1.0
    elif kind == "cauchy":
        x = _centre(np.round(rng.standard_cauchy(n) * 100.0) / 100.0)
    else:
        x = _f2(rng, n)
        if kind == "step": x[n // 3:] += 0.5
        elif kind == "two": x[n // 3:n // 2] += 0.3 if step is None else step
        elif kind == "neg": x[n // 3:n // 2] -= 0.3
        elif kind == "blk": x[1023:1025] += 3.0
        elif kind == "sub": x[63:65] += 3.0
        elif kind == "last": x[n - 1] += 5.0
        elif kind == "first": x[0] -= 5.0
        x = _centre(x)
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return x


def min_size(kind):
    return {"blk": 1026, "sub": 66, "twin": 3003}.get(kind, 4)


MODE0_SIZES = (4, 5, 63, 64, 65, 129, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 3073, 4095, 4096, 4097, 4159, 4160, 4161, 5119, 5120, 5121, 8191, 8192, 8193, 12289, 20481)
MODE0_KIND_SIZES = (4096, 4097, 4160, 4161, 5121, 8193, 12289, 20481)          # every kind but f2
MODE1_SIZES = (4, 5, 255, 256, 257, 510, 511, 512, 513, 514, 1023, 1024, 1025, 1535, 1537, 4096, 4097, 8193)
AL0_SIZES = (4097, 5121)
OVERFLOW_INPUTS = tuple((k, n) for k in ("f2", "two") for n in (5121, 12289))
LARGE_SIZES = (131073, 1048577)
LARGE_STEP = 0.05


def overflow_caps(npairs):
    """pair_cap values around the model's surviving-pair count: the first three overflow, the last two do not"""
    return (1, 4, npairs - 1, npairs, npairs + 1)


def naive_incumbent(sx):
    """NOT the reference's: the arc between argmax and argmin of the prefix sums (without the 0 at position n both extremes start from)"""
    i, j = int(np.argmin(sx)), int(np.argmax(sx)); d = float(sx[j]) - float(sx[i])
    return float(c_of(len(sx), abs(j - i)) * (d * d)) if i != j else 0.0


def al0_values(n):
    return (1, 3, 64, 65, 70, n // 2, n // 2 + 1)


# ---------------------------------------------------------------------------------------------------------------- shared by the two test files (computed once per input)
@functools.lru_cache(maxsize=None)
def reference(kind, n, step=None):
    """(x, sx, incumbent, dmax, first) of a catalogue input, every array read-only"""
    x = make(kind, n, step); sx = prefix(x); dmax, first = per_length(sx)
    for a in (sx, dmax, first): a.setflags(write=False)
    return x, sx, incumbent(sx), dmax, first


@functools.lru_cache(maxsize=None)
def oracle_tmaxo(kind, n, al0, step=None):
    """the oracle's TMaxO of a catalogue input: (statistic, (lo, hi) 1-based); the sum of squares is added up in FindChangePoint's order"""
    import ctypes as C
    import oracle_lib as O
    x = np.ascontiguousarray(make(kind, n, step)); sx = np.zeros_like(x); iseg = np.zeros(2, np.int32); ostat = C.c_double()
    O.lib.orc_tmaxo(O._p(x), len(x), C.c_double(tss_of(x)), O._p(sx), O._p(iseg), C.byref(ostat), int(al0))
    return ostat.value, (int(iseg[0]), int(iseg[1]))


@functools.lru_cache(maxsize=None)
def search(kind, n, al0):
    """(every_arc, block_model, expected path) of a catalogue input at one minimum arc length"""
    x, sx, inc, dmax, _ = reference(kind, n)
    ea = every_arc(sx, al0, dmax); bm = block_model(sx, al0, inc[0])
    return ea, bm, expected_path(x, sx, al0, inc, ea, lambda: oracle_tmaxo(kind, n, al0))


def mode0_cases():
    """(kind, n, al0) of the pruned search's cases: f2 at every size, every other kind at the sizes that hold its pattern; al0 2 everywhere, more of them at 4097 and 5121"""
    out = []
    for kind in KINDS:
        for n in (MODE0_SIZES if kind == "f2" else MODE0_KIND_SIZES):
            if n < min_size(kind): continue
            out.append((kind, n, 2))
            if n in AL0_SIZES: out += [(kind, n, a) for a in al0_values(n)]
    return out
