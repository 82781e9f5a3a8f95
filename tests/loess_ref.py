"""CanvasClean -m LOESS restated from the C# (CanvasClean/LoessGCNormalizer.cs, CanvasClean/LoessInterpolator.cs, Utilities.GoldenSectionSearch) in plain
Python / numpy with every sum in numpy.longdouble (64-bit mantissa on x86-64).  It shares nothing with oracle/*.cpp or canvas_amd/csrc/loess.hpp.

Two layers compute the same quantities:

  literal   point by point: the stable sort, updateBandwidthInterval one index at a time, computeIntervals, Predict over Range(minGC, maxGC) read as
            (start, COUNT), the objective's two trainings, the golden section, the clamped index of Normalize.  For a few thousand points.
  grouped   the abscissa is an integer GC percentage, so the sorted array is <= 101 runs of equal x; every window sum becomes a sum over runs of
            (points of the run inside the window) x (per-run weight), the y sums from per-run longdouble prefix sums.  O(n) numpy plus small fits.

What has no arithmetic freedom is done exactly as the C# does it, in double: the bandwidth and ceil(bandwidth * n), which points a window holds, which
end is `edge`, denom, the tricube weight of a point, xk * w, `fc < fd` (false when either side is NaN).  Only the accumulations (the five weighted sums, the
mean and the squared deviations of the objective, the prefix sums) and what is derived from them (means, beta, alpha, the fit, log, exp) are longdouble.
`meanXX == meanX * meanX` is evaluated on the longdouble means; a fit at which that comparison could come out differently in double is counted in
`degenerate` (see _solve), and the committed cases have none.
"""
import math

import numpy as np

LD = np.longdouble
GOLDEN = 0.618034          # Utilities.cs: "golden ratio - 1", as typed there
NGC = 101


class LoessIndexError(IndexError):
    """the C# indexes fittedByGC past its end (objective: fittedByGC[gc - minGC] with minGC == 0, since Range(minGC, maxGC) has maxGC entries)"""


class Diag:
    def __init__(self):
        self.degenerate = 0      # fits READ by a bin whose value is rounding noise: a finite value from a window inside one GC run, or a variance of x that is noise (see _solve)
        self.fits = 0
        self.flag = False        # whether the last fit was such a fit

    def count_used(self, flags, used):
        self.degenerate += int(flags[np.unique(used)].sum())


def _tricube(a):
    t = 1 - a * a * a
    return t * t * t


def _weights(x, xk, x_edge):
    """per-point double arithmetic of computeCoefficients: w = tricube(|x - xk| * |1 / (x_edge - x)|), xk * w, xk * (xk * w)"""
    with np.errstate(all="ignore"):
        denom = np.abs(np.float64(1.0) / np.float64(x_edge - x))
        w = _tricube(np.abs(np.float64(x) - xk) * denom)
        xkw = xk * w
        return w, xkw, xk * xkw


def _sum(v):
    """left-to-right longdouble sum.  Sequential on purpose: a term that is exactly 0 (a point at the window's edge has tricube weight 0) then leaves the sum bit for bit
    as it was, as it does in the C#'s loop, so two bandwidths that differ only by such points give EQUAL objectives and `fc < fd` is false for every reader
    (numpy's pairwise sum would regroup the other terms and turn that exact tie into rounding noise)"""
    return np.cumsum(v, dtype=LD)[-1] if len(v) else LD(0)


def _solve(x, sw, sx, sxx, sy, sxy, single_run, diag):
    with np.errstate(all="ignore"):
        mx, my, mxy, mxx = sx / sw, sy / sw, sxy / sw, sxx / sw
        var = mxx - mx * mx
        beta = LD(0) if mxx == mx * mx else (mxy - mx * my) / var
        alpha = my - beta * mx
        out = alpha + LD(x) * beta
    diag.fits += 1
    diag.flag = bool(np.isfinite(out) and (single_run or (var != 0 and abs(var) < 1e-9 * abs(mxx))))
    return out


def _median(y):
    s = np.sort(y)
    m = len(s)
    return s[m // 2] if m % 2 else (s[m // 2 - 1] + s[m // 2]) / LD(2)


def _bandwidth_in_points(bandwidth, n):
    k = int(math.ceil(bandwidth * n))
    if k < 2:
        raise ValueError("bandwidth too small for 2 points")
    return k


# ------------------------------------------------------------------------------------------------------------------ literal layer
def _update_literal(x, xs, l, r):
    n = len(xs)
    updated = False
    while r < n - 1 and x > xs[r]:
        l += 1; r += 1; updated = True
    while r < n - 1 and xs[r + 1] - x < x - xs[l]:
        l += 1; r += 1; updated = True
    return l, r, updated


def _intervals(update, first, last, k):
    """computeIntervals with xStep = 1: an interval is closed with the window it had BEFORE the update that ends it"""
    out = []
    l, r = 0, k - 1
    xmin = -math.inf
    x = float(first)
    while x <= last:
        nl, nr, upd = update(x, l, r)
        if upd:
            out.append((xmin, x, l, r))
            xmin = x; l, r = nl, nr
        x += 1.0
    out.append((xmin, math.inf, l, r))
    return out


def _predict(fit, intervals, min_gc, count, diag):
    """LoessModel.Predict(Enumerable.Range(minGC, maxGC)): `count` abscissae from min_gc upwards, the interval index only ever moves right"""
    out = np.zeros(max(count, 0), LD); flags = np.zeros(max(count, 0), bool)
    j = 0
    for i in range(count):
        x = float(min_gc + i)
        while j < len(intervals) - 1 and intervals[j][1] <= x:
            j += 1
        out[i] = fit(x, intervals[j][2], intervals[j][3]); flags[i] = diag.flag
    return out, flags


def _train_predict_literal(gcs, ys, bandwidth, min_gc, count, diag):
    order = np.argsort(gcs, kind="stable")
    xs = gcs[order].astype(np.float64); sy = ys[order]
    xl = xs.tolist()
    k = _bandwidth_in_points(bandwidth, len(xs))

    def fit(x, l, r):
        edge = l if (x - xl[l] > xl[r] - x) else r
        xk = xs[l:r + 1]; yk = sy[l:r + 1]
        w, xkw, xxkw = _weights(x, xk, xl[edge])
        with np.errstate(all="ignore"):
            return _solve(x, _sum(w), _sum(xkw), _sum(xxkw), _sum(yk * w), _sum(yk * xkw), xl[l] == xl[r], diag)

    iv = _intervals(lambda x, l, r: _update_literal(x, xl, l, r), xl[0], xl[-1], k)
    return _predict(fit, iv, min_gc, count, diag)


def _objective_literal(bandwidth, gcs, ys, diag):
    med = _median(ys)
    min_gc, max_gc = int(gcs.min()), int(gcs.max())
    idx = gcs.astype(np.int64) - min_gc
    fit1, flags1 = _train_predict_literal(gcs, ys, bandwidth, min_gc, max_gc, diag)
    if idx.max() >= len(fit1):
        raise LoessIndexError("fittedByGC[gc - minGC] past the end: a bin with GC = 0 in the bandwidth search")
    normalized = ys - fit1[idx] + med
    fit2, flags2 = _train_predict_literal(gcs, normalized, bandwidth, min_gc, max_gc, diag)
    diag.count_used(flags1, idx); diag.count_used(flags2, idx)
    fitted = fit2[idx]
    with np.errstate(all="ignore"):
        mu = _sum(fitted) / LD(len(fitted))
        d = fitted - mu
        return np.sqrt(_sum(d * d) / LD(len(fitted) - 1))


# ------------------------------------------------------------------------------------------------------------------ grouped layer
class _Runs:
    """the sorted array as runs of equal x: off[g] = sorted index of the first point with x == g; pref[g] = longdouble prefix sums of the run's y in file order"""

    def __init__(self, gcs, ys):
        g = gcs.astype(np.int64)
        if g.min() < 0 or g.max() >= NGC:
            raise ValueError("GC outside 0..100")
        order = np.argsort(g, kind="stable")
        cnt = np.bincount(g, minlength=NGC)
        self.off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        self.n = len(g)
        ysorted = ys[order]
        self.pref = [np.concatenate([[LD(0)], np.cumsum(ysorted[self.off[k]:self.off[k + 1]], dtype=LD)]) for k in range(NGC)]
        self.cnt = cnt
        self.shift = np.zeros(NGC, LD)           # y' = y - shift[x]: the second training of the objective
        self.min_gc = int(g.min()); self.max_gc = int(g.max())

    def val(self, i):
        return int(np.searchsorted(self.off, i, side="right")) - 1

    def update(self, x, l, r):
        n = self.n; l0 = l
        if r < n - 1 and x > self.val(r):
            below = int(self.off[min(NGC, max(0, int(math.ceil(x))))])       # points with x' < x: the first loop stops at the first of the others, or at n - 1
            nr = min(n - 1, max(r, below))
            l += nr - r; r = nr
        # second loop: it advances while xs[r + 1 + s] - x < x - xs[l + s]; the left side only grows with s and the right side only shrinks, so the
        # steps taken are the smallest s at which that fails (or the end of the array): bisection
        lo, hi = 0, n - 1 - r
        while lo < hi:
            mid = (lo + hi) // 2
            if self.val(r + 1 + mid) - x < x - self.val(l + mid):
                lo = mid + 1
            else:
                hi = mid
        return l + lo, r + lo, (l + lo) != l0

    def fit(self, x, l, r, diag):
        vl, vr = self.val(l), self.val(r)
        edge = vl if (x - vl > vr - x) else vr
        gs = np.arange(vl, vr + 1)
        a = np.maximum(l, self.off[gs]); b = np.minimum(r, self.off[gs + 1] - 1)
        keep = b >= a
        gs, a, b = gs[keep], a[keep], b[keep]
        m = (b - a + 1).astype(LD)
        ysum = np.array([self.pref[g][bb + 1 - self.off[g]] - self.pref[g][aa - self.off[g]] for g, aa, bb in zip(gs.tolist(), a.tolist(), b.tolist())], LD) - m * self.shift[gs]
        w, xkw, xxkw = _weights(x, gs.astype(np.float64), float(edge))
        with np.errstate(all="ignore"):
            return _solve(x, _sum(m * w), _sum(m * xkw), _sum(m * xxkw), _sum(ysum * w), _sum(ysum * xkw), vl == vr, diag)

    def train_predict(self, bandwidth, min_gc, count, diag):
        k = _bandwidth_in_points(bandwidth, self.n)
        iv = _intervals(self.update, self.min_gc, self.max_gc, k)
        return _predict(lambda x, l, r: self.fit(x, l, r, diag), iv, min_gc, count, diag)


def _objective_grouped(bandwidth, runs, med, diag):
    lo, hi = runs.min_gc, runs.max_gc
    runs.shift[:] = 0
    fit1, flags1 = runs.train_predict(bandwidth, lo, hi, diag)
    if hi - lo >= len(fit1):
        raise LoessIndexError("fittedByGC[gc - minGC] past the end: a bin with GC = 0 in the bandwidth search")
    runs.shift[lo:hi + 1] = fit1[:hi - lo + 1] - med
    fit2, flags2 = runs.train_predict(bandwidth, lo, hi, diag)
    runs.shift[:] = 0
    m = runs.cnt[lo:hi + 1].astype(LD); f = fit2[:hi - lo + 1]
    used = runs.cnt[lo:hi + 1] > 0
    diag.count_used(flags1, np.flatnonzero(used)); diag.count_used(flags2, np.flatnonzero(used))
    m, f = m[used], f[used]
    with np.errstate(all="ignore"):
        mu = _sum(m * f) / LD(runs.n)
        d = f - mu
        return np.sqrt(_sum(m * d * d) / LD(runs.n - 1))


# ------------------------------------------------------------------------------------------------------------------ the normaliser
def golden_section(f, a, b, tol=1e-5):
    """Utilities.GoldenSectionSearch; returns (argmin, [(c, d, fc, fd) at every comparison it made])"""
    c = b - GOLDEN * (b - a)
    d = a + GOLDEN * (b - a)
    fc, fd = f(c), f(d)
    probes = []
    while abs(d - c) > tol:
        probes.append((c, d, fc, fd))
        if fc < fd:
            b = d; d = c; fd = fc
            c = b - GOLDEN * (b - a); fc = f(c)
        else:
            a = c; c = d; fc = fd
            d = a + GOLDEN * (b - a); fd = f(d)
    return (b + a) / 2, probes


def normalize(count, gc, chr_id=None, is_y=None, layer="grouped"):
    """LoessGCNormalizer(bins, null, 0, Math.Log, Math.Exp).Normalize() on float32 counts.  Returns a dict: ld (longdouble counts), f32 (those rounded once to
    float32), nan (mask), bandwidth, probes [(c, d, fc, fd)], degenerate (see Diag), fits.  Raises LoessIndexError where the C# indexes out of range."""
    assert layer in ("literal", "grouped")
    count = np.asarray(count, np.float32); gc = np.asarray(gc, np.int64)
    with np.errstate(all="ignore"):
        logc = np.log(count.astype(LD))
    use = ~np.isinf(logc)                               # !double.IsInfinity(count): a zero count stays out of the model
    not_y = np.ones(len(count), bool) if (is_y is None or chr_id is None) else (np.asarray(is_y, np.uint8)[np.asarray(chr_id)] == 0)
    gcs, ys = gc[use], logc[use]
    g2, y2 = gc[use & not_y], logc[use & not_y]
    diag = Diag()
    lo_bw = max(2.0 / len(g2), 0.3); hi_bw = min(1.0, 0.75)
    if hi_bw < lo_bw:
        hi_bw = lo_bw
    if layer == "literal":
        best, probes = golden_section(lambda b: _objective_literal(b, g2, y2, diag), lo_bw, hi_bw)
    else:
        runs2 = _Runs(g2, y2); med2 = _median(y2)
        best, probes = golden_section(lambda b: _objective_grouped(b, runs2, med2, diag), lo_bw, hi_bw)
    med = _median(ys)
    min_gc, max_gc = int(gcs.min()), int(gcs.max())
    if layer == "literal":
        fitted, flags = _train_predict_literal(gcs, ys, best, min_gc, max_gc, diag)
    else:
        fitted, flags = _Runs(gcs, ys).train_predict(best, min_gc, max_gc, diag)
    if len(fitted) == 0:
        raise LoessIndexError("fittedByGC is empty")
    k = np.minimum(len(fitted) - 1, np.maximum(0, gc - min_gc))
    diag.count_used(flags, k)
    with np.errstate(all="ignore"):
        out = np.exp(logc - fitted[k] + med)
    return dict(ld=out, f32=out.astype(np.float32), nan=np.isnan(out), bandwidth=best, probes=probes, degenerate=diag.degenerate, fits=diag.fits, fitted=fitted, median=med)


def ulp_distance(a, b):
    """distance in float32 units in the last place between two float32 arrays (finite values; a NaN or a sign difference gives a huge number)"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
