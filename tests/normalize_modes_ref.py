"""Plain Python / numpy restatement of the CanvasNormalize pieces the GPU tests check: BestLR2ReferenceGenerator, PCAReferenceGenerator,
RawRatioCalculator, RatiosToCounts with the reference ploidy, WriteCndFile, and the PCA model file.

Sequential sums are np.add.accumulate (element after element, in index order: the reference's loops), never np.sum / np.dot (pairwise or BLAS order);
the log is math.log (the C library's, as .NET Core on Linux); text goes through the formatters of tests/oracle_lib.py."""
import gzip
import math

import numpy as np


def seq_sum(terms):
    """sum of the terms added one after another, left to right"""
    terms = np.ascontiguousarray(terms, np.float64)
    return float(np.add.accumulate(terms)[-1]) if len(terms) else 0.0


def median(values):
    """Utilities.Median / SortedList<double>.Median: middle element, or the mean of the two middle ones"""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    if n == 0:
        return 0.0
    return float(v[n // 2]) if n & 1 else float((v[n // 2 - 1] + v[n // 2]) / 2)


def _log(q):
    q = float(q)
    if math.isnan(q) or q < 0:
        return math.nan
    if q == 0:
        return -math.inf
    if math.isinf(q):
        return math.inf
    return math.log(q)


# ---- BestLR2ReferenceGenerator (BestLR2ReferenceGenerator.cs:31-124)
def weight_of(counts, on_idx=None):
    c = np.asarray(counts, np.float64)
    m = median(c if on_idx is None else c[on_idx])
    return 1.0 / m if m > 0 else 0.0


def mean_squared_log_ratios(tumor, normal, wt, wn, on_idx=None):
    """GetMeanSquaredLogRatios on the weighted on-target counts: (mean, ignored bins)"""
    t = np.asarray(tumor, np.float64); c = np.asarray(normal, np.float64)
    if on_idx is not None:
        t = t[on_idx]; c = c[on_idx]
    tb = t * wt; nb = c * wn                                   # one rounding each, as `cnt * weight`
    terms = []; ignored = 0
    for a, b in zip(tb.tolist(), nb.tolist()):
        if b <= 0:
            ignored += 1
            continue
        lr = _log(a / b)
        sq = lr * lr
        if math.isinf(sq) or math.isnan(sq):
            ignored += 1
            continue
        terms.append(sq)
    s = seq_sum(terms)
    return (s / len(terms) if terms else s), ignored


def best_lr2(tumor, normals, on_idx=None):
    """index of the normal BestLR2 copies, mean squared log ratio and ignored bins per normal"""
    wt = weight_of(tumor, on_idx)
    best, best_v, msl, ign = -1, math.inf, [], []
    for i, c in enumerate(normals):
        v, g = mean_squared_log_ratios(tumor, c, wt, weight_of(c, on_idx), on_idx)
        msl.append(v); ign.append(g)
        if v < best_v:
            best, best_v = i, v
    return best, msl, ign


# ---- PCAReferenceGenerator (PCAReferenceGenerator.cs:32-148, Utilities.cs:601-750)
def two_norm(v):
    v = np.asarray(v, np.float64)
    return math.sqrt(seq_sum(v * v))


def normalize_by_2norm(v):
    v = np.asarray(v, np.float64)
    size = two_norm(v)
    return v.copy() if size == 0 else v / size


def dot(a, b):
    return seq_sum(np.asarray(a, np.float64) * np.asarray(b, np.float64))


def are_orthogonal(units, tolerance=1e-4):
    for i in range(len(units)):
        for j in range(i + 1, len(units)):
            if abs(dot(units[i], units[j])) > tolerance:
                return False
    return True


def f2_round_trip(values, format_f2):
    """(float)ref -> "{F2}" text -> float.Parse (the double parse of the text, then float)"""
    return np.array([float(format_f2(float(v))) for v in np.asarray(values, np.float32)], np.float64).astype(np.float32)


def raw_ratio(sample, reference, min_ref=1.0, max_ref=math.inf):
    """RawRatioCalculator.Run (RawRatioCalculator.cs:21-46) over the zipped prefix: (kept bin indices, float ratios)"""
    n = min(len(sample), len(reference))
    s = np.asarray(sample, np.float32)[:n]; r = np.asarray(reference, np.float32)[:n]
    rd = r.astype(np.float64)
    keep = np.nonzero(~(rd < min_ref) & ~(rd > max_ref))[0].astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (s[keep] / r[keep]).astype(np.float32)        # float / float
    return keep, ratio


def pca_reference(sample, mu, axes, format_f2, min_ref=1.0, max_ref=math.inf):
    """the reference counts PCAReferenceGenerator writes (float32), the median ratio and the projection sizes; None when the axes are not orthogonal.
    sample: float32 counts (cut to the model's length), mu: float32 means, axes: raw float64 axes"""
    sample = np.asarray(sample, np.float32); mu = np.asarray(mu, np.float32)
    units = [normalize_by_2norm(a) for a in axes]
    if not are_orthogonal(units):
        return None
    c = np.where(np.float32(1.0) > sample, np.float32(1.0), sample)           # Math.Max(1, bin.Count) in float
    x = c.astype(np.float64) - mu.astype(np.float64)
    sizes = [dot(x, u) for u in units]
    proj = sizes[0] * units[0]
    for s, u in zip(sizes[1:], units[1:]):
        proj = proj + s * u                                    # Project: each product rounded, then added left to right over the axes
    y = mu.astype(np.float64) + proj
    ref = np.where(1.0 > y, 1.0, y)                            # Math.Max(1, x)
    refq = f2_round_trip(ref.astype(np.float32), format_f2)
    _, ratio = raw_ratio(sample, refq, min_ref, max_ref)
    med = median(ratio.astype(np.float64))
    return (ref * med).astype(np.float32), med, np.array(sizes, np.float64)


# ---- the PCA model file (PCAModel.LoadModel, PCAReferenceGenerator.cs:92-127)
def write_model(path, chrom, start, stop, mu, axes):
    """tab-separated chrom, start, stop, mean, axis values; gzip when the path ends in .gz.  Numbers are written with enough digits to parse back exactly."""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "wt") as f:
        for i in range(len(mu)):
            f.write("\t".join([str(chrom[i]), str(int(start[i])), str(int(stop[i])), "%.9g" % float(mu[i])] + ["%.17g" % float(a[i]) for a in axes]) + "\n")


def read_model(path):
    """(chrom, start, stop, float32 means, list of float64 axes): float.Parse of the mean (a double parse, then float), double.Parse of the axes"""
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    op = gzip.open if gz else open
    chrom, start, stop, mu, axes = [], [], [], [], None
    with op(path, "rt") as f:
        for line in f:
            t = line.rstrip("\r\n").split("\t")
            if axes is None:
                axes = [[] for _ in range(len(t) - 4)]
            chrom.append(t[0]); start.append(int(t[1])); stop.append(int(t[2])); mu.append(float(t[3]))
            for k in range(len(axes)):
                axes[k].append(float(t[4 + k]))
    return chrom, np.array(start, np.int64), np.array(stop, np.int64), np.array(mu, np.float64).astype(np.float32), [np.array(a, np.float64) for a in (axes or [])]


# ---- RatiosToCounts with the reference ploidy and WriteCndFile (CanvasNormalizeUtilities.cs:13-90, PloidyInfo.cs:56-75)
def reference_copy_number(ivs, start, stop):
    """ivs: [(one-based start, end, ploidy)] of the bin's chromosome, None when the VCF does not list it"""
    if ivs is None:
        return 2
    counts = [0, 0, stop - start, 0, 0]
    for s, e, p in ivs:
        if p == 2:
            continue
        o0 = max(start, s - 1)
        if o0 > e:
            continue
        ob = min(stop, e) - o0
        if ob <= 0:
            continue
        counts[2] -= ob; counts[p] += ob
    best, cn = 0, 2
    for c in range(5):
        if counts[c] > best:
            best, cn = counts[c], c
    return cn


def ratios_to_counts(ratio, ploidy):
    return (ratio.astype(np.float64) * (40.0 * np.asarray(ploidy, np.float64) / 2.0)).astype(np.float32)


def cnd_lines(frag_count, ref_count, chrom, start, stop, ratio, format_g7):
    """the .cnd text of the kept bins: comma-joined fields, floats as float.ToString() (7 significant digits)"""
    out = ["Fragment Count,Reference Count,Chromosome,Start,End,Unsmoothed Log Ratio"]
    for i in range(len(ratio)):
        out.append(",".join([format_g7(float(frag_count[i])), format_g7(float(ref_count[i])), str(chrom[i]), str(int(start[i])), str(int(stop[i])), format_g7(float(ratio[i]))]))
    return out
