"""CPU checks of the CanvasNormalize restatement (tests/normalize_modes_ref.py) against literal per-element loops, the PCA model file round trip and
the orthogonality decision on both sides of the 1e-4 tolerance."""
import math

import numpy as np

import normalize_modes_ref as R
import oracle_lib as O


def _loop_sum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def _loop_best_lr2(tumor, normals):
    def med(v):
        v = sorted(v)
        n = len(v)
        return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2

    def weight(v):
        m = med(v)
        return 1.0 / m if m > 0 else 0.0
    wt = weight(tumor)
    tb = [t * wt for t in tumor]
    best, best_v, out = -1, math.inf, []
    for i, c in enumerate(normals):
        wn = weight(c)
        s, nb, ign = 0.0, 0, 0
        for a, x in zip(tb, c):
            b = x * wn
            if b <= 0:
                ign += 1
                continue
            q = a / b
            if q <= 0 or math.isinf(q):
                ign += 1
                continue
            lr = math.log(q)
            sq = lr * lr
            if math.isinf(sq) or math.isnan(sq):
                ign += 1
                continue
            s += sq
            nb += 1
        v = s / nb if nb > 0 else s
        out.append((v, ign))
        if v < best_v:
            best, best_v = i, v
    return best, out


def _loop_pca(sample, mu, axes, min_ref, max_ref):
    units = []
    for a in axes:
        s = 0.0
        for x in a:
            s += x * x
        size = math.sqrt(s)
        units.append([x / size for x in a] if size != 0 else list(a))
    for i in range(len(units)):
        for j in range(i + 1, len(units)):
            d = 0.0
            for x, y in zip(units[i], units[j]):
                d += x * y
            if abs(d) > 1e-4:
                return None
    n = len(mu)
    x = [float(np.float32(max(np.float32(1.0), np.float32(sample[i])))) - float(mu[i]) for i in range(n)]
    sizes = []
    for u in units:
        d = 0.0
        for a, b in zip(x, u):
            d += a * b
        sizes.append(d)
    ref = []
    for i in range(n):
        p = sizes[0] * units[0][i]
        for k in range(1, len(units)):
            p += sizes[k] * units[k][i]
        y = float(mu[i]) + p
        ref.append(1.0 if 1.0 > y else y)
    ratios = []
    for i in range(n):
        rq = float(np.float32(float(O.format_f2(float(np.float32(ref[i]))))))
        if rq < min_ref or rq > max_ref:
            continue
        ratios.append(float(np.float32(sample[i]) / np.float32(rq)))
    ratios.sort()
    m = len(ratios)
    med = 0.0 if m == 0 else (ratios[m // 2] if m % 2 else (ratios[m // 2 - 1] + ratios[m // 2]) / 2)
    return np.array([np.float32(r * med) for r in ref], np.float32), med, sizes


def test_seq_sum_is_left_to_right():
    rng = np.random.RandomState(1)
    x = rng.standard_normal(2000) * 10.0 ** rng.randint(-8, 8, 2000)
    assert R.seq_sum(x) == _loop_sum(x.tolist())
    assert R.seq_sum([1e16, 1.0, -1e16]) == 0.0 and R.seq_sum([]) == 0.0


def test_best_lr2_matches_loop():
    rng = np.random.RandomState(2)
    for trial in range(6):
        n = int(rng.randint(5, 2000))
        base = rng.gamma(2.0, 50.0, n)
        tumor = np.round(rng.poisson(base) * 1.0, 2)
        normals = [np.round(rng.poisson(base * (0.5 + 0.3 * s)) * 1.0, 2) for s in range(int(rng.randint(2, 6)))]
        if trial == 1:
            normals.append(normals[0].copy())
        if trial == 2:
            tumor[:] = 0.0
        best, msl, ign = R.best_lr2(tumor, normals)
        lb, lo = _loop_best_lr2(tumor.tolist(), [c.tolist() for c in normals])
        assert best == lb
        assert [v for v, _ in lo] == msl and [g for _, g in lo] == ign


def test_best_lr2_on_target_list():
    rng = np.random.RandomState(3)
    n = 900
    tumor = rng.poisson(30, n) * 1.0; normals = [rng.poisson(30 + 5 * s, n) * 1.0 for s in range(3)]
    on = np.sort(rng.choice(n, 300, replace=False))
    best, msl, ign = R.best_lr2(tumor, normals, on)
    lb, lo = _loop_best_lr2(tumor[on].tolist(), [c[on].tolist() for c in normals])
    assert best == lb and [v for v, _ in lo] == msl


def test_pca_matches_loop():
    rng = np.random.RandomState(4)
    for n, k, lo, hi in [(40, 1, 1.0, math.inf), (513, 3, 1.0, math.inf), (1500, 4, 20.0, 200.0)]:
        base = rng.gamma(3.0, 30.0, n)
        controls = np.array([rng.poisson(base * (0.8 + 0.1 * s)) for s in range(8)], np.float64)
        mu = controls.mean(axis=0).astype(np.float32)
        _, _, vt = np.linalg.svd(controls - mu.astype(np.float64), full_matrices=False)
        axes = [vt[i] * 3.0 for i in range(k)]                 # not unit length: the reader normalises
        sample = (rng.poisson(base) * 1.0).astype(np.float32)
        sample[:5] = 0.25                                      # counts below 1
        got = R.pca_reference(sample, mu, axes, O.format_f2, lo, hi)
        exp = _loop_pca(sample, mu, axes, lo, hi)
        assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all()
        assert got[1] == exp[1] and list(got[2]) == exp[2]


def test_pca_zero_axis_kept():
    u = R.normalize_by_2norm(np.zeros(7))
    assert (u == 0).all()
    assert R.are_orthogonal([u, R.normalize_by_2norm(np.arange(7.0))])


def test_model_round_trip(tmp_path):
    rng = np.random.RandomState(5)
    n = 300
    chrom = ["chr1"] * 200 + ["chr2"] * 100
    start = np.arange(n) * 1000; stop = start + 1000
    mu = (rng.gamma(2.0, 40.0, n)).astype(np.float32)
    axes = [rng.standard_normal(n) for _ in range(3)]
    for name in ("m.txt.gz", "m.txt"):
        p = str(tmp_path / name)
        R.write_model(p, chrom, start, stop, mu, axes)
        c, s, e, m, a = R.read_model(p)
        assert c == chrom and (s == start).all() and (e == stop).all()
        assert (m.view(np.uint32) == mu.view(np.uint32)).all()
        assert len(a) == 3 and all((x.view(np.uint64) == y.view(np.uint64)).all() for x, y in zip(a, axes))


def orthogonality_edge_axes(above):
    """two axes whose unit vectors have a dot product of exactly the double 1e-4 (orthogonal: |dot| > 1e-4 fails) or of the next double above it"""
    target = 1e-4 if not above else math.nextafter(1e-4, 1.0)
    t = 1.000000005e-4
    for _ in range(200000):
        b = np.array([t, 1.0])
        d = R.dot(R.normalize_by_2norm(np.array([1.0, 0.0])), R.normalize_by_2norm(b))
        if d == target:
            return np.array([1.0, 0.0]), b
        t = math.nextafter(t, 1.0 if d < target else 0.0)
    raise AssertionError("no axis found")


def test_orthogonality_both_sides_of_tolerance():
    a, b = orthogonality_edge_axes(False)
    assert R.dot(R.normalize_by_2norm(a), R.normalize_by_2norm(b)) == 1e-4
    assert R.are_orthogonal([R.normalize_by_2norm(a), R.normalize_by_2norm(b)])
    a, b = orthogonality_edge_axes(True)
    assert not R.are_orthogonal([R.normalize_by_2norm(a), R.normalize_by_2norm(b)])


def test_reference_copy_number():
    ivs = [(1001, 3000, 1), (5001, 6000, 0), (7001, 8000, 2)]
    assert R.reference_copy_number(None, 0, 1000) == 2
    assert R.reference_copy_number(ivs, 1000, 2000) == 1
    assert R.reference_copy_number(ivs, 2500, 3500) == 1          # 500 bases each at 1 and 2: the lower copy number wins the tie
    assert R.reference_copy_number(ivs, 2400, 3500) == 1          # 600 bases at 1, 500 at 2
    assert R.reference_copy_number(ivs, 5000, 6000) == 0
    assert R.reference_copy_number(ivs, 7000, 8000) == 2


def test_cnd_lines():
    lines = R.cnd_lines(np.array([12.5], np.float32), np.array([1.0 / 3], np.float32), ["chr1"], [0], [1000], np.array([1e7], np.float32), O.format_g7)
    assert lines[0] == "Fragment Count,Reference Count,Chromosome,Start,End,Unsmoothed Log Ratio"
    assert lines[1] == "12.5,0.3333333,chr1,0,1000,1E+07"
