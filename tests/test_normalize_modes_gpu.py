"""CanvasNormalize's BestLR2 and PCA reference generators on the GPU (canvas_normalize_best_normal / canvas_normalize_pca_reference) against the
restatement of tests/normalize_modes_ref.py: the PCA reference counts, median ratio and projection sizes as bit patterns, BestLR2's choice exactly."""
import math

import numpy as np
import pytest

import normalize_modes_ref as R
import oracle_lib as O
from gpu_common import get_canvas, to_dev
from test_normalize_modes_ref import orthogonality_edge_axes

pytestmark = pytest.mark.gpu


def _model(rng, n, k, ncontrols):
    base = rng.gamma(3.0, 30.0, n)
    controls = np.array([rng.poisson(base * (0.7 + 0.08 * s)) + rng.randint(0, 4, n) * 0.25 for s in range(ncontrols)], np.float64)
    mu = controls.mean(axis=0).astype(np.float32)
    _, _, vt = np.linalg.svd(controls - mu.astype(np.float64), full_matrices=False)
    axes = [vt[i] * (1.0 + i) for i in range(min(k, len(vt)))]
    return base, mu, axes


def _run_pca(cv, sample, mu, axes, lo=1.0, hi=math.inf):
    got = cv.normalize_pca_reference(to_dev(sample, cv.device), to_dev(mu, cv.device), [to_dev(a, cv.device) for a in axes], lo, hi)
    exp = R.pca_reference(sample, mu, axes, O.format_f2, lo, hi)
    return got, exp


def _same(got, exp):
    assert got is not None and exp is not None
    ref, med, sizes = got
    assert (ref.cpu().numpy().view(np.uint32) == exp[0].view(np.uint32)).all()
    assert np.float64(med).view(np.uint64) == np.float64(exp[1]).view(np.uint64)
    assert (np.asarray(sizes).view(np.uint64) == exp[2].view(np.uint64)).all()


@pytest.mark.parametrize("n,k,ncontrols,lo,hi", [(1, 1, 8, 1.0, math.inf), (513, 5, 8, 1.0, math.inf), (513, 1, 8, 30.0, 150.0),
                                                 (200_001, 5, 8, 1.0, math.inf), (200_001, 12, 16, 20.0, 400.0)])
def test_pca_reference(n, k, ncontrols, lo, hi):
    cv = get_canvas()
    rng = np.random.RandomState(n + 31 * k)
    base, mu, axes = _model(rng, n, k, ncontrols)
    if n == 1:
        axes = [np.array([2.5])]
    sample = (rng.poisson(base) * 1.0 + rng.randint(0, 4, n) * 0.25).astype(np.float32)
    sample[rng.rand(n) < 0.05] = 0.5                          # counts below 1: the centring uses max(1, count), the ratio the count itself
    got, exp = _run_pca(cv, sample, mu, axes, lo, hi)
    _same(got, exp)


def test_pca_zero_axis():
    cv = get_canvas()
    rng = np.random.RandomState(11)
    base, mu, axes = _model(rng, 4097, 3, 8)
    axes.insert(1, np.zeros(4097))
    sample = (rng.poisson(base) * 1.0).astype(np.float32)
    got, exp = _run_pca(cv, sample, mu, axes)
    _same(got, exp)
    assert got[2][1] == 0.0


def test_pca_not_orthogonal():
    cv = get_canvas()
    rng = np.random.RandomState(12)
    base, mu, axes = _model(rng, 2000, 2, 8)
    sample = (rng.poisson(base) * 1.0).astype(np.float32)
    got, exp = _run_pca(cv, sample, mu, [axes[0], axes[0] + 0.05 * axes[1]])
    assert got is None and exp is None


@pytest.mark.parametrize("above", [False, True])
def test_pca_orthogonality_at_the_tolerance(above):
    """|dot| exactly 1e-4 (orthogonal) and one ulp above (not): the parallel dot cannot decide, the chain does"""
    cv = get_canvas()
    a, b = orthogonality_edge_axes(above)
    n = 700
    A = np.zeros(n); B = np.zeros(n); A[:2] = a; B[:2] = b
    rng = np.random.RandomState(13)
    mu = rng.gamma(3.0, 30.0, n).astype(np.float32)
    sample = (rng.poisson(mu) * 1.0).astype(np.float32)
    got, exp = _run_pca(cv, sample, mu, [A, B])
    if above:
        assert got is None and exp is None
    else:
        _same(got, exp)


def _normals(rng, n, k, spread=0.3):
    base = rng.gamma(2.0, 60.0, n)
    tumor = np.round(rng.poisson(base) * 1.0 + rng.randint(0, 3, n) * 0.25, 2)
    normals = [np.round(rng.poisson(base * (1.0 + spread * s) + rng.gamma(1.0, 5.0 * (s + 1), n)) * 1.0, 2) for s in range(k)]
    return tumor, normals


def _run_blr2(cv, tumor, normals, on=None):
    got = cv.normalize_best_normal(to_dev(tumor, cv.device), [to_dev(c, cv.device) for c in normals], None if on is None else to_dev(on.astype(np.int32), cv.device))
    exp = R.best_lr2(tumor, normals, on)
    best, msl, ign, replayed = got
    assert best == exp[0]
    assert list(ign) == exp[2]
    np.testing.assert_allclose(msl, exp[1], rtol=1e-10, atol=0)
    return got, exp


@pytest.mark.parametrize("n,k,with_on", [(50_000, 2, False), (200_001, 8, False), (120_000, 5, True), (3_000, 3, True)])
def test_best_normal_separated(n, k, with_on):
    cv = get_canvas()
    rng = np.random.RandomState(n + k)
    tumor, normals = _normals(rng, n, k)
    for c in normals[1::2]:
        c[rng.rand(n) < 0.02] = 0.0                           # zero bins: ignored
    on = np.sort(rng.choice(n, n // 3, replace=False)) if with_on else None
    (best, msl, ign, replayed), _ = _run_blr2(cv, tumor, normals, on)
    assert replayed == 0


@pytest.mark.parametrize("with_on", [False, True])
def test_best_normal_identical_normals(with_on):
    cv = get_canvas()
    rng = np.random.RandomState(21)
    n = 80_000
    tumor, normals = _normals(rng, n, 4)
    on = np.sort(rng.choice(n, n // 2, replace=False)) if with_on else None
    exp_best = R.best_lr2(tumor, normals, on)[0]
    normals.insert(exp_best, normals[exp_best].copy())         # two identical copies of the best normal: the first one wins
    (best, msl, ign, replayed), exp = _run_blr2(cv, tumor, normals, on)
    assert replayed >= 2
    assert msl[exp[0]] == exp[1][exp[0]] and msl[exp[0] + 1] == exp[1][exp[0] + 1]     # replayed: the reference's values


def test_best_normal_tumour_median_zero():
    cv = get_canvas()
    rng = np.random.RandomState(22)
    n = 30_001
    tumor, normals = _normals(rng, n, 3)
    tumor[rng.rand(n) < 0.6] = 0.0                            # median 0: weight 0, every bin is ignored, every mean is 0 -> the first normal
    (best, msl, ign, replayed), _ = _run_blr2(cv, tumor, normals)
    assert best == 0 and replayed == 3 and list(msl) == [0.0, 0.0, 0.0] and list(ign) == [n] * 3
